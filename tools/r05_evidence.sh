#!/bin/bash
# round-5 evidence batch (GPU box, `gpurun -- "bash tools/r05_evidence.sh <commit>"`): full -m gpu suite, smoke, rocprofv3 summaries (tools/collect_profiles.sh), bench lines of every configuration -> profiles/r05_*
o=gpurun_out/r05z; mkdir -p $o
(timeout 1500 python -m pytest tests -m gpu -q > $o/pytest_gpu.log 2>&1; echo "pytest rc $?" >> $o/pytest_gpu.log); grep -E "^(FAILED|ERROR)|passed|failed|pytest rc" $o/pytest_gpu.log | tail -6
python __graft_entry__.py smoke 2>&1 | tail -2
bash tools/collect_profiles.sh r05 $1 > $o/collect.log 2>&1; head -1 gpurun_out/r05/r05_per_layer_kernel_times.txt
L=$o/r05_bench_lines.jsonl; : > $L
python bench.py --full --steps 20 --warmup 5 >> $L 2>/dev/null
python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --height 480 --width 640 --steps 30 --warmup 5 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --mode infer --steps 30 --warmup 5 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --mode infer --height 480 --width 640 --steps 30 --warmup 5 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --backbone resnet50 --nclasses 17 --height 32 --width 1024 --steps 50 --warmup 10 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --model epmf --steps 50 --warmup 10 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --model salsanext --steps 50 --warmup 10 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --height 256 --width 1024 --steps 30 --warmup 5 --no-cpu-baseline >> $L 2>/dev/null
python bench.py --full --force-dist --steps 50 --warmup 10 --no-cpu-baseline --no-roofline --no-f32-ref >> $L 2>/dev/null
python bench.py --mode loader >> $L 2>/dev/null
python -c "
import json
for l in open('$L'):
    l=l.strip()
    if not l.startswith('{'): print('NON-JSON:', l[:80]); continue
    d=json.loads(l); print(round(d['value'],2), d['unit'], round(d.get('ms_per_step') or 0,3), (d.get('roofline') or {}).get('frac'), (d.get('parity') or {}).get('ok'), d['config']['workload'][:70])"
