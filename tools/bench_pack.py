#!/usr/bin/env python3
"""pack_k alone: the pack tables of the network's training plan (the launches of one step, in plan order), each timed by
itself -- HIP events around replays of a hipGraph of 20 launches -- with the bytes it moves and the time a float4 copy
would need for them (6.3 TB/s, docs/rounds/r06.md section 6).
usage: python tools/bench_pack.py [--model pmf|epmf] [--backbone resnet34] [--nclasses 20] [--height 64] [--width 2048]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PMF_AUTOTUNE", "0")      # the pack tables do not depend on the conv tile configurations
import torch  # noqa: E402

from pmf_amd import _lib as L  # noqa: E402

COPY_TBS = 6.3


def table_bytes(jobs):
    """(OIHW bytes read, packed bytes written) of a list of Plan.pack_jobs entries"""
    rd = wr = 0
    for (w, _buf, taps, _tr, _kp, _ldw, _lane, fmt, _own, cin) in jobs:
        co, ci, khw = w.shape[0], (cin[1] if cin is not None else w.shape[1]), w.shape[2] * w.shape[3]
        rd += 4 * co * ci * khw                     # the tile is staged whole, whatever the tap subset
        wr += (6 if fmt else 4) * co * ci * len(taps)
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pmf", choices=["pmf", "epmf"])
    ap.add_argument("--backbone", default="resnet34")
    ap.add_argument("--nclasses", type=int, default=20)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--bs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pack.py needs a GPU")
    from pmf_amd.models import PMFNet, EPMFNet
    from pmf_amd.models.pmf_net import _get_plan
    from pmf_amd.utils.detinit import deterministic_init
    dev = torch.device("cuda:0")
    net = PMFNet if a.model == "pmf" else EPMFNet
    model = deterministic_init(net(5, 3, a.nclasses, 32, imagenet_pretrained=False, image_backbone=a.backbone)).to(dev).train()
    plan = _get_plan(model, a.bs, a.height, a.width, True, dev)
    lib = L.lib()
    by_buf = {j[1].ptr: j for j in plan.pack_jobs}
    s = torch.cuda.Stream()
    rows, tot_us, tot_b = [], 0.0, 0
    for lane, tab, n, blocks, _bits, is_dgrad in plan.pack_tables:
        raw = bytes(tab.cpu().numpy())
        jobs = [by_buf[J.dst] for J in (L.PackJob * n).from_buffer_copy(raw)]
        rd, wr = table_bytes(jobs)

        def launch(tab=tab, n=n, blocks=blocks):
            L.check(lib.pmf_pack_weights_batched(tab.data_ptr(), n, blocks, C.c_void_p(s.cuda_stream)), "pack")
        with torch.cuda.stream(s):
            launch()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(a.reps):
                    launch()
            for _ in range(3):
                gr.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.replays):
                gr.replay()
            e1.record(s)
            torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (a.reps * a.replays)
        rows.append({"lane": lane, "input_gradient": bool(is_dgrad), "jobs": n, "workgroups": blocks, "read_MB": rd / 1e6,
                     "write_MB": wr / 1e6, "us": round(us, 2), "GBps": round((rd + wr) / us / 1e3, 1),
                     "floor_us": round((rd + wr) / (COPY_TBS * 1e6), 2)})
        tot_us += us
        tot_b += rd + wr
    for r in rows:
        print("lane %d %-4s %3d jobs %5d wg  read %7.2f MB  write %7.2f MB  %8.2f us  %7.1f GB/s  floor %7.2f us" % (
            r["lane"], "dgrad" if r["input_gradient"] else "fwd", r["jobs"], r["workgroups"], r["read_MB"], r["write_MB"],
            r["us"], r["GBps"], r["floor_us"]))
    print(json.dumps({"metric": "pack_k us per step, every table alone", "model": a.model, "backbone": a.backbone,
                      "us_per_step": round(tot_us, 2), "bytes": tot_b, "GBps": round(tot_b / tot_us / 1e3, 1),
                      "floor_us_at_6.3TBps": round(tot_b / (COPY_TBS * 1e6), 2), "tables": rows}))


if __name__ == "__main__":
    main()
