#!/usr/bin/env python3
"""The device work of the nuScenes full-sweep fusion on sweeps of nuScenes size (34 720 points, 17 classes), generated
from --seed: pmf_eval_fill per sweep at B = 1 and B = --batch sweeps per launch (tasks/pmf_eval_nuscenes/testset_eval), and
SweepEvaluator's finish with and without a fallback prediction (pmf_eval_sweep_finish / pmf_eval_sweep_finish_fill,
tasks/epmf_eval_nuscenes).

Each HIP path is timed next to the same steps composed of torch ops on the device plus the host-side IOUEval.addBatch the
reference's loops use (the labels are copied to the host, the confusion matrix lives there), in the same run, alternating.
Per step both paths see the same inputs, taken in turn from a pool of --pool distinct buffer sets (no call re-reads what the
call before it left in the caches), and their labels, confusion matrices and counts are compared.  Reported per sweep: the
median of per-call device-event times (kernel + copy to the host where the task copies), the median host wall clock between
synchronisations, and for the fill alone the time per sweep of --inner launches issued back to back (what the launch costs
when nothing waits for it).  The finish variants get their state refilled, untimed, before every call.

    python tools/bench_nus_fill.py [--batch 8] [--steps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, P_SWEEP, FILL = 17, 34720, 11


def median(v):
    return round(float(np.median(np.asarray(v, np.float64))), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--pool", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    import pc_processor
    from pmf_amd.postproc import fill_labels
    from pmf_amd.postproc.frame_eval import sweep_finish, sweep_finish_fill
    assert torch.cuda.is_available(), "bench_nus_fill.py measures on the GPU only"
    dev = torch.device("cuda")
    g = np.random.Generator(np.random.PCG64(a.seed))
    lut_np = g.integers(0, C, 256).astype(np.int32)
    lut = torch.from_numpy(lut_np).to(dev)

    def sweeps(n):
        P = n * P_SWEEP
        main_ = g.integers(1, C, P).astype(np.int32)
        main_[g.random(P) < 0.55] = 0                       # the share of a sweep no camera sees
        sub = g.integers(1, C, P).astype(np.int32)
        sub[g.random(P) < 0.02] = 0
        sem = g.integers(0, 32, P).astype(np.int32)
        return main_, sub, sem

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    result = {"what": "nus_fill", "points": P_SWEEP, "classes": C, "steps": a.steps, "pool": a.pool}

    # ---- the batched fill ------------------------------------------------------------------------------------------------
    for B in sorted({1, a.batch}):
        pool = []
        for _ in range(a.pool):
            m, s, raw = sweeps(B)
            pool.append(dict(main=torch.from_numpy(m).to(dev), sub=torch.from_numpy(s).to(dev),
                             sem=torch.from_numpy(raw).to(dev), gt=lut_np[raw].astype(np.int64)))
        conf = torch.zeros(C, C, dtype=torch.int64, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        out = torch.empty(B * P_SWEEP, dtype=torch.uint8, device=dev)
        ref = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])
        ref_counts = np.zeros(3, np.int64)

        def hip(x):
            fill_labels(x["main"], x["sub"], C, FILL, x["sem"], lut, conf, counts, out)
            return out.cpu().numpy()

        def composed(x):
            nz = x["main"] != 0
            pred = torch.where(nz, x["main"], x["sub"])
            zero = pred == 0
            pred = torch.where(zero, torch.full_like(pred, FILL), pred)
            n_main, n_fill = nz.sum(), zero.sum()
            host = pred.cpu().numpy()
            ref.addBatch(host, x["gt"])
            nm, nf = int(n_main.item()), int(n_fill.item())
            ref_counts[:] += (nm, host.shape[0] - nm - nf, nf)
            return host.astype(np.uint8)

        t = {k: [] for k in ("hip", "hip_wall", "composed", "composed_wall")}
        same = True
        for step in range(a.warmup + a.steps):
            x = pool[step % a.pool]
            got, d, w = timed(lambda: hip(x))
            want, rd, rw = timed(lambda: composed(x))
            same = same and np.array_equal(got, want)
            if step >= a.warmup:
                for k, v in (("hip", d), ("hip_wall", w), ("composed", rd), ("composed_wall", rw)):
                    t[k].append(v / B)
        same = same and torch.equal(conf.cpu(), ref.conf_matrix) and np.array_equal(counts.cpu().numpy(), ref_counts)
        assert same, "fill: labels, confusion or counts differ from the torch composition"

        def burst():                                        # launches back to back, nothing waits in between
            for i in range(a.inner):
                x = pool[i % a.pool]
                fill_labels(x["main"], x["sub"], C, FILL, x["sem"], lut, conf, counts, out)
        timed(burst)
        bursts = [timed(burst)[1] / (a.inner * B) for _ in range(max(a.steps // 10, 5))]
        result["fill_B%d" % B] = dict({k + "_ms_per_sweep": median(v) for k, v in t.items()},
                                      kernel_back_to_back_ms_per_sweep=median(bursts), identical=bool(same))

    # ---- the sweep finish, plain and fused -----------------------------------------------------------------------------------
    pool = []
    for _ in range(a.pool):
        m, s, raw = sweeps(1)
        cf = (g.random(P_SWEEP) * (m != 0)).astype(np.float32)
        pool.append(dict(lab=torch.from_numpy(m).to(dev), cf=torch.from_numpy(cf).to(dev), sub=torch.from_numpy(s).to(dev),
                         sem=torch.from_numpy(raw).to(dev), gt=lut_np[raw].astype(np.int64)))
    conf_full = torch.zeros(P_SWEEP, dtype=torch.float32, device=dev)
    label_full = torch.zeros(P_SWEEP, dtype=torch.int32, device=dev)
    out = torch.empty(P_SWEEP, dtype=torch.uint8, device=dev)
    cam = {k: torch.zeros(C, C, dtype=torch.int64, device=dev) for k in ("plain", "fused")}
    fused = torch.zeros(C, C, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    ref_cam = {k: pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0]) for k in ("plain", "fused")}
    ref_fused = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])

    def refill(x):
        conf_full.copy_(x["cf"])
        label_full.copy_(x["lab"])

    def hip_plain(x):
        sweep_finish(conf_full, label_full, C, x["sem"], lut, cam["plain"], out)
        return out.cpu().numpy()

    def hip_fused(x):
        sweep_finish_fill(conf_full, label_full, x["sub"], C, FILL, x["sem"], lut, cam["fused"], fused, counts, None, out)
        return out.cpu().numpy()

    def composed_plain(x, key="plain"):
        host = label_full.cpu().numpy()
        ref_cam[key].addBatch(host, x["gt"] * (host != 0))
        conf_full.zero_()
        label_full.zero_()
        return host.astype(np.uint8)

    def composed_fused(x):
        nz = label_full != 0
        pred = torch.where(nz, label_full, x["sub"])
        pred = torch.where(pred == 0, torch.full_like(pred, FILL), pred)
        host = pred.cpu().numpy()
        composed_plain(x, "fused")
        ref_fused.addBatch(host, x["gt"])
        return host.astype(np.uint8)

    variants = (("finish", hip_plain), ("finish_fallback", hip_fused), ("finish_composed", composed_plain),
                ("finish_fallback_composed", composed_fused))
    t = {k: [] for name, _ in variants for k in (name, name + "_wall")}
    same = True
    for step in range(a.warmup + a.steps):
        x = pool[step % a.pool]
        got = {}
        for name, fn in variants:
            refill(x)
            got[name], d, w = timed(lambda: fn(x))
            same = same and not label_full.any().item() and not conf_full.any().item()
            if step >= a.warmup:
                t[name].append(d)
                t[name + "_wall"].append(w)
        same = same and np.array_equal(got["finish"], got["finish_composed"]) and \
            np.array_equal(got["finish_fallback"], got["finish_fallback_composed"])
    same = same and torch.equal(cam["plain"].cpu(), ref_cam["plain"].conf_matrix) and \
        torch.equal(cam["fused"].cpu(), ref_cam["fused"].conf_matrix) and torch.equal(fused.cpu(), ref_fused.conf_matrix) and \
        torch.equal(cam["plain"], cam["fused"])
    assert same, "finish: labels, confusion or state differ from the torch composition"
    result["finish"] = dict({k + "_ms_per_sweep": median(v) for k, v in t.items()}, identical=bool(same))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
