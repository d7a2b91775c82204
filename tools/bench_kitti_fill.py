#!/usr/bin/env python3
"""Full SemanticKITTI sweeps from FOV predictions (pmf_amd.postproc.fov_fill, pmf_kitti_full_fill in csrc/project.hip) on
synthetic KITTI-sized frames (tools/bench_fov.py's); every array is generated from --seed, no data set is read.

    python tools/bench_kitti_fill.py [--frames 16] [--points 120000] [--steps 20] [--warmup 3]

Timed, medians over --steps runs after --warmup:
  device_ms      the three launches of pmf_kitti_full_fill alone (labels, keep mask, kept rows per frame, confusion and source
                 counts), device events around --inner calls, inputs and outputs resident: B = 1 and B = --frames; the bytes
                 the algorithm moves (rows read, keep written, sub / gt words read, main words read, labels written) over
                 that time is device_GBps; device_ms_unscored: the same without gt and conf (a test split)
  call_ms        the whole fov_fill call on host arrays with gt, conf and counts (packed upload, pass, one copy back), host
                 clock: it ends in a device -> host copy
  numpy_ms       the numpy composition of the same rule on that host (kitti_full_cases.numpy_fill: float64 matmul, mask,
                 cumulative rank, three table look-ups, np.add.at confusion)
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NCLS = 20


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def device_pass(frames, dims, proj, main, sub, gt, lut, fill_id, steps, warmup, inner, score=True):
    """-> (median ms of one pmf_kitti_full_fill call on resident arrays, kept rows, rows); score=False: gt and conf NULL"""
    import torch
    from pmf_amd import _lib as L
    from pmf_amd.postproc.fov_fill import workspace_words
    B = len(frames)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in main])]).astype(np.int64)
    P, Kt = int(off[-1]), int(moff[-1])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pts, off_d, moff_d = d(np.concatenate(frames)), d(off), d(moff)
    dim_d, mat, lut_d = d(np.asarray(dims, np.int32)), d(np.asarray(proj, np.float64).reshape(12)), d(lut.astype(np.int32))
    main_d, sub_d, gt_d = (d(np.concatenate(x).view(np.int32)) for x in (main, sub, gt))
    out = torch.empty(P, dtype=torch.int32, device="cuda")
    keep = torch.empty(P, dtype=torch.uint8, device="cuda")
    kept = torch.empty(B, dtype=torch.int64, device="cuda")
    conf = torch.zeros((NCLS, NCLS), dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    ws = torch.empty(workspace_words(P), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for step in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            L.check(L.lib().pmf_kitti_full_fill(
                pts.data_ptr(), off_d.data_ptr(), dim_d.data_ptr(), B, P, mat.data_ptr(), main_d.data_ptr(), moff_d.data_ptr(),
                Kt, sub_d.data_ptr(), gt_d.data_ptr() if score else None, lut_d.data_ptr(), int(lut_d.shape[0]), int(fill_id),
                NCLS, out.data_ptr(), keep.data_ptr(), kept.data_ptr(), counts.data_ptr(), conf.data_ptr() if score else None,
                ws.data_ptr(), st),
                "pmf_kitti_full_fill")
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return median(ms[warmup:]), int(kept.sum().item()), P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="pmf_kitti_full_fill calls per timed window of device_ms")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    import fov_cases as F
    import kitti_full_cases as K
    from bench_fov import H, W, PROJ, synthetic_frame
    from pmf_amd.dataset.semantic_kitti import DEFAULT_CONFIG
    from pmf_amd.postproc import fov_fill
    if not torch.cuda.is_available():
        raise SystemExit("bench_kitti_fill.py measures on the GPU: no device found")
    import yaml
    from pmf_amd.dataset.semantic_kitti.parser import label_tables
    with open(DEFAULT_CONFIG) as f:
        tables = label_tables(yaml.safe_load(f))
    lut = np.zeros(max(tables["learning_map"]) + 100, np.int32)
    for k, v in tables["learning_map"].items():
        lut[k] = v
    ids = np.array(sorted(set(tables["learning_map_inv"].values())), np.uint32)       # what a prediction holds; 0 = unlabelled
    fill_id = int(tables["learning_map_inv"][9])
    g = np.random.Generator(np.random.PCG64(a.seed))
    data = [synthetic_frame(g, a.points + 13 * i) for i in range(a.frames)]
    frames = [d[0] for d in data]
    gt = [(d[1] & 0xFFFF0000) | g.choice(np.array(sorted(tables["learning_map"]), np.uint32), len(d[1])) for d in data]
    dims = [(H, W)] * a.frames
    main = [g.choice(ids, int(F.numpy_keep(f, PROJ, H, W).sum())).astype(np.uint32) for f in frames]
    sub = [g.choice(ids, len(f)).astype(np.uint32) for f in frames]
    res = {"bench": "kitti_fill", "frames": a.frames, "points_per_frame": a.points, "h": H, "w": W, "steps": a.steps,
           "warmup": a.warmup, "inner": a.inner, "device": torch.cuda.get_device_name(0)}
    for tag, n in (("B1", 1), ("B%d" % a.frames, a.frames)):
        ms, kept, P = device_pass(frames[:n], dims[:n], PROJ, main[:n], sub[:n], gt[:n], lut, fill_id, a.steps, a.warmup, a.inner)
        moved = P * (16 + 1) + P * (4 + 4 + 4) + kept * 4
        res["device_ms_" + tag] = round(ms, 4)
        res["device_GBps_" + tag] = round(moved / (ms * 1e-3) / 1e9, 1)
        res["kept_share_" + tag] = round(kept / P, 4)
        res["device_ms_unscored_" + tag] = round(device_pass(frames[:n], dims[:n], PROJ, main[:n], sub[:n], gt[:n], lut, fill_id,
                                                             a.steps, a.warmup, a.inner, score=False)[0], 4)
    conf = torch.zeros((NCLS, NCLS), dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    call, ref = [], []
    for step in range(a.warmup + a.steps):
        conf.zero_()
        counts.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fov_fill(frames, dims, PROJ, main, sub, lut, fill_id, NCLS, gt=gt, conf=conf, counts=counts)
        call.append((time.perf_counter() - t0) * 1e3)
    for step in range(1 + max(3, a.steps // 4)):
        t0 = time.perf_counter()
        want = K.numpy_fill(frames, dims, PROJ, main, sub, lut, fill_id, NCLS, gt)
        ref.append((time.perf_counter() - t0) * 1e3)
    res["call_ms"] = round(median(call[a.warmup:]), 3)
    res["call_ms_per_frame"] = round(median(call[a.warmup:]) / a.frames, 3)
    res["numpy_ms"] = round(median(ref[1:]), 3)
    res["numpy_ms_per_frame"] = round(median(ref[1:]) / a.frames, 3)
    res["numpy_over_call"] = round(median(ref[1:]) / median(call[a.warmup:]), 2)
    res["source_counts"] = [int(v) for v in counts.cpu().tolist()]
    res["equal_to_numpy"] = bool(all(np.array_equal(x, y) for x, y in zip(got, want["out"]))
                                 and np.array_equal(conf.cpu().numpy(), want["conf"])
                                 and np.array_equal(counts.cpu().numpy(), want["counts"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
