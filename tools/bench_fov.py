#!/usr/bin/env python3
"""SemanticKITTI-FOV creation (pmf_amd.dataset.semantic_kitti.fov, pmf_fov_filter in csrc/project.hip) on synthetic
KITTI-sized frames; every array is generated from --seed, no data set is read.

    python tools/bench_fov.py [--frames 16] [--points 120000] [--steps 20] [--warmup 3] [--tree-frames 64] [--no-tree]

Timed, medians over --steps runs after --warmup:
  device_ms      the three launches of pmf_fov_filter alone, device events around --inner calls, inputs and outputs resident:
                 B = 1 and B = --frames; bytes moved by the algorithm (rows and keep read and written, kept rows and label
                 words written) over that time is device_GBps
  call_ms        the whole fov_filter_gpu call on host arrays (upload, pass, copies back), host clock: it ends in a
                 device -> host copy
  numpy_ms       the reference's method on the host for the same frames (fov_cases.numpy_filter: float64 matmul, mask,
                 fancy indexing of rows and labels)
  tree           create_fov_dataset end to end on a synthetic tree of --tree-frames frames in a temporary directory (PNG
                 headers, reads, filter, writes, image copies), with the GPU filter and with the numpy filter, frames/s
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 376, 1241
# a KITTI-like calibration: P2 . Tr with the camera looking along the vehicle's x axis
P2 = np.array([[718.856, 0, 607.1928, 45.38225], [0, 718.856, 185.2157, -0.1130887], [0, 0, 1.0, 0.003779761]])
TR = np.array([[4.2768e-4, -9.99967e-1, -8.0845e-3, -1.1985e-2], [-7.2106e-3, 8.0812e-3, -9.99941e-1, -5.4040e-2],
               [9.99974e-1, 4.8595e-4, -7.2069e-3, -2.9220e-1], [0, 0, 0, 1.0]])
PROJ = P2 @ TR


def synthetic_frame(g, n):
    """a full sweep: points all around the vehicle, about a fifth of them inside the camera's view"""
    r = g.uniform(2.0, 70.0, n)
    a = g.uniform(-np.pi, np.pi, n)
    z = g.uniform(-2.5, 1.0, n)
    pts = np.stack([r * np.cos(a), r * np.sin(a), z, g.random(n)], 1).astype(np.float32)
    lab = (g.integers(0, 300, n).astype(np.uint32) << 16) | g.integers(0, 260, n).astype(np.uint32)
    return pts, lab


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def device_pass(frames, labels, steps, warmup, inner):
    """-> (median ms of one pmf_fov_filter call on resident arrays, kept rows, rows); a timed window is `inner` calls back to
    back between two device events, so that it is long against the clock's resolution"""
    import torch
    from pmf_amd import _lib as L
    B = len(frames)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    P = int(off[-1])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pts, lab = d(np.concatenate(frames)), d(np.concatenate(labels).view(np.int32))
    off_d, dim_d, mat = d(off), d(np.array([(H, W)] * B, np.int32)), d(PROJ.reshape(12))
    keep = torch.empty(P, dtype=torch.uint8, device="cuda")
    out_pts = torch.empty((P, 4), dtype=torch.float32, device="cuda")
    out_lab = torch.empty(P, dtype=torch.int32, device="cuda")
    out_off = torch.empty(B + 1, dtype=torch.int64, device="cuda")
    blk = torch.empty((P + L.FOV_BLOCK - 1) // L.FOV_BLOCK + 1, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for step in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            L.check(L.lib().pmf_fov_filter(pts.data_ptr(), lab.data_ptr(), off_d.data_ptr(), dim_d.data_ptr(), B, P,
                                           mat.data_ptr(), keep.data_ptr(), out_pts.data_ptr(), out_lab.data_ptr(),
                                           out_off.data_ptr(), blk.data_ptr(), st), "pmf_fov_filter")
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return median(ms[warmup:]), int(out_off[B].item()), P


def write_tree(root, g, frames, points):
    from PIL import Image
    sd = os.path.join(root, "00")
    for sub in ("velodyne", "labels", "image_2"):
        os.makedirs(os.path.join(sd, sub))
    with open(os.path.join(sd, "calib.txt"), "w") as f:
        f.write("P2: " + " ".join("%.12e" % v for v in P2.reshape(-1)) + "\n")
        f.write("Tr: " + " ".join("%.12e" % v for v in TR[:3].reshape(-1)) + "\n")
    img = Image.fromarray(g.integers(0, 256, (H, W, 3)).astype(np.uint8))
    for i in range(frames):
        pts, lab = synthetic_frame(g, points + 13 * i)
        pts.tofile(os.path.join(sd, "velodyne", "%06d.bin" % i))
        lab.tofile(os.path.join(sd, "labels", "%06d.label" % i))
        img.save(os.path.join(sd, "image_2", "%06d.png" % i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="pmf_fov_filter calls per timed window of device_ms")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tree-frames", type=int, default=64)
    ap.add_argument("--io-threads", type=int, default=4)
    ap.add_argument("--no-tree", action="store_true")
    a = ap.parse_args()
    import torch
    import fov_cases as F
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset, fov_filter_gpu
    if not torch.cuda.is_available():
        raise SystemExit("bench_fov.py measures on the GPU: no device found")
    g = np.random.Generator(np.random.PCG64(a.seed))
    data = [synthetic_frame(g, a.points + 13 * i) for i in range(a.frames)]
    frames, labels = [d[0] for d in data], [d[1] for d in data]
    dims = [(H, W)] * a.frames
    res = {"bench": "fov", "frames": a.frames, "points_per_frame": a.points, "h": H, "w": W, "steps": a.steps,
           "warmup": a.warmup, "inner": a.inner, "device": torch.cuda.get_device_name(0)}

    for tag, n in (("B1", 1), ("B%d" % a.frames, a.frames)):
        ms, kept, P = device_pass(frames[:n], labels[:n], a.steps, a.warmup, a.inner)
        # count: rows in, keep out; compact: keep in, kept rows and their label words in and out
        moved = P * (16 + 1) + P * 1 + kept * (16 + 16 + 4 + 4)
        res["device_ms_" + tag] = round(ms, 4)
        res["device_GBps_" + tag] = round(moved / (ms * 1e-3) / 1e9, 1)
        res["kept_share_" + tag] = round(kept / P, 4)

    call, ref = [], []
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fov_filter_gpu(frames, dims, PROJ, labels)
        call.append((time.perf_counter() - t0) * 1e3)
    for step in range(1 + max(3, a.steps // 4)):
        t0 = time.perf_counter()
        want = F.numpy_filter(frames, dims, PROJ, labels)
        ref.append((time.perf_counter() - t0) * 1e3)
    res["call_ms"] = round(median(call[a.warmup:]), 3)
    res["call_ms_per_frame"] = round(median(call[a.warmup:]) / a.frames, 3)
    res["numpy_ms"] = round(median(ref[1:]), 3)
    res["numpy_ms_per_frame"] = round(median(ref[1:]) / a.frames, 3)
    res["numpy_over_call"] = round(median(ref[1:]) / median(call[a.warmup:]), 2)
    res["equal_to_numpy"] = bool(all(x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
                                     for x, y in zip(got, want)))

    if not a.no_tree:
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "src")
            write_tree(src, g, a.tree_frames, a.points)
            runs = {"gpu": [], "numpy": []}
            for rep in range(3):                    # alternating; the first pair warms the page cache and is dropped
                for tag, fn in (("gpu", fov_filter_gpu), ("numpy", F.numpy_filter)):
                    t0 = time.perf_counter()
                    st = create_fov_dataset(src, os.path.join(tmp, "dst_" + tag), [0], batch_frames=a.frames,
                                            io_threads=a.io_threads, overwrite=True, filter_fn=fn)
                    runs[tag].append(time.perf_counter() - t0)
            res["tree_frames"] = a.tree_frames
            res["tree_kept_share"] = round(st["00"]["points_kept"] / st["00"]["points_read"], 4)
            for tag in runs:
                res["tree_%s_frames_per_s" % tag] = round(a.tree_frames / median(runs[tag][1:]), 1)
                res["tree_%s_s_all" % tag] = [round(t, 3) for t in runs[tag]]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
