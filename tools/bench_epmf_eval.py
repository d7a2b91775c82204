#!/usr/bin/env python3
"""Per-frame EPMF evaluation pipeline (tasks/epmf_eval_semantickitti) on synthetic KITTI-sized frames, timed with device
events after every padded shape is warmed up.

Frames: ~120 k points of a 64-beam sweep restricted to the camera's field of view (what the reference's FOV dataset
stores), a 376 x 1241 RGB image and public KITTI-style calibration, all generated from --seed.  Stages per frame:
loader (PerspectiveViewLoaderV2._eval_item: upload + projection, one host read of the box), pre (pmf_eval_pre), forward
(EPMFNet eval; --synthetic-prob replaces it by a fixed softmax map), post (pmf_eval_argmax + pmf_eval_points with both
confusion matrices and the uint32 ids).  The same pre + post composed of torch ops as the reference runs them (ZeroPad2d +
normalise, torch.argmax on the cropped slice, gather or pmf_knn_vote, IOUEval.addBatch bincounts on the device) is timed
on the same frames and probability maps; labels and confusion matrices of both are compared.

    python tools/bench_epmf_eval.py [--frames 3] [--steps 12] [--knn] [--synthetic-prob]
    python tools/bench_epmf_eval.py --bytes-from <rocprofv3 kernel_stats.csv> [--knn]   # bytes / kernel time per pass
"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMG_H, IMG_W, C = 376, 1241, 20
MEAN = [12.12, 10.88, 0.23, -1.04, 0.21]
STDS = [12.32, 11.47, 6.91, 0.86, 0.16]
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
# calibration of the public KITTI odometry benchmark's sequence 08 layout (P2 of the left colour camera, Tr velodyne -> camera)
P2 = np.array([[718.856, 0.0, 607.1928, 45.38225], [0.0, 718.856, 185.2157, -0.1130887], [0.0, 0.0, 1.0, 0.003779761]])
TR = np.array([[-1.857739385241e-03, -9.999659513510e-01, -8.039975204516e-03, -4.784029760483e-03],
               [-6.481465826011e-03, 8.051860151134e-03, -9.999466081774e-01, -7.337429464231e-02],
               [9.999773098287e-01, -1.805528627661e-03, -6.496203536139e-03, -3.339968064433e-01],
               [0.0, 0.0, 0.0, 1.0]])


def synthetic_frame(seed, n_target=120000):
    """a 64-beam sweep (elevation -24.8..2 deg, ground at -1.73 m) kept where it projects into the image"""
    g = np.random.Generator(np.random.PCG64(seed))
    M = P2 @ TR
    pts = []
    n = 0
    while n < n_target:
        m = 200000
        az = g.uniform(-0.75, 0.75, m)
        el = np.deg2rad(g.uniform(-24.8, 2.0, m))
        r = g.uniform(4.0, 70.0, m)
        r = np.where(el < 0, np.minimum(r, 1.73 / np.maximum(np.sin(-el), 1e-3)), r)
        x, y, z = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
        p = np.stack([x, y, z, g.random(m)], 1).astype(np.float32)
        hom = np.concatenate([p[:, :3].astype(np.float64), np.ones((m, 1))], 1) @ M.T
        u, v = hom[:, 0] / hom[:, 2], hom[:, 1] / hom[:, 2]
        ok = (hom[:, 2] > 0) & (u >= 0) & (u < IMG_W) & (v >= 0) & (v < IMG_H)
        pts.append(p[ok])
        n += int(ok.sum())
    pts = np.concatenate(pts)[:n_target]
    sem = g.choice([0, 10, 11, 13, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 70, 71, 72, 80, 81], pts.shape[0])
    img = g.integers(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)
    return pts, sem.astype(np.int32), img


class Frames(object):
    """the loader's dataset duck type over in-memory frames"""

    def __init__(self, frames):
        self.frames = frames
        self.proj_matrix = {"08": P2 @ TR}
        learning = {k: i for i, k in enumerate([0, 10, 11, 13, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 70, 71, 72,
                                                80])}
        learning[81] = 19
        self.class_map_lut = np.zeros(360, np.int32)
        for k, v in learning.items():
            self.class_map_lut[k] = v
        self.class_map_lut_inv = np.zeros(C + 100, np.int32)
        for k, v in sorted(learning.items(), reverse=True):
            self.class_map_lut_inv[v] = k

    def __len__(self):
        return len(self.frames)

    def loadImage(self, i):
        return self.frames[i][2]

    def loadDataByIndex(self, i):
        return self.frames[i][0], self.frames[i][1], None

    def parsePathInfoByIndex(self, i):
        return "08", "%06d" % i


def pass_bytes(h, w, H, W, K, knn):
    """algorithmic bytes of each HIP pass for one frame (every input read once, every output written once)"""
    pre = 9 * h * w * 4 + 8 * H * W * 4 + h * w * 4
    argmax = C * h * w * 4 + h * w * 4 + (h * w * 4 if knn else 0)
    points = K * (4 + 4 + 4 + 4 + 4) + (K * 8 if knn else K * C * 4)     # xd, yd, src, sem, inv out; vote or C gathers
    vote = (12 * h * w + 28 * K + 16 * K) if knn else 0                  # knn.hip's 12 HW + 28 P (+ px / py written)
    return {"eval_pre_k": pre, "eval_argmax_k": argmax, "eval_points_k": points, "knn_vote": vote}


def bytes_report(stats_csv, geo, knn):
    rows = list(csv.DictReader(open(stats_csv)))
    b = pass_bytes(*geo, knn)
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0)
        for k in ("eval_pre_k", "eval_argmax_k", "eval_points_k"):
            if name.startswith(k) or ("_Z" in name and k in name):
                out[k] = {"avg_us": avg_ns / 1e3, "calls": int(r.get("Calls", 0)), "bytes": b[k],
                          "GB_s": b[k] / avg_ns if avg_ns else None}
        if "knn_batch" in name and knn:
            out["knn_vote"] = {"avg_us": avg_ns / 1e3, "calls": int(r.get("Calls", 0)), "bytes": b["knn_vote"],
                               "GB_s": b["knn_vote"] / avg_ns if avg_ns else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12, help="timed frames (cycling over --frames)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--knn", action="store_true", help="KNN post-processing instead of the gather")
    ap.add_argument("--synthetic-prob", action="store_true", help="a fixed softmax map instead of the network")
    ap.add_argument("--bytes-from", type=str, default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--geometry", type=str, default=None, help="h,w,H,W,K for --bytes-from (default: frame 0's)")
    ap.add_argument("--geometry-out", type=str, default=None, help="write frame 0's h,w,H,W,K to DIR/geometry.json")
    args = ap.parse_args()
    if args.bytes_from:
        if args.geometry:
            geo = tuple(int(x) for x in args.geometry.split(","))
        else:
            geo = json.load(open(os.path.join(os.path.dirname(args.bytes_from), "geometry.json")))["geometry"]
        print(json.dumps({"bytes_over_kernel_time": bytes_report(args.bytes_from, geo, args.knn), "geometry": geo,
                          "knn": args.knn}))
        return
    import torch
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    from pmf_amd.metrics import IOUEval
    from pmf_amd.models import EPMFNet
    from pmf_amd.postproc import KNN, FrameEvaluator
    from pmf_amd.utils.detinit import deterministic_init
    dev = torch.device("cuda")
    t0 = time.time()
    ds = Frames([synthetic_frame(args.seed * 1000 + i, args.points) for i in range(args.frames)])
    gen_s = time.time() - t0
    loader = PerspectiveViewLoaderV2(ds, {"PVconfig": {"proj_h": 320, "proj_w": 1280}}, is_train=False, return_uproj=True)
    fe = FrameEvaluator(C, MEAN, STDS, KNN_PARAMS if args.knn else None)
    knn = KNN(KNN_PARAMS, C)
    model = None
    if not args.synthetic_prob:
        model = deterministic_init(EPMFNet(5, 3, C, 32, False, "resnet34")).to(dev).eval()
    lut_inv = torch.as_tensor(ds.class_map_lut_inv).to(dev)
    fm = torch.tensor(MEAN, device=dev).view(1, -1, 1, 1)
    fs = torch.tensor(STDS, device=dev).view(1, -1, 1, 1)
    ev_h, px_h = IOUEval(C, dev, [0]), IOUEval(C, dev, [0])
    ev_t, px_t = IOUEval(C, dev, [0]), IOUEval(C, dev, [0])
    probs = {}

    def forward(pcd, rgb, H, W):
        if model is not None:
            return model(pcd, rgb)[0]
        if (H, W) not in probs:
            g = torch.Generator(device=dev).manual_seed(H * 7 + W)
            probs[(H, W)] = torch.softmax(torch.randn((1, C, H, W), device=dev, generator=g), 1)
        return probs[(H, W)]

    def torch_pre(proj):
        x = proj[None, :8].clone()
        pd = x[0, 0].clone()
        pd = pd - pd.eq(0).float()
        h_pad = math.ceil(x.size(2) / 64.0) * 64 - x.size(2)
        w_pad = math.ceil(x.size(3) / 64.0) * 64 - x.size(3)
        pad = torch.nn.ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, h_pad // 2, h_pad - h_pad // 2))
        x = pad(x)
        m = pad(proj[None, 8])
        x[:, 0:5] = (x[:, 0:5] - fm) / fs * m.unsqueeze(1).expand_as(x[:, 0:5])
        return x[:, 0:5], x[:, 5:8], pd, h_pad // 2, w_pad // 2

    def torch_post(pred, proj, pd, top, left, xy, depth, extra):
        h, w = proj.shape[1:]
        out = pred[:, :, top:top + h, left:left + w]
        am = out[0].argmax(dim=0)
        px_t.addBatch(out.argmax(dim=1), proj[9:10].long())
        ux, uy = xy[:, 0].long(), xy[:, 1].long()
        ux, uy = ux - ux.min(), uy - uy.min()
        lab = knn(pd, depth, am, uy, ux) if args.knn else am[ux, uy]
        ev_t.addBatch(lab, extra["lut"][extra["sem"][extra["src"].long()].long()])
        return lut_inv[lab]

    ev = lambda: torch.cuda.Event(enable_timing=True)
    shapes, warm = {}, {}
    for i in range(len(ds)):                 # warm-up of every padded shape (plan build + live tuning of new shapes)
        proj, xy, depth, keep, extra = loader._eval_item(i)
        pcd, rgb = fe.pre(proj)
        H, W = fe.geometry[:2]
        torch.cuda.synchronize()
        t = time.time()
        pred = forward(pcd, rgb, H, W)
        fe.post(pred, depth, extra, px_h.conf_matrix, ev_h.conf_matrix, lut_inv)
        torch_post(pred, proj, *torch_pre(proj)[2:], xy, depth, extra)
        torch.cuda.synchronize()
        if (H, W) not in shapes:
            shapes[(H, W)] = (proj.shape[1], proj.shape[2], int(xy.shape[0]))
            warm["%dx%d" % (H, W)] = round(time.time() - t, 3)
    for e in (ev_h, px_h, ev_t, px_t):
        e.reset()
    T = {k: [] for k in ("loader", "pre", "forward", "post", "torch_pre", "torch_post", "frame")}
    same = True
    for s in range(args.steps):
        i = s % len(ds)
        e = [ev() for _ in range(9)]
        e[0].record()
        proj, xy, depth, keep, extra = loader._eval_item(i)
        e[1].record()
        pcd, rgb = fe.pre(proj)
        e[2].record()
        pred = forward(pcd, rgb, *fe.geometry[:2])
        e[3].record()
        _, inv = fe.post(pred, depth, extra, px_h.conf_matrix, ev_h.conf_matrix, lut_inv)
        e[4].record()
        _, _, pd, top, left = torch_pre(proj)
        e[5].record()
        inv_t = torch_post(pred, proj, pd, top, left, xy, depth, extra)
        e[6].record()
        torch.cuda.synchronize()
        same = same and torch.equal(inv.view(-1), inv_t.view(-1).to(inv.dtype)) and torch.equal(pd, fe.proj_depth)
        for k, (a, b) in (("loader", (0, 1)), ("pre", (1, 2)), ("forward", (2, 3)), ("post", (3, 4)),
                          ("torch_pre", (4, 5)), ("torch_post", (5, 6)), ("frame", (0, 4))):
            T[k].append(e[a].elapsed_time(e[b]))
    same = same and torch.equal(ev_h.conf_matrix, ev_t.conf_matrix) and torch.equal(px_h.conf_matrix, px_t.conf_matrix)
    ms = {k: round(float(np.median(v)), 4) for k, v in T.items()}
    h, w, K = shapes[next(iter(shapes))]
    H, W = next(iter(shapes))
    res = {"tool": "bench_epmf_eval", "knn": args.knn, "network": model is not None, "frames": args.frames,
           "steps": args.steps, "points_per_frame": args.points, "image": [IMG_H, IMG_W],
           "padded_shapes": {"%dx%d" % k: list(v) for k, v in shapes.items()}, "first_frame_s": warm,
           "median_ms": ms, "frames_per_s": round(1e3 / ms["frame"], 2) if ms["frame"] > 0 else None,
           "hip_pre_post_ms": round(ms["pre"] + ms["post"], 4),
           "torch_pre_post_ms": round(ms["torch_pre"] + ms["torch_post"], 4),
           "outputs_identical": bool(same), "synthesis_s": round(gen_s, 1)}
    if args.geometry_out:
        os.makedirs(args.geometry_out, exist_ok=True)
        with open(os.path.join(args.geometry_out, "geometry.json"), "w") as f:
            json.dump({"geometry": [h, w, H, W, K]}, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
