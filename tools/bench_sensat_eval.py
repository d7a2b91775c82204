#!/usr/bin/env python3
"""Per-frame PMF evaluation on SensatUrban (tasks/sensat_urban/pmf_eval) on one synthetic block: --size x --size pixels,
three points per four pixels, tile sizes 320 / 448 / 576, 14 classes; everything is generated from --seed.

HIP path: BevTileEvaluator.frame (one upload, pmf_bev_tile_pre, PMFNet forward of 4 tiles -- with --tta of one tile's six
variants plus the padded one --, pmf_bev_tile_accum, then argmax, gather or KNN and pmf_bev_points).  Its stages are also
timed on their own with device events, each as one loop over all tile groups of the frame on fixed buffers: pre, forward,
accum, finish.  The yardstick is the reference's loop body composed on the SAME device and model: per tile a host crop in
float64, upload, torch normalise, 1 or 7 batch-1 forwards with torch permutations, .cpu() accumulation on the host, then
argmax / gather (or this project's KNN module) / zero -> 1 on the host.  Both are timed by a host clock around whole frames
that end in a device synchronise (the yardstick is host-bound), medians over --steps frames after --warmup frames (every
plan shape is built and warm before the timed window); every frame starts from the host arrays.  The two paths' labels and
confidence maps are compared: they differ only by the rounding between a batch-6 (or batch-4) and a batch-1 forward.

    python tools/bench_sensat_eval.py [--tta] [--knn] [--size 2000] [--backbone resnet34] [--base-channels 32]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C = 14
SIZES = [320, 448, 576]
MEAN = [27.47, 26.90, 27.22, 0.63, 0.81, 0, 0, 0]
STD = [18.43, 18.00, 18.21, 0.40, 0.39, 255.0, 255.0, 255.0]
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}


def synthetic_block(seed, size):
    g = np.random.Generator(np.random.PCG64(seed))
    h = w = size
    npts = 3 * h * w // 4
    pix = g.integers(0, h * w, npts)
    z = (5.0 + 45.0 * g.random(npts)).astype(np.float32)
    fm = np.zeros((8, h * w), np.float64)
    fm[0, pix] = z
    fm[1, pix] = z
    fm[2, pix] = z
    fm[3, pix] = 0.5
    fm[4, pix] = 1.0
    fm[5:8, pix] = g.integers(0, 256, (3, npts))
    label_map = np.full(h * w, -1, np.int64)
    labels = g.integers(0, 13, npts).astype(np.uint8)
    label_map[pix] = labels
    frame = {"feature_map": fm.reshape(8, h, w), "label_map": label_map.reshape(h, w),
             "h_idx": (pix // w).astype(np.int64), "w_idx": (pix % w).astype(np.int64)}
    return frame, labels, z


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def reference_frame(torch, model, frame, z, tta, knn, mean, std):
    """the reference's loop body (infer.py:89-208) on this device and model -> (pred uint8 before - 1, confidence map)"""
    fm = frame["feature_map"]
    h, w = fm.shape[1:]
    conf = torch.zeros((C, h, w)).float()
    pad = torch.nn.ZeroPad2d(16)
    for S in SIZES:
        for r in range(math.ceil(h / S)):
            hs, he = r * S, (r + 1) * S
            if he > h:
                he, hs = h, max(h - S, 0)
            for c in range(math.ceil(w / S)):
                ws, we = c * S, (c + 1) * S
                if we > w:
                    we, ws = w, max(w - S, 0)
                crop = np.zeros((8, S, S))
                crop[:, :he - hs, :we - ws] = fm[:, hs:he, ws:we]
                x = torch.from_numpy(crop).float().cuda().unsqueeze(0)
                x = (x - mean) / std * x[:, 4].unsqueeze(1)
                pcd, rgb = x[:, 0:5], x[:, 5:8]
                out = model(pcd, rgb)[0]
                if tta:
                    out = out + model(pcd.rot90(1, (2, 3)), rgb.rot90(1, (2, 3)))[0].rot90(3, (2, 3))
                    out = out + model(pcd.rot90(2, (2, 3)), rgb.rot90(2, (2, 3)))[0].rot90(2, (2, 3))
                    out = out + model(pcd.flip(3), rgb.flip(3))[0].flip(3)
                    out = out + model(pcd.flip(2), rgb.flip(2))[0].flip(2)
                    out = out + model(pcd.permute(0, 1, 3, 2), rgb.permute(0, 1, 3, 2))[0].permute(0, 1, 3, 2)
                    out = out + model(pad(pcd), pad(rgb))[0][:, :, 16:16 + S, 16:16 + S]
                conf[:, hs:he, ws:we] += out[0].cpu()[:, :he - hs, :we - ws]
    argmax = conf.unsqueeze(0).argmax(dim=1)[0]
    h_idx, w_idx = torch.from_numpy(frame["h_idx"]), torch.from_numpy(frame["w_idx"])
    if knn is not None:
        pred = knn(torch.from_numpy(fm[0]).float().cuda(), torch.from_numpy(z).float().cuda(), argmax.cuda(),
                   w_idx.cuda(), h_idx.cuda()).cpu()
    else:
        pred = argmax[h_idx, w_idx]
    pred[pred.eq(0)] = 1
    return pred.numpy().astype(np.uint8), conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tta", action="store_true")
    ap.add_argument("--knn", action="store_true")
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--backbone", type=str, default="resnet34")
    ap.add_argument("--base-channels", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    import pc_processor
    from pmf_amd.postproc import BevTileEvaluator, KNN, bev_points, bev_tile_accum, bev_tile_pre, tile_windows
    from pmf_amd.postproc.frame_eval import window_argmax
    from pmf_amd.utils.detinit import deterministic_init
    if not torch.cuda.is_available():
        raise SystemExit("bench_sensat_eval.py measures on the GPU: no device found")
    dev = torch.device("cuda")
    frame, labels, z = synthetic_block(a.seed, a.size)
    h, w = frame["feature_map"].shape[1:]
    model = deterministic_init(pc_processor.models.PMFNet(5, 3, C, a.base_channels, False, a.backbone)).to(dev).eval()
    ev = BevTileEvaluator(model, C, MEAN, STD, SIZES, tta=a.tta, knn_params=KNN_PARAMS if a.knn else None)
    knn_mod = KNN(KNN_PARAMS, C) if a.knn else None
    mean = torch.Tensor(MEAN).view(1, 8, 1, 1).to(dev)
    std = torch.Tensor(STD).view(1, 8, 1, 1).to(dev)
    n_tiles = sum(len(tile_windows(h, w, S)) for S in SIZES)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    hip_ms, ref_ms = [], []
    with torch.no_grad():
        for step in range(a.warmup + a.steps):              # alternating, same call: both see the same machine
            (pred, conf_map, n_zero), t_hip = timed(lambda: ev.frame(frame, z=z if a.knn else None))
            (ref_pred, ref_conf), t_ref = timed(lambda: reference_frame(torch, model, frame, z, a.tta, knn_mod, mean, std))
            if step >= a.warmup:
                hip_ms.append(t_hip)
                ref_ms.append(t_ref)
        agree = float((pred.cpu().numpy() == (ref_pred - 1).astype(np.uint8)).mean())
        conf_err = float(((conf_map.cpu() - ref_conf).abs() / ref_conf.abs().clamp_min(1.0)).max())

        # the stages on their own: device events around one loop over all tile groups of the frame
        fm = torch.from_numpy(frame["feature_map"]).float().to(dev)
        T, V = ev.tile_batch, 6 if a.tta else 1
        groups = []
        for S in SIZES:
            wins = tile_windows(h, w, S)
            for g in range(0, len(wins), T):
                real = wins[g:g + T]
                groups.append((S, [(x[0], x[2]) for x in real + [real[-1]] * (T - len(real))], len(real)))
        probs = {S: (torch.rand(T * V, C, S, S, device=dev), torch.rand(T, C, S + 32, S + 32, device=dev) if a.tta else None)
                 for S in SIZES}
        cmap = torch.zeros(C, h, w, device=dev)
        h_idx, w_idx = torch.from_numpy(frame["h_idx"]).to(dev), torch.from_numpy(frame["w_idx"]).to(dev)
        zt = torch.from_numpy(z).to(dev)

        def stage_pre():
            for S, org, _ in groups:
                bev_tile_pre(fm, ev.mean, ev.stds, org, S, V, a.tta, ev._workspace(S))

        def stage_forward():
            for S, _, _ in groups:
                ws = ev._workspace(S)
                model(ws[0], ws[1])
                if a.tta:
                    model(ws[2], ws[3])

        def stage_accum():
            for S, org, n in groups:
                bev_tile_accum(probs[S][0], org[:n], S, V, cmap, probs[S][1])

        def stage_finish():
            amap = window_argmax(conf_map, 0, 0, h, w)
            voted = knn_mod(fm[0], zt, amap, w_idx, h_idx) if a.knn else None
            bev_points(amap, h_idx, w_idx, C, voted)

        stages = {}
        for name, fn in (("pre", stage_pre), ("forward", stage_forward), ("accum", stage_accum), ("finish", stage_finish)):
            ts = []
            for step in range(a.warmup + a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if step >= a.warmup:
                    ts.append(e0.elapsed_time(e1))
            stages[name] = median(ts)
    print(json.dumps({
        "bench": "sensat_eval", "size": a.size, "tta": a.tta, "knn": a.knn, "backbone": a.backbone,
        "base_channels": a.base_channels, "tiles": n_tiles, "points": int(labels.size), "steps": a.steps,
        "hip_frame_ms": median(hip_ms), "torch_host_frame_ms": median(ref_ms),
        "speedup": median(ref_ms) / median(hip_ms), "hip_frame_ms_all": [round(t, 1) for t in hip_ms],
        "torch_host_frame_ms_all": [round(t, 1) for t in ref_ms],
        "stage_ms": {k: round(v, 3) for k, v in stages.items()}, "labels_equal_fraction": agree,
        "conf_map_max_rel_diff": conf_err, "zero_points": n_zero}))


if __name__ == "__main__":
    main()
