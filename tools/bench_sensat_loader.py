#!/usr/bin/env python3
"""SensatLoader, timed: the two kernels of csrc/bev_train.hip, a whole ``batch()``, and the same batch as torch ops on the
device and as the reference's chain on the CPU.

    python tools/bench_sensat_loader.py [--size 800] [--batch 2] [--frame 3000x4000] [--rounds 7] [--calls 20]

Two synthetic float64 frames of the given size (SensatUrban blocks are a few thousand pixels a side) are made from a seed
and handed to SensatLoader, which keeps them on the device.  One fixed set of accepted candidates (seeded draws) is used by
every variant.  Per batch of B items of size x size:
  count_us / gather_us     the kernels alone on structs already uploaded: medians over rounds of device-event timings, the
                           variants alternating within a round
  gather_gb_per_s          (bytes written: B * 9 * H * W * 4) + (bytes gathered: B * H * W * 33), over gather_us
  batch_us                 SensatLoader.batch(): draws, struct uploads, count, the copy of the counts back, gather -- host
                           clock around a call that ends in a device synchronise
  torch_device_us          the chain per item in torch ops on the device, from a resident f32[9,h,w] frame: crop,
                           grid_sample(nearest) rotation, crop, flips, share, jitters; stacked
  cpu_chain_us             tests/sensat_loader_cases.py (the reference's chain restated), including the reference's per-item
                           float64 -> float32 conversion of the whole frame; few repetitions, it takes seconds
One JSON line.  Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


class _Frames(object):
    split = "train"

    def __init__(self, n, h, w, seed=0):
        import numpy as np
        import torch
        g = torch.Generator().manual_seed(seed)
        self.frames = []
        for _ in range(n):
            fm = torch.rand(8, h, w, generator=g, dtype=torch.float64) * 60.0
            fm[4] = (torch.rand(h, w, generator=g) > 0.2).double()
            lm = torch.randint(-1, 13, (h // 16 + 1, w // 16 + 1), generator=g).repeat_interleave(16, 0).repeat_interleave(16, 1)
            self.frames.append({"feature_map": fm.numpy(), "label_map": lm[:h, :w].contiguous().numpy().astype(np.int64)})

    def readDataByIndex(self, i):
        return self.frames[i]

    def __len__(self):
        return len(self.frames)


def _rotate_nearest_device(img, angle):
    """oracle/tensor_aug_ref.rotate_nearest on the device of `img` (same ops; the grid is built there)"""
    import torch
    import torch.nn.functional as F
    from oracle.tensor_aug_ref import inverse_rotation_matrix
    c, h, w = img.shape
    dev = img.device
    theta = torch.tensor(inverse_rotation_matrix(angle), dtype=img.dtype, device=dev).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=img.dtype, device=dev)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w, device=dev))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h, device=dev).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=img.dtype, device=dev)
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)
    return F.grid_sample(img[None], grid, mode="nearest", padding_mode="zeros", align_corners=False)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--frame", default="3000x4000")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sensat_loader: needs a GPU (there is no CPU path to time)")
    from pmf_amd import _lib as L
    from pmf_amd.dataset import SensatLoader
    from tests import sensat_loader_cases as S
    dev = "cuda"
    h, w = (int(v) for v in a.frame.split("x"))
    H = W = a.size
    B = a.batch
    ds = _Frames(2, h, w)
    ld = SensatLoader(ds, img_h=H, img_w=W, n_samples_split=200, device=dev)
    torch.manual_seed(1)
    random.seed(1)
    frame_of = [b % 2 for b in range(B)]
    cands = [ld.draw(h, w) for _ in range(B)]
    jits = [ld.draw_jitter() for _ in range(B)]
    structs = [ld.pack(f, c, j) for f, c, j in zip(frame_of, cands, jits)]
    lib, st = L.lib(), ld._stream()

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    # the device torch chain works on planes, as the reference does
    planes = [torch.cat((torch.from_numpy(f["feature_map"]).float(), torch.from_numpy(f["label_map"]).float()[None])).to(dev)
              for f in ds.frames]

    def torch_chain():
        fs, ls = [], []
        for f, (top1, left1, angle, top2, left2, hf, vf), (jr, jh) in zip(frame_of, cands, jits):
            x = planes[f][:, top1:top1 + 2 * H, left1:left1 + 2 * W]
            x = _rotate_nearest_device(x, angle)[:, top2:top2 + H, left2:left2 + W]
            if hf:
                x = x.flip(-1)
            if vf:
                x = x.flip(-2)
            x = x.clone()
            share = x[8].ge(0).sum().float() / x[8].numel()         # (stays on the device: no host decision here)
            x[5:8] = (x[5:8] + jr) * x[4:5]
            x[0:3] = (x[0:3] + jh) * x[4:5]
            fs.append(x[:8])
            ls.append(x[8])
        return torch.stack(fs), torch.stack(ls), share

    times = {"count": [], "gather": [], "torch_device": [], "batch": []}
    for r in range(a.rounds + 1):                   # round 0 warms every variant up and is dropped
        sdev = ld._upload(structs)                  # fresh addresses every round
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        feat = torch.empty((B, 8, H, W), device=dev)
        lab = torch.empty((B, H, W), device=dev)

        def count():
            L.check(lib.pmf_bev_sample_count(sdev.data_ptr(), B, H, W, counts.data_ptr(), st))

        def gather():
            L.check(lib.pmf_bev_sample_gather(sdev.data_ptr(), B, H, W, feat.data_ptr(), lab.data_ptr(), st))

        def batch():
            ld.batch(list(range(B)))
        for name, fn, calls in (("count", count, a.calls), ("gather", gather, a.calls),
                                ("torch_device", torch_chain, max(2, a.calls // 4))):
            for _ in range(3):
                fn()
            us = timed(fn, calls)
            if r:
                times[name].append(us)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            batch()
        torch.cuda.synchronize()
        if r:
            times["batch"].append((time.perf_counter() - t0) / a.calls * 1e6)
    # same bits as the torch chain on the device, except on rounding edges (tests/test_gpu_sensat_loader.py has the rule)
    tf, tl, _ = torch_chain()
    differ = int(((tf != feat).any(1) | (tl != lab)).sum())
    valid = [int(c) for c in counts.cpu()]

    cpu = []
    for _ in range(a.cpu_reps):
        t0 = time.perf_counter()
        for f, c, j in zip(frame_of, cands, jits):
            amap = S.all_map(ds.frames[f])
            S.ref_share(amap, c, H, W)
            S.ref_item(amap, c, j, H, W)
        cpu.append((time.perf_counter() - t0) * 1e6)

    med = {k: _median(v) for k, v in times.items()}
    moved = B * 9 * H * W * 4 + B * H * W * 33
    print(json.dumps({
        "tool": "bench_sensat_loader", "frame": [h, w], "size": [H, W], "batch": B, "rounds": a.rounds, "calls": a.calls,
        "resident_bytes_per_frame": 33 * h * w, "count_us": med["count"], "gather_us": med["gather"],
        "gather_bytes": moved, "gather_gb_per_s": moved / med["gather"] / 1e3, "batch_us": med["batch"],
        "torch_device_us": med["torch_device"], "cpu_chain_us": _median(cpu),
        "spread_us": {k: [min(v), max(v)] for k, v in times.items()}, "cpu_chain_spread_us": [min(cpu), max(cpu)],
        "pixels_differing_from_torch_device": differ, "valid_counts": valid,
        "angles": [round(c[2], 3) for c in cands]}), flush=True)


if __name__ == "__main__":
    main()
