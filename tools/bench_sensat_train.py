#!/usr/bin/env python3
"""SensatUrban training iteration, timed in parts on synthetic batches with the reference's server configuration
(tasks/sensat_urban/pmf/config_server.yaml: batch 4, 320 x 320, 14 classes, base_channels 48, resnet101, its eight
feature means and stds).

    python tools/bench_sensat_train.py [--part all|objective|optim|step|step_torch_optim|loader_step] [--rounds R] [--calls K]

  objective          the fused objective with the Dice term (sensat_total_loss_fused) against (i) the PMF objective without it
                     (pmf_total_loss_fused, whose kernels this extension leaves as they were) and (ii) sensat_total_loss in
                     torch ops on the device; forward + backward, [4, 14, 320, 320]
  optim              pmf_adamw_amsgrad_range over the flat LiDAR-stream buffer against torch's fused
                     AdamW(amsgrad=True).step() on a tensor of the same size, with the bytes each moves
  step               SensatEngine.train_step with the range optimiser
  step_torch_optim   the same with PMF_OWN_OPTIM=0 (torch's fused step() at the end of the iteration)
  loader_step        SensatLoader.batch() (two synthetic 3000 x 4000 frames resident on the device, the draws, the count and
                     the gather of csrc/bev_train.hip) feeding SensatEngine.train_step, against the step alone on the batch
                     it returned; host clock around iterations that end in a device synchronise

``--part all`` (default) runs the five parts one after the other, each as a child process under its own time limit, and
stops at the first one that fails.  Every figure is a median over rounds of device-event timings; the variants of a part
alternate within a round and every round works on freshly allocated inputs.  One JSON line per figure."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, H, W = 4, 14, 320, 320
BASE, BACKBONE = 48, "resnet101"
MEAN = [27.47, 26.90, 27.22, 0.63, 0.81, 0, 0, 0]
STD = [18.43, 18.00, 18.21, 0.40, 0.39, 255.0, 255.0, 255.0]
FILL = 0.5                                    # labelled fraction of the synthetic label maps
LIMITS = {"objective": 300, "optim": 240, "step": 420, "step_torch_optim": 420, "loader_step": 420}      # seconds per child


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def _time_calls(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3          # microseconds per call


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def part_objective(rounds, calls):
    import torch
    from pmf_amd.engine import sensat_focal_alpha
    from pmf_amd.loss import (ExpLogDiceLoss, FocalSoftmaxLoss, Lovasz_softmax, pmf_total_loss_fused, sensat_total_loss,
                              sensat_total_loss_fused)
    from pmf_amd.utils.detinit import det_tensor, synthetic_batch
    dev = "cuda"
    _, _, label, _ = synthetic_batch(N, H, W, C, seed=1, fill=FILL)
    a0 = torch.softmax(det_tensor("bs.a", (N, C, H, W), -3, 3), 1)
    b0 = torch.softmax(det_tensor("bs.b", (N, C, H, W), -3, 3), 1)
    alpha = torch.from_numpy(sensat_focal_alpha(C))
    focal = FocalSoftmaxLoss(C, gamma=2, alpha=sensat_focal_alpha(C), softmax=False).to(dev)
    lov, dice = Lovasz_softmax(ignore=0), ExpLogDiceLoss()
    variants = {
        "fused_with_dice": lambda a, b, lab: sensat_total_loss_fused(a, b, lab, alpha)[0],
        "fused_without_dice": lambda a, b, lab: pmf_total_loss_fused(a, b, lab, alpha)[0],
        "torch_ops_with_dice": lambda a, b, lab: sensat_total_loss(a, b, lab, focal, lov, dice)[0],
    }
    times = {k: [] for k in variants}
    values = {}
    for r in range(rounds + 1):                 # round 0 warms every variant up and is dropped
        for name, fn in variants.items():
            a, b = a0.to(dev).requires_grad_(True), b0.to(dev).requires_grad_(True)       # fresh addresses
            lab = label.to(dev)

            def call():
                a.grad = b.grad = None
                t = fn(a, b, lab)
                t.backward()
                return t
            for _ in range(3):
                t = call()
            us = _time_calls(torch, call, calls if name != "torch_ops_with_dice" else max(2, calls // 5))
            values[name] = t.item()
            if r:
                times[name].append(us)
    med = {k: _median(v) for k, v in times.items()}
    maps_mb = 2 * N * C * H * W * 4 / 1e6
    _emit(part="objective", shape=[N, C, H, W], labelled_fraction=float((label > 0).float().mean()), rounds=rounds,
          us_per_call=med, spread_us={k: [min(v), max(v)] for k, v in times.items()}, loss=values,
          ratio_to_objective_without_dice=med["fused_with_dice"] / med["fused_without_dice"],
          extra_us_for_dice=med["fused_with_dice"] - med["fused_without_dice"],
          speedup_over_torch_ops=med["torch_ops_with_dice"] / med["fused_with_dice"],
          one_read_of_both_probability_maps_mb=maps_mb)


def part_optim(rounds, calls):
    import ctypes as CT
    import torch
    from pmf_amd import _lib as L
    from pmf_amd.models import PMFNet
    n = sum(p.numel() for p in PMFNet(5, 3, C, BASE, imagenet_pretrained=False,
                                      image_backbone=BACKBONE).lidar_stream.parameters())
    dev = "cuda"
    lib = L.lib()
    st = CT.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = {"range_amsgrad": [], "torch_fused_amsgrad": [], "range_adamw": []}
    for r in range(rounds + 1):
        g = torch.Generator(device=dev).manual_seed(r)
        p = torch.randn(n, device=dev, generator=g)
        grad = torch.randn(n, device=dev, generator=g)
        m, v, x = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        step = torch.ones((), device=dev)
        q = torch.nn.Parameter(p.clone())
        q.grad = grad.clone()
        opt = torch.optim.AdamW([q], lr=1e-3, amsgrad=True, fused=True)

        def own():
            L.check(lib.pmf_adamw_amsgrad_range(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), n,
                                                1e-3, 0.9, 0.999, 1e-8, 0.01, step.data_ptr(), st))

        def plain():
            L.check(lib.pmf_adamw_range(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999,
                                        1e-8, 0.01, step.data_ptr(), st))
        for name, fn in (("range_amsgrad", own), ("torch_fused_amsgrad", opt.step), ("range_adamw", plain)):
            for _ in range(3):
                fn()
            us = _time_calls(torch, fn, calls)
            if r:
                times[name].append(us)
    med = {k: _median(v) for k, v in times.items()}
    _emit(part="optim", parameters=n, rounds=rounds, us_per_call=med, spread_us={k: [min(v), max(v)] for k, v in times.items()},
          bytes_per_parameter={"range_amsgrad": 36, "range_adamw": 28},
          gb_per_s={"range_amsgrad": 36 * n / med["range_amsgrad"] / 1e3, "range_adamw": 28 * n / med["range_adamw"] / 1e3,
                    "torch_fused_amsgrad_at_36_bytes": 36 * n / med["torch_fused_amsgrad"] / 1e3})


def part_step(rounds, calls, own):
    os.environ["PMF_OWN_OPTIM"] = "1" if own else "0"
    import torch
    from pmf_amd.engine import SensatEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    dev = "cuda"
    torch.manual_seed(0)
    model = deterministic_init(PMFNet(5, 3, C, BASE, imagenet_pretrained=False, image_backbone=BACKBONE)).to(dev)
    eng = SensatEngine(model, C, lr=1e-3, warmup_steps=10, max_steps=10 ** 6, feature_mean=MEAN, feature_std=STD)
    assert (eng._ro is not None) == own
    g = torch.Generator().manual_seed(1)
    mean, std = torch.tensor(MEAN).view(1, 8, 1, 1), torch.tensor(STD).view(1, 8, 1, 1)
    feat = mean + std * torch.randn(N, 8, H, W, generator=g)
    feat[:, 4] = (torch.rand(N, H, W, generator=g) < FILL).float()
    raw = torch.randint(0, C - 1, (N, H, W), generator=g)
    feat, raw = feat.to(dev), raw.to(dev)
    times, total = [], None
    for r in range(rounds + 1):
        def call():
            return eng.train_step(feat.clone(), raw)[0]
        for _ in range(3 if r else 8):
            total = call()
        us = _time_calls(torch, call, calls)
        if r:
            times.append(us)
    assert torch.isfinite(total).item(), "the objective diverged"
    _emit(part="step" if own else "step_torch_optim", shape=[N, 8, H, W], base_channels=BASE, backbone=BACKBONE,
          range_optimiser=own, rounds=rounds, ms_per_step=_median(times) / 1e3,
          spread_ms=[min(times) / 1e3, max(times) / 1e3], last_total=total.item())


def part_loader_step(rounds, calls):
    os.environ["PMF_OWN_OPTIM"] = "1"
    import random
    import time
    import numpy as np
    import torch
    from pmf_amd.dataset import SensatLoader
    from pmf_amd.engine import SensatEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    dev = "cuda"
    fh, fw = 3000, 4000

    class Frames(object):
        split = "train"

        def __init__(self, n):
            g = torch.Generator().manual_seed(2)
            mean, std = torch.tensor(MEAN).view(8, 1, 1).double(), torch.tensor(STD).view(8, 1, 1).double()
            self.frames = []
            for _ in range(n):
                fm = mean + std * torch.randn(8, fh, fw, generator=g, dtype=torch.float64)
                fm[4] = (torch.rand(fh, fw, generator=g) < FILL).double()
                lm = torch.randint(-1, C - 1, (fh, fw), generator=g)
                self.frames.append({"feature_map": fm.numpy(), "label_map": lm.numpy().astype(np.int64)})

        def readDataByIndex(self, i):
            return self.frames[i]

        def __len__(self):
            return len(self.frames)
    torch.manual_seed(0)
    random.seed(0)
    ld = SensatLoader(Frames(2), img_h=H, img_w=W, n_samples_split=200, device=dev)
    model = deterministic_init(PMFNet(5, 3, C, BASE, imagenet_pretrained=False, image_backbone=BACKBONE)).to(dev)
    eng = SensatEngine(model, C, lr=1e-3, warmup_steps=10, max_steps=10 ** 6, feature_mean=MEAN, feature_std=STD)
    order = torch.randperm(len(ld)).tolist()
    pos = [0]

    def indices():
        idx = [order[(pos[0] + k) % len(order)] for k in range(N)]
        pos[0] += N
        return idx

    def host_timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    feat, raw = ld.batch(indices())
    variants = {"loader_and_step": lambda: eng.train_step(*ld.batch(indices())),
                "step_alone": lambda: eng.train_step(feat.clone(), raw),
                "loader_alone": lambda: ld.batch(indices())}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):
        for name, fn in variants.items():
            for _ in range(3 if r else 8):
                fn()
            ms = host_timed(fn, calls)
            if r:
                times[name].append(ms)
    total = eng.train_step(*ld.batch(indices()))[0]
    assert torch.isfinite(total).item(), "the objective diverged"
    med = {k: _median(v) for k, v in times.items()}
    _emit(part="loader_step", shape=[N, 8, H, W], frame=[fh, fw], resident_mb=ld.resident_bytes() / 1e6, base_channels=BASE,
          backbone=BACKBONE, rounds=rounds, ms_per_iteration=med, spread_ms={k: [min(v), max(v)] for k, v in times.items()},
          loader_share_of_iteration=(med["loader_and_step"] - med["step_alone"]) / med["loader_and_step"],
          last_total=total.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all"] + list(LIMITS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if a.part == "all":
        for part, limit in LIMITS.items():       # one child per part: its own time limit, and nothing follows a failure
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(a.rounds),
                                     "--calls", str(a.calls)], cwd=ROOT, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                sys.exit("bench_sensat_train: part %r failed (%d); stopping" % (part, rc))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sensat_train: needs a GPU (there is no CPU path to time)")
    if a.part == "objective":
        part_objective(a.rounds, a.calls)
    elif a.part == "optim":
        part_optim(a.rounds, a.calls)
    elif a.part == "loader_step":
        part_loader_step(a.rounds, a.calls)
    else:
        part_step(a.rounds, a.calls, own=a.part == "step")


if __name__ == "__main__":
    main()
