#!/usr/bin/env python3
"""SensatUrban dataset preparation (pmf_amd.dataset.compute_bev_feature, csrc/bev_prepare.hip) on one synthetic block; every
array is generated from --seed, no file is read.

    python tools/bench_bev_prepare.py --block small|large|columns [--arith float32] [--steps 3] [--warmup 1] [--no-save]

  small    2000 x 2000 cells, 3 000 000 points (the block of tools/bench_sensat_eval.py)
  large    4000 x 4000 cells, 40 000 000 points
  columns  the large block with 2000 points stacked in one cell every 50 cells along both axes (6400 columns)

Timed: the stages with device events on arrays that stay put (upload, extent, bin, scan, place, table, cells, download;
`extent` and `table` end in the host reading 32 bytes back), whole blocks numpy-in to numpy-out on the host clock ending in
the download, and torch.save of the dict; medians over --steps runs after --warmup.  Yardsticks on the same box: the
per-point loop restated in tests/bev_prepare_cases.py on a 200 000-point subset (points/s), and a vectorised numpy
composition on the whole block (stable sort by cell, segment reductions).  One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCKS = {"small": (2000, 3000000, 0), "large": (4000, 40000000, 0), "columns": (4000, 40000000, 50)}
GRID = 0.1
OFFSET = (431.7, 88.2)


def synthetic_block(seed, side, npts, column_every):
    g = np.random.Generator(np.random.PCG64(seed))
    x = side * GRID * g.random(npts)
    y = side * GRID * g.random(npts)
    if column_every:
        k = np.arange(0, side, column_every)
        cx, cy = np.meshgrid(k, k)
        n = cx.size * 2000
        x[:n] = np.repeat(cx.reshape(-1), 2000) * GRID + 0.02 + 0.06 * g.random(n)
        y[:n] = np.repeat(cy.reshape(-1), 2000) * GRID + 0.02 + 0.06 * g.random(n)
    x[0] = y[0] = 0.0
    perm = g.permutation(npts)
    c = {"x": (OFFSET[0] + x)[perm].astype(np.float32), "y": (OFFSET[1] + y)[perm].astype(np.float32),
         "z": (5.0 + 45.0 * g.random(npts)).astype(np.float32)}
    rgb = g.integers(0, 256, (3, npts)).astype(np.uint8)
    c.update(red=rgb[0], green=rgb[1], blue=rgb[2], label=g.integers(0, 13, npts).astype(np.uint8))
    return c


def numpy_composition(c, grid, arith):
    """the frame by whole-array numpy: stable sort by cell, then segment reductions"""
    from tests.bev_prepare_cases import pixel_index
    h_idx, w_idx = pixel_index(c["y"], grid, arith), pixel_index(c["x"], grid, arith)
    h, w = int(h_idx.max()) + 1, int(w_idx.max()) + 1
    cell = h_idx.astype(np.int64) * w + w_idx
    order = np.argsort(cell, kind="stable")
    cs = cell[order]
    n = cs.size
    starts = np.flatnonzero(np.concatenate([[True], cs[1:] != cs[:-1]]))
    count = np.diff(np.concatenate([starts, [n]]))
    z = c["z"][order].astype(np.float64)
    zmax = np.maximum.reduceat(z, starts)
    first = np.minimum.reduceat(np.where(z == np.repeat(zmax, count), np.arange(n), n), starts)
    win = order[first]
    occ = cs[starts]
    fm = np.zeros((8, h * w))
    fm[0, occ], fm[1, occ] = zmax, np.minimum.reduceat(z, starts)
    fm[2, occ] = np.add.reduceat(z, starts) / (count + 1e-6)
    fm[3, occ], fm[4, occ] = np.log10(count + 1.0), 1.0
    fm[5, occ], fm[6, occ], fm[7, occ] = c["red"][win], c["green"][win], c["blue"][win]
    lab = np.full(h * w, -1.0)
    lab[occ] = 0.0 if c["label"] is None else c["label"][win]
    return {"feature_map": fm.reshape(8, h, w), "label_map": lab.reshape(h, w), "h_idx": h_idx, "w_idx": w_idx}


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", choices=sorted(BLOCKS), default="small")
    ap.add_argument("--arith", choices=("float32", "float64"), default="float32")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--yardstick-steps", type=int, default=3, help="timed runs of the numpy composition")
    a = ap.parse_args()
    import torch
    from pmf_amd.dataset import compute_bev_feature
    from pmf_amd.dataset.sensat_urban.prepare import BevPrepare
    from tests.bev_prepare_cases import loop_np
    if not torch.cuda.is_available():
        raise SystemExit("bench_bev_prepare.py measures on the GPU: no device found")
    dev = torch.device("cuda")
    side, npts, col = BLOCKS[a.block]
    c = synthetic_block(a.seed, side, npts, col)
    if a.arith == "float64":
        c["label"] = None
    names = ("x", "y", "z", "red", "green", "blue")
    args = [c[k] for k in names]

    # whole blocks, numpy in -> numpy out
    block_ms = []
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = compute_bev_feature(*args, label=c["label"], grid_size=GRID, arith=a.arith)
        block_ms.append((time.perf_counter() - t0) * 1e3)
    block_ms = block_ms[a.warmup:]
    h, w = out["label_map"].shape

    # the stages
    stages = {k: [] for k in ("upload", "extent", "bin", "scan", "place", "table", "cells", "download")}
    max_count = 0
    for step in range(a.warmup + a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
        ev[0].record()
        up = [torch.from_numpy(v).to(dev) for v in args]
        lab = None if c["label"] is None else torch.from_numpy(c["label"]).to(dev)
        ev[1].record()
        bp = BevPrepare(*up, label=lab, grid_size=GRID, arith=a.arith)
        bp.extent()
        ev[2].record()
        bp.bin()
        ev[3].record()
        bp.scan()
        ev[4].record()
        bp.place()
        ev[5].record()
        bp.table()
        ev[6].record()
        bp.cells()
        ev[7].record()
        host = [bp.feature_map.cpu(), bp.label_map.cpu(), bp.h_idx.cpu(), bp.w_idx.cpu()]
        ev[8].record()
        ev[8].synchronize()
        max_count = bp.max_count
        if step >= a.warmup:
            for k, name in enumerate(stages):
                stages[name].append(ev[k].elapsed_time(ev[k + 1]))
        del bp, up, host
    stage_ms = {k: round(median(v), 3) for k, v in stages.items()}

    save_ms = None
    if not a.no_save:
        ts = []
        with tempfile.TemporaryDirectory() as tmp:
            for step in range(a.steps):
                t0 = time.perf_counter()
                torch.save(out, os.path.join(tmp, "block.pth"))
                ts.append((time.perf_counter() - t0) * 1e3)
        save_ms = median(ts)

    res = {"bench": "bev_prepare", "block": a.block, "arith": a.arith, "points": npts, "h": h, "w": w,
           "max_count": max_count, "steps": a.steps, "block_ms": median(block_ms),
           "block_ms_all": [round(t, 1) for t in block_ms], "stage_ms": stage_ms,
           "device_ms": round(sum(stage_ms[k] for k in ("extent", "bin", "scan", "place", "table", "cells")), 3),
           "torch_save_ms": save_ms, "map_bytes": int(9 * 8 * h * w), "points_per_s": npts / (median(block_ms) * 1e-3)}
    if not a.no_yardsticks:
        sub = {k: (None if v is None else v[:200000]) for k, v in c.items()}
        t0 = time.perf_counter()
        loop_np(sub, GRID, a.arith)
        res["loop_points_per_s"] = 200000 / (time.perf_counter() - t0)
        ts = []
        for step in range(a.yardstick_steps):
            t0 = time.perf_counter()
            ref = numpy_composition(c, GRID, a.arith)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["numpy_composition_ms"] = median(ts)
        res["numpy_composition_runs"] = a.yardstick_steps
        res["numpy_points_per_s"] = npts / (median(ts) * 1e-3)
        res["speedup_vs_numpy"] = median(ts) / median(block_ms)
        res["speedup_vs_loop"] = res["points_per_s"] / res["loop_points_per_s"]
        # the composition's segment sums are numpy's (not the loop's order): everything else must agree exactly
        same = {k: bool(np.array_equal(out[k], ref[k])) for k in ("label_map", "h_idx", "w_idx")}
        same["feature_map_but_mean"] = bool(np.array_equal(out["feature_map"][[0, 1, 3, 4, 5, 6, 7]],
                                                           ref["feature_map"][[0, 1, 3, 4, 5, 6, 7]]))
        same["mean_equal_fraction"] = float((out["feature_map"][2] == ref["feature_map"][2]).mean())
        res["equal_to_numpy_composition"] = same
    print(json.dumps(res))


if __name__ == "__main__":
    main()
