#!/usr/bin/env python
"""Regenerate tests/golden/g20_bev_prepare.npz: what the REFERENCE's own _compute_feature
(tasks/sensat_urban/dataset_prepare/compute_bev_feature.py) returns for the clouds of tests/bev_prepare_cases.py.

    python tools/make_golden_bev_prepare.py REFERENCE_ROOT

The reference module imports `sensat_tools` (its PLY reader, not needed for _compute_feature) at load, so an empty module
of that name stands in for it.  The point array is stacked exactly as the reference's run() stacks it, so numpy's promotion
decides the arithmetic: float32 with a uint8 class column, float64 with the float64 zero column of the test split.  The
conditions each cloud exists for are asserted here; the outputs are stored as they are (float64 losslessly, compressed)."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bev_prepare_cases as B  # noqa: E402


def reference_module(reference_root):
    sys.modules.setdefault("sensat_tools", types.ModuleType("sensat_tools"))
    path = os.path.join(reference_root, "tasks", "sensat_urban", "dataset_prepare", "compute_bev_feature.py")
    spec = importlib.util.spec_from_file_location("ref_compute_bev_feature", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_run(mod, c, arith):
    """the stacking of the reference's run(), then its _compute_feature"""
    assert (c["label"] is None) == (arith == "float64")
    label = np.zeros(c["x"].shape) if c["label"] is None else c["label"]
    pointcloud = np.vstack((c["x"], c["y"], c["z"], c["red"], c["green"], c["blue"], label)).T
    assert pointcloud.dtype == np.dtype(arith), pointcloud.dtype
    pre = object.__new__(mod.SenSatPreProcess)
    pre.grid_size = B.GRID
    return pre._compute_feature(pointcloud)


def check_conditions(out):
    """the property each cloud is there for (counts printed, thresholds asserted)"""
    rs = np.random.RandomState(0)
    # ties: cells whose maximum is shared by points of different class
    c, o = B.cloud("ties"), out["ties"]
    cell = o["h_idx"].astype(np.int64) * o["feature_map"].shape[2] + o["w_idx"]
    at_max = c["z"].astype(np.float64) == o["feature_map"][0].reshape(-1)[cell]
    n = sum(1 for k in np.unique(cell[at_max]) if np.unique(c["label"][at_max & (cell == k)]).size > 1)
    print("ties: %d cells share their maximum among classes (of %d occupied)" % (n, np.unique(cell).size))
    assert n >= 10
    # dense
    o = out["dense"]
    count = np.rint(10 ** o["feature_map"][3] - 1)
    empty = float((o["feature_map"][4] == 0).mean())
    print("dense: max count %d, %.0f %% of the cells empty" % (count.max(), 100 * empty))
    assert count.max() >= 3000 and empty >= 0.2
    # order: cells whose mean changes when the in-cell order is scrambled
    c, o = B.cloud("order"), out["order"]
    scr = B.loop_np(c, order=rs.permutation(c["z"].size))
    n = int((scr["feature_map"][2] != o["feature_map"][2]).sum())
    assert np.array_equal(scr["feature_map"][[1, 3, 4]], o["feature_map"][[1, 3, 4]])
    print("order: %d of %d cells change their mean under a scrambled order" % (n, o["feature_map"][2].size))
    assert n >= 50
    # lattice: points whose pixel differs between the arithmetics
    a, b = out["lattice_f32"], out["lattice_f64"]
    n = int(((a["h_idx"] != b["h_idx"]) | (a["w_idx"] != b["w_idx"])).sum())
    print("lattice: %d of %d points fall into a different pixel in float32 and float64" % (n, a["h_idx"].size))
    assert n >= 500
    # and a reciprocal multiply in place of the float32 division would show
    c = B.cloud("lattice")
    rec = ((c["x"] - c["x"].min()) * (np.float32(1) / np.float32(B.GRID))).astype(np.int32)
    o = out["thresholds"]
    count = np.bincount(o["h_idx"].astype(np.int64) * o["feature_map"].shape[2] + o["w_idx"], minlength=len(B.THRESHOLD_COUNTS))
    print("thresholds: counts", count.tolist())
    assert o["feature_map"].shape == (8, 1, len(B.THRESHOLD_COUNTS)) and tuple(count) == B.THRESHOLD_COUNTS
    print("lattice: %d points move under a reciprocal multiply" % int((rec != a["w_idx"]).sum()))


def main(reference_root):
    mod = reference_module(reference_root)
    out, rec = {}, {}
    for key, name, arith in B.RUNS:
        out[key] = reference_run(mod, *B.case(key))
        for k in B.KEYS:
            rec["%s.%s" % (key, k)] = out[key][k]
        print(key, out[key]["feature_map"].shape, out[key]["feature_map"].dtype, out[key]["h_idx"].dtype)
    check_conditions(out)
    np.savez_compressed(B.GOLDEN, **rec)
    print("%s: %d bytes" % (B.GOLDEN, os.path.getsize(B.GOLDEN)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
