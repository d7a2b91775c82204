"""Shared pieces of the SensatUrban dataset-preparation tests (TEST INFRASTRUCTURE, not a conftest): the point clouds by seeded
recipe and a numpy restatement of the reference's per-point loop
(tasks/sensat_urban/dataset_prepare/compute_bev_feature.py, _compute_feature).

What is pinned to a reference RUN: tests/golden/g20_bev_prepare.npz holds what the reference's own _compute_feature returned
for every cloud below (tools/make_golden_bev_prepare.py REFERENCE_ROOT regenerates it and asserts the conditions listed with
each case).  The restatement here is written from reading that function; tests/test_bev_prepare_host.py holds it against
the fixture bit for bit, and the benchmark uses it as the per-point yardstick."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_bev_prepare.npz")
GRID = 0.1
OFFSET = (431.7, 88.2)
SPAN = (3.1, 4.7)                     # metres along x (w) and y (h): a 47 x 31 map
# points per cell of the `thresholds` cloud: either side of every count at which the cell pass changes path (one lane up to
# 32, a workgroup sorting in LDS up to 4096 and in the index list beyond; z replayed 1024 values at a time), and an empty cell
THRESHOLD_COUNTS = (32, 33, 1024, 0, 1025, 4096, 4097, 1)
KEYS = ("feature_map", "label_map", "h_idx", "w_idx")
# (fixture key, cloud, arith): what the GPU tests run; `lattice` in both arithmetics
RUNS = (("ties", "ties", "float32"), ("dense", "dense", "float32"), ("order", "order", "float32"),
        ("test_f64", "test_f64", "float64"), ("lattice_f32", "lattice", "float32"), ("lattice_f64", "lattice", "float64"),
        ("far", "far", "float32"), ("one", "one", "float32"), ("cell65", "cell65", "float32"), ("p257", "p257", "float32"),
        ("thresholds", "thresholds", "float32"))


def _finish(rs, x, y, z, labelled=True):
    """shuffle (index order and cell order unrelated), float32 coordinates, random colours and classes 0..12"""
    n = x.size
    perm = rs.permutation(n)
    x, y, z = (np.asarray(a, np.float64)[perm].astype(np.float32) for a in (x, y, z))
    rgb = rs.randint(0, 256, (3, n)).astype(np.uint8)
    label = rs.randint(0, 13, n).astype(np.uint8) if labelled else None
    return {"x": x, "y": y, "z": z, "red": rgb[0], "green": rgb[1], "blue": rgb[2], "label": label}


def _spread(rs, n, span=SPAN, offset=OFFSET):
    return offset[0] + span[0] * rs.rand(n), offset[1] + span[1] * rs.rand(n)


def cloud(name):
    """-> dict(x, y, z float32[P], red, green, blue uint8[P], label uint8[P] or None)"""
    rs = np.random.RandomState({"ties": 11, "dense": 12, "order": 13, "test_f64": 14, "lattice": 15, "far": 16, "one": 17,
                                "cell65": 18, "p257": 19, "thresholds": 20}[name])
    if name == "ties":                # z in steps of 1/4 over 16 levels: many cells share their maximum among points
        x, y = _spread(rs, 6000)
        return _finish(rs, x, y, 5.0 + rs.randint(0, 16, 6000) / 4.0)
    if name == "dense":               # 3000 of 5000 points inside one 5 cm square: one heavy cell, a quarter of the map empty
        x, y = _spread(rs, 5000)
        x[:3000] = OFFSET[0] + 1.52 + 0.05 * rs.rand(3000)
        y[:3000] = OFFSET[1] + 2.31 + 0.05 * rs.rand(3000)
        return _finish(rs, x, y, 5.0 + 45.0 * rs.rand(5000))
    if name == "order":               # 17 x 13 cells of ~54 points; tiny z next to z near 40: the sum depends on its order
        x, y = _spread(rs, 12000, span=(1.3, 1.7))
        z = 38.0 + 4.0 * rs.rand(12000)
        tiny = rs.rand(12000) < 0.3
        z[tiny] = 1e-7 * rs.rand(int(tiny.sum()))
        return _finish(rs, x, y, z)
    if name == "test_f64":
        x, y = _spread(rs, 6000)
        return _finish(rs, x, y, 5.0 + 45.0 * rs.rand(6000), labelled=False)
    if name == "lattice":             # from (0, 0); half the points exactly on float32(0.1 * k)
        x, y = _spread(rs, 6000, offset=(0.0, 0.0))
        kx, ky = rs.randint(0, 31, 3000), rs.randint(0, 47, 3000)
        kx[0] = ky[0] = 0
        x[:3000] = (0.1 * kx).astype(np.float32)
        y[:3000] = (0.1 * ky).astype(np.float32)
        return _finish(rs, x, y, 5.0 + 45.0 * rs.rand(6000))
    if name == "far":                 # float32 spacing at 43171 is 1/256 m: the subtraction works on coarse coordinates
        x, y = _spread(rs, 6000, offset=(43171.3, 8820.9))
        return _finish(rs, x, y, 5.0 + 45.0 * rs.rand(6000))
    if name == "one":
        return _finish(rs, np.array([OFFSET[0]]), np.array([OFFSET[1]]), np.array([7.25]))
    if name == "cell65":              # 65 points in one cell: h = w = 1
        return _finish(rs, np.full(65, OFFSET[0]), np.full(65, OFFSET[1]), 5.0 + 45.0 * rs.rand(65))
    if name == "p257":
        x, y = _spread(rs, 257)
        return _finish(rs, x, y, 5.0 + 45.0 * rs.rand(257))
    if name == "thresholds":          # a row of cells holding exactly THRESHOLD_COUNTS points, z in steps of 1/8 (ties everywhere)
        k = np.repeat(np.arange(len(THRESHOLD_COUNTS)), THRESHOLD_COUNTS)
        n = k.size
        x, y = OFFSET[0] + 0.1 * k + 0.02 + 0.06 * rs.rand(n), OFFSET[1] + 0.02 + 0.06 * rs.rand(n)
        x[0], y[0] = OFFSET                                      # the minimum: the cells start here
        return _finish(rs, x, y, 5.0 + rs.randint(0, 64, n) / 8.0)
    raise KeyError(name)


def case(key):
    """-> (cloud, arith) of a fixture key.  The reference reaches float64 only through the zero label column of the test
    split, so a float64 run has no labels"""
    name, arith = {k: (n, a) for k, n, a in RUNS}[key]
    c = cloud(name)
    if arith == "float64":
        c["label"] = None
    return c, arith


def pixel_index(v, grid, arith):
    """int32(trunc((v - min v) / grid)) in the arithmetic of the reference's stacked array: float32 columns on the labelled
    splits (the Python float grid takes the array's type), float64 on the test split"""
    if arith == "float32":
        v = np.asarray(v, np.float32)
        return ((v - v.min()) / np.float32(grid)).astype(np.int32)
    v = np.asarray(v, np.float32).astype(np.float64)
    return ((v - v.min()) / float(grid)).astype(np.int32)


def loop_np(c, grid=GRID, arith="float32", order=None):
    """The per-point loop, restated on flat per-cell arrays.  order: a permutation of the points to visit them in instead
    of 0..P-1 (for the generator's proof that the order matters); None = the reference's order."""
    h_idx, w_idx = pixel_index(c["y"], grid, arith), pixel_index(c["x"], grid, arith)
    h, w = int(h_idx.max()) + 1, int(w_idx.max()) + 1
    cell = h_idx.astype(np.int64) * w + w_idx
    z = c["z"].astype(np.float64)
    label = np.zeros(z.size) if c["label"] is None else c["label"].astype(np.float64)
    top, low, total, count = (np.zeros(h * w) for _ in range(4))
    colour = np.zeros((3, h * w))
    lab = np.full(h * w, -1.0)
    for i in (range(z.size) if order is None else order):
        k = cell[i]
        if count[k] == 0 or z[i] > top[k]:                     # strictly greater: the first point at the maximum stays
            top[k] = z[i]
            lab[k] = label[i]
            colour[:, k] = c["red"][i], c["green"][i], c["blue"][i]
        if count[k] == 0 or z[i] < low[k]:
            low[k] = z[i]
        total[k] += z[i]
        count[k] += 1
    fm = np.zeros((8, h * w))
    fm[0], fm[1], fm[2], fm[3], fm[4], fm[5:8] = top, low, total / (count + 1e-6), np.log10(count + 1), count > 0, colour
    return {"feature_map": fm.reshape(8, h, w), "label_map": lab.reshape(h, w), "h_idx": h_idx, "w_idx": w_idx}


def same_bits(a, b):
    """dtype, shape and every bit equal (float64 compared as int64 views: -0.0 and NaN payloads count)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))
                    and np.array_equal(a, b))
    return bool(np.array_equal(a, b))


def load_golden():
    g = np.load(GOLDEN)
    return {key: {k: g["%s.%s" % (key, k)] for k in KEYS} for key, _, _ in RUNS}
