"""SensatUrban dataset preparation on the MI355X: compute_bev_feature (csrc/bev_prepare.hip) against what the reference's own
_compute_feature returned for the clouds of tests/bev_prepare_cases.py (tests/golden/g20_bev_prepare.npz), bit for bit in
all four arrays -- no tolerance anywhere -- and the two preparation scripts end to end into the SensatUrban dataset class.

Clouds (a 47 x 31 map unless noted): `ties` (the first point at a shared maximum wins), `dense` (3001 points in one cell:
the workgroup path with its LDS sort, next to one-lane cells and empty ones), `order` (54 points per cell on average: both
paths, and a float64 sum that changes with the order of its terms), `test_f64` (no labels, float64 pixels), `lattice` in
both arithmetics (1249 points change pixel between them), `far` (coarse float32 coordinates), the launch edges P = 1,
65 points in one cell of a 1 x 1 map, P = 257 (one lane past a workgroup), and `thresholds`: a 1 x 8 map whose cells hold
32, 33, 1024, 0, 1025, 4096, 4097 and 1 points, either side of every count at which the cell pass takes another path."""
import importlib.util
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP = os.path.join(ROOT, "tasks", "sensat_urban", "dataset_prepare")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bev_prepare_cases as B  # noqa: E402
from tests import sensat_eval_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def _golden():
    if "g" not in _CACHE:
        _CACHE["g"] = B.load_golden()
    return _CACHE["g"]


def _run(key, **kw):
    from pmf_amd.dataset import compute_bev_feature
    c, arith = B.case(key)
    return compute_bev_feature(c["x"], c["y"], c["z"], c["red"], c["green"], c["blue"], label=c["label"], grid_size=B.GRID,
                               arith=arith, **kw)


def _assert_same(got, want, what):
    assert sorted(got) == sorted(B.KEYS)
    for k in B.KEYS:
        assert isinstance(got[k], np.ndarray), (what, k)
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        if want[k].dtype == np.float64:
            diff = got[k].view(np.int64) != want[k].view(np.int64)
            assert not diff.any(), (what, k, int(diff.sum()), np.argwhere(diff)[:5].tolist())
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("key", [k for k, _, _ in B.RUNS])
def test_frame_equals_the_reference_run_bit_for_bit(key):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = _run(key)
    dt = time.perf_counter() - t0
    print("%s: %d points, %.1f ms (upload, six passes, download; the first case includes library load)"
          % (key, got["h_idx"].size, 1e3 * dt))
    _assert_same(got, _golden()[key], key)


def test_second_call_returns_identical_bytes():
    a, b = _run("order"), _run("order")
    for k in B.KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    a, b = _run("dense"), _run("dense")
    for k in B.KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_device_tensors_hold_the_same_values():
    for key in ("ties", "test_f64"):
        got = _run(key, to_host=False)
        assert all(torch.is_tensor(v) and v.is_cuda for v in got.values())
        assert got["feature_map"].dtype == torch.float64 and got["label_map"].dtype == torch.float64
        assert got["h_idx"].dtype == torch.int32 and got["w_idx"].dtype == torch.int32
        _assert_same({k: v.cpu().numpy() for k, v in got.items()}, _golden()[key], key)


def test_tensor_inputs_on_the_device_and_another_grid():
    from pmf_amd.dataset import compute_bev_feature
    c = B.cloud("p257")
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    got = compute_bev_feature(t["x"], t["y"], t["z"], t["red"], t["green"], t["blue"], label=t["label"], grid_size=0.25)
    want = B.loop_np(c, grid=0.25)                               # the restatement the host suite pins to the reference run
    _assert_same(got, want, "grid 0.25")


@pytest.mark.parametrize("column", ["x", "y", "z"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_points_are_refused(column, value):
    from pmf_amd.dataset import compute_bev_feature
    c = B.cloud("p257")
    c[column] = c[column].copy()
    c[column][200] = value
    with pytest.raises(ValueError, match="non-finite"):
        compute_bev_feature(c["x"], c["y"], c["z"], c["red"], c["green"], c["blue"], label=c["label"])


def test_extent_beyond_the_cell_index_is_refused():
    from pmf_amd.dataset import compute_bev_feature
    c = B.cloud("p257")
    c["x"] = c["x"].copy()
    c["x"][0] = 1e30                                              # 1e31 cells along x
    with pytest.raises(ValueError, match="2\\^31 cells"):
        compute_bev_feature(c["x"], c["y"], c["z"], c["red"], c["green"], c["blue"], label=c["label"])
    c = B.cloud("p257")
    c["x"], c["y"] = c["x"].copy(), c["y"].copy()
    c["x"][0] += 7000.0
    c["y"][0] += 7000.0                                           # 70 000 x 70 000 cells: each axis fits, the product does not
    with pytest.raises(ValueError, match="int32 cell index"):
        compute_bev_feature(c["x"], c["y"], c["z"], c["red"], c["green"], c["blue"], label=c["label"])


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scripts_end_to_end_into_the_dataset_class(tmp_path, capsys):
    from pmf_amd.dataset import SensatUrban
    blocks = {"val": (("birmingham_block_0", "ties"), ("birmingham_block_5", "dense"), ("cambridge_block_9", "order")),
              "test": (("cambridge_block_7", "test_f64"),)}
    for split, items in blocks.items():
        os.makedirs(str(tmp_path / split))
        for name, key in reversed(items):
            c = B.cloud(key)
            S.write_ply(str(tmp_path / split / (name + ".ply")), np.stack([c["x"], c["y"], c["z"]], 1),
                        np.stack([c["red"], c["green"], c["blue"]], 1), c["label"] if split == "val" else None)
    prep = _load("compute_bev_feature_script", os.path.join(PREP, "compute_bev_feature.py"))
    ext = _load("extract_label_script", os.path.join(PREP, "extract_label.py"))
    prep.main([str(tmp_path), "--split", "val", "test"])
    ext.main([str(tmp_path), "--split", "val"])
    capsys.readouterr()
    for split, items in blocks.items():
        ds = SensatUrban(str(tmp_path), split, keep_idx=True)
        assert ds.data_split == [n + ".pth" for n, _ in items] and len(ds) == len(items)
        for i, (name, key) in enumerate(items):
            _assert_same(ds.readDataByIndex(i), _golden()[key], (split, name))
            if split == "val":
                lab = ds.readLabelByIndex(i)
                assert lab.dtype == np.uint8 and np.array_equal(lab, B.cloud(key)["label"])
                assert lab.size == ds.readDataByIndex(i)["h_idx"].size
    # --skip_existing leaves the files alone
    path = str(tmp_path / "val" / "birmingham_block_0.pth")
    stamp = os.stat(path).st_mtime_ns
    prep.main([str(tmp_path), "--split", "val", "--skip_existing"])
    assert os.stat(path).st_mtime_ns == stamp
