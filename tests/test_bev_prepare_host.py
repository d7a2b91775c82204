"""SensatUrban dataset preparation without a GPU: the numpy restatement of the reference's loop against the reference run
recorded in tests/golden/g20_bev_prepare.npz, the conditions the clouds exist for, the C surface and its argument guards,
extract_label, and the preparation script's file handling (with the device call replaced by the restatement)."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP = os.path.join(ROOT, "tasks", "sensat_urban", "dataset_prepare")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bev_prepare_cases as B  # noqa: E402
from tests import sensat_eval_cases as S  # noqa: E402

NEW = {"pmf_bev_prepare_workspace": 3, "pmf_bev_prepare_extent": 9, "pmf_bev_prepare_bin": 12, "pmf_bev_prepare_scan": 6,
       "pmf_bev_prepare_place": 8, "pmf_bev_prepare_cells": 15}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


@pytest.mark.parametrize("key", [k for k, _, _ in B.RUNS])
def test_restatement_equals_the_reference_run(golden, key):
    c, arith = B.case(key)
    got = B.loop_np(c, arith=arith)
    for k in B.KEYS:
        want = golden[key][k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (key, k)
        if want.dtype == np.float64:
            assert np.array_equal(got[k].view(np.int64), want.view(np.int64)), (key, k)
        assert np.array_equal(got[k], want), (key, k)
    assert golden[key]["feature_map"].dtype == np.float64 and golden[key]["label_map"].dtype == np.float64
    assert golden[key]["h_idx"].dtype == np.int32 and golden[key]["w_idx"].dtype == np.int32


def test_fixture_is_small_and_the_clouds_meet_their_conditions(golden):
    assert os.path.getsize(B.GOLDEN) < (1 << 20)
    assert golden["ties"]["feature_map"].shape == (8, 47, 31) and golden["order"]["feature_map"].shape == (8, 17, 13)
    assert golden["one"]["feature_map"].shape == (8, 1, 1) and golden["cell65"]["feature_map"].shape == (8, 1, 1)
    # ties: >= 10 cells whose maximum is shared by points of different class
    c, o = B.cloud("ties"), golden["ties"]
    cell = o["h_idx"].astype(np.int64) * 31 + o["w_idx"]
    at_max = c["z"].astype(np.float64) == o["feature_map"][0].reshape(-1)[cell]
    shared = sum(1 for k in np.unique(cell[at_max]) if np.unique(c["label"][at_max & (cell == k)]).size > 1)
    assert shared >= 10
    # dense: one cell of >= 3000 points, >= 20 % of the map empty
    fm = golden["dense"]["feature_map"]
    assert np.bincount(golden["dense"]["h_idx"] * 31 + golden["dense"]["w_idx"]).max() >= 3000
    assert (fm[4] == 0).mean() >= 0.2 and not fm[:, fm[4] == 0].any() and (golden["dense"]["label_map"][fm[4] == 0] == -1).all()
    # order: >= 50 cells whose mean changes under a scrambled in-cell order
    c = B.cloud("order")
    scr = B.loop_np(c, order=np.random.RandomState(0).permutation(c["z"].size))
    assert (scr["feature_map"][2] != golden["order"]["feature_map"][2]).sum() >= 50
    assert np.array_equal(scr["feature_map"][[0, 1, 3, 4]], golden["order"]["feature_map"][[0, 1, 3, 4]])
    # lattice: >= 500 points whose pixel differs between the arithmetics
    a, b = golden["lattice_f32"], golden["lattice_f64"]
    assert ((a["h_idx"] != b["h_idx"]) | (a["w_idx"] != b["w_idx"])).sum() >= 500
    # thresholds: the cells hold exactly the counts at which the cell pass changes path
    o = golden["thresholds"]
    assert tuple(np.bincount(o["w_idx"], minlength=len(B.THRESHOLD_COUNTS))) == B.THRESHOLD_COUNTS and not o["h_idx"].any()
    # the test split: label 0 where occupied, -1 elsewhere
    t = golden["test_f64"]
    assert set(np.unique(t["label_map"])) == {-1.0, 0.0} and ((t["label_map"] == 0) == (t["feature_map"][4] == 1)).all()


def test_new_symbols_declared_bound_and_built():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    src = open(os.path.join(ROOT, "pmf_amd", "csrc", "bev_prepare.hip")).read()
    mk = open(os.path.join(ROOT, "pmf_amd", "csrc", "Makefile")).read()
    so = os.path.join(ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    assert re.search(r"^SRCS = .*\bbev_prepare\.hip\b", mk, re.M)
    assert "fast-math" not in mk and "fp contract(off)" in src
    for name, nargs in NEW.items():
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, hdr)
        assert name in _lib.EXPORTS
        assert re.search(r'extern "C" int(64_t)? %s\(' % name, src)
        assert hasattr(ctypes.CDLL(so), name)
        assert len(getattr(_lib.lib(), name).argtypes) == nargs


def test_exports():
    import pc_processor
    from pmf_amd.dataset import compute_bev_feature
    from pmf_amd.dataset.sensat_urban import prepare
    assert pc_processor.dataset.compute_bev_feature is compute_bev_feature is prepare.compute_bev_feature
    assert sys.modules["pc_processor.dataset.sensat_urban.prepare"] is prepare
    assert pc_processor.dataset.sensat_urban.compute_bev_feature is compute_bev_feature
    assert prepare.SPLIT_ARITH == {"train": "float32", "val": "float32", "test": "float64"}
    with np.errstate(divide="ignore"):
        assert np.array_equal(prepare.log10_table(5)[1:], np.log10(np.arange(1, 7)))
    assert prepare.log10_table(5).dtype == np.float64 and prepare.log10_table(5).size == 7


def test_argument_guards_raise_without_a_device():
    from pmf_amd.dataset import compute_bev_feature
    c = B.cloud("p257")
    cols = [c[k] for k in ("x", "y", "z", "red", "green", "blue")]
    with pytest.raises(ValueError, match="arith"):
        compute_bev_feature(*cols, label=c["label"], arith="float16")
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="grid_size"):
            compute_bev_feature(*cols, label=c["label"], grid_size=bad)
    with pytest.raises(ValueError, match="empty"):
        compute_bev_feature(*[a[:0] for a in cols])
    with pytest.raises(ValueError, match="y has 256 entries"):
        compute_bev_feature(cols[0], cols[1][:256], *cols[2:])
    with pytest.raises(ValueError, match="label has"):
        compute_bev_feature(*cols, label=c["label"][:5])
    with pytest.raises(ValueError, match="x must be"):
        compute_bev_feature(cols[0].astype(np.float64), *cols[1:])
    with pytest.raises(ValueError, match="red must be"):
        compute_bev_feature(*cols[:3], cols[3].astype(np.int32), *cols[4:])
    with pytest.raises(ValueError, match="GPU only"):
        compute_bev_feature(*cols, label=c["label"], device="cpu")
    # the library's own guards (host-side: nothing is launched)
    from pmf_amd import _lib
    lib = _lib.lib()
    p, E = 4096, _lib.PMF_E_ARG                                    # a non-null pointer that is never dereferenced
    assert lib.pmf_bev_prepare_workspace(0, 0, 0) == E and lib.pmf_bev_prepare_workspace(2 ** 31 - 1, 0, 0) == E
    assert lib.pmf_bev_prepare_workspace(100, 0, 5) == E and lib.pmf_bev_prepare_workspace(100, 65536, 32768) == E
    assert lib.pmf_bev_prepare_workspace(100, 0, 0) > 0
    small, full = lib.pmf_bev_prepare_workspace(6000, 0, 0), lib.pmf_bev_prepare_workspace(6000, 47, 31)
    assert full >= small + 2 * 47 * 31 * 4 + 6000 * 4
    assert lib.pmf_bev_prepare_extent(p, p, p, 0, 0.1, 0, p, p, None) == E                          # P == 0
    assert lib.pmf_bev_prepare_extent(p, p, p, 2 ** 31, 0.1, 0, p, p, None) == E                    # P >= 2^31
    assert lib.pmf_bev_prepare_extent(p, p, p, 2 ** 31 - 1, 0.1, 0, p, p, None) == E
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, 0.0, 0, p, p, None) == E                         # grid <= 0
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, -0.1, 1, p, p, None) == E
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, float("nan"), 0, p, p, None) == E
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, 1e-60, 0, p, p, None) == E                       # 0 as a float32
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, 0.1, 2, p, p, None) == E                         # arith
    assert lib.pmf_bev_prepare_extent(0, p, p, 10, 0.1, 0, p, p, None) == E                         # null x
    assert lib.pmf_bev_prepare_extent(p, p, p, 10, 0.1, 0, p, 0, None) == E                         # null extent
    assert lib.pmf_bev_prepare_bin(p, p, 10, 0.1, 0, p, 0, 5, p, p, p, None) == E                   # h == 0
    assert lib.pmf_bev_prepare_bin(p, p, 10, 0.1, 0, p, 65536, 32768, p, p, p, None) == E           # h * w = 2^31
    assert lib.pmf_bev_prepare_bin(p, p, 10, 0.0, 0, p, 4, 5, p, p, p, None) == E
    assert lib.pmf_bev_prepare_bin(p, p, 10, 0.1, 0, p, 4, 5, p, 0, p, None) == E                   # null h_idx
    assert lib.pmf_bev_prepare_scan(10, 65536, 32768, p, p, None) == E
    assert lib.pmf_bev_prepare_scan(0, 4, 5, p, p, None) == E
    assert lib.pmf_bev_prepare_scan(10, 4, 5, 0, p, None) == E
    assert lib.pmf_bev_prepare_place(p, p, 10, 4, -1, p, p, None) == E
    assert lib.pmf_bev_prepare_place(p, 0, 10, 4, 5, p, p, None) == E
    assert lib.pmf_bev_prepare_cells(p, p, p, p, 0, 10, 4, 5, p, p, 4, 3, p, p, None) == E          # table shorter than count + 2
    assert lib.pmf_bev_prepare_cells(p, p, p, p, 0, 10, 4, 5, p, p, 40, 11, p, p, None) == E        # max count > P
    assert lib.pmf_bev_prepare_cells(p, p, p, p, 0, 10, 4, 5, p, p, 40, 0, p, p, None) == E
    assert lib.pmf_bev_prepare_cells(p, p, p, p, 0, 10, 4, 5, p, 0, 40, 3, p, p, None) == E         # null table
    assert lib.pmf_bev_prepare_cells(p, p, p, p, 0, 10, 4, 5, p, p, 40, 3, 0, p, None) == E         # null map


def _ply_tree(root, splits=("val", "test")):
    """three blocks per split from the fixture's clouds, written in unsorted order -> {split: {name: cloud}}"""
    tree = {}
    for split in splits:
        os.makedirs(os.path.join(root, split))
        tree[split] = {}
        for name, cl in (("cambridge_block_9", "p257"), ("birmingham_block_0", "far"), ("birmingham_block_5", "cell65")):
            c = B.cloud(cl)
            S.write_ply(os.path.join(root, split, name + ".ply"), np.stack([c["x"], c["y"], c["z"]], 1),
                        np.stack([c["red"], c["green"], c["blue"]], 1), c["label"] if split != "test" else None)
            tree[split][name] = c
        with open(os.path.join(root, split, "notes.txt"), "w") as f:
            f.write("not a block\n")
    return tree


def test_extract_label_writes_the_class_bytes(tmp_path):
    ext = _load("extract_label_under_test", os.path.join(PREP, "extract_label.py"))
    tree = _ply_tree(str(tmp_path))
    lines = []
    written = ext.run(str(tmp_path), ("val",), log=lines.append)
    assert written == [os.path.join(str(tmp_path), "val", n + ".bin")
                       for n in ("birmingham_block_0", "birmingham_block_5", "cambridge_block_9")]
    for name, c in tree["val"].items():
        path = os.path.join(str(tmp_path), "val", name + ".bin")
        assert os.path.getsize(path) == c["label"].size
        assert open(path, "rb").read() == c["label"].tobytes()
    assert ext.run(str(tmp_path), ("val",), skip_existing=True, log=lines.append) == []
    with pytest.raises(ValueError, match="invalid split"):
        ext.run(str(tmp_path), ("test",))
    ext.main([str(tmp_path), "--split", "val", "--skip_existing"])
    with pytest.raises(SystemExit):
        ext.main([str(tmp_path), "--split", "test"])


def test_script_names_order_skip_and_arithmetic_per_split(tmp_path):
    """the script's file handling, with the device call replaced by the restatement (the GPU test runs the real one)"""
    prep = _load("compute_bev_feature_under_test", os.path.join(PREP, "compute_bev_feature.py"))
    tools = _load("sensat_tools_for_prepare", os.path.join(ROOT, "tasks", "sensat_urban", "pmf_eval", "sensat_tools.py"))
    assert os.path.samefile(prep.sensat_tools.__file__, tools.__file__)                            # the shared reader
    assert "def read_ply" not in open(os.path.join(PREP, "compute_bev_feature.py")).read()
    tree = _ply_tree(str(tmp_path))
    calls = []

    def fake(x, y, z, red, green, blue, label=None, grid_size=0.1, arith="float32"):
        calls.append((x.size, arith, label is None, grid_size))
        return B.loop_np({"x": x, "y": y, "z": z, "red": red, "green": green, "blue": blue, "label": label}, grid_size, arith)

    order = ["birmingham_block_0", "birmingham_block_5", "cambridge_block_9"]
    written = prep.run(str(tmp_path), ("val", "test"), compute=fake, log=lambda s: None)
    assert written == [(os.path.join(str(tmp_path), sp, n + ".pth"), a)
                       for sp, a in (("val", "float32"), ("test", "float64")) for n in order]
    assert calls == [(n, a, nolab, 0.1) for a, nolab in (("float32", False), ("float64", True)) for n in (6000, 65, 257)]
    for split in ("val", "test"):
        assert sorted(f for f in os.listdir(os.path.join(str(tmp_path), split)) if f.endswith(".pth")) == \
            [n + ".pth" for n in order]
    golden = B.load_golden()
    frame = torch.load(os.path.join(str(tmp_path), "val", "birmingham_block_0.pth"), weights_only=False)
    assert sorted(frame) == sorted(B.KEYS)
    for k in B.KEYS:                                              # through write_ply, read_ply and torch.save unchanged
        assert B.same_bits(frame[k], golden["far"][k]), k
    # --skip_existing: only the missing frame is computed again
    os.remove(os.path.join(str(tmp_path), "val", "birmingham_block_5.pth"))
    del calls[:]
    again = prep.run(str(tmp_path), ("val",), skip_existing=True, compute=fake, log=lambda s: None)
    assert again == [(os.path.join(str(tmp_path), "val", "birmingham_block_5.pth"), "float32")] and len(calls) == 1
    assert prep.run(str(tmp_path), ("val",), grid_size=0.2, compute=fake, log=lambda s: None)[0][1] == "float32"
    assert calls[-1][3] == 0.2
    with pytest.raises(ValueError, match="invalid split"):
        prep.run(str(tmp_path), ("valid",), compute=fake)
    # a labelled split whose block has no class is an error, not a silent zero label
    os.makedirs(str(tmp_path / "bad" / "train"))
    c = B.cloud("one")
    S.write_ply(str(tmp_path / "bad" / "train" / "a.ply"), np.stack([c["x"], c["y"], c["z"]], 1),
                np.stack([c["red"], c["green"], c["blue"]], 1), None)
    with pytest.raises(ValueError, match="no class"):
        prep.run(str(tmp_path / "bad"), ("train",), compute=fake, log=lambda s: None)
    assert tools.read_ply(str(tmp_path / "bad" / "train" / "a.ply")).shape == (1,)
    # the command line
    ap = prep.main
    with pytest.raises(SystemExit):
        ap([str(tmp_path), "--split", "valid"])
