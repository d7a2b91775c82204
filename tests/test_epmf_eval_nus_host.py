"""EPMF nuScenes evaluation without a GPU: the C surface, the bottom pad geometry, options, the devkit-free dataset's
properties (so that the GPU tests cannot pass vacuously) and the merge stated two ways."""
import ctypes
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = os.path.join(ROOT, "tasks", "epmf_eval_nuscenes")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import nus_v2_cases as N  # noqa: E402

NEW = ("pmf_eval_view_merge", "pmf_eval_sweep_finish")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_symbols_declared_bound_and_built():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    mk = open(os.path.join(ROOT, "pmf_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\beval\.hip\b", mk, re.M)
    src = open(os.path.join(ROOT, "pmf_amd", "csrc", "eval.hip")).read()
    for name in NEW:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    so = os.path.join(ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    lib = ctypes.CDLL(so)
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("h,w", [(1, 1), (63, 65), (450, 960), (640, 1280), (900, 1600), (64, 128), (65, 129), (37, 101)])
def test_pad_geometry_bottom_matches_reference_placement(h, w):
    from pmf_amd.postproc.frame_eval import pad_geometry_bottom
    h_pad = math.ceil(h / 64.0) * 64 - h
    w_pad = math.ceil(w / 64.0) * 64 - w
    H, W, top, left = pad_geometry_bottom(h, w)
    assert (H, W, top, left) == (h + h_pad, w + w_pad, 0, w_pad // 2)
    x = torch.nn.ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, 0, h_pad))(torch.ones(1, 1, h, w))
    nz = x[0, 0].nonzero()
    assert tuple(x.shape[2:]) == (H, W)
    assert tuple(nz.min(0).values.tolist()) == (top, left) and tuple(nz.max(0).values.tolist()) == (h - 1, left + w - 1)


def test_option_loads_the_shipped_config(tmp_path):
    opt = _load("epmf_eval_nus_option", os.path.join(TASK, "option.py"))
    with open(os.path.join(TASK, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["nclasses"] == 17 and cfg["dataset"] == "nuScenes" and cfg["net_type"] == "EPMFNet"
    assert (cfg["PVconfig"]["proj_h"], cfg["PVconfig"]["proj_w"]) == (640, 1280)
    assert cfg["PVconfig"]["pcd_mean"] == N.MEAN and cfg["PVconfig"]["pcd_stds"] == N.STDS
    assert cfg["post"]["KNN"]["use"] is False and cfg["post"]["KNN"]["params"] == N.KNN_PARAMS
    cfg["pretrained_path"] = str(tmp_path / "trained")
    cfg["experiment_id"] = "run3"
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(ValueError):
        opt.Option(path)
    os.makedirs(cfg["pretrained_path"])
    o = opt.Option(path)
    assert o.save_path == os.path.join(cfg["pretrained_path"], "Eval-nuScenes-PMFNet-best_IOU_model-noKNN-run3")
    assert (o.n_classes, o.save_pred_results, o.has_label, o.is_debug) == (17, False, True, False)
    o.check_path()
    o.check_path()
    assert os.path.isdir(o.save_path)


def test_nuscenes_v2_needs_the_devkit():
    import pc_processor
    with pytest.raises(ImportError, match="nuscenes-devkit"):
        pc_processor.dataset.nuScenes.NuscenesV2(root="/nonexistent", version="v1.0-mini", split="val")
    with pytest.raises(ImportError, match="nuscenes-devkit"):
        pc_processor.dataset.nuScenes.Nuscenes(root="/nonexistent", version="v1.0-mini", split="val")


def test_sweep_evaluator_and_wrappers_reject_cpu_tensors():
    from pmf_amd.postproc.frame_eval import SweepEvaluator, sweep_finish, view_merge
    se = SweepEvaluator(6, N.MEAN, N.STDS, device="cpu")
    with pytest.raises(ValueError):
        se.pre(torch.zeros(10, 4, 4))
    with pytest.raises(ValueError):
        se.post_view(torch.zeros(1, 6, 64, 64), torch.zeros(3), {})
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ValueError):
        view_merge(torch.zeros(6, 64, 64), 0, 0, 64, 64, i32(3), i32(3), 0, 0, i32(3), torch.zeros(9), i32(9))
    with pytest.raises(ValueError):
        sweep_finish(torch.zeros(9), i32(9), 6)
    with pytest.raises(RuntimeError):
        se.finish(None, None, 9)                     # no view yet


def test_training_path_on_nuscenes_v2_is_refused():
    from pmf_amd.dataset.perspective_view_loader_v2 import PerspectiveViewLoaderV2
    cfg = {"PVconfig": {"proj_h": 64, "proj_w": 128, "proj_ht": 64, "proj_wt": 128, "img_jitter": [0.4, 0.4, 0.4]}}
    ld = PerspectiveViewLoaderV2(N.SyntheticNusV2(sweeps=1, npts=500), cfg, is_train=True)
    assert ld._is_nus_v2()
    with pytest.raises(NotImplementedError):
        ld[0]


def test_synthetic_dataset_meets_the_conditions_of_the_gpu_tests():
    ds = N.SyntheticNusV2()
    assert not hasattr(ds, "proj_matrix") and len(ds) == 12
    negative = False
    for s in range(2):
        P = ds.loadDataByIndex(6 * s)[0].shape[0]
        seen = np.zeros(P, np.int64)
        shapes = set()
        for v in range(6):
            crop, xy, keep, xd, yd, x_min, y_min, h, w, H, W, left = N.view_geometry(ds, 6 * s + v)
            assert crop.dtype == np.float32 and crop.shape == (int(keep.sum()), 4) and xy.dtype == np.float64
            assert keep.dtype == np.bool_ and keep.shape == (P,) and ds.token_list[6 * s + v]["lidar_token"] == \
                ds.token_list[6 * s]["lidar_token"]
            seen += keep
            shapes.add((H, W))
            negative = negative or x_min < 0 or y_min < 0
            pix = (xd.astype(np.int64) - x_min) * w + (yd - y_min)
            assert np.unique(pix).size < pix.size             # duplicate pixels: the last-writer order matters
        assert (seen >= 2).mean() >= 0.05, "views must overlap"
        assert (seen == 0).mean() >= 0.01, "some points are kept by no view"
        assert len(shapes) >= 2, shapes
    assert negative
    assert os.path.isfile(N.GOLDEN) and os.path.getsize(N.GOLDEN) < (1 << 20)


def test_merge_mask_form_equals_src_form():
    """the reference's boolean-mask merge against the src-indexed form of pmf_eval_view_merge, on merge_case-style data:
    exact ties between views (first wins), zero confidences (never win against the zero state), unseen points"""
    from oracle.cases import merge_case
    for seed in (0, 1, 2):
        P = 4000
        idx, conf, lab = merge_case(seed, P)
        a = (np.zeros(P, np.float32), np.zeros(P, np.int32))
        b = (np.zeros(P, np.float32), np.zeros(P, np.int32))
        for i, c, l in zip(idx, conf, lab):
            order = np.argsort(i, kind="stable")              # a keep mask lists the points in file order
            i, c, l = i[order], c[order], l[order].astype(np.int32)
            assert np.unique(i).size == i.size                # no duplicates inside one view
            keep = np.zeros(P, bool)
            keep[i] = True
            N.merge_mask_form(a[0], a[1], keep, c, l)
            N.merge_src_form(b[0], b[1], np.flatnonzero(keep), c, l)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[1][3] == 4 and a[0][3] == np.float32(0.5)    # tie: the first view
        assert a[1][5] == 11                                  # higher confidence wins
        assert a[0][1] == 0 and a[1][1] == 0 and a[1][2] == 0  # zero confidence never beats the zero state
        assert a[0][0] == 0 and a[1][6] == 0                  # unseen
