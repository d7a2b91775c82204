"""EPMF evaluation task without a GPU: options and save-path layout, the centred pad-to-64 geometry, the C surface."""
import importlib.util
import math
import os
import re
import sys

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = os.path.join(ROOT, "tasks", "epmf_eval_semantickitti")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _task_modules():
    """option.py and infer.py of the task (infer.py imports `option` by its plain name, as the reference does)"""
    opt = _load("epmf_eval_option", os.path.join(TASK, "option.py"))
    saved = sys.modules.get("option")
    sys.modules["option"] = opt
    try:
        inf = _load("epmf_eval_infer", os.path.join(TASK, "infer.py"))
    finally:
        if saved is None:
            sys.modules.pop("option", None)
        else:
            sys.modules["option"] = saved
    return opt, inf


def _config(tmp_path, **kw):
    with open(os.path.join(TASK, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["pretrained_path"] = str(tmp_path / "trained")
    for k, v in kw.items():
        if k == "knn":
            cfg["post"]["KNN"]["use"] = v
        else:
            cfg[k] = v
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, cfg


def test_config_keys_match_the_reference_surface(tmp_path):
    _, cfg = _config(tmp_path)
    for k in ("net_type", "pretrained_path", "best_model", "save_preds", "has_label", "is_debug", "nclasses", "data_root",
              "dataset", "base_channels", "img_backbone", "experiment_id"):
        assert k in cfg, k
    for k in ("proj_h", "proj_w", "pcd_mean", "pcd_stds"):
        assert k in cfg["PVconfig"], k
    assert cfg["net_type"] == "EPMFNet" and cfg["post"]["KNN"]["use"] is False
    assert set(cfg["post"]["KNN"]["params"]) == {"knn", "search", "sigma", "cutoff"}


@pytest.mark.parametrize("knn", [False, True])
def test_option_parsing_and_save_path_layout(tmp_path, knn):
    opt, _ = _task_modules()
    path, cfg = _config(tmp_path, knn=knn, experiment_id="run7", best_model="best_IOU_model.pth")
    with pytest.raises(ValueError):                           # the trained model's folder must exist
        opt.Option(path)
    os.makedirs(cfg["pretrained_path"])
    o = opt.Option(path)
    knn_str = "KNN-{}".format(cfg["post"]["KNN"]["params"]["search"]) if knn else "noKNN"
    # reference option.py: os.path.join(pretrained_path, "Eval-{}-PMFNet-{}-{}-{}".format(dataset,
    # best_model.strip(".pth"), knn_str, experiment_id))
    assert o.save_path == os.path.join(cfg["pretrained_path"], "Eval-SemanticKitti-PMFNet-best_IOU_model-%s-run7" % knn_str)
    assert o.pretrained_model == os.path.join(cfg["pretrained_path"], "checkpoint", "best_IOU_model.pth")
    assert (o.n_classes, o.net_type, o.save_preds, o.has_label, o.is_debug) == (20, "EPMFNet", False, True, False)
    o.check_path()
    o.check_path()                                            # an existing directory: no prompt, no error
    assert os.path.isdir(o.save_path)


def test_only_epmfnet_is_evaluated(tmp_path):
    opt, inf = _task_modules()
    path, cfg = _config(tmp_path, net_type="PMFNet")
    os.makedirs(cfg["pretrained_path"])
    with pytest.raises(NotImplementedError):
        inf.init_model(opt.Option(path))


def _reference_pad(h, w):
    h_pad = math.ceil(h / 64.0) * 64 - h
    w_pad = math.ceil(w / 64.0) * 64 - w
    return (w_pad // 2, w_pad - w_pad // 2, h_pad // 2, h_pad - h_pad // 2)


@pytest.mark.parametrize("h,w", [(64, 128), (128, 64), (1, 1), (63, 65), (37, 101), (376, 1241), (320, 1280), (2, 127),
                                 (65, 129), (140, 182)])
def test_pad_geometry_matches_reference_formula(h, w):
    from pmf_amd.postproc.frame_eval import pad_geometry
    H, W, top, left = pad_geometry(h, w)
    l, r, t, b = _reference_pad(h, w)
    assert (H, W, top, left) == (h + t + b, w + l + r, t, l)
    assert H % 64 == 0 and W % 64 == 0 and 0 <= H - h < 64 and 0 <= W - w < 64
    # where torch.nn.ZeroPad2d puts the frame
    x = torch.nn.ZeroPad2d((l, r, t, b))(torch.ones(1, 1, h, w))
    nz = x[0, 0].nonzero()
    assert tuple(x.shape[2:]) == (H, W) and tuple(nz.min(0).values.tolist()) == (top, left)


def test_eval_symbols_declared_and_bound():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    for name in ("pmf_eval_pre", "pmf_eval_argmax", "pmf_eval_points"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    mk = open(os.path.join(ROOT, "pmf_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\beval\.hip\b", mk, re.M)


def test_frame_evaluator_has_no_cpu_fallback():
    from pmf_amd.postproc.frame_eval import eval_pre, window_argmax
    with pytest.raises(ValueError):
        eval_pre(torch.zeros(10, 4, 4), torch.zeros(5), torch.ones(5))
    with pytest.raises(ValueError):
        window_argmax(torch.zeros(3, 64, 64), 0, 0, 64, 64)
