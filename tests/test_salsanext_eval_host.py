"""SalsaNext nuScenes evaluation without a GPU: the C surface, the wrappers' argument checks, options, the report formatter
and the properties of the devkit-free dataset and the fixture (so that the GPU tests cannot pass vacuously)."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = os.path.join(ROOT, "tasks", "salsanext_eval_nuscenes")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import salsa_eval_cases as S  # noqa: E402

NEW = "pmf_eval_range_batch"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_task():
    """(option module, infer module) of the task, loaded by path (infer.py imports `option` by its bare name)"""
    opt = _load("salsanext_eval_nus_option", os.path.join(TASK, "option.py"))
    saved = sys.modules.get("option")
    sys.modules["option"] = opt
    try:
        inf = _load("salsanext_eval_nus_infer", os.path.join(TASK, "infer.py"))
    finally:
        if saved is None:
            sys.modules.pop("option", None)
        else:
            sys.modules["option"] = saved
    return opt, inf


def test_new_symbol_declared_bound_and_built():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NEW, hdr)
    assert NEW in _lib.EXPORTS
    src = open(os.path.join(ROOT, "pmf_amd", "csrc", "eval.hip")).read()
    assert re.search(r'extern "C" int %s\(' % NEW, src)
    so = os.path.join(ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    assert hasattr(ctypes.CDLL(so), NEW)
    assert _lib.lib().pmf_eval_range_batch.argtypes is not None and len(_lib.lib().pmf_eval_range_batch.argtypes) == 24


def test_wrappers_reject_cpu_tensors_wrong_dtypes_and_even_search():
    from pmf_amd.postproc import RangeSweepEvaluator, range_batch_eval
    B, C, H, W, P = 2, 5, 4, 8, 6
    f32, i32 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    off = torch.tensor([0, 3, 6])
    with pytest.raises(ValueError):                       # CPU tensors
        range_batch_eval(f32(B, C, H, W), f32(B, H, W), off, i32(P), i32(P), f32(P))
    with pytest.raises(ValueError):
        range_batch_eval(f32(B, C, H, W).double(), f32(B, H, W), off, i32(P), i32(P), f32(P))
    with pytest.raises(ValueError, match="Nearest neighbor kernel must be odd number"):
        range_batch_eval(f32(B, C, H, W), f32(B, H, W), off, i32(P), i32(P), f32(P), knn=(5, 4, f32(16), 1.0))
    with pytest.raises(ValueError, match="Nearest neighbor kernel must be odd number"):
        RangeSweepEvaluator(C, {"knn": 5, "search": 6, "sigma": 1.0, "cutoff": 1.0}, device="cpu")
    ev = RangeSweepEvaluator(C, None, device="cpu")
    items = [dict(px=i32(3), py=i32(3), depth=f32(3), sem=i32(3), lut=i32(256), label=f32(H, W), proj_range=f32(H, W))
             for _ in range(B)]
    with pytest.raises(ValueError):
        ev.post(f32(B, C, H, W), items)                   # CPU maps
    with pytest.raises(ValueError):
        ev.post(f32(B + 1, C, H, W), items)               # one map per item
    assert ev.post(f32(0, C, H, W), []) == []
    if torch.cuda.is_available():                         # dtype checks behind the device check need device tensors
        d = lambda t: t.cuda()
        with pytest.raises(ValueError):
            range_batch_eval(d(f32(B, C, H, W)), None, d(off), d(i32(P)).long(), d(i32(P)).long(), None)
        with pytest.raises(ValueError):
            range_batch_eval(d(f32(B, C, H, W)), None, d(off).int(), d(i32(P)), d(i32(P)), None)
        with pytest.raises(ValueError):
            range_batch_eval(d(f32(B, C, H, W)), None, d(off), d(i32(P)), d(i32(P)), None,
                             pixel_conf=d(torch.zeros(C, C, dtype=torch.int32)), label=d(f32(B, H, W)))


def test_option_reads_the_shipped_config(tmp_path):
    opt, _ = load_task()
    with open(os.path.join(TASK, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    s = cfg["sensor"]
    assert (s["proj_h"], s["proj_w"], s["fov_up"], s["fov_down"]) == (32, 2048, 10.0, -30.0)
    assert (s["fov_left"], s["fov_right"]) == (-180, 180)
    assert cfg["n_classes"] == 17 and cfg["dataset"] == "nuScenes" and cfg["net_type"] == "SalsaNext"
    assert cfg["eval_batch_size"] == 4
    assert cfg["post"]["KNN"]["use"] is False and cfg["post"]["KNN"]["params"] == S.KNN_PARAMS
    with open(os.path.join(ROOT, "tasks", "salsanext", "config_server_kitti.yaml")) as f:
        kitti = yaml.safe_load(f)
    assert set(s) == set(kitti["sensor"]) and set(cfg["post"]["KNN"]["params"]) == set(kitti["post"]["KNN"]["params"])
    assert s["img_mean"] == S.CONFIG["sensor"]["img_mean"] and s["img_stds"] == S.CONFIG["sensor"]["img_stds"]
    cfg.update(save_path=str(tmp_path), experiment_id="run3", pretrained_model=None)
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    o = opt.Option(path)
    assert o.save_path == os.path.join(str(tmp_path), "Eval-SV_nuScenes_SalsaNext__run3")
    assert (o.n_classes, o.eval_batch_size, o.has_label, o.pretrained_model) == (17, 4, True, None)
    o.check_path()
    o.check_path()
    assert os.path.isdir(o.save_path)
    cfg["post"]["KNN"]["use"] = True
    del cfg["eval_batch_size"]
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    o = opt.Option(path)
    assert o.save_path.endswith("Eval-SV_nuScenes_SalsaNext_KNN-5_run3") and o.eval_batch_size == 4
    cfg["eval_batch_size"] = 0
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(ValueError):
        opt.Option(path)


def test_nuscenes_lidar_only_dataset_needs_the_devkit():
    import pc_processor
    with pytest.raises(ImportError, match="nuscenes-devkit"):
        pc_processor.dataset.nuScenes.Nuscenes(root="/nonexistent", version="v1.0-trainval", split="val", has_image=False)


def test_report_formatter_on_a_known_confusion_matrix():
    from pmf_amd.metrics import IOUEval
    _, inf = load_task()
    n = 4
    conf = torch.tensor([[7, 1, 2, 3],          # row 0 / column 0: the ignored class
                         [5, 6, 2, 0],
                         [4, 1, 3, 0],
                         [9, 1, 0, 0]])
    ev = IOUEval(n_classes=n, device=torch.device("cpu"), ignore=[0])
    ev.conf_matrix += conf
    ev.external_update()
    names = {i: "c%d" % i for i in range(n)}
    text = "\n".join(inf.report_lines("Point-wise Evaluation Results (3D eval)", ev, names, n, True))
    # by hand: tp = (6, 3, 0); pred totals (rows) 8, 4, 1; gt totals (columns) 8, 5, 0
    iou = [6 / 10, 3 / 6, 0.0]
    acc = [6 / 8, 3 / 4, 0.0]
    rec = [6 / 8, 3 / 5, 0.0]
    assert "Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(sum(acc) / 3, sum(iou) / 3, sum(rec) / 3) in text
    for i in range(3):
        assert re.search(r"^%d\s*\| c%d\s*\| %.4f\s*\| %.4f\s*\| %.4f\s*$" % (i + 1, i + 1, iou[i], acc[i], rec[i]), text, re.M)
    assert " & 60.0 & 50.0 & 0.0 & 36.7" in text
    assert re.search(r"^c1\s*\| 8\s*\| 0.6154\s*$", text, re.M) and re.search(r"^c0\s*\| 0\s*\| 0.0000\s*$", text, re.M)
    assert "fwIoU: {}".format(0.6 * 8 / 13 + 0.5 * 5 / 13) in text
    assert re.search(r"^1 \| 0 \| 6 \| 2 \| 0\s*$", text, re.M) and re.search(r"^0 \| 0 \| 0 \| 0 \| 0\s*$", text, re.M)
    assert re.search(r"---- ACC matrix -+\n\n\s+\| c1\s+\| c2\s+\| c3\s*\n[-+]+\nc1\s*\| 75.0\s*\| 25.0\s*\| 0.0\s*\nc2\s*\| 25.0\s*\| 75.0\s*\| 0.0\s*\nc3\s*\| 100.0\s*\| 0.0", text)
    assert re.search(r"---- Recall matrix -+\n\n\s+\| c1\s+\| c2\s+\| c3\s*\n[-+]+\nc1\s*\| 75.0\s*\| 40.0\s*\| 0.0\s*\nc2\s*\| 12.5\s*\| 60.0\s*\| 0.0", text)
    pix = "\n".join(inf.report_lines("Pixel-wise Evaluation Results (2D eval)", ev, names, n, False))
    assert "Pixel Acc avg:" in pix and "fwIoU" not in pix and "Percentage" not in pix


def test_synthetic_dataset_and_fixture_meet_the_conditions_of_the_gpu_tests():
    ds = S.SyntheticSalsaNus()
    s = S.CONFIG["sensor"]
    H, W = s["proj_h"], s["proj_w"]
    assert len(ds) == 3 and all(isinstance(t, str) for t in ds.token_list)
    assert os.path.isfile(S.GOLDEN) and os.path.getsize(S.GOLDEN) < (1 << 20)
    g = np.load(S.GOLDEN)
    prob = S.prob_maps(int(g["seed"]), 3)
    assert prob.dtype == np.float32 and prob.shape == (3, S.NCLASSES, H, W) and S.top2_gap(prob) > 0
    assert np.abs(prob.sum(1) - 1).max() < 1e-5
    table = ds.map_name_from_general_index_to_segmentation_index
    assert len(table) == 32 and set(table.values()) <= set(range(S.NCLASSES)) and len(ds.mapped_cls_name) == S.NCLASSES
    counts = set()
    changed = total = 0
    for i in range(3):
        pts, raw, _ = ds.loadDataByIndex(i)
        assert pts.dtype == np.float32 and pts.shape[1] == 4 and raw.dtype == np.uint8 and raw.shape == (pts.shape[0], 1)
        assert 5500 <= pts.shape[0] <= 6500
        counts.add(pts.shape[0])
        mapped = ds.labelMapping(raw)
        assert mapped.shape == (pts.shape[0],) and np.array_equal(mapped, [table[int(r)] for r in raw[:, 0]])
        px, py = g["s%d.px" % i], g["s%d.py" % i]
        assert px.dtype == py.dtype == np.int32 and px.shape == (pts.shape[0],)
        assert 0 <= px.min() and px.max() < W and 0 <= py.min() and py.max() < H
        pix = py.astype(np.int64) * W + px
        assert np.unique(pix).size < 0.95 * pix.size                       # points sharing a pixel
        assert (g["s%d.proj_range" % i] < 0).mean() > 0.25                  # empty pixels (range -1)
        am = prob[i].argmax(0)
        assert np.array_equal(g["s%d.gather" % i], am[py, px])
        assert g["s%d.gather" % i].dtype == np.int32 and g["s%d.knn" % i].dtype == np.int32
        changed += int((g["s%d.gather" % i] != g["s%d.knn" % i]).sum())
        total += px.shape[0]
        # the vote of the fixture does not rest on the order among equal distances
        from pmf_amd.postproc.knn import inverse_gaussian_window
        w = inverse_gaussian_window(S.KNN_PARAMS["search"], S.KNN_PARAMS["sigma"]).numpy()
        args = (g["s%d.proj_range" % i], g["s%d.depth" % i], am, px.astype(np.int64), py.astype(np.int64), w, S.NCLASSES)
        assert np.array_equal(S.knn_vote_np(*args), g["s%d.knn" % i])
        assert np.array_equal(S.knn_vote_np(*args, reverse=True), g["s%d.knn" % i])
    assert len(counts) == 3, "ragged batch"
    assert changed >= 0.01 * total
    C = S.NCLASSES
    for key in ("pixel_conf", "point_conf_gather", "point_conf_knn"):
        assert g[key].shape == (C, C) and g[key].dtype == np.int64
    assert g["pixel_conf"].sum() == 3 * H * W and g["point_conf_gather"].sum() == total == g["point_conf_knn"].sum()
    assert g["point_conf_knn"][0].sum() == 0 and g["point_conf_gather"][0].sum() > 0      # the vote never says class 0
