"""Full-sweep nuScenes fusion without a GPU: the C surface, the numpy statement of the rule against the reference's recorded
result (tests/golden/g18_nus_fill.npz, written by tools/make_golden_nus_fill.py: the reference's own MergePred._mergeResult
and IOUEval on tests/nus_fill_cases.py), the wrappers' argument checks, the merge task's options, file reader and
devkit-free validator.  All comparisons are integer and exact."""
import ctypes
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = os.path.join(ROOT, "tasks", "pmf_eval_nuscenes", "testset_eval")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import nus_fill_cases as F  # noqa: E402

NEW = ("pmf_eval_fill", "pmf_eval_sweep_finish_fill")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_task():
    """(option, main, check_valid) modules of the merge task, loaded by path (they import `option` by its bare name)"""
    opt = _load("nus_fill_option", os.path.join(TASK, "option.py"))
    saved = sys.modules.get("option")
    sys.modules["option"] = opt
    try:
        main = _load("nus_fill_main", os.path.join(TASK, "main.py"))
        chk = _load("nus_fill_check_valid", os.path.join(TASK, "check_valid.py"))
    finally:
        if saved is None:
            sys.modules.pop("option", None)
        else:
            sys.modules["option"] = saved
    return opt, main, chk


def test_new_symbols_declared_bound_and_built():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    src = open(os.path.join(ROOT, "pmf_amd", "csrc", "eval.hip")).read()
    so = os.path.join(ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    lib = ctypes.CDLL(so)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert hasattr(lib, name), name
    assert len(_lib.lib().pmf_eval_fill.argtypes) == 12
    assert len(_lib.lib().pmf_eval_sweep_finish_fill.argtypes) == 15
    assert src.count("ev_fill_point(") == 3                       # one statement of the rule, called by both kernels


def test_numpy_rule_reproduces_the_reference_fixture():
    g = np.load(F.GOLDEN, allow_pickle=False)
    assert os.path.getsize(F.GOLDEN) < (1 << 16)
    lut = F.label_lut()
    conf = np.zeros((F.NCLASSES, F.NCLASSES), np.int64)
    counts = np.zeros(3, np.int64)
    for i, npts in enumerate(F.COUNTS):
        main, sub, sem = F.sweep_case(i)
        for name, a in (("main", main), ("sub", sub), ("sem", sem)):
            assert a.dtype == np.int32 and a.shape == (npts,) and np.array_equal(g["s%d.%s" % (i, name)], a), (i, name)
        u8, conf, c = F.fill_np(main, sub, sem, lut, base=conf)
        assert u8.dtype == np.uint8 and np.array_equal(u8, g["s%d.fused" % i]), i
        assert c.min() > 0 and c.sum() == npts                      # all three sources in every sweep
        assert (main == 0).mean() >= 0.4
        counts += c
        pred, source = F.fill_rule_np(main, sub)
        assert np.all(pred[source == 2] == F.FILL_CLASS) and np.all(pred != 0)
        assert np.array_equal(pred[source == 0], main[main != 0])
    assert g["conf"].dtype == np.int64 and np.array_equal(conf, g["conf"])
    assert np.array_equal(counts, g["counts"])
    assert conf.sum() == sum(F.COUNTS) and conf[:, 0].sum() > 0 and conf[0].sum() == 0      # gt 0 is counted, pred 0 never occurs


def test_numpy_rule_wraps_and_skips_labels_outside_the_classes():
    main = np.array([0, 300, -3, 5, 0], np.int32)
    sub = np.array([0, 1, 2, 3, 4], np.int32)
    sem = np.array([1, 2, 3, 400, -1], np.int32)
    u8, conf, counts = F.fill_np(main, sub, sem, F.label_lut())
    assert u8.tolist() == [F.FILL_CLASS, 300 - 256, 256 - 3, 5, 4]
    assert counts.tolist() == [3, 1, 1] and conf.sum() == 3         # 300 and -3 are written wrapped, not counted
    assert conf[5, 0] == 1 and conf[4, 0] == 1                      # raw ids outside the table: class 0, counted


def test_wrappers_reject_cpu_tensors_wrong_dtypes_and_shapes():
    from pmf_amd.postproc import SweepEvaluator, fill_labels, sweep_finish_fill
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ValueError):
        fill_labels(i32(8), i32(8), 17)                             # CPU tensors
    with pytest.raises(ValueError):
        sweep_finish_fill(torch.zeros(8), i32(8), i32(8), 17)
    se = SweepEvaluator(17, [0.0] * 5, [1.0] * 5, device="cpu")
    with pytest.raises(RuntimeError):
        se.finish(None, None, 8, fallback=i32(8))                   # no view yet
    se.views_in_sweep, se.n_points = 1, 8
    with pytest.raises(ValueError):
        se.finish(None, None, 8, fallback=i32(8))                   # CPU state / fallback
    if torch.cuda.is_available():                                   # the checks behind the device check need device tensors
        d = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device="cuda")
        for bad in (lambda: fill_labels(d(8), d(7), 17),                                        # length mismatch
                    lambda: fill_labels(d(8), d(8, torch.int64), 17),                           # dtype
                    lambda: fill_labels(d(8, torch.uint8), d(8), 17),
                    lambda: fill_labels(d(8), d(8), 17, conf=torch.zeros(17, 17, dtype=torch.int64, device="cuda")),  # no sem
                    lambda: fill_labels(d(8), d(8), 17, sem=d(7), lut=d(256),
                                        conf=torch.zeros(17, 17, dtype=torch.int64, device="cuda")),
                    lambda: fill_labels(d(8), d(8), 17, conf=torch.zeros(16, 17, dtype=torch.int64, device="cuda"),
                                        sem=d(8), lut=d(256)),
                    lambda: fill_labels(d(8), d(8), 17, counts=d(3)),                           # counts must be int64
                    lambda: fill_labels(d(8), d(8), 17, out_u8=d(9, torch.uint8)),
                    lambda: fill_labels(d(8), d(8), 65),
                    lambda: sweep_finish_fill(d(8, torch.float32), d(8), d(9), 17),
                    lambda: sweep_finish_fill(d(8, torch.float32), d(8), d(8), 17, out_cam_u8=d(8))):
            with pytest.raises(ValueError):
                bad()


def _config(tmp_path, **kw):
    with open(os.path.join(TASK, "config_server.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(kw)
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return cfg, path


def test_option_keys_are_the_references_and_new_keys_default_to_its_behaviour(tmp_path):
    opt, _, _ = load_task()
    with open(os.path.join(TASK, "config_server.yaml")) as f:
        shipped = yaml.safe_load(f)
    reference_keys = {"save_path", "experiment_id", "gpu", "is_debug", "dataset", "data_root", "n_classes", "has_label",
                      "main_pred_folder", "sub_pred_folder"}
    new_keys = {"main_pred_dtype", "sub_pred_dtype", "fill_class", "merge_batch_size"}
    assert set(shipped) == reference_keys | new_keys
    assert (shipped["n_classes"], shipped["has_label"], shipped["is_debug"], shipped["dataset"]) == (17, True, False, "nuScenes")
    main_dir, sub_dir = tmp_path / "main", tmp_path / "sub"
    cfg = {k: v for k, v in shipped.items() if k in reference_keys}          # the reference's own keys only
    cfg.update(save_path=str(tmp_path / "out"), experiment_id="run1", main_pred_folder=str(main_dir),
               sub_pred_folder=str(sub_dir))
    _, path = _config(tmp_path, **cfg)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(FileNotFoundError, match="main prediction folder"):
        opt.Option(path)
    os.makedirs(main_dir)
    with pytest.raises(FileNotFoundError, match="sub prediction folder"):
        opt.Option(path)
    os.makedirs(sub_dir)
    o = opt.Option(path)
    assert o.save_path == os.path.join(str(tmp_path / "out"), "run1")
    assert (o.main_pred_dtype, o.sub_pred_dtype, o.fill_class, o.merge_batch_size) == ("int32", "int32", 11, 8)
    assert (o.n_classes, o.has_label, o.is_debug, o.gpu) == (17, True, False, "0")
    o.check_path()
    o.check_path()                                                        # an existing directory is reused, no prompt
    assert os.path.isdir(o.save_path)
    for key, bad in (("main_pred_dtype", "int64"), ("sub_pred_dtype", "float32"), ("merge_batch_size", 0)):
        with open(path, "w") as f:
            yaml.safe_dump(dict(cfg, **{key: bad}), f)
        with pytest.raises(ValueError, match=key):
            opt.Option(path)


def test_file_reader_dtype_and_length_checks(tmp_path):
    _, main, _ = load_task()
    for folder in ("m", "s"):
        os.makedirs(tmp_path / folder / "preds" / "lidarseg" / "val")
    m, s = str(tmp_path / "m"), str(tmp_path / "s")
    a, b, _ = F.sweep_case(0)
    a.tofile(main.pred_file(m, "val", "tokA"))
    b.tofile(main.pred_file(s, "val", "tokA"))
    ra, rb = main.read_pair(m, s, "val", "tokA")
    assert ra.dtype == rb.dtype == np.int32 and np.array_equal(ra, a) and np.array_equal(rb, b)
    a.astype(np.uint8).tofile(main.pred_file(m, "val", "tokB"))           # an EPMF folder as the main one
    b.tofile(main.pred_file(s, "val", "tokB"))
    ra, rb = main.read_pair(m, s, "val", "tokB", main_dtype="uint8")
    assert ra.dtype == np.int32 and np.array_equal(ra, a) and np.array_equal(rb, b)
    with pytest.raises(ValueError, match="tokB"):                         # uint8 bytes read as int32: a quarter of the points
        main.read_pair(m, s, "val", "tokB")
    with pytest.raises(FileNotFoundError, match="tokC"):
        main.read_pair(m, s, "val", "tokC")
    a.tofile(main.pred_file(m, "val", "tokC"))
    with pytest.raises(FileNotFoundError, match="tokC"):                  # the sub file is still missing
        main.read_pair(m, s, "val", "tokC")
    b[:-5].tofile(main.pred_file(s, "val", "tokC"))
    with pytest.raises(ValueError, match="tokC"):
        main.read_pair(m, s, "val", "tokC")
    a.astype(np.uint8)[:-1].tofile(main.pred_file(m, "val", "tokD"))      # not a whole number of int32 labels
    with pytest.raises(ValueError, match="tokD"):
        main.read_pred(main.pred_file(m, "val", "tokD"), "int32", "tokD")
    with pytest.raises(ValueError, match="dtype"):
        main.read_pred(main.pred_file(m, "val", "tokA"), "int64", "tokA")
    assert np.array_equal(main.label_lut(F.SyntheticNusSweeps()), F.label_lut())
    ds = F.SyntheticNusSweeps()
    raw = ds.loadLabelByIndex(1)
    assert raw.dtype == np.uint8 and raw.shape == (ds.counts[1], 1)
    assert np.array_equal(ds.labelMapping(raw), F.label_lut()[raw[:, 0]])


def _good_tree(root, ds, split="val"):
    """a valid submission tree for the dataset: the numpy rule's labels, submission.json as main.py writes it"""
    _, main, _ = load_task()
    seg = os.path.join(root, "lidarseg", split)
    os.makedirs(seg)
    os.makedirs(os.path.join(root, split))
    for i, token in enumerate(ds.token_list):
        m, s = ds.main_sub(i)
        F.fill_rule_np(m, s)[0].astype(np.uint8).tofile(os.path.join(seg, "%s_lidarseg.bin" % token))
    with open(os.path.join(root, split, "submission.json"), "w") as f:
        json.dump({"meta": dict(main.SUBMISSION_META)}, f)
    return seg


def test_devkit_free_validator_accepts_a_good_folder_and_names_each_fault(tmp_path):
    _, _, chk = load_task()
    ds = F.SyntheticNusSweeps()
    counts = chk.dataset_point_counts(ds)
    assert counts == dict(zip(ds.token_list, ds.counts))
    root = str(tmp_path / "preds")
    seg = _good_tree(root, ds)
    assert chk.check_submission(root, "val", counts, F.NCLASSES) == []
    path = lambda i: os.path.join(seg, "%s_lidarseg.bin" % ds.token_list[i])
    good = [np.fromfile(path(i), dtype=np.uint8) for i in range(len(ds))]

    def one_fault(token, word):
        faults = chk.check_submission(root, "val", counts, F.NCLASSES)
        assert len(faults) == 1 and token in faults[0] and word in faults[0], faults

    good[0][:-1].tofile(path(0))                                          # a short file
    one_fault("sweep000", "bytes")
    good[0].tofile(path(0))
    bad = good[1].copy()
    bad[7] = 0
    bad.tofile(path(1))                                                   # a label 0
    one_fault("sweep001", "labelled 0")
    bad[7] = F.NCLASSES
    bad.tofile(path(1))                                                   # a label >= n_classes
    one_fault("sweep001", ">= n_classes")
    good[1].tofile(path(1))
    os.rename(path(2), path(2) + ".away")                                 # a missing token (and a file of no token)
    faults = chk.check_submission(root, "val", counts, F.NCLASSES)
    assert len(faults) == 2 and "sweep002" in faults[0] and "no file" in faults[0] and "no token" in faults[1], faults
    os.rename(path(2) + ".away", path(2))
    meta = os.path.join(root, "val", "submission.json")
    with open(meta, "w") as f:
        json.dump({"meta": {"use_camera": True, "use_lidar": 1, "use_radar": False, "use_map": False}}, f)
    faults = chk.check_submission(root, "val", counts, F.NCLASSES)
    assert len(faults) == 2 and "use_lidar" in faults[0] and "use_external" in faults[1], faults
    os.remove(meta)
    one_fault("submission.json", "missing")
