"""Full SemanticKITTI sweeps, host side (no GPU): the seventh header's binding and argument guards, fov_fill's host checks, the
options of the two new tasks and check_valid.py on folders written by the numpy restatement (kitti_full_cases)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import yaml

import fov_cases as F
import kitti_full_cases as K

SALSA_TASK = os.path.join(F.ROOT, "tasks", "salsanext_eval_semantickitti")
FULL_TASK = os.path.join(F.ROOT, "tasks", "pmf_eval_semantickitti", "fullsweep_eval")


def _load(name, path, option=None):
    """a task module loaded by path; `option` stands in for the bare name the tasks import"""
    saved = sys.modules.get("option")
    if option is not None:
        sys.modules["option"] = option
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            sys.modules.pop("option", None)
        else:
            sys.modules["option"] = saved
    return mod


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_seventh_header_binding_and_built_symbol():
    from pmf_amd import _lib
    assert _lib.EXPORTS_FULL == ["pmf_kitti_full_fill"]
    assert os.path.samefile(_lib.FULL_HEADER_PATH, os.path.join(F.ROOT, "include", "pmf_amd_full.h"))
    assert (_lib.FULL_WS_PER_BLOCK, _lib.FULL_WS_FIXED) == (1 + 2 * (_lib.FOV_BLOCK // 64), _lib.FOV_MAX_FRAMES + 2)
    assert not set(_lib.EXPORTS_FULL) & set(_lib.EXPORTS + _lib.EXPORTS_SENSAT + _lib.EXPORTS_WIDE + _lib.EXPORTS_A2D2
                                            + _lib.EXPORTS_NUS + _lib.EXPORTS_FOV)
    so = os.path.join(F.ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    assert hasattr(C.CDLL(so), "pmf_kitti_full_fill")
    lib = _lib.lib()
    V, I, Q, U = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    assert lib.pmf_kitti_full_fill.argtypes == [V, V, V, I, Q, V, V, V, Q, V, V, V, I, U, I, V, V, V, V, V, V, V]
    assert lib.pmf_kitti_full_fill.restype is C.c_int32


def test_build_and_lib_check_the_seventh_list(monkeypatch):
    import __graft_entry__ as g
    from pmf_amd import _lib
    assert _lib.lib() is not None
    monkeypatch.setattr(g.subprocess, "run", lambda *a, **kw: None)
    g.build()
    monkeypatch.setattr(_lib, "EXPORTS_FULL", _lib.EXPORTS_FULL + ["pmf_full_not_there"])
    with pytest.raises(RuntimeError, match="pmf_full_not_there"):
        g.build()
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.PMFLibraryError, match=r"pmf_full_not_there, which include/pmf_amd_full\.h declares"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib() is not None


def test_every_argument_guard_answers_before_a_launch():
    """the guards look at the pointers' values only: plausible numbers stand in for device memory"""
    from pmf_amd import _lib
    p = 4096
    names = ("points", "offsets", "dims", "B", "P", "proj", "main", "main_off", "K", "sub", "gt", "lut", "nlut", "fill", "C",
             "out", "keep", "kept", "counts", "conf", "ws")

    def call(**kw):
        a = dict(points=p, offsets=p, dims=p, B=2, P=100, proj=p, main=p, main_off=p, K=50, sub=p, gt=p, lut=p, nlut=300,
                 fill=40, C=20, out=p, keep=p, kept=p, counts=p, conf=p, ws=p)
        a.update(kw)
        return _lib.lib().pmf_kitti_full_fill(*[a[n] for n in names], None)
    E = _lib.PMF_E_ARG
    for name in ("points", "offsets", "dims", "proj", "main", "main_off", "sub", "lut", "out", "kept", "ws"):
        assert call(**{name: None}) == E, name
    assert call(gt=None) == E                               # conf without gt
    for kw in (dict(B=0), dict(B=-1), dict(B=_lib.FOV_MAX_FRAMES + 1), dict(P=0), dict(P=-1), dict(K=-1), dict(C=0),
               dict(C=65), dict(C=-4), dict(nlut=0), dict(nlut=-7)):
        assert call(**kw) == E, kw
    for off in (4, 8, 12, 1):
        assert call(points=p + off) == E
    assert call(P=2 ** 31) == _lib.PMF_E_UNSUPPORTED and call(P=2 ** 40) == _lib.PMF_E_UNSUPPORTED
    assert call(P=2 ** 31, out=None) == E


# ---- fov_fill's host checks -----------------------------------------------------------------------------------------------
def _args(sizes=(5, 0, 7), seed=1):
    frames, dims, main, sub, gt = K.random_case(sizes, seed)
    return frames, dims, main, sub, gt


def test_fov_fill_checks_its_tables_before_any_device_use(monkeypatch):
    """every one of these raises ValueError with or without a GPU: the device is never asked for"""
    import torch
    from pmf_amd.postproc import fov_fill
    from pmf_amd.dataset import perspective_view_loader as pvl
    monkeypatch.setattr(pvl, "upload_packed", lambda *a, **kw: pytest.fail("an upload before the host checks"))
    frames, dims, main, sub, gt = _args()
    pts, ids = np.concatenate(frames), np.concatenate(main)
    P, Kt = pts.shape[0], ids.shape[0]
    good_off = np.array([0, 5, 5, 12], np.int64)
    main_off = np.concatenate([[0], np.cumsum([len(m) for m in main])]).astype(np.int64)
    call = lambda fr, mn, **kw: fov_fill(fr, dims, F.EXACT_PROJ, mn, kw.pop("sub", sub), K.LUT, K.FILL_ID, K.NCLS, **kw)
    with pytest.raises(ValueError, match=r"offsets of frames decreases at frame 1 \(7 -> 5\)"):
        call((pts, np.array([0, 7, 5, 12], np.int64)), main)
    with pytest.raises(ValueError, match=r"offsets of frames\[3\] is 11 but the array it describes holds 12"):
        call((pts, np.array([0, 5, 5, 11], np.int64)), main)
    with pytest.raises(ValueError, match=r"offsets of frames\[0\] is 1, not 0"):
        call((pts, np.array([1, 5, 5, 12], np.int64)), main)
    bad = main_off.copy()
    bad[1], bad[2] = main_off[2] + 1, main_off[1]
    with pytest.raises(ValueError, match="offsets of main decreases at frame 1"):
        call((pts, good_off), (ids, bad))
    with pytest.raises(ValueError, match=r"offsets of main\[3\] is %d but the array it describes holds %d" % (Kt + 2, Kt)):
        call(frames, (ids, main_off + np.array([0, 0, 0, 2])))
    with pytest.raises(ValueError, match="frame 2 has 7 points but 6 words in sub"):
        call(frames, main, sub=[sub[0], sub[1], sub[2][:6]])
    from pmf_amd import _lib
    n = _lib.FOV_MAX_FRAMES + 1
    one = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError, match="65 frames, a batch holds 1 to 64"):
        fov_fill([one] * n, [(4, 4)] * n, F.EXACT_PROJ, [np.zeros(0, np.uint32)] * n, [np.zeros(2, np.uint32)] * n, K.LUT,
                 K.FILL_ID, K.NCLS)
    with pytest.raises(ValueError, match="0 frames"):
        fov_fill([], [], F.EXACT_PROJ, [], [], K.LUT, K.FILL_ID, K.NCLS)
    with pytest.raises(ValueError, match="a confusion matrix needs gt"):
        call(frames, main, conf=torch.zeros((K.NCLS, K.NCLS), dtype=torch.int64))
    with pytest.raises(ValueError, match="nclasses must be in 1..64"):
        fov_fill(frames, dims, F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, 65)
    with pytest.raises(ValueError, match="frames of frame 0 must be a float32 array"):
        call([frames[0].astype(np.float64)] + frames[1:], main)
    with pytest.raises(ValueError, match="3 x 4"):
        fov_fill(frames, dims, np.eye(4), main, sub, K.LUT, K.FILL_ID, K.NCLS)
    # a tuple of two per-frame arrays is two frames, not (array, offsets): it gets as far as the device question
    two = (frames[0], frames[2])
    with pytest.raises(RuntimeError, match="GPU only"):
        fov_fill(two, dims[:2], F.EXACT_PROJ, (main[0], main[2]), (sub[0], sub[2]), K.LUT, K.FILL_ID, K.NCLS, device="cpu")
    with pytest.raises(ValueError, match="frames of frame 1 must be a float32 array"):
        fov_fill((pts, [0, 5, 5, 12]), dims[:2], F.EXACT_PROJ, main[:2], sub[:2], K.LUT, K.FILL_ID, K.NCLS)


def test_fov_fill_has_no_host_path_and_is_exported():
    import pc_processor
    from pmf_amd.postproc import fov_fill
    assert pc_processor.postproc.fov_fill is fov_fill
    frames, dims, main, sub, gt = _args()
    with pytest.raises(RuntimeError, match="GPU only"):
        fov_fill(frames, dims, F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, K.NCLS, device="cpu")


def test_restatement_states_the_rule_on_a_hand_made_frame():
    """five rows under EXACT_PROJ and a 4 x 4 image: kept, behind, kept, outside, kept; two main words for three kept rows"""
    pts = np.array([[1, 1, 1, 0], [-1, 1, 1, 0], [1, 2, 2, 0], [1, 5, 1, 0], [1, 3, 3, 0]], np.float32)
    main = [np.array([0xABCD0000 | 10, 1], np.uint32)]              # class 1 with a high half; id 1 is class 0
    sub = [np.array([40, 0x00070000 | 252, 0, 5000, 257], np.uint32)]
    gt = [np.array([10, 252, 0x12340000 | 259, 300, 257], np.uint32)]
    w = K.numpy_fill([pts], [(4, 4)], F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, K.NCLS, gt)
    assert w["keep"][0].tolist() == [True, False, True, False, True] and w["kept_count"].tolist() == [3]
    # row 0: main 10; row 1: unkept -> sub 252; row 2: main id 1 is class 0, sub 0 -> fill; row 3: sub 5000 is beyond the table
    # -> fill; row 4: the third kept row has no main word -> sub 257
    assert w["out"][0].tolist() == [10, 252, K.FILL_ID, K.FILL_ID, 257]
    assert w["source"][0].tolist() == [0, 1, 2, 2, 1] and w["counts"].tolist() == [1, 2, 2]
    want = np.zeros((K.NCLS, K.NCLS), np.int64)
    for p, t in ((1, 1), (3, 3), (2, 5), (2, 0), (4, 4)):           # conf[class of pred][class of gt]
        want[p, t] += 1
    assert np.array_equal(w["conf"], want)


# ---- the options of the two tasks ------------------------------------------------------------------------------------------
def test_both_options_load_their_configs(tmp_path):
    opt = _load("kitti_salsa_option", os.path.join(SALSA_TASK, "option.py"))
    s = opt.Option(os.path.join(SALSA_TASK, "config_server_kitti.yaml"))
    assert (s.dataset, s.n_classes, s.eval_batch_size, s.sequences, s.has_label) == ("SemanticKitti", 20, 4, [8], True)
    assert os.path.basename(s.save_path) == "Eval-SV_SemanticKitti_SalsaNext__eval"
    assert s.config["sensor"]["proj_h"] == 64 and s.config["post"]["KNN"]["use"] is False
    with open(os.path.join(FULL_TASK, "config_server.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) >= {"data_root", "main_pred_folder", "sub_pred_folder", "sequences", "has_label", "merge_batch_size",
                        "fill_class", "save_path"}
    opt = _load("kitti_full_option", os.path.join(FULL_TASK, "option.py"))
    with pytest.raises(FileNotFoundError, match="main_pred_folder not found"):
        opt.Option(os.path.join(FULL_TASK, "config_server.yaml"))
    for key in ("main_pred_folder", "sub_pred_folder"):
        os.makedirs(str(tmp_path / key))
        cfg[key] = str(tmp_path / key)
    path = str(tmp_path / "full.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = opt.Option(path)
    assert (s.merge_batch_size, s.fill_class, s.n_classes, s.sequences, s.has_label) == (16, 9, 20, [8], True)
    for key in ("merge_batch_size", "fill_class"):
        cfg.pop(key)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = opt.Option(path)
    assert (s.merge_batch_size, s.fill_class) == (16, 9)
    for bad, what in ((dict(merge_batch_size=65), "merge_batch_size"), (dict(merge_batch_size=0), "merge_batch_size"),
                      (dict(fill_class=0), "fill_class"), (dict(fill_class=20), "fill_class")):
        with open(path, "w") as f:
            yaml.safe_dump(dict(cfg, **bad), f)
        with pytest.raises(ValueError, match=what):
            opt.Option(path)


def test_fill_class_nine_is_road_in_the_packaged_label_file():
    from pmf_amd.dataset.semantic_kitti.parser import DEFAULT_CONFIG, label_tables
    with open(DEFAULT_CONFIG) as f:
        cfg = label_tables(yaml.safe_load(f))
    assert cfg["mapped_class_name"][9] == "road" and cfg["learning_map_inv"][9] == 40


def test_write_prediction_original_ids_and_loader_table(tmp_path):
    """original_ids writes the words as they are, the default still maps learning ids; SalsaNextLoader keeps its 256-entry
    table unless it is handed one"""
    from oracle.cases import kitti_tree
    from pmf_amd.dataset import SalsaNextLoader
    from pmf_amd.dataset.semantic_kitti import SemanticKitti, write_prediction
    root = str(tmp_path / "sequences")
    cfg_path, data = kitti_tree(root, seed=2, seqs=(8,), frames=1, npts=50)
    ds = SemanticKitti(root, [8], cfg_path, has_image=False)
    ids = np.array([0, 259, 13, 30] * 3, np.uint32)
    p = write_prediction(ds, 0, ids, str(tmp_path / "a"), original_ids=True)
    assert p == str(tmp_path / "a" / "sequences" / "08" / "predictions" / "000000.label")
    assert np.array_equal(np.fromfile(p, dtype=np.int32), ids.astype(np.int32))
    cls = np.array([0, 1, 2, 5], np.int32)
    q = write_prediction(ds, 0, cls, str(tmp_path / "b"))
    assert np.array_equal(np.fromfile(q, dtype=np.int32), ds.class_map_lut_inv[cls])
    sensor = dict(fov_up=3.0, fov_down=-25.0, fov_left=-180, fov_right=180, proj_h=16, proj_w=128, img_mean=[0.0] * 5,
                  img_stds=[1.0] * 5)
    assert ds.class_map_lut.shape[0] > 259 and ds.class_map_lut[259] != 0
    whole = SalsaNextLoader(ds, {"sensor": sensor}, is_train=False, device="cpu", label_lut=ds.class_map_lut)._label_lut()
    cut = SalsaNextLoader(ds, {"sensor": sensor}, is_train=False, device="cpu")._label_lut()
    assert tuple(whole.shape) == ds.class_map_lut.shape and np.array_equal(whole.numpy(), ds.class_map_lut)
    assert tuple(cut.shape) == (256,) and np.array_equal(cut.numpy(), ds.class_map_lut[:256])


# ---- check_valid.py ------------------------------------------------------------------------------------------------------
def test_check_valid_accepts_a_good_folder_and_names_the_frame(tmp_path):
    from oracle.cases import kitti_tree
    root = str(tmp_path / "sequences")
    cfg_path, data = kitti_tree(root, seed=4, seqs=(0, 8), frames=3, npts=200)
    opt = _load("kitti_full_option", os.path.join(FULL_TASK, "option.py"))
    chk = _load("kitti_full_check_valid", os.path.join(FULL_TASK, "check_valid.py"), opt)
    ids = chk.allowed_ids(cfg_path)
    with open(cfg_path) as f:
        assert ids == sorted(set(yaml.safe_load(f)["learning_map_inv"].values()))
    rng = np.random.Generator(np.random.PCG64(0))
    out = str(tmp_path / "out")
    for (seq, frame), (pts, raw, img) in data.items():
        d = os.path.join(out, "sequences", seq, "predictions")
        os.makedirs(d, exist_ok=True)
        rng.choice(ids, pts.shape[0]).astype(np.int32).tofile(os.path.join(d, frame + ".label"))
    assert chk.check_submission(out, root, [0, 8], ids) == []
    for key in ("main", "sub"):
        os.makedirs(str(tmp_path / key))
    conf = str(tmp_path / "c.yaml")
    with open(conf, "w") as f:
        yaml.safe_dump(dict(save_path=out, data_root=root, main_pred_folder=str(tmp_path / "main"),
                            sub_pred_folder=str(tmp_path / "sub"), sequences=[0, 8], has_label=True,
                            data_config_path=cfg_path), f)
    chk.Experiment(opt.Option(conf)).run()
    pred = lambda seq, frame: os.path.join(out, "sequences", seq, "predictions", frame + ".label")
    os.remove(pred("00", "000001"))
    np.fromfile(pred("08", "000000"), np.int32)[:-1].tofile(pred("08", "000000"))
    lab = np.fromfile(pred("08", "000002"), np.int32)
    lab[5] = 31                                                     # an id learning_map_inv never gives
    lab[9] |= 1 << 16                                               # a high half
    lab.tofile(pred("08", "000002"))
    np.zeros(3, np.int32).tofile(pred("08", "000007"))
    faults = chk.check_submission(out, root, [0, 8], ids)
    assert len(faults) == 4
    assert "sequence 00 frame 000001: no file" in faults[0]
    assert "sequence 08 frame 000000: %d bytes for a sweep of 200 points" % (4 * 199) in faults[1]
    assert "sequence 08 frame 000002: 2 points carry an id outside learning_map_inv, the first: 31" in faults[2]
    assert "sequence 08: file 000007.label belongs to no sweep" in faults[3]
    with pytest.raises(ValueError, match="4 faults, the first: sequence 00 frame 000001"):
        chk.Experiment(opt.Option(conf)).run()
