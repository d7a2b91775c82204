"""The devkit-free nuScenes reader, host side (no GPU): the fifth header's binding and guards, the tables and their reverse
index, the split logic, the label table, the raw loaders, image sizes, the quaternion matrix, the chain's layout, the
properties of the test tree (so that the GPU tests cannot pass vacuously) and the call sites of the factory."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import nus_tables_cases as N

ROOT = N.ROOT


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("nus") / "tree")
    return dict(root=root, truth=N.write_tree(root))


def _open(v2, root, version="v1.0-mini", split="train", **kw):
    from pmf_amd.dataset.nuScenes import open_nuscenes
    return open_nuscenes(v2, root, version, split, **kw)


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_fifth_header_binding():
    from pmf_amd import _lib
    assert _lib.EXPORTS_NUS == ["pmf_nus_project"]
    assert (_lib.NUS_BLOCK, _lib.NUS_CHAIN, _lib.NUS_IMAGE, _lib.NUS_YAW) == (256, 57, 0, 1)
    assert not set(_lib.EXPORTS_NUS) & set(_lib.EXPORTS + _lib.EXPORTS_SENSAT + _lib.EXPORTS_WIDE + _lib.EXPORTS_A2D2)
    lib = _lib.lib()
    V, I, D, F = C.c_void_p, C.c_int32, C.c_double, C.c_float
    assert lib.pmf_nus_project.argtypes == [V, I, I, V, I, D, F, F, D, D, D, D, D, V, V, V, V, V, V, V, V, V, V]
    assert lib.pmf_nus_project.restype is C.c_int32


def test_build_refuses_a_library_without_the_new_symbol(monkeypatch):
    """build() itself checks the fifth list: with the compile step stubbed out and a name the library lacks, it raises"""
    import __graft_entry__ as g
    from pmf_amd import _lib
    assert _lib.lib() is not None                               # loaded: lib() answers from its cache below
    ran = []
    monkeypatch.setattr(g.subprocess, "run", lambda *a, **kw: ran.append(a))
    g.build()
    assert len(ran) == 1
    monkeypatch.setattr(_lib, "EXPORTS_NUS", _lib.EXPORTS_NUS + ["pmf_nus_not_there"])
    with pytest.raises(RuntimeError, match="pmf_nus_not_there"):
        g.build()


def test_missing_symbol_names_the_header(monkeypatch):
    from pmf_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXPORTS_NUS", _lib.EXPORTS_NUS + ["pmf_nus_not_there"])
    with pytest.raises(_lib.PMFLibraryError, match=r"pmf_nus_not_there, which include/pmf_amd_nus\.h declares"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib() is not None


def _call(**kw):
    """pmf_nus_project with plausible arguments, one of them replaced; the pointers are never dereferenced by a guard"""
    from pmf_amd import _lib
    chain = np.zeros(57, np.float64)
    p = 4096
    a = dict(points=p, P=8, stride=5, chain=chain.ctypes.data, mode=1, min_dist=0.1, lo=-1.0, hi=1.0, bh=160.0, bw=90.0,
             rs=1.0, cs=1.0, sc=1.0, keep=p, src=p, crop=p, xy=p, xd=p, yd=p, depth=p, meta=p, blk=p)
    a.update(kw)
    return _lib.lib().pmf_nus_project(a["points"], a["P"], a["stride"], a["chain"], a["mode"], a["min_dist"], a["lo"],
                                      a["hi"], a["bh"], a["bw"], a["rs"], a["cs"], a["sc"], a["keep"], a["src"], a["crop"],
                                      a["xy"], a["xd"], a["yd"], a["depth"], a["meta"], a["blk"], None)


def test_every_argument_guard_answers_before_a_launch():
    from pmf_amd import _lib
    E = _lib.PMF_E_ARG
    for name in ("points", "chain", "keep", "src", "crop", "xy", "xd", "yd", "depth", "meta", "blk"):
        assert _call(**{name: 0}) == E, name
    assert _call(P=0) == E and _call(P=-3) == E
    for stride in (0, 3, 6, -4):
        assert _call(stride=stride) == E
    assert _call(mode=2) == E and _call(mode=-1) == E
    for name in ("rs", "cs", "sc"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert _call(**{name: bad}) == E, (name, bad)


# ---- quaternions ------------------------------------------------------------------------------------------------------
def test_quaternion_matrix():
    from pmf_amd.dataset.nuScenes import quaternion_rotation_matrix as R
    s = math.sqrt(0.5)
    assert np.array_equal(R(1, 0, 0, 0), np.eye(3)) and R(1, 0, 0, 0).dtype == np.float64
    turns = {(s, s, 0, 0): [[1, 0, 0], [0, 0, -1], [0, 1, 0]],          # a quarter turn about x: y -> z
             (s, 0, s, 0): [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],          # about y: z -> x
             (s, 0, 0, s): [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}          # about z: x -> y
    for q, want in turns.items():
        assert np.abs(R(*q) - np.array(want, np.float64)).max() <= 4 * np.finfo(np.float64).eps, q
    for q in ((2.0, 0.0, 0.0, 2.0), (1.0, 2.0, 3.0, 4.0), (0.3, -1.7, 2.2, 0.9)):
        m = R(*q)
        n = math.sqrt(sum(v * v for v in q))
        assert np.abs(m.T @ m - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(m) - 1.0) <= 1e-15
        assert np.abs(m - R(*(v / n for v in q))).max() <= 4 * np.finfo(np.float64).eps      # normalised first
    assert np.abs(R(2.0, 0.0, 0.0, 2.0) - np.array(turns[(s, 0, 0, s)], np.float64)).max() <= 4 * np.finfo(np.float64).eps
    with pytest.raises(ValueError):
        R(0, 0, 0, 0)
    # the camera convention of the test tree: the optical axis (camera z) is the ego's x, camera x its -y, camera y its -z
    assert np.abs(R(*N.Q_CAM) - np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)).max() <= 1e-15


# ---- tables -----------------------------------------------------------------------------------------------------------
def test_tables_and_reverse_index(tree):
    from pmf_amd.dataset.nuScenes import NuTables
    t = NuTables(tree["root"], "v1.0-mini")
    assert len(t.scene) == 2 and len(t.sample) == 4 and len(t.sample_data) == 4 * (1 + 2 * 6)
    assert t.get("scene", "scene_1")["name"] == "scene-0103"
    for s in t.sample:
        assert sorted(s["data"]) == sorted(("LIDAR_TOP",) + N.CHANNELS)
        for ch, tok in s["data"].items():
            sd = t.get("sample_data", tok)
            assert sd["is_key_frame"] and sd["channel"] == ch and sd["sample_token"] == s["token"]
            assert sd["sensor_modality"] == ("lidar" if ch == "LIDAR_TOP" else "camera")
    assert t.get("sample_data", "sd_0_0_CAM_BACK_sweep")["is_key_frame"] is False
    assert t.lidarseg_idx2name_mapping == dict(enumerate(N.CATEGORIES))
    assert t.get("lidarseg", "sd_1_1_LIDAR_TOP")["filename"].endswith("sd_1_1_LIDAR_TOP_lidarseg.bin")
    with pytest.raises(KeyError):
        t.get("sample", "nope")
    with pytest.raises(KeyError, match="no table"):
        t.get("attribute", "x")
    with pytest.raises(FileNotFoundError):
        NuTables(tree["root"], "v1.0-trainval")


def test_category_without_index_names_the_lidarseg_tables(tmp_path):
    N.write_tree(str(tmp_path), samples=1, npts=50, category_index=False)
    with pytest.raises(ValueError, match="nuScenes-lidarseg"):
        _open(False, str(tmp_path))


def test_label_table_from_the_category_indices(tree):
    for v2 in (False, True):
        ds = _open(v2, tree["root"])
        assert ds.map_name_from_general_index_to_segmentation_index == dict(enumerate(N.CLASS_OF_INDEX))
        assert ds.mapped_cls_name[0] == "ignore" and ds.mapped_cls_name[16] == "vegetation" and len(ds.mapped_cls_name) == 17
        raw = np.arange(32, dtype=np.uint8)[:, None]
        assert np.array_equal(ds.labelMapping(raw), np.array(N.CLASS_OF_INDEX))
        assert ds.fov_angle["CAM_BACK"] == {"fov_left": -50, "fov_right": 50} and len(ds.fov_angle) == 6


def test_token_lists(tree):
    pairs = lambda s, k: [("sd_%d_%d_LIDAR_TOP" % (s, k), "sd_%d_%d_%s" % (s, k, ch), ch) for ch in N.CHANNELS]
    tr, va = _open(True, tree["root"], split="train"), _open(True, tree["root"], split="val")
    assert [(t["lidar_token"], t["cam_token"], t["cam_channel"]) for t in tr.token_list] == pairs(0, 0) + pairs(0, 1)
    assert [(t["lidar_token"], t["cam_token"], t["cam_channel"]) for t in va.token_list] == pairs(1, 0) + pairs(1, 1)
    assert all(t["description"] == "scene 0 of the test tree" for t in tr.token_list)
    assert len(tr) == 12 and tr.split == "train" and tr.parsePathInfoByIndex(7) == (7, '')
    assert _open(True, tree["root"], split="train", has_image=False).token_list == ["sd_0_0_LIDAR_TOP", "sd_0_1_LIDAR_TOP"]
    v1 = _open(False, tree["root"], split="val")
    assert v1.token_list == [dict(lidar_token=a, cam_token=b) for a, b, _ in pairs(1, 0) + pairs(1, 1)]
    assert _open(False, tree["root"], split="test", has_image=False).token_list == ["sd_0_0_LIDAR_TOP", "sd_0_1_LIDAR_TOP"]
    with pytest.raises(ValueError, match="invalid split"):
        _open(False, tree["root"], split="trainval")


def test_split_logic_of_the_three_versions(tmp_path):
    names = ("scene-0001", "scene-0002", "scene-0003")
    lists = str(tmp_path / "splits.json")
    with open(lists, "w") as f:
        json.dump({"train": ["scene-0001", "scene-0003", "scene-0900"], "val": ["scene-0002"], "test": ["scene-0002"],
                   "mini_train": ["scene-0002"], "mini_val": []}, f)
    first = lambda ds: [t if isinstance(t, str) else t["lidar_token"] for t in ds.token_list]
    for version in ("v1.0-trainval", "v1.0-test", "v1.0-mini"):
        root = str(tmp_path / version)
        N.write_tree(root, version=version, scene_names=names, samples=1, npts=40, labels=version != "v1.0-test")
        key = {"v1.0-trainval": "train", "v1.0-test": "test", "v1.0-mini": "mini_train"}[version]
        member = [n in json.load(open(lists))[key] for n in names]
        for v2 in (False, True):
            kw = dict(has_image=False, splits_path=lists)
            want = lambda flag: ["sd_%d_0_LIDAR_TOP" % i for i in range(3) if member[i] == flag]
            assert first(_open(v2, root, version, "train", **kw)) == want(True)
            assert first(_open(v2, root, version, "test", **kw)) == want(True)
            assert first(_open(v2, root, version, "val", **kw)) == want(False)
    # without a file: the test set needs none (every scene is a test scene), the mini names ship with the package (the tree's
    # names are not among them: all go to val), trainval has to be told
    for v2 in (False, True):
        assert len(_open(v2, str(tmp_path / "v1.0-test"), "v1.0-test", "test", has_image=False)) == 3
        assert len(_open(v2, str(tmp_path / "v1.0-test"), "v1.0-test", "val", has_image=False)) == 0
        assert len(_open(v2, str(tmp_path / "v1.0-mini"), "v1.0-mini", "val", has_image=False)) == 3
        with pytest.raises(ValueError, match="splits_path"):
            _open(v2, str(tmp_path / "v1.0-trainval"), "v1.0-trainval", "train", has_image=False)
    with open(lists, "w") as f:
        json.dump({"val": []}, f)
    # a file without a `test` list still serves the test set: the evaluation tasks pass one nus_splits for both runs
    for v2 in (False, True):
        assert len(_open(v2, str(tmp_path / "v1.0-test"), "v1.0-test", "test", has_image=False, splits_path=lists)) == 3
    with pytest.raises(ValueError, match="no `train` list"):
        _open(True, str(tmp_path / "v1.0-trainval"), "v1.0-trainval", "train", splits_path=lists)


def test_shipped_mini_lists():
    from pmf_amd.dataset.nuScenes import tables
    with open(tables.MINI_SPLITS_PATH) as f:
        lists = json.load(f)
    assert sorted(lists) == ["mini_train", "mini_val"] and lists["mini_val"] == ["scene-0103", "scene-0916"]
    assert len(lists["mini_train"]) == 8 and not set(lists["mini_train"]) & set(lists["mini_val"])
    assert all(re.fullmatch(r"scene-\d{4}", n) for n in lists["mini_train"] + lists["mini_val"])


def test_raw_loaders_and_test_split(tree, tmp_path):
    ds = _open(True, tree["root"], split="val")
    truth = tree["truth"]["sd_1_0_LIDAR_TOP"]
    pc, sem, inst = ds.loadDataByIndex(4)                      # CAM_BACK_LEFT of the first validation sample
    assert pc.dtype == np.float32 and pc.shape == (len(truth["points"]), 4) and np.array_equal(pc, truth["points"][:, :4])
    assert sem.dtype == np.uint8 and sem.shape == (len(pc), 1) and np.array_equal(sem[:, 0], truth["labels"])
    assert inst.dtype == np.int32 and inst.shape == (len(pc),) and not inst.any()
    assert np.array_equal(ds.loadLabelByIndex(4), sem) and np.array_equal(ds.loadPointcloud(4), pc)
    v1 = _open(False, tree["root"], split="val", has_image=False)
    assert np.array_equal(v1.loadDataByIndex(0)[0], pc) and np.array_equal(v1.loadDataByIndex(0)[1], sem)
    root = str(tmp_path / "test")
    t = N.write_tree(root, version="v1.0-test", samples=1, npts=60, labels=False)
    for v2 in (False, True):
        te = _open(v2, root, "v1.0-test", "test")
        pc, sem, inst = te.loadDataByIndex(0)
        assert np.array_equal(pc, t["sd_0_0_LIDAR_TOP"]["points"][:, :4])
        assert sem.shape == (len(pc), 1) and sem.dtype == np.zeros(1, int).dtype and not sem.any()
        assert te.loadLabelByIndex(0) is None


def test_image_sizes(tree):
    from PIL import Image
    v1, v2 = _open(False, tree["root"]), _open(True, tree["root"])
    for i, ch in enumerate(N.CHANNELS):
        raw = Image.open(os.path.join(tree["root"], "samples", ch, "s0_k0.png"))
        assert np.array_equal(np.asarray(v1.loadImage(i)), np.asarray(raw)) and raw.size == (N.W, N.H)
        got = v2.loadImage(i)
        if ch == "CAM_BACK":
            assert np.array_equal(np.asarray(got), np.asarray(raw))
        else:
            assert got.size == (int(N.W * 0.6), int(N.H * 0.5))
            assert np.array_equal(np.asarray(got), np.asarray(raw.resize((int(N.W * 0.6), int(N.H * 0.5)), Image.BILINEAR)))


def test_missing_first_sweep_v1_skips_v2_raises(tmp_path):
    root = str(tmp_path)
    N.write_tree(root, scene_names=("scene-0061", "scene-0553", "scene-0103"), samples=1, npts=40)
    os.remove(os.path.join(root, "samples", "LIDAR_TOP", "s1_k0.pcd.bin"))
    assert _open(False, root, split="train", has_image=False).token_list == ["sd_0_0_LIDAR_TOP"]
    # as in the reference, whatever is not a present training scene lands in the other list
    assert _open(False, root, split="val", has_image=False).token_list == ["sd_1_0_LIDAR_TOP", "sd_2_0_LIDAR_TOP"]
    with pytest.raises(FileNotFoundError, match="s1_k0.pcd.bin"):
        _open(True, root, split="train")


def test_chain_layout(tree):
    from pmf_amd.dataset.nuScenes import quaternion_rotation_matrix as R
    ds = _open(True, tree["root"], split="val")
    t = ds.nusc
    for i in (0, 3, 11):
        pair = ds.token_list[i]
        c = ds._chain(i)
        assert c.dtype == np.float64 and c.shape == (57,) and c.flags.c_contiguous and ds._chain(i) is c      # built once
        assert np.array_equal(c, tree["truth"][pair["lidar_token"]]["chains"][pair["cam_channel"]])
        lidar, cam = t.get("sample_data", pair["lidar_token"]), t.get("sample_data", pair["cam_token"])
        cs_c, pose_c = t.get("calibrated_sensor", cam["calibrated_sensor_token"]), t.get("ego_pose", cam["ego_pose_token"])
        pose_l = t.get("ego_pose", lidar["ego_pose_token"])
        assert np.array_equal(c[12:21].reshape(3, 3), R(*pose_l["rotation"])) and list(c[21:24]) == pose_l["translation"]
        assert list(c[24:27]) == [-v for v in pose_c["translation"]]
        assert np.array_equal(c[27:36].reshape(3, 3), R(*pose_c["rotation"]).T)
        assert list(c[36:39]) == [-v for v in cs_c["translation"]]
        assert np.array_equal(c[39:48].reshape(3, 3), R(*cs_c["rotation"]).T)
        assert np.array_equal(c[48:57].reshape(3, 3), np.array(cs_c["camera_intrinsic"]))
        assert pose_l["translation"] != pose_c["translation"]            # lidar and camera time differ


def test_tree_properties(tree):
    """what the GPU tests rely on, by the restatement: every view keeps points, no point sits on a threshold, some points
    are seen by two cameras and some by none, rows and columns go negative, pixels repeat"""
    for tok, t in tree["truth"].items():
        seen = np.zeros(len(t["points"]), np.int64)
        assert 2900 <= len(t["points"]) <= 3000
        for ch in N.CHANNELS:
            lo, hi = N.fov_bounds(ch)
            assert not N.too_close(t["points"], t["chains"][ch], 1, 0.1, lo, hi).any()
            assert not N.too_close(t["points"], t["chains"][ch], 0, 1.0, bound_h=float(N.W), bound_w=float(N.H)).any()
            s = (1.0, 1.0) if ch == "CAM_BACK" else (0.5, 0.6)
            r = N.restate(t["points"], t["chains"][ch], 1, 0.1, lo, hi, row_scale=s[0], col_scale=s[1])
            assert 300 <= r["meta"][0] < len(t["points"]) and r["meta"][1] < 0 and r["meta"][3] < 0
            assert r["meta"][2] - r["meta"][1] < 400 and r["meta"][4] - r["meta"][3] < 400
            assert len(np.unique(r["x_data"].astype(np.int64) * 4096 + r["y_data"])) < r["meta"][0]
            frac = r["xy"] - np.trunc(r["xy"])
            assert (frac[r["xy"] < 0] != 0).any()                        # truncation toward zero is not floor
            r0 = N.restate(t["points"], t["chains"][ch], 0, 1.0, bound_h=float(N.W), bound_w=float(N.H))
            assert r0["meta"][0] >= 100 and r0["meta"][1] >= 1 and r0["meta"][2] <= N.H - 2 and r0["meta"][4] <= N.W - 2
            seen += r["keep"]
        assert (seen == 0).sum() >= 20 and (seen >= 2).sum() >= 100


def test_restatement_against_exact_arithmetic():
    """the chain of the restatement against rational arithmetic rounded to float32 once per step: the float64 rounding of the
    single products and sums can only matter within 2^-29 of a float32 tie, and none of these points comes that close"""
    from fractions import Fraction as Fr
    rng = np.random.default_rng(5)
    chain = N.make_chain(rng, cam=2)
    pts = N.make_points(rng, 6)
    got = N.camera_frame(pts, chain)
    c = [Fr(float(v)) for v in chain]
    r32 = lambda p: [Fr(float(np.float32(float(v)))) for v in p]
    rot = lambda o, p: r32([sum(c[o + 3 * i + k] * p[k] for k in range(3)) for i in range(3)])
    tr = lambda o, p: r32([p[i] + c[o + i] for i in range(3)])
    for n in range(len(pts)):
        p = [Fr(float(v)) for v in pts[n, :3]]
        p = tr(9, rot(0, p))
        p = tr(21, rot(12, p))
        p = rot(27, tr(24, p))
        p = rot(39, tr(36, p))
        assert [float(v) for v in p] == [float(v) for v in got[n]], n
    assert np.abs(got).max() < 60 and (np.abs(got[:, 2]) > 0.5).all()          # camera-frame metres, not global ones


def test_task_modules_call_the_factory():
    sites = ["tasks/epmf/trainer.py", "tasks/salsanext/trainer.py", "tasks/pmf_eval_nuscenes/infer.py",
             "tasks/epmf_eval_nuscenes/infer.py", "tasks/salsanext_eval_nuscenes/infer.py",
             "tasks/pmf_eval_nuscenes/testset_eval/main.py", "tasks/pmf_eval_nuscenes/testset_eval/check_valid.py"]
    for rel in sites + ["tasks/pmf/trainer.py"]:
        with open(os.path.join(ROOT, rel)) as f:
            src = f.read()
        assert not re.search(r"nuScenes\.Nuscenes(V2)?\(", src), rel
        if rel in sites:
            assert "pc_processor.dataset.nuScenes.open_nuscenes(" in src and 'config.get("nus_splits")' in src, rel
    with open(os.path.join(ROOT, "tasks/epmf/trainer.py")) as f:
        src = f.read()
    assert '"v1.0-mini" if s.is_debug else "v1.0-trainval"' in src and "open_nuscenes(True," in src
    with open(os.path.join(ROOT, "tasks/pmf/trainer.py")) as f:
        assert re.search(r'elif s\.dataset == "nuScenes":[^\n]*\n(\s*#[^\n]*\n)*\s*raise NotImplementedError\(', f.read())
    import pc_processor
    from pmf_amd.dataset.nuScenes import NuscenesNative, NuscenesV2Native, open_nuscenes
    assert pc_processor.dataset.nuScenes.open_nuscenes is open_nuscenes
    assert issubclass(NuscenesV2Native, object) and NuscenesNative is not NuscenesV2Native


def test_factory_picks_the_class(tree):
    from pmf_amd.dataset.nuScenes import NuscenesNative, NuscenesV2Native
    assert type(_open(False, tree["root"])) is NuscenesNative and type(_open(True, tree["root"])) is NuscenesV2Native
    v2 = _open(True, tree["root"])
    for name in ("token_list", "split", "map_name_from_general_index_to_segmentation_index", "mapped_cls_name", "fov_angle",
                 "__len__", "parsePathInfoByIndex", "loadDataByIndex", "loadLabelByIndex", "labelMapping", "loadImage",
                 "mapLidar2Camera", "mapLidar2CameraCropYaw", "loadImageDevice", "loadPointcloud", "projectDevice"):
        assert hasattr(v2, name), name
    assert not hasattr(v2, "proj_matrix")                    # PerspectiveViewLoaderV2 tells the dataset kinds apart by it
    assert not hasattr(_open(False, tree["root"]), "projectDevice")


def test_task_configs_load():
    import importlib.util
    for task, key in (("epmf", "nclasses"), ("salsanext", "n_classes")):
        spec = importlib.util.spec_from_file_location("opt_" + task, os.path.join(ROOT, "tasks", task, "option.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        o = mod.Option(os.path.join(ROOT, "tasks", task, "config_server_nus.yaml"))
        assert o.dataset == "nuScenes" and getattr(o, key) == 17 and "nus_splits" in o.config
