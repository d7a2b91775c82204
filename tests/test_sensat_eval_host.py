"""SensatUrban evaluation without a GPU: the tile enumeration and the dataset's crops against the reference run recorded in
tests/golden/g19_sensat_tiles.npz, the dataset surface on a synthetic tree, the PLY reader, the task's options, the C
surface, the wrappers' argument checks, and the properties of the synthetic frames that the GPU tests rely on."""
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
TASK = os.path.join(ROOT, "tasks", "sensat_urban", "pmf_eval")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import sensat_eval_cases as S  # noqa: E402

NEW = ("pmf_bev_tile_pre", "pmf_bev_tile_accum", "pmf_bev_points")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_symbols_declared_bound_and_built():
    from pmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    src = open(os.path.join(ROOT, "pmf_amd", "csrc", "bev_eval.hip")).read()
    so = os.path.join(ROOT, "pmf_amd", "libpmf_amd.so")
    assert os.path.isfile(so), "build() first"
    for name, nargs in zip(NEW, (14, 11, 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in _lib.EXPORTS
        assert re.search(r'extern "C" int %s\(' % name, src)
        assert hasattr(ctypes.CDLL(so), name)
        assert len(getattr(_lib.lib(), name).argtypes) == nargs


def test_tile_windows_and_use_crop_match_the_reference_run(tmp_path):
    import pc_processor
    from pmf_amd.postproc import tile_windows
    g = np.load(S.GOLDEN)
    assert os.path.getsize(S.GOLDEN) < (1 << 20)
    # the tree of the fixture, rebuilt by recipe: the recorded input frames are what the recipe gives
    tree = S.write_tree(str(tmp_path), "val", quantise=True)
    for name, h, w, _ in S.FRAMES:
        assert np.array_equal(tree[name][0]["feature_map"], g[name + ".feature_map"].astype(np.float64))
        assert np.array_equal(tree[name][0]["label_map"], g[name + ".label_map"])
    shapes = {name: (h, w) for name, h, w, _ in S.FRAMES}
    for size in S.G19_SIZES:
        ds = pc_processor.dataset.SensatUrban(str(tmp_path), "val", keep_idx=False, img_h=size, img_w=size, use_crop=True)
        ours = {n.replace(".pth", ""): [] for n in ds.data_split}
        assert "cambridge_block_1" not in ours and set(ours) == set(shapes)
        i = 0
        for n in ds.data_split:                                   # (sorted here, os.listdir order in the reference)
            for _ in tile_windows(*shapes[n.replace(".pth", "")], size):
                ours[n.replace(".pth", "")].append(ds.readDataByIndex(i))
                i += 1
        assert i == len(ds) == g["crop_feature_%d" % size].shape[0]
        j = 0
        for n in g["order_%d" % size]:
            n = str(n)
            h, w = shapes[n]
            wins = tile_windows(h, w, size)
            assert wins == S.windows_np(h, w, size) and len(wins) == len(ours[n])
            for k, (hs, he, ws, we) in enumerate(wins):
                want_f, want_l = g["crop_feature_%d" % size][j].astype(np.float64), g["crop_label_%d" % size][j]
                assert ours[n][k]["feature_map"].dtype == np.float64
                assert np.array_equal(ours[n][k]["feature_map"], want_f), (n, size, k)
                assert np.array_equal(ours[n][k]["label_map"], want_l.astype(np.float64)), (n, size, k)
                # and the window itself: the crop is the frame's window, zero outside it
                full = g[n + ".feature_map"].astype(np.float64)
                assert np.array_equal(want_f[:, :he - hs, :we - ws], full[:, hs:he, ws:we])
                assert not want_f[:, he - hs:].any() and not want_f[:, :, we - ws:].any()
                j += 1
        assert j == i
    assert tile_windows(70, 100, 32)[3] == (0, 32, 68, 100) and tile_windows(70, 100, 32)[-1] == (38, 70, 68, 100)
    assert tile_windows(40, 52, 48) == [(0, 40, 0, 48), (0, 40, 4, 52)]
    assert tile_windows(64, 64, 32) == [(0, 32, 0, 32), (0, 32, 32, 64), (32, 64, 0, 32), (32, 64, 32, 64)]


def test_dataset_surface_on_a_synthetic_tree(tmp_path):
    import pc_processor
    from pmf_amd.dataset import SensatUrban
    assert pc_processor.dataset.SensatUrban is SensatUrban
    assert sys.modules["pc_processor.dataset.sensat_urban"].SensatUrban is SensatUrban
    tree = S.write_tree(str(tmp_path), "val")
    ds = SensatUrban(str(tmp_path), "val", keep_idx=True)
    assert len(ds) == 2 and ds.data_split == [n + ".pth" for n, _, _, _ in S.FRAMES]
    assert ds.split_folder == os.path.join(str(tmp_path), "val")
    assert ds.mapped_cls_name[-1] == "ignore" and ds.mapped_cls_name[0] == "Ground" and ds.mapped_cls_name[12] == "Water"
    assert len(ds.mapped_cls_name) == 14
    for i, (name, h, w, npts) in enumerate(S.FRAMES):
        frame, labels, _ = tree[name]
        got = ds.readDataByIndex(i)
        assert got["feature_map"].shape == (8, h, w) and got["feature_map"].dtype == np.float64
        assert np.array_equal(got["feature_map"], frame["feature_map"]) and np.array_equal(got["h_idx"], frame["h_idx"])
        assert ds.readFileNameByIndex(i) == name + ".bin"
        lab = ds.readLabelByIndex(i)
        assert lab.dtype == np.uint8 and np.array_equal(lab, labels) and lab.size == npts
    dropped = SensatUrban(str(tmp_path), "val", keep_idx=False).readDataByIndex(0)
    assert dropped["h_idx"] is None and dropped["w_idx"] is None
    with pytest.raises(ValueError, match="invalid split"):
        SensatUrban(str(tmp_path), "valid")


def test_read_ply_round_trip(tmp_path):
    tools = _load("sensat_tools_under_test", os.path.join(TASK, "sensat_tools.py"))
    _, labels, xyz, rgb = S.make_frame(3, 20, 24, 300)
    for cls in (labels, None):
        path = str(tmp_path / ("a%d.ply" % (cls is None)))
        S.write_ply(path, xyz, rgb, cls)
        d = tools.read_ply(path)
        assert d.shape == (300,) and d.dtype.names[:6] == ("x", "y", "z", "red", "green", "blue")
        assert d["z"].dtype == np.float32 and np.array_equal(d["z"], xyz[:, 2]) and np.array_equal(d["x"], xyz[:, 0])
        assert d["green"].dtype == np.uint8 and np.array_equal(d["green"], rgb[:, 1])
        assert ("class" in d.dtype.names) == (cls is not None)
        if cls is not None:
            assert np.array_equal(d["class"], labels)
        d["z"][0] = 0                                              # writable copy
    bad = str(tmp_path / "ascii.ply")
    with open(bad, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0.0\n")
    with pytest.raises(ValueError, match="binary_little_endian"):
        tools.read_ply(bad)


def test_option_reads_the_shipped_config(tmp_path):
    opt = _load("sensat_eval_option", os.path.join(TASK, "option.py"))
    with open(os.path.join(TASK, "config_server.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["img_size"] == [320, 448, 576] and cfg["n_classes"] == 14 and cfg["dataset"] == "SensatUrban"
    assert cfg["img_backbone"] == "resnet101" and cfg["base_channels"] == 48 and cfg["imagenet_pretrained"] is True
    assert cfg["feature_mean"] == S.MEAN and cfg["feature_std"] == S.STD
    assert cfg["post"]["KNN"] == {"use": False, "params": S.KNN_PARAMS} and cfg["post"]["tta"] == {"use": False}
    assert cfg["save_scores"] is True and cfg["n_samples_split"] == 400 and cfg["downscale"] == 16
    with pytest.raises(ValueError, match="training path not exists"):
        opt.Option(os.path.join(TASK, "config_server.yaml"))
    cfg.update(training_folder=str(tmp_path), experiment_id="run7")
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    o = opt.Option(path)
    assert o.save_path == os.path.join(str(tmp_path), "Eval-PMFNet_SensatUrban_run7")
    assert o.pretrained_model == os.path.join(str(tmp_path), "checkpoint", "best_last_model.pth")
    assert (o.nclasses, o.img_size, o.has_label, o.save_scores, o.img_backbone) == (14, [320, 448, 576], False, True,
                                                                                    "resnet101")
    o.check_path()
    o.check_path()
    assert os.path.isdir(o.save_path)
    del cfg["save_scores"]
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    assert opt.Option(path).save_scores is True
    cfg["save_scores"] = False
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    assert opt.Option(path).save_scores is False


def test_wrappers_reject_bad_arguments_without_a_device():
    from pmf_amd.postproc import BevTileEvaluator, bev_points, bev_tile_accum, bev_tile_pre
    f32 = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError):                              # CPU tensors
        bev_tile_pre(f32(8, 40, 52), f32(8), f32(8), [(0, 0)], 32)
    with pytest.raises(ValueError):
        bev_tile_accum(f32(1, 14, 32, 32), [(0, 0)], 32, 1, f32(14, 40, 52))
    with pytest.raises(ValueError):
        bev_points(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                   14)
    with pytest.raises(ValueError, match="multiples of 16"):
        BevTileEvaluator(None, 14, S.MEAN, S.STD, [320, 450], device="cpu")
    with pytest.raises(ValueError, match="one entry per channel"):
        BevTileEvaluator(None, 14, S.MEAN[:5], S.STD[:5], [320], device="cpu")
    with pytest.raises(ValueError, match="Nearest neighbor kernel must be odd number"):
        BevTileEvaluator(None, 14, S.MEAN, S.STD, [320], knn_params=dict(S.KNN_PARAMS, search=4), device="cpu")
    with pytest.raises(ValueError, match="tile_batch"):
        BevTileEvaluator(None, 14, S.MEAN, S.STD, [320], tile_batch=65, device="cpu")
    assert BevTileEvaluator(None, 14, S.MEAN, S.STD, [320], device="cpu").tile_batch == 4
    assert BevTileEvaluator(None, 14, S.MEAN, S.STD, [320], tta=True, device="cpu").tile_batch == 1
    # the library's own guards (host-side: nothing is launched)
    from pmf_amd import _lib
    lib = _lib.lib()
    org = (ctypes.c_int32 * 2)(0, 0)
    far = (ctypes.c_int32 * 2)(40, 0)
    p = 4096                                                     # a non-null pointer that is never dereferenced
    assert lib.pmf_bev_tile_pre(0, 40, 52, p, p, org, 1, 32, 1, p, p, 0, 0, None) == _lib.PMF_E_ARG       # null frame
    assert lib.pmf_bev_tile_pre(p, 40, 52, p, p, org, 1, 40, 1, p, p, 0, 0, None) == _lib.PMF_E_ARG       # S % 16
    assert lib.pmf_bev_tile_pre(p, 40, 52, p, p, org, 1, 32, 7, p, p, 0, 0, None) == _lib.PMF_E_ARG       # V
    assert lib.pmf_bev_tile_pre(p, 40, 52, p, p, far, 1, 32, 1, p, p, 0, 0, None) == _lib.PMF_E_ARG       # window outside
    assert lib.pmf_bev_tile_pre(p, 40, 52, p, p, org, 1, 32, 1, p, p, p, 0, None) == _lib.PMF_E_ARG       # one pad only
    assert lib.pmf_bev_tile_pre(p, 40, 52, p, p, org, 65, 32, 1, p, p, 0, 0, None) == _lib.PMF_E_ARG      # too many tiles
    assert lib.pmf_bev_tile_accum(p, 0, 14, org, 1, 32, 1, 0, 40, 52, None) == _lib.PMF_E_ARG             # null map
    assert lib.pmf_bev_tile_accum(p, p, 14, org, 1, 32, 1, p, 40, 52, None) == _lib.PMF_E_ARG             # pad with V = 1
    assert lib.pmf_bev_tile_accum(p, 0, 14, far, 1, 32, 6, p, 40, 52, None) == _lib.PMF_E_ARG
    assert lib.pmf_bev_tile_accum(p, 0, 14, org, 1, 24, 6, p, 40, 52, None) == _lib.PMF_E_ARG
    assert lib.pmf_bev_points(0, 4, 4, p, p, 3, 0, 0, 14, 0, 0, p, None) == _lib.PMF_E_ARG                # no map, no votes
    assert lib.pmf_bev_points(p, 4, 4, p, p, 3, 0, 0, 14, p, 0, p, None) == _lib.PMF_E_ARG                # conf without label
    assert lib.pmf_bev_points(p, 4, 4, p, p, 3, 0, p, 65, p, 0, p, None) == _lib.PMF_E_ARG                # C > 64
    assert lib.pmf_bev_points(p, 4, 4, p, p, 3, 0, 0, 14, 0, 0, 0, None) == _lib.PMF_E_ARG                # no output
    assert lib.pmf_bev_points(p, 4, 4, p, p, 0, 0, 0, 14, 0, 0, 0, None) == 0                             # P == 0


def test_synthetic_frames_meet_the_conditions_of_the_gpu_tests():
    from tests.salsa_eval_cases import knn_vote_np
    from pmf_amd.postproc.knn import inverse_gaussian_window
    wgt = inverse_gaussian_window(S.KNN_PARAMS["search"], S.KNN_PARAMS["sigma"]).numpy()
    for k, (name, h, w, npts) in enumerate(S.FRAMES):
        frame, labels, xyz, rgb = S.make_frame(k, h, w, npts)
        fm = frame["feature_map"]
        assert fm.shape == (8, h, w) and fm.dtype == np.float64 and labels.dtype == np.uint8 and labels.max() <= 12
        assert set(np.unique(fm[4])) == {0.0, 1.0} and 0.1 < (fm[4] == 0).mean() < 0.5
        assert not fm[:, fm[4] == 0].any() and (frame["label_map"][fm[4] == 0] == -1).all()
        pix = frame["h_idx"] * w + frame["w_idx"]
        assert pix.size == npts and np.unique(pix).size < 0.9 * npts                 # points sharing a pixel
        # the vote on a recipe map does not rest on the order among equal distances
        conf = S.prob_recipe(5 + k, 1, max(h, w))[0, :, :h, :w]
        am = conf.argmax(0)
        assert (am[frame["h_idx"], frame["w_idx"]] == 0).sum() > 10
        args = (fm[0].astype(np.float32), xyz[:, 2], am, frame["w_idx"], frame["h_idx"], wgt, S.NCLASSES)
        a, b = knn_vote_np(*args), knn_vote_np(*args, reverse=True)
        assert np.array_equal(a, b) and (a != am[frame["h_idx"], frame["w_idx"]]).mean() > 0.01
    # recipe sums: the order of the seven additions shows in the last bit somewhere
    p = torch.from_numpy(S.prob_recipe(1, 7, 32))
    fwd = ((((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]) + p[6])
    rev = ((((((p[6] + p[5]) + p[4]) + p[3]) + p[2]) + p[1]) + p[0])
    assert not torch.equal(fwd, rev)
