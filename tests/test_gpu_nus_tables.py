"""The devkit-free nuScenes reader on the GPU: pmf_nus_project against the numpy restatement of tests/nus_tables_cases.py,
bit for bit on every output, and the two readers behind the loaders that take them (PerspectiveViewLoaderV2 in its three
layouts and through its host path, NusPerspectiveViewLoader, SweepEvaluator over the six views of a sweep)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nus_tables_cases as N
import nus_v2_cases as V

pytestmark = pytest.mark.gpu

B = 256                              # PMF_NUS_BLOCK (asserted below)
GUARD = 64


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _clean_points(rng, P, cols, checks):
    """exactly P sweep rows none of which sits on a threshold of ``checks`` = [(chain, mode, kwargs of too_close)]"""
    pts = N.make_points(rng, 2 * P + 64, cols)
    bad = np.zeros(len(pts), bool)
    for chain, mode, kw in checks:
        bad |= N.too_close(pts, chain, mode, **kw)
    pts = np.ascontiguousarray(pts[~bad][:P])
    assert len(pts) == P
    return pts


def _raw_call(points, chain, mode, min_dist, fov_lo, fov_hi, bound_h, bound_w, rs, cs, sc):
    """pmf_nus_project into buffers with guard rows behind them and a filled meta: -> numpy dict + what was left untouched"""
    from pmf_amd import _lib as L
    assert L.NUS_BLOCK == B
    P = len(points)
    pts = torch.from_numpy(points).cuda()
    n = P + GUARD
    f = dict(keep=torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda"),
             src=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
             crop=torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda"),
             xy=torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda"),
             xd=torch.full((n,), -7, dtype=torch.int32, device="cuda"), yd=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
             depth=torch.full((n,), -7.0, dtype=torch.float32, device="cuda"),
             meta=torch.full((5 + GUARD,), -7, dtype=torch.int32, device="cuda"),
             blk=torch.full(((P + B - 1) // B + 1 + GUARD,), -7, dtype=torch.int32, device="cuda"))
    chain = np.ascontiguousarray(chain, np.float64)
    rc = L.lib().pmf_nus_project(pts.data_ptr(), P, points.shape[1], chain.ctypes.data, mode, float(min_dist), float(fov_lo),
                                 float(fov_hi), float(bound_h), float(bound_w), float(rs), float(cs), float(sc),
                                 f["keep"].data_ptr(), f["src"].data_ptr(), f["crop"].data_ptr(), f["xy"].data_ptr(),
                                 f["xd"].data_ptr(), f["yd"].data_ptr(), f["depth"].data_ptr(), f["meta"].data_ptr(),
                                 f["blk"].data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in f.items()}


def _check(points, chain, mode, min_dist=0.1, fov=(0.0, 0.0), bounds=(0.0, 0.0), scales=(1.0, 1.0), img_scale=1.0):
    want = N.restate(points, chain, mode, min_dist, fov[0], fov[1], bounds[0], bounds[1], scales[0], scales[1], img_scale)
    got = _raw_call(points, chain, mode, min_dist, fov[0], fov[1], bounds[0], bounds[1], scales[0], scales[1], img_scale)
    P, K = len(points), want["meta"][0]
    assert np.array_equal(got["keep"][:P], want["keep"].astype(np.uint8)) and (got["keep"][P:] == 0x5A).all()
    assert got["meta"][0] == K and (got["meta"][5:] == -7).all()
    if K:
        assert got["meta"][:5].tolist() == want["meta"]
    else:
        assert (got["meta"][1:5] == -7).all()                             # K = 0: nothing else is written
    for name, ref in (("src", want["src"]), ("crop", want["crop"]), ("xy", want["xy"]), ("xd", want["x_data"]),
                      ("yd", want["y_data"]), ("depth", want["depth"])):
        assert got[name][:K].dtype == ref.dtype and got[name][:K].tobytes() == ref.tobytes(), name      # bit for bit
        assert (got[name][K:] == -7).all(), name                          # K rows and not one more
    assert (got["blk"][(P + B - 1) // B:] == -7).all()
    return want


@pytest.fixture(scope="module")
def chains():
    rng = np.random.default_rng(21)
    return [N.make_chain(rng, cam) for cam in range(6)]


@pytest.mark.parametrize("P", [1, B - 1, B, B + 1, 3 * B + 77])
@pytest.mark.parametrize("mode", [0, 1])
def test_project_bit_equal_to_the_restatement(P, mode, chains):
    rng = np.random.default_rng(100 * mode + P)
    for cam, stride, scales, img_scale in ((0, 5, (1.0, 1.0), 1.0), (3, 4, (0.5, 0.6), 1.13)):
        chain = chains[cam]
        lo, hi = N.fov_bounds(N.CHANNELS[cam])
        if mode == 0:
            scales = (1.0, 1.0)
        kw = dict(min_dist=0.1, fov_lo=lo, fov_hi=hi) if mode else dict(min_dist=1.0, bound_h=float(N.W), bound_w=float(N.H))
        pts = _clean_points(rng, P, stride, [(chain, mode, kw)])
        if P == 1:                                       # the one point is in view: the camera's axis in the lidar frame
            a = math.radians(N.CAM_YAW[cam] + 90.0)
            pts[0, :3] = (12.0 * math.cos(a), 12.0 * math.sin(a), 0.4)
            assert not N.too_close(pts, chain, mode, **kw).any()
        want = _check(pts, chain, mode, kw["min_dist"], (lo, hi), (float(N.W), float(N.H)), scales, img_scale)
        assert want["meta"][0] >= 1 and (P == 1 or want["meta"][0] < P)
        if mode == 1 and P > B:
            assert want["meta"][1] < 0 and want["meta"][3] < 0          # negative rows and columns: truncation toward zero
            frac = want["xy"] - np.trunc(want["xy"])
            assert (frac[want["xy"] < 0] != 0).any()


def test_view_that_keeps_nothing_and_view_that_keeps_all(chains):
    from pmf_amd.dataset.nuScenes.tables import nus_project_gpu
    rng = np.random.default_rng(7)
    chain = chains[0]
    lo, hi = N.fov_bounds("CAM_FRONT")
    pts = _clean_points(rng, 2000, 5, [(chain, 1, dict(min_dist=0.1, fov_lo=lo, fov_hi=hi))])
    behind = N.camera_frame(pts, chain)[:, 2] < -1.0
    assert behind.sum() > 200
    none = np.ascontiguousarray(pts[behind])
    assert _check(none, chain, 1, 0.1, (lo, hi))["meta"] == [0]
    assert _check(none, chain, 0, 1.0, bounds=(float(N.W), float(N.H)))["meta"] == [0]
    with pytest.raises(ValueError, match="keeps no point"):
        nus_project_gpu(torch.from_numpy(none).cuda(), chain, 1, 0.1, lo, hi, 0.0, 0.0, 1.0, 1.0, 1.0)
    r = N.restate(pts, chain, 1, 0.1, lo, hi)
    every = np.ascontiguousarray(pts[r["keep"]])
    assert len(every) > B
    assert _check(every, chain, 1, 0.1, (lo, hi))["meta"][0] == len(every)
    r0 = N.restate(pts, chain, 0, 1.0, bound_h=float(N.W), bound_w=float(N.H))
    every0 = np.ascontiguousarray(pts[r0["keep"]][:, :4])
    assert len(every0) > 50
    assert _check(every0, chain, 0, 1.0, bounds=(float(N.W), float(N.H)))["meta"][0] == len(every0)


def test_wrapper_returns_the_restatement(chains):
    from pmf_amd.dataset.nuScenes.tables import nus_project_gpu
    rng = np.random.default_rng(9)
    chain = chains[4]
    lo, hi = N.fov_bounds("CAM_BACK_LEFT")
    pts = _clean_points(rng, 1000, 5, [(chain, 1, dict(min_dist=0.1, fov_lo=lo, fov_hi=hi))])
    want = N.restate(pts, chain, 1, 0.1, lo, hi, row_scale=0.5, col_scale=0.6, img_scale=1.07)
    o = nus_project_gpu(torch.from_numpy(pts).cuda(), chain, 1, 0.1, lo, hi, 0.0, 0.0, 0.5, 0.6, 1.07)
    assert [o["K"], o["x_min"], o["x_max"], o["y_min"], o["y_max"]] == want["meta"]
    for name in ("keep", "src", "crop", "xy", "x_data", "y_data", "depth"):
        assert np.array_equal(o[name].cpu().numpy(), want[name].astype(o[name].cpu().numpy().dtype)), name
    with pytest.raises(AssertionError):
        nus_project_gpu(torch.from_numpy(pts), chain, 1, 0.1, lo, hi, 0.0, 0.0, 1.0, 1.0, 1.0)          # host tensor


# ---- the readers behind the loaders -----------------------------------------------------------------------------------
CFG = {"PVconfig": {"proj_h": 64, "proj_w": 128, "proj_ht": 32, "proj_wt": 64, "img_jitter": [0.4, 0.4, 0.4]}}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("nus") / "tree")
    return dict(root=root, truth=N.write_tree(root))


def _v2(tree, split="val"):
    from pmf_amd.dataset.nuScenes import open_nuscenes
    return open_nuscenes(True, tree["root"], "v1.0-mini", split)


def _view_ref(tree, ds, i, image=None, img_scale=1.0):
    """the restatement of view i + the reference's scatter on it -> (restatement, proj, depth, image)"""
    pair = ds.token_list[i]
    t = tree["truth"][pair["lidar_token"]]
    ch = pair["cam_channel"]
    lo, hi = N.fov_bounds(ch)
    s = (1.0, 1.0) if ch == "CAM_BACK" else (0.5, 0.6)
    r = N.restate(t["points"], t["chains"][ch], 1, 0.1, lo, hi, row_scale=s[0], col_scale=s[1], img_scale=img_scale)
    if image is None:
        image = np.asarray(ds.loadImage(i))
    labels = np.array(N.CLASS_OF_INDEX)[t["labels"]][r["keep"]]
    proj, depth = N.frame_ref(r["crop"], labels, r["xy"], image)
    return r, proj, depth, image, t


class HostOnly(object):
    """the same dataset without projectDevice: PerspectiveViewLoaderV2 takes its host path (_nus_item)"""

    def __init__(self, ds):
        self._ds = ds

    def __getattr__(self, name):
        if name in ("projectDevice", "loadImageDevice", "proj_matrix"):
            raise AttributeError(name)
        return getattr(self._ds, name)

    def __len__(self):
        return len(self._ds)


@pytest.mark.parametrize("i", [1, 3, 8])             # CAM_FRONT_RIGHT, CAM_BACK (unscaled) of sample 0, CAM_BACK_RIGHT of sample 1
def test_loader_v2_layouts_equal_the_restatement(tree, i):
    from PIL import Image
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    ds = _v2(tree)
    r, rp, rd, img, t = _view_ref(tree, ds, i)
    pv = CFG["PVconfig"]
    assert (ds.token_list[i]["cam_channel"] == "CAM_BACK") == (i == 3)
    assert np.array_equal(ds.loadImageDevice(i).cpu().numpy(), img)
    assert np.array_equal(rd, r["depth"])                # the loader's numpy norm and the kernel's sqrtf agree here
    # the dataset's own method, in the reference's layout
    crop, xy, keep = ds.mapLidar2CameraCropYaw(i, None)
    assert crop.dtype == np.float32 and xy.dtype == np.float64 and keep.dtype == np.bool_
    assert np.array_equal(crop, r["crop"]) and np.array_equal(xy, r["xy"]) and np.array_equal(keep, r["keep"])
    # validation item
    val = PerspectiveViewLoaderV2(ds, CFG, is_train=False)[i]
    assert np.array_equal(val.cpu().numpy(), N.center_crop_ref(N.pad_ref(rp, pv["proj_h"], pv["proj_w"]), pv["proj_h"], pv["proj_w"]))
    # return_uproj tuple
    proj, xy, depth, keep, pts = PerspectiveViewLoaderV2(ds, CFG, is_train=False, return_uproj=True)[i]
    assert np.array_equal(proj.cpu().numpy(), rp) and np.array_equal(xy.cpu().numpy(), r["xy"]) and xy.dtype == torch.float64
    assert np.array_equal(depth.cpu().numpy(), rd) and np.array_equal(keep.cpu().numpy(), r["keep"]) and keep.dtype == torch.bool
    assert np.array_equal(pts.numpy(), t["points"][:, :4])
    assert proj[8].sum() > 100 and (proj[9] > 0).any() and (proj[5:8] > 0).any()
    # _eval_item: src is the position in the sweep, sem the sweep's raw labels, lut the 256-entry table
    proj, xy, depth, keep, extra = PerspectiveViewLoaderV2(ds, CFG, is_train=False)._eval_item(i)
    assert np.array_equal(proj.cpu().numpy(), rp)
    assert np.array_equal(extra["x_data"].cpu().numpy(), r["x_data"]) and np.array_equal(extra["y_data"].cpu().numpy(), r["y_data"])
    assert (extra["x_min"], extra["y_min"]) == (r["meta"][1], r["meta"][3])
    assert np.array_equal(extra["src"].cpu().numpy(), r["src"]) and extra["src"].dtype == torch.int32
    assert np.array_equal(extra["sem"].cpu().numpy(), t["labels"].astype(np.int32)) and extra["sem"].dtype == torch.int32
    lut = extra["lut"].cpu().numpy()
    assert lut.shape == (256,) and np.array_equal(lut[:32], N.CLASS_OF_INDEX) and not lut[32:].any()
    # the host path of the same dataset: bit for bit the device path
    host = PerspectiveViewLoaderV2(HostOnly(ds), CFG, is_train=False)
    assert host._is_nus_v2() and not host._has_project_device()
    hp, hxy, hd, hk, hextra = host._eval_item(i)
    assert torch.equal(hp, proj) and torch.equal(hxy, xy) and torch.equal(hd, depth) and torch.equal(hk, keep)
    for k in ("x_data", "y_data", "src", "sem", "lut"):
        assert torch.equal(hextra[k], extra[k]), k
    assert (hextra["x_min"], hextra["y_min"]) == (extra["x_min"], extra["y_min"])
    with pytest.raises(NotImplementedError):
        PerspectiveViewLoaderV2(HostOnly(ds), CFG, is_train=True)[i]
    # training item: same jittered + resized image, same FlipRotateCrop.draw
    ld = PerspectiveViewLoaderV2(ds, CFG, is_train=True, img_aug=True)
    np.random.seed(11 + i)
    torch.manual_seed(11 + i)
    got = ld[i]
    np.random.seed(11 + i)
    torch.manual_seed(11 + i)
    jit = ld.img_jitter.apply(torch.from_numpy(img.copy()).cuda(), *ld.img_jitter.draw()).cpu().numpy()
    assert (jit != img).any()
    sc = np.random.uniform(low=1.0, high=1.2)
    big = np.asarray(Image.fromarray(jit).resize((int(img.shape[1] * sc), int(img.shape[0] * sc)), Image.BILINEAR))
    tr, tp, _, _, _ = _view_ref(tree, ds, i, big, sc)
    padded = N.pad_ref(tp, pv["proj_ht"], pv["proj_wt"])
    draw = ld.aug_ops.draw(padded.shape[1], padded.shape[2])
    want = ld.aug_ops.apply(torch.from_numpy(padded).cuda(), *draw)
    assert got.shape == want.shape == (10, pv["proj_ht"], pv["proj_wt"]) and torch.equal(got, want)
    np.random.seed(11 + i)
    torch.manual_seed(11 + i)
    assert np.array_equal(PerspectiveViewLoaderV2(ds, CFG, is_train=True, img_aug=True, return_uproj=True)[i][1].cpu().numpy(),
                          tr["xy"])


def test_sweep_is_uploaded_once_per_lidar_token(tree):
    ds = _v2(tree)
    ds.mapLidar2CameraCropYaw(0, None)
    first = ds._local.sweep
    for i in range(1, 6):
        ds.mapLidar2CameraCropYaw(i, None)
        assert ds._local.sweep is first and first[1].shape[1] == 5 and first[3].shape == (256,)
    ds.mapLidar2CameraCropYaw(6, None)
    assert ds._local.sweep is not first and ds._local.sweep[0][0] == "sd_1_1_LIDAR_TOP"
    assert len(ds._chains) == 7
    held = ds._local.sweep
    with torch.cuda.stream(torch.cuda.Stream()):             # another stream: not the tensors made on the first one
        ds.mapLidar2CameraCropYaw(7, None)
        assert ds._local.sweep is not held and ds._local.sweep[0][0] == "sd_1_1_LIDAR_TOP"
    torch.cuda.synchronize()


def test_items_built_by_three_threads_on_side_streams(tree):
    """what the training task's prefetch threads do: three threads, a HIP stream each, build the views of ONE dataset object
    concurrently, the sweeps interleaved so that every thread keeps asking for the sweep another has just replaced.  Every
    item equals the restatement and carries the labels of its own sweep; each thread has uploaded into an entry of its own."""
    import threading
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    ds = _v2(tree)
    ld = PerspectiveViewLoaderV2(ds, CFG, is_train=False, return_uproj=True)
    want = {}
    for i in range(len(ds)):
        r, rp, rd, _, t = _view_ref(tree, ds, i)
        want[i] = (rp, r, t["labels"].astype(np.int32))
    assert not np.array_equal(want[0][2][:2000], want[6][2][:2000])      # the two sweeps' labels differ: a mixed-up pair shows
    order = [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11]            # sweep 0, sweep 1, sweep 0, ...
    T, rounds = 3, 3
    barrier = threading.Barrier(T)
    got, errors, entries = {}, [], {}

    def work(j):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                barrier.wait(timeout=30)
                for n in range(rounds):
                    for i in order[j::T] if n % 2 == 0 else order[(j + 1) % T::T]:
                        proj, xy, depth, keep, extra = ld._eval_item(i)
                        got[(j, n, i)] = (proj.cpu().numpy(), xy.cpu().numpy(), extra["src"].cpu().numpy(),
                                          extra["sem"].cpu().numpy(), extra["lut"].cpu().numpy())
                entries[j] = ds._local.sweep
        except Exception as e:                               # reported below, in the main thread
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(T)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(60)
    torch.cuda.synchronize()
    assert not errors, errors
    assert len(got) == rounds * len(order) and len(entries) == T
    for (j, n, i), (proj, xy, src, sem, lut) in got.items():
        rp, r, labels = want[i]
        assert np.array_equal(proj, rp) and np.array_equal(xy, r["xy"]) and np.array_equal(src, r["src"]), (j, n, i)
        assert np.array_equal(sem, labels) and np.array_equal(lut[:32], N.CLASS_OF_INDEX), (j, n, i)
    assert len({id(e) for e in entries.values()}) == T and len({e[0][1] for e in entries.values()}) == T
    assert not hasattr(ds._local, "sweep")                   # the main thread never projected


@pytest.mark.parametrize("i", [0, 3, 10])
def test_nus_perspective_loader_over_the_v1_reader(tree, i):
    from pmf_amd.dataset.nuScenes import NusPerspectiveViewLoader, open_nuscenes
    ds = open_nuscenes(False, tree["root"], "v1.0-mini", "val")
    pair = ds.token_list[i]
    t = tree["truth"][pair["lidar_token"]]
    ch = N.CHANNELS[i % 6]
    assert pair["cam_token"].endswith(ch)
    r = N.restate(t["points"], t["chains"][ch], 0, 1.0, bound_h=float(N.W), bound_w=float(N.H))
    mapped, mask = ds.mapLidar2Camera(i, t["points"][:, :3], N.W, N.H)
    assert mapped.dtype == np.float64 and np.array_equal(mapped, r["xy"]) and np.array_equal(mask, r["keep"])
    img = np.asarray(ds.loadImage(i))
    assert img.shape == (N.H, N.W, 3)
    feature, pmask, plabel, xd, yd, depth, pidx, npts = NusPerspectiveViewLoader(ds, {})[i]
    K = r["meta"][0]
    assert np.array_equal(xd.cpu().numpy(), r["x_data"]) and np.array_equal(yd.cpu().numpy(), r["y_data"])
    assert np.array_equal(pidx.cpu().numpy(), r["src"]) and float(npts.item()) == len(t["points"])
    d = np.linalg.norm(t["points"][:, :3], 2, axis=1)[r["keep"]].astype(np.float32)            # the loader's own depth (:47)
    assert np.array_equal(depth.cpu().numpy(), d) and np.array_equal(d, r["depth"])
    # the reference's scatter (nus_perspective_loader.py:44-58): fancy assignment in file order, the last point wins
    want = np.zeros((10, N.H, N.W), np.float32)
    want[5:8] = (img.astype(np.float32) / 255.0).transpose(2, 0, 1)
    lab = np.array(N.CLASS_OF_INDEX)[t["labels"]]
    for k in range(K):
        p = r["src"][k]
        want[0, r["x_data"][k], r["y_data"][k]] = d[k]
        want[1:5, r["x_data"][k], r["y_data"][k]] = t["points"][p, :4]
        want[8, r["x_data"][k], r["y_data"][k]] = 1.0
        want[9, r["x_data"][k], r["y_data"][k]] = lab[p]
    assert np.array_equal(feature.cpu().numpy(), want[:8]) and np.array_equal(pmask.cpu().numpy(), want[8])
    assert np.array_equal(plabel.cpu().numpy(), want[9]) and want[8].sum() > 100


def test_sweep_evaluator_over_the_six_views_of_a_sweep(tree):
    """random softmax maps (no network) through SweepEvaluator on the loader's items against the numpy merge"""
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    from pmf_amd.postproc.frame_eval import SweepEvaluator, pad_geometry_bottom
    ds = _v2(tree)
    ld = PerspectiveViewLoaderV2(ds, CFG, is_train=False, return_uproj=True)
    nc = 17
    se = SweepEvaluator(nc, V.MEAN, V.STDS, None)
    rng = np.random.default_rng(3)
    t = tree["truth"]["sd_1_0_LIDAR_TOP"]
    P = len(t["points"])
    conf_full, label_full = np.zeros(P, np.float32), np.zeros(P, np.int32)
    extra = None
    for i in range(6):
        proj, xy, depth, keep, extra = ld._eval_item(i)
        r = _view_ref(tree, ds, i)[0]
        h, w = proj.shape[1:]
        H, W, top, left = pad_geometry_bottom(h, w)
        prob = torch.softmax(torch.from_numpy(rng.normal(0, 2, (nc, H, W)).astype(np.float32)), 0)
        se.pre(proj)
        se.post_view(prob.cuda()[None], depth, extra)
        conf, label = V.view_conf_label(prob.numpy()[:, top:top + h, left:left + w], r["x_data"] - r["meta"][1],
                                        r["y_data"] - r["meta"][3])
        V.merge_mask_form(conf_full, label_full, r["keep"].copy(), conf, label)
    assert se.views_in_sweep == 6
    pts_conf = torch.zeros((nc, nc), dtype=torch.int64, device="cuda")
    out = se.finish(extra["sem"], extra["lut"], P, point_conf=pts_conf).cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, label_full.astype(np.uint8))
    assert (out == 0).sum() >= 20 and (out != 0).mean() > 0.5            # points no camera sees stay 0
    pred = label_full.astype(np.int64)                       # the reference scores a point no camera labelled as (0, 0)
    gt = np.array(N.CLASS_OF_INDEX, np.int64)[t["labels"]] * (pred != 0)
    assert np.array_equal(pts_conf.cpu().numpy(), V.np_conf(pred, gt, nc))


def test_tasks_epmf_trains_on_nuscenes(tmp_path, monkeypatch):
    """tasks/epmf with dataset nuScenes and is_debug -- v1.0-mini, and an epoch ends after its first iteration, as in the
    reference -- on a tree of one sample per scene: six views per split, 17 classes, 64 x 128"""
    import os
    import sys
    import yaml
    from pmf_amd.checkpoint import Recorder
    from pmf_amd.dataset.nuScenes import NuscenesV2Native
    from pmf_amd.models import EPMFNet
    from pmf_amd.utils.detinit import deterministic_init
    root = str(tmp_path / "tree")
    N.write_tree(root, samples=1)
    task = os.path.join(N.ROOT, "tasks", "epmf")
    with open(os.path.join(task, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_root=root, is_debug=True, imagenet_pretrained=False, n_threads=0, gpu="0", print_frequency=1,
               save_path=str(tmp_path / "exp"), batch_size=[3, 3], n_epochs=2)
    cfg["PVconfig"].update(proj_h=64, proj_w=128, proj_ht=64, proj_wt=128)
    path = str(tmp_path / "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.syspath_prepend(task)
    for m in ("option", "trainer", "main"):
        monkeypatch.delitem(sys.modules, m, raising=False)
    import option
    import trainer
    s = option.Option(path)
    assert s.dataset == "nuScenes" and s.nclasses == 17 and s.is_debug
    torch.manual_seed(s.seed)
    np.random.seed(s.seed)
    model = deterministic_init(EPMFNet(5, 3, s.nclasses, s.base_channels, imagenet_pretrained=False,
                                       image_backbone=s.img_backbone))
    t = trainer.Trainer(s, model, Recorder(s, s.save_path, use_tensorboard=False))
    train_ds, val_ds = t.train_loader.dataset.dataset, t.val_loader.dataset.dataset
    assert type(train_ds) is NuscenesV2Native and t.train_loader.dataset.is_train and not t.val_loader.dataset.is_train
    assert train_ds.nusc.version == "v1.0-mini" and (train_ds.split, val_ds.split) == ("train", "val")
    assert {p["lidar_token"] for p in train_ds.token_list} == {"sd_0_0_LIDAR_TOP"}
    assert {p["lidar_token"] for p in val_ds.token_list} == {"sd_1_0_LIDAR_TOP"}
    assert len(t.train_loader) == 2 and len(t.val_loader) == 2 and t.ignore_class == [0]
    assert t.mapped_cls_name[4] == "car" and t.alpha.shape == (17,) and t.alpha[0] == 0
    before = sum(float(p.detach().double().sum()) for p in model.parameters())
    t.run(0, mode="Train")
    assert t.engine.iteration == 1 and np.isfinite(t.last_summary["Loss"])
    after = sum(float(p.detach().double().sum()) for p in model.parameters())
    assert np.isfinite(after) and after != before
    res = t.run(0, mode="Validation")
    assert np.isfinite(t.last_summary["Loss"]) and all(v == v for v in res.values())
    for m in ("option", "trainer", "main"):
        sys.modules.pop(m, None)
