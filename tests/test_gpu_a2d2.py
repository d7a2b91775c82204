"""A2D2 on the GPU: pmf_undistort_map, pmf_remap_u8c3 and pmf_a2d2_index against the numpy restatements of
tests/a2d2_cases.py, A2D2_PV + PerspectiveViewLoaderV2 against the host composition of a loader item, and the two tasks
(tasks/epmf with dataset a2d2, tasks/epmf_eval_a2d2) on a synthetic tree."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import a2d2_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _remap_checked(src, m):
    """pmf_remap_u8c3 into a buffer with a guard behind it, twice over different fills: every pixel is written, nothing else"""
    from pmf_amd import _lib as L
    h, w = m.shape[:2]
    n = h * w * 3
    s, md = torch.from_numpy(src).cuda(), torch.from_numpy(np.ascontiguousarray(m)).cuda()
    outs = []
    for fill in (0x5A, 0xA5):
        buf = torch.full((n + 64,), fill, dtype=torch.uint8, device="cuda")
        L.check(L.lib().pmf_remap_u8c3(s.data_ptr(), src.shape[0], src.shape[1], md.data_ptr(), h, w, buf.data_ptr(), _st()),
                "pmf_remap_u8c3")
        got = buf.cpu().numpy()
        assert (got[n:] == fill).all()
        outs.append(got[:n].reshape(h, w, 3))
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def _maps(h, w, sh, sw):
    """name -> int32[h, w, 2] restated maps for a source of sh x sw"""
    K = np.array([[0.9 * w, 0, 0.49 * w], [0, 0.92 * w, 0.52 * h], [0, 0, 1]])

    def shifted(dx, dy):
        k = K.copy()
        k[0, 2] += dx
        k[1, 2] += dy
        return k
    zoom = K.copy()
    zoom[0, 0] *= 0.62           # new focal length shorter: the destination sees far beyond the source
    zoom[1, 1] *= 0.62
    z5 = [0.0] * 5
    return {
        "identity": A.undistort_map("Telecam", K, K, z5, h, w),
        "shift_3_-2": A.undistort_map("Telecam", K, shifted(3, -2), z5, h, w),
        "half_pixel": A.undistort_map("Telecam", K, shifted(0.5, 0.5), z5, h, w),
        "zoom_out": A.undistort_map("Telecam", zoom, K, z5, h, w),
        "telecam": A.undistort_map("Telecam", K * [[0.92], [0.97], [1]], shifted(0.7, -0.4), [-0.26, 0.07, 0.0013, -0.0021, 0.011], h, w),
        "fisheye": A.undistort_map("Fisheye", K * [[0.85], [0.85], [1]], shifted(-0.6, 0.3), [-0.043, 0.012, 0.0031, -0.0007], h, w),
    }


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96)])
def test_remap_bit_equal_to_the_integer_restatement(h, w):
    rng = np.random.RandomState(h)
    src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    for name, (m, t) in _maps(h, w, h, w).items():
        want = A.remap_u8c3(src, m)
        got = _remap_checked(src, m)
        assert np.array_equal(got, want), name
        if name == "identity":
            assert np.array_equal(got, src)
        if name == "zoom_out":
            sx, sy = m[..., 0] >> 5, m[..., 1] >> 5
            outside = (sx < -1) | (sx >= w) | (sy < -1) | (sy >= h)
            partial = ~outside & ((sx < 0) | (sx + 1 >= w) | (sy < 0) | (sy + 1 >= h))
            assert outside.mean() > 1.0 / 3 and partial.any() and not got[outside].any()
    # a source of another size than the destination, and a map with saturated entries
    src2 = rng.randint(0, 256, (29, 41, 3)).astype(np.uint8)
    m = _maps(h, w, 29, 41)["fisheye"][0].copy()
    m[0, 0] = (A.I32_MAX, A.I32_MIN)
    m[-1, -1] = (A.I32_MIN, A.I32_MAX)
    assert np.array_equal(_remap_checked(src2, m), A.remap_u8c3(src2, m))


def test_remap_full_size_frame():
    """one 1208 x 1920 run through the front-centre camera's map"""
    with open(A.CAMS_LIDARS) as f:
        cam = json.load(f)["cameras"]["front_center"]
    h, w = 1208, 1920
    src = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    m, _ = A.undistort_map(cam["Lens"], cam["CamMatrix"], cam["CamMatrixOriginal"], cam["Distortion"], h, w)
    assert np.array_equal(_remap_checked(src, m), A.remap_u8c3(src, m))


def _device_map(lens, newm, orig, dist, h, w):
    from pmf_amd.dataset.a2d2 import undistort_map_gpu
    return undistort_map_gpu(lens, newm, orig, dist, h, w).cpu().numpy()


def _check_map(name, cam, exempt_allowed):
    lens, newm, orig, dist, h, w = cam
    want, t = A.undistort_map(lens, newm, orig, dist, h, w)
    got = _device_map(lens, newm, orig, dist, h, w)
    assert got.shape == want.shape == (h, w, 2) and got.dtype == np.int32
    diff = got.astype(np.int64) - want
    tie = A.near_half(t)
    print("%s: %d of %d entries differ, %d near a tie (%.5f %%)" % (name, int((diff != 0).sum()), diff.size, int(tie.sum()),
                                                                     100.0 * tie.mean()))
    assert (diff[~tie] == 0).all(), name
    assert (np.abs(diff[tie]) <= 1).all(), name
    assert tie.mean() <= (1e-3 if exempt_allowed else 0.0), name
    # end to end: device map, then device remap, equal wherever the maps are equal
    src = np.random.RandomState(7).randint(0, 256, (h, w, 3)).astype(np.uint8)
    same = (diff == 0).all(-1)
    assert np.array_equal(_remap_checked(src, got)[same], A.remap_u8c3(src, want)[same]), name


@pytest.mark.parametrize("name", ["telecam_k1", "telecam_5", "fisheye_k1k2", "fisheye_4"])
def test_device_map_matches_float64_restatement(name):
    _check_map(name, A.map_cameras()[name], True)


def test_device_map_structured_cases_have_no_exemption():
    h, w = 37, 53
    K = np.array([[41.3, 0, 25.7], [0, 40.2, 18.9], [0, 0, 1]])
    for name, dx, dy in (("identity", 0, 0), ("shift", 3, -2), ("half", 0.5, 0.5)):
        k = K.copy()
        k[0, 2] += dx
        k[1, 2] += dy
        _check_map(name, ("Telecam", K, k, [0.0] * 5, h, w), False)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    got = _device_map("Telecam", K, K, [0.0] * 5, h, w)
    assert np.array_equal(got[..., 0], 32 * jj) and np.array_equal(got[..., 1], 32 * ii)
    # degenerate inverse matrix: w' = 0 everywhere -> NaN / infinite coordinates saturate, nothing is read out of bounds
    from pmf_amd import _lib as L
    ir = np.zeros(9)
    ir[2] = 1.0
    d = np.zeros(5)
    out = torch.empty((4, 4, 2), dtype=torch.int32, device="cuda")
    L.check(L.lib().pmf_undistort_map(0, ir.ctypes.data, 10.0, 10.0, 2.0, 2.0, d.ctypes.data, 4, 4, out.data_ptr(), _st()), "map")
    assert set(out.cpu().numpy().reshape(-1).tolist()) <= {A.I32_MIN, A.I32_MAX}


@pytest.fixture(scope="module")
def class_index():
    with open(A.CLASS_INDEX) as f:
        return json.load(f)


@pytest.mark.parametrize("P", [1, 1024, 1025, 3000])
def test_index_kernel_bit_equal_to_numpy(P, class_index):
    from pmf_amd.dataset.a2d2 import a2d2_index_gpu, colour_table
    keys, cls = colour_table(class_index)
    rng = np.random.RandomState(P)
    colours = np.stack(((keys >> 16) & 255, (keys >> 8) & 255, keys & 255), 1).astype(np.uint8)
    sem_image = colours[rng.randint(0, len(colours), (60, 90))]
    pts = rng.uniform(-80, 80, (P, 3)) * rng.choice([1.0, 1e-3, 1e3], (P, 1))
    refl = rng.uniform(0, 1, P)
    rows, cols = rng.randint(0, 60, P).astype(np.int32), rng.randint(0, 90, P).astype(np.int32)
    rows[0], cols[0] = 30, 20                    # 30 * 1.1 = 33.000000000000004, 20 * 1.15 = 23 - 4e-15 (or what numpy says)
    if P > 8:
        rows[1:5], cols[1:5] = (30, 20, 10, 50), (20, 30, 70, 10)
        pts[5] = 0.0
    rgb = sem_image[rows, cols]
    want_sem = A.lookup_loop(class_index, sem_image, rows, cols)
    for sc in (1.0, 1.2, 1.1, 1.15):
        ref = A.index_ref(pts, refl, rows, cols, sc)
        o = a2d2_index_gpu(pts, refl, rows, cols, rgb, keys, cls, sc)
        for k in ("pts", "depth", "xy", "x_data", "y_data"):
            got = o[k].cpu().numpy()
            assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, k
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)), (k, sc)
        assert np.array_equal(o["sem"].cpu().numpy(), want_sem)
        assert o["meta"] == ref["bbox"] + [0, A.I32_MAX]
        if sc == 1.1:
            assert ref["x_data"][0] == 33 and int(o["x_data"][0]) == 33
        if sc == 1.15:
            assert int(o["y_data"][0]) == int(np.float64(20) * np.float64(1.15))
    assert np.array_equal(ref["depth"], np.linalg.norm(pts[:, :3], 2, axis=1).astype(np.float32))
    # no labels: sem is zero, the table is not read
    o = a2d2_index_gpu(pts, refl, rows, cols, None, None, None, 1.0)
    assert not o["sem"].any() and o["meta"][4:] == [0, A.I32_MAX]
    # foreign colours: counted, the first one named
    if P > 8:
        bad = rgb.copy()
        bad[[7, P - 1]] = (1, 2, 3)
        bad[P // 2] = (0, 0, 1)
        o = a2d2_index_gpu(pts, refl, rows, cols, bad, keys, cls, 1.0)
        assert o["meta"][4:] == [3, 7]
        s = o["sem"].cpu().numpy()
        keep = np.ones(P, bool)
        keep[[7, P // 2, P - 1]] = False
        assert np.array_equal(s[keep], want_sem[keep]) and not s[~keep].any()


CFG = {"PVconfig": {"proj_h": 64, "proj_w": 128, "proj_ht": 32, "proj_wt": 64, "img_jitter": [0.4, 0.4, 0.4]}}
KW = dict(unused_index=[], zero_size_index=[], split_bounds=(4, 6))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("a2d2") / "tree")
    cams, cidx, class_index = A.build_tree(root)
    with open(cams) as f:
        return dict(root=root, cams_path=cams, cidx_path=cidx, class_index=class_index, cams=json.load(f))


def _host_frame(ds, tree, i):
    """what the reference's dataset hands the loader for frame i, from the files, with the restated undistortion"""
    from PIL import Image
    d = np.load(ds.lidar_files[i])
    pc = np.concatenate((d["points"], d["reflectance"][:, None]), 1)
    rows, cols = (d["row"] + 0.5).astype(np.int32), (d["col"] + 0.5).astype(np.int32)
    sem = A.lookup_loop(tree["class_index"], np.array(Image.open(ds.label_files[i])), rows, cols)
    img = A.undistorted_ref(tree["cams"], ds._camera_key(i), np.array(Image.open(ds.camera_files[i])))
    return pc, sem, rows, cols, img


@pytest.mark.parametrize("i,cam", [(0, "front_center"), (2, "side_left")])
def test_loader_items_equal_the_restatement(tree, i, cam):
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    from pmf_amd.dataset.a2d2 import A2D2_PV
    ds = A2D2_PV(tree["root"], tree["cams_path"], tree["cidx_path"], split="all", **KW)
    assert ds._camera_key(i) == cam
    pc, sem, rows, cols, img = _host_frame(ds, tree, i)
    from PIL import Image
    assert (img != np.array(Image.open(ds.camera_files[i]))).any()                                # the lens does move pixels
    assert np.array_equal(ds.loadImageDevice(i).cpu().numpy(), img)
    assert np.array_equal(np.asarray(ds.loadImage(i)), img)
    got_pc, got_sem, inst = ds.loadDataByIndex(i)
    assert np.array_equal(got_pc, pc) and got_pc.dtype == np.float64
    assert np.array_equal(got_sem, sem) and got_sem.dtype == np.int32 and not inst.any()
    assert np.array_equal(ds.loadLabelByIndex(i)[0], sem)
    assert len(np.unique(rows.astype(np.int64) * 1000 + cols)) < len(rows)                       # duplicate pixels: last wins
    rp, rxy, rd, rk = A.frame_ref(pc, sem, rows, cols, img)
    pv = CFG["PVconfig"]
    # validation item
    val = PerspectiveViewLoaderV2(ds, CFG, is_train=False)[i]
    assert np.array_equal(val.cpu().numpy(), A.center_crop_ref(A.pad_ref(rp, pv["proj_h"], pv["proj_w"]), pv["proj_h"], pv["proj_w"]))
    # return_uproj tuple
    proj, xy, depth, keep, pts = PerspectiveViewLoaderV2(ds, CFG, is_train=False, return_uproj=True)[i]
    assert np.array_equal(proj.cpu().numpy(), rp) and np.array_equal(xy.cpu().numpy(), rxy) and xy.dtype == torch.float64
    assert np.array_equal(depth.cpu().numpy(), rd) and np.array_equal(keep.cpu().numpy(), rk)
    assert np.array_equal(pts.numpy(), pc)
    # _eval_item
    proj, xy, depth, keep, extra = PerspectiveViewLoaderV2(ds, CFG, is_train=False)._eval_item(i)
    assert np.array_equal(proj.cpu().numpy(), rp) and np.array_equal(depth.cpu().numpy(), rd)
    x_data, y_data = rxy[:, 0].astype(np.int32), rxy[:, 1].astype(np.int32)
    assert np.array_equal(extra["x_data"].cpu().numpy(), x_data) and np.array_equal(extra["y_data"].cpu().numpy(), y_data)
    assert (extra["x_min"], extra["y_min"]) == (int(x_data.min()), int(y_data.min()))
    assert np.array_equal(extra["src"].cpu().numpy(), np.arange(len(pc))) and np.array_equal(extra["sem"].cpu().numpy(), sem)
    assert np.array_equal(extra["lut"].cpu().numpy()[:39], np.arange(39))
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
    tp, txy, _, _ = A.frame_ref(pc, sem, rows, cols, big, sc)
    padded = A.pad_ref(tp, pv["proj_ht"], pv["proj_wt"])
    draw = ld.aug_ops.draw(padded.shape[1], padded.shape[2])
    want = ld.aug_ops.apply(torch.from_numpy(padded).cuda(), *draw)
    assert got.shape == want.shape == (10, pv["proj_ht"], pv["proj_wt"]) and torch.equal(got, want)
    assert got[8].sum() > 0
    np.random.seed(11 + i)
    torch.manual_seed(11 + i)
    assert np.array_equal(PerspectiveViewLoaderV2(ds, CFG, is_train=True, img_aug=True, return_uproj=True)[i][1].cpu().numpy(), txy)


def test_foreign_colour_no_labels_and_empty_frame(tmp_path):
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    from pmf_amd.dataset.a2d2 import A2D2_PV
    root = str(tmp_path / "tree")
    cams, cidx, class_index = A.build_tree(root, foreign=True)
    ds = A2D2_PV(root, cams, cidx, split="all", **KW)
    last = len(ds) - 1
    d = np.load(ds.lidar_files[last])
    rows, cols = (d["row"] + 0.5).astype(np.int32), (d["col"] + 0.5).astype(np.int32)
    sem_image = ds.loadSemImage(ds.label_files[last])
    with pytest.raises(KeyError) as ref:
        A.lookup_loop(class_index, sem_image, rows, cols)
    assert ref.value.args[0] == "#010203"
    for call in (lambda: ds.getLabel(d, sem_image), lambda: ds.loadDataByIndex(last),
                 lambda: PerspectiveViewLoaderV2(ds, CFG, is_train=False)[last]):
        with pytest.raises(KeyError) as got:
            call()
        assert got.value.args == ref.value.args
    assert np.array_equal(ds.getLabel(np.load(ds.lidar_files[0]), ds.loadSemImage(ds.label_files[0])),
                          A.lookup_loop(class_index, ds.loadSemImage(ds.label_files[0]),
                                        *ds._pixel_index(np.load(ds.lidar_files[0]))))
    # has_label=False: the label image is not opened, labels are 0
    nl = A2D2_PV(root, cams, cidx, split="all", has_label=False, **KW)
    item = PerspectiveViewLoaderV2(nl, CFG, is_train=False)[last]
    assert not item[9].any() and item[8].sum() > 0 and not nl.loadDataByIndex(last)[1].any()
    # a frame without points
    np.savez(ds.lidar_files[0], points=np.zeros((0, 3)), reflectance=np.zeros(0), row=np.zeros(0), col=np.zeros(0))
    with pytest.raises(ValueError, match="no points"):
        PerspectiveViewLoaderV2(ds, CFG, is_train=False)[0]


def _task_config(tree, tmp_path, src, **kw):
    import yaml
    with open(src) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_root=tree["root"], cams_lidars_path=tree["cams_path"], class_index_path=tree["cidx_path"],
               a2d2_subset=dict(unused_index=[], zero_size_index=[], split_bounds=[4, 6]), imagenet_pretrained=False,
               n_threads=0, gpu="0", print_frequency=1, **kw)
    cfg["PVconfig"].update(proj_h=64, proj_w=128, proj_ht=64, proj_wt=128)
    path = str(tmp_path / "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def _task_modules(monkeypatch, task, names):
    monkeypatch.syspath_prepend(task)
    for m in names:
        monkeypatch.delitem(sys.modules, m, raising=False)


def test_tasks_epmf_trains_on_a2d2(tree, tmp_path, monkeypatch):
    """two training iterations and one validation pass of tasks/epmf with dataset a2d2, at 39 classes on 64 x 128"""
    from pmf_amd.checkpoint import Recorder
    from pmf_amd.dataset.a2d2 import A2D2_PV
    from pmf_amd.models import EPMFNet
    from pmf_amd.utils.detinit import deterministic_init
    task = os.path.join(ROOT, "tasks", "epmf")
    path = _task_config(tree, tmp_path, os.path.join(task, "config_server_a2d2.yaml"), save_path=str(tmp_path / "exp"),
                        batch_size=[2, 2], n_epochs=2)
    _task_modules(monkeypatch, task, ("option", "trainer", "main"))
    import option
    import trainer
    s = option.Option(path)
    assert s.dataset == "a2d2" and s.nclasses == 39
    torch.manual_seed(s.seed)
    np.random.seed(s.seed)
    model = deterministic_init(EPMFNet(5, 3, s.nclasses, s.base_channels, imagenet_pretrained=False,
                                       image_backbone=s.img_backbone))
    t = trainer.Trainer(s, model, Recorder(s, s.save_path, use_tensorboard=False))
    assert isinstance(t.train_loader.dataset.dataset, A2D2_PV) and t.train_loader.dataset.is_train
    assert len(t.train_loader) == 2 and len(t.val_loader) == 1 and t.ignore_class == [0]
    assert t.mapped_cls_name[1] == "car" and t.alpha.shape == (39,) and t.alpha[0] == 0
    before = sum(float(p.detach().double().sum()) for p in model.parameters())
    res = t.run(0, mode="Train")
    assert t.engine.iteration == 2 and np.isfinite(t.last_summary["Loss"])
    after = sum(float(p.detach().double().sum()) for p in model.parameters())
    assert np.isfinite(after) and after != before
    res = t.run(0, mode="Validation")
    assert np.isfinite(t.last_summary["Loss"]) and all(v == v for v in res.values())
    for m in ("option", "trainer", "main"):
        sys.modules.pop(m, None)


def test_tasks_epmf_eval_a2d2_confusion_matrix(tree, tmp_path, monkeypatch):
    """tasks/epmf_eval_a2d2/infer.py: its confusion matrix equals IOUEval fed with torch's argmax of the same logits"""
    from pmf_amd.metrics import IOUEval
    from pmf_amd.utils.detinit import deterministic_init
    task = os.path.join(ROOT, "tasks", "epmf_eval_a2d2")
    pre = tmp_path / "trained"
    (pre / "checkpoint").mkdir(parents=True)
    path = _task_config(tree, tmp_path, os.path.join(task, "config.yaml"), pretrained_path=str(pre), experiment_id="t")
    _task_modules(monkeypatch, task, ("option", "infer"))
    import option
    import infer
    s = option.Option(path)
    torch.save(deterministic_init(infer.init_model(s)).state_dict(), s.pretrained_model)
    exp = infer.Experiment(s)
    kept = []
    exp.inference.run(keep_outputs=kept)
    assert len(kept) == 2 == len(exp.inference.val_loader)                       # the test split of the synthetic tree
    ev = IOUEval(n_classes=39, device=torch.device("cuda"), ignore=[0])
    for item, pred in kept:
        assert item.shape == (10, 64, 128) and pred.shape == (1, 39, 64, 128)
        ev.addBatch(pred.argmax(dim=1), item[9].long()[None])
    conf = exp.inference.evaluator.conf_matrix
    assert int(conf.sum()) == 2 * 64 * 128 and torch.equal(conf, ev.conf_matrix)
    assert torch.equal(exp.inference.evaluator.getIoU()[1], ev.getIoU()[1])
    with open(os.path.join(s.save_path, "log", "console.log")) as f:
        log = f.read()
    for line in ("Pixel-wise Evaluation Results", "fwIoU", "ACC matrix", "Recall matrix", "Data Distribution", "rain_dirt"):
        assert line in log
    # is_debug: one frame; has_label false: no confusion at all
    s.is_debug = True
    kept = []
    exp.inference.run(keep_outputs=kept)
    assert len(kept) == 1 and int(exp.inference.evaluator.conf_matrix.sum()) == 64 * 128
    for m in ("option", "infer"):
        sys.modules.pop(m, None)
