"""EPMF evaluation on nuScenes on the MI355X: the V2 loader on a NuscenesV2-type dataset against the reference loader's
recorded output (tests/golden/g16_nus_v2.npz, written by tools/make_golden_nus_v2.py: the reference's own
PerspectiveViewLoaderV2 executed on tests/nus_v2_cases.SyntheticNusV2), the per-view merge and the per-sweep finish
(csrc/eval.hip) against the torch / numpy composition of the reference's tasks/epmf_eval_nuscenes/infer.py, and the task
end to end.  Everything is exact except the forward-precision bar of the end-to-end test (the existing EPMF bar)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import nus_v2_cases as N  # noqa: E402
from tests.test_gpu_epmf_eval import WINDOWS, _parse_tables, _miou  # noqa: E402

pytestmark = pytest.mark.gpu

PV = {"PVconfig": {"proj_h": 64, "proj_w": 128, "proj_ht": 64, "proj_wt": 128, "img_jitter": [0.4, 0.4, 0.4],
                   "pcd_mean": N.MEAN, "pcd_stds": N.STDS}}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- loader ------------------------------------------------------------------------------------------------------------
def test_loader_on_nuscenes_v2_dataset_equals_reference_loader():
    from pmf_amd.dataset.perspective_view_loader_v2 import PerspectiveViewLoaderV2
    gold = np.load(N.GOLDEN)
    ds = N.SyntheticNusV2()
    ld = PerspectiveViewLoaderV2(ds, PV, is_train=False, return_uproj=True)
    assert len(ld) == 12
    for i in range(len(ld)):
        proj, xy, depth, keep, pc = ld[i]
        assert proj.dtype == torch.float32 and xy.dtype == torch.float64 and depth.dtype == torch.float32
        assert keep.dtype == torch.bool
        for name, got in (("proj", proj), ("xy", xy), ("depth", depth), ("keep", keep)):
            ref = gold["v%d.%s" % (i, name)]
            assert tuple(got.shape) == ref.shape, (i, name)
            assert np.array_equal(got.cpu().numpy(), ref), (i, name)           # bit-exact, last-writer order included
        assert np.array_equal(pc.numpy(), ds.loadDataByIndex(i)[0])
        p2, xy2, d2, k2, extra = ld._eval_item(i)
        assert torch.equal(p2, proj) and torch.equal(xy2, xy) and torch.equal(d2, depth) and torch.equal(k2, keep)
        g = N.view_geometry(ds, i)
        assert np.array_equal(extra["x_data"].cpu().numpy(), g[3]) and np.array_equal(extra["y_data"].cpu().numpy(), g[4])
        assert (extra["x_min"], extra["y_min"]) == (g[5], g[6])
        assert np.array_equal(extra["src"].cpu().numpy(), np.flatnonzero(g[2]))
        assert extra["src"].dtype == extra["sem"].dtype == extra["lut"].dtype == torch.int32
        assert np.array_equal(extra["sem"].cpu().numpy(), ds.loadDataByIndex(i)[1].reshape(-1))
        assert extra["lut"].shape[0] == 256
        raw = np.arange(32, dtype=np.uint8)[:, None]
        assert np.array_equal(extra["lut"].cpu().numpy()[:32], ds.labelMapping(raw))


# ---- pmf_eval_view_merge -------------------------------------------------------------------------------------------------
def _view_points(g, h, w, K, P):
    x_min, y_min = int(g.integers(-20, 5)), int(g.integers(-20, 5))
    xd = (g.integers(0, h, K) + x_min).astype(np.int32)
    yd = (g.integers(0, w, K) + y_min).astype(np.int32)
    xd[0], yd[0] = x_min, y_min
    xd[1], yd[1] = x_min + h - 1, y_min + w - 1
    src = np.sort(g.choice(np.arange(16, P), K, replace=False)).astype(np.int32)     # points 0..15 are planted by hand
    depth = g.uniform(0.5, 80, K).astype(np.float32)
    return xd, yd, x_min, y_min, src, depth


def _six_views(seed, C, H, W, top, left, h, w, P, gather):
    """six views of one window geometry with the planted cases: coarse probabilities (confidence ties between views are
    frequent) + views 0 and 3 share the map and give point 3 the same pixel (exact tie: view 0 wins); point 4 is seen by
    view 2 only, at a pixel where class 0 is the maximum; point 5's pixel in view 1 holds a NaN (does not win against view
    0's finite confidence, nor against the zero state for point 6); class ties inside a pixel (lowest class)."""
    g = _rng(seed)
    K = min(max(h * w // 3, 2), P // 3)
    views = []
    for v in range(6):
        prob = (np.round(g.random((C, H, W)) * 16) / 16).astype(np.float32)
        am = prob.argmax(0)
        for y, x in zip(g.integers(0, H, 200), g.integers(0, W, 200)):
            prob[int(g.integers(0, C)), y, x] = prob[am[y, x], y, x]              # class ties
        if v == 3:
            prob = views[0][0].copy()
        xd, yd, x_min, y_min, src, depth = _view_points(g, h, w, K, P)
        pr = np.where(g.random((h, w)) < 0.5, g.uniform(0.5, 80, (h, w)), -1.0).astype(np.float32)
        views.append([prob, xd, yd, x_min, y_min, src, depth, pr])

    def put(v, p, r, c):
        prob, xd, yd, x_min, y_min, src, depth, pr = views[v]
        views[v][1] = np.append(xd, np.int32(x_min + r))
        views[v][2] = np.append(yd, np.int32(y_min + c))
        views[v][5] = np.append(src, np.int32(p))
        views[v][6] = np.append(depth, np.float32(7.5))
    r0, c0 = h // 2, w // 2
    put(0, 3, r0, c0); put(3, 3, r0, c0)
    views[0][0][:, top + r0, left + c0] = 0.25
    views[0][0][2, top + r0, left + c0] = 0.75
    views[3][0] = views[0][0].copy()
    views[3][0][:, top + r0, left + c0] = 0.25
    views[3][0][4, top + r0, left + c0] = 0.75             # the same confidence, another class, later view: loses
    put(2, 4, 0, 0)
    views[2][0][:, top, left] = 0.125
    views[2][0][0, top, left] = 0.875
    put(0, 5, h - 1, w - 1); put(1, 5, h - 1, w - 1); put(1, 6, h - 1, w - 1)
    views[0][0][:, top + h - 1, left + w - 1] = 0.0625
    views[0][0][1, top + h - 1, left + w - 1] = 0.5
    if gather:
        views[1][0][3, top + h - 1, left + w - 1] = np.nan
    for v in views:                                        # file order, as a keep mask lists the points
        o = np.argsort(v[5], kind="stable")
        v[1], v[2], v[5], v[6] = v[1][o], v[2][o], v[5][o], v[6][o]
    return views


def _reference_merge(views, C, top, left, h, w, P, use_knn):
    """infer.py:140-173: prob.max(0), the KNN module for both maps (or the gather), the boolean-mask merge on the host"""
    from pmf_amd.postproc import KNN
    conf_full, label_full = np.zeros(P, np.float32), np.zeros(P, np.int32)
    knn = KNN(N.KNN_PARAMS, C)
    for prob, xd, yd, x_min, y_min, src, depth, pr in views:
        win = torch.from_numpy(prob)[:, top:top + h, left:left + w].cuda()
        pred_conf, pred_argmax = win.max(dim=0)
        ux = _t(xd).long() - x_min
        uy = _t(yd).long() - y_min
        if use_knn:
            lab = knn(_t(pr), _t(depth), pred_argmax, uy, ux)
            cf = knn(_t(pr), _t(depth), pred_conf, uy, ux)
        else:
            lab, cf = pred_argmax[ux, uy], pred_conf[ux, uy]
        keep = np.zeros(P, bool)
        keep[src] = True
        N.merge_mask_form(conf_full, label_full, keep, cf.cpu().numpy(), lab.cpu().numpy())
    return conf_full, label_full


@pytest.mark.parametrize("use_knn", [False, True])
@pytest.mark.parametrize("case", WINDOWS + [(17, 128, 192, 0, 31, 84, 130)])            # + a bottom-padded view
def test_view_merge_matches_reference_composition(case, use_knn):
    from pmf_amd.postproc.frame_eval import view_merge, window_argmax
    from pmf_amd.postproc.knn import inverse_gaussian_window
    C, H, W, top, left, h, w = case
    P = 6000
    views = _six_views(sum(case) + use_knn, C, H, W, top, left, h, w, P, gather=not use_knn)
    conf_full = torch.zeros(P, dtype=torch.float32, device="cuda")
    label_full = torch.zeros(P, dtype=torch.int32, device="cuda")
    wgt = inverse_gaussian_window(5, 1.0).cuda()
    for prob, xd, yd, x_min, y_min, src, depth, pr in views:
        p = _t(prob)
        kw = {}
        if use_knn:
            kw = dict(argmax=window_argmax(p, top, left, h, w), proj_range=_t(pr), unproj_range=_t(depth),
                      knn=(5, 5, wgt, 1.0))
        view_merge(p, top, left, h, w, _t(xd), _t(yd), x_min, y_min, _t(src), conf_full, label_full, **kw)
    rc, rl = _reference_merge(views, C, top, left, h, w, P, use_knn)
    assert np.array_equal(conf_full.cpu().numpy(), rc)
    assert np.array_equal(label_full.cpu().numpy(), rl)
    if h * w > 1:
        got = label_full.cpu().numpy()
        assert got[0] == 0 and rc[0] == 0                                   # unseen
        if not use_knn:
            assert got[3] == 2 and rc[3] == np.float32(0.75)                # tie between views: the first
            assert got[4] == 0 and rc[4] == np.float32(0.875)               # one view only, class 0
            assert got[5] == 1 and rc[5] == np.float32(0.5)                 # NaN does not win
            assert got[6] == 0 and rc[6] == 0                               # ... not even against the zero state


# ---- pmf_eval_sweep_finish -----------------------------------------------------------------------------------------------
def _finish_ref(label_full, sem, lut, C, base):
    pred = label_full.astype(np.int64)
    valid = pred != 0
    gt = np.where(sem < lut.shape[0], lut[np.minimum(sem, lut.shape[0] - 1)], 0) * valid
    return pred.astype(np.uint8), N.np_conf(pred, gt, C, base)


def test_sweep_finish_labels_confusion_and_zeroed_state():
    from pmf_amd.postproc.frame_eval import sweep_finish
    C, P = 17, 34720
    g = _rng(5)
    lab = g.integers(0, C, P).astype(np.int32)
    lab[g.random(P) < 0.1] = 0
    cf = g.random(P).astype(np.float32)
    sem = g.integers(0, 300, P).astype(np.int32)                           # raw ids beyond the 256-entry table: class 0
    lut = g.integers(0, C, 256).astype(np.int32)
    base = g.integers(0, 50, (C, C)).astype(np.int64)
    conf = _t(base.copy())
    conf_full, label_full = _t(cf), _t(lab)
    out = torch.full((P,), 255, dtype=torch.uint8, device="cuda")
    assert sweep_finish(conf_full, label_full, C, _t(sem), _t(lut), conf, out) is out
    ru8, rconf = _finish_ref(lab, sem, lut, C, base)
    assert np.array_equal(out.cpu().numpy(), ru8)
    assert np.array_equal(conf.cpu().numpy(), rconf)
    assert not conf_full.any().item() and not label_full.any().item()
    # labels only / confusion only
    label_full.copy_(_t(lab))
    out2 = torch.empty(P, dtype=torch.uint8, device="cuda")
    sweep_finish(conf_full, label_full, C, out_u8=out2)
    assert np.array_equal(out2.cpu().numpy(), ru8) and not label_full.any().item()


@pytest.mark.parametrize("use_knn", [False, True])
def test_sweep_evaluator_nuscenes_sized_sweep_and_reuse(use_knn):
    """34 720 points, six ~450 x 960 views, C = 17, random softmax maps (no network) through SweepEvaluator against the
    composition; then a smaller sweep through the SAME evaluator against a fresh one (the state was zeroed)."""
    from pmf_amd.postproc.frame_eval import SweepEvaluator, pad_geometry_bottom
    C = 17
    lut = _rng(1).integers(0, C, 256).astype(np.int32)

    def sweep(se, seed, P, hw, pix, pts):
        g = _rng(seed)
        sem = g.integers(0, 32, P).astype(np.int32)
        views = []
        for v in range(6):
            h, w = hw[v]
            H, W, top, left = pad_geometry_bottom(h, w)
            K = P // 4
            xd, yd, x_min, y_min, src, depth = _view_points(g, h, w, K, P)
            mask = (g.random((h, w)) < 0.4).astype(np.float32)
            proj = np.zeros((10, h, w), np.float32)
            proj[0] = g.uniform(0.5, 80, (h, w)) * mask
            proj[8] = mask
            proj[9] = g.integers(0, C, (h, w)) * mask
            prob = torch.softmax(torch.from_numpy(g.normal(0, 2, (C, H, W)).astype(np.float32)), 0).numpy()
            se.pre(_t(proj))
            assert se.geometry == (H, W, top, left)
            extra = dict(x_data=_t(xd), y_data=_t(yd), x_min=x_min, y_min=y_min, src=_t(src), sem=_t(sem), lut=_t(lut))
            se.post_view(_t(prob)[None], _t(depth), extra, pixel_conf=pix)
            pr = proj[0] - (proj[0] == 0).astype(np.float32)
            views.append(([prob, xd, yd, x_min, y_min, src, depth, pr], (top, left, h, w), proj[9]))
        assert se.views_in_sweep == 6
        out = se.finish(_t(sem), _t(lut), P, point_conf=pts).cpu().numpy()
        assert se.views_in_sweep == 0
        return out, sem, views

    def reference(sem, views, P):
        conf_full, label_full = np.zeros(P, np.float32), np.zeros(P, np.int32)
        pix = np.zeros((C, C), np.int64)
        for view, (top, left, h, w), label in views:
            rc, rl = _reference_merge([view], C, top, left, h, w, P, use_knn)
            keep = np.zeros(P, bool)
            keep[view[5]] = True
            N.merge_mask_form(conf_full, label_full, keep, rc[view[5]], rl[view[5]])
            am = view[0][:, top:top + h, left:left + w].argmax(0)
            pix = N.np_conf(am, label.astype(np.int64), C, pix)
        u8, pts = _finish_ref(label_full, sem, lut, C, np.zeros((C, C), np.int64))
        return u8, pts, pix

    se = SweepEvaluator(C, N.MEAN, N.STDS, N.KNN_PARAMS if use_knn else None)
    big = [(450, 960), (447, 955), (452, 958), (890, 1590), (449, 960), (440, 700)]
    small = [(40, 78), (44, 77), (43, 78), (84, 130), (43, 78), (41, 47)]
    for seed, P, hw in ((3, 34720, big), (4, 6000, small)):
        pix = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        pts = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        out, sem, views = sweep(se, seed, P, hw, pix, pts)
        u8, rpts, rpix = reference(sem, views, P)
        assert out.dtype == np.uint8 and np.array_equal(out, u8)
        assert np.array_equal(pts.cpu().numpy(), rpts) and np.array_equal(pix.cpu().numpy(), rpix)
        assert (u8 == 0).mean() > 0.05 and (u8 != 0).mean() > 0.3           # unseen points exist, most are labelled
    fresh = SweepEvaluator(C, N.MEAN, N.STDS, N.KNN_PARAMS if use_knn else None)
    pts2 = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    out2, _, _ = sweep(fresh, 4, 6000, small, None, pts2)
    assert np.array_equal(out2, out) and torch.equal(pts2, pts)
    with pytest.raises(RuntimeError):
        fresh.finish(_t(sem), _t(lut), 6000)                                # zero views


# ---- the task end to end -----------------------------------------------------------------------------------------------
DRIVER = """
import os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {task!r})
os.chdir({task!r})
from tests.nus_v2_cases import SyntheticNusV2
from option import Option
import infer
exp = infer.Experiment(Option(sys.argv[1]), dataset=SyntheticNusV2(nclasses={C}), dump_probs=sys.argv[2])
print("===init env success===")
exp.run()
"""


def _torch_pre_bottom(proj):
    """the reference's per-view torch sequence (infer.py:111-127), on the CPU"""
    x = proj[None, :8].clone()
    h_pad = math.ceil(x.size(2) / 64.0) * 64 - x.size(2)
    w_pad = math.ceil(x.size(3) / 64.0) * 64 - x.size(3)
    pad = torch.nn.ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, 0, h_pad))
    x = pad(x)
    m = pad(proj[None, 8])
    fm = torch.tensor(N.MEAN).view(1, -1, 1, 1)
    fs = torch.tensor(N.STDS).view(1, -1, 1, 1)
    x[:, 0:5] = (x[:, 0:5] - fm) / fs * m.unsqueeze(1).expand_as(x[:, 0:5])
    return x[:, 0:5], x[:, 5:8]


def test_epmf_eval_nuscenes_task_end_to_end(tmp_path):
    import yaml
    from oracle import epmf_torch as E
    from pmf_amd.models import EPMFNet
    from pmf_amd.utils.detinit import deterministic_init
    from tests import gpu_helpers as G
    C = 6
    ds = N.SyntheticNusV2(nclasses=C)
    gold = np.load(N.GOLDEN)
    model_dir = tmp_path / "model"
    os.makedirs(model_dir / "checkpoint")
    sd = deterministic_init(EPMFNet(5, 3, C, 32, False, "resnet34")).state_dict()
    torch.save(sd, str(model_dir / "checkpoint" / "best_IOU_model.pth"))
    task = os.path.join(ROOT, "tasks", "epmf_eval_nuscenes")
    with open(os.path.join(task, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(pretrained_path=str(model_dir), data_root="unused", nclasses=C, n_threads=0, save_pred_results=True,
               has_label=True, print_frequency=1, gpu="0")
    driver = str(tmp_path / "driver.py")
    with open(driver, "w") as f:
        f.write(DRIVER.format(root=ROOT, task=task, C=C))
    env = dict(os.environ, PMF_AUTOTUNE="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    lut = np.zeros(256, np.int64)
    lut[:32] = ds.labelMapping(np.arange(32, dtype=np.uint8)[:, None])
    probs = {}
    for use_knn in (False, True):
        cfg["post"]["KNN"]["use"] = use_knn
        cfg["experiment_id"] = "knn" if use_knn else "gather"
        conf_file = str(tmp_path / ("cfg_%d.yaml" % use_knn))
        with open(conf_file, "w") as f:
            yaml.safe_dump(cfg, f)
        dump = str(tmp_path / ("probs_%d" % use_knn))
        r = subprocess.run([sys.executable, driver, conf_file, dump], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out = r.stdout
        assert "Point-wise Evaluation Results" in out and "Pixel-wise Evaluation Results" in out
        assert len(set(re.findall(r"padded shape (\d+)x(\d+)", out))) >= 2, out[-3000:]
        save = os.path.join(str(model_dir), "Eval-nuScenes-PMFNet-best_IOU_model-%s-%s" % (
            "KNN-5" if use_knn else "noKNN", cfg["experiment_id"]))
        pix = np.zeros((C, C), np.int64)
        pts_conf = np.zeros((C, C), np.int64)
        for s in range(2):
            P = ds.loadDataByIndex(6 * s)[0].shape[0]
            sem = ds.loadDataByIndex(6 * s)[1].reshape(-1).astype(np.int64)
            conf_full, label_full = np.zeros(P, np.float32), np.zeros(P, np.int32)
            for v in range(6):
                i = 6 * s + v
                crop, xy, keep, xd, yd, x_min, y_min, h, w, H, W, left = N.view_geometry(ds, i)
                proj = gold["v%d.proj" % i][:9]                             # geometry channels do not depend on nclasses
                label = np.zeros((h, w), np.int64)
                label[xd - x_min, yd - y_min] = lut[sem[keep]]              # numpy fancy assignment: the last writer
                assert proj.shape[1:] == (h, w) and np.array_equal(gold["v%d.keep" % i], keep)
                prob = np.load(os.path.join(dump, "%d.npy" % i))
                assert prob.shape == (C, H, W)
                probs.setdefault(i, (proj, prob))
                win = prob[:, :h, left:left + w]
                ux, uy = xd.astype(np.int64) - x_min, yd.astype(np.int64) - y_min
                knn = None
                if use_knn:
                    knn = (proj[0] - (proj[0] == 0).astype(np.float32), gold["v%d.depth" % i], C)
                cf, lab = N.view_conf_label(win, ux, uy, knn)
                N.merge_mask_form(conf_full, label_full, keep, cf, lab.astype(np.int32))
                pix = N.np_conf(win.argmax(0), label, C, pix)
            got = np.fromfile(os.path.join(save, "preds", "lidarseg", "val", "sweep%03d_lidarseg.bin" % s), dtype=np.uint8)
            assert got.shape[0] == P and np.array_equal(got, label_full.astype(np.uint8))
            assert (got == 0).mean() >= 0.01                                # the points no camera keeps
            pts_conf = N.np_conf(label_full, lut[sem] * (label_full != 0), C, pts_conf)
        pt_tab, px_tab = _parse_tables(out, C)
        for tab, ref in ((pt_tab, pts_conf), (px_tab, pix)):
            ref = ref.copy()
            ref[0] = 0
            ref[:, 0] = 0
            assert np.array_equal(tab, ref)
        m = re.search(r"Point-wise Evaluation Results.*?IOU avg: ([0-9.]+)", out, re.S)
        assert m and m.group(1) == "{:.4f}".format(_miou(pts_conf))
    # forward precision on the padded views (the existing EPMF bar), separately from the exact post path
    ref = E.EPMFNet(5, 3, C, 32, False, "resnet34")
    ref.load_state_dict(sd)
    ref.eval()
    assert len(probs) == 12
    for i, (proj, prob) in probs.items():
        pcd, rgb = _torch_pre_bottom(torch.from_numpy(proj))
        with torch.no_grad():
            rl, _ = ref(pcd, rgb)
        assert G.rel_err(prob, rl[0].numpy()) < 1e-4, i
