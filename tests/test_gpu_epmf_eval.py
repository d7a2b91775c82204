"""EPMF evaluation on the MI355X: the three per-frame HIP passes (csrc/eval.hip) against the torch sequence of the
reference's tasks/epmf_eval_semantickitti/infer.py, and the task end to end on a synthetic SemanticKITTI tree."""
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

pytestmark = pytest.mark.gpu

MEAN = [12.12, 10.88, 0.23, -1.04, 0.21]
STDS = [12.32, 11.47, 6.91, 0.86, 0.16]
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _torch_pre(proj):
    """the reference's per-frame torch sequence (infer.py: clone / eq / ZeroPad2d / normalise * mask), on the CPU"""
    input_feature = proj[None, :8].clone()
    proj_depth = input_feature[0, 0, ...].clone()
    proj_depth = proj_depth - proj_depth.eq(0).float()
    h_pad = math.ceil(input_feature.size(2) / 64.0) * 64 - input_feature.size(2)
    w_pad = math.ceil(input_feature.size(3) / 64.0) * 64 - input_feature.size(3)
    pad = torch.nn.ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, h_pad // 2, h_pad - h_pad // 2))
    input_feature = pad(input_feature)
    input_mask = pad(proj[None, 8])
    fm = torch.tensor(MEAN).view(1, -1, 1, 1)
    fs = torch.tensor(STDS).view(1, -1, 1, 1)
    input_feature[:, 0:5] = (input_feature[:, 0:5] - fm) / fs * input_mask.unsqueeze(1).expand_as(input_feature[:, 0:5])
    return input_feature[:, 0:5], input_feature[:, 5:8], proj_depth, (h_pad // 2, w_pad // 2)


def _random_proj(seed, h, w, nclasses=20):
    g = _rng(seed)
    mask = (g.random((h, w)) < 0.4).astype(np.float32)
    proj = np.zeros((10, h, w), np.float32)
    proj[0] = g.uniform(0.5, 80, (h, w)) * mask
    proj[1:4] = g.normal(0, 20, (3, h, w)) * mask
    proj[4] = g.random((h, w)) * mask
    proj[5:8] = g.random((3, h, w))
    proj[8] = mask
    proj[9] = g.integers(0, nclasses, (h, w)) * mask
    return torch.from_numpy(proj)


@pytest.mark.parametrize("h,w", [(37, 101), (64, 128), (1, 1)])
def test_pre_matches_torch_sequence_exactly(h, w):
    from pmf_amd.postproc.frame_eval import FrameEvaluator
    proj = _random_proj(h * 1000 + w, h, w)
    fe = FrameEvaluator(20, MEAN, STDS)
    pcd, rgb = fe.pre(proj.cuda())
    rp, rr, rd, (top, left) = _torch_pre(proj)
    assert fe.geometry == (rp.shape[2], rp.shape[3], top, left)
    assert torch.equal(pcd.cpu(), rp) and torch.equal(rgb.cpu(), rr) and torch.equal(fe.proj_depth.cpu(), rd)


def _prob_case(seed, C, H, W, nan=True):
    g = _rng(seed)
    prob = g.random((C, H, W)).astype(np.float32)
    # planted ties: the maximum copied to a lower and a higher class; NaNs (torch.argmax: a NaN wins)
    am = prob.argmax(0)
    ys, xs = g.integers(0, H, 300), g.integers(0, W, 300)
    for y, x in zip(ys, xs):
        other = int(g.integers(0, C))
        prob[other, y, x] = prob[am[y, x], y, x]
    if nan:
        ys, xs = g.integers(0, H, 40), g.integers(0, W, 40)
        prob[g.integers(0, C, 40), ys, xs] = np.nan
    return torch.from_numpy(prob)


def _np_conf(pred, gt, C, base=None):
    pred, gt = np.asarray(pred, np.int64).reshape(-1), np.asarray(gt, np.int64).reshape(-1)
    ok = (gt >= 0) & (gt < C)
    c = np.bincount(pred[ok] * C + gt[ok], minlength=C * C).reshape(C, C)
    return c if base is None else c + base


# (C, H, W, top, left, h, w): unaligned windows (odd offsets, w % 4 != 0), an aligned full map, W % 4 == 0 with an odd left
WINDOWS = [(20, 70, 133, 3, 5, 61, 123), (6, 64, 128, 0, 0, 64, 128), (20, 64, 192, 13, 1, 40, 190),
           (6, 64, 64, 31, 31, 1, 1), (6, 128, 256, 2, 7, 100, 246)]


@pytest.mark.parametrize("case", WINDOWS)
def test_window_argmax_and_pixel_confusion_exact(case):
    from pmf_amd.postproc.frame_eval import window_argmax
    C, H, W, top, left, h, w = case
    prob = _prob_case(sum(case), C, H, W)
    g = _rng(7 + C)
    label = g.integers(0, C + 1, (h, w)).astype(np.float32)           # C: outside the class range, not counted
    base = g.integers(0, 50, (C, C)).astype(np.int64)
    conf = torch.from_numpy(base.copy()).cuda()
    am = window_argmax(prob.cuda(), top, left, h, w, torch.from_numpy(label).cuda(), conf)
    ref = prob[:, top:top + h, left:left + w].argmax(0)
    assert torch.equal(am.cpu().long(), ref)
    assert np.array_equal(conf.cpu().numpy(), _np_conf(ref.numpy(), label, C, base))
    # map only / confusion only
    assert torch.equal(window_argmax(prob.cuda(), top, left, h, w).cpu().long(), ref)
    conf2 = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    assert window_argmax(prob.cuda(), top, left, h, w, torch.from_numpy(label).cuda(), conf2, want_map=False) is None
    assert np.array_equal(conf2.cpu().numpy(), _np_conf(ref.numpy(), label, C))


def _points_case(seed, h, w, K, P, C, nlut=300):
    """kept points of a box: int32 truncated coordinates (negative ones included), the box corner, sources in file
    order, raw labels of the whole cloud, a label lut and an inverse lut"""
    g = _rng(seed)
    x_min, y_min = int(g.integers(-20, 5)), int(g.integers(-20, 5))
    xd = (g.integers(0, h, K) + x_min).astype(np.int32)
    yd = (g.integers(0, w, K) + y_min).astype(np.int32)
    xd[0], yd[0] = x_min, y_min                        # the box corner is attained, as in the loader
    xd[1], yd[1] = x_min + h - 1, y_min + w - 1
    src = np.sort(g.choice(P, K, replace=False)).astype(np.int32)
    sem = g.integers(0, nlut + 20, P).astype(np.int32)           # some raw ids beyond the lut: class 0
    lut = g.integers(0, C, nlut).astype(np.int32)
    lut_inv = g.integers(0, 2 ** 31 - 1, C + 3).astype(np.int32)
    lut_inv[1] = -5                                    # uint32 bit pattern 0xFFFFFFFB
    depth = g.uniform(0.5, 80, K).astype(np.float32)
    return xd, yd, x_min, y_min, src, sem, lut, lut_inv, depth


def _points_ref(prob, top, left, h, w, xd, yd, x_min, y_min, src, sem, lut, lut_inv, C, knn_from=None):
    am = prob[:, top:top + h, left:left + w].argmax(0)
    ux = torch.from_numpy(xd).long() - x_min
    uy = torch.from_numpy(yd).long() - y_min
    if knn_from is None:
        pred = am[ux, uy].numpy()
    else:
        from pmf_amd.postproc import KNN
        proj_range, depth = knn_from
        pred = KNN(KNN_PARAMS, C)(proj_range.cuda(), depth.cuda(), am.cuda(), uy.cuda(), ux.cuda()).cpu().numpy()
    t = np.where(sem[src] < lut.shape[0], lut[np.minimum(sem[src], lut.shape[0] - 1)], 0)
    return pred, _np_conf(pred, t, C), lut_inv.view(np.uint32)[pred]


@pytest.mark.parametrize("use_knn", [False, True])
@pytest.mark.parametrize("case", [(20, 70, 133, 3, 5, 61, 123, 3000, 5000), (6, 64, 128, 0, 0, 64, 128, 2000, 2000)])
def test_point_labels_and_confusion_exact(case, use_knn):
    from pmf_amd.postproc.frame_eval import point_labels, window_argmax
    from pmf_amd.postproc.knn import inverse_gaussian_window
    C, H, W, top, left, h, w, K, P = case
    prob = _prob_case(sum(case) + 1, C, H, W, nan=not use_knn)
    xd, yd, x_min, y_min, src, sem, lut, lut_inv, depth = _points_case(K + C, h, w, K, P, C)
    g = _rng(K)
    proj_range = np.where(g.random((h, w)) < 0.5, g.uniform(0.5, 80, (h, w)), -1.0).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    conf = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    kw = {}
    if use_knn:
        kw = dict(argmax=window_argmax(prob.cuda(), top, left, h, w), proj_range=t(proj_range), unproj_range=t(depth),
                  knn=(5, 5, inverse_gaussian_window(5, 1.0).cuda(), 1.0))
    labels, labels_inv = point_labels(prob.cuda(), top, left, h, w, t(xd), t(yd), x_min, y_min, sem=t(sem), src=t(src),
                                      lut=t(lut), conf=conf, lut_inv=t(lut_inv), **kw)
    pred, rconf, rinv = _points_ref(prob, top, left, h, w, xd, yd, x_min, y_min, src, sem, lut, lut_inv, C,
                                    (torch.from_numpy(proj_range), torch.from_numpy(depth)) if use_knn else None)
    assert np.array_equal(labels.cpu().numpy(), pred)
    assert np.array_equal(conf.cpu().numpy(), rconf)
    assert np.array_equal(labels_inv.cpu().numpy().view(np.uint32), rinv)


def test_kitti_sized_frame_all_passes_match_torch():
    """one 376 x 1241 frame with 120 k kept points through (a) - (c), against torch (no network)"""
    from pmf_amd.postproc.frame_eval import FrameEvaluator
    h, w, K, P, C = 376, 1241, 120000, 124000, 20
    proj = _random_proj(11, h, w, C)
    xd, yd, x_min, y_min, src, sem, lut, lut_inv, depth = _points_case(12, h, w, K, P, C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    extra = dict(x_data=t(xd), y_data=t(yd), x_min=x_min, y_min=y_min, src=t(src), sem=t(sem), lut=t(lut))
    rp, rr, rd, _ = _torch_pre(proj)
    for params in (None, KNN_PARAMS):
        fe = FrameEvaluator(C, MEAN, STDS, params)
        pcd, rgb = fe.pre(proj.cuda())
        assert torch.equal(pcd.cpu(), rp) and torch.equal(rgb.cpu(), rr) and torch.equal(fe.proj_depth.cpu(), rd)
        H, W, top, left = fe.geometry
        prob = torch.softmax(torch.from_numpy(_rng(13).normal(0, 2, (1, C, H, W)).astype(np.float32)), 1)
        pix = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        pts = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        labels, inv = fe.post(prob.cuda(), t(depth), extra, pix, pts, t(lut_inv), want_labels=True)
        am = prob[0, :, top:top + h, left:left + w].argmax(0)
        assert np.array_equal(pix.cpu().numpy(), _np_conf(am.numpy(), proj[9].numpy(), C))
        pred, rconf, rinv = _points_ref(prob[0], top, left, h, w, xd, yd, x_min, y_min, src, sem, lut, lut_inv, C,
                                        (rd, torch.from_numpy(depth)) if params else None)
        assert np.array_equal(labels.cpu().numpy(), pred)
        assert np.array_equal(pts.cpu().numpy(), rconf)
        assert np.array_equal(inv.cpu().numpy().view(np.uint32), rinv)


# ---- the task end to end -----------------------------------------------------------------------------------------------
def _frames(root, data, M):
    """replace the tree's sweeps by clouds whose yaw-cropped box stays small (the raw synthetic sweeps reach the camera
    plane: boxes of ~1000 x 250 pixels): two point distributions that pad to different shapes, points outside the yaw
    crop (dropped by the keep mask) and points above the image (negative truncated rows)"""
    out = {}
    for i, key in enumerate(sorted(data)):
        g = _rng(100 + i)
        n = 2500 + 100 * i
        X = g.uniform(6 if i != 1 else 3, 40, n)
        Y = g.uniform(-1, 1, n) * (0.9 if i == 1 else 0.35) * X
        Z = g.uniform(-2.5, 1.5, n) * (1.5 if i == 1 else 1.0)
        pts = np.stack([X, Y, Z, g.random(n)], 1).astype(np.float32)
        out_of_fov = np.stack([g.uniform(-30, -2, 200), g.uniform(-20, 20, 200), g.uniform(-2, 1, 200), g.random(200)], 1)
        pts = np.concatenate([pts, out_of_fov.astype(np.float32)])[g.permutation(n + 200)]
        ids = [0, 1, 10, 11, 13, 30, 40, 44, 48, 50, 70, 72, 80, 252, 259]
        raw = ((g.integers(0, 300, pts.shape[0]).astype(np.uint32) << 16) |
               g.choice(ids, pts.shape[0]).astype(np.uint32))
        seq, fr = key
        pts.tofile(os.path.join(root, seq, "velodyne", fr + ".bin"))
        raw.tofile(os.path.join(root, seq, "labels", fr + ".label"))
        out[key] = (pts, raw, data[key][2])
    return out


def _parse_tables(out, n):
    """the confusion matrices of the report (point-wise first, pixel-wise second)"""
    lines = out.splitlines()
    mats = []
    for k, ln in enumerate(lines):
        if "confusion matrix original data" in ln:
            rows = []
            for row in lines[k + 1:]:
                f = [x.strip() for x in row.split("|")]
                if len(f) == n + 1 and f[0].isdigit():
                    rows.append([int(x) for x in f[1:]])
                    if len(rows) == n:
                        break
            mats.append(np.array(rows, np.int64))
    return mats


def _miou(conf):
    c = conf.astype(np.float64).copy()
    c[0] = 0
    c[:, 0] = 0
    tp = np.diag(c)
    iou = tp / (c.sum(1) + c.sum(0) - tp + 1e-15)
    return iou[1:].mean()


def test_epmf_eval_task_end_to_end(tmp_path):
    import yaml
    from oracle.cases import kitti_tree
    from oracle import loader_v2_ref, knn_ref
    from oracle import epmf_torch as E
    from pmf_amd.models import EPMFNet
    from pmf_amd.utils.detinit import deterministic_init
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    from tests import gpu_helpers as G
    root = str(tmp_path / "sequences")
    cfg_path, data = kitti_tree(root, seqs=(8,), frames=3, npts=100, h=48, w=160)
    ds = SemanticKitti(root, [8], cfg_path)
    M = ds.proj_matrix["08"]
    data = _frames(root, data, M)
    C = 6
    model_dir = tmp_path / "model"
    os.makedirs(model_dir / "checkpoint")
    sd = deterministic_init(EPMFNet(5, 3, C, 32, False, "resnet34")).state_dict()
    torch.save(sd, str(model_dir / "checkpoint" / "best_IOU_model.pth"))
    task = os.path.join(ROOT, "tasks", "epmf_eval_semantickitti")
    with open(os.path.join(task, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(pretrained_path=str(model_dir), data_root=root, data_config_path=cfg_path, sequences={"valid": [8]},
               nclasses=C, n_threads=0, save_preds=True, has_label=True, print_frequency=1)
    env = dict(os.environ, PMF_AUTOTUNE="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    runs = {}
    for use_knn in (False, True):
        cfg["post"]["KNN"]["use"] = use_knn
        cfg["experiment_id"] = "knn" if use_knn else "gather"
        conf_file = str(tmp_path / ("cfg_%d.yaml" % use_knn))
        with open(conf_file, "w") as f:
            yaml.safe_dump(cfg, f)
        dump = str(tmp_path / ("probs_%d" % use_knn))
        r = subprocess.run([sys.executable, "infer.py", conf_file, "--dump-probs", dump], cwd=task, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "Point-wise Evaluation Results" in r.stdout and "Pixel-wise Evaluation Results" in r.stdout
        shapes = set(re.findall(r"padded shape (\d+)x(\d+)", r.stdout))
        assert len(shapes) >= 2, r.stdout[-3000:]
        save = os.path.join(str(model_dir), "Eval-SemanticKitti-PMFNet-best_IOU_model-%s-%s" % (
            "KNN-5" if use_knn else "noKNN", cfg["experiment_id"]))
        runs[use_knn] = (r.stdout, save, dump)
    with open(cfg_path) as f:
        inv_ids = set(yaml.safe_load(f)["learning_map_inv"].values())
    lut, lut_inv = ds.class_map_lut, ds.class_map_lut_inv
    probs = {}
    for use_knn, (out, save, dump) in runs.items():
        pix = np.zeros((C, C), np.int64)
        pts_conf = np.zeros((C, C), np.int64)
        for key in sorted(data):
            pts, raw, img = data[key]
            sem = (raw & 0xFFFF).astype(np.int32)
            proj, xy, depth, keep = loader_v2_ref.project_frame_v2(pts, sem, img, M, lut)
            _, h, w = proj.shape
            prob = np.load(os.path.join(dump, "%s_%s.npy" % key))
            H, W = prob.shape[1:]
            top, left = (H - h) // 2, (W - w) // 2
            assert (H, W) == (math.ceil(h / 64.0) * 64, math.ceil(w / 64.0) * 64)
            probs.setdefault(key, (proj, prob))
            am = prob[:, top:top + h, left:left + w].argmax(0)
            xi, yi = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
            ux, uy = xi - xi.min(), yi - yi.min()
            if use_knn:
                pd = proj[0] - (proj[0] == 0).astype(np.float32)
                pred = knn_ref.knn_vote(pd, depth, am, uy, ux, nclasses=C, **KNN_PARAMS)
            else:
                pred = am[ux, uy]
            got = np.fromfile(os.path.join(save, "preds", "sequences", key[0], "predictions", key[1] + ".label"),
                              dtype=np.uint32)
            assert got.shape[0] == int(keep.sum()) and set(np.unique(got)) <= inv_ids
            assert np.array_equal(got, lut_inv[pred].astype(np.uint32))
            pix = _np_conf(am, proj[9].astype(np.int64), C, pix)
            pts_conf = _np_conf(pred, lut[sem[keep]], C, pts_conf)
        pt_tab, px_tab = _parse_tables(out, C)
        for tab, ref in ((pt_tab, pts_conf), (px_tab, pix)):
            ref = ref.copy()
            ref[0] = 0
            ref[:, 0] = 0
            assert np.array_equal(tab, ref)
        m = re.search(r"Point-wise Evaluation Results.*?IOU avg: ([0-9.]+)", out, re.S)
        assert m and m.group(1) == "{:.4f}".format(_miou(pts_conf))
    # forward precision on the padded frames (the existing EPMF bar), separately from the exact post path
    ref = E.EPMFNet(5, 3, C, 32, False, "resnet34")
    ref.load_state_dict(sd)
    ref.eval()
    for key, (proj, prob) in probs.items():
        pcd, rgb, _, _ = _torch_pre(torch.from_numpy(proj))
        with torch.no_grad():
            rl, _ = ref(pcd, rgb)
        assert G.rel_err(prob, rl[0].numpy()) < 1e-4, key
