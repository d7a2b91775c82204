"""PMF evaluation on SensatUrban on the MI355X: the three passes of csrc/bev_eval.hip and BevTileEvaluator against the
statements of tests/sensat_eval_cases.py (the reference's per-frame composition in torch CPU ops), bit for bit; the task end
to end; the batch-6 forward against six batch-1 forwards; and the task's default backbone against the oracle.

Shapes: frame 70 x 100 at S = 32 and 48 (three / two shifted, overlapping rows and columns, unaligned w_start, the 32 x 32
LDS block and its 16-pixel remainder), frame 40 x 52 at S = 48 (smaller than the tile in one dimension), C = 14."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import sensat_eval_cases as S  # noqa: E402
from tests.gpu_helpers import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

C = S.NCLASSES
SIZES = (32, 48)
_CACHE = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames():
    """the two synthetic frames (continuous heights), made once: [(name, frame, labels uint8[P], xyz)]"""
    if "frames" not in _CACHE:
        _CACHE["frames"] = [(name,) + S.make_frame(k, h, w, n)[:3] for k, (name, h, w, n) in enumerate(S.FRAMES)]
    return _CACHE["frames"]


def _stats():
    return (torch.tensor(S.MEAN, dtype=torch.float32).cuda(), torch.tensor(S.STD, dtype=torch.float32).cuda())


CASES = [(0, 32), (0, 48), (1, 48)]


@pytest.mark.parametrize("fi,size", CASES)
@pytest.mark.parametrize("tta", [False, True])
def test_tile_pre_is_the_reference_composition_bit_for_bit(fi, size, tta):
    from pmf_amd.postproc import bev_tile_pre, tile_windows
    _, frame, _, _ = _frames()[fi]
    fm = frame["feature_map"]
    wins = tile_windows(fm.shape[1], fm.shape[2], size)
    assert wins == S.windows_np(fm.shape[1], fm.shape[2], size)
    mean, stds = _stats()
    V = 6 if tta else 1
    pcd, rgb, pcd_pad, rgb_pad = bev_tile_pre(_t(fm).float(), mean, stds, [(a, c) for a, _, c, _ in wins], size, V, tta)
    T = len(wins)
    assert tuple(pcd.shape) == (T * V, 5, size, size) and tuple(rgb.shape) == (T * V, 3, size, size)
    pcd, rgb = pcd.cpu(), rgb.cpu()
    nonzero = 0
    for k, win in enumerate(wins):
        rp, rr = S.ref_tile_inputs(fm, win, size, tta=tta)
        for v in range(V):
            assert torch.equal(pcd[k * V + v], rp[v][0]), (k, v)
            assert torch.equal(rgb[k * V + v], rr[v][0]), (k, v)
        nonzero += int((rp[0] != 0).sum())
        if tta:
            assert torch.equal(pcd_pad[k].cpu(), rp[6][0]) and torch.equal(rgb_pad[k].cpu(), rr[6][0]), k
            border = pcd_pad[k].clone()
            border[:, 16:16 + size, 16:16 + size] = 0
            assert not border.any()
    assert nonzero > 1000


def _recipe_outputs(h, w, tta):
    """{(S, k): [model outputs of tile k]} by recipe, CPU tensors"""
    outs = {}
    for size in SIZES:
        wins = S.windows_np(h, w, size)
        p = torch.from_numpy(S.prob_recipe(7 * size + h, len(wins) * (6 if tta else 1), size))
        pp = torch.from_numpy(S.prob_recipe(11 * size + h, len(wins), size + 32)) if tta else None
        for k in range(len(wins)):
            outs[(size, k)] = [p[k * 6 + v][None] for v in range(6)] + [pp[k][None]] if tta else [p[k][None]]
    return outs


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("group", [64, 3])
def test_tile_accum_full_tile_list_bit_for_bit(fi, tta, group):
    """all sizes and tiles of a frame, in one call per size (group 64) or in groups of 3 tiles: overlaps, the partial window
    and the sum order make exact equality meaningful"""
    from pmf_amd.postproc import bev_tile_accum
    _, frame, _, _ = _frames()[fi]
    h, w = frame["feature_map"].shape[1:]
    outs = _recipe_outputs(h, w, tta)
    want = S.ref_confidence_map(h, w, SIZES, lambda size, k, win: outs[(size, k)])
    conf = torch.zeros(C, h, w, device="cuda")
    V = 6 if tta else 1
    for size in SIZES:
        wins = S.windows_np(h, w, size)
        for g in range(0, len(wins), group):
            ks = range(g, min(g + group, len(wins)))
            prob = torch.cat([torch.cat(outs[(size, k)][:V]) for k in ks]).cuda().contiguous()
            pad = torch.cat([outs[(size, k)][6] for k in ks]).cuda().contiguous() if tta else None
            bev_tile_accum(prob, [(wins[k][0], wins[k][2]) for k in ks], size, V, conf, pad)
    assert torch.equal(conf.cpu(), want)
    if fi == 1:                                                  # the frame is smaller than the 48 tile: nothing leaked
        assert want.shape[1] < 48 and float(want.min()) > 0


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("use_knn", [False, True])
@pytest.mark.parametrize("with_labels", [False, True])
def test_bev_points_labels_confusion_and_zero_count_exact(fi, use_knn, with_labels):
    from pmf_amd.postproc import KNN, bev_points
    from pmf_amd.postproc.frame_eval import window_argmax
    _, frame, labels, xyz = _frames()[fi]
    h, w = frame["feature_map"].shape[1:]
    conf_map = torch.from_numpy(S.prob_recipe(5 + fi, 1, max(h, w))[0, :, :h, :w].copy())
    ref = S.ref_finish(conf_map, frame, labels if with_labels else None, xyz[:, 2], S.KNN_PARAMS if use_knn else None)
    pix = frame["h_idx"] * w + frame["w_idx"]
    assert np.unique(pix).size < pix.size                                      # points sharing a pixel
    assert (ref["argmax"][frame["h_idx"], frame["w_idx"]] == 0).sum() > 10     # points on class-0 pixels
    amap = window_argmax(conf_map.cuda(), 0, 0, h, w)
    assert np.array_equal(amap.cpu().numpy(), ref["argmax"])
    h_idx, w_idx = _t(frame["h_idx"]), _t(frame["w_idx"])
    voted = None
    if use_knn:
        voted = KNN(S.KNN_PARAMS, C)(_t(frame["feature_map"][0]).float(), _t(xyz[:, 2].copy()), amap, w_idx, h_idx)
    pconf = torch.zeros(C, C, dtype=torch.int64, device="cuda") if with_labels else None
    nz = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = bev_points(amap, h_idx, w_idx, C, voted, _t(labels) if with_labels else None, pconf, nz)
    assert out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), (ref["pred"] - 1).astype(np.uint8))
    assert int(nz.item()) == ref["zero_num"] and (ref["zero_num"] > 0) == (not use_knn)
    if with_labels:
        assert np.array_equal(pconf.cpu().numpy(), ref["point_conf"]) and ref["point_conf"].sum() == labels.size
        out2 = bev_points(amap, h_idx, w_idx, C, voted, _t(labels), pconf, nz)   # accumulates
        assert torch.equal(out, out2) and np.array_equal(pconf.cpu().numpy(), 2 * ref["point_conf"])
        assert int(nz.item()) == 2 * ref["zero_num"]


def _small_model():
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    if "model" not in _CACHE:
        _CACHE["model"] = deterministic_init(PMFNet(5, 3, C, 16, False, "resnet34")).cuda().eval()
    return _CACHE["model"]


@pytest.mark.parametrize("tta,use_knn", [(False, False), (True, True)])
def test_evaluator_frame_end_to_end(tta, use_knn):
    """the captured per-tile probabilities fed through the statement reproduce the confidence map, the class map, both
    confusion matrices and the .label bytes exactly"""
    from pmf_amd.postproc import BevTileEvaluator
    ev = BevTileEvaluator(_small_model(), C, S.MEAN, S.STD, SIZES, tta=tta, knn_params=S.KNN_PARAMS if use_knn else None)
    assert ev.tile_batch == (1 if tta else 4)
    pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    want_pix, want_pts = np.zeros((C, C), np.int64), np.zeros((C, C), np.int64)
    for name, frame, labels, xyz in _frames():
        h, w = frame["feature_map"].shape[1:]
        cap = {}

        def capture(size, wins, prob, prob_pad, cap=cap, h=h, w=w):
            all_wins = S.windows_np(h, w, size)
            V = 6 if tta else 1
            assert prob.shape[0] == len(wins) * V
            for j, win in enumerate(wins):
                k = len([1 for key in cap if key[0] == size])
                assert all_wins[k] == win
                cap[(size, k)] = [prob[j * V + v][None].cpu() for v in range(V)] + \
                    ([prob_pad[j][None].cpu()] if tta else [])
        ev.capture = capture
        pred, conf_map, n_zero = ev.frame(frame, z=xyz[:, 2], label=labels, pixel_conf=pix, point_conf=pts)
        assert len(cap) == sum(len(S.windows_np(h, w, size)) for size in SIZES)
        want = S.ref_confidence_map(h, w, SIZES, lambda size, k, win: cap[(size, k)])
        assert torch.equal(conf_map.cpu(), want), name
        ref = S.ref_finish(want, frame, labels, xyz[:, 2], S.KNN_PARAMS if use_knn else None)
        assert np.array_equal(ev.class_map.cpu().numpy(), ref["argmax"])
        assert pred.dtype == torch.uint8 and np.array_equal(pred.cpu().numpy(), (ref["pred"] - 1).astype(np.uint8))
        assert n_zero == ref["zero_num"]
        want_pix += ref["pixel_conf"]
        want_pts += ref["point_conf"]
    assert np.array_equal(pix.cpu().numpy(), want_pix) and np.array_equal(pts.cpu().numpy(), want_pts)
    assert want_pts.sum() == sum(f[2].size for f in _frames())


def test_batch6_forward_equals_six_batch1_forwards():
    """eval-mode BatchNorm: batch elements are independent, so the six same-size variants may share a forward.  Both sides
    are the same fp32-class HIP path; the bar is the project's probability bar max|d| / max(|ref|, 1) <= 1e-3."""
    model = _small_model()
    _, frame, _, _ = _frames()[0]
    worst = 0.0
    for size in SIZES:
        rp, rr = S.ref_tile_inputs(frame["feature_map"], S.windows_np(70, 100, size)[1], size, tta=True)
        pcd, rgb = torch.cat(rp[:6]).cuda(), torch.cat(rr[:6]).cuda()
        both6 = model(pcd, rgb)
        for v in range(6):
            one = model(pcd[v:v + 1].contiguous(), rgb[v:v + 1].contiguous())
            for a, b in zip(both6, one):
                worst = max(worst, rel_err(a[v:v + 1].cpu().numpy(), b.cpu().numpy()))
    print("batch-6 vs batch-1: max |d| / max(|ref|, 1) = %.3e" % worst)
    assert worst <= 1e-3


def test_resnet101_backbone_forward_matches_oracle():
    """the task's default backbone (and base_channels 48), never constructed before: 1 x 32 x 32, eval mode"""
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init, synthetic_batch
    from oracle import pmf_torch as O
    hip = deterministic_init(PMFNet(5, 3, C, 48, False, "resnet101")).cuda().eval()
    ref = deterministic_init(O.PMFNet(5, 3, C, 48, False, "resnet101")).eval()
    pcd, rgb, _, _ = synthetic_batch(1, 32, 32, C, seed=3)
    with torch.no_grad():
        got = hip(pcd.cuda(), rgb.cuda())
        want = ref(pcd, rgb)
    errs = [rel_err(g.cpu().numpy(), r.numpy()) for g, r in zip(got, want)]
    print("resnet101 vs oracle: lidar %.3e camera %.3e" % tuple(errs))
    assert tuple(got[0].shape) == (1, C, 32, 32) and max(errs) <= 1e-3


# ---- the task end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labelled,tta,use_knn", [(True, True, True), (False, False, False)])
def test_sensat_infer_task_writes_labels_scores_and_reports(tmp_path, labelled, tta, use_knn):
    import yaml
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    task = os.path.join(ROOT, "tasks", "sensat_urban", "pmf_eval")
    split = "val" if labelled else "test"
    tree = S.write_tree(str(tmp_path / "data"), split)
    train = tmp_path / "train"
    os.makedirs(str(train / "checkpoint"))
    torch.save(deterministic_init(PMFNet(5, 3, C, 16, False, "resnet34")).state_dict(), str(train / "checkpoint" / "m.pth"))
    with open(os.path.join(task, "config_server.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_root=str(tmp_path / "data"), training_folder=str(train), pretrained_model="m.pth", has_label=labelled,
               is_debug=False, base_channels=16, img_backbone="resnet34", imagenet_pretrained=False, img_size=list(SIZES),
               experiment_id="t", save_scores=labelled)
    cfg["post"]["KNN"]["use"] = use_knn
    cfg["post"]["tta"]["use"] = tta
    conf_file = str(tmp_path / "cfg.yaml")
    with open(conf_file, "w") as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PMF_AUTOTUNE="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "infer.py", conf_file], cwd=task, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    save = os.path.join(str(train), "Eval-PMFNet_SensatUrban_t", "preds")
    names = [n for n, _, _, _ in S.FRAMES]
    assert sorted(os.listdir(os.path.join(save, split + "_preds"))) == sorted(n + ".label" for n in names)
    total = 0
    for n in names:
        frame, labels, _ = tree[n]
        pred = np.fromfile(os.path.join(save, split + "_preds", n + ".label"), dtype=np.uint8)
        assert pred.size == labels.size and pred.max() < C - 1
        total += labels.size
        if labelled:
            score = np.load(os.path.join(save, split + "_scors", n + ".npy"))
            assert score.dtype == np.float32 and score.shape == (1, C) + frame["feature_map"].shape[1:]
            assert (score >= 0).all() and score.sum() > 0
    if labelled:
        assert "Point-wise Evaluation Results" in out and "Pixel-wise Evaluation Results" in out
        assert "use knn" in out and "use tta" in out and "fwIoU:" in out and "High Vegetation" in out
        assert sorted(os.listdir(os.path.join(save, split + "_scors"))) == sorted(n + ".npy" for n in names)
    else:
        assert "Evaluation Results" not in out and not os.path.exists(os.path.join(save, split + "_scors"))
    assert "cambridge_block_1" not in out
