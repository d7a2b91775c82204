"""SalsaNext evaluation on nuScenes on the MI355X: the batched range-image pass (pmf_eval_range_batch, csrc/eval.hip)
against the reference's recorded composition (tests/golden/g17_salsa_eval.npz, written by tools/make_golden_salsa_eval.py:
the reference's own loader, KNN and IOUEval on tests/salsa_eval_cases.SyntheticSalsaNus), against the existing kernels on
the same maps, its edge cases, and the task end to end.  Everything is exact: labels bit for bit, confusion counts equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import salsa_eval_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

C = S.NCLASSES


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _knn(params=S.KNN_PARAMS):
    from pmf_amd.postproc.knn import inverse_gaussian_window
    return (params["knn"], params["search"], inverse_gaussian_window(params["search"], params["sigma"]).cuda(),
            params["cutoff"])


def _lut(ds):
    lut = np.zeros(256, np.int32)
    for k, v in ds.map_name_from_general_index_to_segmentation_index.items():
        lut[k] = v
    return lut


def _fixture():
    """(prob f32[3,C,H,W], per-sweep dicts of the fixture's arrays + raw ids, lut int32[256], fixture)"""
    g = np.load(S.GOLDEN)
    ds = S.SyntheticSalsaNus()
    prob = S.prob_maps(int(g["seed"]), len(ds))
    sweeps = []
    for i in range(len(ds)):
        d = {k: g["s%d.%s" % (i, k)] for k in ("px", "py", "depth", "proj_range", "label", "gather", "knn")}
        d["sem"] = ds.loadDataByIndex(i)[1].reshape(-1).astype(np.int32)
        sweeps.append(d)
    return prob, sweeps, _lut(ds), g


def _call(prob, sweeps, lut, knn, pixel_conf, point_conf):
    """one pmf_eval_range_batch call on the given sweeps -> per-sweep label arrays"""
    from pmf_amd.postproc import range_batch_eval
    cat = lambda k: _t(np.concatenate([s[k] for s in sweeps]))
    off = np.cumsum([0] + [s["px"].shape[0] for s in sweeps]).astype(np.int64)
    labels, amap = range_batch_eval(
        _t(prob), _t(np.stack([s["proj_range"] for s in sweeps])), _t(off), cat("px"), cat("py"), cat("depth"),
        sem=cat("sem") if point_conf is not None else None, lut=_t(lut) if point_conf is not None else None,
        label=_t(np.stack([s["label"] for s in sweeps])) if pixel_conf is not None else None, knn=knn,
        pixel_conf=pixel_conf, point_conf=point_conf)
    labels = labels.cpu().numpy()
    assert labels.dtype == np.int32 and amap.dtype == torch.int32
    assert np.array_equal(amap.cpu().numpy(), prob.argmax(1))
    return [labels[off[b]:off[b + 1]] for b in range(len(sweeps))]


@pytest.mark.parametrize("use_knn", [False, True])
@pytest.mark.parametrize("one_call", [True, False])
def test_range_batch_matches_reference_fixture(use_knn, one_call):
    prob, sweeps, lut, g = _fixture()
    pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    knn = _knn() if use_knn else None
    if one_call:                                  # B = 3 in one call
        got = _call(prob, sweeps, lut, knn, pix, pts)
    else:                                         # three B = 1 calls accumulating into the same matrices
        got = [_call(prob[b:b + 1], sweeps[b:b + 1], lut, knn, pix, pts)[0] for b in range(3)]
    key = "knn" if use_knn else "gather"
    for b in range(3):
        assert np.array_equal(got[b], sweeps[b][key]), "sweep %d" % b
    assert np.array_equal(pix.cpu().numpy(), g["pixel_conf"])
    assert np.array_equal(pts.cpu().numpy(), g["point_conf_" + key])


@pytest.mark.parametrize("search", [3, 5, 7, 9])
def test_range_batch_equals_existing_kernels_on_the_same_maps(search):
    """pmf_knn_vote_batch_prob (int64 in / out), per-sweep pmf_knn_vote, and per-sweep pmf_eval_argmax + pmf_eval_points;
    search 3 / 5: the LDS-staged vote, 7: the global-gather vote, 9: the run-time window"""
    from pmf_amd.postproc import KNN
    from pmf_amd.postproc.frame_eval import point_labels, window_argmax
    prob, sweeps, lut, _ = _fixture()
    params = dict(S.KNN_PARAMS, search=search)
    H, W = prob.shape[2:]
    pts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    got = _call(prob, sweeps, lut, _knn(params), pix, pts)
    mod = KNN(params, C)
    cat = lambda k: _t(np.concatenate([s[k] for s in sweeps]))
    off = np.cumsum([0] + [s["px"].shape[0] for s in sweeps]).astype(np.int64)
    want = mod.forward_batch_prob(_t(np.stack([s["proj_range"] for s in sweeps])), _t(prob), cat("depth"),
                                  cat("px").long(), cat("py").long(), _t(off)).cpu().numpy()
    assert np.array_equal(np.concatenate(got), want.astype(np.int32))
    pix1 = torch.zeros_like(pix)
    pts1 = torch.zeros_like(pts)
    gat1 = torch.zeros_like(pts)
    gather = _call(prob, sweeps, lut, None, None, gat1)
    gat2 = torch.zeros_like(pts)
    for b, s in enumerate(sweeps):
        one = mod(_t(s["proj_range"]), _t(s["depth"]), _t(prob[b].argmax(0)), _t(s["px"]).long(), _t(s["py"]).long())
        assert np.array_equal(got[b], one.cpu().numpy().astype(np.int32)), "pmf_knn_vote, sweep %d" % b
        p = _t(prob[b])
        amap = window_argmax(p, 0, 0, H, W, _t(s["label"]), pix1)
        kw = dict(sem=_t(s["sem"]), lut=_t(lut))
        lab, _ = point_labels(p, 0, 0, H, W, _t(s["py"]), _t(s["px"]), 0, 0, argmax=amap, proj_range=_t(s["proj_range"]),
                              unproj_range=_t(s["depth"]), knn=_knn(params), conf=pts1, **kw)
        assert np.array_equal(got[b], lab.cpu().numpy()), "pmf_eval_points (KNN), sweep %d" % b
        lab, _ = point_labels(p, 0, 0, H, W, _t(s["py"]), _t(s["px"]), 0, 0, conf=gat2, **kw)
        assert np.array_equal(gather[b], lab.cpu().numpy()), "pmf_eval_points (gather), sweep %d" % b
    assert torch.equal(pix, pix1) and torch.equal(pts, pts1) and torch.equal(gat1, gat2)


def test_range_batch_edge_cases():
    from pmf_amd.postproc import range_batch_eval
    prob, sweeps, lut, g = _fixture()
    H, W = prob.shape[2:]
    # a sweep with zero points inside the batch
    empty = dict(sweeps[1])
    for k in ("px", "py", "depth", "sem", "gather", "knn"):
        empty[k] = empty[k][:0]
    for knn, key in ((None, "gather"), (_knn(), "knn")):
        pts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
        got = _call(prob, [sweeps[0], empty, sweeps[2]], lut, knn, None, pts)
        assert got[1].shape == (0,) and np.array_equal(got[0], sweeps[0][key]) and np.array_equal(got[2], sweeps[2][key])
        want = S.np_conf(sweeps[0][key], lut[sweeps[0]["sem"]], C)
        assert np.array_equal(pts.cpu().numpy(), S.np_conf(sweeps[2][key], lut[sweeps[2]["sem"]], C, want))
        # no points at all: the map stage still runs, the point stage is a no-op; pixel_conf / point_conf None
        pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
        none = [dict(empty), dict(empty, label=sweeps[0]["label"])]
        got = _call(prob[:2], none, lut, knn, pix, None)
        assert all(x.shape == (0,) for x in got)
        assert np.array_equal(pix.cpu().numpy(), S.np_conf(prob[1].argmax(0), sweeps[0]["label"], C,
                                                           S.np_conf(prob[0].argmax(0), sweeps[1]["label"], C)))
        got = _call(prob, sweeps, lut, knn, None, None)
        assert all(np.array_equal(got[b], sweeps[b][key]) for b in range(3))
    # B == 0
    z = lambda dt: torch.zeros(0, dtype=dt, device="cuda")
    lab, amap = range_batch_eval(torch.zeros(0, C, H, W, device="cuda"), None, torch.zeros(1, dtype=torch.int64, device="cuda"),
                                 z(torch.int32), z(torch.int32), None)
    assert lab.shape == (0,) and amap.shape == (0, H, W)
    # NaN in a map: argmax follows torch (a NaN wins, the first one); ties go to the lowest class
    bad = prob.copy()
    rs = np.random.RandomState(5)
    for _ in range(200):
        b, c, y, x = rs.randint(3), rs.randint(C), rs.randint(H), rs.randint(W)
        bad[b, c, y, x] = np.nan
        if rs.rand() < 0.5:
            bad[b, rs.randint(C), y, x] = np.nan
    bad[0, :, 3, 7] = 0.25                                                   # an exact tie of all classes -> class 0
    bad[1, 2:5, 4, 9] = 2.0                                                  # tie of classes 2..4 -> 2
    px0, py0 = sweeps[0]["px"].copy(), sweeps[0]["py"].copy()
    px0[:2], py0[:2] = (7, 9), (3, 4)
    mod = [dict(sweeps[0], px=px0, py=py0), dict(sweeps[1], px=np.where(np.arange(sweeps[1]["px"].shape[0]) == 0, 9,
                                                                        sweeps[1]["px"]).astype(np.int32),
                                                 py=np.where(np.arange(sweeps[1]["py"].shape[0]) == 0, 4,
                                                             sweeps[1]["py"]).astype(np.int32)), sweeps[2]]
    want_map = torch.from_numpy(bad).argmax(1).numpy()
    assert want_map[0, 3, 7] == 0 and want_map[1, 4, 9] == 2 and np.isnan(bad).any(1).sum() >= 150
    pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    labels, amap = range_batch_eval(
        _t(bad), None, _t(np.cumsum([0] + [s["px"].shape[0] for s in mod]).astype(np.int64)),
        _t(np.concatenate([s["px"] for s in mod])), _t(np.concatenate([s["py"] for s in mod])), None,
        label=_t(np.stack([s["label"] for s in mod])), pixel_conf=pix)
    assert np.array_equal(amap.cpu().numpy(), want_map)
    labels = labels.cpu().numpy()
    o = 0
    for b, s in enumerate(mod):
        k = s["px"].shape[0]
        assert np.array_equal(labels[o:o + k], want_map[b][s["py"], s["px"]])
        o += k
    assert labels[0] == 0 and labels[mod[0]["px"].shape[0]] == 2
    assert np.array_equal(pix.cpu().numpy(), S.np_conf(want_map, np.stack([s["label"] for s in mod]), C))
    # labels outside [0, C) are not counted; raw ids outside the lut count as class 0
    lab_out = sweeps[0]["label"].copy()
    lab_out[::3, ::5] = C
    lab_out[1::3, ::7] = -2.0
    lab_out[2::3, ::11] = 300.0
    sem_out = sweeps[0]["sem"].copy()
    sem_out[::4] = 40 + (np.arange(sem_out[::4].shape[0]) % 3) * 1000
    sem_out[1::9] = -5
    short_lut = lut[:40].copy()
    pix = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    got = _call(prob[:1], [dict(sweeps[0], label=lab_out, sem=sem_out)], short_lut, None, pix, pts)
    ok = (lab_out >= 0) & (lab_out < C)
    assert (~ok).sum() > 100
    assert np.array_equal(pix.cpu().numpy(), S.np_conf(prob[0].argmax(0)[ok], lab_out[ok], C))
    gt = np.where((sem_out >= 0) & (sem_out < 40), short_lut[np.clip(sem_out, 0, 39)], 0)
    assert ((sem_out < 0) | (sem_out >= 40)).sum() > 1000
    assert np.array_equal(pts.cpu().numpy(), S.np_conf(got[0], gt, C))


# ---- the task end to end -----------------------------------------------------------------------------------------------
DRIVER = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {task!r})
os.chdir({task!r})
from tests.salsa_eval_cases import SyntheticSalsaNus
from option import Option
import infer
settings = Option(sys.argv[1])
exp = infer.Experiment(settings, dataset=SyntheticSalsaNus())
os.makedirs(sys.argv[2])
seen = []
exp.model.register_forward_hook(lambda m, i, o: (np.save(os.path.join(sys.argv[2], "%d.npy" % len(seen)),
                                                         o.detach().cpu().numpy()), seen.append(1)) and None)
print("===init env success===")
exp.run()
"""


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


def test_salsanext_eval_nuscenes_task_end_to_end(tmp_path):
    """eval_batch_size 1 and 2 (3 sweeps: a short last batch), KNN off and on: the .bin files and both reported confusion
    matrices against the reference's composition (torch argmax, IOUEval.addBatch, fancy indexing or the numpy KNN oracle)
    applied to the network outputs of the SAME batch size (tile choices may differ by shape: equality across batch sizes is
    not asserted)."""
    import yaml
    import pc_processor
    from pmf_amd.models import SalsaNext
    from pmf_amd.utils.detinit import deterministic_init
    ds = S.SyntheticSalsaNus()
    task = os.path.join(ROOT, "tasks", "salsanext_eval_nuscenes")
    ckpt = str(tmp_path / "salsanext.pth")
    torch.save(deterministic_init(SalsaNext(in_channels=5, nclasses=C)).state_dict(), ckpt)
    with open(os.path.join(task, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(save_path=str(tmp_path / "out"), data_root="unused", n_threads=0, has_label=True, print_frequency=1,
               gpu="0", pretrained_model=ckpt, sensor=dict(S.CONFIG["sensor"]))
    driver = str(tmp_path / "driver.py")
    with open(driver, "w") as f:
        f.write(DRIVER.format(root=ROOT, task=task))
    env = dict(os.environ, PMF_AUTOTUNE="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    loader = pc_processor.dataset.SalsaNextLoader(ds, cfg, is_train=False, return_uproj=True)
    items = [loader[i] for i in range(len(ds))]
    from oracle import knn_ref                      # numpy statement of the vote: independent of the HIP vote under test
    for bs in (1, 2):
        for use_knn in (False, True):
            cfg["post"]["KNN"]["use"] = use_knn
            cfg["eval_batch_size"] = bs
            cfg["experiment_id"] = "bs%d_%d" % (bs, use_knn)
            conf_file = str(tmp_path / ("cfg_%s.yaml" % cfg["experiment_id"]))
            with open(conf_file, "w") as f:
                yaml.safe_dump(cfg, f)
            dump = str(tmp_path / ("probs_%s" % cfg["experiment_id"]))
            r = subprocess.run([sys.executable, driver, conf_file, dump], env=env, capture_output=True, text=True,
                               timeout=600)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            out = r.stdout
            assert "Point-wise Evaluation Results" in out and "Pixel-wise Evaluation Results" in out
            save = os.path.join(cfg["save_path"], "Eval-SV_nuScenes_SalsaNext_%s_%s" % (
                "KNN-5" if use_knn else "", cfg["experiment_id"]))
            batches = [list(range(i, min(i + bs, 3))) for i in range(0, 3, bs)]
            assert sorted(os.listdir(dump)) == ["%d.npy" % k for k in range(len(batches))]
            evaluator = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])
            pixel_eval = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])
            changed = 0
            for k, idx in enumerate(batches):
                pred_all = torch.from_numpy(np.load(os.path.join(dump, "%d.npy" % k))).cuda()
                assert tuple(pred_all.shape) == (len(idx), C, 32, 512)
                for j, i in enumerate(idx):                     # the reference's loop body, infer.py:90-128
                    _, input_label, _, proj_depth, ux, uy, ud = items[i]
                    pred_output = pred_all[j:j + 1]
                    pred_argmax = pred_output[0].argmax(dim=0)
                    pixel_eval.addBatch(pred_output.argmax(dim=1).cpu(), input_label[None].long().cpu())
                    if use_knn:
                        unproj = torch.from_numpy(knn_ref.knn_vote(
                            proj_depth.cpu().numpy(), ud.cpu().numpy(), pred_argmax.cpu().numpy(), ux.cpu().numpy(),
                            uy.cpu().numpy(), nclasses=C, **S.KNN_PARAMS))
                    else:
                        unproj = pred_argmax[uy, ux]
                    pred_np = unproj.cpu().numpy().reshape(-1).astype(np.int32)
                    changed += int((pred_np != pred_argmax[uy, ux].cpu().numpy()).sum())
                    evaluator.addBatch(pred_np, ds.labelMapping(ds.loadDataByIndex(i)[1]))
                    path = os.path.join(save, "preds", "lidarseg", "val", "%s_lidarseg.bin" % ds.token_list[i])
                    assert os.path.getsize(path) == 4 * pred_np.shape[0]
                    assert np.array_equal(np.fromfile(path, dtype=np.int32), pred_np), (bs, use_knn, i)
            assert (changed > 0) == use_knn
            pt_tab, px_tab = _parse_tables(out, C)
            for tab, ev in ((pt_tab, evaluator), (px_tab, pixel_eval)):
                ref = ev.conf_matrix.cpu().numpy().copy()
                assert ref.sum() > 0
                ref[0] = 0
                ref[:, 0] = 0
                assert np.array_equal(tab, ref), (bs, use_knn)
            assert "IOU avg: {:.4f}".format(evaluator.getIoU()[0].item()) in out
