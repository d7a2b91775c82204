"""Full-sweep nuScenes fusion on the MI355X: pmf_eval_fill and pmf_eval_sweep_finish_fill (csrc/eval.hip) against the
reference's recorded result (tests/golden/g18_nus_fill.npz) and the numpy statement of the rule (tests/nus_fill_cases.py),
the fused finish against the plain finish + the fill on the same state, and the two tasks end to end on temporary trees.
Everything is integer and exact: labels byte for byte, counts equal."""
import json
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

from tests import nus_fill_cases as F  # noqa: E402
from tests import nus_v2_cases as N  # noqa: E402
from tests.test_gpu_epmf_eval import _parse_tables  # noqa: E402

pytestmark = pytest.mark.gpu

C = F.NCLASSES


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fill(main, sub, sem=None, lut=None, base=None, want=("conf", "counts", "out"), nclasses=C, fill_class=F.FILL_CLASS):
    """one pmf_eval_fill launch -> (uint8 labels or None, confusion or None, counts or None) as numpy"""
    from pmf_amd.postproc import fill_labels
    P = main.shape[0]
    conf = _t(np.zeros((nclasses, nclasses), np.int64) if base is None else base.copy()) if "conf" in want else None
    counts = torch.zeros(3, dtype=torch.int64, device="cuda") if "counts" in want else None
    out = torch.full((P,), 255, dtype=torch.uint8, device="cuda") if "out" in want else None
    r = fill_labels(_t(main), _t(sub), nclasses, fill_class=fill_class, sem=None if sem is None else _t(sem),
                    lut=None if lut is None else _t(lut), conf=conf, counts=counts, out_u8=out)
    assert r is out
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (out, conf, counts))


# ---- pmf_eval_fill -----------------------------------------------------------------------------------------------------
def test_fill_matches_reference_fixture_one_launch_or_three():
    g = np.load(F.GOLDEN, allow_pickle=False)
    lut = F.label_lut()
    sweeps = [F.sweep_case(i) for i in range(len(F.COUNTS))]
    conf = np.zeros((C, C), np.int64)
    counts = np.zeros(3, np.int64)
    per_sweep = []
    for i, (main, sub, sem) in enumerate(sweeps):                         # three launches, the confusion accumulating
        u8, conf, c = _fill(main, sub, sem, lut, base=conf)
        assert np.array_equal(u8, g["s%d.fused" % i]), i
        assert np.array_equal(u8, F.fill_np(main, sub, sem, lut)[0])
        counts += c
        per_sweep.append(u8)
    assert np.array_equal(conf, g["conf"]) and np.array_equal(counts, g["counts"])
    cat = [np.concatenate([s[k] for s in sweeps]) for k in range(3)]      # one launch over the three sweeps concatenated
    u8, conf1, counts1 = _fill(cat[0], cat[1], cat[2], lut)
    assert np.array_equal(u8, np.concatenate(per_sweep))
    assert np.array_equal(conf1, g["conf"]) and np.array_equal(counts1, g["counts"])


def test_fill_each_optional_output_absent_and_empty_input():
    from pmf_amd.postproc import fill_labels
    lut = F.label_lut()
    main, sub, sem = F.sweep_case(1)
    ru8, rconf, rcounts = F.fill_np(main, sub, sem, lut)
    for want in (("counts", "out"), ("conf", "out"), ("conf", "counts"), ("out",), ("conf",), ("counts",), ()):
        with_gt = "conf" in want
        u8, conf, counts = _fill(main, sub, sem if with_gt else None, lut if with_gt else None, want=want)
        assert (u8 is None) == ("out" not in want) and (conf is None) == (not with_gt) and \
            (counts is None) == ("counts" not in want)
        assert u8 is None or np.array_equal(u8, ru8)
        assert conf is None or np.array_equal(conf, rconf)
        assert counts is None or np.array_equal(counts, rcounts)
    e = np.zeros(0, np.int32)                                             # P == 0: nothing is touched
    u8, conf, counts = _fill(e, e, e, lut, base=rconf)
    assert u8.shape == (0,) and np.array_equal(conf, rconf) and not counts.any()
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert fill_labels(empty, empty, C) is None


def test_fill_nuscenes_sized_sweep_with_labels_outside_the_classes():
    """34 720 points; one planted label >= C and one negative label go out as numpy's astype(uint8) writes them and are not
    counted; raw ids beyond the 256-entry table count as class 0; another fill class; batches of eight such sweeps"""
    P = 34720
    g = _rng(11)
    lut = g.integers(0, C, 256).astype(np.int32)
    main = g.integers(1, C, P).astype(np.int32)
    main[g.random(P) < 0.6] = 0
    sub = g.integers(1, C, P).astype(np.int32)
    sub[g.random(P) < 0.1] = 0
    sem = g.integers(0, 300, P).astype(np.int32)
    main[100], main[20000] = C + 300, -3
    sub[100], sub[20000] = 1, 2
    main[101], sub[101] = 0, 250                                          # >= C through the sub prediction
    base = g.integers(0, 50, (C, C)).astype(np.int64)
    for fill_class in (F.FILL_CLASS, 2):
        ru8, rconf, rcounts = F.fill_np(main, sub, sem, lut, fill_class=fill_class, base=base)
        u8, conf, counts = _fill(main, sub, sem, lut, base=base, fill_class=fill_class)
        assert np.array_equal(u8, ru8) and np.array_equal(conf, rconf) and np.array_equal(counts, rcounts)
        assert u8[100] == (C + 300) % 256 and u8[20000] == 253 and u8[101] == 250
        assert conf.sum() - base.sum() == P - 3 and counts.sum() == P and counts.min() > 0
        assert (u8 == fill_class).sum() >= counts[2]
    B = 8                                                                 # a batch: 277 760 points, the grid cap in play
    mains = np.concatenate([np.roll(main, 37 * b) for b in range(B)])
    subs = np.concatenate([np.roll(sub, 37 * b) for b in range(B)])
    sems = np.concatenate([np.roll(sem, 11 * b) for b in range(B)])
    ru8, rconf, rcounts = F.fill_np(mains, subs, sems, lut)
    u8, conf, counts = _fill(mains, subs, sems, lut)
    assert np.array_equal(u8, ru8) and np.array_equal(conf, rconf) and np.array_equal(counts, rcounts)


# ---- pmf_eval_sweep_finish_fill -----------------------------------------------------------------------------------------
def _state(seed, P):
    g = _rng(seed)
    lab = g.integers(1, C, P).astype(np.int32)
    lab[g.random(P) < 0.55] = 0
    cf = (g.random(P) * (lab != 0)).astype(np.float32)
    sub = g.integers(1, C, P).astype(np.int32)
    sub[g.random(P) < 0.1] = 0
    sem = g.integers(0, 300, P).astype(np.int32)
    lut = g.integers(0, C, 256).astype(np.int32)
    return cf, lab, sub, sem, lut


@pytest.mark.parametrize("P", [34720, 1000, 1])
def test_sweep_finish_fill_equals_plain_finish_plus_fill(P):
    from pmf_amd.postproc.frame_eval import sweep_finish, sweep_finish_fill
    cf, lab, sub, sem, lut = _state(20 + P, P)
    base = _rng(3).integers(0, 50, (C, C)).astype(np.int64)
    # the plain finish and the batched fill on copies of the state
    cf0, lab0 = _t(cf), _t(lab)
    conf0 = _t(base.copy())
    cam0 = torch.full((P,), 255, dtype=torch.uint8, device="cuda")
    sweep_finish(cf0, lab0, C, _t(sem), _t(lut), conf0, cam0)
    fu8, fconf, fcounts = _fill(lab, sub, sem, lut, base=base)
    # the fused finish
    cf1, lab1 = _t(cf), _t(lab)
    conf1, fused1 = _t(base.copy()), _t(base.copy())
    counts1 = torch.zeros(3, dtype=torch.int64, device="cuda")
    cam1 = torch.full((P,), 255, dtype=torch.uint8, device="cuda")
    out1 = torch.full((P,), 255, dtype=torch.uint8, device="cuda")
    assert sweep_finish_fill(cf1, lab1, _t(sub), C, F.FILL_CLASS, _t(sem), _t(lut), conf1, fused1, counts1, cam1,
                             out1) is out1
    assert torch.equal(conf1, conf0) and torch.equal(cam1, cam0)          # camera side: bit-identical to the plain finish
    assert not cf1.any().item() and not lab1.any().item() and not cf0.any().item() and not lab0.any().item()
    assert np.array_equal(out1.cpu().numpy(), fu8) and np.array_equal(fused1.cpu().numpy(), fconf)
    assert np.array_equal(counts1.cpu().numpy(), fcounts)
    ru8, rconf, rcounts = F.fill_np(lab, sub, sem, lut, base=base)
    assert np.array_equal(fu8, ru8) and np.array_equal(fconf, rconf) and np.array_equal(fcounts, rcounts)
    # every output optional: labels only, then the fused confusion only
    cf2, lab2 = _t(cf), _t(lab)
    out2 = torch.empty(P, dtype=torch.uint8, device="cuda")
    sweep_finish_fill(cf2, lab2, _t(sub), C, out_u8=out2)
    assert np.array_equal(out2.cpu().numpy(), ru8) and not lab2.any().item() and not cf2.any().item()
    lab2.copy_(_t(lab))
    fused2 = _t(base.copy())
    sweep_finish_fill(cf2, lab2, _t(sub), C, sem=_t(sem), lut=_t(lut), fused_conf=fused2)
    assert np.array_equal(fused2.cpu().numpy(), rconf) and not lab2.any().item()


def test_sweep_evaluator_finish_with_and_without_fallback():
    """finish() without a fallback returns what sweep_finish returns on the same state (today's path); with one, the fused
    labels, and the camera confusion is still the plain finish's"""
    from pmf_amd.postproc.frame_eval import SweepEvaluator, sweep_finish
    P = 6000
    cf, lab, sub, sem, lut = _state(7, P)

    def primed():
        se = SweepEvaluator(C, N.MEAN, N.STDS)
        a, b = se._state(P)
        a.copy_(_t(cf))
        b.copy_(_t(lab))
        se.views_in_sweep, se.n_points = 6, P
        return se

    cam_conf = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    cam = torch.empty(P, dtype=torch.uint8, device="cuda")
    sweep_finish(_t(cf), _t(lab), C, _t(sem), _t(lut), cam_conf, cam)
    se = primed()
    conf = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    out = se.finish(_t(sem), _t(lut), P, point_conf=conf)
    assert out.dtype == torch.uint8 and torch.equal(out, cam) and torch.equal(conf, cam_conf) and se.views_in_sweep == 0
    assert se.finish.__defaults__[:2] == (None, True)
    assert primed().finish(_t(sem), _t(lut), P, want_labels=False) is None
    with pytest.raises(ValueError):
        primed().finish(_t(sem), _t(lut), P, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    se = primed()
    conf2 = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    fused = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    out = se.finish(_t(sem), _t(lut), P, point_conf=conf2, fallback=_t(sub), fused_conf=fused, counts=counts)
    ru8, rconf, rcounts = F.fill_np(lab, sub, sem, lut)
    assert np.array_equal(out.cpu().numpy(), ru8) and np.array_equal(fused.cpu().numpy(), rconf)
    assert np.array_equal(counts.cpu().numpy(), rcounts) and torch.equal(conf2, cam_conf) and se.views_in_sweep == 0
    a, b = se._state(P)
    assert not a.any().item() and not b.any().item()
    with pytest.raises(ValueError):
        primed().finish(_t(sem), _t(lut), P, fallback=_t(sub[:-1]))


# ---- the merge task end to end ---------------------------------------------------------------------------------------------
MERGE_DRIVER = """
import os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {task!r})
os.chdir({task!r})
from tests.nus_fill_cases import SyntheticNusSweeps
from option import Option
import main
import check_valid
ds = SyntheticNusSweeps()
settings = Option(sys.argv[1])
exp = main.Experiment(settings, dataset=ds)
print("===init env success===")
exp.run()
check_valid.Experiment(settings, dataset=ds).run()
"""


def _run(driver, args, timeout=600):
    env = dict(os.environ, PMF_AUTOTUNE="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, driver] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("main_dtype", ["int32", "uint8"])
def test_merge_task_end_to_end(tmp_path, main_dtype):
    import yaml
    from tests.test_nus_fill_host import load_task
    ds = F.SyntheticNusSweeps()
    assert len(ds) == 5
    task = os.path.join(ROOT, "tasks", "pmf_eval_nuscenes", "testset_eval")
    main_dir, sub_dir = str(tmp_path / "main"), str(tmp_path / "sub")
    lut = F.label_lut()
    conf = np.zeros((C, C), np.int64)
    counts = np.zeros(3, np.int64)
    expect = {}
    for d in (main_dir, sub_dir):
        os.makedirs(os.path.join(d, "preds", "lidarseg", "val"))
    for i, token in enumerate(ds.token_list):
        m, s = ds.main_sub(i)
        m.astype(np.dtype(main_dtype)).tofile(os.path.join(main_dir, "preds", "lidarseg", "val", "%s_lidarseg.bin" % token))
        s.tofile(os.path.join(sub_dir, "preds", "lidarseg", "val", "%s_lidarseg.bin" % token))
        expect[token], conf, c = F.fill_np(m, s, ds.loadLabelByIndex(i).reshape(-1), lut, base=conf)
        counts += c
    with open(os.path.join(task, "config_server.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(save_path=str(tmp_path / "out"), experiment_id="merge-" + main_dtype, data_root="unused",
               main_pred_folder=main_dir, sub_pred_folder=sub_dir, main_pred_dtype=main_dtype,
               merge_batch_size=2)                                        # 5 sweeps: batches of 2, 2 and 1
    conf_file = str(tmp_path / "cfg.yaml")
    with open(conf_file, "w") as f:
        yaml.safe_dump(cfg, f)
    driver = str(tmp_path / "driver.py")
    with open(driver, "w") as f:
        f.write(MERGE_DRIVER.format(root=ROOT, task=task))
    out = _run(driver, [conf_file])
    preds = os.path.join(str(tmp_path / "out"), "merge-" + main_dtype, "preds")
    for token, ref in expect.items():
        got = np.fromfile(os.path.join(preds, "lidarseg", "val", "%s_lidarseg.bin" % token), dtype=np.uint8)
        assert np.array_equal(got, ref), token
    assert sorted(os.listdir(os.path.join(preds, "lidarseg", "val"))) == sorted("%s_lidarseg.bin" % t for t in expect)
    with open(os.path.join(preds, "val", "submission.json")) as f:
        assert json.load(f) == {"meta": {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False,
                                         "use_external": False}}
    assert "valid submission: 5 sweeps" in out
    _, _, chk = load_task()
    assert chk.check_submission(preds, "val", dict(zip(ds.token_list, ds.counts)), C) == []
    assert len(re.findall(r"Iter \[\d+\|0005\]", out)) == 3
    tabs = _parse_tables(out, C)
    ref = conf.copy()
    ref[0] = 0
    ref[:, 0] = 0
    assert len(tabs) == 1 and np.array_equal(tabs[0], ref)
    m = re.search(r"Point-wise Evaluation Results.*?IOU avg: ([0-9.]+)", out, re.S)
    assert m and m.group(1) == "{:.4f}".format(F.miou_np(conf))
    assert re.findall(r"meanIOU ([0-9.]+)", out)[-1] == "{:.4f}".format(F.miou_np(conf))
    m = re.search(r"Label source: main [0-9.]+ \((\d+)\), sub [0-9.]+ \((\d+)\), filled [0-9.]+ \((\d+)\) of (\d+) points", out)
    assert m and [int(x) for x in m.groups()] == counts.tolist() + [sum(ds.counts)]
    for title in ("Latext Format String", "Data Distribution", "fwIoU:", "ACC matrix", "Recall matrix"):
        assert title in out, title


# ---- the EPMF task with sub_pred_folder ------------------------------------------------------------------------------------
EPMF_DRIVER = """
import os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {task!r})
os.chdir({task!r})
from tests.nus_v2_cases import SyntheticNusV2
from option import Option
import infer
exp = infer.Experiment(Option(sys.argv[1]), dataset=SyntheticNusV2(nclasses={C}))
print("===init env success===")
exp.run()
"""


def test_epmf_task_with_sub_pred_folder_writes_fused_sweeps(tmp_path):
    import yaml
    from pmf_amd.models import EPMFNet
    from pmf_amd.utils.detinit import deterministic_init
    Cn, fill_class = 6, 3
    ds = N.SyntheticNusV2(nclasses=Cn)
    model_dir = tmp_path / "model"
    os.makedirs(model_dir / "checkpoint")
    torch.save(deterministic_init(EPMFNet(5, 3, Cn, 32, False, "resnet34")).state_dict(),
               str(model_dir / "checkpoint" / "best_IOU_model.pth"))
    task = os.path.join(ROOT, "tasks", "epmf_eval_nuscenes")
    with open(os.path.join(task, "config_server_nus.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(pretrained_path=str(model_dir), data_root="unused", nclasses=Cn, n_threads=0, save_pred_results=True,
               has_label=True, print_frequency=1, gpu="0")
    cfg["post"]["KNN"]["use"] = False
    sub_dir = str(tmp_path / "sub")
    os.makedirs(os.path.join(sub_dir, "preds", "lidarseg", "val"))
    lut = np.zeros(256, np.int64)
    lut[:32] = ds.labelMapping(np.arange(32, dtype=np.uint8)[:, None])
    subs, sems = [], []
    for s in range(2):
        pts, raw, _ = ds.loadDataByIndex(6 * s)
        g = _rng(50 + s)
        sub = g.integers(1, Cn, pts.shape[0]).astype(np.int32)
        sub[g.random(pts.shape[0]) < 0.15] = 0
        sub.tofile(os.path.join(sub_dir, "preds", "lidarseg", "val", "sweep%03d_lidarseg.bin" % s))
        subs.append(sub)
        sems.append(raw.reshape(-1).astype(np.int64))
    driver = str(tmp_path / "driver.py")
    with open(driver, "w") as f:
        f.write(EPMF_DRIVER.format(root=ROOT, task=task, C=Cn))
    outs, saves = {}, {}
    for name, extra in (("cam", {}), ("fused", dict(sub_pred_folder=sub_dir, fill_class=fill_class))):
        c = dict(cfg, experiment_id=name, **extra)
        conf_file = str(tmp_path / ("cfg_%s.yaml" % name))
        with open(conf_file, "w") as f:
            yaml.safe_dump(c, f)
        outs[name] = _run(driver, [conf_file])
        saves[name] = os.path.join(str(model_dir), "Eval-nuScenes-PMFNet-best_IOU_model-noKNN-%s" % name)
    # the camera-only report is unchanged by the key; the run without it has no fused block and no submission.json
    cam_tabs, fused_tabs = _parse_tables(outs["cam"], Cn), _parse_tables(outs["fused"], Cn)
    assert len(cam_tabs) == 2 and len(fused_tabs) == 3
    assert np.array_equal(cam_tabs[0], fused_tabs[0]) and np.array_equal(cam_tabs[1], fused_tabs[1])
    summary = lambda o: re.findall(r"(?:Pixel )?Acc avg: [0-9.]+, IOU avg: [0-9.]+, Recall avg: [0-9.]+", o)
    assert len(summary(outs["cam"])) == 2 and summary(outs["fused"])[:2] == summary(outs["cam"])
    assert "Fused point-wise" not in outs["cam"] and "Label source" not in outs["cam"]
    assert not os.path.exists(os.path.join(saves["cam"], "preds", "val", "submission.json"))
    with open(os.path.join(saves["fused"], "preds", "val", "submission.json")) as f:
        assert sorted(json.load(f)["meta"]) == ["use_camera", "use_external", "use_lidar", "use_map", "use_radar"]
    conf = np.zeros((Cn, Cn), np.int64)
    counts = np.zeros(3, np.int64)
    for s in range(2):
        name = os.path.join("preds", "lidarseg", "val", "sweep%03d_lidarseg.bin" % s)
        cam = np.fromfile(os.path.join(saves["cam"], name), dtype=np.uint8)
        got = np.fromfile(os.path.join(saves["fused"], name), dtype=np.uint8)
        assert (cam == 0).mean() >= 0.01 and cam.shape == subs[s].shape
        ru8, conf, c = F.fill_np(cam.astype(np.int32), subs[s], sems[s], lut, nclasses=Cn, fill_class=fill_class, base=conf)
        counts += c
        assert np.array_equal(got, ru8) and got.min() >= 1
    assert counts.min() > 0
    ref = conf.copy()
    ref[0] = 0
    ref[:, 0] = 0
    assert np.array_equal(fused_tabs[2], ref)
    m = re.search(r"Fused point-wise Evaluation Results.*?IOU avg: ([0-9.]+)", outs["fused"], re.S)
    assert m and m.group(1) == "{:.4f}".format(F.miou_np(conf))
    m = re.search(r"Label source: main [0-9.]+ \((\d+)\), sub [0-9.]+ \((\d+)\), filled [0-9.]+ \((\d+)\)", outs["fused"])
    assert m and [int(x) for x in m.groups()] == counts.tolist()
