"""SensatLoader on the GPU (csrc/bev_train.hip pmf_bev_sample_count / pmf_bev_sample_gather, dataset/sensat_urban/
sensat_loader.py) against the reference's item chain restated on the CPU (tests/sensat_loader_cases.py), and the task's
trainer end to end on a synthetic tree."""
import functools
import os
import random
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd.dataset import SensatLoader, SensatUrban  # noqa: E402
from tests import sensat_eval_cases as E  # noqa: E402
from tests import sensat_loader_cases as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
JIT = (0.1375, -1.625)


@functools.lru_cache(maxsize=None)
def _loader(names):
    H, W = S.FRAMES[names[0]][2:]
    return SensatLoader(S.FrameSet(names), img_h=H, img_w=W, n_samples_split=20000, device=DEV)


@functools.lru_cache(maxsize=None)
def _all_map(name):
    return S.all_map(S.make_frame(name))


def _gather(ld, names, items):
    """items: [(frame number in the loader, candidate, jitter)] -> CPU (f32[B,8,H,W], f32[B,H,W]) of ONE launch"""
    f, l = ld.gather([ld.pack(k, c, j) for k, c, j in items])
    torch.cuda.synchronize()
    assert f.shape == (len(items), 8, ld.img_h, ld.img_w) and l.shape == (len(items), ld.img_h, ld.img_w)
    return f.cpu(), l.cpu()


def _mismatches(got, want):
    return ((got[0] != want[0]).any(0) | (got[1] != want[1])).nonzero().tolist()


def test_exact_cases_flips_on_frames_a_and_b_in_one_launch():
    """angle 0: every flip combination at several crop positions, frames A and B mixed in one launch, bit for bit"""
    names = ("A", "B")
    ld = _loader(names)
    H, W = ld.img_h, ld.img_w
    items = []
    for k, (top1, left1) in ((0, (22, 33)), (0, (0, 0)), (0, (7, 15)), (1, (0, 0))):
        for n, (top2, left2) in enumerate(((0, 0), (H, W), (5, 31), (17, 2))):
            items.append((k, (top1, left1, 0.0, top2, left2, bool(n & 1), bool(n & 2)), JIT))
    got = _gather(ld, names, items)
    for b, (k, cand, jit) in enumerate(items):
        want = S.ref_item(_all_map(names[k]), cand, jit, H, W)
        assert torch.equal(got[0][b], want[0]) and torch.equal(got[1][b], want[1]), (b, cand)
    assert (got[1] == -1).any() and (got[0][:, 4] == 0).any() and (got[0][:, 4] == 1).any()


@pytest.mark.parametrize("angle", [90.0, 180.0, 270.0, -90.0, 360.0])
def test_exact_cases_quarter_turns_on_two_frames_of_one_size(angle):
    """on the square 64 x 64 first crop the restatement's quarter turns are exact (no zero fill, no ties): bit for bit, two
    different frames in one launch"""
    names = ("C", "C2")
    ld = _loader(names)
    H, W = ld.img_h, ld.img_w
    items = [(0, (33, 0, angle, 0, 32, False, False), JIT), (1, (11, 0, angle, 32, 0, True, False), (0.0, 1.25)),
             (0, (0, 0, angle, 13, 7, True, True), (-0.2, 2.0)), (1, (20, 0, angle, 9, 30, False, True), JIT)]
    got = _gather(ld, names, items)
    for b, (k, cand, jit) in enumerate(items):
        want = S.ref_item(_all_map(names[k]), cand, jit, H, W)
        turned = torch.rot90(_all_map(names[k])[:, cand[0]:cand[0] + 64, :64], round(angle / 90) % 4, (1, 2))
        assert torch.equal(S.ref_augment(_all_map(names[k]), cand[:5] + (False, False), H, W),
                           turned[:, cand[3]:cand[3] + H, cand[4]:cand[4] + W])
        assert torch.equal(got[0][b], want[0]) and torch.equal(got[1][b], want[1]), (b, cand)


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_general_angles_and_count(name):
    """ten seeded draws: the gather differs from the restatement only at pixels whose source coordinate (float64) lies
    within 1e-3 of a rounding edge, at most 1e-3 * H * W + 4 of them per item, and is bit-equal elsewhere (jitter
    included); the count kernel equals (label_out >= 0).sum() of the gather's own output exactly and the reference's count
    within the number of mismatching pixels"""
    h, w, H, W = S.FRAMES[name]
    ld = _loader((name,))
    torch.manual_seed(S.GENERAL_SEED[name])
    random.seed(S.GENERAL_SEED[name])
    items = [(0, ld.draw(h, w), ld.draw_jitter()) for _ in range(10)]
    got = _gather(ld, (name,), items)
    counts = ld.count([ld.pack(k, c) for k, c, _ in items])
    assert counts.dtype == torch.int32 and counts.shape == (10,)
    assert any(c[5] for _, c, _ in items) and any(c[6] for _, c, _ in items)
    for b, (k, cand, jit) in enumerate(items):
        want = S.ref_item(_all_map(name), cand, jit, H, W)
        bad = _mismatches((got[0][b], got[1][b]), want)
        print(name, b, "angle %.3f" % cand[2], "mismatching pixels", len(bad), "count", int(counts[b]))
        assert len(bad) <= S.cap(H, W), (b, len(bad))
        for oy, ox in bad:
            assert S.edge_distance(cand, H, W, oy, ox) < 1e-3, (b, oy, ox)
        assert int(counts[b]) == int((got[1][b] >= 0).sum())
        assert abs(int(counts[b]) - S.ref_share(_all_map(name), cand, H, W)[1]) <= len(bad)


REJECTION_SEEDS = [6, 9, 0, 3]          # three rejections, one, none, none (found on the CPU with the restatement)


def _replay(ld, name, seed):
    """the candidates a batch of ONE draws under `seed`, on the host, with the reference's share of each; stops at the
    first accepted one -> ([(cand, share)], jitter)"""
    h, w, H, W = S.FRAMES[name]
    torch.manual_seed(seed)
    random.seed(seed)
    out = []
    while True:
        cand = ld.draw(h, w)
        share, count = S.ref_share(_all_map(name), cand, H, W)
        # no share of these seeds is within the cap of the threshold: a pixel on a rounding edge cannot turn the decision
        assert abs(count - 0.1 * H * W) > S.cap(H, W), (seed, count)
        out.append((cand, share))
        if not bool(share < 0.1):
            return out, ld.draw_jitter()


@pytest.mark.parametrize("seed", REJECTION_SEEDS)
def test_rejection_returns_the_first_accepted_candidate(seed):
    """frame D is unlabelled outside one quadrant: candidates that miss it (and keep little zero fill, which counts as
    labelled) fall below 10 % and are drawn again"""
    ld = _loader(("D",))
    H, W = ld.img_h, ld.img_w
    tried, jit = _replay(ld, "D", seed)
    torch.manual_seed(seed)
    random.seed(seed)
    f, l = ld.batch([2])
    after = (torch.rand(1), random.random())
    torch.cuda.synchronize()
    assert f.shape == (1, 8, H, W) and l.shape == (1, H, W) and f.is_cuda
    assert float((l[0] >= 0).sum()) / (H * W) >= 0.1
    cand = tried[-1][0]
    want = S.ref_item(_all_map("D"), cand, jit, H, W)
    bad = _mismatches((f[0].cpu(), l[0].cpu()), want)
    assert len(bad) <= S.cap(H, W) and all(S.edge_distance(cand, H, W, oy, ox) < 1e-3 for oy, ox in bad)
    if len(tried) > 1:            # the rejected first candidate is not what came back
        first = S.ref_item(_all_map("D"), tried[0][0], jit, H, W)
        assert float(tried[0][1]) < 0.1 and len(_mismatches((f[0].cpu(), l[0].cpu()), first)) > S.cap(H, W)
    # the streams were consumed exactly as the replay (= the reference's loop) consumes them
    _replay(ld, "D", seed)
    assert torch.equal(torch.rand(1), after[0]) and random.random() == after[1]


def test_rejection_happens_for_the_chosen_seeds():
    ld = _loader(("D",))
    lengths = [len(_replay(ld, "D", seed)[0]) for seed in REJECTION_SEEDS]
    assert lengths == [4, 2, 1, 1], lengths


def test_batches_are_deterministic_and_all_accepted():
    ld = _loader(("D", "A"))
    H, W = ld.img_h, ld.img_w
    assert sorted(set(ld.frame_idx_list)) == [0, 1]
    out = []
    for _ in range(2):
        torch.manual_seed(5)
        random.seed(5)
        out.append([(f.clone(), l.clone()) for f, l in ld.batches(4, shuffle=True, drop_last=True)])
    torch.cuda.synchronize()
    assert len(out[0]) == len(ld) // 4 == len(ld.batches(4))
    for (f1, l1), (f2, l2) in zip(*out):
        assert f1.shape == (4, 8, H, W) and torch.equal(f1, f2) and torch.equal(l1, l2)
        assert ((l1 >= 0).flatten(1).sum(1).float() / (H * W) >= 0.1).all()
    f, l = ld[0]
    assert f.shape == (8, H, W) and l.shape == (H, W)


def test_val_split_returns_the_frame_unchanged():
    ds = S.FrameSet(["B", "B"], split="val")
    ld = SensatLoader(ds, device=DEV)
    f, l = ld[1]
    frame = S.make_frame("B")
    assert f.is_cuda and torch.equal(f.cpu(), torch.from_numpy(frame["feature_map"]).float())
    assert torch.equal(l.cpu(), torch.from_numpy(frame["label_map"]).float())
    (bf, bl), = list(ld.batches(2, shuffle=False, drop_last=False))
    assert bf.shape == (2, 8, 48, 80) and torch.equal(bf[0], f) and torch.equal(bl[1], l)


def test_trainer_runs_one_train_and_one_validation_iteration(tmp_path, monkeypatch):
    """tasks/sensat_urban/pmf on a synthetic train / val tree in is_debug mode with a small model"""
    import yaml
    root = str(tmp_path / "data")
    E.write_tree(root, "train", frames=(("birmingham_block_0", 70, 100, 9000), ("cambridge_block_9", 66, 80, 5000)), seed=1)
    E.write_tree(root, "val", seed=2)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tasks", "sensat_urban", "pmf", "config_server.yaml")))
    cfg.update(save_path=str(tmp_path / "exp"), data_root=root, is_debug=True, n_epochs=1, batch_size=[2, 2], img_h=32,
               img_w=32, val_img_h=32, val_img_w=32, n_samples_split=40000, base_channels=32, img_backbone="resnet34", imagenet_pretrained=False, gpu="0")
    path = str(tmp_path / "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    task = os.path.join(ROOT, "tasks", "sensat_urban", "pmf")
    monkeypatch.syspath_prepend(task)
    for m in ("option", "trainer", "main"):
        monkeypatch.delitem(sys.modules, m, raising=False)
    import option
    import trainer
    from pmf_amd.checkpoint import Recorder
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    s = option.Option(path)
    torch.manual_seed(s.seed)
    random.seed(s.seed)
    model = deterministic_init(PMFNet(5, 3, s.nclasses, s.base_channels, imagenet_pretrained=False,
                                      image_backbone=s.img_backbone))
    t = trainer.Trainer(s, model, Recorder(s, s.save_path, use_tensorboard=False))
    assert t.train_loader.loader.is_train and len(t.train_loader) >= 1 and len(t.val_loader) >= 1
    assert isinstance(t.train_loader.loader.dataset, SensatUrban)
    res = t.run(0, mode="Train")
    assert set(res) == {"Acc", "IOU", "Recall", "last"}
    assert t.engine.iteration == 1 and torch.isfinite(torch.tensor(t.last_summary["Loss"])).item()
    res = t.run(0, mode="Validation")
    assert set(res) == {"Acc", "IOU", "Recall", "last"} and all(v == v for v in res.values())
    assert torch.isfinite(torch.tensor(t.last_summary["Loss"])).item()
    for m in ("option", "trainer", "main"):
        sys.modules.pop(m, None)
