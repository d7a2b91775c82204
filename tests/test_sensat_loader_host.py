"""SensatLoader without a GPU: the order and ranges of the draws, the index list, the validation of frames, the struct, the
second header of the binding (include/pmf_amd_sensat.h) and the guards of the two entry points of csrc/bev_train.hip, which
answer before any HIP call.  Host only."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from pmf_amd import _lib as L
from pmf_amd.dataset import SensatLoader
from tests import sensat_loader_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loader(names, **kw):
    H, W = S.FRAMES[names[0]][2:]
    kw.setdefault("n_samples_split", 20000)             # 9 samples of frame A, 4 of B, 7 of C
    return SensatLoader(S.FrameSet(names), img_h=H, img_w=W, device="cpu", **kw)


def test_surface_is_exported_under_both_names():
    import pc_processor
    import pmf_amd.dataset
    assert pc_processor.dataset.SensatLoader is pmf_amd.dataset.SensatLoader is SensatLoader
    import pc_processor.dataset.sensat_urban.sensat_loader as m
    assert m.SensatLoader is SensatLoader


def test_draw_order_and_ranges_match_a_hand_written_sequence():
    ld = _loader(["A"])
    h, w, H, W = S.FRAMES["A"]
    for seed in range(5):
        torch.manual_seed(seed)
        got = ld.draw(h, w)
        torch.manual_seed(seed)
        i1 = int(torch.randint(0, h - 2 * H + 1, size=(1,)).item())
        j1 = int(torch.randint(0, w - 2 * W + 1, size=(1,)).item())
        angle = float(torch.empty(1).uniform_(-360., 360.).item())
        i2 = int(torch.randint(0, 2 * H - H + 1, size=(1,)).item())
        j2 = int(torch.randint(0, 2 * W - W + 1, size=(1,)).item())
        hflip = bool(torch.rand(1) < 0.5)
        vflip = bool(torch.rand(1) < 0.5)
        assert got == (i1, j1, angle, i2, j2, hflip, vflip)
        after = torch.rand(1)
        torch.manual_seed(seed)
        ld.draw(h, w)
        assert torch.equal(torch.rand(1), after)                 # and nothing else was consumed
    torch.manual_seed(0)
    seen = [ld.draw(h, w) for _ in range(400)]
    assert {c[0] for c in seen} == set(range(h - 2 * H + 1)) and {c[1] for c in seen} == set(range(w - 2 * W + 1))
    assert {c[3] for c in seen} == set(range(H + 1)) and {c[4] for c in seen} == set(range(W + 1))
    assert all(-360. <= c[2] <= 360. for c in seen) and min(c[2] for c in seen) < -300 and max(c[2] for c in seen) > 300
    assert {c[5] for c in seen} == {True, False} and {c[6] for c in seen} == {True, False}


def test_frame_of_exactly_the_first_crop_draws_two_randint_fewer():
    ld = _loader(["B"])
    h, w, H, W = S.FRAMES["B"]
    assert (h, w) == (2 * H, 2 * W)
    torch.manual_seed(11)
    got = ld.draw(h, w)
    torch.manual_seed(11)
    angle = float(torch.empty(1).uniform_(-360., 360.).item())
    i2 = int(torch.randint(0, H + 1, size=(1,)).item())
    j2 = int(torch.randint(0, W + 1, size=(1,)).item())
    hflip = bool(torch.rand(1) < 0.5)
    vflip = bool(torch.rand(1) < 0.5)
    assert got == (0, 0, angle, i2, j2, hflip, vflip)


def test_jitter_order_is_rgb_first():
    random.seed(4)
    got = SensatLoader.draw_jitter()
    random.seed(4)
    assert got == (random.uniform(-0.2, 0.2), random.uniform(-2, 2))
    assert abs(got[0]) <= 0.2


def test_frame_idx_list_counts(capsys):
    class Sized(object):
        split = "train"

        def __init__(self, sizes):
            self.frames = [{"feature_map": np.zeros((8, h, w)), "label_map": np.zeros((h, w), np.int64)} for h, w in sizes]

        def readDataByIndex(self, i):
            return self.frames[i]

        def __len__(self):
            return len(self.frames)
    sizes = [(70, 113), (48, 80), (97, 64)]
    n_split = 200000
    ld = SensatLoader(Sized(sizes), img_h=24, img_w=32, n_samples_split=n_split, device="cpu")
    want = [int(n_split * h / 4000 * w / 4000) for h, w in sizes]
    assert want == [98, 48, 77]
    assert [ld.frame_idx_list.count(i) for i in range(3)] == want and ld.frame_idx_list == sorted(ld.frame_idx_list)
    assert len(ld) == ld.total_samples == sum(want) and ld.is_train and ld.split == "train"
    assert "Generate {} samples from train split".format(sum(want)) in capsys.readouterr().out
    assert ld.resident_bytes() == sum(33 * h * w for h, w in sizes)
    sampler = torch.utils.data.distributed.DistributedSampler(ld, num_replicas=2, rank=1, shuffle=True, drop_last=True)
    assert len(sampler) == sum(want) // 2
    assert len(ld.batches(4, sampler=sampler)) == len(sampler) // 4
    assert len(ld.batches(4)) == sum(want) // 4 and len(ld.batches(4, drop_last=False)) == -(-sum(want) // 4)
    val = SensatLoader(S.FrameSet(["A", "B"], split="val"), device="cpu")
    assert len(val) == 2 and not val.is_train and val.frames == []
    f, l = val[0]
    assert f.dtype == l.dtype == torch.float32
    assert torch.equal(f, torch.from_numpy(S.make_frame("A")["feature_map"]).float())
    assert torch.equal(l, torch.from_numpy(S.make_frame("A")["label_map"]).float())


def test_small_frame_and_bad_label_raise():
    ld = SensatLoader(S.FrameSet(["B"]), img_h=25, img_w=40, device="cpu")            # 48 < 2 * 25: at the first draw
    with pytest.raises(ValueError) as e:
        ld.draw(48, 80)
    assert str(e.value) == "Required crop size (50, 80) is larger than input image size (48, 80)"
    with pytest.raises(ValueError):
        SensatLoader(S.FrameSet(["B"]), img_h=24, img_w=41, device="cpu").draw(48, 80)
    ds = S.FrameSet(["A"])
    ds.all_data_frame[0]["label_map"][3, 5] = 200
    with pytest.raises(ValueError) as e:
        SensatLoader(ds, img_h=24, img_w=40, device="cpu")
    assert "[-1, 127]" in str(e.value)
    ds.all_data_frame[0]["label_map"][3, 5] = -2
    with pytest.raises(ValueError):
        SensatLoader(ds, img_h=24, img_w=40, device="cpu")


def test_no_cpu_path():
    ld = _loader(["A"])
    for call in (lambda: ld.batch([0]), lambda: ld[0], lambda: ld.count([ld.pack(0, (0, 0, 0.0, 0, 0, False, False))]),
                 lambda: next(iter(ld.batches(1)))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "no CPU fallback" in str(e.value)


def test_struct_packing_round_trip():
    assert C.sizeof(L.BevSample) == 72            # two pointers, six int32, four float, three int32/flags, two float, padded to 8
    assert [n for n, _ in L.BevSample._fields_] == ["feat", "label", "h", "w", "top1", "left1", "m0", "m1", "m3", "m4", "top2",
                                                    "left2", "flags", "jit_rgb", "jit_h"]
    assert (L.BEV_HFLIP, L.BEV_VFLIP) == (1, 2)
    ld = _loader(["A"])
    cand = (5, 17, 33.25, 24, 0, False, True)
    s = ld.pack(0, cand, (0.125, -1.5))
    feat, label = ld.frames[0]
    assert feat.shape == (70, 113, 8) and feat.dtype == torch.float32 and label.shape == (70, 113) and label.dtype == torch.int8
    assert torch.equal(feat.permute(2, 0, 1), torch.from_numpy(S.make_frame("A")["feature_map"]).float())
    back = L.BevSample.from_buffer_copy(bytes((L.BevSample * 1)(s)))
    r = math.radians(-33.25)
    f32 = lambda v: np.float32(v).item()
    assert (back.feat, back.label, back.h, back.w) == (feat.data_ptr(), label.data_ptr(), 70, 113)
    assert (back.top1, back.left1, back.top2, back.left2, back.flags) == (5, 17, 24, 0, L.BEV_VFLIP)
    assert (back.m0, back.m1, back.m3, back.m4) == (f32(math.cos(r)), f32(math.sin(r)), f32(-math.sin(r)), f32(math.cos(r)))
    assert (back.jit_rgb, back.jit_h) == (0.125, -1.5)
    assert ld.pack(0, (0, 0, 0.0, 0, 0, True, True)).flags == 3
    for bad in ((23, 0, 0.0, 0, 0, False, False), (0, 34, 0.0, 0, 0, False, False), (-1, 0, 0.0, 0, 0, False, False),
                (0, 0, 0.0, 25, 0, False, False), (0, 0, 0.0, 0, 41, False, False), (0, 0, 0.0, 0, -1, False, False)):
        with pytest.raises(ValueError):
            ld.pack(0, bad)


def test_second_header_is_read_strictly_and_bound():
    text = open(os.path.join(ROOT, "include", "pmf_amd_sensat.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = re.findall(r"\b(pmf_\w+)\s*\(([^()]*)\)\s*;", text)
    assert [n for n, _ in found] == L.EXPORTS_SENSAT == ["pmf_sizeof_sensat", "pmf_bev_sample_count", "pmf_bev_sample_gather"]
    first = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pmf_amd.h")).read(), flags=re.S)
    assert L.EXPORTS == re.findall(r"\b(pmf_\w+)\s*\([^()]*\)\s*;", first) and not set(L.EXPORTS) & set(L.EXPORTS_SENSAT)
    lib = L.lib()
    for name, params in found:
        nargs = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert getattr(lib, name).restype is C.c_int32
    assert lib.pmf_bev_sample_gather.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.pmf_sizeof_sensat() == C.sizeof(L.BevSample)
    # alone the header does not know pmf_stream_t: the first header's namespace is what makes it readable
    with pytest.raises(L.PMFLibraryError) as e:
        L.read_header(open(os.path.join(ROOT, "include", "pmf_amd_sensat.h")).read())
    assert "pmf_stream_t" in str(e.value)
    h = L.read_header(open(os.path.join(ROOT, "include", "pmf_amd_sensat.h")).read(), base=L._H)
    assert set(h.structs) == {"pmf_bev_sample_t"} and h.consts == {"PMF_BEV_HFLIP": 1, "PMF_BEV_VFLIP": 2}
    with pytest.raises(L.PMFLibraryError):
        L.read_header("int f(pmf_stream_t s, size_t n);", base=L._H)


def test_missing_second_header_is_reported():
    with pytest.raises(L.PMFLibraryError) as e:
        L._read(os.path.join(ROOT, "include", "no_such_sensat.h"), L._SENSAT_STRUCT_NAMES, L._H)
    assert "no_such_sensat.h not found" in str(e.value)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    p = 0x7F0000001000                        # never dereferenced: every call below is refused by its guard
    cnt, gat = lib.pmf_bev_sample_count, lib.pmf_bev_sample_gather
    E = L.PMF_E_ARG
    assert cnt(None, 1, 8, 8, p, None) == E and cnt(p, 1, 8, 8, None, None) == E
    assert cnt(p, 0, 8, 8, p, None) == E and cnt(p, -3, 8, 8, p, None) == E and cnt(p, 65536, 8, 8, p, None) == E
    assert cnt(p, 1, 0, 8, p, None) == E and cnt(p, 1, 8, 0, p, None) == E and cnt(p, 1, -8, -8, p, None) == E
    assert cnt(p, 1, 65536, 65536, p, None) == E and cnt(p, 1, 2 ** 31 - 1, 2, p, None) == E
    assert gat(None, 1, 8, 8, p, p, None) == E and gat(p, 1, 8, 8, None, p, None) == E and gat(p, 1, 8, 8, p, None, None) == E
    assert gat(p, 0, 8, 8, p, p, None) == E and gat(p, -1, 8, 8, p, p, None) == E and gat(p, 65536, 8, 8, p, p, None) == E
    assert gat(p, 1, 0, 8, p, p, None) == E and gat(p, 1, 8, -1, p, p, None) == E
    assert gat(p, 2, 46341, 46341, p, p, None) == E and gat(p, 2, 2 ** 31 - 1, 2 ** 31 - 1, p, p, None) == E


def test_general_angle_draws_are_well_conditioned():
    """the condition behind the cap of the GPU test: for every seeded draw that test uses, the restatement evaluated in
    float32 and in float64 differs in at most half the allowed pixels"""
    for name in ("A", "B", "C", "E"):
        h, w, H, W = S.FRAMES[name]
        ld = _loader([name])
        frame = S.make_frame(name)
        a32, a64 = S.all_map(frame), S.all_map(frame, torch.float64)
        torch.manual_seed(S.GENERAL_SEED[name])
        for k in range(10):
            cand = ld.draw(h, w)
            differ = int((S.ref_augment(a32, cand, H, W).double() != S.ref_augment(a64, cand, H, W)).any(0).sum())
            assert differ <= S.cap(H, W) / 2, (name, k, differ)
