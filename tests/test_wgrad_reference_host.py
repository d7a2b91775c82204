"""Host side (no GPU) of the direct weight-gradient tests: tests/wgrad_cases.py is what tests/test_gpu_wgrad.py holds
conv_wgrad.hip to, so it is held to something else here.
  * the numpy reference against float64 torch.autograd of F.conv2d on every case (a PMF_SRC_BCAST operand expanded to the map
    the kernels give it), tap subsets against the full window of the same case;
  * the family table: every case reaches the kernel family it names under PMF_WGRAD_S3 set / clear and the three environments
    (pmf_conv_wgrad_variant launches nothing); over the table all eight PMF_WG_* families, wgrad_fewc_k's four KG
    instantiations, N-split's NCO 1 / 2 / 4, RAG true / false, XSL 7 / 9 and the pixel-split form, both stage-2 forms;
  * the exactness conditions of the bit-equality test for every generated input, so the GPU test cannot silently run on
    inputs for which equality is not owed;
  * the argument guards of pmf_conv_wgrad / _partial / _reduce: each returns PMF_E_ARG before any HIP call."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402
from tests import wgrad_cases as W  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
NAMES = [c.name for c in W.CASES]
SWITCHES = ("PMF_WG_S3N", "PMF_WGRAD_WGS")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in W.ENVS[env].items():
        monkeypatch.setenv(k, v)


def _autograd_dw(case, inp):
    """float64 autograd of F.conv2d over the transformed, concatenated operands (transform restated in torch)"""
    k, dil, pad = case.conv
    xs = []
    for i, s in enumerate(case.srcs):
        x = torch.from_numpy(inp["x"][i][..., :s.C].copy())
        if inp["scale"][i] is not None:
            x = x * torch.from_numpy(inp["scale"][i]) + torch.from_numpy(inp["shift"][i])       # float32, like the kernels
        if s.relu:
            x = x.clamp_min(0)
        if inp["cmul"][i] is not None:
            x = x * torch.from_numpy(inp["cmul"][i][:, :s.C].copy())[:, None, None, :]
        x = x.double()
        if s.bcast:
            x = x.expand(case.N, case.OH * case.stride, case.OW * case.stride, s.C)
        xs.append(x.permute(0, 3, 1, 2))
    x = torch.cat(xs, 1)[:, :case.Cin_real].contiguous()
    w = torch.zeros(case.Cout, case.Cin_real, k, k, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x, w, None, case.stride, pad, dil)
    assert tuple(out.shape) == (case.N, case.Cout, case.OH, case.OW)
    dz = torch.from_numpy(inp["dz"][..., :case.Cout].copy()).double().permute(0, 3, 1, 2)
    (out * dz).sum().backward()
    return w.grad.reshape(case.Cout, case.Cin_real, k * k).numpy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_float64_autograd(name):
    """both sides sum the same npix float64 products per weight in their own order: |difference| <= 2 npix eps64 S (each
    side within npix eps64 S of the exact sum, S = sum |terms|)"""
    case = W.BY_NAME[name]
    inp = W.inputs(case, "random")
    dw, S, db = W.reference(case, inp)
    assert not np.isnan(dw).any()
    want = _autograd_dw(case, inp)
    bound = 2 * case.npix * EPS64 * S
    err = np.abs(dw - want)
    assert (err <= bound + 1e-300).all(), "%s: worst %.3e of bound" % (name, float((err / (bound + 1e-300)).max()))
    assert np.abs(want).max() > 0
    # dbias against an exactly rounded column sum (math.fsum): five float32 rows, within 5 eps64 of the sum of their magnitudes
    rows = inp["rows"][:, :case.Cout].astype(np.float64)
    exact = np.array([math.fsum(rows[:, c]) for c in range(case.Cout)])
    assert (np.abs(db - exact) <= 5 * EPS64 * np.abs(rows).sum(0)).all()


@pytest.mark.parametrize("name", W.SUBSET_CASES)
def test_tap_subset_reference_is_the_full_window_without_the_dropped_taps(name):
    case = W.BY_NAME[name]
    sub = case.tap_subset()
    k = case.conv[0]
    assert len(sub.taps) == (k - 1) ** 2 and len(sub.dropped) == 2 * k - 1
    inp = W.inputs(case, "exact")
    full = W.reference(case, inp)[0]
    part = W.reference(sub, inp)[0]
    assert np.isnan(part[:, :, sub.dropped]).all()
    assert np.array_equal(part[:, :, sub.widx], full[:, :, sub.widx])


def test_reference_detects_a_shifted_tap_and_a_lost_pixel():
    """the reference is sensitive to what the GPU test is for: one tap read a column off, or one pixel of dz dropped, changes
    integers of the exact inputs"""
    case = W.BY_NAME["fewc_7x7_c3"]
    inp = W.inputs(case, "exact")
    ref = W.reference(case, inp)[0]
    moved = W.Case("m", case.N, case.OH, case.OW, case.srcs, case.Cout, [(dy, dx + (i == 48)) for i, (dy, dx) in enumerate(case.taps)],
                   case.KHW, None, 1, 0, case.dz_ldc, case.Cin_real)
    assert not np.array_equal(W.reference(moved, inp)[0], ref)
    lost = dict(inp, dz=inp["dz"].copy())
    lost["dz"][0, case.OH - 1, case.OW - 1, :case.Cout] = 0
    assert not np.array_equal(W.reference(case, lost)[0], ref)


# ------------------------------------------------------------------------------------------------ family table
@pytest.mark.parametrize("env", list(W.ENVS))
def test_every_case_reaches_the_family_it_names(env, monkeypatch):
    _env(monkeypatch, env)
    lib = L.lib()
    bad = []
    for case in W.CASES:
        for s3 in (1, 0):
            d = W.host_desc(case, s3, dbias=case.dbias)
            got = lib.pmf_conv_wgrad_variant(C.byref(d))
            if got != W.FAM[case.fam[(s3, env)]]:
                bad.append((case.name, s3, W.FAM_NAME.get(got, got), case.fam[(s3, env)]))
            # the plan's pointer-free probe sizes the workspace: the same split count as the descriptor that is launched
            p = W.host_desc(case, s3, transforms=False)
            p.dz = p.partial = p.dw_oihw = None
            p.dz_ldc = 0
            for i in range(L.MAX_SRC):
                p.src[i].x = None
                p.src[i].flags = 0
            if lib.pmf_conv_wgrad_nsplit(C.byref(p)) != lib.pmf_conv_wgrad_nsplit(C.byref(d)):
                bad.append((case.name, s3, "probe nsplit", lib.pmf_conv_wgrad_nsplit(C.byref(p)), lib.pmf_conv_wgrad_nsplit(C.byref(d))))
    assert not bad, bad


def test_table_covers_every_family_and_instantiation():
    inst = [(c.name, s3, env, W.instantiation(c, s3, env)) for c in W.CASES for s3 in (1, 0) for env in W.ENVS]
    fams = {i[3]["family"] for i in inst}
    assert fams == set(W.FAM), fams                                             # all eight PMF_WG_*
    assert {W.FAM[f] for f in fams} == {L.WG_UNIT, L.WG_PIPE, L.WG_SWP, L.WG_NSPLIT, L.WG_DIRECT, L.WG_DIRECT_S3, L.WG_STREAM,
                                        L.WG_FEWC}

    def over(fam, key):
        return {i[3][key] for i in inst if i[3]["family"] == fam}
    assert over("FEWC", "KG") == {1, 2, 3, 5}                                   # wgrad_fewc_k<1 / 2 / 3 / 5>
    assert over("NSPLIT", "NCO") == {1, 2, 4}
    assert {(i[3]["RAG"], i[3]["XSL"]) for i in inst if i[3]["family"] == "NSPLIT"} == {(r, x) for r in (True, False) for x in (7, 9)}
    assert over("SWP", "XSL") == {7, 9} and over("PIPE", "XSL") == {7, 9}       # (SWP: the pixel-split form)
    assert over("UNIT", "NT") == {1, 2, 4}
    # the ragged 16-pixel group / odd pixel counts the issue asks for
    assert W.BY_NAME["direct_96_32"].npix >= 16384 and W.BY_NAME["direct_96_32"].npix % 16 and W.BY_NAME["direct_96_32"].npix % 2
    assert W.BY_NAME["ds3_64_64_floor"].npix == 4096 and W.BY_NAME["ds3_512_64"].npix == 1024
    assert W.BY_NAME["ds3_64+128_80_odd"].npix % 2 and W.BY_NAME["stream_64+16_16_odd"].npix % 2


def test_stage2_plans_cover_both_forms(monkeypatch):
    _env(monkeypatch, "default")
    lib = L.lib()
    kinds = {}
    for name in W.RED_MULTI:
        case = W.BY_NAME[name]
        d = W.host_desc(case, 1, dbias=case.dbias)
        d.nsplit = lib.pmf_conv_wgrad_nsplit(C.byref(d))
        meta = (C.c_int32 * 8)()
        assert lib.pmf_conv_wgrad_reduce_plan(C.byref(d), meta) == meta[5] * meta[6] > 0
        kinds.setdefault(meta[1], []).append(case)
    assert set(kinds) == {0, 1}
    for k, cs in kinds.items():          # in both forms: dropped padded channels and a ragged last output-channel tile
        assert any(c.Cin_real < c.Ktot for c in cs) and any(c.Cout % 32 for c in cs), k
    assert any(W.BY_NAME[n].dbias for n in W.RED_MULTI)


# ------------------------------------------------------------------------------------------------ exactness conditions
@pytest.mark.parametrize("name", NAMES)
def test_exact_inputs_meet_the_exactness_conditions(name):
    case = W.BY_NAME[name]
    inp = W.inputs(case, "exact")
    assert W.exactness(case, inp) == []
    if name in W.SUBSET_CASES:
        assert W.exactness(case.tap_subset(), inp) == []
    # padding lanes hold NaN: neither may reach the gradient
    assert np.isnan(inp["dz"][..., case.Cout:]).all()
    for i, s in enumerate(case.srcs):
        assert np.isnan(inp["x"][i][..., s.C:]).all()
    if len(case.srcs) == 1:
        assert np.isnan(inp["x"][0][..., case.Cin_real:]).all()
    ref, S, db = W.reference(case, inp)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)       # the float32 conversion is exact
    assert np.array_equal(ref / W.LSB, np.round(ref / W.LSB))


def test_exactness_check_notices_inputs_that_do_not_qualify():
    case = W.BY_NAME["tile_3x3_64_64_8x64"]
    inp = W.inputs(case, "exact")
    a = dict(inp, dz=inp["dz"] + np.float32(1 / 8))
    assert W.exactness(case, a)
    b = dict(inp, x=[inp["x"][0] * np.float32(64)])
    assert W.exactness(case, b)
    assert W.exactness(case, W.inputs(case, "random"))


@pytest.mark.parametrize("name", ["tile_3x3_64_64_15x80", "ds3_64+128_80_odd", "stream_32_20", "direct_64+128_80"])
def test_onehot_inputs_leave_one_term_per_weight(name):
    case = W.BY_NAME[name]
    ns = W.default_nsplit(case, 1)
    inp = W.inputs(case, "onehot_dz", ns)
    z = inp["dz"][..., :case.Cout].reshape(-1, case.Cout)
    assert ((z != 0).sum(0) == 1).all()
    nz = z[z != 0]
    assert np.array_equal(np.abs(nz), 2.0 ** np.round(np.log2(np.abs(nz))))
    used = {int(p) for p in np.nonzero(z)[0]}
    sp = W.special_pixels(case, ns)
    assert used <= set(sp) and {0, case.npix - 1} <= set(sp)
    assert all(s is None for s in inp["scale"])                                 # no affine map: in_t is the float32 operand itself
    # every weight is one operand value times a power of two: the float32 conversion of the reference is exact
    ref = W.reference(case, inp)[0]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    inx = W.inputs(case, "onehot_x", ns)
    for i, s in enumerate(case.srcs):
        x = inx["x"][i][..., :s.C].reshape(-1, s.C)
        assert ((x != 0).sum(0) == 1).all()
    ref = W.reference(case, inx)[0]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)


# ------------------------------------------------------------------------------------------------ guards
def _base():
    case = W.BY_NAME["unit_1x1_32_20"]
    return W.host_desc(case, 1, nsplit=2, dbias=True)


def _set(field, value):
    def f(d):
        setattr(d, field, value)
    return f


def _src(field, value, i=0):
    def f(d):
        setattr(d.src[i], field, value)
    return f


def _widx(value):
    def f(d):
        d.tap_widx[0] = value
    return f


GUARDS = [("null dz", _set("dz", None)), ("null partial", _set("partial", None)), ("null dw_oihw", _set("dw_oihw", None)),
          ("null operand", _src("x", None)), ("N = 0", _set("N", 0)), ("OH = 0", _set("OH", 0)), ("OW = -1", _set("OW", -1)),
          ("Cout = 0", _set("Cout", 0)), ("KHW = 0", _set("KHW", 0)), ("Cin_real = 0", _set("Cin_real", 0)),
          ("Cin_real > Ktot", _set("Cin_real", 33)), ("tap_widx = KHW", _widx(1)), ("tap_widx < 0", _widx(-1)),
          ("dbias_rows without dbias_out", _set("dbias_out", None)), ("dbias_ld < Cout", _set("dbias_ld", 19)),
          ("dz_ldc < Cout", _set("dz_ldc", 16)), ("in_stride = 0", _set("in_stride", 0)), ("in_stride = 3", _set("in_stride", 3)),
          # (from before this file: kept pinned next to the new ones)
          ("nsplit = 0", _set("nsplit", 0)), ("reserved0", _set("reserved0", 1)), ("C % 8", _src("C", 20)), ("nsrc = 0", _set("nsrc", 0))]


@pytest.mark.parametrize("what,breaker", GUARDS, ids=[g[0] for g in GUARDS])
def test_guards_refuse_before_any_launch(what, breaker):
    """every descriptor here is INVALID in exactly one field; the three entry points must return PMF_E_ARG before any HIP call
    (as test_formerly_unbound_entry_point_takes_a_64_bit_stream relies on: this runs without a GPU, on made-up pointers)"""
    lib = L.lib()
    d = _base()
    breaker(d)
    for fn in (lib.pmf_conv_wgrad, lib.pmf_conv_wgrad_partial, lib.pmf_conv_wgrad_reduce):
        assert fn(C.byref(d), None) == L.PMF_E_ARG, what


def test_a_tap_index_beyond_the_window_is_refused_for_every_tap():
    """dw_oihw[(co * Cin_real + k) * KHW + tap_widx[t]]: an index >= KHW is a write beyond the weight's own window -- into the
    next weight, and beyond the flat gradient buffer for the last one"""
    lib = L.lib()
    case = W.BY_NAME["tile_3x3_64_64_8x64"]
    for t in range(9):
        d = W.host_desc(case, 1, nsplit=1)
        d.tap_widx[t] = 9
        assert lib.pmf_conv_wgrad_reduce(C.byref(d), None) == L.PMF_E_ARG
    sub = case.tap_subset()
    d = W.host_desc(sub, 1, nsplit=1)
    assert sub.widx == [1, 2, 4, 5]
    d.KHW = 5                                  # the largest kept window index is now out of range
    assert lib.pmf_conv_wgrad(C.byref(d), None) == L.PMF_E_ARG


def test_streaming_family_refuses_a_split_count_that_is_no_multiple_of_N(monkeypatch):
    """the one family that cannot take every split count: its workgroups stay inside one sample (grid.x = N * S)"""
    _env(monkeypatch, "default")
    lib = L.lib()
    case = W.BY_NAME["stream_32_20"]
    d = W.host_desc(case, 1, nsplit=3)
    assert lib.pmf_conv_wgrad_variant(C.byref(d)) == L.WG_STREAM and case.N == 2
    assert lib.pmf_conv_wgrad(C.byref(d), None) == L.PMF_E_ARG
    assert lib.pmf_conv_wgrad_partial(C.byref(d), None) == L.PMF_E_ARG


def test_host_queries_keep_accepting_the_pointer_free_probe():
    lib = L.lib()
    case = W.BY_NAME["tile_3x3_64_64_8x64"]
    p = L.WgradDesc()
    full = W.host_desc(case, 1)
    p.N, p.OH, p.OW, p.Cout, p.nsrc = case.N, case.OH, case.OW, case.Cout, 1
    p.src[0].C, p.src[0].ldc, p.src[0].H, p.src[0].W = 64, 64, case.OH, case.OW
    p.ntaps = 9
    for t, (dy, dx) in enumerate(case.taps):
        p.tdy[t], p.tdx[t], p.tap_widx[t] = dy, dx, t
    p.in_stride, p.Cin_real, p.KHW, p.flags, p.nsplit = 1, 64, 9, L.WGRAD_S3, 1
    ns = lib.pmf_conv_wgrad_nsplit(C.byref(p))
    assert ns == lib.pmf_conv_wgrad_nsplit(C.byref(full)) >= 1
    p.nsplit = ns
    assert lib.pmf_conv_wgrad_workspace(C.byref(p)) == ns * 9 * 64 * 64 * 4
    assert lib.pmf_conv_wgrad_variant(C.byref(p)) == lib.pmf_conv_wgrad_variant(C.byref(full))


def test_empty_split_counts_leave_splits_without_a_pixel():
    """what the GPU test runs as `a split count above the number of pixel tiles`: at least one split owns nothing"""
    for case in W.CASES:
        for s3 in (1, 0):
            fam = case.fam[(s3, "default")]
            n = W.empty_split_count(case, s3, fam)
            if fam == "STREAM":
                assert n % case.N == 0
                S, units = n // case.N, (case.OH * case.OW + 1) // 2
                assert (S - 1) * -(-units // S) >= units
            elif fam == "DIRECT":
                units = (case.npix + 1) // 2
                assert (n - 1) * -(-units // n) >= units
            elif fam == "DIRECT_S3":
                units = (case.npix + 15) // 16
                assert (n - 1) * -(-units // n) >= units
            else:
                assert n > W.pixel_tiles(case)
            assert n * len(case.taps) * case.Ktot * ((case.Cout + 31) // 32 * 32) * 4 < 64 << 20       # a modest workspace
