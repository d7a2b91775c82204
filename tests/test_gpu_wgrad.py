"""-m gpu: the weight-gradient kernels of csrc/conv_wgrad.hip called directly through the C ABI -- pmf_conv_wgrad,
pmf_conv_wgrad_partial, pmf_conv_wgrad_reduce, pmf_conv_wgrad_reduce_plan / _multi on descriptors the test fills itself --
against the float64 reference of tests/wgrad_cases.py, which tests/test_wgrad_reference_host.py holds to float64 autograd and
whose family table it pins (all eight PMF_WG_* families, every instantiation of the few-channel and N-split kernels).

Every buffer sits between two guard bands of 4 KiB of a NaN-payload sentinel that must be bit-unchanged afterwards; inputs must
be bit-unchanged as a whole.  `partial` is EXACTLY pmf_conv_wgrad_workspace() bytes of that NaN: a slab element stage 2 reads
and stage 1 never wrote shows as a NaN weight.  dz columns [Cout, dz_ldc), the operands' pitch padding [C, ldc) and, for
single-operand cases, the operand channels [Cin_real, C) hold NaN: none may reach dw_oihw.
  a. EXACT (every case, PMF_WGRAD_S3 set and clear, the environments of WGRAD_VARIANT_ENVS): inputs on which no summation order
     can round (wgrad_cases.exactness, asserted on the host): dw_oihw must equal the float64 reference converted to float32 BIT
     FOR BIT, on the fp32 and the split-bf16 families alike -- a lost, doubled or misplaced pixel, tap, channel or split changes
     an integer.  Variations: two runs, nsplit = 1 (N for the streaming kernel), a split count with EMPTY splits (every family
     supports it: their pixel loops start beyond their end and the cleared accumulators are stored -- read in conv_wgrad.hip;
     the NaN workspace would show a slab that was not written), accumulate = 1 over a pre-filled gradient, dbias rows with
     dbias_ld > Cout added to a pre-filled dbias_out, tap subsets with tap_widx from the full window.
  b. ONE-HOT: dz zero but for one power of two per output channel (corners, tile seams, the ragged remainder, first / last pixel
     of a split), operands with full 24-bit mantissas -- and the mirror image.  Every weight is one float32 value times a power
     of two; the six kept plane products reconstruct hi + mid + lo exactly against a single-plane partner:
     equality.  This pins the mid and lo planes per lane.
  c. PRECISION: random full-mantissa inputs, r = |got - ref| / S per element under (1) the worst-case bound of the family's fp32
     accumulation, derived per kernel at chain_bound(), plus the fma allowance of _precision(), and (2) the project's yardstick: split-bf16 max r <= 4 x the fp32 family's on the
     same inputs + 1e-7 (the factor and floor of test_conv_fwd_split_bf16_vs_float64), fp32 families <= 4 x a float32 CPU
     evaluation of the same sum + 1e-7.  Every figure is printed and appended to wgrad_errors.txt in the
     directory PMF_TEST_OUT names (default test_out/), in the manner of s3_conv_errors.txt.
  d. pmf_conv_wgrad_reduce_multi over five layers (both stage-2 forms): bitwise what five pmf_conv_wgrad_reduce calls give."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from tests import wgrad_cases as W  # noqa: E402
from tests.gpu_helpers import BAND, SENT, GBuf, stream  # noqa: E402,F401

U32 = 2.0 ** -24
NAMES = [c.name for c in W.CASES]
TILE_NAMES = [n for n in NAMES if W.BY_NAME[n].fam[(1, "swp_pixel_split")] != W.BY_NAME[n].fam[(1, "default")]
              or W.instantiation(W.BY_NAME[n], 1, "nsplit_two_tiles") != W.instantiation(W.BY_NAME[n], 1, "default")]
S3_FAMILIES = ("SWP", "NSPLIT", "DIRECT_S3")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def f32_of(ref64):
    return (ref64 + 0.0).astype(np.float32)


class Inputs:
    """the device copies of one generated input set (shared by every launch on it) and its reference"""

    def __init__(self, case, mode, nsplit=1):
        self.case, self.inp = case, W.inputs(case, mode, nsplit)
        i = self.inp
        self.x = [GBuf(a.size, a) for a in i["x"]]

        def opt(a):
            return GBuf(a.size, a) if a is not None else None
        self.scale, self.shift, self.cmul = [opt(a) for a in i["scale"]], [opt(a) for a in i["shift"]], [opt(a) for a in i["cmul"]]
        self.dz, self.rows = GBuf(i["dz"].size, i["dz"]), GBuf(i["rows"].size, i["rows"])
        self.ref, self.S, self.dbias = W.reference(case, i)

    def all_inputs(self):
        return self.x + [b for b in self.scale + self.shift + self.cmul if b is not None] + [self.dz, self.rows]


@functools.lru_cache(maxsize=None)
def shared(name, mode, nsplit=1):
    return Inputs(W.BY_NAME[name], mode, nsplit)


def launch(I, s3, case=None, nsplit=None, accumulate=0, dbias=False, dw_prefill=None, phase="both", ws=None, check=True):
    """one pmf_conv_wgrad (or its stages) on a fresh NaN workspace of exactly the size the library asks for; returns
    (dw [Cout, Cin_real, KHW] float32, dbias_out or None, descriptor, buffers)"""
    lib = L.lib()
    case = case or I.case

    def p(b):
        return b.ptr if b is not None else 0
    dwn = case.Cout * case.Cin_real * case.KHW
    dw = GBuf(dwn, dw_prefill)
    db = GBuf(case.Cout, I.inp["db0"]) if dbias else None
    ptr = dict(x=[b.ptr for b in I.x], scale=[p(b) for b in I.scale], shift=[p(b) for b in I.shift], cmul=[p(b) for b in I.cmul],
               dz=I.dz.ptr, partial=0x1000, dw=dw.ptr, rows=I.rows.ptr, db=p(db))
    d = W.fill_desc(case, ptr, s3, 1, accumulate, dbias)
    d.nsplit = nsplit or lib.pmf_conv_wgrad_nsplit(C.byref(d))
    assert d.nsplit >= 1
    nbytes = lib.pmf_conv_wgrad_workspace(C.byref(d))
    assert nbytes == d.nsplit * len(case.taps) * case.Ktot * ((case.Cout + 31) // 32 * 32) * 4
    part = ws or GBuf(nbytes // 4)
    d.partial = part.ptr
    fn = {"both": lib.pmf_conv_wgrad, "partial": lib.pmf_conv_wgrad_partial, "reduce": lib.pmf_conv_wgrad_reduce}[phase]
    rc = fn(C.byref(d), stream())
    assert rc == 0, "%s: rc %d" % (case.name, rc)
    torch.cuda.synchronize()
    if check:
        what = "%s s3=%d nsplit=%d" % (case.name, s3, d.nsplit)
        for b in [part, dw] + ([db] if db else []):
            b.bands_ok(what)
        for b in I.all_inputs():
            b.unchanged(what)
    out = dw.body().reshape(case.Cout, case.Cin_real, case.KHW).copy() if phase != "partial" else None
    return out, (db.body().copy() if db is not None and phase != "partial" else None), d, dict(part=part, dw=dw, db=db)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d weights differ, first at (co, k, widx) = %s: got %r want %r" % (
            what, int(bad.sum()), bad.size, i, float(got[i]), float(want[i])))


def _env(monkeypatch, env):
    for k in ("PMF_WG_S3N", "PMF_WGRAD_WGS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in W.ENVS[env].items():
        monkeypatch.setenv(k, v)


def _family(case, s3):
    d = W.host_desc(case, s3)
    return W.FAM_NAME[L.lib().pmf_conv_wgrad_variant(C.byref(d))]


# ------------------------------------------------------------------------------------------------ a. exact structure
def _exact_runs(name, s3, env):
    case = W.BY_NAME[name]
    I = shared(name, "exact")
    fam = _family(case, s3)
    assert fam == case.fam[(s3, env)], (name, s3, env, fam)
    want = f32_of(I.ref)
    tag = "%s s3=%d %s %s" % (name, s3, env, fam)
    got, _, d, _ = launch(I, s3)
    assert_bits(got, want, tag + " default nsplit %d" % d.nsplit)
    again, _, _, _ = launch(I, s3)
    assert_bits(again, got, tag + " second run")
    one = case.N if fam == "STREAM" else 1
    got1, _, _, _ = launch(I, s3, nsplit=one)
    assert_bits(got1, want, tag + " nsplit %d" % one)
    ne = W.empty_split_count(case, s3, fam)
    gote, _, _, _ = launch(I, s3, nsplit=ne)
    assert_bits(gote, want, tag + " nsplit %d (empty splits)" % ne)
    return I, want, tag


@pytest.mark.parametrize("s3", [1, 0], ids=["s3", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_exact(name, s3, monkeypatch):
    _env(monkeypatch, "default")
    case = W.BY_NAME[name]
    I, want, tag = _exact_runs(name, s3, "default")
    # accumulate = 1 over a pre-filled integer gradient (+ the bias fold into a pre-filled dbias_out)
    dw0 = I.inp["dw0"]
    got, db, _, _ = launch(I, s3, accumulate=1, dbias=case.dbias, dw_prefill=dw0)
    assert_bits(got, f32_of(dw0.astype(np.float64) + I.ref), tag + " accumulate")
    if case.dbias:
        assert_bits(db, f32_of(I.inp["db0"].astype(np.float64) + I.dbias), tag + " dbias")
        # without accumulate the bias fold still ADDS (the plan zeroes the flat gradient once per step)
        got, db, _, _ = launch(I, s3, dbias=True)
        assert_bits(got, want, tag + " dbias, accumulate = 0")
        assert_bits(db, f32_of(I.inp["db0"].astype(np.float64) + I.dbias), tag + " dbias, accumulate = 0")


@pytest.mark.parametrize("env", ["swp_pixel_split", "nsplit_two_tiles"])
@pytest.mark.parametrize("name", TILE_NAMES)
def test_exact_variant_environments(name, env, monkeypatch):
    _env(monkeypatch, env)
    _exact_runs(name, 1, env)


@pytest.mark.parametrize("s3", [1, 0], ids=["s3", "f32"])
@pytest.mark.parametrize("name", W.SUBSET_CASES)
def test_exact_tap_subset(name, s3, monkeypatch):
    """the window without its last row and first column, tap_widx from the full window: the kept entries equal the full
    window's, the dropped entries of dw_oihw keep their pre-filled bits"""
    _env(monkeypatch, "default")
    case = W.BY_NAME[name]
    sub = case.tap_subset()
    I = shared(name, "exact")
    ref = W.reference(sub, I.inp)[0]
    dw0 = I.inp["dw0"]
    for acc in (0, 1):
        got, _, d, _ = launch(I, s3, case=sub, accumulate=acc, dw_prefill=dw0)
        want = dw0.astype(np.float64).copy()
        want[:, :, sub.widx] = ref[:, :, sub.widx] + (dw0[:, :, sub.widx] if acc else 0)
        assert_bits(got, f32_of(want), "%s s3=%d accumulate=%d %s" % (sub.name, s3, acc, _family(sub, s3)))
    got, _, _, _ = launch(I, s3, case=sub)                      # over the NaN sentinel: the dropped entries keep ITS bits
    assert (bits(got[:, :, sub.dropped]).view(np.uint32) == SENT).all()
    assert_bits(got[:, :, sub.widx], f32_of(ref[:, :, sub.widx]), sub.name + " over the sentinel")


# ------------------------------------------------------------------------------------------------ b. one-hot planes
def _onehot(name, env):
    case = W.BY_NAME[name]
    fam = _family(case, 1)
    assert fam == case.fam[(1, env)] and fam in S3_FAMILIES
    ns = W.default_nsplit(case, 1)
    for mode in ("onehot_dz", "onehot_x"):
        I = shared(name, mode, ns)
        want = f32_of(I.ref)
        assert np.array_equal(want.astype(np.float64), I.ref)          # one term per weight: float32 holds it
        assert (want != 0).mean() > 0.02
        got, _, d, _ = launch(I, 1)
        assert d.nsplit == ns
        assert_bits(got, want, "%s %s %s %s" % (name, env, fam, mode))


@pytest.mark.parametrize("name", [n for n in NAMES if W.BY_NAME[n].fam[(1, "default")] in S3_FAMILIES])
def test_onehot_planes(name, monkeypatch):
    _env(monkeypatch, "default")
    _onehot(name, "default")


@pytest.mark.parametrize("name", [n for n in NAMES if W.BY_NAME[n].fam[(1, "swp_pixel_split")] == "SWP"
                                  and W.BY_NAME[n].fam[(1, "default")] != "SWP"])
def test_onehot_planes_pixel_split_form(name, monkeypatch):
    _env(monkeypatch, "swp_pixel_split")
    _onehot(name, "swp_pixel_split")


# ------------------------------------------------------------------------------------------------ c. precision
def chain_bound(case, inst, nsplit):
    """(L, c): a slab element is within (L + c) * 2^-24 * S of the float64 reference, before the fma allowance.

    The error of a float32 sum is bounded through the DEPTH of its longest chain: a term passes through `depth` additions and
    each rounds by at most 2^-24 of its result, so |error| <= depth * 2^-24 * sum |terms| (+ second order).  An fp32 MFMA
    (v_mfma_f32_32x32x2_f32) adds two products to the accumulator: depth 2, and each float32 product may round once (+ 1).  A
    bf16 MFMA (32x32x16) adds sixteen: depth 16 (taken as a chain; round to nearest assumed inside the MFMA); the plane products
    are exact in float32 (8 x 8 bits), six MFMAs per 16-pixel slab and tap, their absolute values summing to < 1.01 |a||b|;
    the three dropped products and the split's remainder stay below 2^-25 |a||b| (+ 1).  The waves' partial accumulators are
    folded through LDS in a fixed order by one wave: + (groups - 1).  T = ceil(pixel tiles / nsplit) tiles of 4 x 32 pixels per
    workgroup.  Per kernel, from its code (conv_wgrad.hip):
      conv_wgrad_k       PG = 4 / 2 / 1 pixel groups for U = TB * NT = 1 / 2 / more units: a wave runs 64 / PG MFMAs per tile
                         (wg_tile: its rows x 16 pixel pairs): 128 T / PG + PG - 1
      conv_wgrad_pipe_k  NT = 1, four pixel groups: 4 pairs x 2 rows x 2 halves = 16 MFMAs per tile: 32 T + 3
      wgrad_fewc_k       two pixel groups: 8 pairs x 2 rows x 2 halves = 32 MFMAs per tile: 64 T + 1
      wgrad_stream_k     per = ceil(pairs of a sample / S) pairs per workgroup, a wave takes 8 of every 32: 16 ceil(per / 32) + 3
      wgrad_1x1_k        per = ceil(pairs / nsplit), a wave takes 4 of every 16 pairs: 8 ceil(per / 16) + 3
      wgrad_1x1_s3_k     per = ceil(16-pixel groups / nsplit), a wave takes every fourth group, 6 MFMAs each: 96 ceil(per / 4) + 3
      conv_wgrad_s3_swp_k  a wave owns one slab of each half tile: 2 x 6 MFMAs per tile and tap: 192 T + 3
      conv_wgrad_s3n_k   NPX = 4 / NCO pixel groups, 8 / NPX slabs per wave and tile: 96 (8 / NPX) T + NPX - 1
    c = 4: stage 2 folds the slabs in float64 (no float32 chain) and converts once (1); the float32 cmul product, rounded on
    either side (2); second-order terms (1).  The affine map is NOT in c: see _precision."""
    fam = inst["family"]
    T = -(-W.pixel_tiles(case) // nsplit)
    if fam == "UNIT":
        tb = 1 if (case.gather or len(case.taps) == 1) else (4 if len(case.taps) <= 4 else 9)
        u = tb * inst["NT"]
        pg = 4 if u == 1 else (2 if u == 2 else 1)
        return 128 * T // pg + pg - 1 + 1, 4
    if fam == "PIPE":
        return 32 * T + 3 + 1, 4
    if fam == "FEWC":
        return 64 * T + 1 + 1, 4
    if fam == "STREAM":
        per = -(-((case.OH * case.OW + 1) // 2) // (nsplit // case.N))
        return 16 * -(-per // 32) + 3 + 1, 4
    if fam == "DIRECT":
        per = -(-((case.npix + 1) // 2) // nsplit)
        return 8 * -(-per // 16) + 3 + 1, 4
    if fam == "DIRECT_S3":
        per = -(-((case.npix + 15) // 16) // nsplit)
        return 1.01 * 96 * -(-per // 4) + 3 + 1, 4
    if fam == "SWP":
        return 1.01 * 192 * T + 3 + 1, 4
    assert fam == "NSPLIT"
    npx = 4 // inst["NCO"]
    return 1.01 * 96 * (8 // npx) * T + npx - 1 + 1, 4


def _log(line):
    out = os.environ.get("PMF_TEST_OUT", "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "wgrad_errors.txt"), "a") as f:
        f.write(line + "\n")
    print(line)


def _precision(name, env):
    """r = |got - ref| / S per element, S = sum |in_t| |dz| (the issue's abs-sum); max r over the elements with S > 0.
    Bar 1, per element: r <= (L + c) 2^-24 + 3 * 2^-24 * M / S, M = sum mag_t |dz| (wgrad_cases.mag_sum): the second term is the
    fma allowance -- some kernels evaluate x * scale + shift as one fma where the reference multiplies and adds in float32; the
    two differ by at most 2^-24 (|x scale| + 2 |v|) <= 3 * 2^-24 mag, ALSO where the ReLU leaves |in_t| = 0 (S = 0: |got - ref|
    <= 3 * 2^-24 M).  Bar 2, the yardsticks, on max r as it is."""
    case = W.BY_NAME[name]
    I = shared(name, "random")
    assert case.widx == list(range(len(case.taps)))
    S, M = I.S, W.mag_sum(case, I.inp)
    pos = S > 0

    def ratios(got):
        err = np.abs(got.astype(np.float64) - I.ref)
        assert np.isfinite(err).all()
        assert (err[~pos] <= 3 * U32 * M[~pos]).all()
        return err / np.where(pos, S, 1.0)
    r = {}
    for s3 in (1, 0):
        fam = _family(case, s3)
        assert fam == case.fam[(s3, env)]
        got, _, d, _ = launch(I, s3)
        rr = ratios(got)
        Lf, c = chain_bound(case, W.instantiation(case, s3, env), d.nsplit)
        bar1 = (Lf + c) * U32 + 3 * U32 * M / np.where(pos, S, 1.0)
        r[s3] = (fam, float(rr[pos].max()), Lf, c, d.nsplit, float((rr / bar1)[pos].max()))
    rc = float(ratios(W.reference(case, I.inp, np.float32)[0])[pos].max())
    for s3 in (1, 0):
        fam, m, Lf, c, ns, worst = r[s3]
        _log("%-28s %-16s s3=%d %-9s nsplit %4d  max r %.3e  (L + c) 2^-24 = (%.0f + %d) 2^-24 = %.3e  worst r / bar 1 %.4f  "
             "fp32 cpu %.3e" % (name, env, s3, fam, ns, m, Lf, c, (Lf + c) * U32, worst, rc))
    for s3 in (1, 0):
        fam, m, Lf, c, ns, worst = r[s3]
        assert worst <= 1, (name, s3, fam, worst)
        if fam in S3_FAMILIES:
            assert r[0][0] not in S3_FAMILIES
            assert m <= 4 * r[0][1] + 1e-7, "%s %s: split-bf16 %.3e vs fp32 family %s %.3e" % (name, fam, m, r[0][0], r[0][1])
        else:
            assert m <= 4 * rc + 1e-7, "%s %s: %.3e vs the float32 CPU evaluation %.3e" % (name, fam, m, rc)


@pytest.mark.parametrize("name", W.PRECISION)
def test_precision(name, monkeypatch):
    _env(monkeypatch, "default")
    _precision(name, "default")


def test_precision_pixel_split_form(monkeypatch):
    _env(monkeypatch, "swp_pixel_split")
    assert W.BY_NAME["tile_3x3_64_64_8x64"].fam[(1, "swp_pixel_split")] == "SWP"
    _precision("tile_3x3_64_64_8x64", "swp_pixel_split")


# ------------------------------------------------------------------------------------------------ d. batched stage 2
def test_reduce_multi_is_bitwise_the_single_reductions(monkeypatch):
    _env(monkeypatch, "default")
    lib = L.lib()
    jobs, single, kinds = [], [], set()
    for name in W.RED_MULTI:
        case = W.BY_NAME[name]
        I = shared(name, "random")
        dw0 = I.inp["dw0"]
        _, _, d, bufs = launch(I, 1, phase="partial", accumulate=1, dbias=case.dbias, dw_prefill=dw0)
        # five pmf_conv_wgrad_reduce calls on the same slabs, into buffers of their own
        dw, db, _, _ = launch(I, 1, phase="reduce", accumulate=1, dbias=case.dbias, dw_prefill=dw0, ws=bufs["part"], nsplit=d.nsplit)
        single.append((dw, db))
        jobs.append((case, I, d, bufs))
    descs = (L.WgradDesc * len(jobs))()
    meta = (C.c_int32 * (8 * len(jobs)))()
    total = 0
    for j, (case, I, d, bufs) in enumerate(jobs):
        C.memmove(C.addressof(descs[j]), C.addressof(d), C.sizeof(L.WgradDesc))
        row = (C.c_int32 * 8)()
        nb = lib.pmf_conv_wgrad_reduce_plan(C.byref(descs[j]), row)
        assert nb > 0
        row[0] = total
        total += nb
        kinds.add(row[1])
        meta[8 * j:8 * j + 8] = list(row)
    assert kinds == {0, 1}
    raw = np.frombuffer(bytes(descs), np.uint8)
    jobs_dev = torch.from_numpy(raw.copy()).to("cuda")
    meta_dev = torch.from_numpy(np.array(list(meta), np.int32)).to("cuda")
    assert jobs_dev.data_ptr() % 8 == 0
    rc = lib.pmf_conv_wgrad_reduce_multi(jobs_dev.data_ptr(), meta_dev.data_ptr(), len(jobs), total, stream())
    assert rc == 0
    torch.cuda.synchronize()
    for (case, I, d, bufs), (dw, db) in zip(jobs, single):
        for b in (bufs["part"], bufs["dw"]) + ((bufs["db"],) if bufs["db"] else ()):
            b.bands_ok(case.name)
        got = bufs["dw"].body().reshape(dw.shape)
        assert not np.isnan(got).any()
        assert_bits(got, dw, case.name + " batched vs single reduction")
        if case.dbias:
            assert_bits(bufs["db"].body(), db, case.name + " dbias, batched vs single")
