"""-m gpu: the forward / input-gradient convolution kernels -- every PIPE of conv_fwd_k, conv_finish_k (csrc/conv_fwd.hip), conv_ws_k
(csrc/conv_ws.hip) and the epilogue they share (csrc/conv_epi.h) -- called directly through pmf_conv_fwd on descriptors the test
fills itself (tests/conv_cases.py: forward form and the input-gradient form of plan_conv.py), against the float64 reference
that tests/test_conv_reference_host.py holds to float64 autograd; which kernel each launch reaches is pinned there too.

Every device buffer sits between two guard bands of 4 KiB of a NaN-payload sentinel that must be bit-unchanged afterwards; inputs
must be bit-unchanged as a whole.  `out` starts as the sentinel (or as an integer pre-fill under accumulate = 1): the pitch
padding [Cout, out_ldc), the pixels of the other parity classes and the pixels beyond OH x OW of a strided launch must keep
their bits.  The operands' pitch padding holds NaN, their padded channels [C_real, C) zero.  splitk_ws is EXACTLY K splits x one
slab of that NaN (a slab element read but never written shows as a NaN output); the ticket array is exactly one counter per
output tile and must read zero after every launch; stats is rows + 2 rows of NaN and exactly pmf_conv_fwd_stat_rows() rows
are written.
  a. EXACT: inputs on which no summation order can round (conv_cases.exactness, asserted on the host): `out` equals the
     restatement of conv_epi.h BIT FOR BIT, on the fp32 pack and the split-bf16 pack, for every tile / K-split / direct-taps /
     wave-scheduled cfg of conv_cases.launches; the statistics rows folded in float64 equal the expected column sums exactly
     where the outputs are integers, within n * 2^-53 * sum |term| elsewhere; two runs are bit-identical; a K split is run
     three times with tickets, once as two launches, once unsplit, and once with a workspace 4 bytes short (the library then
     splits one time fewer -- it has no error for that): all the same bits.  Parity classes into one map, merged launches
     against their per-operand launches, the 24 -> 32 case with the NaN band directly behind dz.
  b. ONE-HOT: one power of two per output column against full-mantissa operands, and one power of two per operand pixel
     against full-mantissa weights through the split pack: out = value * 2^e exactly -- the mid and lo planes, per lane.
  c. PRECISION: random full-mantissa inputs, r = |got - ref64| / S per element; fp32 families under the worst-case bound of
     chain_bound(), split-bf16 families within 4 x the fp32 family's max r + 1e-7; sigmoid at 4 x the error a float32 CPU
     evaluation of the same expression leaves.  Every figure is printed and appended to conv_errors.txt in the directory
     PMF_TEST_OUT names (default test_out/).
  d. the refusals include/pmf_amd.h documents at pmf_conv_fwd: a return code, nothing launched."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from tests import conv_cases as K  # noqa: E402
from tests.gpu_helpers import SENT, GBuf, stream  # noqa: E402

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24
NAMES = [c.name for c in K.CASES]
FORMS = [(c.name, wf) for c in K.CASES for wf in K.wforms(c)]
S3_FAMILIES = (5, 6, 7, 8, 10, 11, 12, 13, 14, 100)
PRECISION = ["f_1x1_16_20", "f_1x1_16+64_48", "f_1x1_3x64_80_full", "f_1x1_s2_64_128", "f_1x1_448_48_resident",
             "f_1x1_512_48_stream", "d_1x1_64_from512_stream", "d_2x2d2_merged_64+64", "f_1x1_1792_32", "f_2x2d2_16+64_48",
             "f_2x2d2_64_64", "f_3x3_64_128", "f_3x3d18_16_20_gather", "f_3x3_s2_64_128", "f_3x3_256_32_ksplit", "f_7x7_8_32_stem_view",
             "d_1x1_32_from20_k32", "d_3x3_32_from64", "d_3x3_256_from256_ksplit", "d_3x3_merged_32+64+32",
             "d_3x3_s2_64_from128.p01", "d_3x3_s2_64_from128.p11"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _p(b):
    return b.ptr if b is not None else 0


class Dev:
    """the device copies of one generated input set (shared by every launch on it) and its reference"""

    def __init__(self, case, mode, salt=0):
        self.case, self.inp = case, K.inputs(case, mode, salt)
        i = self.inp

        def opt(a):
            return GBuf(a.size, a) if a is not None else None
        self.x = [GBuf(a.size, a) for a in i["x"]]
        self.scale, self.shift, self.cmul = ([opt(a) for a in i[k]] for k in ("scale", "shift", "cmul"))
        self.bias, self.pmask = opt(i["bias"]), opt(i["pmask"])
        self.dst = [{k: opt(e[k]) for k in ("cmul", "relu_x", "rs", "rt", "mean")} for e in i["dst"]]
        self.G, self.S, self.M = K.reference(case, i)
        self.packs = {}

    def pack(self, wform):
        if wform not in self.packs:
            a = K.packs(self.case, self.inp, wform)
            self.packs[wform] = GBuf(a.size, a)
        return self.packs[wform]

    def unchanged(self, what):
        bufs = self.x + self.scale + self.shift + self.cmul + [self.bias, self.pmask] + list(self.packs.values())
        for e in self.dst:
            bufs += list(e.values())
        for b in bufs:
            if b is not None:
                b.unchanged(what)


@functools.lru_cache(maxsize=8)
def shared(name, mode, salt=0, plain=False):
    case = K.BY_NAME[name]
    return Dev(case.plain() if plain else case, mode, salt)


class Result:
    pass


def launch(case, dev, wform, cfg=0, split=False, tickets=False, outs=None, act=None, shrink=0):
    """one pmf_conv_fwd of `case` (dev.case itself, or one destination of it as a launch of its own) on fresh guarded outputs
    (or on `outs`), a NaN workspace of exactly the slabs the launch writes and a zeroed ticket array of exactly its tiles;
    returns the destinations [N, out_H, out_W, ldc], the statistics rows [rows, 2, C] float64 and what pmf_conv_fwd_variant
    says"""
    lib = L.lib()
    ks = [case.parent[1]] if case.parent is not None else list(range(len(case.dsts)))
    if outs is None:
        outs = [GBuf(dev.inp["dst"][k]["out0"].size, dev.inp["dst"][k]["out0"]) for k in ks]
    ptr = dict(x=[b.ptr for b in dev.x], scale=[_p(b) for b in dev.scale], shift=[_p(b) for b in dev.shift],
               cmul=[_p(b) for b in dev.cmul], w=dev.pack(wform).ptr, bias=_p(dev.bias) if case.bias else 0,
               pmask=_p(dev.pmask) if case.pmask else 0,
               dst=[dict(out=o.ptr, stats=K.FAKE, **{f: _p(dev.dst[k][f]) for f in ("cmul", "relu_x", "rs", "rt", "mean")})
                    for k, o in zip(ks, outs)])             # (stats: a stand-in until the row count is known)
    ws = tk = None
    if split:
        p = K.pick(case, wform, cfg, tickets)
        assert p["ksplit"] > 1 and p["ws_bytes"] == p["ksplit"] * K.slab_bytes(case)
        ws = GBuf((p["ws_bytes"] - shrink) // 4)
        ptr.update(ws=ws.ptr, ws_bytes=p["ws_bytes"] - shrink)
        if tickets:
            tk = GBuf(p["tickets"], np.zeros(p["tickets"], F32))
            ptr["tickets"] = tk.ptr
    d = K.fill_desc(case, ptr, wform, cfg, act)
    fam, info = K.variant(d)
    assert fam >= 0, (case.name, wform, cfg, fam)
    rows = lib.pmf_conv_fwd_stat_rows(C.byref(d))
    assert rows == info[4] and rows >= 1
    if split and not shrink:
        assert info[2] == p["ksplit"] and info[3] == (1 if tickets else 2)
    stats = []
    for j, dd in enumerate(case.dsts):
        sb = GBuf((rows + 2) * 2 * dd.C * 2) if dd.stat else None
        stats.append(sb)
        if sb is not None:
            if len(case.dsts) == 1:
                d.stats = sb.ptr
            else:
                d.dst[j].stats = sb.ptr
    what = "%s %s cfg %#x family %d" % (case.name, wform, cfg, fam)
    rc = lib.pmf_conv_fwd(C.byref(d), stream())
    if rc > 0:                             # a hipError_t: nothing that follows on this device would mean anything
        pytest.exit("%s: HIP error %d" % (what, rc), 3)
    assert rc == 0, "%s: rc %d" % (what, rc)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s: %s" % (what, e), 3)
    for b in outs + [b for b in stats + [ws, tk] if b is not None]:
        b.bands_ok(what)
    if tk is not None:
        assert not tk.body().view(np.uint32).any(), what + ": the ticket array does not read zero"
    r = Result()
    r.what, r.family, r.info, r.rows, r.outs = what, fam, info, rows, outs
    r.out = [o.body().reshape(dev.inp["dst"][k]["out0"].shape).copy() for k, o in zip(ks, outs)]
    r.stats = []
    for dd, sb in zip(case.dsts, stats):
        if sb is None:
            r.stats.append(None)
            continue
        a = sb.body().view(np.uint64).reshape(rows + 2, 2, dd.C)
        assert (a[rows:] == (SENT << 32 | SENT)).all(), what + ": more statistics rows written than pmf_conv_fwd_stat_rows()"
        a = a[:rows].view(F64)
        assert np.isfinite(a).all(), what + ": a statistics row was not written"
        r.stats.append(a.copy())
    return r


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at (n, y, x, c) = %s: got %r want %r" % (
            what, int(bad.sum()), bad.size, i, float(got[i]), float(want[i])))


def check_exact(case, r, exp, stats=True):
    for j, (dd, e) in enumerate(zip(case.dsts, exp)):
        assert_bits(r.out[j], e["full"], "%s dst %d" % (r.what, j))
        if dd.stat and stats:
            got = r.stats[j].sum(0)                            # the rows folded in float64 on the host
            if K.integer_outputs(case):
                assert np.array_equal(got, e["stat"]), "%s dst %d statistics: %r" % (r.what, j, np.abs(got - e["stat"]).max(1))
            else:
                assert (np.abs(got - e["stat"]) <= case.npix * 2.0 ** -53 * e["statabs"]).all(), "%s dst %d statistics" % (r.what, j)


def same_run(a, b, what, rows=True):
    for x, y in zip(a.out, b.out):
        assert_bits(x, y, what)
    for x, y in zip(a.stats, b.stats):
        if x is not None and rows:
            assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), what + ": statistics rows"


# ------------------------------------------------------------------------------------------------ a. exact structure
@pytest.mark.parametrize("name,wform", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_exact(name, wform):
    case = K.BY_NAME[name]
    dev = shared(name, "exact")
    exp = K.epilogue(case, dev.inp, K.f32_of(dev.G))
    for wf, cfg, split in K.launches(case):
        if wf != wform:
            continue
        if not split:
            r = launch(case, dev, wf, cfg)
            check_exact(case, r, exp)
            same_run(launch(case, dev, wf, cfg), r, r.what + " second run")
            continue
        runs = [launch(case, dev, wf, cfg, True, True) for _ in range(3)]          # combined inside the kernel: tickets
        check_exact(case, runs[0], exp)
        for r in runs[1:]:
            same_run(r, runs[0], r.what + " ticket form, again")
        two = launch(case, dev, wf, cfg, True, False)                               # conv_finish_k
        check_exact(case, two, exp)
        same_run(two, runs[0], two.what + " two-launch form against the ticket form", rows=False)
        one = launch(case, dev, wf, cfg & ~(0xff << 16))                            # no workspace: unsplit
        assert one.info[2] == 1
        same_run(one, runs[0], one.what + " unsplit against the ticket form", rows=one.rows == runs[0].rows)
        short = launch(case, dev, wf, cfg, True, True, shrink=4)                    # 4 bytes short: one split fewer
        assert short.info[2] == (runs[0].info[2] - 1 if runs[0].info[2] > 2 else 1)
        check_exact(case, short, exp)
    dev.unchanged(name)


@pytest.mark.parametrize("wform", ["f32", "s3"])
def test_exact_parity_classes_fill_one_map(wform):
    """the four parity launches of a stride-2 3x3 layer into ONE sentinel-then-zero map, in the order the plan issues them
    (accumulate = 1): the full gradient, the pitch padding untouched"""
    cases = [K.BY_NAME[n] for n in K.PARITY]
    devs = [shared(c.name, "exact") for c in cases]
    dd = cases[0].dsts[0]
    for cfg in (0, K.tile(32, 1), K.tile(64, 2)):
        cur = devs[0].inp["dst"][0]["out0"].copy()
        cur[..., :dd.C] = 0.0
        out = GBuf(cur.size, cur)
        for c, dev in zip(cases, devs):
            assert wform in K.wforms(c)
            inp = dict(dev.inp, dst=[dict(dev.inp["dst"][0], out0=cur)])
            cur = K.epilogue(c, inp, K.f32_of(dev.G))[0]["full"]
            r = launch(c, dev, wform, cfg, outs=[out])
            assert_bits(r.out[0], cur, r.what + " into the shared map")
        assert not np.isnan(cur[..., :dd.C]).any() and (cur[..., dd.C:].view(np.uint32) == SENT).all()
    for dev in devs:
        dev.unchanged("parity")


@pytest.mark.parametrize("name", K.MERGED)
def test_exact_merged_launch_is_its_per_operand_launches(name):
    case = K.BY_NAME[name]
    dev = shared(name, "exact")
    for wf, cfg, split in K.launches(case):
        if split:
            continue
        m = launch(case, dev, wf, cfg)
        for k, dd in enumerate(case.dsts):
            one = case.single(k)
            assert wf in K.wforms(one)
            r = launch(one, dev, wf, cfg)
            assert_bits(r.out[0], m.out[k], "%s against %s" % (m.what, r.what))
            if dd.stat:
                if r.rows == m.rows:
                    assert np.array_equal(r.stats[0].view(np.uint64), m.stats[k].view(np.uint64)), m.what + " statistics rows"
                assert np.array_equal(r.stats[0].sum(0), m.stats[k].sum(0)), m.what + " statistics"
    dev.unchanged(name)


# ------------------------------------------------------------------------------------------------ b. one-hot planes
@pytest.mark.parametrize("name,wform", [f for f in FORMS if f[1] != "f32"], ids=["%s-%s" % f for f in FORMS if f[1] != "f32"])
def test_onehot_planes(name, wform):
    plain = K.BY_NAME[name].plain()
    fams = set()
    for mode in ("onehot_w", "onehot_x"):
        for salt in (0, 1):
            dev = shared(name, mode, salt, True)
            want = K.f32_of(dev.G)
            assert np.array_equal(want.astype(F64), dev.G) and (want != 0).any()     # one term per output: float32 holds it
            exp = K.epilogue(plain, dev.inp, want)
            for wf, cfg, split in K.launches(plain):
                if wf != wform:
                    continue
                r = launch(plain, dev, wf, cfg, split, split)
                assert r.family in S3_FAMILIES
                fams.add(r.family)
                check_exact(plain, r, exp)
            dev.unchanged(name)
    assert fams


# ------------------------------------------------------------------------------------------------ c. precision
def chain_bound(case, ksplit):
    """(L, c): an output is within (L + c) * 2^-24 * S of the float64 reference, before the fma allowance of _precision.

    The error of a float32 sum is bounded through the DEPTH of its longest chain: a term that passes through `depth` additions,
    each rounding by at most 2^-24 of its result, contributes at most depth * 2^-24 * |term| (+ second order).  The fp32 kernels
    (conv_fwd_k PIPE 0, 1, 4) feed v_mfma_f32_32x32x2_f32: one MFMA adds two products to the accumulator, counted as depth 2,
    and one accumulator runs over all taps and all Ktot channels of its K range: L = ntaps * Ktot for the unsplit launch -- a
    term entered first passes through every later addition.  A K split shortens each chain to ntaps * Ktot / ksplit and adds
    the slab sum (ksplit - 1 additions): never more than the unsplit bound + ksplit.  Each product may round once: + 1.
    c = 6: the bias addition (1), LeakyReLU's 0.01 v (1), the product ecm * pm and the product with it (2), + old (1), second
    order (1).  The operand view is NOT in c: see _precision."""
    return len(case.taps) * case.C_real + ksplit + 1, 6


def _log(line):
    out = os.environ.get("PMF_TEST_OUT", "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "conv_errors.txt"), "a") as f:
        f.write(line + "\n")
    print(line)


def _ratios(case, dev, r, act=None):
    """per destination (r = |got - ref64| / S_e, S_e, M_e) on the launch's own pixels, S_e = S scaled by what the epilogue
    multiplies with (|ecm * pm|, 0 where the ReLU mask closes); where S_e = 0 the output is owed within the fma allowance"""
    ref = K.epilogue(case, dev.inp, dev.G, F64, act)
    out, c0 = [], 0
    for j, (dd, e) in enumerate(zip(case.dsts, dev.inp["dst"])):
        got = r.out[j][:, case.rows_y(), case.rows_x(), :dd.C].astype(F64)
        assert np.isfinite(got).all(), r.what
        scale = np.ones(got.shape)
        if e["cmul"] is not None:
            scale = scale * e["cmul"][:, None, None, :dd.C]
        if dev.inp["pmask"] is not None:
            scale = scale * dev.inp["pmask"][:, case.rows_y(), case.rows_x(), None]
        if dd.relu:
            x = e["relu_x"][:, case.rows_y(), case.rows_x(), :dd.C].astype(F64)
            t = x * e["rs"] + e["rt"] if e["rs"] is not None else x
            scale = scale * (t > 0)
        Se, Me = dev.S[..., c0:c0 + dd.C] * scale, dev.M[..., c0:c0 + dd.C] * scale
        err = np.abs(got - ref[j]["v"])
        assert (err[Se == 0] <= 3 * U32 * Me[Se == 0]).all(), r.what
        out.append((err / np.where(Se > 0, Se, 1.0), Se, Me))
        c0 += dd.C
    return out


@pytest.mark.parametrize("name", PRECISION)
def test_precision(name):
    """Bar 1 (fp32 families), per element: r <= (L + c) 2^-24 + 3 * 2^-24 * M / S.  The second term is the fma allowance: a
    kernel may evaluate the view's x * scale + shift as one fma where the reference multiplies and adds in float32; the two
    differ by at most 3 * 2^-24 * mag, also where the ReLU of the view leaves |in_t| = 0.  Bar 2 (split-bf16 families): max r
    <= 4 x the fp32 family's max r on the same inputs and cfg + 1e-7, the yardstick of test_conv_fwd_split_bf16_vs_float64."""
    case = K.BY_NAME[name]
    dev = shared(name, "random")
    runs, seen = [], set()
    for wf, cfg, split in K.launches(case):
        # the first unsplit and the first split launch of each weights form, and EVERY launch of the direct-taps kernel (13)
        # and of the wave-scheduled kernel (100: NCO 1, 2 and 4)
        fam = K.variant(K.host_desc(case, wf, cfg))[0]
        if (wf, split) in seen and (split or fam not in (13, 100)):
            continue
        seen.add((wf, split))
        runs.append((wf, cfg, split))
    worst = {}
    for wf, cfg, split in sorted(runs, key=lambda t: t[0] != "f32"):
        r = launch(case, dev, wf, cfg, split, split)
        Lf, c = chain_bound(case, r.info[2])
        m, w1 = 0.0, 0.0
        for rr, Se, Me in _ratios(case, dev, r):
            pos = Se > 0
            bar1 = (Lf + c) * U32 + 3 * U32 * Me / np.where(pos, Se, 1.0)
            m, w1 = max(m, float(rr[pos].max())), max(w1, float((rr / bar1)[pos].max()))
        worst.setdefault((wf, split), (r.family, m))
        _log("%-28s %-4s cfg %#10x family %3d NCO %d K splits %2d  max r %.3e  (L + c) 2^-24 = (%d + %d) 2^-24 = %.3e  worst r / bar 1 "
             "%.4f" % (name, wf, cfg, r.family, r.info[10], r.info[2], m, Lf, c, (Lf + c) * U32, w1))
        if wf == "f32":
            assert r.family not in S3_FAMILIES and w1 <= 1, (r.what, w1)
        else:
            assert r.family in S3_FAMILIES
            base = worst.get(("f32", split)) or worst[("f32", False)]
            assert m <= 4 * base[1] + 1e-7, "%s: split-bf16 %.3e against fp32 family %d %.3e" % (r.what, m, base[0], base[1])
    dev.unchanged(name)


def test_precision_sigmoid():
    """PMF_ACT_SIGMOID is 1 / (1 + __expf(-v)).  The ROCm device-library documentation with __expf's error bound is not part
    of the installed tree, so the bar is measured: E = the largest error a float32 CPU evaluation of the same expression
    (numpy float32 exp, add, divide) leaves against float64 on the test's own pre-activations, and the kernel is allowed
    4 E on top of the accumulation bound (the sigmoid's slope is at most 1 / 4).  Measured: E = 8.0e-8, the kernels (fp32 and
    split-bf16, both tiles) at 7.6e-8 from float64."""
    case = K.BY_NAME[K.SIGMOID]
    dev = shared(case.name, "random")
    v64 = dev.G + dev.inp["bias"].astype(F64)
    v32 = v64.astype(F32)
    cpu = (F32(1) / (F32(1) + np.exp(-v32))).astype(F64)
    E = float(np.abs(cpu - 1 / (1 + np.exp(-v32.astype(F64)))).max())
    ref = 1 / (1 + np.exp(-v64))
    Lf, c = chain_bound(case, 1)
    for wf in K.wforms(case):
        for cfg in (0, K.tile(32, 2)):
            r = launch(case, dev, wf, cfg, act=L.ACT_SIGMOID)
            err = np.abs(r.out[0][..., :case.Cout].astype(F64) - ref)
            lin = 0.25 * ((Lf + c) * U32 * dev.S + 3 * U32 * dev.M) * (4 if wf != "f32" else 1)
            _log("%-28s %-4s cfg %#9x family %3d sigmoid  max |got - ref64| %.3e  float32 CPU evaluation E %.3e  bar 4 E + chain "
                 "%.3e" % (case.name, wf, cfg, r.family, err.max(), E, 4 * E + lin.max()))
            assert (err <= 4 * E + lin).all(), r.what
            second = launch(case, dev, wf, cfg, act=L.ACT_SIGMOID)
            same_run(second, r, r.what + " sigmoid, second run")
    dev.unchanged(case.name)


# ------------------------------------------------------------------------------------------------ d. refusals
def test_refusals_launch_nothing():
    lib = L.lib()

    def refused(case, dev, wform, want, change):
        outs = [GBuf(e["out0"].size, e["out0"]) for e in dev.inp["dst"]]
        ptr = dict(x=[b.ptr for b in dev.x], scale=[_p(b) for b in dev.scale], shift=[_p(b) for b in dev.shift],
                   cmul=[_p(b) for b in dev.cmul], w=dev.pack(wform).ptr, bias=_p(dev.bias), pmask=_p(dev.pmask),
                   dst=[dict(out=o.ptr, stats=0, **{f: _p(e[f]) for f in ("cmul", "relu_x", "rs", "rt", "mean")})
                        for o, e in zip(outs, dev.dst)])
        d = K.fill_desc(case, ptr, wform)
        st = [GBuf(8 * 2 * dd.C * 2) for dd in case.dsts]          # (room for the rows of an accepted launch: none is owed)
        for j, dd in enumerate(case.dsts):
            if dd.stat:
                (d if len(case.dsts) == 1 else d.dst[j]).stats = st[j].ptr
        change(d)
        assert lib.pmf_conv_fwd(C.byref(d), stream()) == want, (case.name, want)
        torch.cuda.synchronize()
        for b in outs + st:
            b.unchanged(case.name + ": a refused descriptor wrote")

    E_ARG, E_UNS = L.PMF_E_ARG, L.PMF_E_UNSUPPORTED
    f, g = K.BY_NAME["f_1x1_16_20"], K.BY_NAME["d_3x3_32_from64"]
    m, w = K.BY_NAME["d_3x3_merged_32+64+32"], K.BY_NAME["f_3x3d18_16_20_gather"]
    df, dg, dm, dw = (shared(c.name, "exact") for c in (f, g, m, w))
    refused(f, df, "f32", E_ARG, lambda d: setattr(d.src[0], "x", None))                  # a null operand
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "Cout", 0))
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "out", None))
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "w", None))                         # neither w nor w_s3
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "ldw", d.ldw + 2))
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "in_stride", 3))

    def bad_layout(d):                     # 48 + 48 + 32 channels: the second range starts inside a 32-channel tile
        d.dst[0].C, d.dst[1].C = 48, 48
    assert lib.pmf_conv_multi_ok(C.byref(K.host_desc(m, "s3"))) == 1
    refused(m, dm, "s3", E_ARG, bad_layout)
    refused(g, dg, "f32", E_ARG, lambda d: setattr(d, "stats", None))                     # ep_stat_mean without stats
    refused(f, df, "f32", E_ARG, lambda d: setattr(d, "ep_flags", L.EP_STAT_X_ONLY))      # ... X_ONLY without ep_stat_mean

    def s3_on_gather(d):                   # split-bf16 weights on a descriptor pmf_conv_s3_eligible refuses (per-tap staging)
        assert lib.pmf_conv_s3_eligible(C.byref(d)) == 0
        d.w_s3, d.w = d.w, None
    refused(w, dw, "f32", E_UNS, s3_on_gather)
