"""-m gpu: every exported function of csrc/bn.hip, called directly through the C ABI, against the float64 references of
tests/bn_cases.py (which tests/test_bn_reference_host.py holds to torch's batch_norm).

The rules are those of tests/test_gpu_elementwise.py.  Comparison: element by element, ``|got - ref64| <= K * eps32 * mag``
with K twice the float32 roundings on the longest path (bn_cases.K); sums that a kernel keeps in float64 and casts once count
from the cast, plus ``n * eps64 * sum|terms|`` for the float64 sum.  Guards: every operand and output has its own pitch
(gy C+4, a C+8, dz C+12, dbias C+4) and sits between guard bands; padding and bands hold a NaN-payload sentinel and must be
bit-unchanged afterwards, inputs included; partial rows beyond pmf_col_rows keep the sentinel.  Accumulate: dgamma and dbeta
are +=, run onto zeros and onto a random prefill.  Determinism: two runs are ``torch.equal`` in every output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from tests import bn_cases as B  # noqa: E402
from tests.bn_cases import DBuf, K  # noqa: E402
from tests.test_gpu_elementwise import EPS, SENT, Buf, close, col_npix, col_shape, gen, ok, rnd, st  # noqa: E402

MOM = 0.1


def vec(t):
    """a per-channel vector (or [k, C] block of them) between guard bands"""
    t = t.reshape(-1, t.shape[-1])
    return Buf(t.shape[0], t.shape[1], t.shape[1], fill=t)


class Case:
    """the inputs of one backward case on the device; `unchanged` asserts that no kernel wrote into any of them"""

    def __init__(self, npix, C, act, x=None):
        x = x or B.bn_inputs(npix, C, act, B.case_seed(npix, C, act))
        self.npix, self.C, self.act, self.x = npix, C, act, x
        self.gy, self.a = Buf(npix, C, C + 4, fill=x["gy"]), Buf(npix, C, C + 8, fill=x["a"])
        self.mean, self.invstd, self.gamma = vec(x["mean"]), vec(x["invstd"]), vec(x["gamma"])
        self.pre = rnd(x["g"], 2, C)                          # the dgamma / dbeta prefill of the accumulate run
        self.refs = {}

    def ref(self, train):
        if train not in self.refs:
            x = self.x
            self.refs[train] = B.bn_bwd_ref(x["a"], x["gy"], x["gamma"], x["mean"], x["invstd"], self.act, train)
        return self.refs[train]

    def unchanged(self):
        for name in ("gy", "a", "mean", "invstd", "gamma"):
            getattr(self, name).check("input " + name, rows_written=0)


def same(a, b, what):
    assert torch.equal(a, b), "%s differs between two runs / two forms" % what


def check_sums(cs, train, out, pre, what, coef=True):
    """coef / dgamma / dbeta of one run against the reference; pre [2, C]: what dgamma, dbeta held before"""
    ref, n = cs.ref(train), cs.npix
    pg, pb = pre[0].double(), pre[1].double()
    for name, p in (("dgamma", pg), ("dbeta", pb)):
        mag = ref["mag_" + name] + p.abs()
        close(out[name], ref[name] + p, mag, K[name], "%s %s" % (what, name), floor=B.f64_floor(n, mag))
    if coef:
        for i in range(3):
            close(out["coef"][i], ref["coef"][i], ref["mag_coef"][i], K["coef%d" % i], "%s coef[%d]" % (what, i),
                  floor=B.f64_floor(n, ref["mag_coef"][i]))
        if not train:
            assert (out["coef"][1:] == 0).all(), "%s: eval-mode coef rows 1 and 2 are not 0.0" % what


def run_reduce(cs, train, pre):
    lib, C, npix = L.lib(), cs.C, cs.npix
    nrows = lib.pmf_col_rows(npix, C)
    part, coef, dg, db = DBuf(nrows + 2, 2 * C), Buf(3, C, C), vec(pre[0]), vec(pre[1])
    ok(lib.pmf_bn_bwd_reduce(cs.gy.ptr, cs.gy.ldc, cs.a.ptr, cs.a.ldc, npix, C, cs.mean.ptr, cs.gamma.ptr, cs.invstd.ptr,
                             train, part.ptr, coef.ptr, dg.ptr, db.ptr, st()), "pmf_bn_bwd_reduce")
    rows = part.check("bn_bwd_reduce part", rows_written=nrows)[:nrows]      # rows beyond nrows keep the sentinel
    assert not rows.isnan().any(), "fewer than pmf_col_rows partial rows written"
    return {"part": rows, "coef": coef.check("coef"), "dgamma": dg.check("dgamma")[0], "dbeta": db.check("dbeta")[0]}


def run_apply(cs, coef, act, with_rows=True):
    lib, C, npix = L.lib(), cs.C, cs.npix
    nrows = lib.pmf_col_rows(npix, C)
    cb, dz = vec(coef), Buf(npix, C, C + 12)
    rb = Buf(nrows + 2, C, C + 4) if with_rows else None
    ok(lib.pmf_bn_bwd_apply(cs.gy.ptr, cs.gy.ldc, cs.a.ptr, cs.a.ldc, npix, C, cb.ptr, cs.mean.ptr, act, dz.ptr, dz.ldc,
                            rb.ptr if rb else None, C + 4, st()), "pmf_bn_bwd_apply")
    cb.check("apply coef (input)", rows_written=0)
    out = {"dz": dz.check("bn_bwd_apply dz")}
    if rb:
        r = rb.check("bn_bwd_apply dbias rows", rows_written=nrows)[:nrows]
        assert not r.isnan().any(), "fewer than pmf_col_rows dbias rows written"
        out["rows"] = r
    return out


def check_three_launch(cs, train, what="", twice=True):
    """reduce -> fold -> apply on one case: every output against float64, accumulate, determinism, guards"""
    C, npix, act = cs.C, cs.npix, cs.act
    what = "reduce/apply %sC=%d npix=%d act=%d train=%d" % (what, C, npix, act, train)
    rows_, gx, visits, _ = col_shape(npix, C)
    assert L.lib().pmf_col_rows(npix, C) == gx
    ref, zero = cs.ref(train), torch.zeros(2, C)
    r0 = run_reduce(cs, train, zero)
    check_sums(cs, train, r0, zero, what)
    r1 = run_reduce(cs, train, cs.pre)                        # the accumulate run is the second run of part and coef
    same(r0["part"], r1["part"], what + " part")
    same(r0["coef"], r1["coef"], what + " coef")
    for i, name in enumerate(("dgamma", "dbeta")):
        close(r1[name], cs.pre[i].double() + r0[name].double(), cs.pre[i].abs() + r0[name].abs(), K["acc"],
              "%s %s prefill + run onto zeros" % (what, name))
    if twice:
        r2 = run_reduce(cs, train, zero)
        for name in ("part", "coef", "dgamma", "dbeta"):
            same(r0[name], r2[name], "%s %s" % (what, name))
    a0 = run_apply(cs, r0["coef"], act)
    close(a0["dz"], ref["dz"], ref["mag_dz"], K["dz"], what + " dz")
    close(a0["rows"].double().sum(0), ref["dbias"], ref["mag_dbias"], K["dbias_rows"](visits, rows_), what + " dbias rows")
    if twice:
        a1 = run_apply(cs, r0["coef"], act)
        same(a0["dz"], a1["dz"], what + " dz")
        same(a0["rows"], a1["rows"], what + " dbias rows")
    same(a0["dz"], run_apply(cs, r0["coef"], act, with_rows=False)["dz"], what + " dz without dbias_rows")
    cs.unchanged()
    return r0


def by_act(cases):
    out = {}
    for npix, act, train in cases:
        out.setdefault((npix, act), []).append(train)
    return sorted(out.items())


# ================================================================================================ a. three launches
@pytest.mark.parametrize("C,which", [(C, i) for C in B.BWD_C for i in range(3)])
def test_bwd_reduce_apply(C, which):
    assert col_npix(C) == B.col_npix_host(C) and col_shape(1, C)[3] == B.COL_CAP
    n = col_npix(C)[which]
    for (npix, act), trains in by_act(c for c in B.reduce_cases(C) if c[0] == n):
        cs = Case(npix, C, act)
        for train in trains:
            check_three_launch(cs, train)


@pytest.mark.parametrize("C", [20, 1028])
def test_bwd_reduce_apply_eight_pixel_trip(C):
    lib = L.lib()
    npix = col_npix(C)[1]
    cap = lib.pmf_debug_col(0, 0)
    try:
        assert lib.pmf_debug_col(0, 8) == cap                 # the cap stays as queried
        for act in B.ACTS:
            cs = Case(npix, C, act)
            for train in (1, 0):
                check_three_launch(cs, train, what="U=8 ")
    finally:
        assert lib.pmf_debug_col(0, 4) == cap


# ================================================================================================ b. one launch
def ppt_of(npix):
    return 1 if npix <= 512 else (2 if npix <= 1024 else 4)


def run_small(cs, train, pre, with_row=True):
    lib, C, npix = L.lib(), cs.C, cs.npix
    dz, dg, db = Buf(npix, C, C + 12), vec(pre[0]), vec(pre[1])
    rb = Buf(2, C, C + 4) if with_row else None
    assert lib.pmf_bn_bwd_small_ok(npix, C) == 1
    ok(lib.pmf_bn_bwd_small(cs.gy.ptr, cs.gy.ldc, cs.a.ptr, cs.a.ldc, npix, C, cs.mean.ptr, cs.gamma.ptr, cs.invstd.ptr, train,
                            cs.act, dz.ptr, dz.ldc, rb.ptr if rb else None, dg.ptr, db.ptr, st()), "pmf_bn_bwd_small")
    out = {"dz": dz.check("bn_bwd_small dz"), "dgamma": dg.check("dgamma")[0], "dbeta": db.check("dbeta")[0]}
    if rb:
        out["row"] = rb.check("bn_bwd_small dbias row", rows_written=1)[0]   # ONE row of C floats and nothing after it
    return out


def check_small(cs, train):
    C, npix, act = cs.C, cs.npix, cs.act
    what = "small C=%d npix=%d act=%d train=%d" % (C, npix, act, train)
    ref, zero = cs.ref(train), torch.zeros(2, C)
    s0 = run_small(cs, train, zero)
    check_sums(cs, train, s0, zero, what, coef=False)
    close(s0["dz"], ref["dz"], ref["mag_dz"], K["dz"], what + " dz")
    assert not s0["row"].isnan().any(), what + ": dbias row not fully written"
    close(s0["row"], ref["dbias"], ref["mag_dbias"], K["dbias_small"](ppt_of(npix)), what + " dbias row")
    s1 = run_small(cs, train, cs.pre)
    same(s0["dz"], s1["dz"], what + " dz")
    same(s0["row"], s1["row"], what + " dbias row")
    for i, name in enumerate(("dgamma", "dbeta")):
        close(s1[name], cs.pre[i].double() + s0[name].double(), cs.pre[i].abs() + s0[name].abs(), K["acc"],
              "%s %s prefill + run onto zeros" % (what, name))
    s2 = run_small(cs, train, zero, with_row=False)
    for name in ("dz", "dgamma", "dbeta"):
        same(s0[name], s2[name], "%s %s (without dbias_row)" % (what, name))
    cs.unchanged()


@pytest.mark.parametrize("npix", B.SMALL_NPIX)
@pytest.mark.parametrize("C", B.BWD_C)
def test_bwd_small(C, npix):
    for (n, act), trains in by_act(c for c in B.small_cases(C) if c[0] == npix):
        cs = Case(n, C, act)
        for train in trains:
            check_small(cs, train)
            check_three_launch(cs, train, what="(small map) ", twice=False)     # the same inputs through the other form


def test_bwd_small_refuses_what_it_cannot_do():
    lib = L.lib()
    b, v = Buf(16, 8, 12), Buf(1, 8, 8)
    E = L.PMF_E_ARG
    for npix, C in ((0, 8), (2049, 8), (4, 6)):
        assert lib.pmf_bn_bwd_small_ok(npix, C) == 0
        assert lib.pmf_bn_bwd_small(b.ptr, 12, b.ptr, 12, npix, C, v.ptr, v.ptr, v.ptr, 1, 0, b.ptr, 12, v.ptr, v.ptr, v.ptr,
                                    st()) == E
    b.check("bn_bwd_small (refused)", rows_written=0)
    v.check("bn_bwd_small (refused)", rows_written=0)


# ================================================================================================ c. each pixel, each row once
def one_hot_case(npix, C, p, seed=7):
    x = B.bn_inputs(npix, C, L.ACT_LRELU, seed)
    hot = rnd(x["g"], C)
    x["gy"] = torch.zeros(npix, C)
    x["gy"][p] = hot
    return Case(npix, C, L.ACT_LRELU, x), hot


def second_trip(C, npix):
    rows_, gx, _, _ = col_shape(npix, C)
    return 4 * gx * rows_, 8 * gx * rows_ - 1


def test_reduce_counts_each_pixel_once():
    C = 20
    npix = col_npix(C)[2]
    first, last = second_trip(C, npix)
    assert 0 < first < last < npix - 1
    for p in (0, npix - 1, first, last):
        cs, hot = one_hot_case(npix, C, p)
        same(run_reduce(cs, 1, torch.zeros(2, C))["dbeta"], hot, "dbeta of a one-hot gy at pixel %d" % p)


def test_small_counts_each_pixel_once():
    C, npix = 20, 2048
    for p in (0, 511, 512, 1023, 1024, 2047):
        cs, hot = one_hot_case(npix, C, p)
        same(run_small(cs, 1, torch.zeros(2, C))["dbeta"], hot, "dbeta of a one-hot gy at pixel %d" % p)


ONE_ROW = (0, 255, 256, 1023, 1024)                          # (the last is nrows - 1)


def run_fold(rows, npix, train, gamma, invstd, pre):
    lib = L.lib()
    nrows, _, C = rows.shape
    part, coef, dg, db = DBuf(nrows, 2 * C, fill=rows), Buf(3, C, C), vec(pre[0]), vec(pre[1])
    gb, ib = vec(gamma), vec(invstd)
    ok(lib.pmf_bn_bwd_fold(part.ptr, nrows, C, npix, train, gb.ptr, ib.ptr, coef.ptr, dg.ptr, db.ptr, st()), "pmf_bn_bwd_fold")
    for b in (part, gb, ib):
        b.check("bn_bwd_fold input", rows_written=0)
    return {"coef": coef.check("coef"), "dgamma": dg.check("dgamma")[0], "dbeta": db.check("dbeta")[0]}


def run_finalize(rows, count, x, running=True, save=True, momentum=MOM, eps=B.BN_EPS):
    lib = L.lib()
    nrows, _, C = rows.shape
    sb, gb, bb = DBuf(nrows, 2 * C, fill=rows), vec(x["gamma"]), vec(x["beta"])
    rm, rv = (vec(x["rm"]), vec(x["rv"])) if running else (None, None)
    sm, si = (Buf(1, C, C), Buf(1, C, C)) if save else (None, None)
    sc, sh = Buf(1, C, C), Buf(1, C, C)
    ptr = lambda b: b.ptr if b else None                      # noqa: E731
    ok(lib.pmf_bn_finalize(sb.ptr, nrows, count, gb.ptr, bb.ptr, ptr(rm), ptr(rv), momentum, eps, sc.ptr, sh.ptr, ptr(sm),
                           ptr(si), C, st()), "pmf_bn_finalize")
    for b in (sb, gb, bb):
        b.check("bn_finalize input", rows_written=0)
    out = {"scale": sc.check("scale")[0], "shift": sh.check("shift")[0], "bufs": (sm, si)}
    if running:
        out.update({"rm": rm.check("running_mean")[0], "rv": rv.check("running_var")[0]})
    if save:
        out.update({"mean": sm.check("save_mean")[0], "invstd": si.check("save_invstd")[0]})
    return out


def test_fold_and_finalize_count_each_row_once():
    nrows, C, count = 1025, 5, 4.0
    assert ONE_ROW[-1] == nrows - 1
    g = gen(11)
    x = B.finalize_inputs(1, C, 12)
    for r in ONE_ROW:
        v = rnd(g, C)
        rows = torch.zeros(nrows, 2, C, dtype=torch.float64)
        rows[r, 0] = v.double()
        rows[r, 1] = v.double() ** 2 / count + count            # variance 1
        f = run_fold(rows, 4, 1, x["gamma"], x["rv"], torch.zeros(2, C))
        same(f["dbeta"], v, "fold: dbeta of the single non-zero row %d" % r)
        z = run_finalize(rows, count, x)
        same(z["mean"], v / 4, "finalize: save_mean of the single non-zero row %d" % r)
        close(z["invstd"], torch.full((C,), 1 / (1 + B.BN_EPS) ** 0.5), torch.ones(C), K["save_invstd"], "finalize invstd, row %d" % r)


# ================================================================================================ d. the fold alone
@pytest.mark.parametrize("C", [4, 5, 20])
@pytest.mark.parametrize("nrows", [1, 255, 256, 257, 1024, 1025, 2500])
def test_bwd_fold(nrows, C):
    g = gen(200 + nrows + C)
    rows = (torch.rand(nrows, 2, C, generator=g, dtype=torch.float64) * 2 - 1) * 64
    gamma, r = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 3 + 0.2
    gamma[::3] *= -1
    npix = 3 * nrows + 1
    pre = rnd(g, 2, C)
    sg, sgc = rows[:, 0].sum(0), rows[:, 1].sum(0)
    ag, agc = rows[:, 0].abs().sum(0), rows[:, 1].abs().sum(0)
    rd, gd = r.double(), gamma.double()
    for train in (1, 0):
        what = "fold nrows=%d C=%d train=%d" % (nrows, C, train)
        f0 = run_fold(rows, npix, train, gamma, r, torch.zeros(2, C))
        f1 = run_fold(rows, npix, train, gamma, r, pre)
        same(f0["coef"], run_fold(rows, npix, train, gamma, r, torch.zeros(2, C))["coef"], what + " coef")
        same(f0["coef"], f1["coef"], what + " coef")
        for name, ref, mag, i in (("dgamma", rd * sgc, rd * agc, 0), ("dbeta", sg, ag, 1)):
            close(f0[name], ref, mag, K[name], "%s %s" % (what, name), floor=B.f64_floor(nrows, mag))
            close(f1[name], pre[i].double() + f0[name].double(), pre[i].abs() + f0[name].abs(), K["acc"],
                  "%s %s prefill + run onto zeros" % (what, name))
        refs = ((gd * rd, (gd * rd).abs()), (rd * rd * sgc / npix, rd * rd * agc / npix), (sg / npix, ag / npix))
        for i, (ref, mag) in enumerate(refs):
            if train or i == 0:
                close(f0["coef"][i], ref, mag, K["coef%d" % i], "%s coef[%d]" % (what, i), floor=B.f64_floor(nrows, mag))
            else:
                assert (f0["coef"][i] == 0).all()


@pytest.mark.parametrize("C,which", [(4, 0), (4, 1), (20, 0), (20, 1), (20, 2), (1028, 2)])
def test_bwd_fold_equals_the_fold_inside_reduce(C, which):
    npix = col_npix(C)[which]
    cs = Case(npix, C, L.ACT_LRELU)
    for train in (1, 0):
        r = run_reduce(cs, train, cs.pre)
        f = run_fold(r["part"].view(-1, 2, C), npix, train, cs.x["gamma"], cs.x["invstd"], cs.pre)
        for name in ("coef", "dgamma", "dbeta"):
            same(r[name], f[name], "C=%d npix=%d train=%d %s" % (C, npix, train, name))


# ================================================================================================ e. finalize, eval affine
def check_finalize(out, ref, what, running=True, save=True):
    names = [("scale", "scale", "scale"), ("shift", "shift", "shift")]
    if save:
        names += [("mean", "mean", "save_mean"), ("invstd", "invstd", "save_invstd")]
    if running:
        names += [("rm", "rm", "running"), ("rv", "rv", "running")]
    for o, r, k in names:
        close(out[o], ref[r], ref["mag_" + r], K[k], "%s %s" % (what, o), floor=ref["floor_" + r])


@pytest.mark.parametrize("C", [1, 5, 96])
@pytest.mark.parametrize("nrows", [1, 255, 256, 257, 1024, 1025, 2500])
def test_finalize(nrows, C):
    npix = 3 * nrows + 1
    x = B.finalize_inputs(npix, C, 300 + nrows + C)
    rows = B.stat_rows(x["x"], nrows)
    ref = B.finalize_ref(rows, npix, x["gamma"], x["beta"], x["rm"], x["rv"], MOM, B.BN_EPS)
    what = "finalize nrows=%d C=%d" % (nrows, C)
    full = run_finalize(rows, float(npix), x)
    check_finalize(full, ref, what)
    again = run_finalize(rows, float(npix), x)
    no_run = run_finalize(rows, float(npix), x, running=False)
    no_save = run_finalize(rows, float(npix), x, save=False)
    for name in ("scale", "shift", "mean", "invstd", "rm", "rv"):
        same(full[name], again[name], "%s %s" % (what, name))
        if name not in ("rm", "rv"):
            same(full[name], no_run[name], "%s %s (no running pair)" % (what, name))
        if name not in ("mean", "invstd"):
            same(full[name], no_save[name], "%s %s (no save pair)" % (what, name))


def test_finalize_count_one():
    C = 5
    x = B.finalize_inputs(1, C, 21)
    rows = B.stat_rows(x["x"], 1)
    ref = B.finalize_ref(rows, 1, x["gamma"], x["beta"], x["rm"], x["rv"], MOM, B.BN_EPS)
    out = run_finalize(rows, 1.0, x)
    check_finalize(out, ref, "finalize count=1")
    assert all(out[k].isfinite().all() for k in ("scale", "shift", "mean", "invstd", "rm", "rv"))
    m = torch.tensor(MOM)                                     # the variance of one value is 0: (1 - m) * rv + m * 0
    close(out["rv"], (1 - m.double()) * x["rv"].double(), x["rv"].double(), K["running"], "finalize count=1 running_var")


def test_finalize_variance_a_hair_below_zero():
    C, count = 5, 1024
    x = B.finalize_inputs(1, C, 22)
    rows = torch.zeros(1, 2, C, dtype=torch.float64)
    rows[0, 0], rows[0, 1] = 3.0 * count, 9.0 * count * (1 - 1e-15)
    assert ((rows[0, 1] / count - 9.0) < 0).all()
    out = run_finalize(rows, float(count), x)
    eps32 = torch.tensor(B.BN_EPS, dtype=torch.float32).double()
    same(out["invstd"], (1 / eps32.sqrt()).float().expand(C), "invstd of a clamped variance")
    same(out["mean"], torch.full((C,), 3.0), "save_mean")
    assert out["rv"].isfinite().all() and out["scale"].isfinite().all()


@pytest.mark.parametrize("C", [1, 255, 256, 257, 1028])
def test_eval_affine(C):
    lib = L.lib()
    x = B.finalize_inputs(1, C, 400 + C)
    eps = float(torch.tensor(B.BN_EPS, dtype=torch.float32))
    inv = 1 / (x["rv"].double() + eps).sqrt()
    scale = x["gamma"].double() * inv
    res = []
    for save in (True, False):
        ins = [vec(x[k]) for k in ("gamma", "beta", "rm", "rv")]
        sc, sh = Buf(1, C, C), Buf(1, C, C)
        sm, si = (Buf(1, C, C), Buf(1, C, C)) if save else (None, None)
        ok(lib.pmf_bn_eval_affine(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, B.BN_EPS, sc.ptr, sh.ptr, sm.ptr if sm else None,
                                  si.ptr if si else None, C, st()), "pmf_bn_eval_affine")
        for b in ins:
            b.check("bn_eval_affine input", rows_written=0)
        res.append((sc.check("scale")[0], sh.check("shift")[0]))
        close(res[-1][0], scale, scale.abs(), K["eval_scale"], "eval_affine scale C=%d" % C)
        close(res[-1][1], x["beta"].double() - x["rm"].double() * scale, x["beta"].double().abs() + (x["rm"].double() * scale).abs(),
              K["eval_shift"], "eval_affine shift C=%d" % C)
        if save:
            same(sm.check("save_mean")[0], x["rm"], "save_mean is a copy of running_mean")
            close(si.check("save_invstd")[0], inv, inv, K["eval_invstd"], "eval_affine save_invstd C=%d" % C)
    same(res[0][0], res[1][0], "scale with / without the save pair")
    same(res[0][1], res[1][1], "shift with / without the save pair")


# ================================================================================================ f. chain
@pytest.mark.parametrize("npix,C", B.CHAIN)
def test_chain_finalize_then_backward(npix, C):
    """rows from a -> pmf_bn_finalize -> its save_mean / save_invstd feed the backward, against float64 autograd through
    batch_norm on a.  K["chain"] is 4 x what torch's float32 CPU batch_norm loses on these inputs (host test)."""
    lib = L.lib()
    x, ref, mag = B.chain_case(npix, C)
    g = gen(31)
    fin = {"gamma": x["gamma"], "beta": rnd(g, C), "rm": rnd(g, C), "rv": torch.rand(C, generator=g) + 0.1}
    out = run_finalize(B.stat_rows(x["a"], 257), float(npix), fin)
    x = dict(x, mean=out["mean"], invstd=out["invstd"])       # (the values; the kernels below read finalize's own buffers)
    cs = Case(npix, C, L.ACT_LRELU, x)
    cs.mean, cs.invstd = out["bufs"]
    cs.mean.before, cs.invstd.before = cs.mean.raw.cpu(), cs.invstd.raw.cpu()
    zero = torch.zeros(2, C)
    if lib.pmf_bn_bwd_small_ok(npix, C):
        assert npix == 513
        dz = run_small(cs, 1, zero)["dz"]
    else:
        assert npix == 4099
        dz = run_apply(cs, run_reduce(cs, 1, zero)["coef"], L.ACT_LRELU)["dz"]
    close(dz, ref, mag, K["chain"], "chain npix=%d C=%d" % (npix, C))
    cs.unchanged()


# ================================================================================================ argument checks
def test_refused_calls_write_nothing():
    lib = L.lib()
    b, v, d = Buf(16, 8, 12), Buf(3, 8, 8), DBuf(4, 16)
    p, q, s, E = b.ptr, v.ptr, st(), L.PMF_E_ARG
    for nrows, count, C in ((0, 4.0, 8), (4, 4.0, 0), (4, 0.0, 8), (4, 0.5, 8), (-1, 4.0, 8)):
        assert lib.pmf_bn_finalize(d.ptr, nrows, count, q, q, q, q, MOM, B.BN_EPS, q, q, q, q, C, s) == E
    assert lib.pmf_bn_eval_affine(q, q, q, q, B.BN_EPS, q, q, q, q, 0, s) == E
    for nrows, C, npix in ((0, 8, 4), (4, 0, 4), (4, 8, 0)):
        assert lib.pmf_bn_bwd_fold(d.ptr, nrows, C, npix, 1, q, q, q, q, q, s) == E
    for npix, C in ((0, 8), (4, 0), (4, 6), (-1, 8)):
        assert lib.pmf_bn_bwd_reduce(p, 12, p, 12, npix, C, q, q, q, 1, d.ptr, q, q, q, s) == E
        assert lib.pmf_bn_bwd_apply(p, 12, p, 12, npix, C, q, q, 0, p, 12, p, 12, s) == E
    for buf in (b, v, d):
        buf.check("refused calls", rows_written=0)
    assert b.raw[b.lo].item() == SENT and EPS > 0
