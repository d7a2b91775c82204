"""-m gpu: every exported function of csrc/elementwise.hip, called directly through the C ABI, against the same operation in
float64 torch on the CPU.

Comparison rule
  * copy / select / mask kernels: ``torch.equal`` on float32.
  * arithmetic kernels: element by element, ``|got - ref64| <= K * eps32 * mag`` where ``mag`` is the same formula in
    float64 on the absolute values of the operands and K is TWICE the number of float32 roundings on the longest path
    to one output (table ``K`` below).  One wrong border pixel fails.
Guard rule: every output has ``ldc = C + 4`` (or more) and sits between two guard bands; everything the kernel does not
own is prefilled with a NaN-payload sentinel and must be bit-unchanged afterwards.  softmax_bwd, logits_bwd and
nchw_to_nhwc own the padding channels and must leave zeros there.  Inputs carry the same NaN in their padding, so a
kernel that reads padding poisons its output.
Accumulate rule: acc=0 onto the NaN prefill leaves no NaN; acc=1 onto a random prefill equals prefill + the acc=0 result
within one extra rounding."""
import ctypes as C_
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402

DEV = "cuda"
EPS = float(torch.finfo(torch.float32).eps)
TINY = float(torch.finfo(torch.float32).tiny)      # float32 underflow: exp(-160) is 0 in float32, 3e-70 in float64
SENT = 0x7FC0BEEF                                  # a quiet NaN with a payload
BAND = 64
VIEW_R = 3                                         # roundings of a view load: x*scale, +shift, *cmul

# what measure_gate_units() / measure_softmax_units(span) return on the CPU (float32 torch against float64, worst element in
# units of eps32 * mag); tests/test_elementwise_bounds_host.py keeps these figures and the helpers together
MEASURED = {
    "fusion_gate": 2.17,
    "fusion_gate_bwd": 2.88,
    "softmax": {80.0: 33.76, 100.0: 33.14},
    "softmax_bwd": {80.0: 1.55, 100.0: 1.32},
}

# K = 2 * (float32 roundings on the longest path to one output).  VIEW_R = 3 per view operand.
K = {
    # two views, their sum, the LeakyReLU product with 0.01f (itself rounded)
    "add_act": 2 * (2 * VIEW_R + 1 + 2),
    # acc=0 is a masked copy (exact); acc=1 adds once
    "acc": 2 * 1,
    # g * slope, slope = 0.01f is itself a rounded constant
    "act_bwd": 2 * 2,
    # 0.01f and the product, a thread's sequential sum over the pixels it visits, the sequential LDS fold over `rows`
    "act_bwd_rows": lambda visits, rows: 2 * (2 + visits + rows),
    # thread sum, LDS fold, `gx` workgroups arriving one after the other at the atomic, the *1.f
    "colsum": lambda visits, rows, gx: 2 * (visits + rows + gx + 1),
    # thread sum, LDS fold, stage 2: ceil(gx/256) sequential terms per thread + 8 tree levels, *1.f, += out
    "colsum_rows": lambda visits, rows, gx: 2 * (visits + rows + (gx + 255) // 256 + 8 + 2),
    # view, ceil(HW/R) sequential terms per row thread, fold over R rows, 1/HW (rounded) and the product with it
    "global_mean": lambda HW, R: 2 * (VIEW_R + (HW + R - 1) // R + R + 2),
    # 1/HW (rounded), * gout, * cmul, + prefill
    "global_mean_bwd": 2 * 4,
    # view, nine-term sum, /9
    "avgpool": 2 * (VIEW_R + 9 + 1),
    # four-term sum, /9, * cmul, + prefill
    "avgpool_bwd": 2 * (4 + 1 + 1 + 1),
    # view; lx, ly in {0, .25, .75} are exact, so per row pair two products and a sum (3), the row weight (1), the sum (1)
    "bilinear": 2 * (VIEW_R + 3 + 1 + 1),
    # an input pixel feeds at most 4 output rows x 4 output columns (2y-1 .. 2y+2); the weight products are exact
    # (multiples of 1/16); per term a product and a sum; + prefill
    "bilinear_bwd": 2 * (16 * 2 + 1),
    # view, * out_cmul
    "pixel_shuffle": 2 * (VIEW_R + 1),
    # * out_cmul, * in_cmul, + prefill
    "pixel_shuffle_bwd": 2 * 3,
    # MEASURED (expf and the division have no derivable count; measure_gate_units below): the float32 torch-CPU evaluation
    # of f*sigmoid(att)+pcd behind affine views against float64, in units of eps32*mag, mag = |f|*sigmoid(att)+|pcd|,
    # worst over the inputs of test_fusion_gate_fwd_bwd: 2.17; K = 4 x that, rounded up = 9
    "fusion_gate": math.ceil(4 * MEASURED["fusion_gate"]),
    # MEASURED the same way, worst over gf = g*s and gatt = g*f*s*(1-s), mag = |g|*s and |g|*|f|*s*(1+s): 2.88 -> 12
    "fusion_gate_bwd": math.ceil(4 * MEASURED["fusion_gate_bwd"]),
    # MEASURED (measure_softmax_units): float32 torch.softmax on the CPU against float64, C <= 32, in units of eps32*p
    # beyond the float32 subnormal floor TINY, per logit span: 33.76 -> 136 at +-80, 33.14 -> 133 at +-100 (x - max is
    # rounded, and exp turns that absolute error into a relative one; a p above TINY has |x - max| < 88 at either span, hence
    # figures that are alike)
    "softmax": {span: math.ceil(4 * u) for span, u in MEASURED["softmax"].items()},
    # MEASURED: float32 p*(g - sum(p*g)), what torch's softmax backward evaluates, against float64 on the same float32 p, in
    # units of eps32 * p*(|g| + sum(p*|g|)) beyond TINY: 1.55 -> 7 at +-80, 1.32 -> 6 at +-100
    "softmax_bwd": {span: math.ceil(4 * u) for span, u in MEASURED["softmax_bwd"].items()},
    # x * mask is exact (mask in {0, 1}); acc=1 adds once
    "pmask_mul_bwd": 2 * 1,
}

CHANNELS = [4, 20, 96]
SPATIAL = [(1, 1), (1, 7), (7, 1), (5, 9), (12, 20)]
NB = 3
WRAP = (1, 260, 256, 64)                           # 1,064,960 float4 items > the 4096 x 256 threads of ew_grid


def st():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def grid_rnd(g, *shape):
    """multiples of 2^-6 in [-8, 8): sums, products with {0.5, 1, 2, 1.25} and shifts on the same grid are exact in float32"""
    return torch.randint(-512, 512, shape, generator=g).float() / 64


class Buf:
    """rows x ldc floats between two guard bands; [:, :C] is what the kernel may write (or what it reads); the rest holds the
    sentinel.  offset: floats by which the body is moved off 16-byte alignment."""

    def __init__(self, rows, C, ldc=None, fill=None, offset=0):
        self.rows, self.C, self.ldc = rows, C, ldc or C
        self.n = rows * self.ldc
        self.band = (max(BAND, min(2 * self.ldc, 4096)) + 63) // 64 * 64
        self.lo = self.band + offset
        self.raw = torch.full((self.lo + self.n + self.band,), SENT, dtype=torch.int32, device=DEV)
        self.fill = None
        if fill is not None:
            self.fill = fill.reshape(rows, C).float().contiguous()
            self._body(self.raw)[:, :C] = self.fill.to(DEV)
        self.before = self.raw.cpu()
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        assert (self.raw.data_ptr() & 255) == 0

    def _body(self, raw):
        return raw[self.lo:self.lo + self.n].view(torch.float32).view(self.rows, self.ldc)

    def check(self, what, zero_pad=False, rows_written=None):
        """guard bands and padding bit-unchanged (zero_pad: padding channels all zero bits); returns [rows, C] float32"""
        now = self.raw.cpu()
        own = torch.zeros(now.shape, dtype=torch.bool)
        body = own[self.lo:self.lo + self.n].view(self.rows, self.ldc)
        body[:self.rows if rows_written is None else rows_written, :self.ldc if zero_pad else self.C] = True
        stray = (now != self.before) & ~own
        assert not stray.any(), "%s: %d stray writes outside the output, first at float %d of the body" % (
            what, int(stray.sum()), int(stray.nonzero()[0]) - self.lo)
        if zero_pad:
            pad = now[self.lo:self.lo + self.n].view(self.rows, self.ldc)[:, self.C:]
            assert not pad.any(), "%s: padding channels are not zero" % what
        return self._body(now)[:, :self.C].clone()


def close(got, ref, mag, k, what, floor=0.0):
    got, ref, mag = got.double().reshape(-1), ref.double().reshape(-1), mag.double().reshape(-1)
    err, bound = (got - ref).abs(), k * EPS * mag + floor
    bad = ~(err <= bound)                                     # (a NaN is bad)
    if bad.any():
        i = int(bad.nonzero()[0])
        units = (err / (EPS * mag).clamp_min(1e-300))[bad]
        raise AssertionError("%s: %d of %d elements outside %g*eps*mag, first at %d: got %r ref %r, worst %.3g units" % (
            what, int(bad.sum()), got.numel(), k, i, got[i].item(), ref[i].item(), units[~units.isnan()].max().item()
            if (~units.isnan()).any() else float("nan")))


def check_acc(call, rows, C, ldc, g, what):
    """the accumulate rule.  call(buf, acc) runs the kernel into buf.  Returns the acc=0 result [rows, C]."""
    b0 = Buf(rows, C, ldc)
    call(b0, 0)
    r0 = b0.check(what + " acc=0")
    assert not r0.isnan().any(), "%s acc=0 left NaN (read the prefill?)" % what
    pre = rnd(g, rows, C)
    b1 = Buf(rows, C, ldc, fill=pre)
    call(b1, 1)
    r1 = b1.check(what + " acc=1")
    close(r1, pre.double() + r0.double(), pre.abs() + r0.abs(), K["acc"], what + " acc=1 vs prefill + acc=0")
    return r0


class ViewMath:
    """the CPU side of a pmf_view_t over x [N, H, W, C] (float32): its parameters, its float64 value y and magnitude mag,
    and y32, the same arithmetic in float32 torch (what the measured K entries are measured on)"""
    KINDS = ("plain", "affine", "affine_relu", "cmul", "affine_relu_cmul")

    def __init__(self, kind, x, g, exact=False):
        N, C = x.shape[0], x.shape[-1]
        self.x, self.kind = x, kind
        self.y, self.y32 = x.double(), x
        self.mag = x.double().abs()
        bc = (1,) * (x.dim() - 1) + (C,)
        self.sc = self.sh = self.cm = None
        if "affine" in kind:
            if exact:
                sc = torch.tensor([0.5, -1.0, 2.0, 1.0, -0.5])[torch.randint(0, 5, (C,), generator=g)]
                sh = grid_rnd(g, C) / 8
            else:
                sc, sh = rnd(g, C) * 0.5 + 1.0, rnd(g, C) * 0.5
                sc[::3] *= -1
            self.sc, self.sh = sc, sh
            self.y = self.y * sc.double().view(bc) + sh.double().view(bc)
            self.y32 = self.y32 * sc.view(bc) + sh.view(bc)
            self.mag = self.mag * sc.double().abs().view(bc) + sh.double().abs().view(bc)
        self.pre_relu = self.y
        if "relu" in kind:
            self.y, self.y32 = self.y.clamp_min(0), self.y32.clamp_min(0)
        if "cmul" in kind:
            self.cm = (torch.rand(N, C, generator=g) > 0.3).float() * 1.25     # distinct rows per sample
            bn = (N,) + (1,) * (x.dim() - 2) + (C,)
            self.y, self.mag, self.y32 = self.y * self.cm.double().view(bn), self.mag * self.cm.double().view(bn), \
                self.y32 * self.cm.view(bn)


class ViewCase(ViewMath):
    """ViewMath with its buffers on the device and the pmf_view_t that describes them"""

    def __init__(self, kind, x, g, exact=False):
        super().__init__(kind, x, g, exact)
        N, C = x.shape[0], x.shape[-1]
        self.buf = Buf(x.numel() // C, C, C + 4, fill=x)
        v = self.v = L.View()
        v.x, v.ldc = self.buf.ptr, self.buf.ldc
        if self.sc is not None:
            self.sc_d, self.sh_d = self.sc.to(DEV), self.sh.to(DEV)
            v.scale, v.shift = self.sc_d.data_ptr(), self.sh_d.data_ptr()
        if "relu" in kind:
            v.flags = L.SRC_RELU
        if self.cm is not None:
            self.cmbuf = Buf(N, C, C + 8, fill=self.cm)
            v.cmul, v.cmul_ld = self.cmbuf.ptr, C + 8
        self.ref = C_.byref(v)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


# ================================================================================================ add + activation
def run_add_act(N, H, W, C, kind, act, has_b, seed=0):
    g = gen(seed)
    a = ViewCase(kind, rnd(g, N, H, W, C), g)
    b = ViewCase("affine" if kind == "plain" else "plain", rnd(g, N, H, W, C), g) if has_b else None
    out = Buf(N * H * W, C, C + 4)
    ok(L.lib().pmf_add_act(a.ref, b.ref if b else None, act, out.ptr, out.ldc, N * H * W, H * W, C, st()), "pmf_add_act")
    got = out.check("add_act")
    y, mag = (a.y + b.y, a.mag + b.mag) if b else (a.y, a.mag)
    if act == L.ACT_RELU:
        y = y.clamp_min(0)
    elif act == L.ACT_LRELU:
        y = torch.where(y > 0, y, 0.01 * y)
    close(got, y, mag, K["add_act"], "add_act %s act=%d" % (kind, act))


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_add_act(C, hw):
    for kind in ViewCase.KINDS:
        for act, has_b in ((L.ACT_NONE, True), (L.ACT_RELU, True), (L.ACT_LRELU, True), (L.ACT_RELU, False)):
            run_add_act(NB, hw[0], hw[1], C, kind, act, has_b)


def run_add_act_bwd(N, H, W, C, act, seed=1, acc_too=True):
    g = gen(seed)
    npix = N * H * W
    go, o = rnd(g, npix, C), rnd(g, npix, C)
    o[::3] = 0.0                                              # relu'(0) = 0
    gob, ob = Buf(npix, C, C + 4, fill=go), Buf(npix, C, C + 8, fill=o)
    ref = go * (o > 0) if act == L.ACT_RELU else go
    lib = L.lib()
    for which in ("a", "b", "ab"):
        def call(buf, acc, other=None):
            pa = buf.ptr if "a" in which else None
            pb = (other or buf).ptr if "b" in which else None
            ok(lib.pmf_add_act_bwd(gob.ptr, gob.ldc, ob.ptr, ob.ldc, act, pa, buf.ldc, acc, pb, (other or buf).ldc, acc, npix,
                                   C, st()), "pmf_add_act_bwd")
        if which == "ab":
            ba, bb = Buf(npix, C, C + 4), Buf(npix, C, C + 8)
            call(ba, 0, bb)
            assert torch.equal(ba.check("add_act_bwd ga"), ref) and torch.equal(bb.check("add_act_bwd gb"), ref)
            # the two accumulate flags are separate arguments
            pa, pb = rnd(g, npix, C), rnd(g, npix, C)
            ba, bb = Buf(npix, C, C + 4, fill=pa), Buf(npix, C, C + 8, fill=pb)
            ok(lib.pmf_add_act_bwd(gob.ptr, gob.ldc, ob.ptr, ob.ldc, act, ba.ptr, ba.ldc, 1, bb.ptr, bb.ldc, 0, npix, C, st()),
               "pmf_add_act_bwd")
            close(ba.check("ga"), pa.double() + ref.double(), pa.abs() + ref.abs(), K["acc"], "add_act_bwd ga acc=1")
            assert torch.equal(bb.check("gb"), ref)
        elif acc_too:
            r0 = check_acc(call, npix, C, C + 4, g, "add_act_bwd g%s act=%d" % (which, act))
            assert torch.equal(r0, ref)


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_add_act_bwd(C, hw):
    for act in (L.ACT_NONE, L.ACT_RELU):
        run_add_act_bwd(NB, hw[0], hw[1], C, act)


# ================================================================================================ column kernels
def col_shape(npix, C):
    cap = L.lib().pmf_debug_col(0, 0)                         # (0, 0) queries, changes nothing
    Q = C // 4
    rows = 256 // min(Q, 256)
    gx = max(1, min(cap, -(-npix // (rows * 4))))
    return rows, gx, -(-npix // (gx * rows)), cap


def col_npix(C):
    cap = L.lib().pmf_debug_col(0, 0)
    rows = 256 // min(C // 4, 256)
    return [1, rows * 4 - 1, 4 * rows * cap * 2 + 3]


COL_CASES = [(C, i) for C in CHANNELS + [1028] for i in range(3)]


@pytest.mark.parametrize("C,which", COL_CASES)
def test_act_bwd_rows(C, which):
    npix = col_npix(C)[which]
    rows, gx, visits, _ = col_shape(npix, C)
    lib = L.lib()
    nrows = lib.pmf_col_rows(npix, C)
    assert nrows == gx
    g = gen(10 + which)
    g0, a = rnd(g, npix, C), rnd(g, npix, C)
    a[::5] = 0.0                                              # the slope at 0 is the non-positive branch
    ab = Buf(npix, C, C + 8, fill=a)
    for act, slope in ((L.ACT_NONE, None), (L.ACT_LRELU, 0.01), (L.ACT_RELU, 0.0)):
        gb = Buf(npix, C, C + 4, fill=g0)
        rb = Buf(nrows + 2, C, C + 4)
        ok(lib.pmf_act_bwd(gb.ptr, gb.ldc, ab.ptr, ab.ldc, act, rb.ptr, rb.ldc, npix, C, st()), "pmf_act_bwd")
        got = gb.check("act_bwd g")
        if slope is None:
            ref = g0.double()
            assert torch.equal(got, g0)
        else:
            ref = g0.double() * torch.where(a > 0, 1.0, slope).double()
            close(got, ref, ref.abs(), K["act_bwd"], "act_bwd g act=%d" % act)
        r = rb.check("act_bwd rows", rows_written=nrows)      # rows beyond nrows keep the sentinel
        assert not r[:nrows].isnan().any(), "fewer than pmf_col_rows rows written"
        close(r[:nrows].double().sum(0), ref.sum(0), ref.abs().sum(0), K["act_bwd_rows"](visits, rows),
              "act_bwd rows act=%d npix=%d" % (act, npix))
        # no rows asked for: g alone
        gb2 = Buf(npix, C, C + 4, fill=g0)
        ok(lib.pmf_act_bwd(gb2.ptr, gb2.ldc, ab.ptr, ab.ldc, act, None, 0, npix, C, st()), "pmf_act_bwd")
        assert torch.equal(gb2.check("act_bwd g (no rows)"), got)


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("C,which", COL_CASES)
def test_colsum_and_colsum_rows(C, which, nz):
    npix = col_npix(C)[which]
    rows, gx, visits, _ = col_shape(npix, C)
    lib = L.lib()
    g = gen(20 + which)
    x = rnd(g, nz, npix, C)
    xb = Buf(nz * npix, C, C + 4, fill=x)
    pre = rnd(g, nz, C)
    ref, mag = x.double().sum(1) + pre.double(), x.double().abs().sum(1) + pre.double().abs()
    ob = Buf(nz, C, C, fill=pre)                              # out advances C per sample: no padding, bands only
    ok(lib.pmf_colsum(xb.ptr, xb.ldc, npix, C, ob.ptr, nz, st()), "pmf_colsum")
    close(ob.check("colsum"), ref, mag, K["colsum"](visits, rows, gx), "colsum npix=%d nz=%d" % (npix, nz))
    res = []
    for rep in range(2):
        ob = Buf(nz, C, C, fill=pre)
        sb = Buf(nz * gx, C, C)
        ok(lib.pmf_colsum_rows(xb.ptr, xb.ldc, npix, C, ob.ptr, nz, sb.ptr, st()), "pmf_colsum_rows")
        res.append(ob.check("colsum_rows"))
        assert not sb.check("colsum_rows scratch").isnan().any()
    close(res[0], ref, mag, K["colsum_rows"](visits, rows, gx), "colsum_rows npix=%d nz=%d" % (npix, nz))
    assert torch.equal(res[0], res[1]), "colsum_rows is not deterministic"
    assert lib.pmf_colsum_rows(xb.ptr, xb.ldc, npix, C, ob.ptr, nz, None, st()) == L.PMF_E_ARG


# ================================================================================================ global mean
def run_global_mean(N, H, W, C, kind, seed=30):
    g = gen(seed)
    v = ViewCase(kind, rnd(g, N, H, W, C), g)
    out = Buf(N, C, C)
    ok(L.lib().pmf_global_mean(v.ref, N, H * W, C, out.ptr, st()), "pmf_global_mean")
    R = 256 // min(C // 4, 256)
    close(out.check("global_mean"), v.y.mean((1, 2)), v.mag.mean((1, 2)), K["global_mean"](H * W, R),
          "global_mean %s" % kind)


def run_global_mean_bwd(N, H, W, C, cmul, seed=31):
    g = gen(seed)
    go = rnd(g, N, C)
    gob = Buf(N, C, C, fill=go)
    cm = (torch.rand(N, C, generator=g) > 0.3).float() * 1.25 if cmul else None
    cmb = Buf(N, C, C + 8, fill=cm) if cmul else None
    ref = (go.double() / (H * W))[:, None, :].expand(N, H * W, C)
    if cmul:
        ref = ref * cm.double()[:, None, :]

    def call(buf, acc):
        ok(L.lib().pmf_global_mean_bwd(gob.ptr, N, H * W, C, cmb.ptr if cmul else None, C + 8 if cmul else 0, buf.ptr, buf.ldc,
                                       acc, st()), "pmf_global_mean_bwd")
    r0 = check_acc(call, N * H * W, C, C + 4, g, "global_mean_bwd")
    close(r0, ref, ref.abs(), K["global_mean_bwd"], "global_mean_bwd cmul=%d" % cmul)


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS + [1028])
def test_global_mean_fwd_bwd(C, hw):
    for kind in ViewCase.KINDS:
        run_global_mean(NB, hw[0], hw[1], C, kind)
    for cmul in (False, True):
        run_global_mean_bwd(NB, hw[0], hw[1], C, cmul)


# ================================================================================================ avg pool
def run_avgpool(N, H, W, C, kind, seed=40):
    g = gen(seed)
    v = ViewCase(kind, rnd(g, N, H, W, C), g)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = Buf(N * OH * OW, C, C + 4)
    ok(L.lib().pmf_avgpool3s2(v.ref, N, H, W, C, out.ptr, out.ldc, st()), "pmf_avgpool3s2")
    ref, mag = (nhwc(F.avg_pool2d(nchw(t), 3, 2, 1)) for t in (v.y, v.mag))      # count_include_pad: always / 9
    assert ref.shape[1:3] == (OH, OW)
    close(out.check("avgpool"), ref, mag, K["avgpool"], "avgpool %s" % kind)


def run_avgpool_bwd(N, H, W, C, cmul, seed=41, acc_too=True):
    g = gen(seed)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    go = rnd(g, N, OH, OW, C)
    gob = Buf(N * OH * OW, C, C + 4, fill=go)
    cm = (torch.rand(N, C, generator=g) > 0.3).float() * 1.25 if cmul else None
    cmb = Buf(N, C, C + 8, fill=cm) if cmul else None

    def bwd(gg):
        x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
        xs = x * cm.double()[:, :, None, None] if cmul else x
        (F.avg_pool2d(xs, 3, 2, 1) * nchw(gg)).sum().backward()
        return nhwc(x.grad)
    ref, mag = bwd(go.double()), bwd(go.double().abs())

    def call(buf, acc):
        ok(L.lib().pmf_avgpool3s2_bwd(gob.ptr, gob.ldc, N, H, W, C, cmb.ptr if cmul else None, C + 8 if cmul else 0, buf.ptr,
                                      buf.ldc, acc, st()), "pmf_avgpool3s2_bwd")
    if acc_too:
        r0 = check_acc(call, N * H * W, C, C + 4, g, "avgpool_bwd")
    else:
        b = Buf(N * H * W, C, C + 4)
        call(b, 0)
        r0 = b.check("avgpool_bwd")
    close(r0, ref, mag, K["avgpool_bwd"], "avgpool_bwd cmul=%d" % cmul)


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_avgpool_fwd_bwd(C, hw):
    for kind in ViewCase.KINDS:
        run_avgpool(NB, hw[0], hw[1], C, kind)
    for cmul in (False, True):
        run_avgpool_bwd(NB, hw[0], hw[1], C, cmul)


# ================================================================================================ max pool
def window_ref(y):
    """y [N, H, W, C] float64 -> (max [N, OH, OW, C], first-argmax window position 0..8), padding = -inf, NaN wins"""
    N, H, W, C = y.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(nchw(y), (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(p, 3, stride=2).view(N, C, 9, OH, OW)
    isn = win.isnan()
    key = torch.where(isn, torch.full_like(win, float("inf")), win)
    m = key.max(2, keepdim=True).values
    eq = key == m
    first = eq & (eq.cumsum(2) == 1)
    idx = (first * torch.arange(9).view(1, 1, 9, 1, 1)).sum(2)
    val = (torch.where(first, win, torch.zeros_like(win)).nan_to_num(nan=0.0, posinf=0, neginf=0)).sum(2)
    val = torch.where(isn.any(2), torch.full_like(val, float("nan")), val)
    return nhwc(val), nhwc(idx).to(torch.uint8), first


def run_maxpool(N, H, W, C, kind, x=None, seed=50, acc_too=True, bwd=True):
    g = gen(seed)
    if x is None:
        x = grid_rnd(g, N, H, W, C)
    v = ViewCase(kind, x, g, exact=True)
    assert torch.equal(v.y.float().double(), v.y) or v.y.isnan().any()       # the view values are exact in float32
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = Buf(N * OH * OW, C, C + 4)
    idx = torch.full((N * OH * OW * C + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    lib = L.lib()
    ok(lib.pmf_maxpool3s2(v.ref, N, H, W, C, out.ptr, out.ldc, idx.data_ptr(), st()), "pmf_maxpool3s2")
    rv, ri, first = window_ref(v.y)
    got = out.check("maxpool").view(N, OH, OW, C)
    assert torch.equal(got.isnan(), rv.isnan())
    assert torch.equal(got.nan_to_num(nan=0.0), rv.float().nan_to_num(nan=0.0)), "maxpool values (%s)" % kind
    if not rv.isnan().any() and "cmul" not in kind:
        assert torch.equal(got, nhwc(F.max_pool2d(nchw(v.y), 3, 2, 1)).float())
    gi = idx.cpu()
    assert torch.equal(gi[:-64].view(N, OH, OW, C), ri), "maxpool argmax bytes (%s)" % kind
    assert (gi[-64:] == 0xEE).all()
    # without idx: the same values, nothing else written
    out2 = Buf(N * OH * OW, C, C + 4)
    ok(lib.pmf_maxpool3s2(v.ref, N, H, W, C, out2.ptr, out2.ldc, None, st()), "pmf_maxpool3s2")
    assert torch.equal(out2.check("maxpool (no idx)").nan_to_num(nan=0.0), got.reshape(-1, C).nan_to_num(nan=0.0))
    if "cmul" in kind or not bwd:
        return None                                           # the backward kernel takes the view for its relu' mask only
    # backward: route gout to the first maximum of every window; relu view: masked by relu'(BN output)
    go = grid_rnd(g, N, OH, OW, C)
    gob = Buf(N * OH * OW, C, C + 8, fill=go)
    route = first.double() * nchw(go.double()).unsqueeze(2)            # [N, C, 9, OH, OW]
    ref = nhwc(F.fold(route.view(N, C * 9, OH * OW), (H + 2, W + 2), 3, stride=2)[:, :, 1:H + 1, 1:W + 1])
    if "relu" in kind:
        ref = ref * (v.pre_relu > 0)

    def call(buf, acc):
        ok(lib.pmf_maxpool3s2_bwd(gob.ptr, gob.ldc, idx.data_ptr(), N, H, W, C, v.ref, buf.ptr, buf.ldc, acc, st()),
           "pmf_maxpool3s2_bwd")
    if acc_too:
        r0 = check_acc(call, N * H * W, C, C + 4, g, "maxpool_bwd %s" % kind)
    else:
        b = Buf(N * H * W, C, C + 4)
        call(b, 0)
        r0 = b.check("maxpool_bwd")
    assert torch.equal(r0.view(N, H, W, C), ref.float()), "maxpool gradient routing (%s)" % kind
    return ref, v, go


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_maxpool_fwd_bwd_exact(C, hw):
    for kind in ViewCase.KINDS:
        run_maxpool(NB, hw[0], hw[1], C, kind)


def test_maxpool_matches_autograd_with_relu_view():
    """the hand-built routing reference of run_maxpool against float64 autograd, once (same tie rule: first maximum)"""
    N, H, W, C = 2, 5, 9, 4
    ref, v, go = run_maxpool(N, H, W, C, "affine_relu", x=grid_rnd(gen(49), N, H, W, C))
    y = v.pre_relu.clone().requires_grad_(True)
    o = F.max_pool2d(F.relu(nchw(y)), 3, 2, 1)
    (o * nchw(go.double())).sum().backward()
    assert torch.equal(y.grad, ref)


def test_maxpool_padding_is_minus_infinity():
    g = gen(51)
    run_maxpool(NB, 5, 9, 8, "plain", x=-grid_rnd(g, NB, 5, 9, 8).abs() - 1.0)
    run_maxpool(NB, 1, 1, 4, "plain", x=-grid_rnd(g, NB, 1, 1, 4).abs() - 1.0)


def test_maxpool_ties_first_position_wins():
    g = gen(52)
    x = grid_rnd(g, 2, 6, 7, 8)
    x[:, 1:4, 1:4, :] = 9.0                                   # a 3 x 3 plateau above the data range: ties in several windows
    x[:, :, 5:, 4:] = x[:, :, 4:5, 4:]
    run_maxpool(2, 6, 7, 8, "plain", x=x)
    run_maxpool(2, 3, 3, 4, "plain", x=torch.zeros(2, 3, 3, 4))


def test_maxpool_nan_propagates_and_index_points_at_it():
    g = gen(53)
    x = grid_rnd(g, 1, 5, 7, 4)
    x[0, 2, 3, 1] = float("nan")
    N, H, W, C = x.shape
    v = ViewCase("plain", x, g)
    OH, OW = 3, 4
    out = Buf(N * OH * OW, C, C + 4)
    idx = torch.zeros(N * OH * OW * C, dtype=torch.uint8, device=DEV)
    ok(L.lib().pmf_maxpool3s2(v.ref, N, H, W, C, out.ptr, out.ldc, idx.data_ptr(), st()), "pmf_maxpool3s2")
    rv, ri, _ = window_ref(x.double())
    got = out.check("maxpool nan").view(N, OH, OW, C)
    assert torch.equal(got.isnan(), rv.isnan()) and int(got.isnan().sum()) == 2      # rows 2y-1..2y+1: windows oy=1, ox=1 and 2
    assert torch.equal(got.nan_to_num(nan=0.0), rv.float().nan_to_num(nan=0.0))
    gi = idx.cpu().view(N, OH, OW, C)
    assert torch.equal(gi, ri)
    assert gi[0, 1, 1, 1] == 1 * 3 + 2 and gi[0, 1, 2, 1] == 1 * 3 + 0


# ================================================================================================ bilinear x2
def run_bilinear(N, H, W, C, kind, seed=60):
    g = gen(seed)
    v = ViewCase(kind, rnd(g, N, H, W, C), g)
    out = Buf(N * 4 * H * W, C, C + 4)
    ok(L.lib().pmf_bilinear2x(v.ref, N, H, W, C, out.ptr, out.ldc, st()), "pmf_bilinear2x")
    ref, mag = (nhwc(F.interpolate(nchw(t), scale_factor=2, mode="bilinear", align_corners=False)) for t in (v.y, v.mag))
    close(out.check("bilinear"), ref, mag, K["bilinear"], "bilinear %s" % kind)


def run_bilinear_bwd(N, H, W, C, seed=61, acc_too=True):
    g = gen(seed)
    go = rnd(g, N, 2 * H, 2 * W, C)
    gob = Buf(N * 4 * H * W, C, C + 8, fill=go)

    def bwd(gg):
        x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
        (F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) * nchw(gg)).sum().backward()
        return nhwc(x.grad)
    ref, mag = bwd(go.double()), bwd(go.double().abs())

    def call(buf, acc):
        ok(L.lib().pmf_bilinear2x_bwd(gob.ptr, gob.ldc, N, H, W, C, buf.ptr, buf.ldc, acc, st()), "pmf_bilinear2x_bwd")
    if acc_too:
        r0 = check_acc(call, N * H * W, C, C + 4, g, "bilinear_bwd")
    else:
        b = Buf(N * H * W, C, C + 4)
        call(b, 0)
        r0 = b.check("bilinear_bwd")
    close(r0, ref, mag, K["bilinear_bwd"], "bilinear_bwd")


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_bilinear_fwd_bwd(C, hw):
    for kind in ViewCase.KINDS:
        run_bilinear(NB, hw[0], hw[1], C, kind)
    run_bilinear_bwd(NB, hw[0], hw[1], C)


# ================================================================================================ PixelShuffle(2)
def run_pixel_shuffle(N, H, W, Ci, kind, ocmul, seed=70):
    g = gen(seed)
    Co = Ci // 4
    v = ViewCase(kind, rnd(g, N, H, W, Ci), g)
    out = Buf(N * 4 * H * W, Co, Co + 4)
    ocm = (torch.rand(N, Co, generator=g) > 0.3).float() * 1.25 if ocmul else None
    ocb = Buf(N, Co, Co + 8, fill=ocm) if ocmul else None
    ok(L.lib().pmf_pixel_shuffle2(v.ref, N, H, W, Co, ocb.ptr if ocmul else None, Co + 8 if ocmul else 0, out.ptr, out.ldc,
                                  st()), "pmf_pixel_shuffle2")
    ref, mag = (nhwc(F.pixel_shuffle(nchw(t), 2)) for t in (v.y, v.mag))
    if ocmul:
        ref, mag = (t * ocm.double()[:, None, None, :] for t in (ref, mag))
    got = out.check("pixel_shuffle")
    if kind == "plain" and not ocmul:
        assert torch.equal(got.view(ref.shape), ref.float()), "pixel_shuffle (copy)"
    else:
        close(got, ref, mag, K["pixel_shuffle"], "pixel_shuffle %s ocmul=%d" % (kind, ocmul))


def run_pixel_shuffle_bwd(N, H, W, Ci, ocmul, icmul, seed=71, acc_too=True):
    g = gen(seed)
    Co = Ci // 4
    go = rnd(g, N, 2 * H, 2 * W, Co)
    gob = Buf(N * 4 * H * W, Co, Co + 4, fill=go)
    ocm = (torch.rand(N, Co, generator=g) > 0.3).float() * 1.25 if ocmul else None
    icm = (torch.rand(N, Ci, generator=g) > 0.3).float() * 1.25 if icmul else None
    ocb = Buf(N, Co, Co + 8, fill=ocm) if ocmul else None
    icb = Buf(N, Ci, Ci + 8, fill=icm) if icmul else None
    ref = nhwc(F.pixel_unshuffle(nchw(go.double() * (ocm.double()[:, None, None, :] if ocmul else 1.0)), 2))
    if icmul:
        ref = ref * icm.double()[:, None, None, :]

    def call(buf, acc):
        ok(L.lib().pmf_pixel_shuffle2_bwd(gob.ptr, gob.ldc, N, H, W, Co, ocb.ptr if ocmul else None, Co + 8 if ocmul else 0,
                                          icb.ptr if icmul else None, Ci + 8 if icmul else 0, buf.ptr, buf.ldc, acc, st()),
           "pmf_pixel_shuffle2_bwd")
    if acc_too:
        r0 = check_acc(call, N * H * W, Ci, Ci + 4, g, "pixel_shuffle_bwd")
    else:
        b = Buf(N * H * W, Ci, Ci + 4)
        call(b, 0)
        r0 = b.check("pixel_shuffle_bwd")
    if not ocmul and not icmul:
        assert torch.equal(r0.view(ref.shape), ref.float())
    else:
        close(r0, ref, ref.abs(), K["pixel_shuffle_bwd"], "pixel_shuffle_bwd")


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_pixel_shuffle_fwd_bwd(C, hw):
    for kind in ViewCase.KINDS:
        for ocmul in (False, True):
            run_pixel_shuffle(NB, hw[0], hw[1], C, kind, ocmul)
    for ocmul, icmul in ((False, False), (True, False), (False, True), (True, True)):
        run_pixel_shuffle_bwd(NB, hw[0], hw[1], C, ocmul, icmul)


# ================================================================================================ fusion gate
GATE_KINDS = ("plain", "affine", "affine_relu")


def gate_ref(f, a, p, go=None, mag=False):
    """forward f*s+p, or (gf, gatt) for an upstream gradient; mag: the formulas on absolute values, where 1 - s is 1 + s"""
    s = torch.sigmoid(a)
    if go is None:
        return f * s + p
    return go * s, go * f * s * ((1 + s) if mag else (1 - s))


def gate_case(npix, C, fk, ak, seed=80, view=ViewMath):
    """the inputs of one fusion-gate case: the generator (for further draws), the two views, pcd and the upstream gradient"""
    g = gen(seed)
    f = view(fk, rnd(g, 1, npix, C), g)
    a = view(ak, rnd(g, 1, npix, C) * 2, g)
    return g, f, a, rnd(g, npix, C), rnd(g, npix, C)


def run_gate(npix, C, fk, ak, acc_too=True):
    g, f, a, p, go = gate_case(npix, C, fk, ak, view=ViewCase)
    pb = Buf(npix, C, C + 8, fill=p)
    out = Buf(npix, C, C + 4)
    lib = L.lib()
    ok(lib.pmf_fusion_gate(f.ref, a.ref, pb.ptr, pb.ldc, out.ptr, out.ldc, npix, C, st()), "pmf_fusion_gate")
    fy, ay, fm = f.y.view(npix, C), a.y.view(npix, C), f.mag.view(npix, C)
    close(out.check("fusion_gate"), gate_ref(fy, ay, p.double()), gate_ref(fm, ay, p.double().abs()), K["fusion_gate"],
          "fusion_gate %s/%s" % (fk, ak))
    # backward
    gob = Buf(npix, C, C + 4, fill=go)
    rf, ra = gate_ref(fy, ay, None, go.double())
    mf, ma = gate_ref(fm, ay, None, go.double().abs(), mag=True)

    def run(gfb, accf, gab, gpb, accp):
        ok(lib.pmf_fusion_gate_bwd(gob.ptr, gob.ldc, f.ref, a.ref, gfb.ptr, gfb.ldc, accf, gab.ptr, gab.ldc,
                                   gpb.ptr if gpb else None, gpb.ldc if gpb else 0, accp, npix, C, st()), "pmf_fusion_gate_bwd")
    gfb, gab, gpb = Buf(npix, C, C + 4), Buf(npix, C, C + 8), Buf(npix, C, C + 4)
    run(gfb, 0, gab, gpb, 0)
    gf0, ga0, gp0 = gfb.check("gate_bwd gf"), gab.check("gate_bwd gatt"), gpb.check("gate_bwd gpcd")
    close(gf0, rf, mf, K["fusion_gate_bwd"], "gate_bwd gf %s/%s" % (fk, ak))
    close(ga0, ra, ma, K["fusion_gate_bwd"], "gate_bwd gatt %s/%s" % (fk, ak))
    assert torch.equal(gp0, go)
    if acc_too:
        # the two accumulate flags one at a time; gatt has none: it is overwritten; gpcd may be absent
        pf, pp = rnd(g, npix, C), rnd(g, npix, C)
        gfb, gab, gpb = Buf(npix, C, C + 4, fill=pf), Buf(npix, C, C + 8, fill=pp), Buf(npix, C, C + 4, fill=pp)
        run(gfb, 1, gab, gpb, 0)
        close(gfb.check("gf acc"), pf.double() + gf0.double(), pf.abs() + gf0.abs(), K["acc"], "gate_bwd gf acc=1")
        assert torch.equal(gab.check("gatt"), ga0) and torch.equal(gpb.check("gpcd"), go)
        gfb, gab, gpb = Buf(npix, C, C + 4, fill=pf), Buf(npix, C, C + 8), Buf(npix, C, C + 4, fill=pp)
        run(gfb, 0, gab, gpb, 1)
        assert torch.equal(gfb.check("gf"), gf0) and torch.equal(gab.check("gatt"), ga0)
        close(gpb.check("gpcd acc"), pp.double() + go.double(), pp.abs() + go.abs(), K["acc"], "gate_bwd gpcd acc=1")
        gfb, gab = Buf(npix, C, C + 4), Buf(npix, C, C + 8)
        run(gfb, 0, gab, None, 1)
        assert torch.equal(gfb.check("gf"), gf0) and torch.equal(gab.check("gatt"), ga0)


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_fusion_gate_fwd_bwd(C, hw):
    for fk in GATE_KINDS:
        for ak in GATE_KINDS:
            run_gate(NB * hw[0] * hw[1], C, fk, ak)


def measure_gate_units():
    """how MEASURED['fusion_gate'] / ['fusion_gate_bwd'] were measured: the float32 torch-CPU evaluation of the formulas of
    gate_ref against the float64 one, worst element in units of eps32 * mag, over the inputs of test_fusion_gate_fwd_bwd"""
    worst = [0.0, 0.0]
    for C in CHANNELS:
        for hw in SPATIAL:
            npix = NB * hw[0] * hw[1]
            for fk in GATE_KINDS:
                for ak in GATE_KINDS:
                    _, f, a, p, go = gate_case(npix, C, fk, ak)
                    f32, a32 = f.y32.view(npix, C), a.y32.view(npix, C)
                    fy, ay, fm = f.y.view(npix, C), a.y.view(npix, C), f.mag.view(npix, C)
                    u = (gate_ref(f32, a32, p).double() - gate_ref(fy, ay, p.double())).abs() / \
                        (EPS * gate_ref(fm, ay, p.double().abs()))
                    worst[0] = max(worst[0], u.max().item())
                    for r32, r64, mg in zip(gate_ref(f32, a32, None, go), gate_ref(fy, ay, None, go.double()),
                                            gate_ref(fm, ay, None, go.double().abs(), mag=True)):
                        worst[1] = max(worst[1], ((r32.double() - r64).abs() / (EPS * mg).clamp_min(1e-300)).max().item())
    return worst


def test_fusion_gate_argument_checks():
    g = gen(81)
    f, a = ViewCase("cmul", rnd(g, 1, 6, 8), g), ViewCase("plain", rnd(g, 1, 6, 8), g)
    pb, out = Buf(6, 8, 12, fill=rnd(g, 6, 8)), Buf(6, 8, 12)
    lib = L.lib()
    assert lib.pmf_fusion_gate(f.ref, a.ref, pb.ptr, 12, out.ptr, 12, 6, 8, st()) == L.PMF_E_ARG
    assert lib.pmf_fusion_gate(a.ref, f.ref, pb.ptr, 12, out.ptr, 12, 6, 8, st()) == L.PMF_E_ARG
    out.check("fusion_gate (refused)")


# ================================================================================================ channel softmax family
SM_C = [1, 3, 19, 20, 32]


def sm_layouts(C):
    return [((C + 7) // 8 * 8, 0), (C, 1)]                    # (ldc, offset in floats): the VEC and the scalar instantiation


def softmax_case(N, HW, C, span, seed=90):
    """logits [N, HW, C] in [-span, span] and the upstream gradient [N, C, HW]"""
    g = gen(seed)
    return rnd(g, N, HW, C) * span, rnd(g, N, C, HW)


def run_softmax_family(N, HW, C, ldc, off, span=80.0, k_span=None):
    lib = L.lib()
    x, go = softmax_case(N, HW, C, span)
    ksm, ksb = K["softmax"][k_span or span], K["softmax_bwd"][k_span or span]
    xb = Buf(N * HW, C, ldc, fill=x, offset=off)
    # forward
    pb = Buf(N * C, HW, HW)
    ok(lib.pmf_softmax_nhwc_to_nchw(xb.ptr, ldc, N, HW, C, pb.ptr, st()), "pmf_softmax_nhwc_to_nchw")
    p64 = torch.softmax(x.double(), 2).permute(0, 2, 1)
    close(pb.check("softmax"), p64, p64, ksm, "softmax C=%d ldc=%d span=%g" % (C, ldc, span), floor=TINY)
    lb = Buf(N * C, HW, HW)
    ok(lib.pmf_logits_nhwc_to_nchw(xb.ptr, ldc, N, HW, C, lb.ptr, st()), "pmf_logits_nhwc_to_nchw")
    assert torch.equal(lb.check("logits").view(N, C, HW), x.permute(0, 2, 1))
    # backward, on float32 probabilities as the forward pass hands them over
    p32 = torch.softmax(x, 2).permute(0, 2, 1).contiguous()
    p32b, gob = Buf(N * C, HW, HW, fill=p32), Buf(N * C, HW, HW, fill=go)
    db = Buf(N * HW, C, ldc, offset=off)
    ok(lib.pmf_softmax_bwd_nchw_to_nhwc(p32b.ptr, gob.ptr, N, HW, C, db.ptr, ldc, st()), "pmf_softmax_bwd_nchw_to_nhwc")
    pd, gd = p32.double(), go.double()
    ref = pd * (gd - (pd * gd).sum(1, keepdim=True))
    mag = pd * (gd.abs() + (pd * gd.abs()).sum(1, keepdim=True))
    close(db.check("softmax_bwd", zero_pad=True).view(N, HW, C), ref.permute(0, 2, 1), mag.permute(0, 2, 1), ksb,
          "softmax_bwd C=%d ldc=%d span=%g" % (C, ldc, span), floor=TINY)
    db = Buf(N * HW, C, ldc, offset=off)
    ok(lib.pmf_logits_bwd_nchw_to_nhwc(gob.ptr, N, HW, C, db.ptr, ldc, st()), "pmf_logits_bwd_nchw_to_nhwc")
    assert torch.equal(db.check("logits_bwd", zero_pad=True).view(N, HW, C), go.permute(0, 2, 1))


SM_HW = {80.0: (1, 7, 45, 300), 100.0: (7, 45)}


@pytest.mark.parametrize("C", SM_C)
def test_softmax_family(C):
    for ldc, off in sm_layouts(C):
        for HW in SM_HW[80.0]:
            run_softmax_family(NB, HW, C, ldc, off)


@pytest.mark.parametrize("C", SM_C)
def test_softmax_needs_the_max_subtraction(C):
    """logits in [-100, 100]: exp(100) is beyond FLT_MAX (exp(88.7)), so a softmax without the max subtraction gives inf / inf.
    ([-80, 80] does not show that: 32 terms of exp(80) = 5.5e34 stay finite in float32.)"""
    assert math.exp(100.0) > float(torch.finfo(torch.float32).max) > 32 * math.exp(80.0)
    for ldc, off in sm_layouts(C):
        for HW in SM_HW[100.0]:
            run_softmax_family(NB, HW, C, ldc, off, span=100.0)


def test_softmax_family_grid_stride_wrap():
    run_softmax_family(1, 1025 * 1024, 3, 8, 0, span=8.0, k_span=80.0)       # (the bound of the wider span holds a fortiori)


def measure_softmax_units(span):
    """how MEASURED['softmax'][span] / ['softmax_bwd'][span] were measured (the inputs of the softmax tests at that span)"""
    worst = [0.0, 0.0]
    for C in SM_C:
        for HW in SM_HW[span]:
            x, go = softmax_case(NB, HW, C, span)
            p64, p32 = torch.softmax(x.double(), 2), torch.softmax(x, 2)
            u = ((p32.double() - p64).abs() - TINY).clamp_min(0) / (EPS * p64)
            worst[0] = max(worst[0], u.max().item())
            p32 = p32.permute(0, 2, 1).contiguous()
            r32 = p32 * (go - (p32 * go).sum(1, keepdim=True))
            pd, gd = p32.double(), go.double()
            ref = pd * (gd - (pd * gd).sum(1, keepdim=True))
            mag = pd * (gd.abs() + (pd * gd.abs()).sum(1, keepdim=True))
            worst[1] = max(worst[1], (((r32.double() - ref).abs() - TINY).clamp_min(0) / (EPS * mag).clamp_min(1e-300)).max().item())
    return worst


def test_softmax_family_refuses_more_than_32_channels():
    b = Buf(4 * 33, 1, 1)
    lib = L.lib()
    U = L.PMF_E_UNSUPPORTED
    assert lib.pmf_softmax_nhwc_to_nchw(b.ptr, 40, 1, 4, 33, b.ptr, st()) == U
    assert lib.pmf_logits_nhwc_to_nchw(b.ptr, 40, 1, 4, 33, b.ptr, st()) == U
    assert lib.pmf_softmax_nhwc_to_nchw(b.ptr, 8, 1, 4, 0, b.ptr, st()) == U
    assert lib.pmf_softmax_bwd_nchw_to_nhwc(b.ptr, b.ptr, 1, 4, 33, b.ptr, 40, st()) == U
    assert lib.pmf_softmax_bwd_nchw_to_nhwc(b.ptr, b.ptr, 1, 4, 20, b.ptr, 40, st()) == U
    assert lib.pmf_logits_bwd_nchw_to_nhwc(b.ptr, 1, 4, 33, b.ptr, 40, st()) == U
    b.check("softmax (refused)", rows_written=0)


# ================================================================================================ broadcast / layout / fill / vec_add
def run_broadcast(N, HW, C, seed=100):
    g = gen(seed)
    src = rnd(g, N, C)
    sb = Buf(N, C, C + 8, fill=src)
    out = Buf(N * HW, C, C + 4)
    ok(L.lib().pmf_broadcast_rows(sb.ptr, sb.ldc, N, HW, C, out.ptr, out.ldc, st()), "pmf_broadcast_rows")
    assert torch.equal(out.check("broadcast_rows").view(N, HW, C), src[:, None, :].expand(N, HW, C))


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_broadcast_rows(C, hw):
    run_broadcast(NB, hw[0] * hw[1], C)
    lib = L.lib()
    b = Buf(4, 8, 8)
    for args in ((8, 1, 4, 6, 8), (6, 1, 4, 8, 8), (8, 1, 4, 8, 6), (8, 0, 4, 8, 8), (8, 1, 0, 8, 8)):
        sl, n, hwn, c, ol = args
        assert lib.pmf_broadcast_rows(b.ptr, sl, n, hwn, c, b.ptr, ol, st()) == L.PMF_E_ARG


def run_nchw_to_nhwc(N, C, HW, ldc, off, seed=110, slack=5):
    g = gen(seed)
    x = rnd(g, N, C + slack, HW + 3)                          # a strided source: sample / channel strides are not C*HW / HW
    xd = x.to(DEV)
    out = Buf(N * HW, C, ldc, offset=off)
    ok(L.lib().pmf_nchw_to_nhwc(xd.data_ptr(), xd.stride(0), xd.stride(1), N, C, HW, out.ptr, ldc, st()), "pmf_nchw_to_nhwc")
    assert torch.equal(out.check("nchw_to_nhwc", zero_pad=True).view(N, HW, C), x[:, :C, :HW].permute(0, 2, 1))


@pytest.mark.parametrize("C", [1, 3, 5, 8, 20])
def test_nchw_to_nhwc(C):
    for HW in (1, 7, 45, 240):
        for ldc, off in (((C + 7) // 8 * 8, 0), (C + 3, 0), (C + 4, 1)):
            run_nchw_to_nhwc(NB, C, HW, ldc, off)


def test_nchw_to_nhwc_grid_stride_wrap():
    run_nchw_to_nhwc(1, 3, 1025 * 1024, 8, 0, slack=0)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1027, 4096 * 256 * 4 + 7])
def test_fill(n):
    b = Buf(1, n, n) if n else Buf(1, 0, 1)
    ok(L.lib().pmf_fill(b.ptr, 1.5, n, st()), "pmf_fill")
    got = b.check("fill", rows_written=1 if n else 0)
    assert got.numel() == n and (got == 1.5).all()
    assert L.lib().pmf_fill(b.ptr + 4, 1.5, 1, st()) == L.PMF_E_ARG
    b.check("fill (refused)", rows_written=1 if n else 0)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_vec_add(n):
    g = gen(120)
    a, b = rnd(g, n), rnd(g, n)
    ab, bb = Buf(1, n, n, fill=a), Buf(1, n, n, fill=b)
    out = Buf(1, n, n)
    ok(L.lib().pmf_vec_add(ab.ptr, bb.ptr, out.ptr, n, st()), "pmf_vec_add")
    assert torch.equal(out.check("vec_add").view(-1), a + b)
    out = Buf(1, n, n)
    ok(L.lib().pmf_vec_add(ab.ptr, None, out.ptr, n, st()), "pmf_vec_add")
    assert torch.equal(out.check("vec_add (copy)").view(-1), a)


# ================================================================================================ EPMF pixel masks
def run_pmask_from_mul(N, H, W, C, kind, seed=130, acc_too=True):
    g = gen(seed)
    npix = N * H * W
    x = grid_rnd(g, N, H, W, C)
    x.view(npix, C)[torch.rand(npix, generator=g) < 0.4] = 0.0
    if C >= 4 and npix > 1:
        x.view(npix, C)[1] = 0.0
        x.view(npix, C)[1, 0], x.view(npix, C)[1, 3] = 2.0, -2.0      # sums to zero, |.| does not
    v = ViewCase(kind, x, g, exact=True)
    lib = L.lib()
    mb = Buf(1, npix, npix)
    ok(lib.pmf_pmask_from(v.ref, npix, H * W, C, mb.ptr, st()), "pmf_pmask_from")
    m = (v.y.abs().sum(-1) != 0).float().view(-1)
    assert torch.equal(mb.check("pmask_from").view(-1), m), "pmask_from %s" % kind
    # x * mask on an independent sparse mask
    m2 = (torch.rand(npix, generator=g) < 0.5).float()
    m2b = Buf(1, npix, npix, fill=m2)
    out = Buf(npix, C, C + 4)
    ok(lib.pmf_pmask_mul(v.ref, m2b.ptr, npix, H * W, C, out.ptr, out.ldc, st()), "pmf_pmask_mul")
    ref = (v.y.view(npix, C) * m2.double()[:, None]).float()
    assert torch.equal(out.check("pmask_mul"), ref), "pmask_mul %s" % kind
    if kind != "plain":
        return
    go = rnd(g, npix, C)
    gob = Buf(npix, C, C + 8, fill=go)

    def call(buf, acc):
        ok(lib.pmf_pmask_mul_bwd(gob.ptr, gob.ldc, m2b.ptr, npix, C, buf.ptr, buf.ldc, acc, st()), "pmf_pmask_mul_bwd")
    if acc_too:
        r0 = check_acc(call, npix, C, C + 4, g, "pmask_mul_bwd")
    else:
        b = Buf(npix, C, C + 4)
        call(b, 0)
        r0 = b.check("pmask_mul_bwd")
    assert torch.equal(r0, go * m2[:, None])
    # in place: gx == gy, acc = 0
    inp = Buf(npix, C, C + 4, fill=go)
    ok(lib.pmf_pmask_mul_bwd(inp.ptr, inp.ldc, m2b.ptr, npix, C, inp.ptr, inp.ldc, 0, st()), "pmf_pmask_mul_bwd")
    assert torch.equal(inp.check("pmask_mul_bwd in place"), go * m2[:, None])


@pytest.mark.parametrize("hw", SPATIAL)
@pytest.mark.parametrize("C", CHANNELS)
def test_pmask_from_mul_and_bwd(C, hw):
    for kind in ViewCase.KINDS:
        run_pmask_from_mul(NB, hw[0], hw[1], C, kind)


def run_pmask_pool(N, H, W, k, dil, pad, stride, seed=140, density=0.1):
    g = gen(seed)
    m = (torch.rand(N, H, W, generator=g) < density).float()
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    mb = Buf(1, N * H * W, N * H * W, fill=m)
    out = Buf(1, N * OH * OW, N * OH * OW)
    ok(L.lib().pmf_pmask_pool(mb.ptr, N, H, W, k, k, dil, pad, stride, out.ptr, OH, OW, st()), "pmf_pmask_pool")
    ref = F.max_pool2d(F.pad(m[:, None], (pad,) * 4), k, stride, 0, dil)[:, 0]
    assert ref.shape == (N, OH, OW)
    assert torch.equal(out.check("pmask_pool").view(N, OH, OW), ref), (k, dil, pad, stride)


# (kernel, dilation, padding, stride): the SparseVariantConv geometries of the EPMF model, and the 1 x 1 ones
PMASK_GEOM = [(3, 1, 1, 1), (3, 2, 2, 1), (3, 1, 1, 2), (3, 2, 2, 2), (1, 1, 0, 1), (1, 1, 0, 2)]


@pytest.mark.parametrize("geom", PMASK_GEOM)
def test_pmask_pool(geom):
    for H, W in ((7, 9), (1, 5), (5, 1), (13, 21)):
        run_pmask_pool(NB, H, W, *geom)


# ================================================================================================ grid-stride wrap
def test_grid_stride_wrap_add_gate_mask():
    N, H, W, C = WRAP
    run_add_act(N, H, W, C, "plain", L.ACT_RELU, True)
    run_add_act_bwd(N, H, W, C, L.ACT_RELU, acc_too=False)
    run_gate(N * H * W, C, "plain", "plain", acc_too=False)
    run_pmask_from_mul(N, H, W, C, "plain", acc_too=False)
    run_broadcast(N, H * W, C)
    run_global_mean_bwd(N, H, W, C, False)


def test_grid_stride_wrap_pools():
    N, H, W, C = WRAP
    run_avgpool(N, 2 * H, 2 * W - 1, C, "plain")               # 260 x 256 outputs
    run_avgpool_bwd(N, H, W, C, False, acc_too=False)
    run_maxpool(N, 2 * H - 1, 2 * W, C, "plain", bwd=False)    # forward: items are outputs, 260 x 256 of them
    run_maxpool(N, H, W, C, "plain", acc_too=False)            # backward: items are inputs


def test_grid_stride_wrap_resamplers():
    N, H, W, C = WRAP
    run_bilinear(N, H // 2, W // 2, C, "plain")                 # 260 x 256 outputs
    run_bilinear_bwd(N, H, W, C, acc_too=False)
    run_pixel_shuffle(N, H, W, C, "plain", False)               # one item per (input pixel, output channel)
    run_pixel_shuffle_bwd(N, H, W, C, False, False, acc_too=False)


def test_grid_stride_wrap_per_pixel_masks():
    """pmask_from and pmask_pool stride over pixels, not float4 items: 1025 x 1024 = 1,049,600 of them > 4096 x 256 threads"""
    run_pmask_pool(1, 1025, 1024, 3, 1, 1, 1)
    run_pmask_from_mul(1, 1025, 1024, 4, "plain", acc_too=False)


# ================================================================================================ argument checks
def test_channel_counts_that_are_no_multiple_of_four_are_refused():
    g = gen(150)
    lib = L.lib()
    C = 6
    v = ViewCase("plain", rnd(g, 1, 2, 2, 8), g)
    b = Buf(16, 8, 12)
    p, s = b.ptr, st()
    E = L.PMF_E_ARG
    assert lib.pmf_add_act(v.ref, None, 0, p, 12, 4, 4, C, s) == E
    assert lib.pmf_add_act_bwd(p, 12, p, 12, 0, p, 12, 0, None, 0, 0, 4, C, s) == E
    assert lib.pmf_add_act_bwd(p, 12, p, 12, L.ACT_LRELU, p, 12, 0, None, 0, 0, 4, 8, s) == E
    assert lib.pmf_act_bwd(p, 12, p, 12, 0, None, 0, 4, C, s) == E
    assert lib.pmf_colsum(p, 12, 4, C, p, 1, s) == E
    assert lib.pmf_colsum_rows(p, 12, 4, C, p, 1, p, s) == E
    assert lib.pmf_global_mean(v.ref, 1, 4, C, p, s) == E
    assert lib.pmf_global_mean_bwd(p, 1, 4, C, None, 0, p, 12, 0, s) == E
    assert lib.pmf_avgpool3s2(v.ref, 1, 2, 2, C, p, 12, s) == E
    assert lib.pmf_avgpool3s2_bwd(p, 12, 1, 2, 2, C, None, 0, p, 12, 0, s) == E
    assert lib.pmf_maxpool3s2(v.ref, 1, 2, 2, C, p, 12, None, s) == E
    assert lib.pmf_maxpool3s2_bwd(p, 12, p, 1, 2, 2, C, v.ref, p, 12, 0, s) == E
    assert lib.pmf_bilinear2x(v.ref, 1, 2, 2, C, p, 12, s) == E
    assert lib.pmf_bilinear2x_bwd(p, 12, 1, 2, 2, C, p, 12, 0, s) == E
    assert lib.pmf_fusion_gate(v.ref, v.ref, p, 12, p, 12, 4, C, s) == E
    assert lib.pmf_fusion_gate_bwd(p, 12, v.ref, v.ref, p, 12, 0, p, 12, None, 0, 0, 4, C, s) == E
    assert lib.pmf_broadcast_rows(p, 12, 1, 4, C, p, 12, s) == E
    assert lib.pmf_pmask_from(v.ref, 4, 4, C, p, s) == E
    assert lib.pmf_pmask_mul(v.ref, p, 4, 4, C, p, 12, s) == E
    assert lib.pmf_pmask_mul_bwd(p, 12, p, 4, C, p, 12, 0, s) == E
    b.check("refused calls", rows_written=0)
    assert math.isnan(b.check("refused calls")[0, 0].item())
