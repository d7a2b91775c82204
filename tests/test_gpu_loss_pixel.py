"""-m gpu: the per-pixel stage of csrc/loss.hip, called directly through the C ABI -- pmf_loss_pixel, pmf_loss_pixel_w,
pmf_loss_pixel_dice (loss_count_k, loss_pixel_k<false / true>, loss_dice_sums_k, loss_dice_fold_k) and pmf_loss_dice_finish --
against the float64 reference of tests/loss_pixel_cases.py, which tests/test_loss_pixel_reference_host.py holds to float64
autograd through the project's loss modules and whose bounds it shows to notice ten deliberately wrong variants.

The rules are those of tests/test_gpu_lovasz.py.  Every buffer sits between guard bands of a NaN-payload sentinel that must be
bit-unchanged afterwards; inputs must be bit-unchanged as a whole; the gradient maps, key, rows, parts and dice start from that
NaN, so an element that is not written shows; cnt starts from garbage (the stage zeroes it) and the confusion matrices from
non-zero counts (the stage adds).
  * gradients: pmf_loss_pixel_w with w6 a unit vector leaves ONE term's gradient in gl / gc; each is compared element by element
    with that term's reference under its derived bound; then a generic w6, the unweighted call and the call with the Dice term.
    w6[1] and w6[3] (the Lovasz weights) must not matter.  Pixels within the derived error of a gate are left out (at most 5 %);
    hand-made pixels exactly ON a gate (d = 0) are compared on the side float32 takes.
  * rows: per block of 256 pixels and column under its bound.  cnt, both confusion matrices and the keys: EXACT (the keys are
    bit-identical to float32 |fg - p|, -1 where the label is 0).  parts and dice: float64, n eps64 sum |terms|.
Pinned behaviour that is NOT the torch modules':
  * a batch without a labelled pixel: FocalSoftmaxLoss divides 0 by 0 (NaN); the stage gives focal value 0 and finite gradients
    (the perception terms alone);
  * a probability of exactly 0 under an open gate: autograd of xlogy gives -inf; the stage takes ln max(p, 1e-38).
Labels outside [0, C) (the modules would raise): outside the contract; pinned only that nothing outside the buffers is written,
that cnt and the confusion matrices ignore them and that they get no focal or Dice gradient.
Guards: pmf_loss_pixel(_w) refuse a null pointer and a conf_lidar / conf_camera pair of which one alone is null, as
pmf_loss_pixel_dice does, before anything is launched.
Each test prints worst err / bound per quantity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from tests import loss_pixel_cases as V  # noqa: E402
from tests.bn_cases import DBuf  # noqa: E402
from tests.lovasz_cases import WBuf  # noqa: E402
from tests.test_gpu_elementwise import Buf, st  # noqa: E402

F64 = np.float64


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Run:
    """the buffers of one call on the device; collect() checks every band and input and returns the outputs"""

    def __init__(self, x):
        lib = L.lib()
        self.x = x
        N, C, HW, P = x["N"], x["C"], x["HW"], x["P"]
        assert lib.pmf_loss_rows(P) == x["nrows"] and lib.pmf_loss_dice_parts(P) == x["nrows"]
        t = torch.from_numpy
        self.p, self.q = Buf(N * C, HW, HW, fill=t(x["p"])), Buf(N * C, HW, HW, fill=t(x["q"]))
        self.label, self.alpha = WBuf(t(x["label"])), Buf(1, C, C, fill=t(x["alpha"]))
        self.cnt = WBuf(torch.full((C,), 77, dtype=torch.int64))
        self.gl, self.gc = Buf(N * C, HW, HW), Buf(N * C, HW, HW)
        self.key, self.rows = Buf(2 * C, P, P), DBuf(x["nrows"], 4)
        self.conf_pre = (np.arange(2 * C * C, dtype=np.int64).reshape(2, C, C) * 3 + 1)
        self.cl, self.cc = WBuf(t(self.conf_pre[0])), WBuf(t(self.conf_pre[1]))
        self.parts, self.dice = DBuf(x["nrows"], 4 * C), DBuf(2, 2 + 2 * C)
        self.w6 = Buf(1, 6, 6, fill=torch.zeros(6))
        self.kind = None

    def head(self):
        x = self.x
        return (self.p.ptr, self.q.ptr, self.label.ptr, self.alpha.ptr, x["N"], x["C"], x["HW"], x["fg"], x["tau"])

    def tail(self):
        return (self.cnt.ptr, self.gl.ptr, self.gc.ptr, self.key.ptr, self.rows.ptr, self.cl.ptr, self.cc.ptr)

    def call(self, kind, w6=None):
        lib, x = L.lib(), self.x
        self.kind = kind
        if kind == "w":
            self.w6 = Buf(1, 6, 6, fill=torch.tensor(w6, dtype=torch.float32))
            rc = lib.pmf_loss_pixel_w(*self.head(), self.w6.ptr, *self.tail(), st())
        elif kind == "dice":
            rc = lib.pmf_loss_pixel_dice(*self.head(), x["gper"], *self.tail(), self.parts.ptr, self.dice.ptr, st())
        else:
            rc = lib.pmf_loss_pixel(*self.head(), x["gper"], *self.tail(), st())
        assert rc == 0, "pmf_loss_pixel (%s) returned %d" % (kind, rc)
        return self.collect()

    def unchanged(self, what):
        """nothing at all was written: a refused call"""
        for b in (self.p, self.q, self.alpha, self.w6, self.gl, self.gc, self.key, self.rows, self.parts, self.dice):
            b.check(what, rows_written=0)
        for b in (self.label, self.cnt, self.cl, self.cc):
            b.check(what)

    def collect(self):
        torch.cuda.synchronize()
        x = self.x
        for b in (self.p, self.q, self.alpha, self.w6):
            b.check("input", rows_written=0)
        self.label.check("label (input)")
        dice = self.kind == "dice"
        out = {"gl": V.to_pix(self.gl.check("gl").numpy(), x), "gc": V.to_pix(self.gc.check("gc").numpy(), x),
               "key": self.key.check("key").numpy(), "rows": self.rows.check("rows").numpy(),
               "cnt": self.cnt.check("cnt", written=True).numpy(),
               "conf": np.stack([self.cl.check("conf_lidar", written=True).numpy(),
                                 self.cc.check("conf_camera", written=True).numpy()]) - self.conf_pre,
               "parts": self.parts.check("parts", rows_written=None if dice else 0).numpy(),
               "dice": self.dice.check("dice", rows_written=None if dice else 0).numpy()}
        return out


def check_exact(x, got, ref, what, keys=True):
    assert np.array_equal(got["cnt"], ref["cnt"]), "%s: cnt %s, reference %s" % (what, got["cnt"], ref["cnt"])
    assert np.array_equal(got["conf"], ref["conf"]), "%s: a confusion matrix differs" % what
    if keys:
        bad = np.argwhere(bits(got["key"]) != bits(ref["key"]))
        assert bad.size == 0, "%s: %d keys are not bit-equal to float32 |fg - p|, first at %s" % (what, bad.shape[0], bad[0])


def check_rows(x, got, ref, what):
    r = V.worst_ratio(got["rows"], ref["rows"], ref["rows_bound"])
    assert r <= 1.0, "%s: a row sum is %.3g x its bound off" % (what, r)
    return r


def check_grad(x, got, ref, spec, what):
    gl, gc, bl, bc = V.grad_ref(x, ref, spec)
    worst = 0.0
    for name, g, want, b in (("gl", got["gl"], gl, bl), ("gc", got["gc"], gc, bc)):
        assert not np.isnan(g).any(), "%s %s: %d elements are NaN (not written?)" % (what, name, int(np.isnan(g).sum()))
        r = V.worst_ratio(g, want, b, ref["cmp"])
        if not r <= 1.0:
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.where(ref["cmp"][:, None], np.abs(g.astype(F64) - want) / b, 0.0)
            e[np.abs(g.astype(F64) - want) == 0] = 0
            i, c = np.unravel_index(np.nanargmax(e), e.shape)
            raise AssertionError("%s %s: worst element %.3g x its bound off at pixel %d class %d (edge %s): got %r reference %r" % (
                what, name, r, i, c, bool(x["edge"][i]), float(g[i, c]), float(want[i, c])))
        worst = max(worst, r)
    return worst


def check_dice_outputs(x, got, ref, what):
    d = ref["dice"]
    rp = V.worst_ratio(got["parts"], d["parts"], d["parts_bound"])
    rd = V.worst_ratio(got["dice"], d["dice"], d["dice_bound"])
    assert rp <= 1.0 and rd <= 1.0, "%s: parts %.3g x, dice %.3g x their bounds off; dice got %s reference %s" % (
        what, rp, rd, got["dice"], d["dice"])
    for h in range(2):
        if d["below"][h]:                                     # mean dice below 1e-6: the K = 0 branch, exactly
            assert got["dice"][h, 1] == 0.0
    return rp, rd


# ================================================================================================ the stage, term by term
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_pixel_stage(name):
    x, ref = V.inputs(name), V.case_ref(name)
    assert ref["left_out"].mean() <= 0.05
    worst = {}
    for spec, w6 in V.WSPECS.items():
        what = "%s %s" % (name, spec)
        got = Run(x).call("plain" if w6 is None else "w", w6)
        check_exact(x, got, ref, what)
        worst["rows"] = max(worst.get("rows", 0.0), check_rows(x, got, ref, what))
        q = V.QUANTITY[spec]
        worst[q] = max(worst.get(q, 0.0), check_grad(x, got, ref, spec, what))
        if spec == "w6":
            other = Run(x).call("w", V.W6_OTHER_LOV)
            for k in ("gl", "gc", "rows", "key"):
                assert got[k].tobytes() == other[k].tobytes(), "%s: %s depends on w6[1] / w6[3]" % (what, k)
    lov = Run(x).call("w", V.W_LOV_ONLY)
    assert not lov["gl"].any() and not lov["gc"].any(), name + ": a gradient under the Lovasz weights alone"
    got = Run(x).call("dice")
    check_exact(x, got, ref, name + " dice")
    worst["rows"] = max(worst["rows"], check_rows(x, got, ref, name + " dice"))
    worst["grad_dice"] = check_grad(x, got, ref, "dice", name + " dice")
    worst["parts"], worst["dice"] = check_dice_outputs(x, got, ref, name + " dice")
    if name == "dicezero":
        assert all(ref["dice"]["below"])
    if name == "allunlab":          # pinned: focal value 0 (the torch modules give NaN), finite gradients
        assert not got["rows"][:, :2].any() and np.isfinite(got["gl"]).all() and np.isfinite(got["gc"]).all()
        assert got["dice"][0, 0] == got["dice"][1, 0]
    print("%s: worst err / bound: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ================================================================================================ Dice pre-pass and fold
@pytest.mark.parametrize("name", V.DICE_NAMES)
def test_dice_parts_fold_and_gradient(name):
    """nparts around the fold's 16 groups and its 128-tile trips; the <true> gradient = the <false> gradient + the Dice term"""
    x, ref = V.inputs(name), V.case_ref(name)
    assert x["nrows"] in V.DICE_NPARTS
    got, plain = Run(x).call("dice"), Run(x).call("plain")
    check_exact(x, got, ref, name)
    rr = check_rows(x, got, ref, name)
    rp, rd = check_dice_outputs(x, got, ref, name)
    rg = check_grad(x, got, ref, "dice", name)
    check_grad(x, plain, ref, "plain", name + " <false>")
    # the leaves the two instantiations share come out bit-equal (rows: float64 sums of w_img Lp, w_pcd Lq and the focal values;
    # the keys); the gradients need not: compiled for gfx950, both hold 331 float32 fused multiply-adds and <true> 159 plain
    # multiplies against 164, although the Dice term gives <true> alone two more products and a sum per head and class
    # (four classes per unrolled trip): the shared expression is contracted differently.  Bound: loss_pixel_cases.
    # instantiation_bound, 12 u of the shared part's magnitudes + 7 u of the Dice term's + u of the result.  (The issue's
    # "existing per-element reasoning", 2^-22 |sum| + 2^-21 |term|, takes |sum| where the roundings are those of the pieces.)
    assert got["rows"].tobytes() == plain["rows"].tobytes() and got["key"].tobytes() == plain["key"].tobytes()
    tl, tc, _, _ = V.grad_ref(x, ref, "dice_term")
    bl, bc = V.instantiation_bound(x, ref)
    worst = 0.0
    for k, term, b in (("gl", tl, bl), ("gc", tc, bc)):
        want = plain[k].astype(F64) + term
        worst = max(worst, V.worst_ratio(got[k], want, b + V.U * np.abs(want), ref["cmp"]))
    assert worst <= 1.0, "%s: <true> - <false> is %.3g x its bound off the Dice term" % (name, worst)
    print("%s: worst err / bound: parts %.3f, dice %.3f, rows %.3f, gradient %.3f, <true> - <false> %.3f" % (name, rp, rd, rr, rg, worst))


def test_dice_finish_on_a_prefilled_out10():
    lib = L.lib()
    C = 14
    d = V.case_ref("dice17_c14")["dice"]["dice"]
    pre = np.arange(10, dtype=np.float32) * 0.375 + 1
    dice, out = DBuf(2, 2 + 2 * C, fill=torch.from_numpy(d)), Buf(1, 10, 10, fill=torch.from_numpy(pre))
    assert lib.pmf_loss_dice_finish(dice.ptr, C, out.ptr, st()) == 0
    torch.cuda.synchronize()
    dice.check("dice (input)", rows_written=0)
    o = out.check("out10").numpy().reshape(10)
    want = pre.copy()
    want[8], want[9] = np.float32(d[0, 0]), np.float32(d[1, 0])
    want[0] = np.float32(float(pre[0]) + d[0, 0] + d[1, 0])
    assert np.array_equal(bits(o), bits(want)), (o, want)


# ================================================================================================ the histogram's grid-stride loop
def test_count_beyond_the_grid():
    """C = 2, P = 2048 * 1024 + 2049: loss_count_k's 1024 workgroups wrap.  cnt, the confusion matrices and the keys only"""
    x = V.inputs("count")
    got = Run(x).call("plain")
    ref = {"cnt": V.histogram(x["label"], x["C"]), "conf": V.confusion_of(x), "key": V.keys_of(x)}
    assert int(ref["cnt"].sum()) == x["P"] > 2048 * 1024 + 2048
    check_exact(x, got, ref, "count")
    assert not np.isnan(got["rows"]).any()


# ================================================================================================ outside the contract
def test_out_of_range_labels_are_ignored():
    x = dict(V.inputs("c5"))
    lab = x["label"].copy()
    lab[::7], lab[3::11], lab[5::13] = -1, x["C"], 255
    x["label"] = lab
    ref = V.reference(x)
    ref["conf"] = V.confusion_of(x)
    odd = (lab < 0) | (lab >= x["C"])
    assert odd.sum() > 100 and int(ref["cnt"].sum()) == x["P"] - int(odd.sum())
    assert not ref["K"]["valid"][odd].any()                   # the reference has no focal and no Dice gradient at these pixels
    for kind in ("plain", "dice"):
        got = Run(x).call(kind)                               # (collect() checks every guard band)
        check_exact(x, got, ref, "out-of-range " + kind, keys=False)
        check_grad(x, got, ref, kind, "out-of-range " + kind)
    check_dice_outputs(x, got, ref, "out-of-range")


# ================================================================================================ argument checks
def test_pixel_entry_points_refuse_bad_arguments():
    """a null pointer, one confusion matrix without the other, C < 2, C > 32, N < 1, HW < 1: PMF_E_ARG, and N * HW beyond
    2^31 blocks of 256 pixels: PMF_E_UNSUPPORTED, before anything is launched -- every buffer, prefilled, is bit-unchanged --
    and the same buffers are then accepted"""
    lib = L.lib()
    x, ref = V.inputs("c2"), V.case_ref("c2")
    r = Run(x)
    r.w6 = Buf(1, 6, 6, fill=torch.tensor(V.W6))
    A = L.PMF_E_ARG

    def call(weighted, head=None, tail=None, w6=r.w6.ptr):
        head, tail = head or r.head(), tail or r.tail()
        if weighted:
            return lib.pmf_loss_pixel_w(*head, w6, *tail, st())
        return lib.pmf_loss_pixel(*head, x["gper"], *tail, st())

    for weighted in (False, True):
        for i in range(4):                                    # lidar_prob, camera_prob, label, alpha
            h = list(r.head())
            h[i] = None
            assert call(weighted, head=h) == A, ("head", i, weighted)
        for i in range(5):                                    # cnt, grad_lidar, grad_camera, key, rows
            t = list(r.tail())
            t[i] = None
            assert call(weighted, tail=t) == A, ("tail", i, weighted)
        for i in (5, 6):                                      # conf_lidar without conf_camera and the reverse
            t = list(r.tail())
            t[i] = None
            assert call(weighted, tail=t) == A, ("conf", i, weighted)
        for N, C, HW in ((0, 2, 77), (1, 1, 77), (1, 33, 77), (1, 2, 0), (-1, 2, 77), (1, 2, -3)):
            h = list(r.head())
            h[4:7] = N, C, HW
            assert call(weighted, head=h) == A, (N, C, HW, weighted)
        h = list(r.head())
        h[6] = 1 << 40                                        # more blocks of 256 pixels than a grid dimension holds
        assert call(weighted, head=h) == L.PMF_E_UNSUPPORTED
    assert call(True, w6=None) == A
    torch.cuda.synchronize()
    r.unchanged("refused calls")
    t = list(r.tail())
    t[5] = t[6] = None                                        # both null: no confusion matrices
    assert call(False, tail=t) == 0
    torch.cuda.synchronize()
    r.cl.check("conf_lidar (not given)")
    r.cc.check("conf_camera (not given)")
    assert call(True) == 0
    r.kind = "w"
    got = r.collect()
    check_exact(x, got, ref, "accepted after the refusals")
    check_grad(x, got, ref, "w6", "accepted after the refusals")
