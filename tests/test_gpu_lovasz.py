"""-m gpu: the Lovasz stage of csrc/loss.hip, called directly through the C ABI -- pmf_loss_lovasz_sort(_w) (the in-library
radix sort, the Jaccard kernels, the fold), pmf_loss_lovasz(_w) (the same kernels behind a caller's int64 permutation) and
pmf_lovasz_grad -- against the float64 reference of tests/lovasz_cases.py, which tests/test_lovasz_reference_host.py holds
to Lovasz-softmax and whose bounds it shows to have room.

The rules are those of tests/test_gpu_elementwise.py and tests/test_gpu_bn.py.  Every buffer the caller owns (key, label,
cnt, rows, w6, bsum, dots, gl, gc, out8, the permutation and the sort's workspace) sits between guard bands of a NaN-payload
sentinel that must be bit-unchanged afterwards; inputs must be bit-unchanged as a whole.  gl and gc start from a random
prefill, because the stage adds.  Sort: the permutation and the sorted errors are read back from the workspace and must be
BIT-EQUAL to the reference's stable descending order over the first P - cnt[0] ranks of every row of a present class (equal
errors in ascending pixel order: the gradient depends on it, the value does not).  Outputs: lovasz_cases' derived bounds;
what the stage may not touch -- unlabelled pixels, class 0, absent classes, pixels of error 0 -- is bit-equal to the prefill.
Each test prints worst err / bound per quantity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from tests import lovasz_cases as V  # noqa: E402
from tests.bn_cases import DBuf  # noqa: E402
from tests.lovasz_cases import WBuf  # noqa: E402
from tests.test_gpu_elementwise import Buf, ok, st  # noqa: E402

PASSES = 4


def sorted_from_workspace(words, C, P):
    """THE place that knows the workspace layout (include/pmf_amd.h, pmf_loss_sort_workspace): four blocks of R * P 32-bit
    words, R = 2C; the sorted pixel indices are block 3 (uint32), the sorted errors block 0 (float).
    Returns (idx int64 [R][P], err float32 [R][P]); only the first P - cnt[0] ranks of present rows mean anything."""
    R = 2 * C
    w = words.numpy()
    assert w.size >= PASSES * R * P
    block = lambda k: w[k * R * P:(k + 1) * R * P].reshape(R, P)                                            # noqa: E731
    return block(3).view(np.uint32).astype(np.int64), block(0).view(np.float32)


class Case:
    """the buffers of one run on the device; collect() checks every band and input and returns the outputs"""

    def __init__(self, x, weighted):
        lib = L.lib()
        self.x, self.weighted = x, weighted
        N, HW, C, P = x["N"], x["HW"], x["C"], x["P"]
        self.nb = lib.pmf_loss_chunks(P)
        assert self.nb == -(-P // V.CHUNK) and lib.pmf_loss_rows(P) == x["nrows"]
        t = torch.from_numpy
        self.key = Buf(2 * C, P, P, fill=t(x["key"]))
        self.label, self.cnt = WBuf(t(x["label"])), WBuf(t(x["cnt"]))
        self.rows = DBuf(x["nrows"], 4, fill=t(x["rows"]))
        self.w6 = Buf(1, 6, 6, fill=torch.tensor(V.W6))
        self.bsum, self.dots = Buf(2 * C, self.nb, self.nb), DBuf(2 * C, self.nb)
        self.gl, self.gc = Buf(N * C, HW, HW, fill=t(x["pre_gl"])), Buf(N * C, HW, HW, fill=t(x["pre_gc"]))
        self.out8 = Buf(1, 8, 8)
        self.tail = (self.bsum.ptr, self.dots.ptr, self.rows.ptr, self.gl.ptr, self.gc.ptr, self.out8.ptr, st())
        self.ws = self.perm = self.vals = None

    def sort(self):
        lib, x = L.lib(), self.x
        self.ws = WBuf(words=lib.pmf_loss_sort_workspace(x["C"], x["P"]) // 4)
        head = (self.key.ptr, self.label.ptr, x["N"], x["C"], x["HW"], self.cnt.ptr)
        if self.weighted:
            ok(lib.pmf_loss_lovasz_sort_w(*head, self.w6.ptr, self.ws.ptr, *self.tail), "pmf_loss_lovasz_sort_w")
        else:
            ok(lib.pmf_loss_lovasz_sort(*head, V.LAMBDA, V.GAMMA_PER, self.ws.ptr, *self.tail), "pmf_loss_lovasz_sort")
        return self.collect()

    def int64(self, ref):
        """pmf_loss_lovasz(_w) behind the reference's full-length permutation and sorted keys"""
        lib, x = L.lib(), self.x
        self.perm = WBuf(torch.from_numpy(ref["perm_full"]))
        self.vals = Buf(2 * x["C"], x["P"], x["P"], fill=torch.from_numpy(ref["val_full"]))
        head = (self.perm.ptr, self.vals.ptr, self.label.ptr, x["N"], x["C"], x["HW"], self.cnt.ptr)
        if self.weighted:
            ok(lib.pmf_loss_lovasz_w(*head, self.w6.ptr, *self.tail), "pmf_loss_lovasz_w")
        else:
            ok(lib.pmf_loss_lovasz(*head, V.LAMBDA, V.GAMMA_PER, *self.tail), "pmf_loss_lovasz")
        return self.collect()

    def unchanged(self, what):
        """nothing at all was written: a refused call"""
        for b in (self.key, self.rows, self.w6, self.bsum, self.dots, self.gl, self.gc, self.out8):
            b.check(what, rows_written=0)
        for b in (self.label, self.cnt, self.ws, self.perm):
            if b is not None:
                b.check(what)

    def collect(self):
        torch.cuda.synchronize()
        x = self.x
        for b in (self.key, self.rows, self.w6, self.vals):
            if b is not None:
                b.check("input", rows_written=0)
        for b in (self.label, self.cnt, self.perm):
            if b is not None:
                b.check("input")
        self.bsum.check("bsum")
        shape = (x["N"], x["C"], x["HW"])
        out = {"gl": self.gl.check("gl").numpy().reshape(shape), "gc": self.gc.check("gc").numpy().reshape(shape),
               "dots": self.dots.check("dots").numpy(), "out8": self.out8.check("out8").numpy().reshape(8)}
        if self.ws is not None:
            out["idx"], out["err"] = sorted_from_workspace(self.ws.check("sort workspace", written=True), x["C"], x["P"])
        return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_sort(got, ref, what):
    m = ref["m"]
    for r, row in ref["rows"].items():
        idx = got["idx"][r, :m]
        bad = np.nonzero(idx != row["perm"])[0]
        assert bad.size == 0, "%s row %d: %d of %d ranks hold another pixel, first at rank %d: pixel %d, reference %d" % (
            what, r, bad.size, m, bad[0], idx[bad[0]], row["perm"][bad[0]])
        assert np.array_equal(bits(got["err"][r, :m]), bits(row["err"])), "%s row %d: sorted errors are not bit-equal" % (what, r)


def check_outputs(x, got, ref, what):
    """gl, gc, the row values and out8 against the reference; prints worst err / bound"""
    for h, name in enumerate(("gl", "gc")):
        t = ref["touched"][h]
        same = bits(got[name]) == bits(x["pre_" + name])
        assert same[~t].all(), "%s %s: %d elements outside the stage's reach differ from the prefill" % (
            what, name, int((~same[~t]).sum()))
    assert not any(np.isnan(got["dots"][r]).any() for r in ref["rows"]), what + ": a chunk of a present row has no dot product"
    got = dict(got, values={r: float(got["dots"][r].sum()) for r in ref["rows"]})
    rt = V.ratios(got, ref)
    print("%s: worst err / bound: gradient %.3f, row values %.3f, out8 %.3f" % (what, rt["grad"], rt["row"], rt["out8"]))
    assert rt["grad"] <= 1.0, "%s: a gradient element is %.3g x its bound off" % (what, rt["grad"])
    assert rt["row"] <= 1.0, "%s: a row value is %.3g x its bound off" % (what, rt["row"])
    e8 = np.abs(got["out8"].astype(np.float64) - ref["out8"]) / ref["out8_bound"]
    assert rt["out8"] <= 1.0, "%s: out8 err / bound %s: got %s reference %s" % (what, e8, got["out8"], ref["out8"])
    if ref["m"] == 0:                                         # everything unlabelled
        assert got["out8"][2] == 0 and got["out8"][4] == 0


def same_run(a, b, ref, what):
    for k in ("gl", "gc", "out8"):
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s: %s differs between two runs" % (what, k)
    for r in ref["rows"]:
        assert np.array_equal(a["idx"][r, :ref["m"]], b["idx"][r, :ref["m"]]), "%s: the permutation differs between two runs" % what


# ================================================================================================ the stage with its sort
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_lovasz_sort(name):
    x = V.inputs(name)
    for weighted in (False, True):
        ref = V.case_ref(name, weighted)
        what = "%s %s" % ("lovasz_sort_w" if weighted else "lovasz_sort", name)
        got = Case(x, weighted).sort()
        check_sort(got, ref, what)
        check_outputs(x, got, ref, what)
        if not weighted:
            same_run(got, Case(x, weighted).sort(), ref, what)


# ================================================================================================ behind a caller's permutation
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_lovasz_int64_permutation(name):
    """labelled pixels first in stable descending order, unlabelled at the tail with key -1: the <int64_t, false> kernels on
    the two-dimensional grid"""
    x = V.inputs(name)
    for weighted in (False, True):
        ref = V.case_ref(name, weighted)
        what = "%s %s" % ("lovasz_w" if weighted else "lovasz", name)
        m, lab = ref["m"], x["label"]
        assert (lab[ref["perm_full"][:, :m]] != 0).all() and (ref["val_full"][:, m:] == -1).all()
        check_outputs(x, Case(x, weighted).int64(ref), ref, what)


# ================================================================================================ pmf_lovasz_grad
@pytest.mark.parametrize("P", V.GRAD_P)
def test_lovasz_grad(P):
    lib, worst = L.lib(), 0.0
    for nv in V.grad_nvalid(P):
        fg = V.grad_inputs(P, nv)
        nb = -(-P // V.CHUNK)
        f, n = Buf(3, P, P, fill=torch.from_numpy(fg)), WBuf(torch.tensor([nv], dtype=torch.int64))
        bsum, grad = Buf(3, nb, nb), Buf(3, P, P)
        ok(lib.pmf_lovasz_grad(f.ptr, 3, P, n.ptr, bsum.ptr, grad.ptr, st()), "pmf_lovasz_grad")
        torch.cuda.synchronize()
        f.check("fg (input)", rows_written=0)
        n.check("n_valid (input)")
        bsum.check("bsum")
        g = grad.check("grad").numpy()
        assert not np.isnan(g).any(), "P=%d n_valid=%d: grad not fully written" % (P, nv)
        assert not bits(g[:, nv:]).any(), "P=%d n_valid=%d: elements from n_valid on are not 0.0" % (P, nv)
        e = np.abs(g.astype(np.float64) - V.grad_ref(fg, nv)) / V.GRAD_BOUND
        worst = max(worst, float(e.max()))
        assert e.max() <= 1.0, "P=%d n_valid=%d: %d elements beyond 3 * 2^-24, worst %.3g x, first at %s" % (
            P, nv, int((e > 1).sum()), e.max(), np.argwhere(e > 1)[0])
    print("pmf_lovasz_grad P=%d: worst err / bound %.3f" % (P, worst))


# ================================================================================================ argument checks
def test_lovasz_entry_points_refuse_bad_arguments():
    """C < 2, C > 32, N < 1, HW < 1, a null workspace, a null w6: PMF_E_ARG; more than 2^24 pixels: PMF_E_UNSUPPORTED (ranks and
    counts are float32).  A refused call launches nothing: every buffer, prefilled, is bit-unchanged"""
    lib = L.lib()
    x = V.inputs("wave")
    ref = V.case_ref("wave", False)
    cs = Case(x, True)
    cs.ws = WBuf(words=lib.pmf_loss_sort_workspace(x["C"], x["P"]) // 4)
    cs.perm = WBuf(torch.from_numpy(ref["perm_full"]))
    cs.vals = Buf(2 * x["C"], x["P"], x["P"], fill=torch.from_numpy(ref["val_full"]))
    A, UNS, big = L.PMF_E_ARG, L.PMF_E_UNSUPPORTED, V.P_MAX + 1
    bad = [(1, 1, 35, A), (1, 33, 35, A), (0, 3, 35, A), (-1, 3, 35, A), (1, 3, 0, A), (1, 3, -5, A),
           (1, 3, big, UNS), (4097, 3, 4096, UNS), (2, 3, 1 << 40, UNS)]

    def sort(N, C, HW, ws=cs.ws.ptr, w6=cs.w6.ptr, weighted=False):
        head = (cs.key.ptr, cs.label.ptr, N, C, HW, cs.cnt.ptr)
        if weighted:
            return lib.pmf_loss_lovasz_sort_w(*head, w6, ws, *cs.tail)
        return lib.pmf_loss_lovasz_sort(*head, V.LAMBDA, V.GAMMA_PER, ws, *cs.tail)

    def int64(N, C, HW, w6=cs.w6.ptr, weighted=False):
        head = (cs.perm.ptr, cs.vals.ptr, cs.label.ptr, N, C, HW, cs.cnt.ptr)
        if weighted:
            return lib.pmf_loss_lovasz_w(*head, w6, *cs.tail)
        return lib.pmf_loss_lovasz(*head, V.LAMBDA, V.GAMMA_PER, *cs.tail)

    for N, C, HW, want in bad:
        for weighted in (False, True):
            assert sort(N, C, HW, weighted=weighted) == want, (N, C, HW, weighted)
            assert int64(N, C, HW, weighted=weighted) == want, (N, C, HW, weighted)
    assert sort(1, 3, 35, ws=None) == A and sort(1, 3, 35, ws=None, weighted=True) == A
    assert sort(1, 3, 35, w6=None, weighted=True) == A and int64(1, 3, 35, w6=None, weighted=True) == A
    for C, P, want in ((0, 35, A), (3, 0, A), (3, -1, A), (3, big, UNS), (1, 1 << 31, UNS)):
        assert lib.pmf_lovasz_grad(cs.vals.ptr, C, P, cs.cnt.ptr, cs.bsum.ptr, cs.gl.ptr, st()) == want, (C, P)
    torch.cuda.synchronize()
    cs.unchanged("refused calls")
