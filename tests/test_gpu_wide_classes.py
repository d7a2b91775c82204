"""-m gpu: 33 to 64 classes (include/pmf_amd_wide.h) -- the wide softmax family, the per-pixel and Lovasz stages of the fused
objective behind pmf_loss_pixel_wide / pmf_loss_lovasz_sort_wide, the three fused objectives end to end, and the networks and
the EPMF engine at 39 classes.

The references, bounds and rules (guard bands of a NaN-payload sentinel, outputs prefilled with that NaN, inputs bit-unchanged)
are those of tests/test_gpu_elementwise.py, tests/test_gpu_loss_pixel.py and tests/test_gpu_lovasz.py, whose buffers and checks
this file reuses; the cases, the softmax bounds measured over the wide channel counts and the recorded restatement ratios are
in tests/wide_class_cases.py (held on the host by tests/test_wide_classes_host.py).  Below the boundary (C = 20, 32) the wide
entry points must give the very bits of the entry points of pmf_amd.h: they launch the same kernels."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.utils.detinit import deterministic_init, det_tensor, synthetic_batch  # noqa: E402
from tests import gpu_helpers as G  # noqa: E402
from tests import loss_pixel_cases as PV  # noqa: E402
from tests import lovasz_cases as LV  # noqa: E402
from tests import wide_class_cases as W  # noqa: E402
from tests import test_gpu_loss_pixel as TP  # noqa: E402
from tests import test_gpu_lovasz as TL  # noqa: E402
from tests.test_gpu_elementwise import Buf, NB, TINY, close, ok, sm_layouts, softmax_case, st  # noqa: E402

F64 = np.float64


# ================================================================================================ 1. softmax family
def run_softmax_wide(N, HW, C, ldc, off, span):
    """test_gpu_elementwise.run_softmax_family through pmf_softmax_wide / pmf_softmax_wide_bwd under the wide K"""
    lib = L.lib()
    x, go = softmax_case(N, HW, C, span)
    ksm, ksb = W.SM_K["softmax"][span], W.SM_K["softmax_bwd"][span]
    what = "C=%d ldc=%d HW=%d span=%g" % (C, ldc, HW, span)
    xb = Buf(N * HW, C, ldc, fill=x, offset=off)
    pb = Buf(N * C, HW, HW)
    ok(lib.pmf_softmax_wide(xb.ptr, ldc, N, HW, C, 0, pb.ptr, st()), "pmf_softmax_wide")
    p64 = torch.softmax(x.double(), 2).permute(0, 2, 1)
    close(pb.check("softmax"), p64, p64, ksm, "softmax " + what, floor=TINY)
    xb.check("logits (input)", rows_written=0)
    lb = Buf(N * C, HW, HW)
    ok(lib.pmf_softmax_wide(xb.ptr, ldc, N, HW, C, 1, lb.ptr, st()), "pmf_softmax_wide (ident)")
    assert torch.equal(lb.check("logits").view(N, C, HW), x.permute(0, 2, 1)), "pass-through " + what
    # backward, on float32 probabilities as the forward pass hands them over
    p32 = torch.softmax(x, 2).permute(0, 2, 1).contiguous()
    p32b, gob = Buf(N * C, HW, HW, fill=p32), Buf(N * C, HW, HW, fill=go)
    db = Buf(N * HW, C, ldc, offset=off)
    ok(lib.pmf_softmax_wide_bwd(p32b.ptr, gob.ptr, N, HW, C, 0, db.ptr, ldc, st()), "pmf_softmax_wide_bwd")
    pd, gd = p32.double(), go.double()
    ref = pd * (gd - (pd * gd).sum(1, keepdim=True))
    mag = pd * (gd.abs() + (pd * gd.abs()).sum(1, keepdim=True))
    close(db.check("softmax_bwd", zero_pad=True).view(N, HW, C), ref.permute(0, 2, 1), mag.permute(0, 2, 1), ksb,
          "softmax_bwd " + what, floor=TINY)
    db = Buf(N * HW, C, ldc, offset=off)
    ok(lib.pmf_softmax_wide_bwd(None, gob.ptr, N, HW, C, 1, db.ptr, ldc, st()), "pmf_softmax_wide_bwd (ident)")
    assert torch.equal(db.check("logits_bwd", zero_pad=True).view(N, HW, C), go.permute(0, 2, 1)), "pass-through backward " + what
    for b in (p32b, gob):
        b.check("input", rows_written=0)


@pytest.mark.parametrize("C", W.SM_C)
def test_softmax_family_wide(C):
    """both layouts (VEC: ldc rounded up to 8 at offset 0; scalar: ldc = C at offset 1); HW 1, 7, 45, 300 at span 80 and 7, 45 at
    span 100 (exp(100) overflows float32: the max subtraction).  The wide kernels run one thread per pixel on a grid without a
    cap, so there is no grid-stride wrap to test."""
    for span in sorted(W.SM_HW):
        for ldc, off in sm_layouts(C):
            for HW in W.SM_HW[span]:
                run_softmax_wide(NB, HW, C, ldc, off, span)


def test_softmax_wide_pad_beyond_one_vector():
    """C = 33 in rows of ldc = 64: 31 pad channels, all written as 0 by the backward, none read into the forward"""
    run_softmax_wide(2, 45, 33, 64, 0, 80.0)


# ================================================================================================ 2. per-pixel stage
class WideRun(TP.Run):
    """test_gpu_loss_pixel.Run with every call through pmf_loss_pixel_wide"""

    def call(self, kind, w6=None):
        lib, x = L.lib(), self.x
        self.kind = kind
        parts = dice = wp = None
        if kind == "w":
            self.w6 = Buf(1, 6, 6, fill=torch.tensor(w6, dtype=torch.float32))
            wp = self.w6.ptr
        elif kind == "dice":
            parts, dice = self.parts.ptr, self.dice.ptr
        rc = lib.pmf_loss_pixel_wide(*self.head(), x["gper"], *self.tail(), parts, dice, wp, st())
        assert rc == 0, "pmf_loss_pixel_wide (%s) returned %d" % (kind, rc)
        return self.collect()


@pytest.mark.parametrize("name", W.PIXEL_NAMES)
def test_pixel_stage_wide(name):
    """test_gpu_loss_pixel.test_pixel_stage on the wide cases"""
    x, ref = W.pixel_inputs(name), W.pixel_ref(name)
    assert ref["left_out"].mean() <= 0.05
    worst = {}
    for spec, w6 in PV.WSPECS.items():
        what = "%s %s" % (name, spec)
        got = WideRun(x).call("plain" if w6 is None else "w", w6)
        TP.check_exact(x, got, ref, what)
        worst["rows"] = max(worst.get("rows", 0.0), TP.check_rows(x, got, ref, what))
        q = PV.QUANTITY[spec]
        worst[q] = max(worst.get(q, 0.0), TP.check_grad(x, got, ref, spec, what))
        if spec == "w6":
            other = WideRun(x).call("w", PV.W6_OTHER_LOV)
            for k in ("gl", "gc", "rows", "key"):
                assert got[k].tobytes() == other[k].tobytes(), "%s: %s depends on w6[1] / w6[3]" % (what, k)
    lov = WideRun(x).call("w", PV.W_LOV_ONLY)
    assert not lov["gl"].any() and not lov["gc"].any(), name + ": a gradient under the Lovasz weights alone"
    got = WideRun(x).call("dice")
    TP.check_exact(x, got, ref, name + " dice")
    worst["rows"] = max(worst["rows"], TP.check_rows(x, got, ref, name + " dice"))
    worst["grad_dice"] = TP.check_grad(x, got, ref, "dice", name + " dice")
    worst["parts"], worst["dice"] = TP.check_dice_outputs(x, got, ref, name + " dice")
    print("%s: worst err / bound: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", W.PIXEL_DICE_NAMES)
def test_dice_parts_fold_and_gradient_wide(name):
    """test_gpu_loss_pixel.test_dice_parts_fold_and_gradient on the wide Dice cases: 17 tiles (one past the fold's 16 groups,
    a ragged last tile) at 39 classes, 16 full tiles at 64"""
    x, ref = W.pixel_inputs(name), W.pixel_ref(name)
    got, plain = WideRun(x).call("dice"), WideRun(x).call("plain")
    TP.check_exact(x, got, ref, name)
    rr = TP.check_rows(x, got, ref, name)
    rp, rd = TP.check_dice_outputs(x, got, ref, name)
    rg = TP.check_grad(x, got, ref, "dice", name)
    TP.check_grad(x, plain, ref, "plain", name + " <false>")
    assert got["rows"].tobytes() == plain["rows"].tobytes() and got["key"].tobytes() == plain["key"].tobytes()
    tl, tc, _, _ = PV.grad_ref(x, ref, "dice_term")
    bl, bc = PV.instantiation_bound(x, ref)
    worst = 0.0
    for k, term, b in (("gl", tl, bl), ("gc", tc, bc)):
        want = plain[k].astype(F64) + term
        worst = max(worst, PV.worst_ratio(got[k], want, b + PV.U * np.abs(want), ref["cmp"]))
    assert worst <= 1.0, "%s: <true> - <false> is %.3g x its bound off the Dice term" % (name, worst)
    print("%s: worst err / bound: parts %.3f, dice %.3f, rows %.3f, gradient %.3f, <true> - <false> %.3f" % (name, rp, rd, rr, rg, worst))


def test_dice_finish_wide_on_a_prefilled_out10():
    lib = L.lib()
    C = 39
    d = W.pixel_ref("wd39")["dice"]["dice"]
    pre = np.arange(10, dtype=np.float32) * 0.375 + 1
    dice, out = TP.DBuf(2, 2 + 2 * C, fill=torch.from_numpy(d)), Buf(1, 10, 10, fill=torch.from_numpy(pre))
    assert lib.pmf_loss_dice_finish_wide(dice.ptr, C, out.ptr, st()) == 0
    torch.cuda.synchronize()
    dice.check("dice (input)", rows_written=0)
    o = out.check("out10").numpy().reshape(10)
    want = pre.copy()
    want[8], want[9] = np.float32(d[0, 0]), np.float32(d[1, 0])
    want[0] = np.float32(float(pre[0]) + d[0, 0] + d[1, 0])
    assert np.array_equal(TP.bits(o), TP.bits(want)), (o, want)


def test_wide_pixel_refusals_write_nothing():
    """on the device: the refused calls of the host test leave every prefilled buffer bit-unchanged, and the same buffers are then
    accepted"""
    lib = L.lib()
    x, ref = W.pixel_inputs("w40"), W.pixel_ref("w40")
    r = WideRun(x)
    A = L.PMF_E_ARG
    h = list(r.head())
    h[5] = 65
    assert lib.pmf_loss_pixel_wide(*h, x["gper"], *r.tail(), None, None, None, st()) == A
    assert lib.pmf_loss_pixel_wide(*r.head(), x["gper"], *r.tail(), r.parts.ptr, r.dice.ptr, r.w6.ptr, st()) == A
    assert lib.pmf_loss_pixel_wide(*r.head(), x["gper"], *r.tail(), r.parts.ptr, None, None, st()) == A
    t = list(r.tail())
    t[6] = None
    assert lib.pmf_loss_pixel_wide(*r.head(), x["gper"], *t, None, None, None, st()) == A
    assert lib.pmf_loss_pixel(*r.head(), x["gper"], *r.tail(), st()) == A            # 40 classes: pmf_amd.h still refuses
    torch.cuda.synchronize()
    r.unchanged("refused calls")
    got = r.call("plain")
    TP.check_exact(x, got, ref, "accepted after the refusals")
    TP.check_grad(x, got, ref, "plain", "accepted after the refusals")


# ================================================================================================ 3. Lovasz stage
class WideCase(TL.Case):
    """test_gpu_lovasz.Case with the sort through pmf_loss_lovasz_sort_wide"""

    def sort(self):
        lib, x = L.lib(), self.x
        self.ws = TL.WBuf(words=lib.pmf_loss_sort_workspace(x["C"], x["P"]) // 4)
        head = (self.key.ptr, self.label.ptr, x["N"], x["C"], x["HW"], self.cnt.ptr)
        w6 = self.w6.ptr if self.weighted else None
        ok(lib.pmf_loss_lovasz_sort_wide(*head, LV.LAMBDA, LV.GAMMA_PER, self.ws.ptr, *self.tail[:-1], w6, self.tail[-1]),
           "pmf_loss_lovasz_sort_wide")
        return self.collect()


@pytest.mark.parametrize("name", W.LOVASZ_NAMES)
def test_lovasz_sort_wide(name):
    x = W.lovasz_inputs(name)
    for weighted in (False, True):
        ref = W.lovasz_ref(name, weighted)
        what = "lovasz_sort_wide%s %s" % (" (w6)" if weighted else "", name)
        got = WideCase(x, weighted).sort()
        TL.check_sort(got, ref, what)
        TL.check_outputs(x, got, ref, what)
        if not weighted:
            TL.same_run(got, WideCase(x, weighted).sort(), ref, what)


# ================================================================================================ 4. same bits below the boundary
@pytest.mark.parametrize("name", ["c20", "c32"])
def test_pixel_stage_same_bits_as_the_narrow_entry_points(name):
    x = PV.inputs(name)
    assert x["C"] in (20, 32)
    for kind, w6 in (("plain", None), ("w", PV.W6), ("dice", None)):
        a, b = TP.Run(x).call(kind, w6), WideRun(x).call(kind, w6)
        for k in sorted(a):
            if kind != "dice" and k in ("parts", "dice"):
                continue                                       # (not written: the sentinel, NaN != NaN)
            assert a[k].tobytes() == b[k].tobytes(), "%s %s: %s differs between pmf_amd.h's entry point and the wide one" % (name, kind, k)


@pytest.mark.parametrize("C", [20, 32])
def test_lovasz_stage_same_bits_as_the_narrow_entry_points(C):
    x = W.lovasz_make(LV._case("same%d" % C, 1, 8229, C, 4097, "absent_single", ("special", "eighths")))
    for weighted in (False, True):
        ca, cb = TL.Case(x, weighted), WideCase(x, weighted)
        a, b = ca.sort(), cb.sort()
        ref = W.lovasz_reference(x, weighted)
        # (bsum: rows of class 0 and of absent classes are not written and keep the sentinel in both)
        assert torch.equal(ca.bsum.check("bsum").view(torch.int32), cb.bsum.check("bsum (wide)").view(torch.int32)), "C=%d: bsum" % C
        TL.check_outputs(x, b, ref, "same%d" % C)
        for k in ("gl", "gc", "out8"):
            assert a[k].tobytes() == b[k].tobytes(), "C=%d: %s differs between pmf_amd.h's entry point and the wide one" % (C, k)
        for r in ref["rows"]:
            assert a["dots"][r].tobytes() == b["dots"][r].tobytes()
            assert np.array_equal(a["idx"][r, :ref["m"]], b["idx"][r, :ref["m"]])
            assert a["err"][r, :ref["m"]].tobytes() == b["err"][r, :ref["m"]].tobytes()


@pytest.mark.parametrize("C", [20, 32])
def test_softmax_family_same_bits_as_the_narrow_entry_points(C):
    lib = L.lib()
    N, HW = NB, 45
    for ldc, off in sm_layouts(C):
        x, go = softmax_case(N, HW, C, 80.0)
        xb = Buf(N * HW, C, ldc, fill=x, offset=off)
        pa, pb, la, lb = (Buf(N * C, HW, HW) for _ in range(4))
        ok(lib.pmf_softmax_nhwc_to_nchw(xb.ptr, ldc, N, HW, C, pa.ptr, st()), "narrow")
        ok(lib.pmf_softmax_wide(xb.ptr, ldc, N, HW, C, 0, pb.ptr, st()), "wide")
        ok(lib.pmf_logits_nhwc_to_nchw(xb.ptr, ldc, N, HW, C, la.ptr, st()), "narrow ident")
        ok(lib.pmf_softmax_wide(xb.ptr, ldc, N, HW, C, 1, lb.ptr, st()), "wide ident")
        p = pa.check("softmax")
        assert torch.equal(p.view(torch.int32), pb.check("softmax (wide)").view(torch.int32))
        assert torch.equal(la.check("logits"), lb.check("logits (wide)"))
        pin, gob = Buf(N * C, HW, HW, fill=p), Buf(N * C, HW, HW, fill=go)
        da, db, ia, ib = (Buf(N * HW, C, ldc, offset=off) for _ in range(4))
        ok(lib.pmf_softmax_bwd_nchw_to_nhwc(pin.ptr, gob.ptr, N, HW, C, da.ptr, ldc, st()), "narrow bwd")
        ok(lib.pmf_softmax_wide_bwd(pin.ptr, gob.ptr, N, HW, C, 0, db.ptr, ldc, st()), "wide bwd")
        ok(lib.pmf_logits_bwd_nchw_to_nhwc(gob.ptr, N, HW, C, ia.ptr, ldc, st()), "narrow ident bwd")
        ok(lib.pmf_softmax_wide_bwd(None, gob.ptr, N, HW, C, 1, ib.ptr, ldc, st()), "wide ident bwd")
        assert torch.equal(da.check("bwd", zero_pad=True).view(torch.int32), db.check("bwd (wide)", zero_pad=True).view(torch.int32))
        assert torch.equal(ia.check("ident bwd", zero_pad=True), ib.check("ident bwd (wide)", zero_pad=True))


# ================================================================================================ 5. objective end to end
def _objective_inputs(n, c, h, w, variant):
    la, lb = det_tensor("wide.a", (n, c, h, w), -4, 4), det_tensor("wide.b", (n, c, h, w), -4, 4)
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=5, fill=0.7 if variant == "ignored" else 1.0)
    label = label.long()
    if variant == "absent":
        label = torch.where(label == 7, torch.zeros_like(label), label)
        assert not (label == 7).any()
    assert (label == 0).any() and label.max().item() < c and (label > 0).any()
    alpha = np.linspace(0.2, 1.0, c).astype(np.float32)
    alpha[0] = 0
    return la, lb, label, alpha


@pytest.mark.parametrize("variant", ["ignored", "absent"])
@pytest.mark.parametrize("shape", [(2, 39, 16, 32), (1, 64, 8, 32)])
def test_fused_objectives_match_float64_autograd(shape, variant):
    """pmf_total_loss_fused, weighted_loss_fused and sensat_total_loss_fused against float64 autograd of the torch-op objectives
    (tolerances of test_gpu_parity.test_fused_loss_matches_reference_objective); confusion matrices exact"""
    from pmf_amd.loss import (ExpLogDiceLoss, FocalSoftmaxLoss, Lovasz_softmax, pmf_total_loss, pmf_total_loss_fused,
                              sensat_total_loss_fused, weighted_loss_fused)
    from pmf_amd.loss.perception import EPMF_TERMS, epmf_total_loss, sensat_total_loss
    from pmf_amd.metrics import IOUEval
    n, c, h, w = shape
    la, lb, label, alpha = _objective_inputs(n, c, h, w, variant)
    w6 = torch.tensor(PV.W6, dtype=torch.float32)
    order = ("foc", "lov", "foc_cam", "lov_cam", "per", "per_img")        # w6's order, in epmf_total_loss's names

    def weighted_sum(terms):
        return sum(float(w6[order.index(k)]) * t for k, t in zip(EPMF_TERMS, terms))

    def reference(kind):
        pa = torch.softmax(la.double(), 1).requires_grad_(True)
        pb = torch.softmax(lb.double(), 1).requires_grad_(True)
        foc, lov = FocalSoftmaxLoss(c, gamma=2, alpha=alpha, softmax=False).double(), Lovasz_softmax(ignore=0)
        if kind == "pmf":
            tot, t = pmf_total_loss(pa, pb, label, foc, lov, 1.0, 0.5, 0.7)
        elif kind == "sensat":
            tot, t = sensat_total_loss(pa, pb, label, foc, lov, ExpLogDiceLoss(), 1.0, 0.5, 0.7)
        else:
            tot, t = epmf_total_loss(pa, pb, label, foc, lov, weighted_sum, 0.7)
        tot.backward()
        return pa, pb, tot, t

    for kind in ("pmf", "weighted", "sensat"):
        pa, pb, ref, rt = reference(kind)
        ga, gb = pa.detach().float().cuda().requires_grad_(True), pb.detach().float().cuda().requires_grad_(True)
        ml, mc = IOUEval(c, "cuda", ignore=[0]), IOUEval(c, "cuda", ignore=[0])
        al = torch.from_numpy(alpha)
        if kind == "pmf":
            tot, tt = pmf_total_loss_fused(ga, gb, label.cuda(), al, 1.0, 0.5, 0.7, 2.0, ml.conf_matrix, mc.conf_matrix)
            keys = ("foc", "lov", "foc_cam", "lov_cam", "per")
        elif kind == "sensat":
            tot, tt = sensat_total_loss_fused(ga, gb, label.cuda(), al, 1.0, 0.5, 0.7, 2.0, ml.conf_matrix, mc.conf_matrix)
            keys = ("foc", "lov", "foc_cam", "lov_cam", "per", "dice", "dice_cam")
        else:
            tot, tt = weighted_loss_fused(ga, gb, label.cuda(), al, w6.cuda(), 0.7, 2.0, ml.conf_matrix, mc.conf_matrix)
            keys = order
        tot.backward()
        what = "%s %s %s" % (kind, shape, variant)
        assert abs(tot.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item())), what
        for k in keys:
            assert abs(tt[k].item() - rt[k].item()) < 2e-6 * max(1.0, abs(rt[k].item())), (what, k)
        for got, want in ((ga.grad, pa.grad), (gb.grad, pb.grad)):
            err = (got.cpu().double() - want).abs().max().item()
            assert err < 1e-6 * max(want.abs().max().item(), 1e-3) + 1e-9, (what, err)
        rl, rc = IOUEval(c, "cpu", ignore=[0]), IOUEval(c, "cpu", ignore=[0])
        rl.addBatch(pa.argmax(1), label)
        rc.addBatch(pb.argmax(1), label)
        assert torch.equal(ml.conf_matrix.cpu(), rl.conf_matrix) and torch.equal(mc.conf_matrix.cpu(), rc.conf_matrix), what


def test_fused_objective_refuses_65_classes():
    from pmf_amd.loss import pmf_total_loss_fused
    p = torch.softmax(torch.zeros(1, 65, 4, 8), 1).cuda()
    with pytest.raises(ValueError) as e:
        pmf_total_loss_fused(p, p, torch.ones(1, 4, 8, dtype=torch.long).cuda(), torch.ones(65))
    assert "65 classes" in str(e.value)


# ================================================================================================ 6. networks
NCLS = 39


def test_epmf_39_classes_eval_and_train_match_oracle():
    """test_gpu_parity.test_epmf_eval_and_train_match_oracle at 39 classes, minus its fixture lines: the 1x1 logits convolution
    and the decoder's 3x3 convolution at Cout = 39 in forward, input gradient and weight gradient, the wide softmax pair"""
    from pmf_amd.models import EPMFNet
    from oracle import epmf_torch as E
    from oracle import pmf_torch as O
    from oracle import losses_ref
    from tests.test_gpu_parity import _dump, _masks
    hip = deterministic_init(EPMFNet(5, 3, NCLS, 32, False, "resnet34")).cuda()
    ref = deterministic_init(E.EPMFNet(5, 3, NCLS, 32, False, "resnet34"))
    n, h, w = 2, 64, 128
    pcd, rgb, label, _ = synthetic_batch(n, h, w, NCLS, seed=1, fill=0.3)
    hip.eval()
    ref.eval()
    with torch.no_grad():
        rl, rc = ref(pcd, rgb)
        lp, cp = hip(pcd.cuda(), rgb.cuda())
    plan = next(iter(hip._plans.values()))
    assert lp.shape == (n, NCLS, h, w) and cp.shape == (n, NCLS, h, w)
    assert G.rel_err(plan.read(plan.tensors["logits"]).cpu().numpy(), ref.lidar_stream.last_logits.numpy()) < 1e-3
    assert (lp.cpu() - rl).abs().max() < 1e-4 and (cp.cpu() - rc).abs().max() < 1e-4
    # ---- train step, dropout on with injected masks
    hip.train()
    ref.train()
    m = _masks(ref, n)
    O.set_dropout_masks(ref, m)
    hip.set_dropout_masks({k: v.cuda() for k, v in m.items()})
    ref64 = copy.deepcopy(ref).double()
    O.set_dropout_masks(ref64, {k: v.double() for k, v in m.items()})
    alpha = torch.linspace(0.2, 1.0, NCLS)
    alpha[0] = 0
    rl, rc = ref(pcd, rgb)
    losses_ref.pmf_total_loss(rl, rc, label, alpha)[0].backward()
    dl, dc = ref64(pcd.double(), rgb.double())
    total_d, _ = losses_ref.pmf_total_loss(dl, dc, label, alpha.double())
    total_d.backward()
    lp, cp = hip(pcd.cuda(), rgb.cuda())
    lp.retain_grad()
    cp.retain_grad()
    total_h, _ = losses_ref.pmf_total_loss(lp, cp, label.cuda(), alpha.cuda())
    total_h.backward()
    torch.cuda.synchronize()
    plan = [p for p in hip._plans.values() if p.training][0]
    assert G.rel_err(plan.read(plan.tensors["logits"]).cpu().numpy(), ref64.lidar_stream.last_logits.detach().float().numpy()) < 1e-3
    assert abs(total_h.item() - total_d.item()) < 1e-4 * max(1.0, abs(total_d.item()))
    rsd = ref.state_dict()
    for k, v in hip.state_dict().items():
        if "running_" in k:
            assert G.scale_err(v.cpu().numpy(), rsd[k].numpy()) < 1e-4, k
    rows = G.masked_grad_rows(hip, plan, deterministic_init(E.EPMFNet(5, 3, NCLS, 32, False, "resnet34")), m, pcd, rgb,
                              (lp.grad, cp.grad))
    _dump("epmf39_train_grads.txt", rows)
    G.assert_masked_bar(rows, "EPMF train step at 39 classes")


def test_pmf_39_classes_eval_forward_matches_oracle():
    from pmf_amd.models import PMFNet
    from oracle import pmf_torch as O
    from tests.test_gpu_parity import _dump, _report
    hip = deterministic_init(PMFNet(5, 3, NCLS, 32, False, "resnet34")).cuda().eval()
    ref = deterministic_init(O.PMFNet(5, 3, NCLS, 32, False, "resnet34")).eval()
    n, h, w = 2, 32, 64
    pcd, rgb, _, _ = synthetic_batch(n, h, w, NCLS, seed=1)
    cap, hs = G.capture_oracle(ref)
    with torch.no_grad():
        rl, rc = ref(pcd, rgb)
        lp, cp = hip(pcd.cuda(), rgb.cuda())
    torch.cuda.synchronize()
    plan = next(iter(hip._plans.values()))
    rows = G.compare_plan_to_oracle(plan, cap)
    _dump("eval_fwd_pmf39.txt", rows)
    bad, txt = _report(rows, 1e-3)
    assert not bad, "intermediate mismatch (rel err, oracle order):\n" + txt
    assert (lp.cpu() - rl).abs().max() < 1e-4 and (cp.cpu() - rc).abs().max() < 1e-4


def test_salsanext_39_classes_logits_match_oracle():
    """SalsaNext(softmax=False): the wide pass-through; logits at the parity file's tolerance for logits, rel_err < 1e-3"""
    from pmf_amd.models import SalsaNext
    from oracle import pmf_torch as O
    hip = deterministic_init(SalsaNext(5, NCLS, 32, softmax=False)).cuda().eval()
    ref = deterministic_init(O.SalsaNext(5, NCLS, 32, softmax=False)).eval()
    pcd, _, _, _ = synthetic_batch(2, 32, 64, NCLS, seed=1)
    with torch.no_grad():
        want = ref(pcd)
        got = hip(pcd.cuda())
    assert got.shape == want.shape == (2, NCLS, 32, 64)
    assert G.rel_err(got.cpu().numpy(), want.numpy()) < 1e-3


def test_epmf_engine_two_steps_at_39_classes():
    from pmf_amd.engine import EPMFEngine
    from pmf_amd.models import EPMFNet
    m = deterministic_init(EPMFNet(5, 3, NCLS, 32, imagenet_pretrained=False, image_backbone="resnet34")).cuda()
    alpha = np.linspace(0.2, 1.0, NCLS).astype(np.float32)
    alpha[0] = 0
    eng = EPMFEngine(m, NCLS, lr=1e-3, momentum=0.9, weight_decay=1e-5, alpha=alpha, warmup_steps=1, max_steps=10 ** 9)
    pcd, rgb, label, mask = synthetic_batch(2, 64, 128, NCLS, seed=1, fill=0.3)
    feat = torch.cat((pcd, rgb), 1).cuda()
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    losses = []
    for _ in range(2):
        total, t = eng.train_step(feat.clone(), torch.ones_like(mask).cuda(), label.cuda())
        losses.append(total.item())
        assert all(np.isfinite(v.item()) for v in t.values() if torch.is_tensor(v) and v.numel() == 1), t
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses), losses
    moved = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert any(k.startswith("lidar_stream.logits") for k in moved) and len(moved) > 0.9 * len(before), (len(moved), len(before))
