"""33 to 64 classes (include/pmf_amd_wide.h) without a GPU: the third header of the binding, the guards of its entry points
(all of which answer before the first HIP call), the plans of PMFNet / EPMFNet at 39, 64 and 65 classes, and the references of
tests/test_gpu_wide_classes.py -- the per-pixel stage, the Lovasz stage and the softmax bounds at wide class counts
(tests/wide_class_cases.py).  Needs the built libpmf_amd.so, as tests/test_plan_guards_host.py does."""
import ctypes as C
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.loss import FocalSoftmaxLoss  # noqa: E402
from pmf_amd.loss.perception import pmf_total_loss  # noqa: E402
from pmf_amd.models import EPMFNet, PMFNet  # noqa: E402
from tests import loss_pixel_cases as PV  # noqa: E402
from tests import wide_class_cases as W  # noqa: E402

CPU = torch.device("cpu")
TOL = 0.02                # (tests/test_loss_pixel_reference_host.py: another summation order of the CPU library's float64 sums)
LIBM = 1.0                # (tests/test_elementwise_bounds_host.py: one unit of eps32 * mag between two libms)
PTR = 0x7F0000001000      # never dereferenced: every call that takes it is refused by its guard


# ================================================================================================ 1. binding
def test_third_header_is_read_strictly_and_bound():
    path = os.path.join(ROOT, "include", "pmf_amd_wide.h")
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    found = re.findall(r"\b(pmf_\w+)\s*\(([^()]*)\)\s*;", text)
    assert [n for n, _ in found] == L.EXPORTS_WIDE == [
        "pmf_wide_max_classes", "pmf_softmax_wide", "pmf_softmax_wide_bwd", "pmf_loss_pixel_wide", "pmf_loss_lovasz_sort_wide",
        "pmf_loss_dice_finish_wide"]
    assert not set(L.EXPORTS_WIDE) & set(L.EXPORTS) and not set(L.EXPORTS_WIDE) & set(L.EXPORTS_SENSAT)
    h = L.read_header(open(path).read(), base=L._H)
    assert list(h.protos) == L.EXPORTS_WIDE and not h.structs and not h.consts
    with pytest.raises(L.PMFLibraryError) as e:       # alone the header does not know pmf_stream_t
        L.read_header(open(path).read())
    assert "pmf_stream_t" in str(e.value)
    lib = L.lib()
    for name, params in found:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32, name
        assert fn.argtypes == h.protos[name][1], name
        assert len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    v, i32, i64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert lib.pmf_softmax_wide.argtypes == [v, i32, i32, i32, i32, i32, v, v]
    assert lib.pmf_softmax_wide_bwd.argtypes == [v, v, i32, i32, i32, i32, v, i32, v]
    # pmf_loss_pixel_dice's list plus w6; pmf_loss_lovasz_sort's plus w6
    assert lib.pmf_loss_pixel_wide.argtypes == lib.pmf_loss_pixel_dice.argtypes[:-1] + [v, v]
    assert lib.pmf_loss_pixel_wide.argtypes[4:10] == [i32, i32, i64, f, f, f]
    assert lib.pmf_loss_lovasz_sort_wide.argtypes == lib.pmf_loss_lovasz_sort.argtypes[:-1] + [v, v]
    assert lib.pmf_loss_dice_finish_wide.argtypes == lib.pmf_loss_dice_finish.argtypes
    assert lib.pmf_wide_max_classes() == L.WIDE_CLASSES == W.WIDE == 64 and L.NARROW_CLASSES == W.NARROW == 32


def test_missing_third_header_is_reported():
    with pytest.raises(L.PMFLibraryError) as e:
        L._read(os.path.join(ROOT, "include", "no_such_wide.h"), {}, L._H)
    assert "no_such_wide.h not found" in str(e.value)


# ================================================================================================ 2. guards without a device
def _pixel(lib, C_=39, N=1, HW=77, head=None, tail=None, parts=None, dice=None, w6=None):
    head = [PTR] * 4 if head is None else head               # lidar_prob, camera_prob, label, alpha
    tail = [PTR] * 7 if tail is None else tail               # cnt, grad_lidar, grad_camera, key, rows, conf_lidar, conf_camera
    return lib.pmf_loss_pixel_wide(*head, N, C_, HW, 2.0, 0.7, 0.5, *tail, parts, dice, w6, None)


def test_wide_entry_points_refuse_bad_arguments_before_any_hip_call():
    lib = L.lib()
    A, U = L.PMF_E_ARG, L.PMF_E_UNSUPPORTED
    # the softmax pair: C outside [1, 64] (ldc beyond 64 in the backward) is PMF_E_UNSUPPORTED, as in pmf_amd.h
    assert lib.pmf_softmax_wide(PTR, 72, 1, 4, 65, 0, PTR, None) == U
    assert lib.pmf_softmax_wide(PTR, 72, 1, 4, 65, 1, PTR, None) == U
    assert lib.pmf_softmax_wide(PTR, 8, 1, 4, 0, 0, PTR, None) == U
    assert lib.pmf_softmax_wide_bwd(PTR, PTR, 1, 4, 65, 0, PTR, 72, None) == U
    assert lib.pmf_softmax_wide_bwd(None, PTR, 1, 4, 65, 1, PTR, 72, None) == U
    assert lib.pmf_softmax_wide_bwd(PTR, PTR, 1, 4, 39, 0, PTR, 72, None) == U
    assert lib.pmf_softmax_wide_bwd(PTR, PTR, 1, 4, 20, 0, PTR, 72, None) == U
    # the per-pixel stage, in its three forms
    forms = [dict(), dict(w6=PTR), dict(parts=PTR, dice=PTR)]
    for kw in forms:
        for c in (65, 1, 0, -3, 1 << 20):
            assert _pixel(lib, C_=c, **kw) == A, (c, kw)
        for N, HW in ((0, 77), (-1, 77), (1, 0), (1, -3)):
            assert _pixel(lib, N=N, HW=HW, **kw) == A, (N, HW, kw)
        for i in range(4):
            h = [PTR] * 4
            h[i] = None
            assert _pixel(lib, head=h, **kw) == A, ("head", i, kw)
        for i in range(5):
            t = [PTR] * 7
            t[i] = None
            assert _pixel(lib, tail=t, **kw) == A, ("tail", i, kw)
        for i in (5, 6):                                       # a lone confusion matrix
            t = [PTR] * 7
            t[i] = None
            assert _pixel(lib, tail=t, **kw) == A, ("conf", i, kw)
        assert _pixel(lib, HW=1 << 40, **kw) == U, kw           # more blocks of 256 pixels than a grid dimension holds
        for c in (2, 20, 32, 33, 64):                          # ... and that is the class count's doing in no case
            assert _pixel(lib, C_=c, head=[None] * 4, **kw) == A
    assert _pixel(lib, parts=PTR, dice=PTR, w6=PTR) == A        # w6 together with dice
    assert _pixel(lib, parts=PTR) == A and _pixel(lib, dice=PTR) == A and _pixel(lib, dice=PTR, w6=PTR) == A
    # the Lovasz stage
    def lov(c=39, N=1, HW=77, ws=PTR, w6=None):
        return lib.pmf_loss_lovasz_sort_wide(PTR, PTR, N, c, HW, PTR, 0.75, 0.375, ws, PTR, PTR, PTR, PTR, PTR, PTR, w6, None)
    for w6 in (None, PTR):
        for c in (65, 1, 0, -1):
            assert lov(c=c, w6=w6) == A
        assert lov(N=0, w6=w6) == A and lov(HW=0, w6=w6) == A and lov(ws=None, w6=w6) == A
        assert lov(HW=(1 << 24) + 1, w6=w6) == U and lov(N=3, HW=1 << 23, w6=w6) == U
    # the Dice finish
    fin = lib.pmf_loss_dice_finish_wide
    assert fin(PTR, 65, PTR, None) == A and fin(PTR, 1, PTR, None) == A
    assert fin(None, 39, PTR, None) == A and fin(PTR, 39, None, None) == A
    # pmf_amd.h's own entry points keep their limit
    assert lib.pmf_loss_dice_finish(PTR, 33, PTR, None) == A
    assert lib.pmf_softmax_nhwc_to_nchw(PTR, 40, 1, 4, 33, PTR, None) == U


# ================================================================================================ 3. plans
@pytest.mark.parametrize("net", [PMFNet, EPMFNet])
@pytest.mark.parametrize("nclasses", [39, 64])
def test_plans_build_at_wide_class_counts(net, nclasses):
    m = net(nclasses=nclasses, imagenet_pretrained=False)
    for training in (True, False):
        P = m.train(training)._build(2, 32, 64, training, CPU)
        kinds = [L.OP_NAMES[k] for k in P.fwd_kinds]
        assert kinds.count("OP_SOFTMAX") == 2
        if training:
            assert [L.OP_NAMES[k] for k in P.bwd_kinds].count("OP_SOFTMAX_BWD") == 2
        assert all(s["shape"] == (2, nclasses, 32, 64) for s in P.out_slots.values())


@pytest.mark.parametrize("net", [PMFNet, EPMFNet])
def test_plan_refuses_65_classes_when_it_is_built(net):
    m = net(nclasses=65, imagenet_pretrained=False)
    for training in (True, False):
        with pytest.raises(ValueError) as e:
            m.train(training)._build(2, 32, 64, training, CPU)
        assert "65 classes" in str(e.value) and "64" in str(e.value)


def test_fused_objective_names_the_limit():
    from pmf_amd.loss import fused
    assert fused._wide(32) is False and fused._wide(33) is True and fused._wide(64) is True
    with pytest.raises(ValueError) as e:
        fused._wide(65)
    assert "65 classes" in str(e.value) and "64" in str(e.value)


# ================================================================================================ 4. per-pixel stage
@functools.lru_cache(None)
def pixel_measured(name):
    return W.pixel_measure(name)


def test_pixel_cases_are_the_listed_ones():
    shapes = [(c["name"], c["N"], c["C"], c["HW"], c["labels"], c["edges"], c["par"]) for c in W.PIXEL_CASES + W.PIXEL_DICE_CASES]
    assert shapes == [("w33", 2, 33, 333, "mixed", True, 1), ("w39", 2, 39, 527, "mixed", True, 0),
                      ("w40", 1, 40, 300, "absent", False, 2), ("w64", 1, 64, 300, "mixed", True, 1),
                      ("w64n3", 3, 64, 70, "mixed", False, 0), ("wd39", 1, 39, 17 * 256 - 3, "mixed", False, 2),
                      ("wd64", 1, 64, 16 * 256, "mixed", False, 0)]
    assert W.pixel_inputs("wd39")["nrows"] == 17 and W.pixel_inputs("wd64")["nrows"] == 16
    cnt = PV.histogram(W.pixel_inputs("w40")["label"], 40)
    assert cnt[39] == 0 and cnt[1:39].all()                   # "absent": the last class does not occur


@pytest.mark.parametrize("name", W.PIXEL_NAMES + W.PIXEL_DICE_NAMES)
def test_pixel_exclusion_caps_and_gate_states(name):
    x, ref = W.pixel_inputs(name), W.pixel_ref(name)
    K, K32 = ref["K"], ref["K32"]
    gp, gq = (K["gp"] & ref["cmp"]).mean(), (K["gq"] & ref["cmp"]).mean()
    print("%s: left out %.4f, gate_p open %.3f, gate_q open %.3f" % (name, ref["left_out"].mean(), gp, gq))
    assert ref["left_out"].mean() <= 0.05
    assert gp >= 0.10 and gq >= 0.10
    flips = (ref["own_gates"][0] != K32["gp"]) | (ref["own_gates"][1] != K32["gq"])
    assert not (flips & ~ref["margin"]).any(), "float32 flips a gate outside the derived margins"
    on_branch = ref["margin"] & x["edge"]
    assert (ref["d_own"][on_branch] == 0).all() and (K32["d"][on_branch] == 0).all()


@pytest.mark.parametrize("name", W.PIXEL_NAMES + W.PIXEL_DICE_NAMES)
def test_pixel_restatement_stays_inside_the_bounds(name):
    m = pixel_measured(name)
    print("%s: restate32 worst err / bound: %s" % (name, ", ".join("%s %.3f" % kv for kv in m.items())))
    for k, v in m.items():
        assert v <= 1.0 and v <= W.PIXEL_MEASURED[k] + TOL, k


def test_pixel_recorded_ratios_are_the_measured_ones():
    worst = {k: max(pixel_measured(n)[k] for n in W.PIXEL_NAMES + W.PIXEL_DICE_NAMES) for k in W.PIXEL_MEASURED}
    print("measured", worst, "recorded", W.PIXEL_MEASURED)
    for k, v in worst.items():
        assert abs(v - W.PIXEL_MEASURED[k]) <= TOL and W.PIXEL_MEASURED[k] <= 1.0, k


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    mag = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    assert err <= 1e-11 * mag, "%s: %.3g off, magnitude %.3g" % (what, err, mag)


def test_closed_form_at_39_classes_is_autograd_of_pmf_total_loss():
    """w39 without the edge pixels that sit on a clamp: float64 autograd through pmf_total_loss (the Lovasz term switched off:
    it belongs to the other stage) gives the closed form's values and its unweighted gradient"""
    x = PV.make_inputs(W._PIXEL["w39"], safe_only=True)
    assert not x["exact"].any()
    N, C_, HW = x["N"], x["C"], x["HW"]
    K = PV.core(x, np.float64, clamps=(1e-8, 1e-6))           # (the modules clamp at the doubles)
    p = torch.from_numpy(x["p"]).double().view(N, C_, HW, 1).requires_grad_(True)
    q = torch.from_numpy(x["q"]).double().view(N, C_, HW, 1).requires_grad_(True)
    lab = torch.from_numpy(x["label"]).view(N, HW, 1)
    focal = FocalSoftmaxLoss(C_, gamma=x["fg"], alpha=torch.from_numpy(x["alpha"]), softmax=False)
    total, t = pmf_total_loss(p, q, lab, focal, lambda prob, _l: prob.sum() * 0, lambda_=1.0, gamma_=x["gper"],
                              tau=float(np.float32(x["tau"])))
    rows = PV.rows_of(x, K).sum(0)
    _close(rows[0], t["foc"].item(), "foc")
    _close(rows[1], t["foc_cam"].item(), "foc_cam")
    _close(rows[2] + rows[3], t["per"].item(), "per")
    _close(rows[0] + rows[1] + x["gper"] * (rows[2] + rows[3]), total.item(), "total")
    g = torch.autograd.grad(total, (p, q))
    got = PV.combine(x, K, None)
    _close(got[0], PV.to_pix(g[0].numpy(), x), "gradient (lidar)")
    _close(got[1], PV.to_pix(g[1].numpy(), x), "gradient (camera)")


# ================================================================================================ 5. Lovasz stage
@functools.lru_cache(None)
def lovasz_measured(name):
    return W.lovasz_measure(name)


def test_lovasz_cases_are_the_listed_ones():
    got = [(c["name"], c["N"], c["HW"], c["C"], c["m"], c["makeup"], c["pats"]) for c in W.LOVASZ_CASES]
    assert got == [("w33", 1, 8229, 33, 4097, "absent_single", ("special", "eighths")),
                   ("w39", 2, 4096, 39, 6000, "full", ("uniform", "saturated")),
                   ("w64", 1, 8229, 64, 8229, "full", ("eighths", "uniform")),
                   ("w64few", 3, 2743, 64, 40, "full", ("uniform", "equal"))]
    x = W.lovasz_inputs("w33")
    assert x["cnt"][1] == 1 and x["cnt"][32] == 0 and x["cnt"][2:32].all()
    assert (W.lovasz_inputs("w64few")["cnt"][1:] > 0).sum() == 40          # fewer labelled pixels than classes
    assert (W.lovasz_inputs("w64")["cnt"][1:] > 0).all() and W.lovasz_inputs("w64")["cnt"][0] == 0


@pytest.mark.parametrize("name", W.LOVASZ_NAMES)
def test_lovasz_restatement_stays_inside_the_bounds(name):
    m = lovasz_measured(name)
    print("%s: restate32 worst err / bound: %s" % (name, ", ".join("%s %.3f" % kv for kv in m.items())))
    for k, v in m.items():
        assert v < 1.0 and v <= W.LOVASZ_MEASURED[k] + TOL, k


def test_lovasz_recorded_ratios_are_the_measured_ones():
    worst = {k: max(lovasz_measured(n)[k] for n in W.LOVASZ_NAMES) for k in W.LOVASZ_MEASURED}
    print("measured", worst, "recorded", W.LOVASZ_MEASURED)
    for k, v in worst.items():
        assert abs(v - W.LOVASZ_MEASURED[k]) <= TOL and W.LOVASZ_MEASURED[k] < 1.0, k


# ================================================================================================ 6. softmax bounds
@pytest.mark.parametrize("span", sorted(W.SM_MEASURED["softmax"]))
def test_softmax_bounds_are_four_times_the_measured_error(span):
    fwd, bwd = W.measure_softmax_units(span)
    for name, measured in (("softmax", fwd), ("softmax_bwd", bwd)):
        recorded, k = W.SM_MEASURED[name][span], W.SM_K[name][span]
        print("%s span %g: measured %.4f recorded %.3f K %d" % (name, span, measured, recorded, k))
        assert abs(measured - recorded) <= LIBM, "%s: measured %.3f, the table records %.3f" % (name, measured, recorded)
        assert k == math.ceil(4 * recorded)
    assert W.SM_C == [33, 39, 40, 63, 64]
    assert W.SM_K == {"softmax": {80.0: 136, 100.0: 135}, "softmax_bwd": {80.0: 8, 100.0: 5}}
