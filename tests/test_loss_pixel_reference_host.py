"""The reference and the derived bounds of tests/test_gpu_loss_pixel.py, on the host (no GPU, no built library).

(a) the closed-form float64 reference of the per-pixel stage (tests/loss_pixel_cases.py core / combine / dice_ref) against
    float64 autograd through the project's own modules -- FocalSoftmaxLoss, perception_aware_loss, ExpLogDiceLoss and
    epmf_total_loss (which fixes the order of w6) -- term by term, value and gradient, on every case; edge pixels with a 0 or
    a value exactly on a clamp are left out there (the modules' thresholds are doubles and ln 0 is -inf), and the batch
    without a labelled pixel has no focal term to compare (the modules give NaN);
(b) the kernel's float32 arithmetic, restated on the host, stays inside the derived bounds on every GPU case, and the recorded
    worst ratios (MEASURED) are what the helper returns;
(c) the caps: at most 5 % of a case's pixels are left out for sitting within the derived error of a gate, at least 10 % stay in
    each open-gate state, float32 flips no gate outside the margins, and every hand-made pixel inside a margin has d = 0
    exactly, in float32 and in float64;
(d) the bounds are not vacuous: each of ten deliberately wrong variants of the reference exceeds them on at least one case."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd.loss.dice_loss import ExpLogDiceLoss  # noqa: E402
from pmf_amd.loss.focal_softmax import FocalSoftmaxLoss  # noqa: E402
from pmf_amd.loss.multi_task_loss import MultiTaskLoss  # noqa: E402
from pmf_amd.loss.perception import EPMF_TERMS, epmf_total_loss, perception_aware_loss  # noqa: E402
from tests import loss_pixel_cases as V  # noqa: E402

TOL = 0.02                # another summation order of the CPU library's float64 sums may move a ratio in its last digits
SIGMA = [0.5, 1.0, 2.0, 0.25, 4.0, 0.125]                    # powers of two: 1 / (2 sigma^2) is exact in float32


def close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    mag = max(float(np.abs(want).max()), 1e-300) if want.size else 1.0
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) if want.size else 0.0
    assert err <= 1e-11 * mag, "%s: %.3g off, magnitude %.3g" % (what, err, mag)


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_closed_form_is_autograd_of_the_modules(name):
    cs = V._ALL[name]
    x = V.make_inputs(cs, safe_only=True)
    N, C, HW = x["N"], x["C"], x["HW"]
    K = V.core(x, np.float64, clamps=(1e-8, 1e-6))             # (the modules clamp at the doubles, the kernel at their float32 roundings)
    dice = V.dice_ref(x)
    p = torch.from_numpy(x["p"]).double().view(N, C, HW, 1).requires_grad_(True)
    q = torch.from_numpy(x["q"]).double().view(N, C, HW, 1).requires_grad_(True)
    lab = torch.from_numpy(x["label"]).view(N, HW, 1)
    mask = lab.gt(0)

    def grads(v):
        g = torch.autograd.grad(v, (p, q), retain_graph=True, allow_unused=True)
        return [V.to_pix(np.zeros((N, C, HW)) if t is None else t.numpy(), x) for t in g]

    for h, prob in enumerate((p, q)):                         # the Dice term, every case
        v = ExpLogDiceLoss()(prob, lab, mask=mask)
        close(dice["dice"][h, 0], v.item(), "dice value")
        want = grads(v)
        got = V.combine(x, K, (0, 0, 0, 0, 0, 0), dice["dice"])
        close(got[h], want[h], "dice gradient")
        assert not want[1 - h].any()
    if x["exact"].any():
        return
    tau = float(np.float32(x["tau"]))
    focal = FocalSoftmaxLoss(C, gamma=x["fg"], alpha=torch.from_numpy(x["alpha"]), softmax=False)
    mt = MultiTaskLoss(6, sigma=SIGMA)
    total, t = epmf_total_loss(p, q, lab, focal, lambda prob, _l: prob.sum() * 0, mt, tau=tau)
    w = (1.0 / (2.0 * mt.sigma.detach() ** 2)).numpy()
    w6 = tuple(float(w[EPMF_TERMS.index(k)]) for k in ("foc", "lov", "foc_cam", "lov_cam", "per", "per_img"))
    assert len(set(w6)) == 6 and all(float(np.float32(v)) == v for v in w6)
    rows = V.rows_of(x, K).sum(0)
    terms = {"per": ("per_p", 2), "per_img": ("per_q", 3)}
    if name != "allunlab":
        terms.update({"foc": ("foc", 0), "foc_cam": ("foc_cam", 1)})
    else:
        assert torch.isnan(t["foc"]) and rows[0] == 0 and rows[1] == 0          # the pinned deviation
    for k, (spec, col) in terms.items():
        close(rows[col], t[k].item(), k + " value")
        got, want = V.combine(x, K, V.UNIT[spec]), grads(t[k])
        close(got[0], want[0], k + " gradient (lidar)")
        close(got[1], want[1], k + " gradient (camera)")
    both = perception_aware_loss(p, q, tau)[0]
    close(rows[2] + rows[3], both.item(), "per value")
    if name != "allunlab":
        got, want = V.combine(x, K, w6), grads(total)
        close(got[0], want[0], "weighted total (lidar): the order of w6")
        close(got[1], want[1], "weighted total (camera): the order of w6")


def test_reference_by_hand():
    """two classes, two pixels: keys, confusion (first maximum wins, label 0 counted), histogram"""
    x = {"N": 1, "C": 2, "HW": 3, "P": 3, "pp": np.array([[0.5, 0.5], [0.25, 0.75], [1, 0]], dtype=np.float32),
         "qq": np.array([[0.125, 0.875], [0.5, 0.5], [0, 1]], dtype=np.float32), "label": np.array([1, 0, 1])}
    assert np.array_equal(V.keys_of(x), np.array([[0.5, -1, 1], [0.5, -1, 1], [0.125, -1, 0], [0.125, -1, 0]], dtype=np.float32))
    assert np.array_equal(V.confusion_of(x), [[[0, 2], [1, 0]], [[1, 0], [0, 2]]])
    assert np.array_equal(V.histogram(np.array([1, 0, 1, -1, 2, 255]), 2), [1, 2])


@functools.lru_cache(None)
def measured(name):
    return V.measure(name)


@pytest.mark.parametrize("name", V.CASE_NAMES + V.DICE_NAMES)
def test_restated_kernel_arithmetic_stays_inside_the_bounds(name):
    m = measured(name)
    print("%s: restate32 worst err / bound: %s" % (name, ", ".join("%s %.3f" % kv for kv in m.items())))
    for k, v in m.items():
        assert v < 1.0 and v <= V.MEASURED[k] + TOL, k


def test_recorded_ratios_are_the_measured_ones():
    worst = {k: max(measured(n)[k] for n in V.CASE_NAMES + V.DICE_NAMES) for k in V.MEASURED}
    print("measured", worst, "recorded", V.MEASURED)
    for k, v in worst.items():
        assert abs(v - V.MEASURED[k]) <= TOL and V.MEASURED[k] < 1.0, k


@pytest.mark.parametrize("name", V.CASE_NAMES + V.DICE_NAMES)
def test_exclusion_caps_and_gate_states(name):
    x, ref = V.inputs(name), V.case_ref(name)
    K, K32 = ref["K"], ref["K32"]
    assert ref["left_out"].mean() <= 0.05
    if name != "p1":                                          # (the one exemption: a single pixel has one gate state)
        assert (K["gp"] & ref["cmp"]).mean() >= 0.10 and (K["gq"] & ref["cmp"]).mean() >= 0.10
    flips = (ref["own_gates"][0] != K32["gp"]) | (ref["own_gates"][1] != K32["gq"])
    assert not (flips & ~ref["margin"]).any(), "float32 flips a gate outside the derived margins"
    on_branch = ref["margin"] & x["edge"]
    assert (ref["d_own"][on_branch] == 0).all() and (K32["d"][on_branch] == 0).all()
    if x["edges"]:
        assert on_branch.sum() >= 3
        assert (K["gp"] & x["edge"]).any() and (K["gq"] & x["edge"]).any()


@pytest.mark.parametrize("mut", V.MUTANTS)
def test_bounds_notice_a_wrong_formula(mut):
    r = {n: V.mutant_ratio(n, mut) for n in V.CASE_NAMES}
    print("%s: caught on %d of %d cases, worst %.3g x the bound" % (mut, sum(v > 1 for v in r.values()), len(r), max(r.values())))
    assert max(r.values()) > 1.0


def test_case_lists_cover_what_they_claim():
    shapes = {(c["N"], c["C"], c["HW"]) for c in V.CASES}
    assert {(1, 2, 77), (2, 5, 333), (3, 14, 527), (2, 20, 1031), (1, 32, 300)} <= shapes
    assert {1, 255, 256, 257} <= {c["N"] * c["HW"] for c in V.CASES}
    assert any(c["N"] > 1 and c["C"] == C and c["HW"] % 64 for c in V.CASES for C in (2,)) and any(
        c["N"] > 1 and c["C"] == 32 and c["HW"] % 64 for c in V.CASES)
    assert {V.inputs(n)["nrows"] for n in V.DICE_NAMES} == set(V.DICE_NPARTS)
    assert {(c["C"]) for c in V.DICE_CASES} == set(V.DICE_C) and len(V.DICE_CASES) == len(V.DICE_NPARTS) * len(V.DICE_C)
    assert sum(c["edges"] for c in V.CASES) >= 2
    assert {p[0] for p in V.PARAMS} == {2.0, 1.0, 1.5} and {p[1] for p in V.PARAMS} == {0.7, 0.3}
    assert all(p[2] != 0.5 for p in V.PARAMS) and {c["par"] for c in V.CASES} == {0, 1, 2}
    x = {n: V.inputs(n) for n in V.CASE_NAMES}
    cnt = {n: V.histogram(v["label"], v["C"]) for n, v in x.items()}
    assert any((c[1:] == 0).any() and c[1:].any() for c in cnt.values())              # a class absent
    assert any(c[0] == 0 for c in cnt.values()) and any(c[0] == c.sum() for c in cnt.values())
    assert all(cnt["dicezero"] > 0) and all(V.case_ref("dicezero")["dice"]["below"])
    # the edge pixels: 0, 1, both neighbours of both clamps and the clamps themselves, in both heads; ties; identical heads
    for C in (2, 5):
        e = V.edge_pixels(C)
        for head in (0, 1):
            vals = np.concatenate([r[head] for r in e])
            assert all((vals == s).any() for s in V.SPECIALS) and (vals == 1).any()
            assert any((r[head] == r[head].max()).sum() == 2 for r in e)
        assert any(np.array_equal(r[0], r[1]) for r in e) and {r[2] for r in e} == {0, 1}
    assert float(V.SPECIALS[1]) < float(V.T8) < float(V.SPECIALS[3]) and float(V.SPECIALS[4]) < float(V.T6) < float(V.SPECIALS[6])
    assert V.W6[4] != V.W6[5] and all(float(np.float32(w)) == w for w in V.W6 + V.W6_OTHER_LOV)
    assert V.COUNT_CASE["N"] * V.COUNT_CASE["HW"] == 2048 * 1024 + 2049 and V.COUNT_CASE["C"] == 2
