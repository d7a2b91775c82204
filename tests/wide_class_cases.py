"""CPU side of tests/test_gpu_wide_classes.py and tests/test_wide_classes_host.py: 33 to 64 classes (include/pmf_amd_wide.h).

The references, the float32 restatements and the derived bounds are the ones of tests/loss_pixel_cases.py (per-pixel stage),
tests/lovasz_cases.py (Lovasz stage) and tests/test_gpu_elementwise.py (softmax family): all three are written in terms of
C and hold at any class count.  This module adds the case lists at wide counts, the input builder of the Lovasz cases (the one
of lovasz_cases is tied to its own list), the softmax figures measured over the wide channel counts, and the recorded worst
ratios of the restatements on exactly these cases.  Nothing here touches the GPU or the built library."""
import functools
import math
import zlib

import numpy as np
import torch

from tests import loss_pixel_cases as PV
from tests import lovasz_cases as LV

NARROW, WIDE = 32, 64                      # class limit of pmf_amd.h's entry points, and of pmf_amd_wide.h's

# ------------------------------------------------------------------------------------------------ per-pixel stage
PIXEL_CASES = [
    PV._case("w33", 2, 33, 333, edges=True, par=1),
    PV._case("w39", 2, 39, 527, edges=True, par=0),
    PV._case("w40", 1, 40, 300, labels="absent", edges=False, par=2),
    PV._case("w64", 1, 64, 300, edges=True, par=1),
    PV._case("w64n3", 3, 64, 70, edges=False, par=0),
]
PIXEL_DICE_CASES = [
    PV._case("wd39", 1, 39, 17 * 256 - 3, edges=False, par=2),
    PV._case("wd64", 1, 64, 16 * 256, edges=False, par=0),
]
PIXEL_NAMES = [c["name"] for c in PIXEL_CASES]
PIXEL_DICE_NAMES = [c["name"] for c in PIXEL_DICE_CASES]
_PIXEL = {c["name"]: c for c in PIXEL_CASES + PIXEL_DICE_CASES}

# worst error / bound of the float32 restatement (loss_pixel_cases.core in float32) over PIXEL_CASES and PIXEL_DICE_CASES
# (pixel_measure()); tests/test_wide_classes_host.py holds these figures to what the helper returns
PIXEL_MEASURED = {
    "grad_foc": 0.17,
    "grad_per": 0.46,
    "grad_total": 0.46,
    "grad_dice": 0.47,
    "rows": 0.04,
}


@functools.lru_cache(None)
def pixel_inputs(name):
    return PV.make_inputs(_PIXEL[name])


@functools.lru_cache(None)
def pixel_ref(name):
    x = pixel_inputs(name)
    ref = PV.reference(x)
    ref["key"], ref["conf"] = PV.keys_of(x), PV.confusion_of(x)
    return ref


def pixel_measure(name):
    """loss_pixel_cases.measure on one of the cases above"""
    x, ref = pixel_inputs(name), pixel_ref(name)
    out = dict.fromkeys(PIXEL_MEASURED, 0.0)
    for spec, qty in PV.QUANTITY.items():
        if name in PIXEL_DICE_NAMES and spec != "dice":
            continue
        gl, gc, bl, bc = PV.grad_ref(x, ref, spec)
        rl, rc = PV.restate32(x, ref, spec)
        out[qty] = max(out[qty], PV.worst_ratio(rl, gl, bl, ref["cmp"]), PV.worst_ratio(rc, gc, bc, ref["cmp"]))
    out["rows"] = PV.worst_ratio(PV.rows_of(x, ref["K32"]), ref["rows"], ref["rows_bound"])
    return out


# ------------------------------------------------------------------------------------------------ Lovasz stage
LOVASZ_CASES = [
    LV._case("w33", 1, 8229, 33, 4097, "absent_single", ("special", "eighths")),
    LV._case("w39", 2, 4096, 39, 6000, "full", ("uniform", "saturated")),
    LV._case("w64", 1, 8229, 64, 8229, "full", ("eighths", "uniform")),
    LV._case("w64few", 3, 2743, 64, 40, "full", ("uniform", "equal")),
]
LOVASZ_NAMES = [c["name"] for c in LOVASZ_CASES]
_LOVASZ = {c["name"]: c for c in LOVASZ_CASES}

# worst error / bound of lovasz_cases.restate32 over LOVASZ_CASES, unweighted and with W6 (lovasz_measure())
LOVASZ_MEASURED = {
    "grad": 0.48,
    "row": 0.25,
    "out8": 0.78,
}


def lovasz_make(cs, seed_name=None):
    """lovasz_cases.inputs for a case of any list: key f32[2C][P], label, cnt, rows f64[nrows][4], the prefills of gl and gc"""
    N, HW, C, m = cs["N"], cs["HW"], cs["C"], cs["m"]
    P = N * HW
    rng = np.random.default_rng(zlib.crc32(("lovasz " + (seed_name or cs["name"])).encode()))
    label = LV.labels_of(P, C, m, cs["makeup"], rng)
    assert int((label != 0).sum()) == m
    key = np.empty((2 * C, P), dtype=np.float32)
    for r in range(2 * C):
        key[r] = LV.pattern(cs["pats"][r // C], P, rng, r)
    key[:, label == 0] = -1.0
    nrows = (P + 255) // 256
    return dict(cs, P=P, key=key, label=label, cnt=np.bincount(label, minlength=C).astype(np.int64),
                rows=rng.random((nrows, 4)) * 2 - 1, nrows=nrows,
                pre_gl=(rng.random((N, C, HW), dtype=np.float32) * 2 - 1), pre_gc=(rng.random((N, C, HW), dtype=np.float32) * 2 - 1))


@functools.lru_cache(None)
def lovasz_inputs(name):
    return lovasz_make(_LOVASZ[name])


def lovasz_reference(x, weighted):
    return LV.reference(x["key"], x["label"], x["N"], x["HW"], x["C"], x["rows"], x["pre_gl"], x["pre_gc"],
                        w6=LV.W6 if weighted else None)


@functools.lru_cache(None)
def lovasz_ref(name, weighted):
    return lovasz_reference(lovasz_inputs(name), weighted)


def lovasz_measure(name):
    worst = dict.fromkeys(LOVASZ_MEASURED, 0.0)
    for weighted in (False, True):
        x, ref = lovasz_inputs(name), lovasz_ref(name, weighted)
        rt = LV.ratios(LV.restate32(x, ref, weighted), ref)
        worst = {k: max(worst[k], rt[k]) for k in worst}
    return worst


# ------------------------------------------------------------------------------------------------ softmax family
SM_C = [33, 39, 40, 63, 64]
SM_HW = {80.0: (1, 7, 45, 300), 100.0: (7, 45)}       # (test_gpu_elementwise.SM_HW)
SM_NB = 3                                             # (test_gpu_elementwise.NB)
# what measure_softmax_units(span) returns on the CPU: float32 torch against float64, worst element in units of eps32 * mag,
# over SM_C and the inputs of test_gpu_elementwise.softmax_case
# (three decimals: 4 x 33.7515 lies just above 135, and the rule rounds up -- K = 136, 8 at span 80 and 135, 5 at span 100)
SM_MEASURED = {
    "softmax": {80.0: 33.752, 100.0: 33.518},
    "softmax_bwd": {80.0: 1.968, 100.0: 1.236},
}
# the project's rule (tests/test_gpu_elementwise.py K): 4 x the measured error, rounded up
SM_K = {kind: {span: math.ceil(4 * u) for span, u in by_span.items()} for kind, by_span in SM_MEASURED.items()}


def measure_softmax_units(span):
    """test_gpu_elementwise.measure_softmax_units over the wide channel counts"""
    from tests import test_gpu_elementwise as E
    assert E.SM_HW == SM_HW and E.NB == SM_NB
    worst = [0.0, 0.0]
    for C in SM_C:
        for HW in SM_HW[span]:
            x, go = E.softmax_case(SM_NB, HW, C, span)
            p64, p32 = torch.softmax(x.double(), 2), torch.softmax(x, 2)
            u = ((p32.double() - p64).abs() - E.TINY).clamp_min(0) / (E.EPS * p64)
            worst[0] = max(worst[0], u.max().item())
            p32 = p32.permute(0, 2, 1).contiguous()
            r32 = p32 * (go - (p32 * go).sum(1, keepdim=True))
            pd, gd = p32.double(), go.double()
            ref = pd * (gd - (pd * gd).sum(1, keepdim=True))
            mag = pd * (gd.abs() + (pd * gd.abs()).sum(1, keepdim=True))
            worst[1] = max(worst[1], (((r32.double() - ref).abs() - E.TINY).clamp_min(0) / (E.EPS * mag).clamp_min(1e-300)).max().item())
    return worst
