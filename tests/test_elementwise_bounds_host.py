"""The measured entries of the K table of tests/test_gpu_elementwise.py, on the host (no GPU, no built library).

The bounds of the sigmoid and softmax kernels are 4 x the error of the float32 torch-CPU evaluation of the same formula
against float64.  The measuring helpers share the input builders and the view arithmetic of the GPU tests; this test runs
them and holds the recorded figures to what they return, so that neither can drift away from the other unnoticed."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_elementwise as E  # noqa: E402

# expf, the division and the summation order of another libm or another vector width may differ in the last place of a
# result: one unit of eps32 * mag.  The figures themselves are recorded to two decimals.
LIBM = 1.0


def _check(name, measured, recorded, k):
    print("%s: measured %.4f recorded %.2f K %d" % (name, measured, recorded, k))
    assert abs(measured - recorded) <= LIBM, "%s: measured %.3f, the table records %.2f" % (name, measured, recorded)
    assert k == math.ceil(4 * recorded)


def test_gate_bounds_are_four_times_the_measured_error():
    fwd, bwd = E.measure_gate_units()
    _check("fusion_gate", fwd, E.MEASURED["fusion_gate"], E.K["fusion_gate"])
    _check("fusion_gate_bwd", bwd, E.MEASURED["fusion_gate_bwd"], E.K["fusion_gate_bwd"])


@pytest.mark.parametrize("span", sorted(E.MEASURED["softmax"]))
def test_softmax_bounds_are_four_times_the_measured_error(span):
    fwd, bwd = E.measure_softmax_units(span)
    _check("softmax", fwd, E.MEASURED["softmax"][span], E.K["softmax"][span])
    _check("softmax_bwd", bwd, E.MEASURED["softmax_bwd"][span], E.K["softmax_bwd"][span])
