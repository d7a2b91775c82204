"""The references and the measured bounds of tests/test_gpu_bn.py, on the host (no GPU, no built library).

(a) the float64 reference of the BatchNorm backward (tests/bn_cases.py: written from the definition) against float64 autograd
    through torch's batch_norm, to 1e-12 * mag: what the GPU tests compare the kernels with IS BatchNorm;
(b) the kernels' coefficient form, restated in float32 torch, stays within a quarter of the K the GPU tests allow, over the
    inputs of every GPU backward case: the bound has room, and a kernel that misses it is wrong, not unlucky;
(c) the bound of the chain test (finalize -> backward from raw activations) is 4 x what torch's own float32 CPU batch_norm
    loses against float64 on the same inputs.
The recorded figures (bn_cases.MEASURED) are held to what the measuring helpers return, within one unit."""
import functools
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bn_cases as B  # noqa: E402
from tests.test_gpu_elementwise import close, gen, rnd  # noqa: E402

L = B.L
UNIT = 1.0                # another vector width or summation order of the CPU library may move a figure by one unit


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("npix", [1, 2, 7, 513])
def test_reference_is_batchnorm(npix, C, act, train):
    x = B.bn_inputs(npix, C, act, B.case_seed(npix, C, act))
    z = x["z"].double().requires_grad_(True)
    gamma = x["gamma"].double().requires_grad_(True)
    beta = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    gy = x["gy"].double()
    a = B.act_fwd(z, act)
    if train:
        y, mean, invstd = torch.native_batch_norm(a, gamma, beta, None, None, True, 0.1, B.BN_EPS)
    else:
        g = gen(5)
        mean, rv = rnd(g, C).double() * 8, torch.rand(C, generator=g).double() * 4 + 0.05
        invstd = 1 / (rv + B.BN_EPS).sqrt()
        y = torch.native_batch_norm(a, gamma, beta, mean, rv, False, 0.1, B.BN_EPS)[0]
    (y * gy).sum().backward()
    ref = B.bn_bwd_ref(a.detach(), gy, gamma.detach(), mean.detach(), invstd.detach(), act, train)
    what = "npix=%d C=%d act=%d train=%d " % (npix, C, act, train)
    eps32_units = 1e-12 / B.EPS                               # close() counts in eps32
    close(ref["dz"], z.grad, ref["mag_dz"], eps32_units, what + "dz")
    close(ref["dgamma"], gamma.grad, ref["mag_dgamma"], eps32_units, what + "dgamma")
    close(ref["dbeta"], beta.grad, ref["mag_dbeta"], eps32_units, what + "dbeta")
    close(ref["dbias"], z.grad.sum(0), ref["mag_dbias"], eps32_units, what + "dbias")


@functools.lru_cache(None)
def restate_units(C):
    return B.measure_restate_units([C])


@pytest.mark.parametrize("C", B.BWD_C)
def test_coefficient_form_has_room_under_the_bound(C):
    """restate32 against the reference, over the inputs of every GPU backward case at C: within K/4"""
    u = restate_units(C)
    print("restate32 at C=%d: %.4f units, K %d" % (C, u, B.K["dz"]))
    assert u <= B.K["dz"] / 4
    assert u <= B.MEASURED["restate"] + UNIT


def test_restate_figure_is_the_recorded_one():
    u = max(restate_units(C) for C in B.BWD_C)
    print("restate32: measured %.4f recorded %.2f" % (u, B.MEASURED["restate"]))
    assert abs(u - B.MEASURED["restate"]) <= UNIT
    assert B.MEASURED["restate"] <= B.K["dz"] / 4


def test_chain_bound_is_four_times_the_measured_error():
    u = B.measure_chain_units()
    print("chain: measured %.4f recorded %.2f K %d" % (u, B.MEASURED["chain"], B.K["chain"]))
    assert abs(u - B.MEASURED["chain"]) <= UNIT
    assert B.K["chain"] == math.ceil(4 * B.MEASURED["chain"])


def test_case_lists_cover_what_they_claim():
    assert {c[1:] for C in B.BWD_C for c in B.reduce_cases(C) if c[0] == B.col_npix_host(C)[2]} == set(B.COMBOS)
    assert {c[1:] for C in B.BWD_C for c in B.small_cases(C) if c[0] > 513} == set(B.COMBOS)
    assert B.R_DZ == 13 and B.K["dz"] == 26


def test_finalize_reference_is_batchnorm():
    """finalize_ref over the partial rows of a map against torch's float64 batch_norm statistics and running updates"""
    for npix, nrows in ((7, 1), (1000, 257)):
        x = B.finalize_inputs(npix, 5, 3)
        ref = B.finalize_ref(B.stat_rows(x["x"], nrows), npix, x["gamma"], x["beta"], x["rm"], x["rv"], 0.1, B.BN_EPS)
        rm, rv = x["rm"].double(), x["rv"].double()
        m32, e32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.1, B.BN_EPS))
        _, mean, invstd = torch.native_batch_norm(x["x"].double(), x["gamma"].double(), x["beta"].double(), rm, rv, True, m32, e32)
        for got, want in ((ref["mean"], mean), (ref["invstd"], invstd), (ref["rm"], rm), (ref["rv"], rv),
                          (ref["scale"], x["gamma"].double() * invstd), (ref["shift"], x["beta"].double() - mean * x["gamma"].double() * invstd)):
            assert torch.allclose(got, want, rtol=1e-11, atol=0), (got, want)
