"""Graph-building guards of the element-wise primitives, on the host (no GPU; the graphs are built on "cpu" and never run).

* ``pmf_fusion_gate_bwd`` has accumulate flags for the gradients of ``f`` and ``pcd`` and none for ``att``: it overwrites.
  A graph in which another consumer of the attention map has already written that gradient buffer must not build.
* Only ``pmf_maxpool3s2_bwd`` applies the relu' mask of a ``relu=True`` view.  The other backward kernels deliver
  dL/d(view output); handing them a relu view in training mode would silently drop the mask.
* The shipped PMF and EPMF training plans trip none of the guards.

No GPU is needed, but the built libpmf_amd.so is: ``Plan.finalise`` lays the plan out through ``_lib.lib()``, as in
tests/test_wgrad_dispatch_host.py.  In a checkout that has not been built these tests fail with PMFLibraryError."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.models import EPMFNet, PMFNet  # noqa: E402
from pmf_amd.plan import Plan, V  # noqa: E402

CPU = torch.device("cpu")
N, C, H, W = 2, 8, 4, 6


def _plan(n_inputs, training=True):
    P = Plan(CPU, training)
    P.masks = torch.ones(64)
    ts = []
    for i in range(n_inputs):
        t = P.input_nchw("in%d" % i, N, C, H, W, "in%d" % i)
        t.needs_grad = True
        ts.append(t)
    return P, ts


def test_gate_refuses_an_attention_gradient_that_is_already_written():
    # backward order is the reverse of the forward order: global_mean writes the gradient of `b` first, the gate would
    # then overwrite it
    P, (a, b, c) = _plan(3)
    P.external_grad(V(P.gate(V(a), V(b), c, name="gate")))
    P.external_grad(V(P.global_mean(V(b), name="gm")))
    with pytest.raises(NotImplementedError, match=r"gate backward overwrites the gradient of att.*in1\.g.*in1"):
        P.finalise()


def test_gate_builds_when_it_writes_the_attention_gradient_first():
    # the other consumer comes first in the forward order, i.e. later in the backward order: it accumulates onto the
    # gate's overwrite
    P, (a, b, c) = _plan(3)
    P.external_grad(V(P.global_mean(V(b), name="gm")))
    P.external_grad(V(P.gate(V(a), V(b), c, name="gate")))
    P.finalise()
    kinds = [L.OP_NAMES[k] for k in P.bwd_kinds]
    assert kinds.index("OP_GATE_BWD") < kinds.index("OP_GMEAN_BWD")
    gm = P.bwd_ops[kinds.index("OP_GMEAN_BWD")].u.sm
    assert gm.i[5] == 1                                      # accumulate


def _pm(P, t):
    return P.pmask_from(V(t))


RELU_CASES = {
    "add_act.a": lambda P, t: P.add_act(V(t[0], relu=True), V(t[1]), L.ACT_NONE),
    "add_act.b": lambda P, t: P.add_act(V(t[0]), V(t[1], relu=True), L.ACT_RELU),
    "avgpool": lambda P, t: P.avgpool(V(t[0], relu=True)),
    "bilinear": lambda P, t: P.bilinear(V(t[0], relu=True)),
    "pixel_shuffle": lambda P, t: P.pixel_shuffle(V(t[0], relu=True)),
    "global_mean": lambda P, t: P.global_mean(V(t[0], relu=True)),
    "gate.f": lambda P, t: P.gate(V(t[0], relu=True), V(t[1]), t[2]),
    "gate.att": lambda P, t: P.gate(V(t[0]), V(t[1], relu=True), t[2]),
    "pmask_mul": lambda P, t: P.pmask_mul(V(t[0], relu=True), _pm(P, t[1])),
}


@pytest.mark.parametrize("case", sorted(RELU_CASES))
def test_backward_without_relu_mask_refuses_a_relu_view(case):
    P, ts = _plan(3)
    with pytest.raises(NotImplementedError, match=r"%s: .*relu' mask.*in[01]" % case.split(".")[0]):
        RELU_CASES[case](P, ts)
    # the forward kernels do apply the ReLU of the view: an evaluation plan takes the same graph
    P, ts = _plan(3, training=False)
    RELU_CASES[case](P, ts)
    P.finalise()


def test_maxpool_takes_a_relu_view_in_training_mode():
    P, ts = _plan(1)
    P.external_grad(V(P.maxpool(V(ts[0], relu=True), name="mp")))
    P.finalise()
    assert [L.OP_NAMES[k] for k in P.bwd_kinds].count("OP_MAXPOOL_BWD") == 1


@pytest.mark.parametrize("net", [PMFNet, EPMFNet])
def test_shipped_training_plans_trip_no_guard(net):
    m = net(imagenet_pretrained=False).train(True)
    P = m._build(2, 32, 64, True, CPU)
    kinds = [L.OP_NAMES[k] for k in P.bwd_kinds]
    assert kinds.count("OP_GATE_BWD") == 4
