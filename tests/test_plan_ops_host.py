"""Every op a plan emits, pinned on the host (no GPU) against tests/golden/plan_ops.json.

A plan finalised on CPU memory is a complete, never-run description of the step: if its op arrays are equal, the device sees
the same launches.  For every op of ``fwd_ops`` and ``bwd_ops`` the table holds the kind name and ten hex digits of the SHA-1
of the op's bytes, made position-independent first: the op is read as little-endian 64-bit words, and every word that falls
inside a known allocation (the four arenas, the FlatState buffers, the model's parameters and buffers, ``P.masks``, the pack
tables and the reduce tables) is replaced by ``name+offset``.  The pack and reduce tables (pointers and block layout) are
hashed the same way; the arena sizes, ``fwd_shift``, ``bwd_shift``, ``fwd_pack_skip``, ``n_events``, the ``_conv_fin`` /
``_conv_fold`` maps and ``dp_events`` are stored as they are, ``grad_done`` (by parameter, in the order of the ``pgrad``
calls) and ``meta_fwd`` / ``meta_bwd`` as one hash each.  Hashes are per op, so a failure names the first differing op index and
kind.

Cases: the PMFNet and EPMFNet training plans at 2 x 32 x 64, as built and with a FlatState (the deferred ``flush_reds``
path); the same under the environment switches of ENVS that change the op list; every CONVS entry of tests/test_gpu_ops.py
and the EXTRA graphs below, which reach the branches of ``conv()`` / ``_dgrad()`` that none of those reaches.  Some switches
are read once per process, so every environment is built in a child Python process of its own.

The table was recorded from the plan code as it was BEFORE ``conv()`` and ``_dgrad()`` were split into methods
(``python tests/test_plan_ops_host.py OUT.json`` writes it for whatever tree it runs in).  Equality, no tolerance: neither the
order of ``alloc``, ``add_pack``, ``pgrad`` and ``emit`` calls nor one byte of one op may move."""
import bisect
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.plan import Plan, V  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_ops.json")
# environment -> (switches, flat builds too, unit graphs too)
ENVS = {"default": ({}, True, True),
        "merge0": ({"PMF_DGRAD_MERGE": "0"}, False, False),
        "small0": ({"PMF_BN_SMALL": "0"}, False, False),
        "fused0": ({"PMF_BN_BWD_FUSED": "0"}, False, False),
        "f32": ({"PMF_CONV_F32": "1"}, False, False),
        "lane0": ({"PMF_WGRAD_LANE": "0"}, False, False),
        "red0": ({"PMF_RED_BATCH": "0"}, None, False)}          # (None: the FlatState builds only)
SWITCHES = sorted({k for env, _, _ in ENVS.values() for k in env})
CPU = torch.device("cpu")
HASH = 10                       # hex digits of SHA-1 kept per op


# ---- graphs for the branches of conv() / _dgrad() that neither a network plan nor a CONVS entry reaches ----------------
def _harness(shapes, masks=4):
    from tests.test_gpu_ops import Harness
    return Harness(shapes, masks=masks, dev="cpu")


def _x_bn_eval():
    """a BatchNorm module in eval mode inside a training plan: OP_BN_EVAL forward, backward through the fixed affine map;
    PMF_BN_SMALL is on, so its backward is the one-launch form with the training flag clear"""
    Hn = _harness([(2, 32, 8, 32)])
    conv, bn = nn.Conv2d(32, 32, 3, 1, 1), nn.BatchNorm2d(32).eval()
    return Hn.P, Hn.P.conv([V(Hn.inputs[0])], conv, L.ACT_LRELU, bn, name="u"), (conv, bn)


def _x_bn_eval_big():
    """the same on a map above the one-launch limit: reduce + apply with the training flag clear"""
    Hn = _harness([(1, 16, 64, 64)])
    conv, bn = nn.Conv2d(16, 16, 3, 1, 1, bias=False), nn.BatchNorm2d(16).eval()
    return Hn.P, Hn.P.conv([V(Hn.inputs[0])], conv, L.ACT_NONE, bn, "bn_act", True, name="u"), (conv, bn)


def _x_bcast():
    """a broadcast operand (a 1 x 1 map seen at image size) next to a plain one: the temporary + OP_COLSUM path"""
    Hn = _harness([(2, 32, 1, 1), (2, 32, 4, 24)])
    conv = nn.Conv2d(64, 32, 1)
    return Hn.P, Hn.P.conv([V(Hn.inputs[0], bcast=True), V(Hn.inputs[1])], conv, L.ACT_LRELU, name="u"), (conv,)


def _x_cat_twice():
    """torch.cat of one tensor twice, large and aligned enough for the merged launch: the ``holders`` test refuses it"""
    Hn = _harness([(1, 64, 32, 64)])
    conv, bn = nn.Conv2d(128, 64, 3, 1, 1), nn.BatchNorm2d(64)
    v = V(Hn.inputs[0])
    return Hn.P, Hn.P.conv([v, v], conv, L.ACT_LRELU, bn, name="u"), (conv, bn)


def _x_chain():
    """three conv + BatchNorm layers in a row on a map above the one-launch limit.  The stride-1 input gradient of the second
    is the last writer of the first one's gy and carries its column sums (OP_BN_BWD_FOLD; EP_STAT_X_ONLY, the view has no
    ReLU); the parity launches of the stride-2 third never carry them, so the second layer reduces (OP_BN_BWD_REDUCE)"""
    Hn = _harness([(1, 32, 64, 64)])
    c1, b1 = nn.Conv2d(32, 32, 3, 1, 1), nn.BatchNorm2d(32)
    c2, b2 = nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
    c3, b3 = nn.Conv2d(32, 64, 3, 2, 1, bias=False), nn.BatchNorm2d(64)
    c4 = nn.Conv2d(64, 20, 3, 1, 1)
    P = Hn.P
    v1 = P.conv([V(Hn.inputs[0])], c1, L.ACT_LRELU, b1, name="a")
    v2 = P.conv([v1], c2, L.ACT_NONE, b2, "bn_act", True, name="b")
    v3 = P.conv([v2], c3, L.ACT_NONE, b3, "bn_act", True, name="c")
    return P, P.conv([v3], c4, L.ACT_NONE, name="d"), (c1, b1, c2, b2, c3, b3, c4)


def _x_mask_bias():
    """EPMF's SparseVariantConv outside the network: per-pixel mask with conv bias + extra bias, with and without
    BatchNorm, and with no bias at all"""
    Hn = _harness([(2, 8, 16, 32)])
    P = Hn.P
    c1, b1, e1 = nn.Conv2d(8, 32, 3, 1, 1), nn.BatchNorm2d(32), nn.Parameter(torch.zeros(32))
    c2, e2 = nn.Conv2d(32, 32, 3, 1, 1), nn.Parameter(torch.zeros(32))
    pm = P.pmask_from(V(Hn.inputs[0]))
    m1 = P.pmask_pool(pm, c1)
    v1 = P.conv([V(Hn.inputs[0])], c1, L.ACT_LRELU, b1, name="a", pmask=m1, extra_bias=e1)
    m2 = P.pmask_pool(m1, c2)
    v2 = P.conv([v1], c2, L.ACT_LRELU, name="b", pmask=m2, extra_bias=e2)
    c3 = nn.Conv2d(32, 32, 3, 1, 1, bias=False)             # (no bias at all: the mask multiplies, nothing is summed)
    out = P.conv([v2], c3, L.ACT_LRELU, name="c", pmask=P.pmask_pool(m2, c3))
    holder = nn.Module()
    holder.e1, holder.e2 = e1, e2
    return P, out, (c1, b1, c2, c3, holder)


def _x_plain_nobias():
    """no bias, no activation, no BatchNorm: the gradient of the conv output is used as it arrives"""
    Hn = _harness([(1, 32, 8, 32)])
    conv = nn.Conv2d(32, 32, 3, 1, 1, bias=False)
    return Hn.P, Hn.P.conv([V(Hn.inputs[0])], conv, L.ACT_NONE, name="u"), (conv,)


def _x_side():
    """a BatchNorm view produced on lane 0 and consumed on lane 1: the consumer accumulates into a private tensor of its lane,
    the producer's BatchNorm backward folds it in first (``_side``)"""
    Hn = _harness([(1, 32, 8, 32)])
    P = Hn.P
    c1, b1, c2 = nn.Conv2d(32, 32, 3, 1, 1), nn.BatchNorm2d(32), nn.Conv2d(32, 32, 3, 1, 1)
    v1 = P.conv([V(Hn.inputs[0])], c1, L.ACT_LRELU, b1, name="a")
    P.lane = 1
    out = P.conv([v1], c2, L.ACT_LRELU, name="b")
    P.lane = 0
    return P, out, (c1, b1, c2)


def _x_unaligned():
    """a 5-channel operand in front of a 32-channel one: the second neither starts on a 32-column fragment nor can every
    operand have a pack of its own (5 is no multiple of 8), so the input gradients leave the split-bf16 kernels"""
    Hn = _harness([(1, 5, 8, 32), (1, 32, 8, 32)])
    conv = nn.Conv2d(37, 32, 3, 1, 1)
    return Hn.P, Hn.P.conv([V(t) for t in Hn.inputs], conv, L.ACT_LRELU, name="u"), (conv,)


def _x_merge_relu():
    """two conv -> BatchNorm -> ReLU views concatenated into a third conv on a map above the one-launch limit: ONE merged
    input-gradient launch applies the ReLU mask of each destination and carries both BatchNorm-backward column sums (two
    folds behind one launch)"""
    Hn = _harness([(1, 32, 48, 64)])
    P = Hn.P
    c1, b1 = nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
    c2, b2 = nn.Conv2d(32, 64, 1, bias=False), nn.BatchNorm2d(64)
    c3 = nn.Conv2d(96, 32, 3, 1, 1)
    v1 = P.conv([V(Hn.inputs[0])], c1, L.ACT_NONE, b1, "bn_act", True, name="a")
    v2 = P.conv([V(Hn.inputs[0])], c2, L.ACT_NONE, b2, "bn_act", True, name="b")
    return P, P.conv([v1, v2], c3, L.ACT_LRELU, name="c"), (c1, b1, c2, b2, c3)


def _x_c20_gather():
    """20 output channels behind a dilation-18 3x3 on a 40 x 40 map (per-tap staging): rounded up to 32, the K of the input
    gradient still gets no split-bf16 kernel, so it falls back to 24"""
    Hn = _harness([(1, 32, 40, 40)])
    conv = nn.Conv2d(32, 20, 3, 1, 18, 18)
    return Hn.P, Hn.P.conv([V(Hn.inputs[0])], conv, L.ACT_NONE, name="u"), (conv,)


def _x_eval_plan():
    """a plan built for inference: forward ops only, BatchNorm from the running statistics"""
    P = Plan(CPU, False)
    P.masks = torch.ones(4)
    t = P.input_nchw("in0", 1, 32, 8, 32, "in0")
    conv, bn = nn.Conv2d(32, 32, 3, 1, 1), nn.BatchNorm2d(32).eval()
    return P, P.conv([V(t)], conv, L.ACT_LRELU, bn, name="u"), (conv, bn)


EXTRA = {"x_bn_eval": _x_bn_eval, "x_bn_eval_big": _x_bn_eval_big, "x_bcast": _x_bcast, "x_cat_twice": _x_cat_twice,
         "x_chain": _x_chain, "x_mask_bias": _x_mask_bias, "x_side": _x_side, "x_unaligned": _x_unaligned,
         "x_merge_relu": _x_merge_relu, "x_c20_gather": _x_c20_gather, "x_eval_plan": _x_eval_plan,
         "x_plain_nobias": _x_plain_nobias}


# ---- position-independent bytes ----------------------------------------------------------------------------------------
class Ranges:
    """named allocations; ``norm(bytes)`` replaces every 64-bit word that points into one by name+offset"""

    def __init__(self):
        self.r = []

    def add(self, name, base, size):
        if size > 0 and not any(b <= base and base + size <= b + s for b, s, _ in self.r):       # (a view of an earlier one)
            self.r.append((base, size, name))

    def tensor(self, name, t):
        self.add(name, t.data_ptr(), t.numel() * t.element_size())

    def freeze(self):
        self.r.sort()
        self.bases = [b for b, _, _ in self.r]

    def norm(self, raw):
        raw = raw + b"\0" * (-len(raw) % 8)
        out = []
        for (w,) in struct.iter_unpack("<Q", raw):
            i = bisect.bisect_right(self.bases, w) - 1
            if i >= 0 and w < self.r[i][0] + self.r[i][1]:
                out.append("%s+%d" % (self.r[i][2], w - self.r[i][0]))
            else:
                out.append("%x" % w)
        return hashlib.sha1(" ".join(out).encode()).hexdigest()[:HASH]


def pin(P, modules):
    """the pinned record of a finalised plan"""
    R = Ranges()
    for a in (P.act, P.zero_fwd, P.zero_bwd, P.persist):
        R.add(a.name, a.base, max(a.size, 256))
    if P.flat is not None:
        R.tensor("flat.param", P.flat.param)
        R.tensor("flat.grad", P.flat.grad)
    for k, m in enumerate(modules):
        for n, t in list(m.named_parameters()) + list(m.named_buffers()):
            R.tensor("m%d.%s" % (k, n), t)
    if P.masks is not None:
        R.tensor("masks", P.masks)
    for k, tab in enumerate(P.pack_tables):
        R.tensor("pack%d" % k, tab[1])
    for k, (jd, md) in enumerate(P._red_tables):
        R.tensor("red%d.desc" % k, jd)
        R.tensor("red%d.meta" % k, md)
    R.freeze()

    def short(v):
        return hashlib.sha1(json.dumps(v, sort_keys=True).encode()).hexdigest()[:HASH]

    def ops(arr, n):
        return ["%s %s" % (L.OP_NAMES[arr[i].kind][3:], R.norm(bytes(arr[i]))) for i in range(n)]
    return {"sizes": {a.name: a.size for a in (P.act, P.zero_fwd, P.zero_bwd, P.persist)},
            "fwd_shift": P.fwd_shift, "bwd_shift": P.bwd_shift, "fwd_pack_skip": P.fwd_pack_skip, "n_events": P.n_events,
            "conv_fin": sorted([k, v] for k, v in P._conv_fin.items()),
            "conv_fold": sorted([k, v] for k, v in P._conv_fold.items()),
            "pack_tables": [[t[0], t[2], t[3], t[4], int(t[5]), R.norm(bytes(t[1].numpy()))] for t in P.pack_tables],
            "red_tables": [[R.norm(bytes(jd.numpy())), R.norm(bytes(md.numpy()))] for jd, md in P._red_tables],
            # what the data-parallel scheduler and bench.py read next to the ops: the op that completes each parameter's
            # gradient (in P.params order, i.e. the order of the pgrad calls), the event lists, the per-op records
            "dp_events": [[n, list(e)] for n, e in P.dp_events],
            "grad_done": short([P.grad_done.get(id(p)) for p in P.params]),
            "meta": [short(sorted(m.items())) for m in (P.meta_fwd, P.meta_bwd)],
            "fwd": ops(P.fwd_ops, P.n_fwd), "bwd": ops(P.bwd_ops, P.n_bwd)}


def records(envname):
    """{case name: record} of one environment"""
    from pmf_amd.models import EPMFNet, PMFNet
    from pmf_amd.models.pmf_net import flatten_training_state
    from tests.test_gpu_ops import CONVS, _conv_graph
    _, flat, unit = ENVS[envname]
    out = {}
    for net in (EPMFNet, PMFNet):
        for with_flat in ((False, True) if flat else (True,) if flat is None else (False,)):
            m = net(imagenet_pretrained=False).train(True)
            if with_flat:
                flatten_training_state(m, [[p for p in m.parameters() if p.requires_grad]], CPU)
            out["%s%s/%s" % (net.__name__, ".flat" if with_flat else "", envname)] = pin(m._build(2, 32, 64, True, CPU), [m])
    if unit:
        for case in CONVS:
            Hn, conv_out, conv, bn = _conv_graph(case, "cpu")[:4]
            Hn.P.external_grad(conv_out)
            out["unit.%s/%s" % (case[0], envname)] = pin(Hn.P.finalise(), [conv] + ([bn] if bn is not None else []))
        for name, graph in EXTRA.items():
            P, conv_out, modules = graph()
            if P.training:
                P.external_grad(conv_out)
            out["unit.%s/%s" % (name, envname)] = pin(P.finalise(), list(modules))
    return out


def child(envname, out):
    for k in SWITCHES:
        assert os.environ.get(k) == ENVS[envname][0].get(k), (k, os.environ.get(k))
    torch.manual_seed(0)
    with open(out, "w") as f:
        json.dump(records(envname), f)


def table(script=os.path.abspath(__file__)):
    """all records: one child process per environment (CPU only), all running at once"""
    recs = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for ename, (env, _, _) in ENVS.items():
            e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            e.update(env, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
            out = os.path.join(tmp, ename + ".json")
            procs.append((ename, out, subprocess.Popen([sys.executable, script, "--child", ename, out], env=e, cwd=ROOT)))
        for ename, out, p in procs:
            assert p.wait() == 0, ename
            with open(out) as f:
                recs.update(json.load(f))
    return recs


def pack(recs):
    """{case: record} -> the compact form on disk.  Every distinct op ("KIND hash") is stored once, in "ops", as two hex
    digits of its index in "kinds" followed by the hash, in order of first use; an op list is runs of that table, flattened
    [start, count, start, count, ...] -- the environments share most ops of the default build, and new ops arrive in order.
    Every other field is an index into "values", the distinct field values."""
    kinds = sorted({op.split()[0] for r in recs.values() for lst in ("fwd", "bwd") for op in r[lst]})
    ops, values, cases = {}, {}, {}
    for name in sorted(recs, key=lambda n: (not n.endswith("/default"), ".flat" in n, n)):      # (the plain builds first)
        cases[name] = c = {}
        for k, v in recs[name].items():
            if k not in ("fwd", "bwd"):
                c[k] = values.setdefault(json.dumps(v, separators=(",", ":")), len(values))
                continue
            c[k] = runs = []
            for op in v:
                i = ops.setdefault(op, len(ops))
                if runs and runs[-2] + runs[-1] == i:
                    runs[-1] += 1
                else:
                    runs += [i, 1]
    return {"kinds": kinds, "ops": "".join("%02x%s" % (kinds.index(op.split()[0]), op.split()[1]) for op in ops),
            "values": [json.loads(v) for v in values], "cases": cases}


def unpack(packed):
    flat, w = "".join(packed["ops"]), 2 + HASH
    ops = ["%s %s" % (packed["kinds"][int(flat[i:i + 2], 16)], flat[i + 2:i + w]) for i in range(0, len(flat), w)]
    recs = {}
    for name, c in packed["cases"].items():
        recs[name] = r = {}
        for k, v in c.items():
            if k in ("fwd", "bwd"):
                r[k] = [op for a, n in zip(v[::2], v[1::2]) for op in ops[a:a + n]]
            else:
                r[k] = packed["values"][v]
    return recs


def dump(packed, f):
    """the packed table as JSON: twenty ops, one value or one case per line"""
    o, per = packed["ops"], 20 * (2 + HASH)
    parts = ['"kinds":%s' % json.dumps(packed["kinds"], separators=(",", ":")),
             '"ops":[\n%s\n]' % ",\n".join('"%s"' % o[i:i + per] for i in range(0, len(o), per)),
             '"values":[\n%s\n]' % ",\n".join(json.dumps(v, separators=(",", ":")) for v in packed["values"]),
             '"cases":{\n%s\n}' % ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":")))
                                              for k, v in packed["cases"].items())]
    f.write("{\n%s\n}\n" % ",\n".join(parts))


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return unpack(json.load(f))


@pytest.fixture(scope="module")
def got():
    return table()


def test_plan_cases_are_the_recorded_ones(recorded, got):
    assert sorted(got) == sorted(recorded)


def test_plan_layout_matches_recorded(recorded, got):
    """arena sizes, prologue lengths, event count, the conv -> finalize / fold maps, pack and reduce tables"""
    bad = [(name, k, got[name][k], rec[k]) for name, rec in sorted(recorded.items()) for k in rec
           if k not in ("fwd", "bwd") and got[name][k] != rec[k]]
    assert not bad, "plan layout moved: %s" % bad[:4]


def test_plan_ops_match_recorded(recorded, got):
    bad = []
    for name, rec in sorted(recorded.items()):
        for lst in ("fwd", "bwd"):
            g, w = got[name][lst], rec[lst]
            first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), None)
            if first is not None:
                bad.append("%s %s op %d: %s, recorded %s" % (name, lst, first, g[first], w[first]))
            elif len(g) != len(w):
                bad.append("%s %s: %d ops, recorded %d" % (name, lst, len(g), len(w)))
    assert not bad, "%d op lists differ from the recorded table; first differing op of each:\n%s" % (len(bad), "\n".join(bad[:12]))


def test_plan_ops_cover_every_backward_form(recorded):
    """the default-environment records contain every kind of op conv() and its helpers emit"""
    kinds = {op.split()[0] for name, rec in recorded.items() if name.endswith("/default") for op in rec["fwd"] + rec["bwd"]}
    assert {"BN_FINALIZE", "BN_EVAL", "BN_BWD_SMALL", "BN_BWD_FOLD", "BN_BWD_REDUCE", "BN_BWD_APPLY", "ACT_BWD",
            "PMASK_MUL_BWD", "VEC_ADD", "COLSUM", "WGRAD_PART", "WGRAD_RED", "WGRAD_RED_MULTI", "CONV"} <= kinds


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        recs = table()
        with open(sys.argv[1], "w") as f:
            dump(pack(recs), f)
        print("%d plans, %d ops -> %s" % (len(recs), sum(len(r["fwd"]) + len(r["bwd"]) for r in recs.values()), sys.argv[1]))
