"""Which weight-gradient kernel a descriptor gets, and the split count / workspace / stage-2 plan that go with it, pinned on
the host (no GPU): pmf_conv_wgrad_nsplit, pmf_conv_wgrad_workspace, pmf_conv_wgrad_reduce_plan and pmf_conv_wgrad_variant
against tests/golden/wgrad_dispatch.json, for every CONVS entry of tests/test_gpu_ops.py and every shape of
tools/bench_conv.py, with PMF_WGRAD_S3 set and clear, under the default environment and the two environments of
test_conv_unit_wgrad_variants.  A split count computed for another kernel than the one launched is a partial-slab workspace
of the wrong size, i.e. an out-of-bounds write no GPU test is certain to see.

The numbers of the table were recorded from the library as it was BEFORE the selection moved into wg_pick()
(``python tests/test_wgrad_dispatch_host.py OUT.json`` writes the table for whatever library is built in the tree); its
"kernel" column is the kernel template that build launched for the row.  Equality, no tolerance."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402
from tests.test_gpu_ops import CONVS, WGRAD_VARIANT_ENVS, _conv_graph  # noqa: E402
from tools.bench_conv import CASES, wgrad_desc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_dispatch.json")
ENVS = dict({"default": {}}, **WGRAD_VARIANT_ENVS)
SWITCHES = ("PMF_WG_S3N", "PMF_WGRAD_WGS")
# kernel template -> code of pmf_conv_wgrad_variant (include/pmf_amd.h)
KERNEL_VARIANT = {"conv_wgrad_k": L.WG_UNIT, "conv_wgrad_pipe_k": L.WG_PIPE, "conv_wgrad_s3_swp_k": L.WG_SWP,
                  "conv_wgrad_s3n_k": L.WG_NSPLIT, "wgrad_1x1_k": L.WG_DIRECT, "wgrad_1x1_s3_k": L.WG_DIRECT_S3,
                  "wgrad_stream_k": L.WG_STREAM, "wgrad_fewc_k": L.WG_FEWC} if hasattr(L, "WG_UNIT") else {}


def _copy(d):
    c = L.WgradDesc()
    C.memmove(C.addressof(c), C.addressof(d), C.sizeof(L.WgradDesc))
    return c


def descriptors():
    """(name, descriptor as the plan / the micro-benchmark fills it) -- host memory only, nothing is ever launched"""
    out = []
    for case in CONVS:
        Hn, conv_out = _conv_graph(case, "cpu")[:2]
        P = Hn.P
        P.external_grad(conv_out)
        P.finalise()
        ds = [_copy(P.bwd_ops[i].u.wgrad) for i in range(P.n_bwd) if P.bwd_ops[i].kind in (L.OP_WGRAD, L.OP_WGRAD_PART)]
        assert len(ds) == 1, case[0]
        out.append(("unit." + case[0], ds[0]))
    for case in CASES:
        out.append(("bench." + case[0], wgrad_desc(case)))
    # (neither table reaches the few-channel stem kernel: their 7x7 layers carry 8 padded input channels) the RGB stem
    stem = wgrad_desc(("full_stem_3_64_7x7", 2, 64, 2048, 8, 64, 7, 1))
    stem.Cin_real = 3
    out.append(("extra.full_stem_3_64_7x7", stem))
    return out


def _probe(d):
    """what Plan._wgrad asks pmf_conv_wgrad_nsplit with: the shape, no pointers, no operand flags, no dz pitch"""
    p = _copy(d)
    p.dz = p.partial = p.dw_oihw = p.dbias_rows = p.dbias_out = None
    p.dz_ldc = p.accumulate = p.dbias_nrows = p.dbias_ld = p.reserved0 = 0
    for i in range(L.MAX_SRC):
        s = p.src[i]
        s.x = s.scale = s.shift = s.cmul = None
        s.flags = s.cmul_ld = 0
    return p


def row(lib, d, s3):
    """[nsplit, nsplit of the plan's probe, workspace bytes, stage-2 workgroups, meta8 x 8] (+ [variant] when exported)"""
    d, p = _copy(d), _probe(d)
    d.flags = p.flags = L.WGRAD_S3 if s3 else 0
    d.nsplit = p.nsplit = 1
    ns, nsp = lib.pmf_conv_wgrad_nsplit(C.byref(d)), lib.pmf_conv_wgrad_nsplit(C.byref(p))
    d.nsplit = ns
    meta = (C.c_int32 * 8)()
    r = [ns, nsp, lib.pmf_conv_wgrad_workspace(C.byref(d)), lib.pmf_conv_wgrad_reduce_plan(C.byref(d), meta)] + list(meta)
    if hasattr(lib, "pmf_conv_wgrad_variant"):
        r.append(lib.pmf_conv_wgrad_variant(C.byref(d)))
    return r


def table(setenv, delenv):
    lib = L.lib()
    rows = {}
    descs = descriptors()
    for ename, env in ENVS.items():
        for k in SWITCHES:
            delenv(k)
        for k, v in env.items():
            setenv(k, v)
        for name, d in descs:
            for s3 in (1, 0):
                rows["%s/s3=%d/%s" % (name, s3, ename)] = row(lib, d, s3)
    for k in SWITCHES:
        delenv(k)
    return rows


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_wgrad_dispatch_matches_recorded_table(recorded, monkeypatch):
    got = table(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    want = recorded["rows"]
    assert sorted(got) == sorted(want)
    assert len(got) == (len(CONVS) + len(CASES) + 1) * 2 * len(ENVS)
    bad = [k for k in sorted(got) if got[k][:12] != want[k][:12]]
    assert not bad, "split count / workspace / stage-2 plan moved: %s" % [(k, got[k][:12], want[k][:12]) for k in bad[:8]]
    # the family: the kernel template the recorded build launched for this row
    kern = recorded["kernel"]
    assert sorted(kern) == sorted(want)
    badv = [(k, got[k][12], kern[k]) for k in sorted(got) if got[k][12] != KERNEL_VARIANT[kern[k].split("<")[0]]]
    assert not badv, "pmf_conv_wgrad_variant disagrees with the launched kernel: %s" % badv[:8]
    assert {KERNEL_VARIANT[v.split("<")[0]] for v in kern.values()} == set(KERNEL_VARIANT.values())   # every family is covered


if __name__ == "__main__":
    def _del(k):
        os.environ.pop(k, None)
    rows = table(os.environ.__setitem__, _del)
    with open(sys.argv[1], "w") as f:
        json.dump({"rows": {k: v[:12] for k, v in rows.items()}}, f, indent=0, sort_keys=True)
    print("%d rows -> %s" % (len(rows), sys.argv[1]))
