"""Which forward / input-gradient convolution kernel a descriptor gets, and the statistics-row count, K-stage count, K split,
combine form, LDS size and grid that go with it, pinned on the host (no GPU): pmf_conv_fwd_stat_rows, pmf_conv_fwd_kstages,
pmf_conv_fwd_stat_rows_max, pmf_conv_s3_eligible, pmf_conv_ws_ok, pmf_conv_ws_rows, pmf_conv_multi_ok and
pmf_conv_fwd_variant against tests/golden/conv_dispatch.json.

Descriptors: every OP_CONV of the forward and backward op arrays of every CONVS entry of tests/test_gpu_ops.py and of the PMF
and EPMF training plans (built on CPU memory, never run).  Rows: descriptor x cfg (as built, 0, TILE_CFGS) x ticket array (as
built, cleared) in the default environment, and cfg (as built, 0) under six more environments.  Three of the switches are read
once per process, so every environment is evaluated in a child Python process of its own.

A statistics-row count computed for another kernel than the one launched is a float64 partial-row buffer of the wrong size:
an out-of-bounds write, or uninitialised rows summed into the batch statistics, that no GPU test is certain to see.

The "rows" of the table were recorded from the library as it was BEFORE the selection moved into conv_pick()
(``python tests/test_conv_dispatch_host.py OUT.json`` writes them for whatever library is built in the tree); its "launch"
column is what that build launched for the row: [family (PIPE of conv_fwd_k, 100 = conv_ws_k), BN, MT, ksplit, combine,
dynamic LDS bytes, grid x, y, z] or [return code].  Equality, no tolerance."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmf_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")
ENVS = {"default": {},
        "stem_off": {"PMF_STEM_DIRECT": "0"},
        "ws_on": {"PMF_CONV_WS": "1"},
        "ws_off": {"PMF_CONV_WS": "0"},
        "ws_on_nco2": {"PMF_CONV_WS": "1", "PMF_CONV_WS_NCO": "2"},
        "force_32_1_4": {"PMF_CONV_FORCE": "32,1,4"},
        "force_64_2_0": {"PMF_CONV_FORCE": "64,2,0"}}
SWITCHES = ("PMF_STEM_DIRECT", "PMF_CONV_WS", "PMF_CONV_WS_NCO", "PMF_CONV_FORCE")
FAMILIES = {0, 1, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 100}
QUERIES = ("pmf_conv_fwd_stat_rows", "pmf_conv_fwd_kstages", "pmf_conv_fwd_stat_rows_max", "pmf_conv_s3_eligible",
           "pmf_conv_ws_ok", "pmf_conv_ws_rows", "pmf_conv_multi_ok")
NQ = len(QUERIES)
CPU = torch.device("cpu")


def _copy(d):
    c = L.ConvDesc()
    C.memmove(C.addressof(c), C.addressof(d), C.sizeof(L.ConvDesc))
    return c


def _convs(prefix, P, out):
    for tag, ops, n in (("f", P.fwd_ops, P.n_fwd), ("b", P.bwd_ops, P.n_bwd)):
        k = 0
        for i in range(n):
            if ops[i].kind == L.OP_CONV:
                out.append(("%s.%s%d" % (prefix, tag, k), _copy(ops[i].u.conv)))
                k += 1


def descriptors():
    """(name, descriptor as the plan fills it) of the CONVS entries (+ extras) and of the training plans -- host memory only,
    nothing is ever launched"""
    from pmf_amd.models import EPMFNet, PMFNet
    from tests.test_gpu_ops import CONVS, _conv_graph
    unit, plan = [], []
    for case in CONVS:
        Hn, conv_out = _conv_graph(case, "cpu")[:2]
        Hn.P.external_grad(conv_out)
        Hn.P.finalise()
        _convs("unit." + case[0], Hn.P, unit)
    # (neither table reaches PIPE 7, four 16-channel slabs per stage: one tap on split-bf16 weights whose fragments neither fit
    # LDS nor stream in chunks, i.e. from 1792 input channels on -- pmf_conv_s3_eligible refuses the layer, so no plan sets w_s3
    # for it, but pmf_conv_fwd runs it)
    Hn, conv_out = _conv_graph(("c1x1_1792_32", 1, 4, 32, [1792], 32, 1, 1, 0, 1, False, "none", False), "cpu")[:2]
    Hn.P.external_grad(conv_out)
    Hn.P.finalise()
    extra = []
    _convs("extra.c1x1_1792_32_s3", Hn.P, extra)
    name, d = extra[0]
    d.w_s3, d.w = d.w_s3 or d.w, None
    unit.append((name, d))
    for net in (PMFNet, EPMFNet):
        m = net(imagenet_pretrained=False).train(True)
        _convs("plan." + net.__name__, m._build(2, 32, 64, True, CPU), plan)
    return unit, plan


def cases(envname):
    """(key, descriptor) of every row of one environment"""
    from tests.test_gpu_ops import TILE_CFGS
    unit, plan = descriptors()
    for name, d in unit + plan:
        cfgs = [("built", d.cfg), ("0", 0)]
        if envname == "default":
            cfgs += [("%#x" % c, c) for c in TILE_CFGS]
        for cname, cfg in cfgs:
            for tk in (1, 0):
                if not tk and (envname != "default" or not d.splitk_tickets):
                    continue            # (only the default environment clears the array; nothing to clear: same row)
                c = _copy(d)
                c.cfg = cfg
                if not tk:
                    c.splitk_tickets = None
                yield "%s/cfg=%s/tk=%d/%s" % (name, cname, tk, envname), c


def pack(rows, launch):
    """flat {key: [queries]} + {key: [launch]} -> the compact form on disk.  Every distinct list of ints is stored once:
    "queries" (the seven query exports) and "launches" (the launch record) are the rows' two halves, "values" the distinct
    (query, launch) pairs, flattened.  A descriptor is a "pattern": the index of its key list ("cfg/tk/environment", in
    "keys") followed by one index into "values" per key; the layers of the plans repeat, so the distinct patterns are stored
    once and "rows" maps a descriptor name without its running number ("plan.PMFNet.f") to the patterns of f0, f1, ..."""
    def intern(table, item):
        return table.setdefault(item, len(table))
    queries, launches, values, keys, patterns, per_desc = {}, {}, {}, {}, {}, {}
    for k in sorted(rows):
        name, sub = k.split("/", 1)
        v = intern(values, (intern(queries, tuple(rows[k][:NQ])), intern(launches, tuple(launch.get(k, [])))))
        per_desc.setdefault(name, []).append((sub, v))
    tree = {}
    for name, subs in per_desc.items():
        pat = (intern(keys, tuple(s for s, _ in subs)),) + tuple(v for _, v in subs)
        prefix, number = re.match(r"^(.*\.[fb])(\d+)$", name).groups()
        tree.setdefault(prefix, {})[int(number)] = intern(patterns, pat)
    return {"queries": list(queries), "launches": list(launches), "values": [i for v in values for i in v], "keys": list(keys),
            "patterns": list(patterns), "rows": {p: [d[i] for i in range(len(d))] for p, d in tree.items()}}


def unpack(packed):
    rows, launch = {}, {}
    for prefix, pats in packed["rows"].items():
        for number, pat in enumerate(pats):
            pat = packed["patterns"][pat]
            for sub, v in zip(packed["keys"][pat[0]], pat[1:]):
                k = "%s%d/%s" % (prefix, number, sub)
                rows[k] = packed["queries"][packed["values"][2 * v]]
                launch[k] = packed["launches"][packed["values"][2 * v + 1]]
    return {"rows": rows, "launch": launch}


def dump(packed, f):
    """the tables as JSON with short lines: a pattern or a name list per line, eight lists of ints (32 pair indices) per line"""
    def lines(v, per):
        return ",\n".join(",".join(json.dumps(x, separators=(",", ":")) for x in v[i:i + per]) for i in range(0, len(v), per))
    per = {"queries": 8, "launches": 8, "values": 64, "keys": 1, "patterns": 1}
    parts = ['"%s":[\n%s\n]' % (k, lines(packed[k], n)) for k, n in per.items()]
    parts.append('"rows":{\n%s\n}' % ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in packed["rows"].items()))
    f.write("{\n%s\n}\n" % ",\n".join(parts))


def bind(lib):
    for q in QUERIES + ("pmf_conv_fwd_variant",):
        if hasattr(lib, q):
            getattr(lib, q).restype = C.c_int
            getattr(lib, q).argtypes = [C.POINTER(L.ConvDesc)] + ([C.POINTER(C.c_int32 * 12)] if q.endswith("variant") else [])
    return lib


def row(lib, d):
    """the seven queries (+ [variant, info x 12] when the library exports pmf_conv_fwd_variant)"""
    r = [getattr(lib, q)(C.byref(d)) for q in QUERIES]
    if hasattr(lib, "pmf_conv_fwd_variant"):
        info = (C.c_int32 * 12)()
        r.append(lib.pmf_conv_fwd_variant(C.byref(d), C.byref(info)))
        r += list(info)
    return r


def child(envname, out):
    for k in SWITCHES:
        assert os.environ.get(k) == ENVS[envname].get(k), (k, os.environ.get(k))
    lib = bind(L.lib())
    with open(out, "w") as f:
        json.dump({k: row(lib, d) for k, d in cases(envname)}, f)


def table(script=os.path.abspath(__file__)):
    """all rows: one child process per environment (CPU only), all running at once"""
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for ename, env in ENVS.items():
            e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            e.update(env, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
            out = os.path.join(tmp, ename + ".json")
            procs.append((ename, out, subprocess.Popen([sys.executable, script, "--child", ename, out], env=e, cwd=ROOT)))
        for ename, out, p in procs:
            assert p.wait() == 0, ename
            with open(out) as f:
                rows.update(json.load(f))
    return rows


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return unpack(json.load(f))


@pytest.fixture(scope="module")
def got():
    return table()


def test_conv_dispatch_matches_recorded_table(recorded, got):
    want = recorded["rows"]
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(got) if got[k][:NQ] != want[k]]
    assert not bad, "statistics rows / K stages / eligibility moved: %s" % [(k, got[k][:NQ], want[k]) for k in bad[:8]]


def test_conv_fwd_variant_matches_recorded_launch(recorded, got):
    launch = recorded["launch"]
    assert sorted(launch) == sorted(got)
    bad = []
    for k in sorted(got):
        variant, info = got[k][NQ], got[k][NQ + 1:]
        rec = launch[k]
        if len(rec) == 1:                  # the recorded build refused the descriptor: the same return code, nothing else
            if variant != rec[0]:
                bad.append((k, variant, rec))
            continue
        # info: BN, MT, ksplit, combine, stat rows, K stages, LDS bytes, grid x, y, z, NCO, A-slab variant
        if [variant] + info[:4] + info[6:10] != rec[:9] or (variant == 100) != (info[10] != 0) or \
                (variant == 100 and [info[10], info[11]] != rec[9:11]):
            bad.append((k, variant, info, rec))
        if info[4] != got[k][0] or info[5] != got[k][1]:       # the two query exports read the same pick
            bad.append((k, "stat rows / K stages", info[4:6], got[k][:2]))
    assert not bad, "pmf_conv_fwd_variant disagrees with the recorded launch: %s" % bad[:8]
    assert {r[0] for r in launch.values() if len(r) > 1} == FAMILIES         # every family is covered


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        rows, launch = table(), {}
        if len(sys.argv) > 2:              # the launch record of the same rows (a build whose launches were recorded)
            with open(sys.argv[2]) as f:
                launch = json.load(f)
        with open(sys.argv[1], "w") as f:
            dump(pack(rows, launch), f)
        print("%d rows -> %s" % (len(rows), sys.argv[1]))
