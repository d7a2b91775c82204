"""No GPU: the float64 reference of tests/conv_cases.py held to float64 F.conv2d and to its autograd input gradient; the exactness
conditions of the "exact" inputs; and which kernel every launch of tests/test_gpu_conv.py reaches, pinned with
pmf_conv_fwd_variant (nothing is launched) against tests/golden/conv_case_launches.json, with the coverage that table owes:
every family of test_conv_dispatch_host.FAMILIES, every family the recorded input-gradient rows (*.b*) of
tests/golden/conv_dispatch.json launch, the wave-scheduled kernel with 1, 2 and 4 output tiles per workgroup, both K-split
combine forms.  Kernels are selected with cfg, w against w_s3 and the ticket pointer -- never with the environment switches
(PMF_STEM_DIRECT, PMF_CONV_WS*, PMF_CONV_FORCE are read once per process): the table is what the DEFAULT environment gives."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pmf_amd import _lib as L
from tests import conv_cases as K
from tests.test_conv_dispatch_host import FAMILIES, GOLDEN, unpack
from tests.wgrad_cases import transformed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_case_launches.json")
NAMES = [c.name for c in K.CASES]


def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), what


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _operand(case, inp):
    """the concatenated, transformed operands as a float64 NCHW tensor of Ktot channels"""
    cols = []
    for i, s in enumerate(case.srcs):
        v = np.array(transformed(case, inp, i)[0])
        v = np.concatenate([v, np.zeros(v.shape[:3] + (s.C - v.shape[3],))], -1)      # (a pitch below C: nothing there)
        cols.append(v)
    x = np.concatenate(cols, -1)
    if len(case.srcs) == 1:
        x[..., case.C_real:] = 0.0
    return _nchw(x)


def _layer_gradient(case, inp):
    """autograd's input gradient of the whole layer [N, H, W, all input channels from the pack's column 0 on]"""
    cv = case.conv
    k, Cf = cv["k"], cv["Cf"]
    w = torch.from_numpy(inp["Wwin"].astype(np.float64))[:, :Cf, :].permute(1, 2, 0).reshape(Cf, -1, k, k)   # [cf][column][ky][kx]
    x = torch.zeros(case.N, w.shape[1], cv["H"], cv["W"], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, cv["stride"], cv["pad"], cv["dil"])
    dz = _operand(case, inp)[:, :Cf]
    assert y.shape == dz.shape
    return torch.autograd.grad(y, x, dz)[0].permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_float64_autograd(name):
    case = K.BY_NAME[name]
    inp = K.inputs(case, "random")
    G, S, M = K.reference(case, inp)
    assert (S >= np.abs(G) * (1 - 1e-12)).all() and (M >= S * (1 - 1e-12)).all()
    cv = case.conv
    if case.form == "fwd":
        k = cv["k"]
        w = torch.from_numpy(inp["Wwin"].astype(np.float64)).permute(2, 1, 0).reshape(case.Cout, case.Ktot, k, k)
        ref = F.conv2d(_operand(case, inp), w, None, cv["stride"], cv["pad"], cv["dil"]).permute(0, 2, 3, 1).numpy()
        _close(G, ref, name)
        return
    gx = _layer_gradient(case, inp)
    _close(G, gx[:, case.rows_y(), case.rows_x(), case.coloff:case.coloff + case.Cout], name)
    # a merged launch against the per-operand launches it replaces
    c0 = 0
    for k_, d in enumerate(case.dsts if len(case.dsts) > 1 else []):
        one = case.single(k_)
        G1 = K.reference(one, K.inputs(one, "random"))[0]
        _close(G1, G[..., c0:c0 + d.C], one.name + " against the merged launch")
        _close(G1, gx[..., one.coloff:one.coloff + d.C], one.name)
        c0 += d.C


def test_parity_classes_reassemble_the_full_gradient():
    cases = [K.BY_NAME[n] for n in K.PARITY]
    inp = K.inputs(cases[0], "random")
    gx = _layer_gradient(cases[0], inp)
    full = np.full(gx.shape, np.nan)
    for c in cases:
        i = K.inputs(c, "random")
        assert np.array_equal(i["x"][0], inp["x"][0]) and np.array_equal(i["Wwin"], inp["Wwin"])     # one layer, one dz
        assert np.isnan(full[:, c.rows_y(), c.rows_x()]).all()                                         # disjoint classes
        full[:, c.rows_y(), c.rows_x()] = K.reference(c, i)[0]
    _close(full, gx, "parity classes")


@pytest.mark.parametrize("name", NAMES)
def test_exact_inputs_cannot_round(name):
    case = K.BY_NAME[name]
    inp = K.inputs(case, "exact")
    assert K.exactness(case, inp) == []
    G = K.reference(case, inp)[0]
    assert np.array_equal(K.f32_of(G).astype(np.float64), G)
    for d, e, r in zip(case.dsts, inp["dst"], K.epilogue(case, inp, K.f32_of(G))):
        # what the launch does not own keeps the sentinel: pitch padding, other parity classes, pixels beyond OH x OW
        keep = np.ones(e["out0"].shape, bool)
        keep[:, case.rows_y(), case.rows_x(), :d.C] = False
        assert np.array_equal(r["full"].view(np.uint32)[keep], e["out0"].view(np.uint32)[keep])
        assert np.isfinite(r["v"]).all() and (r["v"] != 0).mean() > 0.1
        if K.integer_outputs(case):
            assert np.array_equal(r["v"], np.round(r["v"]))
    # the one-hot forms: every output is ONE product, a float32 number
    for mode in ("onehot_w", "onehot_x"):
        for salt in (0, 1):
            p = case.plain()
            G = K.reference(p, K.inputs(p, mode, salt))[0]
            assert np.array_equal(K.f32_of(G).astype(np.float64), G) and (G != 0).any()


def test_onehot_weights_hit_every_k_position_and_lane():
    """over the two salts the single weight of the output columns visits all 16 K positions of a step and, for every column
    residue the case has, both halves of the B fragment (lane = column % 32 + 32 * ((k % 16) / 8))"""
    for case in K.CASES:
        forms = K.wforms(case)
        if len(forms) < 2:
            continue
        p = case.plain()
        kpos, lanes = set(), set()
        for salt in (0, 1):
            W = K.inputs(p, "onehot_w", salt)["W"]
            t, k, co = np.nonzero(W)
            if "stem" in forms:
                k = t * 8 + k          # pack format 2: ONE virtual tap, K index tap * 8 + channel -- two taps per 16-deep step
            kpos |= set(k % 16)
            lanes |= set(co % 32 + 32 * ((k % 16) // 8))
        if "stem" in forms:            # both taps of a step, every real channel of each
            assert kpos == {h * 8 + c for h in (0, 1) for c in range(case.C_real)}, case.name
        else:
            assert kpos == set(range(min(16, case.C_real))), case.name
        assert lanes == {c + 32 * h for c in range(min(32, case.Ctot)) for h in (0, 1)}, case.name


# ------------------------------------------------------------------------------------------------ which kernel a launch reaches
@pytest.fixture(scope="module")
def table():
    return K.launch_table()


def test_launch_table_is_pinned(table):
    with open(TABLE) as f:
        want = json.load(f)
    assert sorted(table) == sorted(want)
    bad = [(k, table[k], want[k]) for k in sorted(table) if table[k] != want[k]]
    assert not bad, "family / BN / MT / K splits / combine form moved: %s" % bad[:8]


def test_table_reaches_every_forward_family(table):
    assert {r[0] for r in table.values()} == FAMILIES
    # four 16-channel slabs per stage: the 1792-channel descriptor (test_conv_dispatch_host.descriptors), refused by
    # pmf_conv_s3_eligible and run by pmf_conv_fwd all the same
    case = K.BY_NAME["f_1x1_1792_32"]
    assert L.lib().pmf_conv_s3_eligible(K.C.byref(K.host_desc(case, "f32"))) == 0
    assert table["f_1x1_1792_32/s3/0x0/0"][0] == 7
    # the (BN, MT) tiles each family is run on: all four, but 4 and 12 (128-pixel tiles only), 10 (a 256-pixel tile runs as 5),
    # 7 (one descriptor of 32 output channels)
    all4 = {(32, 1), (32, 2), (64, 1), (64, 2)}
    owed = {0: all4, 1: all4, 5: all4, 8: all4, 11: all4, 14: all4, 4: {(32, 1), (64, 1)}, 12: {(32, 1), (64, 1)},
            10: {(32, 1), (64, 1)}, 6: {(32, 1), (32, 2), (64, 1)}, 13: {(32, 1), (32, 2), (64, 2)}, 7: {(32, 1)}}
    for fam in FAMILIES - {100}:
        tiles = {(r[1], r[2]) for r in table.values() if r[0] == fam}
        assert tiles >= owed[fam], (fam, tiles)


def test_one_tap_weight_forms_either_side_of_the_streaming_threshold(table):
    """the one-tap direct kernel (family 11) keeps all weight fragments of a 32-channel output tile in LDS up to 96 KiB and
    streams them in chunks beyond (conv_direct_lds: K steps x 3 KiB + 16 Ktot + 256 bytes of tables, chunks of 8 K steps twice
    in LDS); the generic loop (family 0) takes what is no multiple of 16 channels; 1792 channels neither fit nor stream
    (family 7).  The LDS size of the pinned rows is what tells resident from streamed"""
    def lds(key):
        assert table[key][0] == 11, key
        return table[key][6]
    resident = lambda K_: (K_ // 16) * 3 * 1024 + 16 * K_ + 256
    streamed = lambda K_: 2 * 8 * 3 * 1024 + 16 * K_ + 256
    assert resident(448) <= 96 * 1024 < resident(512)
    assert lds("f_1x1_448_48_resident/s3/0x0/0") == resident(448)
    assert lds("f_1x1_512_48_stream/s3/0x0/0") == streamed(512) and lds("f_1x1_512_48_stream/s3/0x220/0") == streamed(512)
    assert lds("d_1x1_64_from512_stream/s3/0x0/0") == streamed(512)
    assert lds("f_1x1_3x64_80_full/s3/0x120/0") == resident(192)
    assert table["f_1x1_8_32_raw/f32/0x0/0"][0] == 0 and table["f_1x1_1792_32/s3/0x0/0"][0] == 7


def test_dgrad_cases_reach_every_recorded_backward_family(table):
    with open(GOLDEN) as f:
        rec = unpack(json.load(f))["launch"]
    owed = {r[0] for k, r in rec.items() if len(r) > 1 and re.search(r"\.b\d+$", k.split("/")[0])}
    assert owed
    got = {r[0] for k, r in table.items() if K.BY_NAME[k.split("/")[0]].form == "dgrad"}
    assert got >= owed, sorted(owed - got)


def test_wave_scheduled_and_combine_forms_are_reached(table):
    assert {r[7] for r in table.values() if r[0] == 100} == {1, 2, 4}          # NCO through cfg bits 26 and 27
    assert {K.BY_NAME[k.split("/")[0]].form for k, r in table.items() if r[0] == 100} == {"fwd", "dgrad"}
    split = [r for r in table.values() if r[3] > 1]
    assert {r[4] for r in split} == {1} and {r[5] for r in split} == {2}         # 1 = tickets, 2 = conv_finish_k
    assert {r[0] for r in split} >= {0, 1, 4, 5, 6, 7, 8, 10, 12}


def test_workspace_size_is_the_slab_layout():
    """there is no size query: K splits x [N][OH][OW][Cout rounded up to 4] floats (conv_epi.h).  With 4 bytes fewer the
    library does not fail: it splits one time fewer (choose_ksplit), so no slab can lie beyond the workspace"""
    n = 0
    for case in K.CASES:
        for wf, cfg, split in K.launches(case):
            if not split:
                continue
            p = K.pick(case, wf, cfg, True)
            assert p["ws_bytes"] == p["ksplit"] * K.slab_bytes(case)
            assert K.variant(K.host_desc(case, wf, cfg, p["ws_bytes"], True))[1][2] == p["ksplit"]
            fewer = K.variant(K.host_desc(case, wf, cfg, p["ws_bytes"] - 4, True))[1][2]
            assert fewer == (p["ksplit"] - 1 if p["ksplit"] > 2 else 1), (case.name, wf, cfg)
            assert p["tickets"] <= 16384
            n += 1
    assert n > 50
