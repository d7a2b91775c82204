"""-m gpu: the HIP path (through the C ABI) against the CPU oracle and the committed golden fixtures.

Tolerance (BASELINE.json north_star / SURVEY.md 7): |d| <= 1e-3 * max(|ref|, 1) on pre-softmax logits,
abs <= 1e-4 on probabilities; integer outputs (KNN labels, loader indices / scatter) bit-exact.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.utils.detinit import deterministic_init, det_tensor, synthetic_batch  # noqa: E402
from tests import gpu_helpers as G  # noqa: E402


def _sync_check(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- single ops
CONV_CASES = [
    # name, N, H, W, [Cin...], Cout, k, dil, pad, stride, act, transforms
    ("3x3_32_32", 2, 16, 64, [32], 32, 3, 1, 1, 1, 1, False),
    ("3x3d2_64_64_xf", 1, 24, 40, [64], 64, 3, 2, 2, 1, 1, True),
    ("2x2d2_32", 2, 8, 32, [32], 32, 2, 2, 1, 1, 1, False),
    ("1x1_cat3", 2, 16, 32, [64, 64, 64], 64, 1, 1, 0, 1, 1, True),
    ("3x3_cat2_80_32", 1, 16, 96, [16, 64], 32, 3, 1, 1, 1, 1, True),
    ("1x1_8_32", 2, 16, 32, [8], 32, 1, 1, 0, 1, 1, False),
    ("7x7_8_64", 1, 16, 48, [8], 64, 7, 1, 3, 1, 0, False),
    ("7x7_8_64_xf", 2, 19, 70, [8], 64, 7, 1, 3, 1, 1, True),      # stem class through an operand view (zero padding!)
    ("3x3s2_64_128", 2, 16, 32, [64], 128, 3, 1, 1, 2, 0, False),
    ("1x1s2_64_128", 2, 16, 32, [64], 128, 1, 1, 0, 2, 0, False),
    ("3x3d6_64_64", 1, 8, 40, [64], 64, 3, 6, 6, 1, 0, False),
    ("3x3d18_64_64", 1, 8, 40, [64], 64, 3, 18, 18, 1, 0, False),
    ("3x3_16_20", 1, 16, 32, [16], 20, 3, 1, 1, 1, 0, False),
    ("3x3_256_256_small", 2, 4, 16, [256], 256, 3, 1, 1, 1, 1, False),
    # 1x1 shapes of the direct split-bf16 variant (PIPE 11): 5 k-steps (guarded tail of the 4-step loop), ragged output
    # tile and image edge, operand transforms; a plain one with 20 output channels
    ("1x1_cat2_80_48_xf", 2, 17, 45, [16, 64], 48, 1, 1, 0, 1, 1, True),
    ("1x1_32_20", 1, 16, 64, [32], 20, 1, 1, 0, 1, 0, False),
]


def _nan_rows(n, Cout):
    return torch.full((n, 2, Cout), float("nan"), device="cuda", dtype=torch.float64)


def _written_rows(stats, rows):
    """the first ``rows`` rows of a _nan_rows(rows + 2) buffer after a launch; the two guard rows behind them must still hold
    the NaN bit pattern they were filled with (a launch that writes more rows than pmf_conv_fwd_stat_rows said)"""
    assert torch.equal(stats[rows:].view(torch.int64), _nan_rows(2, stats.shape[2]).view(torch.int64))
    return stats[:rows]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_fwd_vs_torch_cpu(case):
    name, N, H, W, cins, Cout, k, dil, pad, stride, act, xf = case
    lib = L.lib()
    xs = [det_tensor("%s.x%d" % (name, i), (N, c, H, W)) for i, c in enumerate(cins)]
    w = det_tensor(name + ".w", (Cout, sum(cins), k, k), -0.2, 0.2)
    b = det_tensor(name + ".b", (Cout,))
    srcs, ref_in = [], []
    for i, (x, c) in enumerate(zip(xs, cins)):
        s = dict(x=G.nhwc(x), C=c)
        xr = x
        if xf:
            sc, sh = det_tensor("%s.sc%d" % (name, i), (c,), 0.5, 1.5), det_tensor("%s.sh%d" % (name, i), (c,))
            cm = (det_tensor("%s.cm%d" % (name, i), (N, c)) > -0.6).float() * 1.25
            s.update(scale=sc.cuda(), shift=sh.cuda(), cmul=cm.cuda().contiguous(), relu=(i % 2 == 0))
            xr = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
            if i % 2 == 0:
                xr = xr.clamp_min(0)
            xr = xr * cm[:, :, None, None]
        srcs.append(s)
        ref_in.append(xr)
    ref = F.conv2d(torch.cat(ref_in, 1), w, b, stride=stride, padding=pad, dilation=dil)
    if act == 1:
        ref = F.leaky_relu(ref, 0.01)
    OH, OW = ref.shape[2], ref.shape[3]
    ldw = (Cout + 63) // 64 * 64
    wpk = G.pack_fwd(w, sum(cins), ldw)
    out = torch.zeros(N, OH, OW, (Cout + 7) // 8 * 8, device="cuda")
    b_dev = b.cuda()   # keep alive: the descriptor only holds raw pointers
    d = G.conv_desc(srcs, wpk, ldw, b_dev, out, N, OH, OW, Cout, G.taps_of(k, k, dil, pad), stride, act)
    rows = lib.pmf_conv_fwd_stat_rows(C.byref(d))          # one partial (sum, sumsq) row per workgroup tile
    stats = _nan_rows(rows + 2, Cout)                        # exactly `rows` rows are written: two guard rows behind them
    d.stats = stats.data_ptr()
    _sync_check(lib.pmf_conv_fwd(C.byref(d), G.stream()), "pmf_conv_fwd")
    got = G.from_nhwc(out, Cout)
    assert G.rel_err(got.numpy(), ref.numpy()) < 2e-5
    st = _written_rows(stats, rows).sum(0).cpu()
    assert torch.isfinite(st).all()
    assert G.rel_err(st[0].numpy() / ref[0, 0].numel(), (ref.sum((0, 2, 3)) / ref[0, 0].numel()).numpy()) < 1e-3
    assert G.rel_err(st[1].numpy() / ref[0, 0].numel(), ((ref * ref).sum((0, 2, 3)) / ref[0, 0].numel()).numpy()) < 1e-3


S3_CASES = [c for c in CONV_CASES if c[0] in ("3x3_32_32", "3x3d2_64_64_xf", "2x2d2_32", "1x1_cat3", "3x3_cat2_80_32",
                                               "3x3_16_20", "3x3_256_256_small", "1x1_cat2_80_48_xf", "1x1_32_20",
                                               "1x1s2_64_128", "3x3s2_64_128", "7x7_8_64", "7x7_8_64_xf")]


@pytest.mark.parametrize("cfg", [0, 32 | (1 << 8) | (1 << 16), 64 | (1 << 8) | (1 << 16), 32 | (2 << 8) | (1 << 16),
                                 64 | (2 << 8) | (1 << 16), 64 | (1 << 8) | (2 << 16),
                                 32 | (1 << 8) | (1 << 16) | (1 << 24), 64 | (2 << 8) | (1 << 16) | (1 << 24)])
@pytest.mark.parametrize("case", S3_CASES, ids=[c[0] for c in S3_CASES])
def test_conv_fwd_split_bf16_vs_float64(case, cfg):
    """the same convolutions on the bf16 matrix pipe with three-way split operands (conv_fwd.hip PIPE 5): fp32-class
    error against float64 -- within 4x of what the fp32 MFMA path leaves on the same inputs, and below 2e-6."""
    name, N, H, W, cins, Cout, k, dil, pad, stride, act, xf = case
    lib = L.lib()
    xs = [det_tensor("%s.x%d" % (name, i), (N, c, H, W)) for i, c in enumerate(cins)]
    w = det_tensor(name + ".w", (Cout, sum(cins), k, k), -0.2, 0.2)
    b = det_tensor(name + ".b", (Cout,))
    srcs, ref_in = [], []
    for i, (x, c) in enumerate(zip(xs, cins)):
        s = dict(x=G.nhwc(x), C=c)
        xr = x.double()
        if xf:
            sc, sh = det_tensor("%s.sc%d" % (name, i), (c,), 0.5, 1.5), det_tensor("%s.sh%d" % (name, i), (c,))
            cm = (det_tensor("%s.cm%d" % (name, i), (N, c)) > -0.6).float() * 1.25
            s.update(scale=sc.cuda(), shift=sh.cuda(), cmul=cm.cuda().contiguous(), relu=(i % 2 == 0))
            xr = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).double()     # the affine map itself is fp32 on both paths
            if i % 2 == 0:
                xr = xr.clamp_min(0)
            xr = xr * cm[:, :, None, None].double()
        srcs.append(s)
        ref_in.append(xr)
    ref = F.conv2d(torch.cat(ref_in, 1), w.double(), b.double(), stride=stride, padding=pad, dilation=dil)
    if act == 1:
        ref = F.leaky_relu(ref, 0.01)
    OH, OW = ref.shape[2], ref.shape[3]
    ldw = (Cout + 63) // 64 * 64
    b_dev = b.cuda()
    errs = {}
    for kind in ("f32", "s3"):
        out = torch.zeros(N, OH, OW, (Cout + 7) // 8 * 8, device="cuda")
        stem = k == 7 and cins == [8] and os.environ.get("PMF_STEM_DIRECT") != "0"      # (PIPE 14, default since round 6)
        if k == 7 and not stem and kind == "s3":
            continue
        wpk = G.pack_fwd(w, sum(cins), ldw) if kind == "f32" else (
            G.pack_fwd_s3_stem(w, ldw) if stem else G.pack_fwd_s3(w, sum(cins), ldw))
        d = G.conv_desc(srcs, wpk, ldw, b_dev, out, N, OH, OW, Cout, G.taps_of(k, k, dil, pad), stride, act)
        ws = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
        d.cfg = cfg
        if kind == "s3":
            d.w, d.w_s3 = None, wpk.data_ptr()
            assert lib.pmf_conv_s3_eligible(C.byref(d)) == (3 if stem else (2 if k == 1 else 1))   # 2: direct 1x1, 3: stem
        rows = lib.pmf_conv_fwd_stat_rows(C.byref(d))
        stats = _nan_rows(rows + 2, Cout)
        d.stats = stats.data_ptr()
        _sync_check(lib.pmf_conv_fwd(C.byref(d), G.stream()), "pmf_conv_fwd")
        got = G.from_nhwc(out, Cout).double()
        errs[kind] = float((got - ref).abs().max() / ref.abs().max())
        st = _written_rows(stats, rows).sum(0).cpu()
        assert torch.isfinite(st).all()
        assert G.rel_err(st[0].numpy() / ref[0, 0].numel(), (ref.sum((0, 2, 3)) / ref[0, 0].numel()).numpy()) < 1e-5
        if ((cfg >> 16) & 255) > 1 and not (cfg >> 24):
            # the same split-K launch with a ticket array (round 6): the last-arriving workgroup of an output tile combines the
            # slabs INSIDE the kernel -- one launch, statistics rows as without the split, tickets back at zero, and the result
            # does not depend on which workgroup arrived last (three runs, bit for bit)
            tk = torch.zeros(16384, dtype=torch.int32, device="cuda")
            d.splitk_tickets = tk.data_ptr()
            rows_t = lib.pmf_conv_fwd_stat_rows(C.byref(d))
            outs = []
            for rep in range(3):
                out_t = torch.zeros_like(out)
                stats_t = _nan_rows(rows_t + 2, Cout)
                d.out, d.stats = out_t.data_ptr(), stats_t.data_ptr()
                _sync_check(lib.pmf_conv_fwd(C.byref(d), G.stream()), "pmf_conv_fwd (tickets)")
                assert int(tk.abs().sum()) == 0
                outs.append((out_t, _written_rows(stats_t, rows_t)))
            got_t = G.from_nhwc(outs[0][0], Cout).double()
            e_t = float((got_t - ref).abs().max() / ref.abs().max())
            assert e_t < 2e-6 and e_t <= 4 * errs["f32"] + 1e-7, (kind, e_t, errs)
            st_t = outs[0][1].sum(0).cpu()
            assert G.rel_err(st_t[0].numpy() / ref[0, 0].numel(), (ref.sum((0, 2, 3)) / ref[0, 0].numel()).numpy()) < 1e-5
            for o, s_ in outs[1:]:
                assert torch.equal(o, outs[0][0]) and torch.equal(s_, outs[0][1])
            d.splitk_tickets = None
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/s3_conv_errors.txt", "a") as f:
        f.write("%-22s cfg %#8x  f32 %.3e  s3 %.3e\n" % (name, cfg, errs["f32"], errs.get("s3", float("nan"))))
    if "s3" not in errs:
        pytest.skip("stem-class variant switched off (PMF_STEM_DIRECT=0)")
    assert errs["s3"] < 2e-6 and errs["s3"] <= 4 * errs["f32"] + 1e-7, errs


def test_stem_direct_variant_can_be_switched_off():
    """PIPE 14 (stem class: 8 padded channels, two taps per MFMA step, pack format 2) is the default since round 6 (its float64
    pins are the 7x7 cases above: plain and through an operand view with zero padding, every tile configuration);
    PMF_STEM_DIRECT=0 (read once per process) puts the stem back on fp32 MFMA -- the A/B switch keeps working"""
    import subprocess
    import sys
    env = dict(os.environ, PMF_STEM_DIRECT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-k", "split_bf16_vs_float64 and 7x7"],
                       env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " skipped" in r.stdout.splitlines()[-1] and "failed" not in r.stdout, r.stdout[-1500:]


@pytest.mark.parametrize("transpose", [0, 1])
def test_pack_split_bf16_bit_exact(transpose):
    """the batched pack kernel (format 1) against the host packer: same three planes, same fragment slots."""
    lib = L.lib()
    w = det_tensor("pack.s3.w", (48, 32, 3, 3), -0.3, 0.3)
    Cout, Cin = w.shape[0], w.shape[1]
    K, Nn = (Cout, Cin) if transpose else (Cin, Cout)
    k_pad, ldw = (K + 15) // 16 * 16, (Nn + 63) // 64 * 64
    wd = w.cuda()
    dst = torch.zeros(9 * k_pad * ldw * 3, dtype=torch.int16, device="cuda")
    jobs = (L.PackJob * 1)()
    J = jobs[0]
    ct = lib.pmf_pack_tile_ci(Cin, 9)
    J.w, J.dst = wd.data_ptr(), dst.data_ptr()
    J.Cout, J.Cin, J.KHW, J.ntaps, J.transpose = Cout, Cin, 9, 9, transpose
    J.K_pad, J.ldw, J.CT, J.format = k_pad, ldw, ct, 1
    J.tiles_ci = (Cin + ct - 1) // ct
    J.block_start = 0
    for i in range(9):
        J.tap_idx[i] = i
    tab = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
    _sync_check(lib.pmf_pack_weights_batched(tab.data_ptr(), 1, J.tiles_ci * ((Cout + 31) // 32), G.stream()), "pack")
    wl = w.permute(1, 0, 2, 3).contiguous() if transpose else w     # GEMM view: [n][k][kh][kw]
    ref = G.pack_fwd_s3(wl, k_pad, ldw)
    assert torch.equal(dst.view(ref.shape).cpu(), ref.cpu())


# ---------------------------------------------------------------------------------------------- whole network
def _models(backbone="resnet34", ncls=20):
    from pmf_amd.models import PMFNet
    from oracle import pmf_torch as O
    hip = deterministic_init(PMFNet(5, 3, ncls, 32, False, backbone)).cuda()
    ref = deterministic_init(O.PMFNet(5, 3, ncls, 32, False, backbone))
    return hip, ref


def _report(rows, tol):
    bad = [(n, e) for n, e in rows if not e <= tol]
    txt = "\n".join("%-28s %.3e%s" % (n, e, "   <-- FAIL" if not e <= tol else "") for n, e in rows)
    return bad, txt


@pytest.mark.parametrize("backbone,ncls,n,h,w", [("resnet34", 20, 2, 32, 64), ("resnet34", 20, 1, 64, 512),
                                                 ("resnet50", 17, 1, 32, 64)])
def test_eval_forward_matches_oracle(backbone, ncls, n, h, w, golden):
    hip, ref = _models(backbone, ncls)
    hip.eval()
    ref.eval()
    pcd, rgb, _, _ = synthetic_batch(n, h, w, ncls, seed=1)
    cap, hs = G.capture_oracle(ref)
    with torch.no_grad():
        rl, rc = ref(pcd, rgb)
        # strided channel views of one [N,8,H,W] tensor, like tasks/pmf/trainer.py:296-297
        both = torch.cat((pcd, rgb), 1).cuda()
        lp, cp = hip(both[:, 0:5], both[:, 5:8])
    torch.cuda.synchronize()
    plan = next(iter(hip._plans.values()))
    rows = G.compare_plan_to_oracle(plan, cap)
    _dump("eval_fwd_%s_%d_%d_%d.txt" % (backbone, n, h, w), rows)
    bad, txt = _report(rows, 1e-3)
    assert not bad, "intermediate mismatch (rel err, oracle order):\n" + txt
    assert (lp.cpu() - rl).abs().max() < 1e-4 and (cp.cpu() - rc).abs().max() < 1e-4
    if (backbone, n, h, w) == ("resnet34", 2, 32, 64):      # also straight against the reference-run fixture
        g = golden("g3_wholenet")
        lg = plan.read(plan.tensors["logits"]).cpu().numpy()
        assert G.rel_err(lg, g["r34.eval.lidar_logits"]) < 1e-3
        assert np.abs(cp.cpu().numpy() - g["r34.eval.cam_prob"]).max() < 1e-4
    if backbone == "resnet50":
        g = golden("g3_wholenet")
        lg = plan.read(plan.tensors["logits"]).cpu().numpy()
        assert G.rel_err(lg, g["r50.eval.lidar_logits"]) < 1e-3


def test_precision_probe_split_bf16_vs_fp32_mfma():
    """BASELINE.md's precision probe (eval forward, deterministic init, pre-softmax logits against float64) on both
    arithmetic paths of the conv kernels: v_mfma_f32_32x32x2_f32 (PMF_CONV_F32=1) and the three-way split on the bf16
    matrix pipe (default).  Both must sit at fp32 rounding level -- three orders of magnitude below what bf16 inputs
    leave (1.8e-3 in BASELINE.md) -- and the split path within 3x of the fp32 pipe."""
    import copy
    from pmf_amd.models import PMFNet
    from oracle import pmf_torch as O
    n, h, w = 1, 64, 512
    pcd, rgb, _, _ = synthetic_batch(n, h, w, 20, seed=1)
    ref64 = deterministic_init(O.PMFNet(5, 3, 20, 32, False, "resnet34")).double().eval()
    with torch.no_grad():
        ref64(pcd.double(), rgb.double())
    want = ref64.lidar_stream.last_logits.detach()
    errs = {}
    for tag, env in (("split_bf16", None), ("fp32_mfma", "1")):
        if env is None:
            os.environ.pop("PMF_CONV_F32", None)
        else:
            os.environ["PMF_CONV_F32"] = env
        try:
            hip = deterministic_init(PMFNet(5, 3, 20, 32, False, "resnet34")).cuda().eval()
            with torch.no_grad():
                hip(pcd.cuda(), rgb.cuda())
            torch.cuda.synchronize()
            plan = next(iter(hip._plans.values()))
            n_split = sum(1 for i in range(plan.n_fwd) if plan.fwd_kinds[i] == L.OP_CONV and plan.fwd_ops[i].u.conv.w_s3)
            assert (n_split > 60) == (env is None)      # (3x3 / 2x2 staged split kernels + direct 1x1 variant; the stem and ragged layers stay on fp32 MFMA)
            got = plan.read(plan.tensors["logits"]).cpu().double()
            errs[tag] = ((got - want).abs().max().item(), want.abs().max().item())
        finally:
            os.environ.pop("PMF_CONV_F32", None)
    _dump("precision_probe.txt", [(k, v[0], v[1]) for k, v in errs.items()])
    e3, ef = errs["split_bf16"][0], errs["fp32_mfma"][0]
    scale = errs["split_bf16"][1]
    assert ef < 2e-5 * max(scale, 1.0) and e3 < 2e-5 * max(scale, 1.0), errs
    assert e3 <= 3 * ef + 1e-6, errs


def _masks(ref, n, seed=3):
    from oracle import pmf_torch as O
    g = torch.Generator().manual_seed(seed)
    return {nm: (torch.rand(n, c, generator=g) > 0.2).float() / 0.8 for nm, _, c in O.dropout_sites(ref)}


def _dump(name, rows):
    import os
    os.makedirs("gpurun_out", exist_ok=True)
    with open(os.path.join("gpurun_out", name), "w") as f:
        for r in rows:
            f.write("  ".join(("%-52s" % x) if isinstance(x, str) else ("%.3e" % x) for x in r) + "\n")


# (rounds 1-5 ran the first two cases at 2 x 32 x 64: the deepest BatchNorm layers normalise over 16 values there, which amplifies
# ANY fp32 rounding into 1e-3..1e-2 of the gradients -- also with every product on fp32 MFMA, gpurun_out/r06e -- so no bar tighter
# than the old "x20" can hold at that size; at 2 x 64 x 128 (64 values) the full-size bar does)
@pytest.mark.parametrize("n,h,w,drop", [(2, 64, 128, False), (2, 64, 128, True), (1, 64, 512, True)])
def test_train_step_matches_oracle(n, h, w, drop):
    """forward (batch-stat BN, Dropout2d masks), 5-term loss, backward.  Ground truth = the oracle in FLOAT64;
    the HIP fp32 gradients must be as close to it as the fp32 CPU oracle is (up to a small factor): tiny-batch
    BatchNorm makes the backward pass ill-conditioned, so fp32-vs-fp32 differences are not a bug signal."""
    import copy
    from oracle import pmf_torch as O
    from oracle import losses_ref
    hip, ref = _models()
    hip.train()
    ref.train()
    if drop:
        m = _masks(ref, n)
    else:
        m = {nm: torch.ones(n, c) for nm, _, c in O.dropout_sites(ref)}
    O.set_dropout_masks(ref, m)
    hip.set_dropout_masks({k: v.cuda() for k, v in m.items()})
    ref64 = copy.deepcopy(ref).double()
    O.set_dropout_masks(ref64, {k: v.double() for k, v in m.items()})
    pcd, rgb, label, _ = synthetic_batch(n, h, w, 20, seed=1)
    alpha = torch.linspace(0.2, 1.0, 20)
    alpha[0] = 0
    cap, hs = G.capture_oracle(ref)
    rl, rc = ref(pcd, rgb)
    total_r, _ = losses_ref.pmf_total_loss(rl, rc, label, alpha)
    total_r.backward()
    dl, dc = ref64(pcd.double(), rgb.double())
    total_d, _ = losses_ref.pmf_total_loss(dl, dc, label, alpha.double())
    total_d.backward()
    lp, cp = hip(pcd.cuda(), rgb.cuda())
    lp.retain_grad()
    cp.retain_grad()
    total_h, _ = losses_ref.pmf_total_loss(lp, cp, label.cuda(), alpha.cuda())   # same torch ops, on the GPU
    total_h.backward()
    torch.cuda.synchronize()
    plan = next(iter(hip._plans.values()))
    skip = [k for k in cap if drop and (k.startswith("upBlock") or k.startswith("resBlock5"))]
    rows = G.compare_plan_to_oracle(plan, cap, skip)
    _dump("train_fwd_%d_%d_%d_%d.txt" % (n, h, w, drop), rows)
    bad, txt = _report(rows, 1e-3)
    assert not bad, "train-mode forward mismatch:\n" + txt
    assert G.rel_err(plan.read(plan.tensors["logits"]).cpu().numpy(), dl.new_tensor(ref64.lidar_stream.last_logits).numpy()) < 1e-3
    assert abs(total_h.item() - total_d.item()) < 1e-4 * max(1.0, abs(total_d.item()))
    rsd = ref.state_dict()
    for k, v in hip.state_dict().items():
        if "running_" in k:
            assert G.scale_err(v.cpu().numpy(), rsd[k].numpy()) < 1e-4, k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(rsd[k]) == 1
    # gradients: LeakyReLU / ReLU derivatives are discontinuous -- ONE pre-activation within rounding distance of zero flips a
    # slope and moves the gradients upstream of it by 1e-3..1e-2 (rounds 1-5 carried a 5e-2 / "85 % within x20" allowance for
    # that here).  Round 6: the float64 and fp32 oracle passes replay the HIP path's decisions and upstream gradient
    # (G.masked_grad_rows), and EVERY parameter is held to max(3 x the fp32 oracle's distance from float64, 2e-4)
    rows = G.masked_grad_rows(hip, plan, _models()[1], m, pcd, rgb, (lp.grad, cp.grad))
    _dump("train_grads_%d_%d_%d_%d.txt" % (n, h, w, drop), rows)
    G.assert_masked_bar(rows, "train step %dx%dx%d" % (n, h, w))


@pytest.mark.parametrize("tag,seed,h,w,npts,q", [("a", 11, 64, 512, 20000, False), ("b", 12, 48, 160, 6000, False),
                                                 ("ties", 13, 32, 64, 3000, True), (None, 21, 384, 1232, 130000, False),
                                                 (None, 22, 64, 2048, 40000, True)])
def test_knn_labels_exact(tag, seed, h, w, npts, q, golden):
    from pmf_amd.postproc import KNN
    from oracle import knn_ref
    from oracle.cases import knn_case
    pr, ur, am, px, py = knn_case(seed, h, w, npts, q)
    knn = KNN({"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}, 20)
    t = lambda a: torch.from_numpy(a).cuda()
    got = knn(t(pr), t(ur), t(am), t(px), t(py)).cpu().numpy()
    np.testing.assert_array_equal(got, knn_ref.knn_vote(pr, ur, am, px, py))
    if tag is not None and not q:
        np.testing.assert_array_equal(got, golden("g4_knn")["knn.%s.labels" % tag].astype(np.int64))


def test_knn_errors():
    from pmf_amd.postproc import KNN
    z = torch.zeros(4, 4).cuda()
    with pytest.raises(ValueError):
        KNN({"knn": 5, "search": 4, "sigma": 1.0, "cutoff": 1.0}, 20)(z, z[0], z.long(), z[0].long(), z[0].long())
    with pytest.raises(ValueError):
        KNN({"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}, 20)(z, z[0], z.long(), z[0, :2].long(), z[0].long())


# ---------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("tag,seed,npts,h,w", [("a", 0, 5000, 96, 320), ("b", 5, 20000, 64, 208),
                                               (None, 8, 120000, 376, 1241), (None, 9, 0, 32, 64)])
def test_projection_scatter_exact(tag, seed, npts, h, w, golden):
    from pmf_amd.dataset import project_frame_gpu, center_crop_pad_gpu
    from oracle import loader_ref
    M, pts, sem, img, lut = loader_ref.synthetic_frame(seed, max(npts, 20), h, w)
    if npts == 0:
        pts, sem = pts[:0], sem[:0]
    proj, xd, yd, depth, keep = project_frame_gpu(pts, sem, img, M, lut)
    rp, rx, ry, rd = loader_ref.project_frame(pts, sem, img, M, lut)
    np.testing.assert_array_equal(xd.cpu().numpy(), rx)
    np.testing.assert_array_equal(yd.cpu().numpy(), ry)
    np.testing.assert_array_equal(depth.cpu().numpy(), rd)
    np.testing.assert_array_equal(proj.cpu().numpy(), rp)
    if tag:
        np.testing.assert_array_equal(proj.cpu().numpy(), golden("g5_loader")["loader.%s.proj" % tag])
    # validation crop + pad window (perspective_view_loader.py:71-74)
    for (oh, ow, hp, wp) in ((h - 8, w - 16, 3, 5), (h + 14, w + 6, 7, 3)):
        got = center_crop_pad_gpu(proj, oh, ow, hp, wp).cpu().numpy()
        np.testing.assert_array_equal(got, loader_ref.center_crop_pad(rp, oh, ow, hp, wp))


def test_projection_two_launch_form_reuses_its_workspace(monkeypatch):
    """pmf_project_scatter2 (projection + ordered compaction + scatter in ONE kernel, gather in a second; the per-pixel
    winner table is never cleared, entries carry the call's generation): a run of DIFFERENT frames of one image size through
    the same persistent workspace -- incl. the generation wrap at 4095 and an empty sweep -- against the numpy oracle, and the
    legacy five-launch form (PMF_PROJECT_LEGACY=1) on the same frames"""
    from pmf_amd.dataset import project_frame_gpu, perspective_view_loader as PV
    from oracle import loader_ref
    h, w = 96, 320
    frames = [loader_ref.synthetic_frame(seed, n, h, w) for seed, n in ((1, 30000), (2, 2500), (3, 61000), (4, 1100), (5, 9000))]
    project_frame_gpu(*[frames[0][i] for i in (1, 2, 3, 0, 4)])              # creates this thread's workspace
    ws = PV._PROJ_TLS.ws[(str(torch.device("cuda")), h, w, int(torch.cuda.current_stream().cuda_stream))]
    ws[2] = 4092                                                             # ... three calls before the wrap
    for rep in range(2):
        for k, (M, pts, sem, img, lut) in enumerate(frames):
            if rep == 1 and k == 2:
                pts, sem = pts[:0], sem[:0]                                    # a frame with no points at all
            proj, xd, yd, depth, keep = project_frame_gpu(pts, sem, img, M, lut)
            rp, rx, ry, rd = loader_ref.project_frame(pts, sem, img, M, lut)
            np.testing.assert_array_equal(proj.cpu().numpy(), rp)
            np.testing.assert_array_equal(xd.cpu().numpy(), rx)
            np.testing.assert_array_equal(yd.cpu().numpy(), ry)
            np.testing.assert_array_equal(depth.cpu().numpy(), rd)
            assert int(keep.sum()) == rx.shape[0]
    assert 1 <= ws[2] <= 10                                                   # the counter wrapped and restarted
    monkeypatch.setenv("PMF_PROJECT_LEGACY", "1")
    M, pts, sem, img, lut = frames[2]
    a = project_frame_gpu(pts, sem, img, M, lut)
    monkeypatch.delenv("PMF_PROJECT_LEGACY")
    b = project_frame_gpu(pts, sem, img, M, lut)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # a second stream gets a workspace of its own (calls of one thread on two streams may overlap on the GPU: ADVICE r04)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = project_frame_gpu(pts, sem, img, M, lut)
    side.synchronize()
    assert len([k for k in PV._PROJ_TLS.ws if k[1:3] == (h, w)]) == 2      # (other tests of this process left theirs)
    for x, y in zip(b, c):
        assert torch.equal(x, y)
    # a ticket counter that is not 0 on entry (unzeroed / foreign workspace, an aborted call) must neither write
    # out of bounds nor hang the device: the call reports it (n_kept = -1 -> RuntimeError), leaves the counter at 0, and the
    # next call on a fresh workspace is exact again
    ws = PV._PROJ_TLS.ws[(str(torch.device("cuda")), h, w, int(torch.cuda.current_stream().cuda_stream))]
    ws[1][0] = 7
    with pytest.raises(RuntimeError, match="ticket workspace"):
        project_frame_gpu(pts, sem, img, M, lut)
    torch.cuda.synchronize()
    assert int(ws[1][0]) == 0
    d = project_frame_gpu(pts, sem, img, M, lut)
    for x, y in zip(b, d):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------- losses
def test_losses_gpu_match_cpu_and_fixture(golden):
    """product loss modules on the GPU (incl. the HIP Lovasz Jaccard-gradient kernel) vs the same ops on CPU and the
    reference-run fixture: values and gradients w.r.t. the logits."""
    from pmf_amd.loss import FocalSoftmaxLoss, Lovasz_softmax, pmf_total_loss
    g = golden("g6_losses")
    n, c, h, w = 2, 20, 16, 32
    a0, b0 = det_tensor("g6.logits", (n, c, h, w), -3, 3), det_tensor("g6.logits2", (n, c, h, w), -3, 3)
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=3, fill=0.4)
    alpha = np.linspace(0.2, 1.0, c).astype(np.float32)
    alpha[0] = 0
    a, b = a0.cuda().requires_grad_(True), b0.cuda().requires_grad_(True)
    foc, lov = FocalSoftmaxLoss(c, gamma=2, alpha=alpha, softmax=False).cuda(), Lovasz_softmax(ignore=0)
    total, t = pmf_total_loss(torch.softmax(a, 1), torch.softmax(b, 1), label.cuda(), foc, lov)
    total.backward()
    vals = np.array([total.item()] + [t[k].item() for k in ("foc", "lov", "foc_cam", "lov_cam", "per")])
    assert np.abs(vals - g["loss.values"]).max() < 5e-6
    assert np.abs(a.grad.cpu().numpy() - g["loss.grad_a"]).max() < 5e-7
    assert np.abs(b.grad.cpu().numpy() - g["loss.grad_b"]).max() < 5e-7
    # bench-size row lengths (262144 pixels): HIP Jaccard gradient vs the torch formula
    from pmf_amd.loss.lovasz_softmax import _jaccard_grad
    torch.manual_seed(0)
    fg = (torch.rand(20, 262144) < 0.07).float()
    nvalid = 200000
    nv = (torch.arange(262144) < nvalid).float()[None].expand(20, -1)
    fg = fg * nv
    ref = _jaccard_grad(fg, nv, torch.tensor(nvalid))
    got = _jaccard_grad(fg.cuda(), nv.cuda(), torch.tensor(nvalid).cuda()).cpu()
    assert (got - ref).abs().max() < 1e-6


@pytest.mark.gpu
def test_fused_loss_matches_reference_objective(golden):
    """the fused HIP objective (value, analytic gradient w.r.t. both probability maps, confusion matrices) against
    (1) the reference-run fixture g6_losses and (2) float64 autograd of the torch-op restatement, incl. a bench-size
    map with ignored pixels and a class that is absent."""
    from pmf_amd.loss import FocalSoftmaxLoss, Lovasz_softmax, pmf_total_loss, pmf_total_loss_fused
    from pmf_amd.metrics import IOUEval
    g = golden("g6_losses")
    n, c, h, w = 2, 20, 16, 32
    a0, b0 = det_tensor("g6.logits", (n, c, h, w), -3, 3), det_tensor("g6.logits2", (n, c, h, w), -3, 3)
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=3, fill=0.4)
    alpha = np.linspace(0.2, 1.0, c).astype(np.float32)
    alpha[0] = 0
    a, b = a0.cuda().requires_grad_(True), b0.cuda().requires_grad_(True)
    total, t = pmf_total_loss_fused(torch.softmax(a, 1), torch.softmax(b, 1), label.cuda(), torch.from_numpy(alpha))
    total.backward()
    vals = np.array([total.item()] + [t[k].item() for k in ("foc", "lov", "foc_cam", "lov_cam", "per")])
    assert np.abs(vals - g["loss.values"]).max() < 5e-6, (vals, g["loss.values"])
    assert np.abs(a.grad.cpu().numpy() - g["loss.grad_a"]).max() < 5e-7
    assert np.abs(b.grad.cpu().numpy() - g["loss.grad_b"]).max() < 5e-7

    for (n, h, w, fill, drop_cls) in ((1, 8, 32, 0.7, None), (2, 64, 2048, 0.25, 7)):
        la, lb = det_tensor("fl.a", (n, c, h, w), -4, 4), det_tensor("fl.b", (n, c, h, w), -4, 4)
        _, _, label, _ = synthetic_batch(n, h, w, c, seed=5, fill=fill)
        if drop_cls is not None:
            label = torch.where(label == drop_cls, torch.zeros_like(label), label)
        pa = torch.softmax(la.double(), 1).requires_grad_(True)
        pb = torch.softmax(lb.double(), 1).requires_grad_(True)
        foc, lov = FocalSoftmaxLoss(c, gamma=2, alpha=alpha, softmax=False).double(), Lovasz_softmax(ignore=0)
        ref, rt = pmf_total_loss(pa, pb, label.long(), foc, lov, 1.0, 0.5, 0.7)
        ref.backward()
        ga, gb = pa.detach().float().cuda().requires_grad_(True), pb.detach().float().cuda().requires_grad_(True)
        ml, mc = IOUEval(c, "cuda", ignore=[0]), IOUEval(c, "cuda", ignore=[0])
        tot, tt = pmf_total_loss_fused(ga, gb, label.cuda(), torch.from_numpy(alpha), 1.0, 0.5, 0.7, 2.0,
                                       ml.conf_matrix, mc.conf_matrix)
        tot.backward()
        assert abs(tot.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item()))
        for k in ("foc", "lov", "foc_cam", "lov_cam", "per"):
            assert abs(tt[k].item() - rt[k].item()) < 2e-6 * max(1.0, abs(rt[k].item())), k
        for got, want in ((ga.grad, pa.grad), (gb.grad, pb.grad)):
            err = (got.cpu().double() - want).abs().max().item()
            assert err < 1e-6 * max(want.abs().max().item(), 1e-3) + 1e-9, err
        rl, rc = IOUEval(c, "cpu", ignore=[0]), IOUEval(c, "cpu", ignore=[0])
        rl.addBatch(pa.argmax(1), label)
        rc.addBatch(pb.argmax(1), label)
        assert torch.equal(ml.conf_matrix.cpu(), rl.conf_matrix) and torch.equal(mc.conf_matrix.cpu(), rc.conf_matrix)


@pytest.mark.gpu
def test_fused_loss_nan_probabilities_stay_in_bounds():
    """diverged training: NaN probabilities must give a NaN loss, not out-of-bounds scatters (the in-library
    Lovasz sort used to drop NaN keys in pass 0, leaving row tails of the permutation unwritten)"""
    from pmf_amd.loss import pmf_total_loss_fused
    n, c, h, w = 2, 20, 64, 512
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=5, fill=0.5)
    alpha = np.linspace(0.2, 1.0, c).astype(np.float32)
    alpha[0] = 0
    for _ in range(3):
        a = torch.softmax(det_tensor("nan.a", (n, c, h, w), -3, 3), 1)
        b = torch.softmax(det_tensor("nan.b", (n, c, h, w), -3, 3), 1)
        a[0, :, 10:20, 100:200] = float("nan")
        b[1, 3, :, :] = float("nan")
        ga, gb = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        tot, _ = pmf_total_loss_fused(ga, gb, label.cuda(), torch.from_numpy(alpha))
        tot.backward()
        torch.cuda.synchronize()
        assert not torch.isfinite(tot).item()
        assert ga.grad.shape == a.shape
    # and the library still works afterwards (no sticky fault)
    a = torch.softmax(det_tensor("nan.a", (n, c, h, w), -3, 3), 1).cuda().requires_grad_(True)
    b = torch.softmax(det_tensor("nan.b", (n, c, h, w), -3, 3), 1).cuda().requires_grad_(True)
    tot, _ = pmf_total_loss_fused(a, b, label.cuda(), torch.from_numpy(alpha))
    tot.backward()
    assert torch.isfinite(tot).item() and torch.isfinite(a.grad).all()


@pytest.mark.gpu
def test_flat_training_state_matches_per_tensor_path():
    """FlatState (parameters / gradients as views of two flat buffers, gradients written in place by the backward plan) must
    produce bit-identical parameters to the per-tensor path when both step with the same optimiser kernels (torch's fused
    AdamW / SGD: PMF_OWN_OPTIM=0 on the flat side).  With the range optimiser of libpmf_amd.so -- the default on the flat
    state -- the same trajectory to float32 rounding of the update arithmetic."""
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init

    def run(flat, own="1"):
        torch.manual_seed(0)
        m = PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34")
        deterministic_init(m)
        m = m.cuda()
        os.environ["PMF_OWN_OPTIM"] = own
        try:
            eng = TrainEngine(m, 20, lr=1e-3, warmup_steps=2, max_steps=10, flat_state=flat)
        finally:
            os.environ.pop("PMF_OWN_OPTIM", None)
        pcd, rgb, label, mask = synthetic_batch(2, 32, 64, 20, seed=11, fill=0.5)
        feat = torch.cat((pcd, rgb), 1)
        torch.manual_seed(123)                       # same dropout masks in both runs
        torch.cuda.manual_seed(123)
        losses = []
        for _ in range(3):
            tot, _ = eng.train_step(feat.cuda().clone(), mask.cuda(), label.cuda())
            losses.append(tot.item())
        conf = eng.metrics.conf_matrix.clone()
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, conf

    l0, s0, c0 = run(False)
    l1, s1, c1 = run(True, own="0")
    assert l0 == l1, (l0, l1)
    assert torch.equal(c0, c1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    l2, s2, c2 = run(True)                       # range optimiser
    assert l2[0] == l0[0] and all(abs(a - b) < 1e-4 * abs(b) for a, b in zip(l2, l0)), (l2, l0)
    # camera stream (SGD: linear in the gradient) convolution weights stay within rounding; AdamW (LiDAR stream) turns the
    # last-bit difference of a near-zero gradient element into a full +-lr step, so there only the bound that follows from
    # three steps of at most lr each holds (one step: test_range_optimiser_equals_torch_fused_step compares everything)
    errs = sorted(((((s2[k] - s0[k]).abs().max() / s0[k].abs().max().clamp_min(1e-6)).item(), k)
                   for k in s0 if s0[k].dim() == 4 and k.startswith("camera_stream")), reverse=True)
    assert errs and errs[0][0] < 1e-3, errs[:6]
    lr_sum = 1e-3 * (1 + 2 + 2) / 2 * 1.05
    assert all((s2[k] - s0[k]).abs().max().item() <= 2 * lr_sum for k in s0 if k.startswith("lidar_stream") and s0[k].dim() == 4)


@pytest.mark.gpu
def test_data_parallel_range_allreduce_world1():
    """distributed=True on one rank (RCCL, world 1): the backward plan runs in segments, finished gradient ranges are
    all-reduced between them (identity here) -- the parameters after 3 steps must equal the single-process run."""
    import torch.distributed as dist
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        def run(distributed):
            m = PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34")
            deterministic_init(m)
            m = m.cuda()
            eng = TrainEngine(m, 20, lr=1e-3, warmup_steps=2, max_steps=10, distributed=distributed, device_ids=[0])
            pcd, rgb, label, mask = synthetic_batch(2, 32, 64, 20, seed=11, fill=0.5)
            feat = torch.cat((pcd, rgb), 1)
            torch.manual_seed(7)
            torch.cuda.manual_seed(7)
            for _ in range(3):
                eng.train_step(feat.cuda().clone(), mask.cuda(), label.cuda())
            plan = next(iter(m._plans.values()))
            if distributed and os.environ.get("PMF_DP_MODE") == "events":
                gates = plan.dp_gates()
                assert gates and all(evs for _, evs in gates) and all(a[0] < b[0] for a, b in zip(gates, gates[1:]))
            cuts = plan.segment_cuts(4)
            assert cuts[0] == 0 and cuts[-1] == plan.n_bwd and all(a < b for a, b in zip(cuts, cuts[1:]))
            fr = [plan.grad_frontier(c) for c in cuts[1:]]
            assert fr[-1] == [b for (_, b) in plan.flat.ranges]           # everything final at the end
            assert all(x <= y for f0, f1 in zip(fr, fr[1:]) for x, y in zip(f0, f1))   # frontiers only advance
            return {k: v.detach().clone() for k, v in m.state_dict().items()}
        a = run(False)
        # both data-parallel forms: all-reduce hung behind plan events of ONE backward range (default), and the backward
        # plan cut into segments (PMF_DP_MODE=segments)
        for mode in ("events", "segments"):
            os.environ["PMF_DP_MODE"] = mode
            try:
                b = run(True)
            finally:
                os.environ.pop("PMF_DP_MODE", None)
            for k in a:
                assert torch.equal(a[k], b[k]), (mode, k)
    finally:
        if created:
            dist.destroy_process_group()


# ---- EPMF ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_epmf_eval_and_train_match_oracle(golden):
    """EPMFNet on the HIP plan (SparseVariantConv masks in the conv epilogue, stride-2 context block, extraUpSample,
    LiDAR feature into the camera decoder) against the reference-run fixture g8_epmf (eval logits) and the float64
    oracle (train: loss, running statistics, gradients of every parameter)."""
    import copy
    from pmf_amd.models import EPMFNet
    from oracle import epmf_torch as E
    from oracle import pmf_torch as O
    from oracle import losses_ref
    g = golden("g8_epmf")
    hip = deterministic_init(EPMFNet(5, 3, 20, 32, False, "resnet34")).cuda()
    ref = deterministic_init(E.EPMFNet(5, 3, 20, 32, False, "resnet34"))
    assert sorted(hip.state_dict().keys()) == list(g["keys"])
    n, h, w = 2, 64, 128
    pcd, rgb, label, _ = synthetic_batch(n, h, w, 20, seed=1, fill=0.3)
    hip.eval()
    ref.eval()
    with torch.no_grad():
        rl, rc = ref(pcd, rgb)
        lp, cp = hip(pcd.cuda(), rgb.cuda())
    plan = next(iter(hip._plans.values()))
    assert G.rel_err(plan.read(plan.tensors["logits"]).cpu().numpy(), g["eval.lidar_logits"]) < 1e-3
    assert G.rel_err(plan.read(plan.tensors["dec.logits"]).cpu().numpy(), g["eval.cam_logits"]) < 1e-3
    assert (lp.cpu() - rl).abs().max() < 1e-4 and (cp.cpu() - rc).abs().max() < 1e-4
    # ---- train step, dropout on with injected masks
    hip.train()
    ref.train()
    m = _masks(ref, n)
    O.set_dropout_masks(ref, m)
    hip.set_dropout_masks({k: v.cuda() for k, v in m.items()})
    ref64 = copy.deepcopy(ref).double()
    O.set_dropout_masks(ref64, {k: v.double() for k, v in m.items()})
    alpha = torch.linspace(0.2, 1.0, 20)
    alpha[0] = 0
    rl, rc = ref(pcd, rgb)
    losses_ref.pmf_total_loss(rl, rc, label, alpha)[0].backward()
    dl, dc = ref64(pcd.double(), rgb.double())
    total_d, _ = losses_ref.pmf_total_loss(dl, dc, label, alpha.double())
    total_d.backward()
    lp, cp = hip(pcd.cuda(), rgb.cuda())
    lp.retain_grad()
    cp.retain_grad()
    total_h, _ = losses_ref.pmf_total_loss(lp, cp, label.cuda(), alpha.cuda())
    total_h.backward()
    torch.cuda.synchronize()
    plan = [p for p in hip._plans.values() if p.training][0]
    assert G.rel_err(plan.read(plan.tensors["logits"]).cpu().numpy(), ref64.lidar_stream.last_logits.detach().float().numpy()) < 1e-3
    assert abs(total_h.item() - total_d.item()) < 1e-4 * max(1.0, abs(total_d.item()))
    rsd = ref.state_dict()
    for k, v in hip.state_dict().items():
        if "running_" in k:
            assert G.scale_err(v.cpu().numpy(), rsd[k].numpy()) < 1e-4, k
    # every parameter, decisions of the HIP path replayed by both oracle passes (see test_train_step_matches_oracle)
    rows = G.masked_grad_rows(hip, plan, deterministic_init(E.EPMFNet(5, 3, 20, 32, False, "resnet34")), m, pcd, rgb,
                              (lp.grad, cp.grad))
    _dump("epmf_train_grads.txt", rows)
    G.assert_masked_bar(rows, "EPMF train step")


@pytest.mark.gpu
def test_r50_train_step_matches_oracle():
    """BASELINE configs[3] family: PMF-ResNet50 (Bottleneck blocks, 17 classes) forward + backward against the float64
    oracle (same criteria as the ResNet34 train-step test)."""
    import copy
    from oracle import pmf_torch as O
    from oracle import losses_ref
    hip, ref = _models("resnet50", 17)
    hip.train()
    ref.train()
    n, h, w = 2, 64, 64        # 32 values per channel at the deepest BatchNorm (1 x 32 x 64 leaves 8: pure noise)
    m = _masks(ref, n)
    O.set_dropout_masks(ref, m)
    hip.set_dropout_masks({k: v.cuda() for k, v in m.items()})
    ref64 = copy.deepcopy(ref).double()
    O.set_dropout_masks(ref64, {k: v.double() for k, v in m.items()})
    pcd, rgb, label, _ = synthetic_batch(n, h, w, 17, seed=1, fill=0.4)
    alpha = torch.linspace(0.2, 1.0, 17)
    alpha[0] = 0
    rl, rc = ref(pcd, rgb)
    losses_ref.pmf_total_loss(rl, rc, label, alpha)[0].backward()
    dl, dc = ref64(pcd.double(), rgb.double())
    total_d, _ = losses_ref.pmf_total_loss(dl, dc, label, alpha.double())
    total_d.backward()
    lp, cp = hip(pcd.cuda(), rgb.cuda())
    lp.retain_grad()
    cp.retain_grad()
    total_h, _ = losses_ref.pmf_total_loss(lp, cp, label.cuda(), alpha.cuda())
    total_h.backward()
    torch.cuda.synchronize()
    assert abs(total_h.item() - total_d.item()) < 1e-4 * max(1.0, abs(total_d.item()))
    # every parameter, decisions of the HIP path replayed by both oracle passes (see test_train_step_matches_oracle)
    plan = [p for p in hip._plans.values() if p.training][0]
    rows = G.masked_grad_rows(hip, plan, _models("resnet50", 17)[1], m, pcd, rgb, (lp.grad, cp.grad))
    _dump("r50_train_grads.txt", rows)
    G.assert_masked_bar(rows, "PMF-R50 train step")


@pytest.mark.gpu
def test_loader_v2_matches_oracle_and_fixture(golden):
    """EPMF loader on the GPU (pmf_project_v2_*): keep mask, float64 (row, col), depth and the [10,h,w] frame are
    bit-exact against the reference-run fixture and the numpy oracle; validation pad + centre crop vs the oracle."""
    from oracle import loader_ref, loader_v2_ref
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    g = golden("g9_loader_v2")
    for tag, seed, npts, h, w in (("a", 0, 5000, 96, 320), ("b", 5, 20000, 64, 208), ("c", 9, 130000, 376, 1241)):
        M, pts, sem, img, lut = loader_ref.synthetic_frame(seed, npts, h, w)

        class DS:
            proj_matrix = {"00": M}
            class_map_lut = lut
            def loadDataByIndex(self, i): return pts, sem, np.zeros_like(sem)
            def loadImage(self, i): return img
            def parsePathInfoByIndex(self, i): return "00", "000000"
            def __len__(self): return 1
        cfg = {"PVconfig": {"proj_h": h, "proj_w": w, "proj_ht": h, "proj_wt": w}}
        proj, xy, depth, keep, pc = PerspectiveViewLoaderV2(DS(), cfg, is_train=False, return_uproj=True)[0]
        rp, rxy, rd, rk = loader_v2_ref.project_frame_v2(pts, sem, img, M, lut)
        assert np.array_equal(keep.cpu().numpy(), rk)
        assert np.array_equal(xy.cpu().numpy(), rxy)
        assert np.array_equal(depth.cpu().numpy(), rd)
        assert np.array_equal(proj.cpu().numpy(), rp)
        if tag in ("a", "b"):
            assert np.array_equal(proj.cpu().numpy(), g["v2.%s.proj" % tag])
            assert np.array_equal(xy.cpu().numpy(), g["v2.%s.xy" % tag])
        val = PerspectiveViewLoaderV2(DS(), cfg, is_train=False)[0]
        assert np.array_equal(val.cpu().numpy(), loader_v2_ref.pad_center_crop(rp, h, w, h, w))
        # training path: random rescale (numpy RNG + PIL bilinear), scaled coordinates, pad, flip / rotate / crop
        from PIL import Image
        from oracle import tensor_aug_ref as T
        tcfg = {"PVconfig": {"proj_h": h, "proj_w": w, "proj_ht": h - 16, "proj_wt": w - 32}}
        np.random.seed(40 + seed)
        torch.manual_seed(40 + seed)
        got = PerspectiveViewLoaderV2(DS(), tcfg, is_train=True)[0].cpu()
        np.random.seed(40 + seed)
        torch.manual_seed(40 + seed)
        sc = np.random.uniform(low=1.0, high=1.2)
        big = np.asarray(Image.fromarray(img).resize((int(w * sc), int(h * sc)), Image.BILINEAR))
        tp, txy, _, _ = loader_v2_ref.project_frame_v2(pts, sem, big, M, lut, sc)
        fh, fw = tp.shape[1:]
        mh, mw = max(h - 16, fh), max(w - 32, fw)
        left = (mw - fw) // 2
        padded = F.pad(torch.from_numpy(tp), (left, mw - fw - left, 0, mh - fh))
        flip, angle, top, lft = T.draw_params(mh, mw, h - 16, w - 32)
        want = T.flip_rotate_crop(padded, flip, angle, top, lft, h - 16, w - 32)
        assert got.shape == want.shape == (10, h - 16, w - 32)
        nbad = int((got != want).any(0).sum())
        assert nbad <= 1e-4 * got[0].numel() + 2, (tag, nbad)           # rounding-edge pixels of the rotation only
        pu = PerspectiveViewLoaderV2(DS(), tcfg, is_train=True, return_uproj=True)
        np.random.seed(40 + seed)
        assert np.array_equal(pu[0][1].cpu().numpy(), txy)              # scaled float64 (row, col), bit for bit
    # img_aug (perspective_view_loader_v2.py:19-23,46-47): ColorJitter(*PVconfig.img_jitter) before everything else
    from oracle import color_jitter_ref as CJ
    jcfg = {"PVconfig": dict(cfg["PVconfig"], img_jitter=[0.4, 0.4, 0.4, 0.1])}
    torch.manual_seed(77)
    got = PerspectiveViewLoaderV2(DS(), jcfg, is_train=False, img_aug=True)[0]
    torch.manual_seed(77)
    order, fac = CJ.draw_params(CJ.jitter_ranges(0.4, 0.4, 0.4, 0.1))
    jp = loader_v2_ref.project_frame_v2(pts, sem, CJ.color_jitter(img, order, fac), M, lut)[0]
    assert np.array_equal(got.cpu().numpy(), loader_v2_ref.pad_center_crop(jp, h, w, h, w))
    torch.manual_seed(78)
    np.random.seed(78)
    tj = PerspectiveViewLoaderV2(DS(), dict(PVconfig=dict(tcfg["PVconfig"], img_jitter=[0.4, 0.4, 0.4, 0.1])),
                                 is_train=True, img_aug=True)[0]
    assert tj.shape == (10, h - 16, w - 32) and torch.isfinite(tj).all()


@pytest.mark.gpu
def test_autotuned_plan_matches_heuristic_plan():
    """the plan autotuner (on by default outside the tests) only changes tile shapes / K splits: the logits of an
    autotuned plan must agree with the heuristic plan to rounding, in eval and in train mode (batch statistics)."""
    from pmf_amd.models import PMFNet
    pcd, rgb, _, _ = synthetic_batch(2, 64, 256, 20, seed=2, fill=0.3)
    outs = {}
    old = os.environ.get("PMF_AUTOTUNE")
    try:
        for mode in ("0", "1"):
            os.environ["PMF_AUTOTUNE"] = mode
            m = deterministic_init(PMFNet(5, 3, 20, 32, False, "resnet34")).cuda()
            res = []
            for train in (False, True):
                m.train(train)
                if train:
                    m.set_dropout_masks({k: v.cuda() for k, v in _masks_for(m, 2).items()})
                with torch.no_grad():
                    m(pcd.cuda(), rgb.cuda())
                plan = [p for p in m._plans.values() if p.training == train][0]
                res.append((plan.read(plan.tensors["logits"]).cpu().numpy(), plan.read(plan.tensors["dec.logits"]).cpu().numpy()))
                if mode == "1":
                    from pmf_amd import plan as PL
                    assert len(PL._TUNED) > 20          # the tuner really ran
            outs[mode] = res
    finally:
        if old is None:
            os.environ.pop("PMF_AUTOTUNE", None)
        else:
            os.environ["PMF_AUTOTUNE"] = old
    for (a0, a1), (b0, b1) in zip(outs["0"], outs["1"]):
        assert G.rel_err(b0, a0) < 1e-3 and G.rel_err(b1, a1) < 1e-3      # the parity bar for logits


def _masks_for(model, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {nm: (torch.rand(n, c, generator=g) > 0.2).float() / 0.8 for nm, c in model._mask_sites()}


def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)     # two ranks share cuda:0 (RCCL refuses that)
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    torch.manual_seed(100 + rank)                                    # DIFFERENT initial weights: rank 0's must win
    m = PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34").cuda()
    eng = TrainEngine(m, 20, lr=1e-3, warmup_steps=2, max_steps=10, distributed=True, device_ids=[0])
    pcd, rgb, label, mask = synthetic_batch(2, 32, 64, 20, seed=20 + rank, fill=0.5)      # per-rank data
    feat = torch.cat((pcd, rgb), 1).cuda()
    torch.manual_seed(5)                                             # same dropout masks on both ranks
    torch.cuda.manual_seed(5)
    losses = [float(eng.train_step(feat.clone(), mask.cuda(), label.cuda())[0]) for _ in range(2)]
    flat = eng.flat.param.detach().clone()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    if rank == 0:
        ret["same"] = bool(all(torch.equal(gathered[0], g) for g in gathered))
        ret["finite"] = bool(all(np.isfinite(l) for l in losses))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_data_parallel_on_one_gpu():
    """the real N>1 path (FlatState, segmented backward graphs, asynchronous range all-reduce, initial broadcast) with
    two processes on one GPU over gloo: parameters stay identical across ranks although data and initial weights differ."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(2, 29551, ret), nprocs=2, join=True)
    assert ret["finite"] and ret["same"], dict(ret)


def _dp_worker_rccl(rank, world, port, ret):
    """two ranks, ONE device, backend nccl (= RCCL): either the real N>1 RCCL path runs end to end or RCCL's refusal
    is recorded verbatim"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_IGNORE_DISABLED_P2P="1")
    torch.cuda.set_device(0)
    try:
        dist.init_process_group("nccl", rank=rank, world_size=world)
        t = torch.full((1024,), float(rank + 1), device="cuda")
        dist.all_reduce(t)
        torch.cuda.synchronize()
        assert float(t[0]) == 3.0
    except Exception as e:                                            # RCCL refuses duplicate devices: keep the text
        ret["rccl_error_%d" % rank] = "%s: %s" % (type(e).__name__, str(e)[:600])
        return
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    torch.manual_seed(100 + rank)
    m = PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34").cuda()
    eng = TrainEngine(m, 20, lr=1e-3, warmup_steps=2, max_steps=10, distributed=True, device_ids=[0])
    pcd, rgb, label, mask = synthetic_batch(2, 32, 64, 20, seed=20 + rank, fill=0.5)
    feat = torch.cat((pcd, rgb), 1).cuda()
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    losses = [float(eng.train_step(feat.clone(), mask.cuda(), label.cuda())[0]) for _ in range(3)]
    eng.eval_step(feat.clone(), mask.cuda(), label.cuda())            # broadcasts rank 0's BN statistics first
    flat = eng.flat.param.detach().clone()
    bufs = torch.cat([b.reshape(-1).float() for b in m.buffers()])
    gp = [torch.zeros_like(flat) for _ in range(world)]
    gb = [torch.zeros_like(bufs) for _ in range(world)]
    dist.all_gather(gp, flat)
    dist.all_gather(gb, bufs)
    if rank == 0:
        ret["same"] = bool(all(torch.equal(gp[0], g) for g in gp))
        ret["same_buffers"] = bool(all(torch.equal(gb[0], g) for g in gb))
        ret["finite"] = bool(all(np.isfinite(l) for l in losses))
        ret["world"] = dist.get_world_size()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_data_parallel_on_one_gpu_rccl():
    """the N>1 path over RCCL with two ranks sharing the one GPU of the test box.  RCCL may refuse two ranks on one
    device ("Duplicate GPU detected"): then the test records the refusal in gpurun_out/rccl_two_ranks.txt and the gloo
    variant above remains the N>1 coverage; when it runs, parameters AND BatchNorm buffers must agree across ranks"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    try:
        mp.spawn(_dp_worker_rccl, args=(2, 29557, ret), nprocs=2, join=True)
    except Exception as e:
        ret["spawn_error"] = "%s: %s" % (type(e).__name__, str(e)[:600])
    out = dict(ret)
    os.makedirs("gpurun_out", exist_ok=True)
    with open(os.path.join("gpurun_out", "rccl_two_ranks.txt"), "w") as f:
        for k in sorted(out):
            f.write("%s: %s\n" % (k, out[k]))
    if any(k.startswith("rccl_error") or k == "spawn_error" for k in out):
        pytest.skip("RCCL refuses two ranks on one device here: " + "; ".join("%s=%s" % kv for kv in out.items())[:400])
    assert out.get("finite") and out.get("same") and out.get("same_buffers") and out.get("world") == 2, out


# ---------------------------------------------------------------------------------------------- SalsaNext range loader
def _range_boundary_ok(pts, cfg, ux_a, uy_a, ux_b, uy_b):
    """index pairs may differ only for points whose exact (float64) pixel coordinate sits on a pixel edge: numpy's
    float32 arctan2 / arcsin are platform dependent in the last ulp (see range_project.hip) -> affected pixel set"""
    s = cfg["sensor"]
    bad = np.nonzero((ux_a != ux_b) | (uy_a != uy_b))[0]
    assert bad.size <= 8, "%d index mismatches" % bad.size
    p = pts[bad].astype(np.float64)
    d = np.sqrt((p[:, :3] ** 2).sum(1))
    fl, fr = abs(s["fov_left"]) / 180 * np.pi, abs(s["fov_right"]) / 180 * np.pi
    fu, fd = abs(s["fov_up"]) / 180 * np.pi, abs(s["fov_down"]) / 180 * np.pi
    col = (-np.arctan2(p[:, 1], p[:, 0]) + fl) / (fl + fr) * s["proj_w"]
    row = (1 - (np.arcsin(p[:, 2] / d) + fd) / (fu + fd)) * s["proj_h"]
    for i in range(bad.size):
        near = min(abs(col[i] - round(col[i])), abs(row[i] - round(row[i])))
        assert near < 1e-3, "point %d: indices differ away from a pixel edge" % bad[i]
        assert abs(int(ux_a[bad[i]]) - int(ux_b[bad[i]])) <= 1 and abs(int(uy_a[bad[i]]) - int(uy_b[bad[i]])) <= 1
    touched = np.zeros((s["proj_h"], s["proj_w"]), bool)
    touched[uy_a[bad], ux_a[bad]] = True
    touched[uy_b[bad], ux_b[bad]] = True
    return ~touched


def _range_dataset(pts, sem, lut):
    import types
    ds = types.SimpleNamespace()
    ds.loadDataByIndex = lambda i: (pts.copy(), sem, np.zeros_like(sem))
    ds.labelMapping = lambda l: lut[l]
    return ds


@pytest.mark.parametrize("case_id", [0, 1])
def test_range_loader_matches_oracle_and_fixture(case_id, golden):
    """SalsaNextLoader (HIP kernels through the C ABI) vs oracle/range_projection_ref.py and the reference's outputs"""
    import random
    from oracle import range_projection_ref as RR
    from oracle.cases import lidar_sweep, RANGE_CASES
    from pmf_amd.dataset import SalsaNextLoader
    tag, seed, npts, cfg = RANGE_CASES[case_id]
    s = cfg["sensor"]
    g = golden("g10_range")
    pts, sem, lut = lidar_sweep(seed, npts, s["fov_up"], s["fov_down"])
    ds = _range_dataset(pts, sem, lut)
    ld = SalsaNextLoader(ds, cfg, is_train=False, return_uproj=True)
    feat, label, mask, rng, ux, uy, ud = [t.cpu().numpy() for t in ld[0]]
    pc, pr, pidx, pmask = [t.cpu().numpy() for t in ld.projection.doProjection(pts)]
    fov = RR.fov_constants(s["fov_up"], s["fov_down"], s["fov_left"], s["fov_right"])
    o = RR.loader_item(pts, lut[sem], fov, s["proj_h"], s["proj_w"], s["img_mean"], s["img_stds"])
    opc, _, oidx, omask, _, _, _ = RR.do_projection(pts, fov, s["proj_h"], s["proj_w"])
    assert ux.dtype == np.int64 and ud.dtype == np.float32 and mask.dtype == np.int32 and feat.shape == (5, s["proj_h"], s["proj_w"])
    np.testing.assert_array_equal(ud, o[6])                      # depth: sqrt / mul / add only -> exact everywhere
    np.testing.assert_array_equal(ud, g[tag + ".ud"])
    ok = _range_boundary_ok(pts, cfg, ux, uy, o[4], o[5])
    ok &= _range_boundary_ok(pts, cfg, ux, uy, g[tag + ".ux"], g[tag + ".uy"])
    assert ok.mean() > 0.999
    for name, got, want in (("feature", feat, o[0]), ("label", label, o[1]), ("mask", mask, o[2]), ("range", rng, o[3]),
                            ("proj_idx", pidx, oidx), ("proj_mask", pmask, omask), ("proj_range", pr, o[3])):
        sel = (slice(None), ok) if got.ndim == 3 else ok
        assert np.array_equal(got[sel], want[sel]), name
        if name in ("feature", "label", "mask", "range", "proj_idx", "proj_mask"):
            assert np.array_equal(got[sel], g["%s.%s" % (tag, name)][sel]), name + " (fixture)"
    assert np.array_equal(pc[ok], opc[ok])
    # training path: Python's `random` drives the draws as in the reference
    random.seed(100 + seed)
    ldt = SalsaNextLoader(ds, cfg, is_train=True, return_uproj=True)
    aug = ldt.augmentor.doAugmentation(pts.copy()).cpu().numpy()
    np.testing.assert_array_equal(aug, g[tag + ".augmented"])
    random.seed(100 + seed)
    ft, lt, mt, _, uxt, uyt, _ = [t.cpu().numpy() for t in ldt[0]]
    ot = RR.loader_item(aug, lut[sem], fov, s["proj_h"], s["proj_w"], s["img_mean"], s["img_stds"])
    okt = _range_boundary_ok(aug, cfg, uxt, uyt, ot[4], ot[5])
    assert np.array_equal(ft[:, okt], g[tag + ".train.feature"][:, okt]) and np.array_equal(lt[okt], g[tag + ".train.label"][okt])
    assert np.array_equal(mt[okt], g[tag + ".train.mask"][okt])


def test_range_projection_edges_and_knn_chain():
    """ties (equal depth on one pixel -> lower index), empty sweep, argument errors, and the SalsaNext inference chain
    loader -> KNN with (x, y) in loader order (tasks/salsanext_eval_nuscenes/infer.py:99-105) against the oracles"""
    from oracle import range_projection_ref as RR, knn_ref
    from oracle.cases import lidar_sweep
    from pmf_amd.dataset.preprocess.projection import RangeProjection
    from pmf_amd.postproc import KNN
    fov = RR.fov_constants(3., -25., -45, 45)
    pts, _, _ = lidar_sweep(1, 4000, duplicates=True)
    rp = RangeProjection(3., -25., 64, 16, -45, 45)
    pc, pr, pidx, pmask = [t.cpu().numpy() for t in rp.doProjection(pts)]
    o = RR.do_projection(pts, fov, 16, 64)
    ux, uy = rp.cached_data["uproj_x_idx"].cpu().numpy(), rp.cached_data["uproj_y_idx"].cpu().numpy()
    if np.array_equal(ux, o[4]) and np.array_equal(uy, o[5]):
        assert np.array_equal(pidx, o[2]) and np.array_equal(pr, o[1]) and np.array_equal(pc, o[0])
    e = rp.doProjection(np.zeros((0, 4), np.float32))
    assert (e[2] == -1).all() and (e[1] == -1).all() and e[3].sum() == 0 and (e[0] == -1).all()
    with pytest.raises(ValueError):
        rp.doProjection(np.zeros((5, 2), np.float32))
    assert L.lib().pmf_range_project_index(None, 1, 4, 1.0, 1.0, 1.0, 1.0, 4, 4, None, None, None, None, None) == -1
    # inference chain on a full sweep: range image + per-point (x, y, depth) from the loader feed the KNN vote
    pts, _, _ = lidar_sweep(5, 60000, 10., -30.)
    rp = RangeProjection(10., -30., 2048, 32)
    _, pr, _, _ = rp.doProjection(pts)
    c = rp.cached_data
    rng_ = np.random.Generator(np.random.PCG64(3))
    am = torch.as_tensor(rng_.integers(0, 17, (32, 2048)), dtype=torch.int64).cuda()
    knn = KNN({"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}, 17)
    got = knn(pr, c["uproj_depth"], am, c["uproj_x_idx"].long(), c["uproj_y_idx"].long()).cpu().numpy()
    want = knn_ref.knn_vote(pr.cpu().numpy(), c["uproj_depth"].cpu().numpy(), am.cpu().numpy(),
                            c["uproj_x_idx"].cpu().numpy().astype(np.int64), c["uproj_y_idx"].cpu().numpy().astype(np.int64))
    np.testing.assert_array_equal(got, want)


def test_salsanext_engine_train_steps_match_oracle():
    """tasks/salsanext/trainer.py step (Lovasz + masked focal, AdamW, warm-up cosine schedule) on the HIP plan with the
    flat training state, two iterations against the torch CPU oracle with the same injected Dropout2d masks"""
    from oracle import pmf_torch as O, losses_ref
    from pmf_amd.engine import SalsaNextEngine
    from pmf_amd.models import SalsaNext
    from pmf_amd.utils import WarmupCosineLR
    n, h, w, ncls = 2, 32, 64, 20
    hip = deterministic_init(SalsaNext(5, ncls, 32)).cuda()
    ref = deterministic_init(O.SalsaNext(5, ncls, 32))
    masks = _masks_for(hip, n)
    hip._forced_masks = {k: v.cuda() for k, v in masks.items()}
    for name, m in masks.items():
        blk, _, site = name.partition(".")
        getattr(getattr(ref, blk), "dropout" + site[1:] if site else "dropout").mask = m
    alpha = np.linspace(0.2, 1.0, ncls).astype(np.float32)
    alpha[0] = 0
    eng = SalsaNextEngine(hip, ncls, lr=1e-3, alpha=alpha, warmup_steps=2, max_steps=10)
    assert eng.flat is not None
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    sched = WarmupCosineLR(opt, 1e-3, 2, 0.9, 10)
    ref.train()
    trace = []
    for it in range(2):
        pcd, _, label, mask = synthetic_batch(n, h, w, ncls, seed=20 + it, fill=0.6)
        lab = label * label.ge(1).long()
        msk = mask * lab.ge(1).float()
        out = ref(pcd)
        want = losses_ref.lovasz_softmax(out, lab, 0) + losses_ref.focal_loss(out, lab, torch.from_numpy(alpha), 2.0, msk)
        opt.zero_grad()
        want.backward()
        opt.step()
        sched.step()
        got, terms = eng.train_step(pcd.cuda(), label.cuda(), mask.cuda())
        trace.append((it, got.item(), want.item(), terms["focal"].item(), terms["lovasz"].item()))
        if it == 0:
            # the optimiser step is compared after ONE iteration: from the second AdamW step on, m / sqrt(v) of a
            # weight whose two gradients nearly cancel amplifies rounding noise (the float32 and float64 CPU oracles
            # agree on only 80 % of the weights to 2e-4 after two steps, on 99.96 % after one)
            rsd = ref.state_dict()
            close = total = 0
            rows = []
            for k, v in hip.state_dict().items():
                if k.endswith("num_batches_tracked"):
                    assert int(v) == int(rsd[k]) == 1
                    continue
                d = (v.cpu() - rsd[k]).abs()
                close += int((d < 2e-4).sum())
                total += d.numel()
                rows.append((k, float((d < 2e-4).float().mean()), float(d.max()), d.numel()))
                assert d.max() < 4e-3, k
            _dump("salsanext_engine_params.txt", rows)
            assert close > 0.995 * total, (close / total, sorted(rows, key=lambda r: r[1])[:12])
    assert abs(trace[0][1] - trace[0][2]) <= 1e-5 * abs(trace[0][2]), trace
    assert abs(trace[1][1] - trace[1][2]) <= 1e-3 * abs(trace[1][2]), trace
    assert eng.optimizer.param_groups[0]["lr"] == pytest.approx(opt.param_groups[0]["lr"], rel=1e-6)
    assert eng.metrics.conf_matrix.sum().item() == 2 * n * h * w


def test_on_disk_kitti_tree_through_both_loaders(tmp_path):
    """SemanticKITTI files on disk -> SemanticKitti parser -> perspective (PMF) and range (SalsaNext) loaders on the
    GPU -> prediction file: every stage against the oracles on the arrays that were written"""
    from oracle import loader_ref, range_projection_ref as RR
    from oracle.cases import kitti_tree, RANGE_CASES
    from pmf_amd.dataset import PerspectiveViewLoader, SalsaNextLoader
    from pmf_amd.dataset.semantic_kitti import SemanticKitti, write_prediction
    root = str(tmp_path)
    cfg_path, data = kitti_tree(root, npts=4000, h=48, w=160)
    ds = SemanticKitti(root, [0, 8], cfg_path)
    pts, raw, img = data[("08", "000002")]
    idx = 5
    assert ds.parsePathInfoByIndex(idx) == ("08", "000002")
    pv = PerspectiveViewLoader(ds, {"sensor": dict(h_pad=0, w_pad=0, proj_h=48, proj_w=160, proj_ht=48, proj_wt=160)},
                               is_train=False, return_uproj=True)
    feat, mask, label, xd, yd, depth = pv[idx]
    rp, rx, ry, rd = loader_ref.project_frame(pts, (raw & 0xFFFF).astype(np.int32), img, ds.proj_matrix["08"],
                                              ds.class_map_lut)
    np.testing.assert_array_equal(torch.cat((feat, mask[None], label[None])).cpu().numpy(), rp)
    np.testing.assert_array_equal(xd.cpu().numpy(), rx)
    cfg = RANGE_CASES[0][3]
    s = cfg["sensor"]
    item = SalsaNextLoader(ds, cfg, is_train=False, return_uproj=True)[idx]
    fov = RR.fov_constants(s["fov_up"], s["fov_down"], s["fov_left"], s["fov_right"])
    o = RR.loader_item(pts, ds.labelMapping((raw & 0xFFFF).astype(np.int32)), fov, s["proj_h"], s["proj_w"],
                       s["img_mean"], s["img_stds"])
    ok = _range_boundary_ok(pts, cfg, item[4].cpu().numpy(), item[5].cpu().numpy(), o[4], o[5])
    assert np.array_equal(item[0].cpu().numpy()[:, ok], o[0][:, ok]) and np.array_equal(item[1].cpu().numpy()[ok], o[1][ok])
    # per-point prediction (here: the projected label looked up per point) -> KITTI submission file
    pred = item[1][item[5], item[4]].long().cpu().numpy()
    path = write_prediction(ds, idx, pred, os.path.join(root, "pred"))
    assert np.array_equal(np.fromfile(path, np.int32), ds.class_map_lut_inv[pred])


@pytest.mark.parametrize("tag,seed,pc", [("a", 0, 3000), ("b", 4, 347), (None, 9, 34720)])
def test_camera_merge_exact(tag, seed, pc, golden):
    """getMergePred (pmf_merge_pred through the C ABI) vs the oracle and the reference-run fixture; edge cases"""
    from oracle import merge_ref
    from oracle.cases import merge_case
    from pmf_amd.postproc import getMergePred
    idx, conf, lab = merge_case(seed, pc)
    t = lambda xs: [torch.from_numpy(x).cuda() for x in xs]
    got = getMergePred(t(idx), t(conf), t(lab), pc).cpu().numpy()
    np.testing.assert_array_equal(got, merge_ref.get_merge_pred(idx, conf, lab, pc))
    if tag:
        np.testing.assert_array_equal(got, golden("g12_merge")["merge." + tag])
    # points outside every camera view take the label of the LiDAR-only model (more_experiment_config.md:10)
    fb = np.random.default_rng(seed).integers(0, 17, pc).astype(np.int64)
    got_fb = getMergePred(t(idx), t(conf), t(lab), pc, fallback=torch.from_numpy(fb).cuda()).cpu().numpy()
    want = merge_ref.get_merge_pred(idx, conf, lab, pc)
    assert (want == -1).any()
    np.testing.assert_array_equal(got_fb, np.where(want == -1, fb, want))
    with pytest.raises(ValueError):
        getMergePred(t(idx), t(conf), t(lab), pc, fallback=torch.from_numpy(fb[:-1]).cuda())
    # a view that sees nothing, a single view, no points at all
    e = torch.zeros(0, dtype=torch.int64).cuda()
    one = getMergePred([torch.tensor([2, 0]).cuda(), e], [torch.tensor([0.5, 0.25]).cuda(), e.float()],
                       [torch.tensor([3, 0]).cuda(), e], 4).cpu().tolist()
    assert one == [0, -1, 3, -1]
    assert getMergePred([e], [e.float()], [e], 0).numel() == 0
    with pytest.raises(ValueError):
        getMergePred([e], [e.float()], [], 3)
    with pytest.raises(RuntimeError):
        getMergePred([e.cpu()], [e.float().cpu()], [e.cpu()], 3)


def test_training_tensor_augmentation_matches_torch_grid_sample(tmp_path):
    """FlipRotateCrop (pmf_flip_rotate_crop) vs the torch-CPU restatement of torchvision's flip -> rotate(nearest) -> crop
    -> pad: identical except where the inverse-rotated coordinate sits on a rounding edge; then the loader's training path"""
    import math
    from oracle import tensor_aug_ref as T
    from oracle.cases import kitti_tree
    from pmf_amd.dataset import FlipRotateCrop, PerspectiveViewLoader
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    rng = np.random.Generator(np.random.PCG64(5))
    total_bad = 0
    for case, (h, w, ch, cw, hp, wp) in enumerate(((96, 320, 80, 256, 0, 0), (64, 208, 64, 208, 4, 8), (376, 1241, 352, 1216, 0, 0))):
        img = torch.from_numpy((rng.random((10, h, w)) * (rng.random((1, h, w)) < 0.4)).astype(np.float32))
        op = FlipRotateCrop(ch, cw, hp, wp)
        torch.manual_seed(case)
        for rep in range(3):
            flip, angle, top, left = op.draw(h, w)
            if rep == 2:
                angle = 0.0                                    # flip + crop + pad only: an exact copy
            got = op.apply(img.cuda(), flip, angle, top, left).cpu()
            want = T.flip_rotate_crop(img, flip, angle, top, left, ch, cw, hp, wp)
            assert got.shape == want.shape == (10, ch + 2 * hp, cw + 2 * wp)
            bad = torch.nonzero((got != want).any(0))
            if angle == 0.0:
                assert bad.numel() == 0
            total_bad += bad.shape[0]
            assert bad.shape[0] <= 1e-4 * got[0].numel() + 2, (case, rep, bad.shape[0])
            r = math.radians(-angle)
            for oy, ox in bad.tolist():                       # exact source coordinate in float64
                xg, yg = left + ox - wp - w / 2 + 0.5, top + oy - hp - h / 2 + 0.5
                ix = ((math.cos(r) * xg + math.sin(r) * yg) / (w / 2) + 1) * w / 2 - 0.5
                iy = ((-math.sin(r) * xg + math.cos(r) * yg) / (h / 2) + 1) * h / 2 - 0.5
                assert min(abs(ix - math.floor(ix) - 0.5), abs(iy - math.floor(iy) - 0.5)) < 1e-3, (oy, ox, ix, iy)
    # loader: training item shapes with padding, seeded repeatability, point augmentation on the GPU path
    root = str(tmp_path)
    cfg_path, data = kitti_tree(root, npts=4000, h=48, w=160)
    ds = SemanticKitti(root, [0], cfg_path)
    from oracle.cases import RANGE_CASES
    cfg = {"augmentation": RANGE_CASES[0][3]["augmentation"],
           "sensor": dict(h_pad=2, w_pad=4, proj_h=48, proj_w=160, proj_ht=40, proj_wt=128)}
    ld = PerspectiveViewLoader(ds, cfg, is_train=True, use_padding=True, pcd_aug=True)
    import random
    random.seed(3); torch.manual_seed(3)
    f1, m1, l1 = ld[1]
    random.seed(3); torch.manual_seed(3)
    f2, m2, l2 = ld[1]
    assert f1.shape == (8, 40, 128) and m1.shape == l1.shape == (40, 128)
    assert torch.equal(f1, f2) and torch.equal(l1, l2)
    assert (f1[:, :2] == 0).all() and (f1[:, :, :4] == 0).all() and m1.sum() > 0     # the Pad frame


def test_engine_overfits_a_fixed_batch():
    """end-to-end sanity of the whole training path (plans, fused objective, flat state, both optimisers, schedules):
    40 iterations on one fixed batch must drive the objective down and keep every parameter finite"""
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    torch.manual_seed(0)
    m = PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34").cuda()
    eng = TrainEngine(m, 20, lr=2e-3, warmup_steps=5, max_steps=200)
    pcd, rgb, label, mask = synthetic_batch(2, 32, 64, 20, seed=12, fill=0.7)
    feat = torch.cat((pcd, rgb), 1).cuda()
    losses = []
    for _ in range(40):
        total, _ = eng.train_step(feat.clone(), mask.cuda(), label.cuda())
        losses.append(total.item())
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:3]), (losses[:3], losses[-5:])
    assert all(torch.isfinite(p).all() for p in m.parameters())
    acc = eng.metrics.getAcc()[0].item()
    assert 0.0 <= acc <= 1.0


DEV = "cuda"


def test_range_optimiser_equals_torch_fused_step():
    """TrainEngine with the range optimiser of libpmf_amd.so (updates queued behind the backward plan's events) against the
    same engine with torch's fused AdamW / SGD step() at the end of the iteration (PMF_OWN_OPTIM=0): after ONE iteration
    (identical gradients on both sides) the parameters and the optimiser state agree to float32 rounding of one update;
    after three the checkpoint layout is identical.  (Parameter VALUES are not compared after three steps: a convolution
    bias in front of a BatchNorm has a true gradient of zero, AdamW turns the rounding noise it receives instead into
    +-lr steps, and two runs that differ in the last bit after step one take different signs there.)"""
    import os
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    out = {}
    for own in ("1", "0"):
        os.environ["PMF_OWN_OPTIM"] = own
        try:
            torch.manual_seed(3)
            model = deterministic_init(PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34")).to(DEV)
            eng = TrainEngine(model, 20, lr=1e-3, momentum=0.9, weight_decay=1e-5, warmup_steps=2, max_steps=10)
        finally:
            os.environ.pop("PMF_OWN_OPTIM", None)
        assert (eng._ro is not None) == (own == "1")
        g = torch.Generator().manual_seed(5)
        first = None
        for it in range(3):
            feat = torch.randn(2, 8, 32, 64, generator=g).to(DEV)
            mask = (torch.rand(2, 32, 64, generator=g) > 0.2).float().to(DEV)
            label = torch.randint(0, 20, (2, 32, 64), generator=g).to(DEV)
            eng.train_step(feat, mask, label)
            if it == 0:
                torch.cuda.synchronize()
                st = eng.optimizer.state[eng.optimizer.param_groups[0]["params"][0]]
                sg = eng.aux_optimizer.state[eng.aux_optimizer.param_groups[0]["params"][0]]
                first = (eng.flat.param.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                         sg["momentum_buffer"].clone(), float(st["step"]))
        torch.cuda.synchronize()
        out[own] = (first, eng.optimizer_view.state_dict(), eng.aux_optimizer_view.state_dict())
    fa, fb = out["1"][0], out["0"][0]
    assert fa[4] == fb[4] == 1.0
    assert torch.allclose(fa[0], fb[0], rtol=1e-5, atol=1e-7), (fa[0] - fb[0]).abs().max().item()
    for i in (1, 2, 3):
        assert torch.allclose(fa[i], fb[i], rtol=1e-5, atol=1e-30 if i == 2 else 1e-12), i
    for sa, sb in ((out["1"][1], out["0"][1]), (out["1"][2], out["0"][2])):
        assert sa["param_groups"] == sb["param_groups"]
        assert sa["state"].keys() == sb["state"].keys()
        for k in sa["state"]:
            assert sa["state"][k].keys() == sb["state"][k].keys()
            for name, t in sa["state"][k].items():
                u = sb["state"][k][name]
                assert t.shape == u.shape and t.dtype == u.dtype, (k, name)
                if name == "step":
                    assert float(t) == float(u) == 3.0


def test_objective_row_mapping_is_bit_identical():
    """the objective's row-wise kernels launched one XCD per row (default) against the 2-D (chunk, row) grids
    (PMF_LOSS_XCD_ROWS=0): the mapping only decides WHERE a (chunk, row) pair runs -- loss and both gradient maps must be
    bit-identical (the knob is read once per process: two processes)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for v in ("1", "0"):
        env = dict(os.environ, PMF_LOSS_XCD_ROWS=v)
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_loss.py"), "3"], env=env, capture_output=True,
                           text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        fp = [ln for ln in r.stdout.splitlines() if ln.startswith("fingerprint")]
        assert len(fp) == 1, r.stdout
        out.append(fp[0])
    assert out[0] == out[1], out


@pytest.mark.parametrize("search,knn_k,cutoff", [(5, 5, 1.0), (3, 3, 0.0), (7, 5, 1.0)])
def test_knn_batch_equals_per_frame_calls(search, knn_k, cutoff):
    """pmf_knn_vote_batch (window staged through LDS per 256-point workgroup for search <= 5; global gathers when the
    workgroup's bounding box is too large, and for 7x7) against one pmf_knn_vote call per frame: bit-identical labels for
    sweep-ordered points, shuffled points (fallback), an EMPTY frame, frame sizes that are no multiple of 256, points on
    the image border and points far outside the image, sparse range images (-1 pixels)."""
    from pmf_amd.postproc import KNN
    H, W, B = 64, 512, 4
    g = torch.Generator().manual_seed(search * 10 + knn_k)
    knn = KNN({"knn": knn_k, "search": search, "sigma": 1.0, "cutoff": cutoff}, 20)
    pr = torch.rand(B, H, W, generator=g) * 40 + 2
    pr = torch.where(torch.rand(B, H, W, generator=g) < 0.5, pr, torch.full_like(pr, -1.0))
    am = torch.randint(0, 20, (B, H, W), generator=g)
    counts = [3001, 0, 777, 5000]
    for order in ("sweep", "shuffled"):
        frames = []
        for b in range(B):
            n = counts[b]
            y = torch.randint(0, H, (n,), generator=g)
            x = torch.randint(0, W, (n,), generator=g)
            if n:
                y[:8] = torch.tensor([0, 0, H - 1, H - 1, 0, H - 1, 5, 9])                 # borders and corners
                x[:8] = torch.tensor([0, W - 1, 0, W - 1, 7, 11, 0, W - 1])
            if order == "sweep" and n:
                o = torch.argsort(x * H + y, stable=True)
                x, y = x[o], y[o]
            if b == 3 and n:                                                              # far outside: every tap is padding
                x[100], y[100] = 10 * W, -3 * H
            ur = torch.rand(n, generator=g) * 40 + 2
            frames.append((pr[b].cuda(), ur.cuda(), am[b].cuda(), x.cuda(), y.cuda()))
        got = knn.batch(frames)
        for b, f in enumerate(frames):
            want = knn(f[0], f[1], f[2], f[3], f[4]) if counts[b] else torch.empty(0, dtype=torch.int64, device="cuda")
            assert got[b].shape == want.shape and torch.equal(got[b], want), (order, b)
        # pmf_knn_vote_batch_prob: the same labels from probability maps whose channel argmax is `am` -- with exact TIES (two
        # classes share the maximum: torch.argmax takes the lower one) and a NaN channel (torch.argmax takes it)
        prob = torch.rand(B, 20, H, W, generator=g) * 0.5
        prob.scatter_(1, am[:, None], 0.75)
        tie = torch.rand(B, H, W, generator=g) < 0.1
        hi = torch.clamp(am + 3, max=19)
        prob.scatter_(1, hi[:, None], torch.where(tie, torch.tensor(0.75), prob.gather(1, hi[:, None])[:, 0])[:, None])
        prob[0, 7, 5, 9] = float("nan")
        am_t = prob.argmax(1)
        assert bool((am_t == am).float().mean() > 0.99) and int(am_t[0, 5, 9]) == 7
        frames_t = [(f[0], f[1], am_t[b].cuda(), f[3], f[4]) for b, f in enumerate(frames)]
        want_p = knn.batch(frames_t)
        got_p = knn.batch_prob(prob.cuda(), [(f[0], f[1], f[3], f[4]) for f in frames])
        for b in range(B):
            assert torch.equal(got_p[b], want_p[b]), (order, b)


@pytest.mark.parametrize("search,knn_k,cutoff", [(1, 1, 1.0), (9, 5, 1.0), (11, 5, 1.0), (11, 7, 0.0), (13, 8, 0.5)])
def test_knn_any_odd_window_vs_oracle(search, knn_k, cutoff):
    """Every odd search window the reference accepts (pc_processor/postproc/knn.py:73-74 only rejects even sizes; the nuScenes
    config ships search 11): the run-time-window kernel against the numpy oracle, one frame and batched, incl. border
    pixels, sparse maps and quantised ranges (distance ties).  search = 1 used to fall into the 5 x 5 LDS kernel."""
    from pmf_amd.postproc import KNN
    from oracle import knn_ref
    H, W, n = 32, 256, 4000
    rng = np.random.default_rng(search * 100 + knn_k)
    frames, want = [], []
    for b in range(2):
        pr = (np.round(rng.random((H, W)) * 40 * 4) / 4 + 2).astype(np.float32)          # quantised: ties
        pr[rng.random((H, W)) < 0.4] = -1.0
        am = rng.integers(0, 20, (H, W)).astype(np.int64)
        py = rng.integers(0, H, n).astype(np.int64)
        px = rng.integers(0, W, n).astype(np.int64)
        py[:4], px[:4] = [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]
        ur = (np.round(rng.random(n) * 40 * 4) / 4 + 2).astype(np.float32)
        frames.append((pr, ur, am, px, py))
        want.append(knn_ref.knn_vote(pr, ur, am, px, py, knn=knn_k, search=search, sigma=1.0, cutoff=cutoff, nclasses=20))
    knn = KNN({"knn": knn_k, "search": search, "sigma": 1.0, "cutoff": cutoff}, 20)
    t = lambda a: torch.from_numpy(a).cuda()
    for f, w_ in zip(frames, want):
        np.testing.assert_array_equal(knn(*[t(a) for a in f]).cpu().numpy(), w_)
    got = knn.batch([tuple(t(a) for a in f) for f in frames])
    for g_, w_ in zip(got, want):
        np.testing.assert_array_equal(g_.cpu().numpy(), w_)


def test_weights_repacked_behind_optimiser_bitwise_and_invalidation(monkeypatch):
    """Round 5: the forward-format weight packs of a training step are launched right behind the range optimiser's update of
    their gradient range (engine._behind_events -> Plan.pack_ranges) and the next forward plan starts behind its pack launches
    (Plan.fwd_pack_skip).  Same arithmetic in another order: four training steps with and without it (PMF_PACK_BEHIND_OPTIM=0)
    end with BIT-IDENTICAL parameters.  A parameter write torch can see (load_state_dict) invalidates the packed copy: the next
    forward equals that of a fresh model with those weights."""
    from pmf_amd.engine import TrainEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PMF_PACK_BEHIND_OPTIM", mode)
        torch.manual_seed(3)
        model = deterministic_init(PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34")).to(DEV)
        eng = TrainEngine(model, 20, lr=1e-3, momentum=0.9, weight_decay=1e-5, warmup_steps=2, max_steps=10)
        g = torch.Generator().manual_seed(5)
        for it in range(4):
            feat = torch.randn(2, 8, 32, 64, generator=g).to(DEV)
            mask = (torch.rand(2, 32, 64, generator=g) > 0.2).float().to(DEV)
            label = torch.randint(0, 20, (2, 32, 64), generator=g).to(DEV)
            eng.train_step(feat, mask, label)
        torch.cuda.synchronize()
        plan = next(p for k, p in model._plans.items() if k[3])
        skipped = any(k[0] == "forward" and k[1] > 0 for k in list(plan._graphs) + list(plan._graph_seen))
        assert skipped == (mode == "1"), (mode, list(plan._graph_seen))
        assert (getattr(plan, "packed_version", None) is not None) == (mode == "1")
        res[mode] = (eng.flat.param.clone(), model, eng, (feat, mask))
    assert torch.equal(res["1"][0], res["0"][0])
    # invalidation: other weights through load_state_dict -> the packed copy is stale and must not be used
    model, eng, (feat, mask) = res["1"][1], res["1"][2], res["1"][3]
    fresh = deterministic_init(PMFNet(5, 3, 20, 32, imagenet_pretrained=False, image_backbone="resnet34"), 11).to(DEV)
    model.load_state_dict(fresh.state_dict())
    model.train()
    fresh.train()
    m = {n: torch.ones(2, c, device=DEV) for n, c in model._mask_sites()}
    model.set_dropout_masks(m)
    fresh.set_dropout_masks(m)
    x = feat.clone()
    a = model(x[:, 0:5], x[:, 5:8])[0]
    b = fresh(x[:, 0:5], x[:, 5:8])[0]
    assert torch.allclose(a, b, atol=1e-6), (a - b).abs().max().item()
