"""The SensatUrban training iteration on the GPU: the fused objective with the exp-log Dice term (csrc/loss.hip
pmf_loss_pixel_dice / pmf_loss_dice_finish, loss/fused.py sensat_total_loss_fused), the AMSGrad range update
(csrc/optim.hip pmf_adamw_amsgrad_range) and SensatEngine (engine.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.utils.detinit import det_tensor, synthetic_batch  # noqa: E402

DEV = "cuda"
NCLS = 14
TERMS = ("foc", "dice", "lov", "foc_cam", "dice_cam", "lov_cam", "per")
# (n, c, h, w, fill, dropped classes)
SHAPES = {"one_partial_workgroup": (1, 14, 5, 7, 0.7, ()),
          "fixture_shape": (2, 14, 16, 32, 0.4, ()),
          "tail_and_absent_classes": (3, 14, 17, 31, 0.6, (5, 12)),
          "several_workgroups_sparse": (2, 14, 64, 96, 0.05, ()),
          "no_unlabelled_pixel": (1, 14, 8, 8, 1.0, ())}


def _alpha():
    from pmf_amd.engine import sensat_focal_alpha
    return sensat_focal_alpha(NCLS)


def _labels(n, h, w, c, fill, drop):
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=5, fill=fill)
    if fill >= 1.0:
        label = label.clamp(min=1)
    for k in drop:
        label = torch.where(label == k, torch.zeros_like(label), label)
    return label.long()


@functools.lru_cache(maxsize=None)
def _case(name):
    """probabilities (float64, CPU), labels and the float64 autograd reference of sensat_total_loss -- computed once"""
    from pmf_amd.loss import ExpLogDiceLoss, FocalSoftmaxLoss, Lovasz_softmax, sensat_total_loss
    n, c, h, w, fill, drop = SHAPES[name]
    label = _labels(n, h, w, c, fill, drop)
    pa = torch.softmax(det_tensor("sl.a", (n, c, h, w), -6, 6).double(), 1).requires_grad_(True)
    pb = torch.softmax(det_tensor("sl.b", (n, c, h, w), -6, 6).double(), 1).requires_grad_(True)
    foc = FocalSoftmaxLoss(c, gamma=2, alpha=_alpha(), softmax=False).double()
    ref, rt = sensat_total_loss(pa, pb, label, foc, Lovasz_softmax(ignore=0), ExpLogDiceLoss(), 1.0, 0.5, 0.7)
    ref.backward()
    return pa.detach(), pb.detach(), label, ref.item(), {k: rt[k].item() for k in TERMS}, pa.grad, pb.grad


def _fused(pa, pb, label, conf=False, fn=None):
    from pmf_amd.loss import sensat_total_loss_fused
    from pmf_amd.metrics import IOUEval
    ga, gb = pa.float().to(DEV).requires_grad_(True), pb.float().to(DEV).requires_grad_(True)
    ml = mc = None
    args = ()
    if conf:
        ml, mc = IOUEval(NCLS, DEV, ignore=[0]), IOUEval(NCLS, DEV, ignore=[0])
        args = (ml.conf_matrix, mc.conf_matrix)
    tot, tt = (fn or sensat_total_loss_fused)(ga, gb, label.to(DEV), torch.from_numpy(_alpha()), 1.0, 0.5, 0.7, 2.0, *args)
    tot.backward()
    torch.cuda.synchronize()
    return tot, tt, ga.grad, gb.grad, ml, mc


def test_fused_sensat_objective_matches_reference_fixture(golden):
    """value of every term and gradient w.r.t. both LOGIT maps against the reference-run fixture (the reference's own modules
    composed as its SensatUrban trainer does): values 5e-6, gradients 5e-7"""
    from pmf_amd.loss import sensat_total_loss_fused
    g = golden("g21_sensat_loss")
    n, c, h, w = 2, 14, 16, 32
    a = det_tensor("g21.logits", (n, c, h, w), -6, 6).to(DEV).requires_grad_(True)
    b = det_tensor("g21.logits2", (n, c, h, w), -6, 6).to(DEV).requires_grad_(True)
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=3, fill=0.4)
    total, t = sensat_total_loss_fused(torch.softmax(a, 1), torch.softmax(b, 1), label.to(DEV), torch.from_numpy(_alpha()))
    total.backward()
    vals = np.array([total.item()] + [t[k].item() for k in TERMS])
    print("fixture: |values - ref| =", np.abs(vals - g["values"]), "grad err",
          np.abs(a.grad.cpu().numpy() - g["grad_a"]).max(), np.abs(b.grad.cpu().numpy() - g["grad_b"]).max())
    assert set(t) == set(TERMS)
    assert np.abs(vals - g["values"]).max() < 5e-6, (vals, g["values"])
    assert np.abs(a.grad.cpu().numpy() - g["grad_a"]).max() < 5e-7
    assert np.abs(b.grad.cpu().numpy() - g["grad_b"]).max() < 5e-7


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_sensat_objective_matches_float64_autograd(name):
    from pmf_amd.metrics import IOUEval
    pa, pb, label, ref, rt, gra, grb = _case(name)
    tot, tt, ga, gb, ml, mc = _fused(pa, pb, label, conf=True)
    print(name, "total err", abs(tot.item() - ref), {k: abs(tt[k].item() - rt[k]) for k in TERMS},
          "grad err", (ga.cpu().double() - gra).abs().max().item(), (gb.cpu().double() - grb).abs().max().item(),
          "grad max", gra.abs().max().item(), grb.abs().max().item())
    assert rt["dice"] > 0 and rt["dice_cam"] > 0
    assert abs(tot.item() - ref) < 2e-6 * max(1.0, abs(ref))
    for k in TERMS:
        assert abs(tt[k].item() - rt[k]) < 2e-6 * max(1.0, abs(rt[k])), k
    for got, want in ((ga, gra), (gb, grb)):
        err = (got.cpu().double() - want).abs().max().item()
        assert err < 1e-6 * max(want.abs().max().item(), 1e-3) + 1e-9, err
    rl, rc = IOUEval(NCLS, "cpu", ignore=[0]), IOUEval(NCLS, "cpu", ignore=[0])
    rl.addBatch(pa.float().argmax(1), label)
    rc.addBatch(pb.float().argmax(1), label)
    assert torch.equal(ml.conf_matrix.cpu(), rl.conf_matrix) and torch.equal(mc.conf_matrix.cpu(), rc.conf_matrix)


def test_fused_sensat_objective_is_deterministic():
    pa, pb, label = _case("tail_and_absent_classes")[:3]
    r1, r2 = _fused(pa, pb, label), _fused(pa, pb, label)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[2], r2[2]) and torch.equal(r1[3], r2[3])
    for k in TERMS:
        assert torch.equal(r1[1][k], r2[1][k]), k


def test_dice_leaves_the_rest_of_the_objective_alone():
    """the five terms the PMF objective has are bit-identical with and without the Dice extension, and each gradient map of
    the new path equals (the old path's map + the closed-form Dice gradient in float64) to the gradient bar of the float64
    parity test, taken on that sum"""
    from pmf_amd.loss import pmf_total_loss_fused
    from pmf_amd.loss.dice_loss import explog_dice_closed_form
    pa, pb, label = _case("fixture_shape")[:3]
    new = _fused(pa, pb, label)
    old = _fused(pa, pb, label, fn=pmf_total_loss_fused)
    for k in ("foc", "lov", "foc_cam", "lov_cam", "per"):
        assert torch.equal(new[1][k], old[1][k]), k
    for p, gn, go in ((pa, new[2], old[2]), (pb, new[3], old[3])):
        val, dg = explog_dice_closed_form(p.float().double(), label)
        assert dg.abs().max() > 0
        want = go.cpu().double() + dg
        err = (gn.cpu().double() - want).abs().max().item()
        assert err < 1e-6 * max(want.abs().max().item(), 1e-3) + 1e-9, err
        # The focal gradient (1 / p_t at small p_t) sets the maximum of the map, so the bar above says little about the Dice
        # part, which is ~1e-3.  Element by element: with x the per-pixel kernel's value before the Dice term, the old map
        # holds fl(x + lov) (the Lovasz stage adds its gradient to the stored value) and the new one fl(fl(x + term) + lov):
        # three roundings at the magnitude of the sum between the two, 3 * 2^-24 |sum|; 2^-22 leaves one more for a fused
        # multiply-add landing on the other neighbour.  Plus the float32 error of the term itself: K/C, dice_c and 1/D_c
        # rounded to float32, one subtraction and two multiplications -- at most six roundings, 8 * 2^-24 |term| with room.
        elem = (gn.cpu().double() - want).abs()
        bound = 2.0 ** -22 * want.abs() + 2.0 ** -21 * dg.abs() + 1e-12
        print("dice gradient: max |term| %.3e, max err %.3e, worst err / bound %.3f"
              % (dg.abs().max().item(), elem.max().item(), (elem / bound).max().item()))
        assert (elem <= bound).all()
    assert abs(new[0].item() - (old[0].item() + new[1]["dice"].item() + new[1]["dice_cam"].item())) < 2e-6 * max(1.0, new[0].item())


def test_dice_entry_points_refuse_bad_arguments():
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, c, hw = 1, NCLS, 64
    p = torch.full((n, c, hw), 1.0 / c, device=DEV)
    lab = torch.ones(n, hw, dtype=torch.int64, device=DEV)
    al = torch.ones(c, device=DEV)
    gl, gc = torch.full_like(p, 7.0), torch.full_like(p, 7.0)
    key = torch.empty(2 * c, n * hw, device=DEV)
    rows = torch.empty(lib.pmf_loss_rows(n * hw), 4, dtype=torch.float64, device=DEV)
    cnt = torch.full((c,), 5, dtype=torch.int64, device=DEV)
    parts = torch.empty(lib.pmf_loss_dice_parts(n * hw), 4 * c, dtype=torch.float64, device=DEV)
    dice = torch.full((2, 2 + 2 * c), 3.0, dtype=torch.float64, device=DEV)

    def call(cc=c, parts_p=parts.data_ptr(), dice_p=dice.data_ptr(), nn=n):
        return lib.pmf_loss_pixel_dice(p.data_ptr(), p.data_ptr(), lab.data_ptr(), al.data_ptr(), nn, cc, hw, 2.0, 0.7, 0.5,
                                       cnt.data_ptr(), gl.data_ptr(), gc.data_ptr(), key.data_ptr(), rows.data_ptr(), None,
                                       None, parts_p, dice_p, st)
    assert call(cc=33) == L.PMF_E_ARG and call(cc=1) == L.PMF_E_ARG and call(nn=0) == L.PMF_E_ARG
    assert call(parts_p=None) == L.PMF_E_ARG and call(dice_p=None) == L.PMF_E_ARG
    out = torch.full((10,), 9.0, device=DEV)
    assert lib.pmf_loss_dice_finish(None, c, out.data_ptr(), st) == L.PMF_E_ARG
    assert lib.pmf_loss_dice_finish(dice.data_ptr(), c, None, st) == L.PMF_E_ARG
    assert lib.pmf_loss_dice_finish(dice.data_ptr(), 40, out.data_ptr(), st) == L.PMF_E_ARG
    torch.cuda.synchronize()
    assert (gl == 7).all() and (gc == 7).all() and (cnt == 5).all() and (dice == 3).all() and (out == 9).all()
    assert call() == 0                                                # and the same buffers are accepted
    torch.cuda.synchronize()
    assert int(cnt[1]) == hw and int(cnt.sum()) == hw and torch.isfinite(gl).all()


# ---- AMSGrad range update (csrc/optim.hip) against torch.optim.AdamW(amsgrad=True) on the CPU -----------------------------
@pytest.mark.parametrize("n,off", [(1, 0), (7, 0), (4099, 64), (100003, 1)])
def test_adamw_amsgrad_range_matches_torch(n, off):
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n + off, generator=g)
    ref = torch.nn.Parameter(p0[off:].clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01, amsgrad=True)
    grads = [torch.randn(n + off, generator=g) * (10.0 ** (1 - k)) for k in range(4)]
    want = []
    for k, gr in enumerate(grads):              # gradients shrink 10x per step: the running maximum stops following exp_avg_sq
        ref.grad = gr[off:].clone()
        opt.param_groups[0]["lr"] = 1e-3 * (k + 1)
        opt.step()
        s = opt.state[ref]
        want.append((ref.data.clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone(), s["max_exp_avg_sq"].clone()))
    assert (want[-1][3] != want[-1][2]).float().mean().item() > 0.5      # plain AdamW would not pass what follows
    p = p0.clone().to(DEV)
    m, v, x = (torch.zeros(n + off, device=DEV) for _ in range(3))
    step = torch.zeros((), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = L.lib().pmf_adamw_amsgrad_range
    for k, gr in enumerate(grads):
        gd = gr.to(DEV)
        step += 1
        rc = fn(p.data_ptr() + 4 * off, gd.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                x.data_ptr() + 4 * off, n, 1e-3 * (k + 1), 0.9, 0.999, 1e-8, 0.01, step.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(p[:off].cpu(), p0[:off])                     # nothing outside the range is touched
        assert not m[:off].any() and not v[:off].any() and not x[:off].any()
        wp, wm, wv, wx = want[k]
        assert torch.allclose(p[off:].cpu(), wp, rtol=2e-6, atol=2e-7), (k, (p[off:].cpu() - wp).abs().max().item())
        assert (m[off:].cpu() - wm).abs().max() <= 1e-6 * wm.abs().max()
        assert (v[off:].cpu() - wv).abs().max() <= 1e-6 * wv.abs().max()
        assert (x[off:].cpu() - wx).abs().max() <= 1e-6 * wx.abs().max()
    # argument guards: nothing is launched, nothing is written
    before = (p.clone(), m.clone(), v.clone(), x.clone())
    gd = grads[0].to(DEV)
    assert fn(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, 1e-3, 0.9, 0.999, 1e-8, 0.01,
              step.data_ptr(), st) == L.PMF_E_ARG
    assert fn(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.01,
              None, st) == L.PMF_E_ARG
    torch.cuda.synchronize()
    for a, b in zip(before, (p, m, v, x)):
        assert torch.equal(a, b)


MEAN = [27.47, 26.90, 27.22, 0.63, 0.81, 0, 0, 0]
STD = [18.43, 18.00, 18.21, 0.40, 0.39, 255.0, 255.0, 255.0]


def _sensat_batch(n, h, w, g):
    feat = torch.tensor(MEAN).view(1, 8, 1, 1) + torch.tensor(STD).view(1, 8, 1, 1) * torch.randn(n, 8, h, w, generator=g)
    feat[:, 4] = (torch.rand(n, h, w, generator=g) > 0.2).float()
    return feat, torch.randint(0, NCLS - 1, (n, h, w), generator=g)


def test_sensat_engine_range_optimiser_equals_torch_fused_step():
    """SensatEngine with the range optimiser (AMSGrad range updates behind the backward plan's events) against the same engine
    with torch's fused AdamW(amsgrad=True) / SGD step() (PMF_OWN_OPTIM=0): after ONE iteration parameters and optimiser
    state agree to float32 rounding of one update; after three the checkpoint layout is identical (parameter values are not
    compared after three steps, see test_range_optimiser_equals_torch_fused_step)."""
    from pmf_amd.engine import SensatEngine
    from pmf_amd.models import PMFNet
    from pmf_amd.utils.detinit import deterministic_init
    out = {}
    for own in ("1", "0"):
        os.environ["PMF_OWN_OPTIM"] = own
        try:
            torch.manual_seed(3)
            model = deterministic_init(PMFNet(5, 3, NCLS, 32, imagenet_pretrained=False, image_backbone="resnet34")).to(DEV)
            eng = SensatEngine(model, NCLS, lr=1e-3, momentum=0.9, weight_decay=1e-5, warmup_steps=2, max_steps=10,
                               feature_mean=MEAN, feature_std=STD)
        finally:
            os.environ.pop("PMF_OWN_OPTIM", None)
        assert eng.optimizer.param_groups[0]["amsgrad"] is True
        assert (eng._ro is not None) == (own == "1")
        g = torch.Generator().manual_seed(5)
        first = None
        for it in range(3):
            feat, label = _sensat_batch(2, 32, 64, g)
            total, terms = eng.train_step(feat.to(DEV), label.to(DEV))
            if it == 0:
                torch.cuda.synchronize()
                assert torch.isfinite(total).item() and set(TERMS) <= set(terms)
                st = eng.optimizer.state[eng.optimizer.param_groups[0]["params"][0]]
                sg = eng.aux_optimizer.state[eng.aux_optimizer.param_groups[0]["params"][0]]
                first = (eng.flat.param.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                         sg["momentum_buffer"].clone(), float(st["step"]), st["max_exp_avg_sq"].clone())
        torch.cuda.synchronize()
        out[own] = (first, eng.optimizer_view.state_dict(), eng.aux_optimizer_view.state_dict(),
                    len(list(model.lidar_stream.parameters())))
    fa, fb = out["1"][0], out["0"][0]
    assert fa[4] == fb[4] == 1.0
    assert torch.allclose(fa[0], fb[0], rtol=1e-5, atol=1e-7), (fa[0] - fb[0]).abs().max().item()
    for i in (1, 2, 3, 5):
        assert torch.allclose(fa[i], fb[i], rtol=1e-5, atol=1e-30 if i in (2, 5) else 1e-12), i
    assert fa[5].abs().max() > 0
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
    for own in ("1", "0"):
        sd, nlidar = out[own][1], out[own][3]
        assert len(sd["state"]) == nlidar
        assert all("max_exp_avg_sq" in e and float(e["step"]) == 3.0 for e in sd["state"].values())


@pytest.mark.parametrize("n", [2, 1])
def test_sensat_prepare_is_bit_identical_to_the_torch_expression(n):
    """the mask is channel 4 of the tensor that pmf_normalise_inplace rewrites: the engine must hand the kernel a copy taken
    before the launch (n = 1: the channel slice is contiguous by itself, so .contiguous() would still be a view)"""
    from pmf_amd.engine import SensatEngine

    class _Streams(torch.nn.Module):            # prepare() needs an engine, the engine three parameter groups
        def __init__(self):
            super().__init__()
            self.lidar_stream = torch.nn.Conv2d(5, NCLS, 1)
            self.camera_stream_encoder = torch.nn.Conv2d(3, 4, 1)
            self.camera_stream_decoder = torch.nn.Conv2d(4, NCLS, 1)
    eng = SensatEngine(_Streams().to(DEV), NCLS, feature_mean=MEAN, feature_std=STD, flat_state=False)
    g = torch.Generator().manual_seed(7)
    feat, raw = _sensat_batch(n, 5, 7, g)
    assert (feat[:, 4] == 0).any() and (feat[:, 4] == 1).any()
    x = feat.to(DEV)
    mean, std = torch.tensor(MEAN, device=DEV).view(1, 8, 1, 1), torch.tensor(STD, device=DEV).view(1, 8, 1, 1)
    mask = x[:, 4].clone()
    want = (x - mean) / std * mask.unsqueeze(1)
    want_label = (raw.to(DEV).long() + 1) * mask.long()
    xin = x.clone()
    pcd, rgb, label = eng.prepare(xin, raw.to(DEV))
    torch.cuda.synchronize()
    assert pcd.data_ptr() == xin.data_ptr()                                  # in place: the kernel ran, not the torch expression
    assert torch.equal(pcd, want[:, 0:5]) and torch.equal(rgb, want[:, 5:8]) and torch.equal(label, want_label)
    assert (pcd[:, 4][mask == 0] == 0).all() and (pcd[:, 4][mask == 1] != 0).all()
