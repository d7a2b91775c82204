"""tests/golden/g21_sensat_loss.npz: the SensatUrban training objective evaluated with the reference's own loss modules.

    python tools/make_golden_sensat_loss.py /path/to/reference

pc_processor/loss/{dice_loss,focal_softmax,lovasz_softmax}.py of the reference are imported by file path at run time (plain
torch, CPU) and composed the way tasks/sensat_urban/pmf/trainer.py does: _computeClassifyLoss (focal + exp-log Dice with
mask = label > 0, Lovasz with ignore 0) for both heads, _computePerceptionAwareLoss with the 0.7 threshold, and
total = foc + lov + foc_cam + lov_cam + 0.5 * per, where foc already contains the Dice term.

Inputs by recipe (tests regenerate them): softmax of det_tensor("g21.logits" / "g21.logits2", (2, 14, 16, 32), -6, 6), labels
of synthetic_batch(2, 16, 32, 14, seed=3, fill=0.4), the trainer's focal alpha.  Stored: OUTPUTS only --
values = [total, foc, dice, lov, foc_cam, dice_cam, lov_cam, per] (foc = the pure focal value) and the gradients of the total
with respect to both logit maps.  (Logits in [-6, 6]: in [-3, 3] no pixel of 14 classes reaches the 0.7 confidence
threshold and the perception term would be 0.)"""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmf_amd.utils.detinit import det_tensor, synthetic_batch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_sensat_loss.npz")
SHAPE = (2, 14, 16, 32)


def _load(modname, path):
    spec = importlib.util.spec_from_file_location(modname, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def trainer_alpha(nclasses):
    a = np.ones(nclasses)
    for c, v in ((0, 0), (4, 2), (5, 2.5), (7, 3), (12, 10), (13, 2.5)):
        a[c] = v
    return a


def main(ref):
    d = os.path.join(ref, "pc_processor", "loss")
    dice_m = _load("ref_dice_loss", os.path.join(d, "dice_loss.py"))
    focal_m = _load("ref_focal_softmax", os.path.join(d, "focal_softmax.py"))
    lovasz_m = _load("ref_lovasz_softmax", os.path.join(d, "lovasz_softmax.py"))
    n, c, h, w = SHAPE
    crit = {"lovasz": lovasz_m.Lovasz_softmax(ignore=0), "kl": torch.nn.KLDivLoss(reduction="none"),
            "focal": focal_m.FocalSoftmaxLoss(c, gamma=2, alpha=trainer_alpha(c), softmax=False),
            "dice": dice_m.ExpLogDiceLoss()}
    a = det_tensor("g21.logits", SHAPE, -6, 6).requires_grad_(True)
    b = det_tensor("g21.logits2", SHAPE, -6, 6).requires_grad_(True)
    _, _, label, _ = synthetic_batch(n, h, w, c, seed=3, fill=0.4)
    label = label.long()
    mask = label.gt(0)
    lp, cp = torch.softmax(a, 1), torch.softmax(b, 1)

    def classify(pred):                                    # _computeClassifyLoss, the two summands kept apart
        return crit["lovasz"](pred, label), crit["focal"](pred, label, mask=mask), crit["dice"](pred, label, mask=mask)

    llog = torch.log(lp.clamp(min=1e-8))
    pent = -(lp * llog).sum(1) / math.log(c)
    lov, foc, dice = classify(lp)
    clog = torch.log(cp.clamp(min=1e-8))
    ient = -(cp * clog).sum(1) / math.log(c)
    lov_cam, foc_cam, dice_cam = classify(cp)
    pconf, iconf = 1 - pent, 1 - ient                      # _computePerceptionAwareLoss
    imp = pconf - iconf
    wp = imp.gt(0).float() * imp.abs() * pconf.ge(0.7).float()
    wi = imp.lt(0).float() * imp.abs() * iconf.ge(0.7).float()
    per = (crit["kl"](llog, cp) * wi.unsqueeze(1)).mean() + (crit["kl"](clog, lp) * wp.unsqueeze(1)).mean()
    total = (foc + dice) + lov + (foc_cam + dice_cam) + lov_cam + per * 0.5
    total.backward()
    vals = np.array([t.item() for t in (total, foc, dice, lov, foc_cam, dice_cam, lov_cam, per)], np.float64)
    assert np.isfinite(vals).all() and dice.item() > 0 and dice_cam.item() > 0 and per.item() > 0, vals
    np.savez_compressed(GOLDEN, values=vals, grad_a=a.grad.numpy().astype(np.float32),
                        grad_b=b.grad.numpy().astype(np.float32))
    print("g21_sensat_loss: values %s, %d bytes" % (np.round(vals, 6).tolist(), os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
