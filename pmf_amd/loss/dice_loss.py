"""Dice and exp-log Dice losses over class probabilities (pc_processor/loss/dice_loss.py of the reference; the SensatUrban
trainer adds ExpLogDiceLoss()(pred, label, mask = label > 0) to the focal term of both heads).

    dice_c = (2 sum_i x_ci onehot_ci + 1e-6) / (sum_i (x_ci + onehot_ci) + 1e-6)       sums over all N*H*W pixels
    DiceLoss = mean_c dice_c          ExpLogDiceLoss = (-log(clamp(DiceLoss, 1e-6))) ** 0.3

With a mask, both the target and the probabilities are multiplied by it first: masked pixels then count as class 0 in the
one-hot sums and contribute nothing to the probability sums.  Device-agnostic torch ops; the GPU training path computes the
same value and its gradient in csrc/loss.hip (loss/fused.py sensat_total_loss_fused)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class DiceLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.epsilon = 1e-6

    def forward(self, x, target, mask=None):
        """x: [N, C] or [N, C, H, W] probabilities; target: [N] or [N, H, W] integer labels; mask: like target (or like x)."""
        if mask is not None:
            target = target * mask
            x = x * (mask.unsqueeze(1) if mask.dim() == x.dim() - 1 else mask)
        c = x.size(1)
        onehot = F.one_hot(target, num_classes=c).reshape(-1, c)
        pred = x.flatten(2).transpose(1, 2).reshape(-1, c) if x.dim() > 2 else x
        inter = (pred * onehot).sum(0) * 2 + self.epsilon
        denom = (pred + onehot).sum(0) + self.epsilon
        return (inter / denom).mean()


class ExpLogDiceLoss(nn.Module):
    def __init__(self, gamma=0.3):
        super().__init__()
        self.gamma = 0.3            # the reference's constructor ignores its argument: always 0.3
        self.dc = DiceLoss()

    def forward(self, x, target, mask=None):
        return torch.pow(-self.dc(x, target, mask).clamp(min=1e-6).log(), self.gamma)


def explog_dice_closed_form(x, target):
    """value and gradient of ExpLogDiceLoss()(x, target, mask = target > 0) in closed form -- what csrc/loss.hip evaluates
    (m_i = [0 < t_i < C]; T_c = label histogram, T_0 = unlabelled pixels):
        I_c = sum m x_c [t = c],  S_c = sum m x_c,  D_c = S_c + T_c + 1e-6,  dice_c = (2 I_c + 1e-6) / D_c,  dc = mean_c dice_c
        L = (-ln max(dc, 1e-6)) ** 0.3,   dL/dx_ci = m_i K/C (2 [t_i = c] - dice_c) / D_c,   K = -0.3 (-ln dc) ** -0.7 / dc
    x: [N, C, H, W]; returns (L, dL/dx)."""
    c = x.shape[1]
    m = ((target > 0) & (target < c))
    t = torch.where(m, target, torch.zeros_like(target))
    onehot = F.one_hot(t, c).movedim(-1, 1).to(x.dtype)                       # [N, C, H, W]
    mx = m.unsqueeze(1).to(x.dtype)
    dims = (0, 2, 3)
    inter = (x * onehot * mx).sum(dims)
    s = (x * mx).sum(dims)
    hist = onehot.sum(dims)
    d = s + hist + 1e-6
    dice = (2 * inter + 1e-6) / d
    dc = dice.mean()
    nl = -torch.log(dc.clamp(min=1e-6))
    k = torch.where(dc < 1e-6, torch.zeros_like(dc), -0.3 * nl ** -0.7 / dc)
    grad = mx * (k / c) * (2 * onehot - dice.view(1, c, 1, 1)) / d.view(1, c, 1, 1)
    return nl ** 0.3, grad
