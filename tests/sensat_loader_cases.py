"""Shared pieces of the SensatLoader tests (TEST INFRASTRUCTURE, not a conftest): the reference's item chain on the CPU,
restated from pc_processor/dataset/sensat_urban/sensat_loader.py:57-73, and synthetic frames.

The chain is torchvision's RandomCrop -> RandomRotation -> RandomCrop -> flips with the parameters GIVEN (the draws are
tested separately): slicing, oracle.tensor_aug_ref.rotate_nearest (the project's restatement of torchvision's tensor
rotation with torch's own grid_sample -- torchvision is not installed, so its parity is unpinned), slicing, flip, and the
two jitter lines verbatim in torch float32."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.tensor_aug_ref import rotate_nearest  # noqa: E402

# name -> (h, w, H, W): small, odd and non-square, so that an h / w swap or a stride slip shows
#   A  first crop 48 x 80 inside 70 x 113;  B  exactly 48 x 80: the first crop draws nothing;
#   C / C2  97 x 64 with H = W = 32: a square 64 x 64 first crop for the quarter turns;  D  rejection (labels mostly -1);
#   E  137 x 480 items are 18 x 15 = 270 tiles of 8 x 32 pixels: more than the 256 workgroups the count kernel gives a
#      candidate, so that some of them walk a second tile
FRAMES = {"A": (70, 113, 24, 40), "B": (48, 80, 24, 40), "C": (97, 64, 32, 32), "C2": (97, 64, 32, 32),
          "D": (70, 113, 24, 40), "E": (280, 970, 137, 480)}
GENERAL_SEED = {"A": 1, "B": 2, "C": 3, "E": 4}         # torch.manual_seed before the ten general-angle draws of a frame


def make_frame(name):
    """-> frame dict as the dataset preparation writes it: feature_map f64[8,h,w] with a distinct value per pixel and plane
    (not float32-representable: the .float() rounding is part of the item), channel 4 a 0/1 mask with about 40 % zeros,
    label_map int64[h,w] in {-1, 0..12} with a block of -1 (frame D: -1 except the top-left quadrant)"""
    h, w = FRAMES[name][:2]
    seed = sorted(FRAMES).index(name)
    rs = np.random.RandomState(100 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    fm = np.stack([(c * 300007 + yy * w + xx + 1 + 1000 * seed) * 0.37 for c in range(8)]).astype(np.float64)
    fm[4] = (rs.rand(h, w) >= 0.4).astype(np.float64)
    assert np.unique(fm[[0, 1, 2, 3, 5, 6, 7]].astype(np.float32)).size == 7 * h * w
    lm = ((yy // 5 + xx // 7 + seed) % 13).astype(np.int64)
    lm[h // 3:h // 2, w // 4:w // 2] = -1
    if name == "D":
        keep = lm[:h // 2, :w // 2].copy()
        lm[:] = -1
        lm[:h // 2, :w // 2] = np.abs(keep)
    return {"feature_map": fm, "label_map": lm, "h_idx": None, "w_idx": None}


class FrameSet(object):
    """what SensatLoader needs of a SensatUrban dataset"""

    def __init__(self, names, split="train"):
        self.split, self.names = split, list(names)
        self.all_data_frame = [make_frame(n) for n in self.names]

    def readDataByIndex(self, i):
        return self.all_data_frame[i]

    def __len__(self):
        return len(self.all_data_frame)


def all_map(frame, dtype=torch.float32):
    """sensat_loader.py:57-62: the nine planes the augmentation sees"""
    feature_map = torch.from_numpy(frame["feature_map"]).float()
    label_map = torch.from_numpy(frame["label_map"]).float()
    return torch.cat((feature_map, label_map.unsqueeze(0)), dim=0).to(dtype)


def ref_augment(amap, cand, H, W):
    """the aug_pos chain with the drawn parameters cand = (top1, left1, angle, top2, left2, hflip, vflip) -> [9,H,W]"""
    top1, left1, angle, top2, left2, hflip, vflip = cand
    x = amap[:, top1:top1 + 2 * H, left1:left1 + 2 * W]
    assert x.shape[1:] == (2 * H, 2 * W)
    x = rotate_nearest(x, angle)
    x = x[:, top2:top2 + H, left2:left2 + W]
    if hflip:
        x = x.flip(-1)
    if vflip:
        x = x.flip(-2)
    return x.clone()


def ref_share(amap, cand, H, W):
    """sensat_loader.py:68 -> (valid_percent as the float32 tensor the reference compares with 0.1, the count)"""
    tmp_map = ref_augment(amap, cand, H, W)
    return tmp_map[8].ge(0).sum().float() / tmp_map[8].numel(), int(tmp_map[8].ge(0).sum())


def ref_item(amap, cand, jitter, H, W):
    """sensat_loader.py:67-73 for an accepted candidate -> (f32[8,H,W], f32[H,W])"""
    all_map = ref_augment(amap, cand, H, W)
    jit_rgb, jit_h = jitter
    all_map[5:8] = (all_map[5:8] + jit_rgb) * all_map[4:5]
    all_map[0:3] = (all_map[0:3] + jit_h) * all_map[4:5]
    return all_map[:8], all_map[8]


def edge_distance(cand, H, W, oy, ox):
    """distance of the source coordinate of OUTPUT pixel (oy, ox) from the nearest rounding edge, recomputed in float64 as
    tests/test_gpu_parity.py:1270-1275 does (w := 2W, h := 2H, the flips undone first)"""
    _, _, angle, top2, left2, hflip, vflip = cand
    cx, cy = (W - 1 - ox if hflip else ox), (H - 1 - oy if vflip else oy)
    w, h = 2 * W, 2 * H
    r = math.radians(-angle)
    xg, yg = left2 + cx - w / 2 + 0.5, top2 + cy - h / 2 + 0.5
    ix = ((math.cos(r) * xg + math.sin(r) * yg) / (w / 2) + 1) * w / 2 - 0.5
    iy = ((-math.sin(r) * xg + math.cos(r) * yg) / (h / 2) + 1) * h / 2 - 0.5
    return min(abs(ix - math.floor(ix) - 0.5), abs(iy - math.floor(iy) - 0.5))


def cap(H, W):
    """pixels of an item that may differ from the restatement (each of them on a rounding edge): a condition, not a
    measurement -- the restatement in float32 and in float64 differs in at most half as many for every draw the tests use
    (test_general_angle_draws_are_well_conditioned, host)"""
    return 1e-3 * H * W + 4
