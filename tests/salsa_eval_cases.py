"""Shared pieces of the SalsaNext nuScenes evaluation tests (TEST INFRASTRUCTURE, not a conftest): a devkit-free LiDAR-only
nuScenes-type dataset, the probability maps by recipe, and numpy statements of the per-sweep composition of the
reference's tasks/salsanext_eval_nuscenes/infer.py:90-119 (argmax, pixel confusion, gather or KNN, point confusion)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.cases import lidar_sweep  # noqa: E402

NCLASSES = 17
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_salsa_eval.npz")
_AUG = dict(p_flipx=0., p_flipy=0.5, p_transx=0.5, trans_xmin=-5, trans_xmax=5, p_transy=0.5, trans_ymin=-3, trans_ymax=3,
            p_transz=0.5, trans_zmin=-1, trans_zmax=0., p_rot_roll=0.5, rot_rollmin=-5, rot_rollmax=5, p_rot_pitch=0.5,
            rot_pitchmin=-5, rot_pitchmax=5, p_rot_yaw=0.5, rot_yawmin=5, rot_yawmax=-5)
# the nuScenes sensor block of the task's config at a quarter of the width
CONFIG = {"augmentation": _AUG,
          "sensor": dict(name="HDL32", type="spherical", proj_h=32, proj_w=512, fov_up=10., fov_down=-30., fov_left=-180,
                         fov_right=180, img_mean=[12.12, 10.88, 0.23, -1.04, 0.21], img_stds=[12.32, 11.47, 6.91, 0.86, 0.16]),
          "post": {"KNN": {"use": False, "params": dict(KNN_PARAMS)}}}


class SyntheticSalsaNus(object):
    """The attributes of pc_processor/dataset/nuScenes/dataset_nuscenes.py (has_image=False) that SalsaNextLoader and the
    SalsaNext inference loop use: one index = one sweep, token_list[i] a plain string, loadDataByIndex -> (f32[P,4],
    uint8[P,1] raw ids 0..31, int32[P]), labelMapping = a table lookup over
    map_name_from_general_index_to_segmentation_index (32 raw ids -> 17 classes), mapped_cls_name.  Sweeps have different
    point counts; a block of every sweep repeats the positions of another block with other labels (points sharing a pixel
    beyond the natural collisions); ~6000 points on 32 x 512 pixels leave most pixels empty."""

    def __init__(self, seed=0, counts=(6000, 5800, 6200), nclasses=NCLASSES):
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        self.nclasses = nclasses
        self.sweeps = []
        for s, npts in enumerate(counts):
            pts, _, _ = lidar_sweep(200 + 10 * seed + s, npts, 10., -30.)
            n = npts // 20
            pts[n:2 * n, :3] = pts[2 * n:3 * n, :3]
            raw = rng.integers(0, 32, (npts, 1)).astype(np.uint8)
            self.sweeps.append((pts, raw))
        self.map_name_from_general_index_to_segmentation_index = {i: int(rng.integers(0, nclasses)) for i in range(32)}
        self.mapped_cls_name = {i: "class_%d" % i for i in range(nclasses)}
        self.token_list = ["sweep%03d" % i for i in range(len(counts))]

    def __len__(self):
        return len(self.token_list)

    def loadDataByIndex(self, index):
        pts, raw = self.sweeps[index]
        return pts, raw, np.zeros(pts.shape[0], dtype=np.int32)

    def labelMapping(self, sem_label):
        lut = np.zeros(32, np.int64)
        for k, v in self.map_name_from_general_index_to_segmentation_index.items():
            lut[k] = v
        return lut[np.asarray(sem_label)[:, 0]]


def prob_maps(seed, B, C=NCLASSES, H=32, W=512):
    """f32[B,C,H,W] by recipe (numpy.random.RandomState(seed); additions, one division: the same bits everywhere): blocks of
    4 x 8 pixels share a dominant class (so the KNN vote, which looks at a 5 x 5 window, changes labels next to the block
    borders and wherever the dominant class is 0), plus per-pixel noise; every pixel's classes sum to 1."""
    rs = np.random.RandomState(seed)
    coarse = rs.rand(B, C, H // 4, W // 8).astype(np.float32)
    fine = rs.rand(B, C, H, W).astype(np.float32)
    p = np.repeat(np.repeat(coarse, 4, axis=2), 8, axis=3) + np.float32(0.25) * fine + np.float32(0.01)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def top2_gap(prob):
    """smallest difference between the two largest class probabilities of any pixel (argmax must not rest on a tie)"""
    s = np.sort(prob, axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def knn_vote_np(proj_range, unproj_range, argmax, px, py, inv_gauss, nclasses, knn=5, search=5, cutoff=1.0, reverse=False):
    """knn.py:55-143 in numpy with float32 arithmetic; the k nearest by a stable sort over the window taps in ascending
    (reverse=False) or descending (reverse=True) tap order: equal labels from both = no point's vote depends on the order
    among equal distances.  inv_gauss f32[search * search]."""
    H, W = proj_range.shape
    pad, S2 = (search - 1) // 2, search * search
    rp = np.zeros((H + 2 * pad, W + 2 * pad), np.float32)
    rp[pad:pad + H, pad:pad + W] = proj_range
    lp = np.zeros((H + 2 * pad, W + 2 * pad), np.int64)
    lp[pad:pad + H, pad:pad + W] = argmax
    dy, dx = np.divmod(np.arange(S2), search)
    neigh = rp[py[:, None] + dy[None], px[:, None] + dx[None]].copy()
    labs = lp[py[:, None] + dy[None], px[:, None] + dx[None]]
    neigh[neigh < 0] = np.inf
    neigh[:, (S2 - 1) // 2] = unproj_range
    with np.errstate(invalid="ignore"):
        dist = (np.abs(neigh - unproj_range[:, None].astype(np.float32)) * inv_gauss.reshape(1, S2)).astype(np.float32)
    if reverse:
        dist, labs = dist[:, ::-1], labs[:, ::-1]
    sel = np.argsort(dist, axis=1, kind="stable")[:, :knn]
    sd = np.take_along_axis(dist, sel, 1)
    sl = np.take_along_axis(labs, sel, 1).copy()
    if cutoff > 0:
        sl[sd > np.float32(cutoff)] = nclasses
    votes = np.zeros((px.shape[0], nclasses + 1), np.int64)
    np.add.at(votes, (np.repeat(np.arange(px.shape[0]), knn), sl.reshape(-1)), 1)
    return (votes[:, 1:-1].argmax(1) + 1).astype(np.int32)


def np_conf(pred, gt, C, base=None):
    pred, gt = np.asarray(pred, np.int64).reshape(-1), np.asarray(gt, np.int64).reshape(-1)
    c = np.bincount(pred * C + gt, minlength=C * C).reshape(C, C)
    return c if base is None else c + base
