"""Shared pieces of the EPMF nuScenes evaluation tests (TEST INFRASTRUCTURE, not a conftest): a devkit-free NuscenesV2-type
dataset, and numpy statements of the reference's per-sweep merge (tasks/epmf_eval_nuscenes/infer.py:96-107,166-202)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.cases import SyntheticNus  # noqa: E402

MEAN = [12.87, 0.01, 0.44, 11.97, 19.07]
STDS = [13.21, 6.05, 1.96, 12.50, 21.23]
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_nus_v2.npz")


class SyntheticNusV2(SyntheticNus):
    """SyntheticNus with the attributes of dataset_nuscenes_v2.py that PerspectiveViewLoaderV2 and the EPMF loop use:
    mapLidar2CameraCropYaw(index, pointcloud) -> (camera-frame rows f32[K,4] = (right, down, forward, intensity),
    (row, col) f64[K,2], keep bool[P]) and NO proj_matrix.  One yaw rotation per camera + the pinhole of mapLidar2Camera;
    kept = forward > 0.1 and the camera's yaw window (no pixel-margin masks: coordinates leave the image, some truncate to
    negative values).  Windows: cameras 0..4 are 68 degrees wide (neighbours 60 degrees apart overlap by 8), camera 5 is 44
    degrees wide (4-degree gaps on both sides: points no camera keeps).  As the devkit reader scales the coordinates of
    every camera but CAM_BACK by (0.5, 0.6), every camera but number 3 does here -- boxes pad to different shapes; cameras 1
    and 2 have a shifted principal point (negative columns / rows).  A block of points is repeated with other
    intensities: equal pixels, the scatter's last-writer order decides."""

    HALF_WINDOW_DEG = (34.0, 34.0, 34.0, 34.0, 34.0, 22.0)
    BACK = 3
    SHIFT = {1: (0.0, -70.0), 2: (-45.0, 0.0)}           # camera -> (row, col) principal point shift in pixels

    def __init__(self, seed=0, sweeps=2, npts=6000, h=80, w=160, nclasses=17):
        super().__init__(seed=seed, sweeps=sweeps, npts=npts, h=h, w=w, nclasses=nclasses)
        n = npts // 20
        for s, (pts, raw) in enumerate(self.sweeps):
            pts = pts.copy()
            pts[n:2 * n, :3] = pts[2 * n:3 * n, :3]       # same pixel, different intensity / label, earlier in the file
            self.sweeps[s] = (pts, raw)

    def mapLidar2CameraCropYaw(self, index, pointcloud, min_dist=0.1):
        cam = index % self.N_CAM
        yaw = np.deg2rad(60.0 * cam)
        x, y, z = (pointcloud[:, k].astype(np.float64) for k in range(3))
        fwd = np.cos(yaw) * x + np.sin(yaw) * y
        right = np.sin(yaw) * x - np.cos(yaw) * y
        down = -z - 0.3
        half = np.deg2rad(self.HALF_WINDOW_DEG[cam])
        rel = np.arctan2(right, fwd)
        keep = np.logical_and(fwd > min_dist, np.logical_and(rel >= -half, rel <= half))
        cam_pts = np.stack([right, down, fwd, pointcloud[:, 3].astype(np.float64)], 1).astype(np.float32)[keep]
        dr, dc = self.SHIFT.get(cam, (0.0, 0.0))
        u = self.fx * right[keep] / fwd[keep] + 0.5 * self.w + dc
        v = self.fx * down[keep] / fwd[keep] + 0.5 * self.h + dr
        mapped = np.stack([v, u], 1)
        if cam != self.BACK:
            mapped[:, 0] *= 0.5
            mapped[:, 1] *= 0.6
        return cam_pts, mapped, keep


def view_geometry(ds, index):
    """(crop, xy, keep, x_data, y_data, x_min, y_min, h, w, H, W, left) of one view, as the reference computes them"""
    pts, _, _ = ds.loadDataByIndex(index)
    crop, xy, keep = ds.mapLidar2CameraCropYaw(index, pts)
    xd, yd = xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32)
    x_min, y_min = int(xd.min()), int(yd.min())
    h, w = int(xd.max()) - x_min + 1, int(yd.max()) - y_min + 1
    h_pad = math.ceil(h / 64.0) * 64 - h
    w_pad = math.ceil(w / 64.0) * 64 - w
    return crop, xy, keep, xd, yd, x_min, y_min, h, w, h + h_pad, w + w_pad, w_pad // 2


def merge_mask_form(conf_full, label_full, keep_mask, conf, label):
    """the reference's boolean-mask merge of one view, verbatim semantics (infer.py:170-173), in place"""
    keep_mask_np = keep_mask.copy()
    keep_conf_mask = conf_full[keep_mask_np] < conf
    keep_mask_np[keep_mask_np] = np.logical_and(keep_mask_np[keep_mask_np], keep_conf_mask)
    conf_full[keep_mask_np] = conf[keep_conf_mask]
    label_full[keep_mask_np] = label[keep_conf_mask]


def merge_src_form(conf_full, label_full, src, conf, label):
    """what the kernel does: point k of the view goes to src[k], taken where strictly more confident"""
    for k in range(src.shape[0]):
        p = src[k]
        if conf_full[p] < conf[k]:
            conf_full[p] = conf[k]
            label_full[p] = label[k]


def view_conf_label(prob_win, ux, uy, knn=None):
    """(confidence f32[K], label int[K]) of one view from its cropped probability window [C,h,w] (infer.py:140-164).
    knn = (proj_depth f32[h,w], depth f32[K], nclasses): both maps through oracle.knn_ref.knn_vote, the confidence map
    truncated to integers as the reference's KNN module does."""
    with np.errstate(invalid="ignore"):
        am = _argmax_nan_first(prob_win)
    conf_map = np.take_along_axis(prob_win, am[None], 0)[0]
    if knn is None:
        return conf_map[ux, uy].astype(np.float32), am[ux, uy]
    from oracle import knn_ref
    pd, depth, C = knn
    lab = knn_ref.knn_vote(pd, depth, am.astype(np.int64), uy, ux, nclasses=C, **KNN_PARAMS)
    with np.errstate(invalid="ignore"):
        cm = np.where(np.isnan(conf_map), 0, conf_map).astype(np.int64)
    cf = knn_ref.knn_vote(pd, depth, cm, uy, ux, nclasses=C, **KNN_PARAMS)
    return cf.astype(np.float32), lab


def _argmax_nan_first(prob):
    """torch.max / argmax over dim 0: first maximum, a NaN is the maximum (numpy's argmax does the same)"""
    return np.argmax(prob, axis=0)


def np_conf(pred, gt, C, base=None):
    pred, gt = np.asarray(pred, np.int64).reshape(-1), np.asarray(gt, np.int64).reshape(-1)
    c = np.bincount(pred * C + gt, minlength=C * C).reshape(C, C)
    return c if base is None else c + base
