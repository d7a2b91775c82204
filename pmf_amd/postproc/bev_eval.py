"""Per-frame device work of PMF evaluation on SensatUrban (tasks/sensat_urban/pmf_eval/infer.py), around the network.

A frame is a bird's-eye-view map f32[8,h,w] of one block (a few thousand pixels a side).  The reference cuts it into
S x S tiles for every S of img_size, crops each tile on the host in float64, uploads and normalises it, runs the network once
(or seven times with test-time augmentation: the tile, five same-size variants and a 16-pixel padded one, each permuted by
its own torch op), copies the probabilities to the host and adds them to a confidence map there; the class map's labels
are then read at the points' pixels or voted by KNN.  Here the frame is uploaded once and stays on the device with the
confidence map (csrc/bev_eval.hip):

  pre     T tiles x V variants -> pcd f32[T*V,5,S,S], rgb f32[T*V,3,S,S] (+ padded [T,.,S+32,S+32])     (pmf_bev_tile_pre)
  accum   prob f32[T*V,C,S,S] (+ padded): variants undone, summed in the reference's order, += the map  (pmf_bev_tile_accum)
  finish  argmax + pixel confusion (pmf_eval_argmax over the whole map), the points' labels by gather or the KNN module,
          0 -> 1, += point confusion, uint8 labels                                                     (pmf_bev_points)

The six same-size variants are ONE batch-6 forward: in eval mode BatchNorm uses its running statistics, so batch elements
do not influence each other.  No GPU work falls back to torch: a missing kernel is an error.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..dataset.sensat_urban import tile_windows  # noqa: F401  (one enumeration for the dataset's crops and this loop)
from .frame_eval import _is_dev, _ptr, _stream, window_argmax
from .knn import KNN

PAD = 16            # border of the padded test-time variant
MAX_TILES = 64      # tiles per call of the library


def _origins(origins, h, w, S, V):
    if S < 16 or S % 16 != 0:
        raise ValueError("the tile size must be a positive multiple of 16, got %r" % (S,))
    if V not in (1, 6):
        raise ValueError("V must be 1 (the tile) or 6 (the tile and its five same-size variants), got %r" % (V,))
    org = [(int(a), int(b)) for a, b in origins]
    if not 1 <= len(org) <= MAX_TILES:
        raise ValueError("1..%d tiles per call, got %d" % (MAX_TILES, len(org)))
    for a, b in org:
        if not (0 <= a < h and 0 <= b < w):
            raise ValueError("tile origin (%d, %d) outside the %d x %d frame" % (a, b, h, w))
    return (C.c_int32 * (2 * len(org)))(*[x for ab in org for x in ab]), len(org)


def bev_tile_pre(frame, mean, stds, origins, S, V=1, want_pad=False, out=None):
    """frame f32[8,h,w], mean / stds f32[8] on the device; origins [(h_start, w_start)] of T tiles -> (pcd [T*V,5,S,S],
    rgb [T*V,3,S,S], pcd_pad [T,5,S+32,S+32] or None, rgb_pad or None): (x - mean) / std * mask, zero past the frame, the
    variants in the reference's order, tile-major.  out: the four tensors to write into (workspaces)."""
    if not (_is_dev(frame, torch.float32) and frame.dim() == 3 and frame.shape[0] == 8):
        raise ValueError("frame must be a contiguous float32 CUDA tensor [8, h, w]")
    if not (_is_dev(mean, torch.float32, (8,)) and _is_dev(stds, torch.float32, (8,))):
        raise ValueError("mean / stds must be float32 CUDA tensors [8]")
    _, h, w = frame.shape
    org, T = _origins(origins, h, w, S, V)
    dev = frame.device
    SP = S + 2 * PAD
    shapes = ((T * V, 5, S, S), (T * V, 3, S, S), (T, 5, SP, SP), (T, 3, SP, SP))
    if out is None:
        out = [torch.empty(s, dtype=torch.float32, device=dev) if k < 2 or want_pad else None for k, s in enumerate(shapes)]
    for k, s in enumerate(shapes):
        if (k < 2 or want_pad) and not _is_dev(out[k], torch.float32, s):
            raise ValueError("output %d must be a contiguous float32 CUDA tensor %s" % (k, s))
    pcd, rgb = out[0], out[1]
    pcd_pad, rgb_pad = (out[2], out[3]) if want_pad else (None, None)
    L.check(L.lib().pmf_bev_tile_pre(frame.data_ptr(), h, w, mean.data_ptr(), stds.data_ptr(), org, T, S, V, pcd.data_ptr(),
                                     rgb.data_ptr(), _ptr(pcd_pad), _ptr(rgb_pad), _stream(dev)), "pmf_bev_tile_pre")
    return pcd, rgb, pcd_pad, rgb_pad


def bev_tile_accum(prob, origins, S, V, conf_map, prob_pad=None):
    """prob f32[>=T*V,C,S,S] (batch elements behind the T listed tiles are ignored), prob_pad f32[>=T,C,S+32,S+32] or None;
    conf_map f32[C,h,w] += per tile, in list order, the sum of the undone variants in the reference's order.  Only the
    part of a tile that lies inside the frame is added: where the reference raises a shape error on a frame smaller than
    the tile (and avoids it by skipping one tiny block by name), this takes the part the frame filled."""
    if not (_is_dev(conf_map, torch.float32) and conf_map.dim() == 3):
        raise ValueError("conf_map must be a contiguous float32 CUDA tensor [C, h, w]")
    Cn, h, w = conf_map.shape
    org, T = _origins(origins, h, w, S, V)
    if not (_is_dev(prob, torch.float32) and prob.dim() == 4 and prob.shape[0] >= T * V
            and tuple(prob.shape[1:]) == (Cn, S, S)):
        raise ValueError("prob must be a contiguous float32 CUDA tensor [>= %d, %d, %d, %d]" % (T * V, Cn, S, S))
    if prob_pad is not None:
        SP = S + 2 * PAD
        if V != 6:
            raise ValueError("the padded variant goes with V = 6")
        if not (_is_dev(prob_pad, torch.float32) and prob_pad.dim() == 4 and prob_pad.shape[0] >= T
                and tuple(prob_pad.shape[1:]) == (Cn, SP, SP)):
            raise ValueError("prob_pad must be a contiguous float32 CUDA tensor [>= %d, %d, %d, %d]" % (T, Cn, SP, SP))
    L.check(L.lib().pmf_bev_tile_accum(prob.data_ptr(), _ptr(prob_pad), Cn, org, T, S, V, conf_map.data_ptr(), h, w,
                                       _stream(conf_map.device)), "pmf_bev_tile_accum")
    return conf_map


def bev_points(class_map, h_idx, w_idx, nclasses, pred_in=None, label=None, conf=None, n_zero=None, out=None):
    """class_map int32[h,w]; h_idx / w_idx int64[P] -> uint8[P] = pred - 1 with pred = class_map[h_idx, w_idx] (or pred_in
    int64[P], the KNN votes), 0 -> 1; label uint8[P] + conf int64[C,C] (both or neither): conf[pred, label + 1] += 1, the
    layout of IOUEval.addBatch; n_zero int64[1] on the device += the zeros replaced."""
    if not (_is_dev(class_map, torch.int32) and class_map.dim() == 2):
        raise ValueError("class_map must be a contiguous int32 CUDA tensor [h, w]")
    if not (_is_dev(h_idx, torch.int64) and h_idx.dim() == 1 and _is_dev(w_idx, torch.int64, h_idx.shape)):
        raise ValueError("h_idx / w_idx must be contiguous int64 CUDA tensors [P]")
    P = int(h_idx.shape[0])
    if pred_in is not None and not _is_dev(pred_in, torch.int64, (P,)):
        raise ValueError("pred_in must be a contiguous int64 CUDA tensor [%d]" % P)
    if (label is None) != (conf is None):
        raise ValueError("label and conf go together")
    if conf is not None:
        if not 1 <= int(nclasses) <= 64:
            raise ValueError("a confusion matrix needs 1..64 classes, got %r" % (nclasses,))
        if not _is_dev(conf, torch.int64, (nclasses, nclasses)):
            raise ValueError("conf must be a contiguous int64 CUDA tensor [%d, %d]" % (nclasses, nclasses))
        if not _is_dev(label, torch.uint8, (P,)):
            raise ValueError("label must be a contiguous uint8 CUDA tensor [%d]" % P)
    if n_zero is not None and not (_is_dev(n_zero, torch.int64) and n_zero.numel() == 1):
        raise ValueError("n_zero must be an int64 CUDA tensor of one element")
    if out is None:
        out = torch.empty(P, dtype=torch.uint8, device=class_map.device)
    elif not _is_dev(out, torch.uint8, (P,)):
        raise ValueError("out must be a contiguous uint8 CUDA tensor [%d]" % P)
    h, w = class_map.shape
    L.check(L.lib().pmf_bev_points(class_map.data_ptr(), h, w, h_idx.data_ptr(), w_idx.data_ptr(), P, _ptr(pred_in),
                                   _ptr(label), int(nclasses), _ptr(conf), _ptr(n_zero), out.data_ptr(),
                                   _stream(class_map.device)), "pmf_bev_points")
    return out


class BevTileEvaluator(object):
    """One SensatUrban frame at a time: frame() is the reference's loop body (infer.py:89-215) without its host round trips.
    model: a PMFNet in eval mode on the device (one plan per network input shape: [T*V, ., S, S] per size and, with tta,
    [T, ., S+32, S+32]); tta: the seven-way test-time augmentation; knn_params: post.KNN.params of the config, None =
    the label at the point's pixel; tile_batch: tiles per forward (default 4, with tta 1: network batch 4 or 6).
    capture: None or a callable (S, windows, prob, prob_pad) called per group with the (h_start, h_end, w_start, w_end)
    of its tiles and the network's probabilities for them (views: copy what you keep)."""

    def __init__(self, model, nclasses, feature_mean, feature_std, img_sizes, tta=False, knn_params=None, tile_batch=None,
                 device="cuda"):
        self.model, self.nclasses, self.tta = model, int(nclasses), bool(tta)
        self.device = torch.device(device)
        self.img_sizes = [int(s) for s in img_sizes]
        for s in self.img_sizes:
            if s < 16 or s % 16 != 0:
                raise ValueError("img_size entries must be positive multiples of 16, got %r" % (s,))
        if len(feature_mean) != 8 or len(feature_std) != 8:
            raise ValueError("feature_mean / feature_std have one entry per channel of the frame (8)")
        self.tile_batch = int(tile_batch) if tile_batch is not None else (1 if tta else 4)
        if not 1 <= self.tile_batch <= MAX_TILES:
            raise ValueError("tile_batch must be in 1..%d, got %r" % (MAX_TILES, tile_batch))
        self.mean = torch.tensor(feature_mean, dtype=torch.float32).to(self.device)
        self.stds = torch.tensor(feature_std, dtype=torch.float32).to(self.device)
        self.knn = None
        if knn_params is not None:
            if int(knn_params["search"]) % 2 == 0:
                raise ValueError("Nearest neighbor kernel must be odd number")        # knn.py:73-74
            self.knn = KNN(knn_params, self.nclasses)
        self.capture = None
        self._ws = {}

    def _workspace(self, S):
        key = (S, self.tile_batch)
        ws = self._ws.get(key)
        if ws is None:
            T, V, SP = self.tile_batch, 6 if self.tta else 1, S + 2 * PAD
            e = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
            ws = [e(T * V, 5, S, S), e(T * V, 3, S, S), e(T, 5, SP, SP) if self.tta else None,
                  e(T, 3, SP, SP) if self.tta else None]
            self._ws[key] = ws
        return ws

    @torch.no_grad()
    def frame(self, data_frame, z=None, label=None, pixel_conf=None, point_conf=None):
        """data_frame: the dataset's dict (feature_map [8,h,w], label_map [h,w], h_idx / w_idx [P]); z f32[P] (the points'
        heights, needed with KNN); label uint8[P] raw point labels with point_conf; pixel_conf / point_conf: int64 [C,C]
        device tensors to add to (or None).  -> (uint8[P] device tensor = pred - 1: the bytes of the .label file,
        confidence map f32[C,h,w] on the device, number of points whose class 0 became 1); .class_map keeps the int32[h,w]
        argmax of the confidence map."""
        if self.model.training:
            raise RuntimeError("BevTileEvaluator needs the model in eval mode: tiles and variants share a forward, and "
                               "only eval-mode BatchNorm keeps batch elements independent")
        dev, Cn = self.device, self.nclasses
        fm = torch.from_numpy(np.ascontiguousarray(data_frame["feature_map"])).float().to(dev)    # the one upload
        _, h, w = fm.shape
        conf_map = torch.zeros((Cn, h, w), dtype=torch.float32, device=dev)
        T, V = self.tile_batch, 6 if self.tta else 1
        for S in self.img_sizes:
            wins = tile_windows(h, w, S)
            ws = self._workspace(S)
            for g in range(0, len(wins), T):
                real = wins[g:g + T]
                grp = real + [real[-1]] * (T - len(real))          # a short last group: one plan per size all the same
                pcd, rgb, pcd_pad, rgb_pad = bev_tile_pre(fm, self.mean, self.stds, [(a, c) for a, _, c, _ in grp], S, V,
                                                          self.tta, ws)
                prob = self.model(pcd, rgb)[0]
                prob_pad = self.model(pcd_pad, rgb_pad)[0] if self.tta else None
                if self.capture is not None:
                    self.capture(S, real, prob[:len(real) * V], None if prob_pad is None else prob_pad[:len(real)])
                bev_tile_accum(prob, [(a, c) for a, _, c, _ in real], S, V, conf_map, prob_pad)
        lab_map = None
        if pixel_conf is not None:
            lab_map = (torch.from_numpy(np.ascontiguousarray(data_frame["label_map"])).to(dev) + 1).float().contiguous()
        amap = window_argmax(conf_map, 0, 0, h, w, lab_map, pixel_conf)
        h_idx = torch.from_numpy(np.ascontiguousarray(data_frame["h_idx"])).long().to(dev)
        w_idx = torch.from_numpy(np.ascontiguousarray(data_frame["w_idx"])).long().to(dev)
        voted = None
        if self.knn is not None:
            if z is None:
                raise ValueError("the KNN vote needs the points' z")
            zt = torch.as_tensor(np.ascontiguousarray(z)).float().to(dev)
            voted = self.knn(fm[0], zt, amap, w_idx, h_idx)        # proj_range = the first height map, px = w_idx, py = h_idx
        lab = None
        if point_conf is not None:
            if label is None:
                raise ValueError("point_conf needs the points' labels")
            lab = torch.as_tensor(np.ascontiguousarray(label)).to(dev)
        n_zero = torch.zeros(1, dtype=torch.int64, device=dev)
        pred = bev_points(amap, h_idx, w_idx, Cn, voted, lab, point_conf, n_zero)
        self.class_map = amap
        return pred, conf_map, int(n_zero.item())
