"""Per-frame device work of EPMF evaluation (tasks/epmf_eval_semantickitti/infer.py), around the network.

The reference pads every frame centred up to multiples of 64, normalises it with torch, crops the prediction back, takes
torch.argmax, gathers or KNN-votes the point labels, copies them to the host and fills two confusion matrices there.
Here that is three HIP passes (csrc/eval.hip):

  pre     proj f32[10,h,w] -> pcd f32[1,5,H,W], rgb f32[1,3,H,W], proj_depth f32[h,w]            (pmf_eval_pre)
  pixels  argmax over the (top, left, h, w) window of the padded probability map, += pixel confusion (pmf_eval_argmax)
  points  gather (or KNN vote) of the kept points' labels, += point confusion, uint32 ids     (pmf_eval_points)

The confusion matrices are IOUEval.conf_matrix tensors (int64, on the device) updated in place; call
IOUEval.external_update() after a frame.  No GPU work falls back to torch: a missing kernel is an error.
"""
import ctypes as C
import math

import torch

from .. import _lib as L
from .knn import inverse_gaussian_window


def pad_geometry(h, w):
    """centred pad-to-64 of the reference: -> (H, W, top, left) with h_pad = ceil(h / 64) * 64 - h, top = h_pad // 2
    (ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, h_pad // 2, h_pad - h_pad // 2)))."""
    h_pad = int(math.ceil(h / 64.0)) * 64 - h
    w_pad = int(math.ceil(w / 64.0)) * 64 - w
    return h + h_pad, w + w_pad, h_pad // 2, w_pad // 2


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check_prob(prob):
    if prob.dim() == 4:
        if prob.shape[0] != 1:
            raise ValueError("frame evaluation takes one frame: prob [1, C, H, W], got %s" % (tuple(prob.shape),))
        prob = prob[0]
    if not (prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous()):
        raise ValueError("prob must be a contiguous float32 CUDA tensor [C, H, W]")
    return prob


def eval_pre(proj, mean, stds, pcd=None, rgb=None, proj_depth=None):
    """proj f32[10,h,w] (the V2 loader's frame); mean / stds f32[5] on the device -> (pcd [1,5,H,W], rgb [1,3,H,W],
    proj_depth [h,w], (H, W, top, left))."""
    if not (proj.is_cuda and proj.dtype == torch.float32 and proj.is_contiguous() and proj.dim() == 3
            and proj.shape[0] >= 9):
        raise ValueError("proj must be a contiguous float32 CUDA tensor [10, h, w]")
    _, h, w = proj.shape
    H, W, top, left = pad_geometry(h, w)
    dev = proj.device
    pcd = torch.empty((1, 5, H, W), dtype=torch.float32, device=dev) if pcd is None else pcd
    rgb = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) if rgb is None else rgb
    proj_depth = torch.empty((h, w), dtype=torch.float32, device=dev) if proj_depth is None else proj_depth
    L.check(L.lib().pmf_eval_pre(proj.data_ptr(), h, w, H, W, top, left, mean.data_ptr(), stds.data_ptr(),
                                 pcd.data_ptr(), rgb.data_ptr(), proj_depth.data_ptr(), _stream(dev)), "pmf_eval_pre")
    return pcd, rgb, proj_depth, (H, W, top, left)


def window_argmax(prob, top, left, h, w, label=None, conf=None, want_map=True, out=None):
    """argmax int32[h,w] of prob [C,H,W] over the window at (top, left) (None unless want_map); label f32[h,w] +
    conf int64[C,C] (both or neither): conf[argmax, label] += 1 per window pixel."""
    prob = _check_prob(prob)
    Cn, H, W = prob.shape
    if (label is None) != (conf is None):
        raise ValueError("label and conf go together")
    if conf is not None:
        if not (conf.dtype == torch.int64 and conf.is_contiguous() and tuple(conf.shape) == (Cn, Cn)):
            raise ValueError("conf must be a contiguous int64 [%d, %d] tensor" % (Cn, Cn))
        if not (label.dtype == torch.float32 and label.is_contiguous() and tuple(label.shape) == (h, w)):
            raise ValueError("label must be a contiguous float32 [h, w] tensor")
    amap = None
    if want_map:
        amap = torch.empty((h, w), dtype=torch.int32, device=prob.device) if out is None else out
    L.check(L.lib().pmf_eval_argmax(prob.data_ptr(), Cn, H, W, top, left, h, w, _ptr(label), _ptr(amap), _ptr(conf),
                                    _stream(prob.device)), "pmf_eval_argmax")
    return amap


def point_labels(prob, top, left, h, w, x_data, y_data, x_min, y_min, argmax=None, proj_range=None, unproj_range=None,
                 knn=None, sem=None, src=None, lut=None, conf=None, lut_inv=None, want_labels=True, knn_ws=None,
                 labels=None, labels_inv=None):
    """labels of the K kept points at (x_data - x_min, y_data - y_min) of the window: argmax None -> read from prob
    (gather); argmax int32[h,w] -> KNN vote (knn = (k, search, inv_gauss f32 device, cutoff), proj_range f32[h,w],
    unproj_range f32[K]).  conf int64[C,C] += (label, lut[sem[src]]); lut_inv -> also uint32 labels_inv.
    Returns (labels int32[K] or None, labels_inv uint32[K] or None)."""
    prob = _check_prob(prob)
    Cn, H, W = prob.shape
    dev = prob.device
    K = int(x_data.shape[0])
    if not (x_data.dtype == y_data.dtype == torch.int32 and y_data.shape[0] == K):
        raise ValueError("x_data / y_data must be int32 [K]")
    if conf is not None:
        if not (conf.dtype == torch.int64 and conf.is_contiguous() and tuple(conf.shape) == (Cn, Cn)):
            raise ValueError("conf must be a contiguous int64 [%d, %d] tensor" % (Cn, Cn))
        if sem is None or lut is None:
            raise ValueError("conf needs sem and lut")
        if not (sem.dtype == lut.dtype == torch.int32 and (src is None or (src.dtype == torch.int32 and src.shape[0] == K))
                and (src is not None or sem.shape[0] == K)):
            raise ValueError("sem / lut / src must be int32, src (or sem without src) one entry per point")
    if lut_inv is not None and lut_inv.dtype != torch.int32:
        raise ValueError("lut_inv must be int32")
    k_, search, inv_g, cutoff = (0, 0, None, 0.0) if argmax is None else knn
    if argmax is not None:
        if proj_range is None or unproj_range is None or unproj_range.shape[0] != K or tuple(proj_range.shape) != (h, w):
            raise ValueError("the KNN vote needs proj_range [h, w] and unproj_range [K]")
        if tuple(argmax.shape) != (h, w) or argmax.dtype != torch.int32:
            raise ValueError("argmax must be int32 [h, w]")
        if knn_ws is None:
            knn_ws = torch.empty(3 * K + 2, dtype=torch.int64, device=dev)
    if want_labels and labels is None:
        labels = torch.empty(K, dtype=torch.int32, device=dev)
    if lut_inv is not None and labels_inv is None:
        labels_inv = torch.empty(K, dtype=torch.int32, device=dev)        # uint32 bits (torch has no uint32 kernels)
    L.check(L.lib().pmf_eval_points(
        prob.data_ptr(), Cn, H, W, top, left, h, w, x_data.data_ptr(), y_data.data_ptr(), int(x_min), int(y_min), K,
        _ptr(argmax), _ptr(proj_range), _ptr(unproj_range), int(k_), int(search), _ptr(inv_g), C.c_float(float(cutoff)),
        _ptr(knn_ws), _ptr(sem), _ptr(src), _ptr(lut), 0 if lut is None else int(lut.shape[0]), _ptr(conf),
        _ptr(lut_inv), 0 if lut_inv is None else int(lut_inv.shape[0]), _ptr(labels if want_labels else None),
        _ptr(labels_inv), _stream(dev)), "pmf_eval_points")
    return (labels if want_labels else None), labels_inv


class FrameEvaluator(object):
    """the three passes for one frame at a time, with grow-only workspaces reused across frames (frame sizes differ).
    Tensors returned by pre() / post() are views of those workspaces: consume them before the next frame."""

    def __init__(self, nclasses, pcd_mean, pcd_stds, knn_params=None, device="cuda"):
        self.nclasses = int(nclasses)
        self.device = torch.device(device)
        self.mean = torch.tensor(pcd_mean, dtype=torch.float32).to(self.device)
        self.stds = torch.tensor(pcd_stds, dtype=torch.float32).to(self.device)
        self.knn = None
        if knn_params is not None:
            search = int(knn_params["search"])
            if search % 2 == 0:
                raise ValueError("Nearest neighbor kernel must be odd number")        # knn.py:73-74
            w = inverse_gaussian_window(search, knn_params["sigma"]).to(self.device)
            self.knn = (int(knn_params["knn"]), search, w, float(knn_params["cutoff"]))
        self._buf = {}
        self.geometry = None

    def _ws(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= int(s)
        b = self._buf.get(name)
        if b is None or b.numel() < n or b.dtype != dtype:
            b = torch.empty(max(n, 1), dtype=dtype, device=self.device)
            self._buf[name] = b
        return b[:n].view(shape)

    def pre(self, proj):
        """-> (pcd [1,5,H,W], rgb [1,3,H,W]); keeps proj_depth and the pad geometry for post()."""
        _, h, w = proj.shape
        H, W, _, _ = pad_geometry(h, w)
        pcd, rgb, self.proj_depth, self.geometry = eval_pre(
            proj, self.mean, self.stds, self._ws("pcd", (1, 5, H, W), torch.float32),
            self._ws("rgb", (1, 3, H, W), torch.float32), self._ws("pdepth", (h, w), torch.float32))
        self.proj = proj
        return pcd, rgb

    def post(self, prob, depth, extra, pixel_conf=None, point_conf=None, lut_inv=None, want_labels=False):
        """prob: the network's probability map [1, C, H, W] of the frame pre() prepared; depth f32[K] and extra (the
        loader's _eval_item); pixel_conf / point_conf: int64 [C, C] device tensors to add to (or None).
        -> (labels int32[K] or None, labels_inv uint32[K] as int32 or None)."""
        H, W, top, left = self.geometry
        _, h, w = self.proj.shape
        prob = _check_prob(prob)
        if tuple(prob.shape[1:]) != (H, W):
            raise ValueError("prob is %s, the frame was padded to %dx%d" % (tuple(prob.shape), H, W))
        amap = None
        if self.knn is not None or pixel_conf is not None:
            amap = window_argmax(prob, top, left, h, w, self.proj[9] if pixel_conf is not None else None, pixel_conf,
                                 want_map=self.knn is not None,
                                 out=self._ws("amap", (h, w), torch.int32) if self.knn is not None else None)
        K = int(extra["x_data"].shape[0])
        return point_labels(
            prob, top, left, h, w, extra["x_data"], extra["y_data"], extra["x_min"], extra["y_min"],
            argmax=amap if self.knn is not None else None, proj_range=self.proj_depth, unproj_range=depth, knn=self.knn,
            sem=extra["sem"], src=extra["src"], lut=extra["lut"], conf=point_conf, lut_inv=lut_inv,
            want_labels=want_labels,
            knn_ws=self._ws("knn", (3 * K + 2,), torch.int64) if self.knn is not None else None,
            labels=self._ws("labels", (K,), torch.int32) if want_labels else None,
            labels_inv=self._ws("labels_inv", (K,), torch.int32) if lut_inv is not None else None)
