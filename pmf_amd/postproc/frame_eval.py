"""Per-frame device work of EPMF evaluation (tasks/epmf_eval_semantickitti/infer.py), around the network.

The reference pads every frame centred up to multiples of 64, normalises it with torch, crops the prediction back, takes
torch.argmax, gathers or KNN-votes the point labels, copies them to the host and fills two confusion matrices there.
Here that is three HIP passes (csrc/eval.hip):

  pre     proj f32[10,h,w] -> pcd f32[1,5,H,W], rgb f32[1,3,H,W], proj_depth f32[h,w]            (pmf_eval_pre)
  pixels  argmax over the (top, left, h, w) window of the padded probability map, += pixel confusion (pmf_eval_argmax)
  points  gather (or KNN vote) of the kept points' labels, += point confusion, uint32 ids     (pmf_eval_points)

nuScenes (tasks/epmf_eval_nuscenes/infer.py) has six views per sweep, padded with the rows at the bottom only, and merges
them as it goes -- SweepEvaluator:

  view    per kept point (max probability, class) or the two KNN votes, merged into the sweep's running
          (confidence, label) state where strictly more confident                              (pmf_eval_view_merge)
  finish  after the sixth view: += point confusion over the labelled points, uint8 labels, state zeroed (pmf_eval_sweep_finish)

SalsaNext range images (tasks/salsanext_eval_nuscenes/infer.py) all have the sensor's proj_h x proj_w, so B sweeps go
through the network per forward and everything behind it is one batched pass -- RangeSweepEvaluator:

  range   argmax of the B maps, += pixel confusion; per point the label at its pixel or the KNN vote, int32 labels,
          += point confusion: two launches per batch                                          (pmf_eval_range_batch)

Full nuScenes sweeps (tasks/pmf_eval_nuscenes/testset_eval/main.py, MergePred): the camera + LiDAR labels cover the points
some camera sees, a LiDAR-only prediction fills the rest, what is still 0 becomes one class, and all points are scored:

  fill    per point main != 0 ? main : sub, 0 -> fill_class; uint8 labels, += confusion over ALL points, += the three
          source counts; any number of sweeps concatenated                                    (pmf_eval_fill)
  finish  with a fallback: the plain finish and the fill in one pass over the sweep's state    (pmf_eval_sweep_finish_fill)

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


def pad_geometry_bottom(h, w):
    """pad-to-64 of the reference's nuScenes loop: -> (H, W, 0, w_pad // 2): columns centred, rows at the bottom only
    (ZeroPad2d((w_pad // 2, w_pad - w_pad // 2, 0, h_pad)))."""
    H, W, _, left = pad_geometry(h, w)
    return H, W, 0, left


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


def eval_pre(proj, mean, stds, pcd=None, rgb=None, proj_depth=None, geometry=pad_geometry):
    """proj f32[10,h,w] (the V2 loader's frame); mean / stds f32[5] on the device -> (pcd [1,5,H,W], rgb [1,3,H,W],
    proj_depth [h,w], (H, W, top, left)).  geometry: pad_geometry (centred) or pad_geometry_bottom."""
    if not (proj.is_cuda and proj.dtype == torch.float32 and proj.is_contiguous() and proj.dim() == 3
            and proj.shape[0] >= 9):
        raise ValueError("proj must be a contiguous float32 CUDA tensor [10, h, w]")
    _, h, w = proj.shape
    H, W, top, left = geometry(h, w)
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


def _check_points(x_data, y_data, src):
    K = int(x_data.shape[0])
    for t in (x_data, y_data, src):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.shape[0] == K):
            raise ValueError("x_data / y_data / src must be contiguous int32 CUDA tensors [K]")
    return K


def _check_state(conf_full, label_full):
    P = int(conf_full.shape[0])
    if not (conf_full.is_cuda and conf_full.dtype == torch.float32 and conf_full.is_contiguous() and label_full.is_cuda
            and label_full.dtype == torch.int32 and label_full.is_contiguous() and label_full.shape[0] == P):
        raise ValueError("conf_full must be a float32 and label_full an int32 contiguous CUDA tensor [P]")
    return P


def view_merge(prob, top, left, h, w, x_data, y_data, x_min, y_min, src, conf_full, label_full, argmax=None,
               proj_range=None, unproj_range=None, knn=None, knn_ws=None, conf_ws=None):
    """one view of a sweep into the running state conf_full f32[P] / label_full int32[P] (pmf_eval_view_merge): argmax None
    -> (max probability, its class) at each kept point's pixel; argmax int32[h,w] -> the KNN votes over that map and over
    the truncated confidence map (knn = (k, search, inv_gauss f32 device, cutoff), proj_range f32[h,w], unproj_range
    f32[K]).  The state is updated in place where the view is strictly more confident."""
    prob = _check_prob(prob)
    Cn, H, W = prob.shape
    dev = prob.device
    K = _check_points(x_data, y_data, src)
    P = _check_state(conf_full, label_full)
    k_, search, inv_g, cutoff = (0, 0, None, 0.0) if argmax is None else knn
    if argmax is not None:
        if proj_range is None or unproj_range is None or unproj_range.shape[0] != K or tuple(proj_range.shape) != (h, w):
            raise ValueError("the KNN vote needs proj_range [h, w] and unproj_range [K]")
        if not (argmax.is_cuda and tuple(argmax.shape) == (h, w) and argmax.dtype == torch.int32):
            raise ValueError("argmax must be an int32 CUDA tensor [h, w]")
        if not (proj_range.is_cuda and unproj_range.is_cuda and proj_range.dtype == unproj_range.dtype == torch.float32
                and proj_range.is_contiguous() and unproj_range.is_contiguous()):
            raise ValueError("proj_range / unproj_range must be contiguous float32 CUDA tensors")
        if knn_ws is None:
            knn_ws = torch.empty(4 * K + 2, dtype=torch.int64, device=dev)
        if conf_ws is None:
            conf_ws = torch.empty(h * w, dtype=torch.int32, device=dev)
    L.check(L.lib().pmf_eval_view_merge(
        prob.data_ptr(), Cn, H, W, top, left, h, w, x_data.data_ptr(), y_data.data_ptr(), int(x_min), int(y_min), K,
        src.data_ptr(), P, _ptr(argmax), _ptr(proj_range), _ptr(unproj_range), int(k_), int(search), _ptr(inv_g),
        C.c_float(float(cutoff)), _ptr(knn_ws), _ptr(conf_ws), conf_full.data_ptr(), label_full.data_ptr(), _stream(dev)),
        "pmf_eval_view_merge")


def sweep_finish(conf_full, label_full, nclasses, sem=None, lut=None, conf=None, out_u8=None):
    """after the last view (pmf_eval_sweep_finish): conf int64[C,C] += (label, lut[sem] where the label is non-zero, else
    0) over the P points, out_u8 uint8[P] = label, and the state back to zero."""
    P = _check_state(conf_full, label_full)
    if conf is not None:
        if not (conf.is_cuda and conf.dtype == torch.int64 and conf.is_contiguous()
                and tuple(conf.shape) == (nclasses, nclasses)):
            raise ValueError("conf must be a contiguous int64 CUDA tensor [%d, %d]" % (nclasses, nclasses))
        if sem is None or lut is None or not (sem.is_cuda and lut.is_cuda and sem.dtype == lut.dtype == torch.int32
                                              and sem.is_contiguous() and lut.is_contiguous() and sem.dim() == 1
                                              and sem.shape[0] >= P):
            raise ValueError("conf needs sem int32[P] and lut int32 on the device")
    else:
        sem = lut = None
    if out_u8 is not None and not (out_u8.is_cuda and out_u8.dtype == torch.uint8 and out_u8.is_contiguous()
                                   and out_u8.shape[0] >= P):
        raise ValueError("out_u8 must be a contiguous uint8 CUDA tensor [P]")
    L.check(L.lib().pmf_eval_sweep_finish(
        conf_full.data_ptr(), label_full.data_ptr(), P, _ptr(sem), _ptr(lut), 0 if lut is None else int(lut.shape[0]),
        int(nclasses), _ptr(conf), _ptr(out_u8), _stream(conf_full.device)), "pmf_eval_sweep_finish")
    return out_u8


def _check_conf(name, conf, nclasses):
    if conf is not None and not (isinstance(conf, torch.Tensor) and conf.is_cuda and conf.dtype == torch.int64
                                 and conf.is_contiguous() and tuple(conf.shape) == (nclasses, nclasses)):
        raise ValueError("%s must be a contiguous int64 CUDA tensor [%d, %d]" % (name, nclasses, nclasses))


def _check_fill(P, nclasses, sem, lut, need_gt, counts, out_u8):
    """the optional arguments the two fill entry points share -> (sem, lut) or (None, None) without a confusion"""
    if not 1 <= int(nclasses) <= 64:
        raise ValueError("nclasses must be in 1..64, got %r" % (nclasses,))
    if need_gt:
        if not (_is_dev(sem, torch.int32) and _is_dev(lut, torch.int32) and sem.dim() == 1 and lut.dim() == 1
                and sem.shape[0] == P and lut.shape[0] >= 1):
            raise ValueError("a confusion needs sem int32[%d] and lut int32 on the device" % P)
    else:
        sem = lut = None
    if counts is not None and not _is_dev(counts, torch.int64, (3,)):
        raise ValueError("counts must be a contiguous int64 CUDA tensor [3]")
    if out_u8 is not None and not _is_dev(out_u8, torch.uint8, (P,)):
        raise ValueError("out_u8 must be a contiguous uint8 CUDA tensor [%d]" % P)
    return sem, lut


def fill_labels(main, sub, nclasses, fill_class=11, sem=None, lut=None, conf=None, counts=None, out_u8=None):
    """the reference's MergePred rule on the device (pmf_eval_fill), for P points = any number of sweeps concatenated: main /
    sub int32[P] (the camera + LiDAR labels, 0 where no camera saw the point, and the LiDAR-only labels): pred = main where
    non-zero, else sub, else fill_class.  out_u8 uint8[P] = pred (numpy's astype(uint8)); conf int64[C,C] += (pred,
    lut[sem]) over ALL points (sem int32[P] raw ids, lut int32); counts int64[3] += points taken from main / from sub /
    filled.  Each output is optional.  -> out_u8."""
    if not (_is_dev(main, torch.int32) and main.dim() == 1):
        raise ValueError("main must be a contiguous int32 CUDA tensor [P]")
    P = int(main.shape[0])
    if not _is_dev(sub, torch.int32, (P,)):
        raise ValueError("sub must be a contiguous int32 CUDA tensor [%d], one label per point of main" % P)
    _check_conf("conf", conf, nclasses)
    sem, lut = _check_fill(P, nclasses, sem, lut, conf is not None, counts, out_u8)
    L.check(L.lib().pmf_eval_fill(
        main.data_ptr(), sub.data_ptr(), P, int(fill_class), _ptr(sem), _ptr(lut), 0 if lut is None else int(lut.shape[0]),
        int(nclasses), _ptr(conf), _ptr(counts), _ptr(out_u8), _stream(main.device)), "pmf_eval_fill")
    return out_u8


def sweep_finish_fill(conf_full, label_full, sub, nclasses, fill_class=11, sem=None, lut=None, conf=None, fused_conf=None,
                      counts=None, out_cam_u8=None, out_u8=None):
    """sweep_finish and fill_labels(label_full, sub) in one pass over the state (pmf_eval_sweep_finish_fill): conf /
    out_cam_u8 as sweep_finish gives them (camera-only, scored where the label is non-zero), fused_conf / counts / out_u8 as
    fill_labels gives them, and the state back to zero.  -> out_u8."""
    P = _check_state(conf_full, label_full)
    if not _is_dev(sub, torch.int32, (P,)):
        raise ValueError("sub must be a contiguous int32 CUDA tensor [%d], one label per point of the sweep" % P)
    _check_conf("conf", conf, nclasses)
    _check_conf("fused_conf", fused_conf, nclasses)
    sem, lut = _check_fill(P, nclasses, sem, lut, conf is not None or fused_conf is not None, counts, out_u8)
    if out_cam_u8 is not None and not _is_dev(out_cam_u8, torch.uint8, (P,)):
        raise ValueError("out_cam_u8 must be a contiguous uint8 CUDA tensor [%d]" % P)
    L.check(L.lib().pmf_eval_sweep_finish_fill(
        conf_full.data_ptr(), label_full.data_ptr(), P, sub.data_ptr(), int(fill_class), _ptr(sem), _ptr(lut),
        0 if lut is None else int(lut.shape[0]), int(nclasses), _ptr(conf), _ptr(fused_conf), _ptr(counts),
        _ptr(out_cam_u8), _ptr(out_u8), _stream(conf_full.device)), "pmf_eval_sweep_finish_fill")
    return out_u8


class SweepEvaluator(FrameEvaluator):
    """nuScenes: the views of one sweep at a time.  pre() / post_view() per view, finish() after the last one; the
    running (confidence, label) state of the sweep lives on the device, sized to the largest sweep seen, zero between
    sweeps.  Workspaces are FrameEvaluator's grow-only ones; returned tensors are views of them."""

    def __init__(self, nclasses, pcd_mean, pcd_stds, knn_params=None, device="cuda"):
        super().__init__(nclasses, pcd_mean, pcd_stds, knn_params, device)
        self.views_in_sweep = 0
        self.n_points = 0
        self._conf_full = self._label_full = None

    def pre(self, proj):
        """-> (pcd [1,5,H,W], rgb [1,3,H,W]) padded at the bottom / centred columns; keeps proj_depth and the geometry."""
        if not isinstance(proj, torch.Tensor) or proj.dim() != 3:
            raise ValueError("proj must be a contiguous float32 CUDA tensor [10, h, w]")
        _, h, w = proj.shape
        H, W, _, _ = pad_geometry_bottom(h, w)
        pcd, rgb, self.proj_depth, self.geometry = eval_pre(
            proj, self.mean, self.stds, self._ws("pcd", (1, 5, H, W), torch.float32),
            self._ws("rgb", (1, 3, H, W), torch.float32), self._ws("pdepth", (h, w), torch.float32),
            geometry=pad_geometry_bottom)
        self.proj = proj
        return pcd, rgb

    def post(self, *a, **kw):
        raise TypeError("SweepEvaluator: use post_view() per view and finish() per sweep")

    def _state(self, n_points):
        if self._conf_full is None or self._conf_full.shape[0] < n_points:       # only between sweeps: the state is zero
            self._conf_full = torch.zeros(n_points, dtype=torch.float32, device=self.device)
            self._label_full = torch.zeros(n_points, dtype=torch.int32, device=self.device)
        return self._conf_full[:n_points], self._label_full[:n_points]

    def post_view(self, prob, depth, extra, pixel_conf=None):
        """prob: the probability map [1, C, H, W] of the view pre() prepared; depth f32[K] and extra (the loader's
        _eval_item: x_data, y_data, x_min, y_min, src, sem int32[P]); pixel_conf int64[C,C] to add the view's pixel
        confusion to (or None).  Merges the view into the sweep's state."""
        prob = _check_prob(prob)
        if self.geometry is None:
            raise RuntimeError("post_view() before pre()")
        H, W, top, left = self.geometry
        _, h, w = self.proj.shape
        if tuple(prob.shape) != (self.nclasses, H, W):
            raise ValueError("prob is %s, the view was padded to %dx%d with %d classes" % (
                tuple(prob.shape), H, W, self.nclasses))
        n_points = int(extra["sem"].shape[0])
        if self.views_in_sweep and n_points != self.n_points:
            raise RuntimeError("view of a sweep with %d points inside a sweep of %d points (finish() missing?)" % (
                n_points, self.n_points))
        conf_full, label_full = self._state(n_points)
        self.n_points = n_points
        use_knn = self.knn is not None
        amap = None
        if use_knn or pixel_conf is not None:
            amap = window_argmax(prob, top, left, h, w, self.proj[9] if pixel_conf is not None else None, pixel_conf,
                                 want_map=use_knn, out=self._ws("amap", (h, w), torch.int32) if use_knn else None)
        K = int(extra["x_data"].shape[0])
        view_merge(prob, top, left, h, w, extra["x_data"], extra["y_data"], extra["x_min"], extra["y_min"], extra["src"],
                   conf_full, label_full, argmax=amap if use_knn else None, proj_range=self.proj_depth,
                   unproj_range=depth, knn=self.knn,
                   knn_ws=self._ws("knn", (4 * K + 2,), torch.int64) if use_knn else None,
                   conf_ws=self._ws("cmap", (h * w,), torch.int32) if use_knn else None)
        self.views_in_sweep += 1

    def finish(self, sem, lut, n_points, point_conf=None, want_labels=True, fallback=None, fill_class=11, fused_conf=None,
               counts=None):
        """after the last view of the sweep: point_conf int64[C,C] += the sweep's point confusion (sem int32[P] raw ids, lut
        int32), -> uint8[P] labels (None unless want_labels); the state is zero again.
        fallback int32[P] (a LiDAR-only prediction of the same sweep): the same pass also fills the points no camera
        labelled (fill_labels' rule), fused_conf int64[C,C] += the confusion over ALL points, counts int64[3] += the source
        counts, and the labels returned are the FUSED uint8 labels."""
        if self.views_in_sweep == 0:
            raise RuntimeError("finish() without a view")
        if int(n_points) != self.n_points:
            raise RuntimeError("finish() for %d points, the sweep's views carried %d" % (int(n_points), self.n_points))
        conf_full, label_full = self._state(self.n_points)
        out = self._ws("labels_u8", (self.n_points,), torch.uint8) if want_labels else None
        if fallback is None:
            if fused_conf is not None or counts is not None:
                raise ValueError("fused_conf / counts need a fallback prediction")
            out = sweep_finish(conf_full, label_full, self.nclasses, sem, lut, point_conf, out)
        else:
            out = sweep_finish_fill(conf_full, label_full, fallback, self.nclasses, fill_class, sem, lut, point_conf,
                                    fused_conf, counts, None, out)
        self.views_in_sweep = 0
        return out


def _is_dev(t, dtype, shape=None):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and (shape is None or tuple(t.shape) == tuple(shape)))


def range_batch_eval(prob, proj_range, offsets, px, py, unproj_range, sem=None, lut=None, label=None, knn=None,
                     pixel_conf=None, point_conf=None, argmax_ws=None, labels=None):
    """B range-image sweeps in one call (pmf_eval_range_batch).  prob f32[B,C,H,W]; proj_range f32[B,H,W]; the points of
    the B sweeps concatenated: px (column) / py (row) int32[P], unproj_range f32[P], sem int32[P] raw ids, sweep b owning
    [offsets[b], offsets[b+1]) (offsets int64[B+1] on the device); lut int32; label f32[B,H,W] with pixel_conf; knn None
    (the label at the point's pixel) or (k, search, inv_gauss f32 device, cutoff); pixel_conf / point_conf int64[C,C]
    to add to, or None.  -> (labels int32[P], argmax int32[B,H,W]).  All tensors contiguous on the device."""
    if knn is not None and int(knn[1]) % 2 == 0:
        raise ValueError("Nearest neighbor kernel must be odd number")        # knn.py:73-74
    if not (isinstance(prob, torch.Tensor) and prob.dim() == 4 and _is_dev(prob, torch.float32)):
        raise ValueError("prob must be a contiguous float32 CUDA tensor [B, C, H, W]")
    B, Cn, H, W = prob.shape
    dev = prob.device
    if not _is_dev(offsets, torch.int64, (B + 1,)):
        raise ValueError("offsets must be a contiguous int64 CUDA tensor [B + 1]")
    if not (_is_dev(px, torch.int32) and px.dim() == 1 and _is_dev(py, torch.int32, px.shape)):
        raise ValueError("px / py must be contiguous int32 CUDA tensors [P]")
    P = int(px.shape[0])
    if knn is not None:
        if not (_is_dev(proj_range, torch.float32, (B, H, W)) and _is_dev(unproj_range, torch.float32, (P,))):
            raise ValueError("the KNN vote needs proj_range float32 [B, H, W] and unproj_range float32 [P] on the device")
        if not _is_dev(knn[2], torch.float32, (int(knn[1]) ** 2,)):
            raise ValueError("inv_gauss must be a float32 CUDA tensor [search * search]")
    if (label is None) != (pixel_conf is None):
        raise ValueError("label and pixel_conf go together")
    for name, c in (("pixel_conf", pixel_conf), ("point_conf", point_conf)):
        if c is not None and not _is_dev(c, torch.int64, (Cn, Cn)):
            raise ValueError("%s must be a contiguous int64 CUDA tensor [%d, %d]" % (name, Cn, Cn))
    if label is not None and not _is_dev(label, torch.float32, (B, H, W)):
        raise ValueError("label must be a contiguous float32 CUDA tensor [B, H, W]")
    if point_conf is not None and not (_is_dev(sem, torch.int32, (P,)) and _is_dev(lut, torch.int32)
                                       and lut.dim() == 1 and lut.shape[0] >= 1):
        raise ValueError("point_conf needs sem int32 [P] and lut int32 on the device")
    if argmax_ws is None:
        argmax_ws = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    elif not (_is_dev(argmax_ws, torch.int32) and argmax_ws.numel() == B * H * W):
        raise ValueError("argmax_ws must be a contiguous int32 CUDA tensor of B * H * W elements")
    if labels is None:
        labels = torch.empty(P, dtype=torch.int32, device=dev)
    elif not _is_dev(labels, torch.int32, (P,)):
        raise ValueError("labels must be a contiguous int32 CUDA tensor [P]")
    k_, search, inv_g, cutoff = (0, 0, None, 0.0) if knn is None else knn
    nlut = int(lut.shape[0]) if point_conf is not None else 0
    L.check(L.lib().pmf_eval_range_batch(
        prob.data_ptr(), B, Cn, H, W, _ptr(label), _ptr(proj_range if knn is not None else None), offsets.data_ptr(), P,
        px.data_ptr(), py.data_ptr(), _ptr(unproj_range if knn is not None else None),
        _ptr(sem if point_conf is not None else None), _ptr(lut if point_conf is not None else None), nlut, int(k_),
        int(search), _ptr(inv_g), C.c_float(float(cutoff)), argmax_ws.data_ptr(), labels.data_ptr(), _ptr(pixel_conf),
        _ptr(point_conf), _stream(dev)), "pmf_eval_range_batch")
    return labels, argmax_ws.view(B, H, W)


class RangeSweepEvaluator(object):
    """SalsaNext range images, B sweeps per forward: post() is the whole device work behind the network for a batch.
    Owns the workspaces (grow-only, reused across batches: returned tensors are views, consume them before the next
    batch) and the cached inverse-Gaussian window.  knn_params: post.KNN.params of the config, None = gather."""

    def __init__(self, nclasses, knn_params=None, device="cuda"):
        self.nclasses = int(nclasses)
        self.device = torch.device(device)
        self.knn = None
        if knn_params is not None:
            search = int(knn_params["search"])
            if search % 2 == 0:
                raise ValueError("Nearest neighbor kernel must be odd number")        # knn.py:73-74
            w = inverse_gaussian_window(search, knn_params["sigma"]).to(self.device)
            self.knn = (int(knn_params["knn"]), search, w, float(knn_params["cutoff"]))
        self._buf = {}
        self.labels = None          # int32[P] of the last batch, all its sweeps in order (what post() returns slices of)

    _ws = FrameEvaluator._ws

    def post(self, prob, items, pixel_conf=None, point_conf=None):
        """prob: the network's probability maps [B, C, H, W] of the B sweeps in items; items: B dicts of the loader's
        _eval_item (label f32[H,W], proj_range f32[H,W], px / py int32[P_b], depth f32[P_b], sem int32[P_b], lut int32);
        pixel_conf / point_conf: int64 [C, C] device tensors to add to (or None).  The ragged point arrays are
        concatenated with one copy per array.  -> list of B int32 label tensors (views of one workspace)."""
        B = len(items)
        if not (isinstance(prob, torch.Tensor) and prob.dim() == 4 and prob.shape[0] == B):
            raise ValueError("prob must be [B, C, H, W] with one map per item")
        if B == 0:
            self.labels = torch.empty(0, dtype=torch.int32, device=self.device)
            return []
        H, W = prob.shape[2], prob.shape[3]
        counts = [int(it["px"].shape[0]) for it in items]
        P = sum(counts)
        off = [0]
        for n in counts:
            off.append(off[-1] + n)
        offsets = torch.tensor(off, dtype=torch.int64).to(self.device, non_blocking=True)
        cat = lambda key, dtype: torch.cat([it[key] for it in items], out=self._ws(key, (P,), dtype))
        px, py = cat("px", torch.int32), cat("py", torch.int32)
        use_knn = self.knn is not None
        depth = cat("depth", torch.float32) if use_knn else None
        sem = cat("sem", torch.int32) if point_conf is not None else None
        rng = torch.stack([it["proj_range"] for it in items], out=self._ws("range", (B, H, W), torch.float32)) \
            if use_knn else None
        label = torch.stack([it["label"] for it in items], out=self._ws("label", (B, H, W), torch.float32)) \
            if pixel_conf is not None else None
        labels, _ = range_batch_eval(
            prob, rng, offsets, px, py, depth, sem=sem, lut=items[0]["lut"] if point_conf is not None else None,
            label=label, knn=self.knn, pixel_conf=pixel_conf, point_conf=point_conf,
            argmax_ws=self._ws("amap", (B, H, W), torch.int32), labels=self._ws("labels", (P,), torch.int32))
        self.labels = labels
        return [labels[off[b]:off[b + 1]] for b in range(B)]
