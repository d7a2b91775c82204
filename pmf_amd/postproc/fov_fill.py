"""Full SemanticKITTI sweeps from field-of-view predictions: the inverse of dataset/semantic_kitti/fov.py.

A camera + LiDAR model labels only the points the left colour camera sees (the SemanticKITTI-FOV tree, or the loader's keep
mask on a raw tree); the benchmark scores every point of the sweep.  pmf_kitti_full_fill (csrc/project.hip) puts the FOV
label words back on their rows of the raw sweep -- the rows project_point keeps, in file order -- takes a LiDAR-only model's
word for every other row and one fixed id for what neither labels, for a batch of frames in three launches.  Everything is
stated on annotation ids (the words of the .label files); lut (class_map_lut) decides what counts as "unlabelled".  No GPU
work falls back to numpy: without a GPU fov_fill raises.
"""
import ctypes as C

import numpy as np

from .. import _lib as L

MAX_CLASSES = 64


def workspace_words(P):
    """int32 words of pmf_kitti_full_fill's workspace for P points"""
    return L.FULL_WS_PER_BLOCK * ((int(P) + L.FOV_BLOCK - 1) // L.FOV_BLOCK) + L.FULL_WS_FIXED


def _check_table(name, table, B, total):
    """one offsets table on the host -> int64[B + 1]: starts at 0, never decreases, ends at the length of its array"""
    t = np.ascontiguousarray(table, np.int64).reshape(-1)
    if t.shape[0] != B + 1:
        raise ValueError("fov_fill: %s holds %d entries for %d frames, it needs %d" % (name, t.shape[0], B, B + 1))
    if t[0] != 0:
        raise ValueError("fov_fill: %s[0] is %d, not 0" % (name, t[0]))
    down = np.flatnonzero(np.diff(t) < 0)
    if down.size:
        raise ValueError("fov_fill: %s decreases at frame %d (%d -> %d)" % (name, down[0], t[down[0]], t[down[0] + 1]))
    if t[B] != total:
        raise ValueError("fov_fill: %s[%d] is %d but the array it describes holds %d entries" % (name, B, t[B], total))
    return t


def _is_pair(value):
    """(concatenated array, offsets): a tuple of two whose second entry is a one-dimensional int64 array.  Per-frame arrays are
    float32 rows or 32-bit words, so a tuple of two frames is never taken for it."""
    return (isinstance(value, tuple) and len(value) == 2 and isinstance(value[1], np.ndarray) and value[1].ndim == 1
            and value[1].dtype == np.int64)


def _ragged(name, value, B, dtype, width=None):
    """a list or tuple of B per-frame arrays, or (concatenated array, offsets int64[B + 1]) -> (array, int64[B + 1] checked)"""
    def words(a, what):
        ok = isinstance(a, np.ndarray) and (a.dtype == dtype or (dtype == np.uint32 and a.dtype == np.int32)) and \
            (a.ndim == 1 if width is None else a.ndim == 2 and a.shape[1] == width)
        if not ok:
            raise ValueError("fov_fill: %s must be a %s array [%s], got %s %s" % (
                what, np.dtype(dtype).name, "n" if width is None else "n, %d" % width, getattr(a, "dtype", type(a).__name__),
                getattr(a, "shape", "")))
        return a
    if _is_pair(value):
        arr = words(value[0], name)
        return arr, _check_table("the offsets of " + name, value[1], B, arr.shape[0])
    if len(value) != B:
        raise ValueError("fov_fill: %d frames but %d arrays in %s" % (B, len(value), name))
    parts = [words(a, "%s of frame %d" % (name, b)) for b, a in enumerate(value)]
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in parts])
    empty = np.zeros((0,) if width is None else (0, width), dtype)
    return (np.concatenate(parts) if parts else empty), off


def _check_fill(frames, dims, proj_matrix, main, sub, lut, fill_id, nclasses, gt, conf):
    """everything that can be decided on the host, before any device use -> the host arrays of the upload"""
    if conf is not None and gt is None:
        raise ValueError("fov_fill: a confusion matrix needs gt, the raw label words of the data set")
    if not 1 <= int(nclasses) <= MAX_CLASSES:
        raise ValueError("fov_fill: nclasses must be in 1..%d, got %r" % (MAX_CLASSES, nclasses))
    B = len(frames[1]) - 1 if _is_pair(frames) else len(frames)
    if not 1 <= B <= L.FOV_MAX_FRAMES:
        raise ValueError("fov_fill: %d frames, a batch holds 1 to %d" % (B, L.FOV_MAX_FRAMES))
    pts, offsets = _ragged("frames", frames, B, np.float32, 4)
    P = int(offsets[B])
    if P >= 2 ** 31:
        raise ValueError("fov_fill: %d points in one batch, at most 2^31 - 1" % P)
    d = np.ascontiguousarray(dims, np.int32)
    if d.shape != (B, 2):
        raise ValueError("fov_fill: dims must hold one (h, w) per frame")
    m = np.ascontiguousarray(proj_matrix, np.float64)
    if m.size != 12:
        raise ValueError("fov_fill: the projection matrix must be 3 x 4")
    main_ids, main_off = _ragged("main", main, B, np.uint32)
    per_point = [("sub", sub)] + ([("gt", gt)] if gt is not None else [])
    words = []
    for name, value in per_point:
        if isinstance(value, np.ndarray):
            value = (value, offsets.copy())
        arr, off = _ragged(name, value, B, np.uint32)
        if not np.array_equal(off, offsets):
            b = int(np.flatnonzero(np.diff(off) != np.diff(offsets))[0])
            raise ValueError("fov_fill: frame %d has %d points but %d words in %s" % (
                b, offsets[b + 1] - offsets[b], off[b + 1] - off[b], name))
        words.append(arr)
    table = np.ascontiguousarray(lut, np.int32).reshape(-1)
    if table.shape[0] < 1:
        raise ValueError("fov_fill: an empty label table")
    if not 0 <= int(fill_id) < 2 ** 16:
        raise ValueError("fov_fill: fill_id must be an annotation id in 0..65535, got %r" % (fill_id,))
    return B, P, pts, offsets, d, m.reshape(12), main_ids, main_off, words, table


def fov_fill(frames, dims, proj_matrix, main, sub, lut, fill_id, nclasses, gt=None, conf=None, counts=None, device="cuda"):
    """frames: list of f32[P_b, 4] host arrays of ONE sequence (the raw sweeps), dims: (h, w) of every frame's image,
    proj_matrix f64[3, 4]; main: list of u32[K_b], the camera + LiDAR model's label words of the frame's FOV points in file
    order; sub: list of u32[P_b], the LiDAR-only model's label words; lut: annotation id -> class (class_map_lut), host;
    fill_id: the annotation id of what neither labels; gt: list of u32[P_b] raw label words or None.  frames and main may also
    be (concatenated array, offsets) with offsets a numpy int64[B + 1], sub and gt one concatenated array: both tables are
    checked on the host.
    conf int64[C, C] / counts int64[3]: device tensors to ADD the confusion over ALL points (needs gt) / the rows by source
    (main, sub, filled) to, or None.
    -> list of u32[P_b] host arrays: the annotation id of every point (high half zero).
    One packed upload, one pmf_kitti_full_fill call (at most FOV_MAX_FRAMES frames), one copy back that carries the labels
    and the kept rows per frame; a frame whose main prediction does not hold exactly one word per kept row is a ValueError
    naming the frame, raised before anything is returned and before conf / counts change: the call accumulates into
    tensors of its own and adds them to the caller's only after that check."""
    import torch
    from ..dataset.perspective_view_loader import upload_packed
    B, P, pts, offsets, d, m, main_ids, main_off, words, table = _check_fill(
        frames, dims, proj_matrix, main, sub, lut, fill_id, nclasses, gt, conf)
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("fov_fill runs on the GPU only (there is no host path), got device %r" % (device,))
    nclasses = int(nclasses)
    for name, t, shape in (("conf", conf, (nclasses, nclasses)), ("counts", counts, (3,))):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                                  and tuple(t.shape) == shape):
            raise ValueError("fov_fill: %s must be a contiguous int64 CUDA tensor %s" % (name, list(shape)))
    main_len = np.diff(main_off)
    if P == 0:
        kept = np.zeros(B, np.int64)
        out_h = np.zeros(0, np.uint32)
    else:
        host = [pts, offsets, d, m, main_off, table, words[0].view(np.int32)]
        host += [words[1].view(np.int32)] if gt is not None else []
        host += [main_ids.view(np.int32)] if main_ids.shape[0] else []
        up = upload_packed(host, dev)                                              # one host -> device copy
        gt_d = up[7] if gt is not None else None
        main_d = up[-1] if main_ids.shape[0] else None
        back = torch.empty(8 * B + 4 * P, dtype=torch.uint8, device=dev)           # kept_count | out: one copy back
        ws = torch.empty(workspace_words(P), dtype=torch.int32, device=dev)
        own_conf = None if conf is None else torch.zeros_like(conf)               # the caller's only after the length check
        own_counts = None if counts is None else torch.zeros_like(counts)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            rc = L.lib().pmf_kitti_full_fill(
                up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), B, P, up[3].data_ptr(), ptr(main_d), up[4].data_ptr(),
                int(main_ids.shape[0]), up[6].data_ptr(), ptr(gt_d), up[5].data_ptr(), int(table.shape[0]), int(fill_id),
                nclasses, back.data_ptr() + 8 * B, None, back.data_ptr(), ptr(own_counts), ptr(own_conf), ws.data_ptr(),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        L.check(rc, "pmf_kitti_full_fill")
        back_h = back.cpu().numpy()
        kept = back_h[:8 * B].view(np.int64)
        out_h = back_h[8 * B:].view(np.uint32)
    wrong = np.flatnonzero(kept != main_len)
    if wrong.size:
        b = int(wrong[0])
        raise ValueError("fov_fill: frame %d: the camera sees %d of its %d points but the main prediction holds %d labels "
                         "(written under another keep rule?)" % (b, kept[b], offsets[b + 1] - offsets[b], main_len[b]))
    if P:
        with torch.cuda.device(dev):
            if conf is not None:
                conf += own_conf
            if counts is not None:
                counts += own_counts
    return [out_h[offsets[b]:offsets[b + 1]] for b in range(B)]
