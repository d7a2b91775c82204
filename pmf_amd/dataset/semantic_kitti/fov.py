"""SemanticKITTI-FOV on the device: the points of every sweep that the left colour camera sees
(tasks/process_semantickitti_fov/create_fov_dataset.py of the reference), a batch of frames per pass.

The reference decodes the PNG to learn its size, runs a float64 matmul over the sweep on the host, builds a mask,
fancy-indexes two arrays and writes two files, frame by frame.  Here the image size comes from the PNG header, a batch of
sweeps goes up in one copy, pmf_fov_filter (csrc/project.hip) applies the loader's own keep rule -- project_point, the one
pmf_project_scatter / pmf_project_scatter2 use -- and compacts rows and label words in file order, and only the kept
prefix comes back.  The written tree is therefore exactly the set of points PerspectiveViewLoader keeps.  No GPU work falls
back to numpy: without a GPU fov_filter_gpu raises.
"""
import ctypes as C
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ... import _lib as L
from .parser import DEFAULT_CONFIG, SemanticKitti

MAX_IO_THREADS = 8


def _check_batch(frames, dims, proj_matrix, labels):
    """shapes and offsets of one batch, on the host -> (offsets i64[B + 1], dims i32[B, 2], proj f64[12])"""
    B = len(frames)
    if not 1 <= B <= L.FOV_MAX_FRAMES:
        raise ValueError("fov_filter_gpu: %d frames, a batch holds 1 to %d" % (B, L.FOV_MAX_FRAMES))
    if len(dims) != B:
        raise ValueError("fov_filter_gpu: %d frames but %d image sizes" % (B, len(dims)))
    if labels is not None and len(labels) != B:
        raise ValueError("fov_filter_gpu: %d frames but %d label arrays" % (B, len(labels)))
    offsets = np.zeros(B + 1, np.int64)
    for b, f in enumerate(frames):
        if not (isinstance(f, np.ndarray) and f.dtype == np.float32 and f.ndim == 2 and f.shape[1] == 4):
            raise ValueError("fov_filter_gpu: frame %d must be a float32 array [P, 4], got %s %s"
                             % (b, getattr(f, "dtype", type(f).__name__), getattr(f, "shape", "")))
        if labels is not None:
            lab = labels[b]
            if not (isinstance(lab, np.ndarray) and lab.dtype in (np.uint32, np.int32) and lab.ndim == 1):
                raise ValueError("fov_filter_gpu: labels of frame %d must be a one-dimensional uint32 array" % b)
            if lab.shape[0] != f.shape[0]:
                raise ValueError("fov_filter_gpu: frame %d has %d points but %d labels" % (b, f.shape[0], lab.shape[0]))
        offsets[b + 1] = offsets[b] + f.shape[0]
    d = np.ascontiguousarray(dims, np.int32)
    if d.shape != (B, 2):
        raise ValueError("fov_filter_gpu: dims must hold one (h, w) per frame")
    if offsets[B] >= 2 ** 31:
        raise ValueError("fov_filter_gpu: %d points in one batch, at most 2^31 - 1" % offsets[B])
    m = np.ascontiguousarray(proj_matrix, np.float64)
    if m.size != 12:
        raise ValueError("fov_filter_gpu: the projection matrix must be 3 x 4")
    return offsets, d, m.reshape(12)


def fov_filter_gpu(frames, dims, proj_matrix, labels=None, device="cuda"):
    """frames: list of f32[P_b, 4] host arrays of ONE sequence, dims: (h, w) of every frame's image, proj_matrix f64[3, 4],
    labels: list of u32[P_b] raw .label words or None -> list of (points f32[K_b, 4], labels u32[K_b] or None,
    keep bool[P_b]) host arrays: the rows project_point keeps, in file order, rows and words copied as bits.
    One upload and one pmf_fov_filter call for the batch (at most FOV_MAX_FRAMES frames); out_offsets and the keep mask come
    back in one copy, then the kept prefix of the rows and of the label words: nothing of the rows' capacity comes back."""
    import torch
    from ..perspective_view_loader import upload_packed
    offsets, d, m = _check_batch(frames, dims, proj_matrix, labels)
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("fov_filter_gpu runs on the GPU only (there is no host path), got device %r" % (device,))
    B, P = len(frames), int(offsets[-1])
    if P == 0:
        return [(f[:0].copy(), None if labels is None else labels[b][:0].view(np.uint32).copy(), np.zeros(0, bool))
                for b, f in enumerate(frames)]
    host = [np.concatenate(frames), offsets, d, m]
    if labels is not None:
        host.append(np.concatenate([lab.view(np.int32) for lab in labels]))
    up = upload_packed(host, dev)
    pts, off_d, dim_d, mat_d = up[:4]
    lab_d = up[4] if labels is not None else None
    head = torch.empty(8 * (B + 1) + P, dtype=torch.uint8, device=dev)         # out_offsets | keep: one copy back
    out_off, keep = head[:8 * (B + 1)].view(torch.int64), head[8 * (B + 1):]
    out_pts = torch.empty((P, 4), dtype=torch.float32, device=dev)
    out_lab = torch.empty(P, dtype=torch.int32, device=dev) if labels is not None else None
    blk = torch.empty((P + L.FOV_BLOCK - 1) // L.FOV_BLOCK + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.lib().pmf_fov_filter(pts.data_ptr(), None if lab_d is None else lab_d.data_ptr(), off_d.data_ptr(),
                                    dim_d.data_ptr(), B, P, mat_d.data_ptr(), keep.data_ptr(), out_pts.data_ptr(),
                                    None if out_lab is None else out_lab.data_ptr(), out_off.data_ptr(), blk.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "pmf_fov_filter")
    head_h = head.cpu().numpy()
    o = head_h[:8 * (B + 1)].view(np.int64)
    keep_h = head_h[8 * (B + 1):].view(bool)
    if o[0] != 0 or (np.diff(o) < 0).any() or o[B] > P:
        raise RuntimeError("pmf_fov_filter: inconsistent out_offsets %r" % (o.tolist(),))
    K = int(o[B])
    pts_h = out_pts[:K].cpu().numpy()
    lab_h = out_lab[:K].cpu().numpy().view(np.uint32) if labels is not None else None
    return [(pts_h[o[b]:o[b + 1]], None if lab_h is None else lab_h[o[b]:o[b + 1]], keep_h[offsets[b]:offsets[b + 1]])
            for b in range(B)]


def _frame_id(path):
    return os.path.basename(path).split(".")[0]


def _read_frame(pcd_path, label_path, image_path):
    """-> (points f32[P, 4], label words u32[P] or None, (h, w)); the image size from the PNG header, nothing is decoded"""
    from PIL import Image
    pts = np.fromfile(pcd_path, dtype=np.float32)
    if pts.size % 4:
        raise ValueError("%s: %d floats are no whole number of x, y, z, intensity rows" % (pcd_path, pts.size))
    pts = pts.reshape(-1, 4)
    lab = None
    if label_path is not None:
        lab = np.fromfile(label_path, dtype=np.uint32)
        if lab.shape[0] != pts.shape[0]:
            raise ValueError("%s holds %d labels, %s holds %d points" % (label_path, lab.shape[0], pcd_path, pts.shape[0]))
    with Image.open(image_path) as im:
        w, h = im.size
    return pts, lab, (h, w)


def _write_frame(pcd_path, label_path, pts, lab):
    np.ascontiguousarray(pts, np.float32).tofile(pcd_path)
    if label_path is not None:
        np.ascontiguousarray(lab, np.uint32).tofile(label_path)


def create_fov_dataset(src_root, dst_root, sequences, config_path=None, batch_frames=16, io_threads=4, has_label=True,
                       overwrite=False, filter_fn=fov_filter_gpu):
    """src_root/<seq>/{velodyne,labels,image_2,calib.txt} -> dst_root/<seq>/ with the same layout, every sweep reduced to the
    points its image sees: velodyne/<frame>.bin (float32 rows), labels/<frame>.label (the uint32 words of the kept points;
    not written with has_label=False), image_2/ copied byte for byte, calib.txt copied, poses.txt / times.txt copied when
    present.  A frame that keeps no point writes empty files.  Frames are read by a pool of io_threads (at most 8) threads,
    filtered batch_frames (at most FOV_MAX_FRAMES) at a time by filter_fn and written by the pool; the result does not
    depend on either number.  An existing dst_root/<seq> is a FileExistsError before anything is written unless overwrite,
    which replaces its velodyne / labels / image_2.
    -> {seq: {"frames", "points_read", "points_kept", "seconds"}}"""
    batch_frames = max(1, min(int(batch_frames), L.FOV_MAX_FRAMES))
    io_threads = max(1, min(int(io_threads), MAX_IO_THREADS))
    config_path = DEFAULT_CONFIG if config_path is None else config_path
    seqs = sorted("{0:02d}".format(int(s)) for s in sequences)
    for seq in seqs:
        src, dst = os.path.join(src_root, seq), os.path.join(dst_root, seq)
        if not os.path.isfile(os.path.join(src, "calib.txt")):
            raise FileNotFoundError("%s: no calib.txt" % src)
        if os.path.exists(dst):
            if os.path.realpath(src) == os.path.realpath(dst):
                raise ValueError("%s: source and destination are the same directory" % src)
            if not overwrite:
                raise FileExistsError("%s exists (pass overwrite=True to replace it)" % dst)
    stats = {}
    with ThreadPoolExecutor(max_workers=io_threads) as pool:
        for seq in seqs:
            stats[seq] = _one_sequence(pool, src_root, dst_root, seq, config_path, batch_frames, has_label, filter_fn)
    return stats


def _one_sequence(pool, src_root, dst_root, seq, config_path, batch_frames, has_label, filter_fn):
    t0 = time.time()
    ds = SemanticKitti(src_root, [seq], config_path, has_image=True, has_pcd=True, has_label=has_label)
    n = len(ds)
    ids = [_frame_id(p) for p in ds.pointcloud_files]
    names = [ids, [_frame_id(p) for p in ds.image_files]] + ([[_frame_id(p) for p in ds.label_files]] if has_label else [])
    if any(other != ids for other in names[1:]):
        raise ValueError("%s: velodyne, image_2 and labels do not hold the same frames" % os.path.join(src_root, seq))
    src, dst = os.path.join(src_root, seq), os.path.join(dst_root, seq)
    for sub in ("velodyne", "image_2") + (("labels",) if has_label else ()):
        if os.path.isdir(os.path.join(dst, sub)):           # overwrite: no frame of an earlier run stays behind
            shutil.rmtree(os.path.join(dst, sub))
        os.makedirs(os.path.join(dst, sub))
    proj = np.ascontiguousarray(ds.proj_matrix[seq], np.float64)
    copies = [pool.submit(shutil.copyfile, os.path.join(src, "image_2", f), os.path.join(dst, "image_2", f))
              for f in sorted(os.listdir(os.path.join(src, "image_2")))]
    for f in ("calib.txt", "poses.txt", "times.txt"):
        if os.path.isfile(os.path.join(src, f)):
            copies.append(pool.submit(shutil.copyfile, os.path.join(src, f), os.path.join(dst, f)))

    def reads(start):
        return [pool.submit(_read_frame, ds.pointcloud_files[i], ds.label_files[i] if has_label else None, ds.image_files[i])
                for i in range(start, min(start + batch_frames, n))]
    n_read = n_kept = 0
    nxt, writes = reads(0), []
    for start in range(0, n, batch_frames):
        cur = [f.result() for f in nxt]
        nxt = reads(start + batch_frames)                   # the next batch is read while this one is filtered
        out = filter_fn([c[0] for c in cur], [c[2] for c in cur], proj, [c[1] for c in cur] if has_label else None)
        if len(out) != len(cur):
            raise RuntimeError("filter_fn answered %d frames for %d" % (len(out), len(cur)))
        for f in writes:                                    # at most one batch of writes in flight
            f.result()
        writes = []
        for j, (pts, lab, keep) in enumerate(out):
            if pts.shape[0] != int(np.count_nonzero(keep)) or (has_label and lab.shape[0] != pts.shape[0]):
                raise RuntimeError("filter_fn: frame %s keeps %d points but answers %d rows" %
                                   (ids[start + j], int(np.count_nonzero(keep)), pts.shape[0]))
            n_read += cur[j][0].shape[0]
            n_kept += pts.shape[0]
            writes.append(pool.submit(_write_frame, os.path.join(dst, "velodyne", ids[start + j] + ".bin"),
                                      os.path.join(dst, "labels", ids[start + j] + ".label") if has_label else None, pts, lab))
    for f in writes + copies:
        f.result()
    return {"frames": n, "points_read": n_read, "points_kept": n_kept, "seconds": time.time() - t0}
