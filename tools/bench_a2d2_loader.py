#!/usr/bin/env python3
"""The A2D2 loader stage by stage on a synthetic full-size frame (1208 x 1920, both lenses of A2D2's own cams_lidars.json):
PNG decode (host), upload, map build (once per camera), remap, per-point pass + scatter, a whole validation item and a
whole training item -- next to the host composition written out in tests/a2d2_cases.py (numpy map + remap, the per-point
label loop, the numpy frame).  ``cv2`` is not installed here, so the undistortion baseline is that numpy restatement of
OpenCV's algorithm and NOT OpenCV itself, which would be far faster than numpy at this.
The remap is also set beside a float4 copy (torch's device copy) of the same number of bytes, and the time 6.3 TB/s would need.
Device stages: HIP events around `reps` back-to-back launches; stages with a host part: a host clock around work that ends
in a synchronise, median of `reps`.
usage: python tools/bench_a2d2_loader.py [--points 12000] [--reps 20] [--no-host-baseline]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import a2d2_cases as A  # noqa: E402
from pmf_amd import _lib as L  # noqa: E402

COPY_TBS = 6.3
H, W = 1208, 1920


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)                      # ms


def device_only(ds, i, img_dev, reps):
    """(pmf_a2d2_index, pmf_project_v2_scatter) in us, inputs already on the device"""
    from pmf_amd.dataset.perspective_view_loader import upload_packed
    d = np.load(ds.lidar_files[i])
    rows, cols = ds._pixel_index(d)
    rgb = np.ascontiguousarray(ds.loadSemImage(ds.label_files[i])[rows, cols][:, :3])
    P = len(rows)
    up = upload_packed([np.ascontiguousarray(d["points"], np.float64), np.ascontiguousarray(d["reflectance"], np.float64),
                        rows, cols, rgb, ds._keys.view(np.int32), ds._cls], "cuda")
    dev = img_dev.device
    pts = torch.empty((P, 4), dtype=torch.float32, device=dev)
    depth = torch.empty(P, dtype=torch.float32, device=dev)
    xy = torch.empty((P, 2), dtype=torch.float64, device=dev)
    xd, yd, sem = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    meta = torch.empty(6, dtype=torch.int32, device=dev)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    index = lambda: L.check(lib.pmf_a2d2_index(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3].data_ptr(),
                                               up[4].data_ptr(), P, up[5].data_ptr(), up[6].data_ptr(), int(up[5].shape[0]), 1.0,
                                               pts.data_ptr(), depth.data_ptr(), xy.data_ptr(), xd.data_ptr(), yd.data_ptr(),
                                               sem.data_ptr(), meta.data_ptr(), st()), "index")
    t_index = events(index, reps)
    x_min, x_max, y_min, y_max = [int(v) for v in meta.tolist()[:4]]
    h, w = x_max - x_min + 1, y_max - y_min + 1
    ident = torch.arange(P, dtype=torch.int32, device=dev)
    lut = torch.arange(64, dtype=torch.int32, device=dev)
    proj = torch.empty((10, h, w), dtype=torch.float32, device=dev)
    pix = torch.empty(h * w, dtype=torch.int32, device=dev)
    scatter = lambda: L.check(lib.pmf_project_v2_scatter(pts.data_ptr(), sem.data_ptr(), ident.data_ptr(), xd.data_ptr(),
                                                         yd.data_ptr(), depth.data_ptr(), P, img_dev.data_ptr(),
                                                         img_dev.shape[0], img_dev.shape[1], lut.data_ptr(), 64, x_min, y_min,
                                                         h, w, proj.data_ptr(), pix.data_ptr(), st()), "scatter")
    return t_index, events(scatter, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=12000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_a2d2_loader.py needs a GPU")
    from PIL import Image
    from pmf_amd.dataset import PerspectiveViewLoaderV2
    from pmf_amd.dataset.a2d2 import A2D2_PV, remap_gpu, undistort_map_gpu
    with open(A.CAMS_LIDARS) as f:
        cams = json.load(f)
    out = {"frame": [H, W], "points": a.points, "reps": a.reps, "cv2": "absent: host baseline is the numpy restatement"}
    print("frame %d x %d, %d points per frame, %d repetitions; cv2 is absent: the host baseline is the numpy restatement of "
          "tests/a2d2_cases.py, not OpenCV" % (H, W, a.points, a.reps))
    with tempfile.TemporaryDirectory() as tmp:
        A.build_tree(tmp, frames=1, npts=a.points, h=H, w=W, cams=cams, scenes=A.SCENES[:1], blocky=True)
        ds = A2D2_PV(tmp, A.CAMS_LIDARS, A.CLASS_INDEX, split="all", unused_index=[], zero_size_index=[])
        cfg = {"PVconfig": {"proj_h": 480, "proj_w": 1280, "proj_ht": 320, "proj_wt": 960, "img_jitter": [0.4, 0.4, 0.4]}}
        val = PerspectiveViewLoaderV2(ds, cfg, is_train=False)
        trn = PerspectiveViewLoaderV2(ds, cfg, is_train=True, img_aug=True)
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in range(len(ds)):
            key = ds._camera_key(i)
            cam = cams["cameras"][key]
            r = {"lens": cam["Lens"]}
            r["png_decode_ms"] = clock(lambda: np.array(Image.open(ds.camera_files[i])), a.reps)
            host = np.ascontiguousarray(np.array(Image.open(ds.camera_files[i]))[:, :, :3])
            r["upload_ms"] = clock(lambda: torch.from_numpy(host).cuda(), a.reps)
            src = torch.from_numpy(host).cuda()
            build = lambda: undistort_map_gpu(cam["Lens"], cam["CamMatrix"], cam["CamMatrixOriginal"], cam["Distortion"], H, W)
            r["map_build_us"] = events(build, a.reps)
            m = build()
            dst = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
            r["remap_us"] = events(lambda: L.check(L.lib().pmf_remap_u8c3(
                src.data_ptr(), H, W, m.data_ptr(), H, W, dst.data_ptr(), st()), "remap"), a.reps)
            assert torch.equal(dst, remap_gpu(src, m))
            nbytes = H * W * (8 + 3 + 3)               # map read, output written, every source byte read once
            x = torch.empty(nbytes // 2 // 16 * 4, dtype=torch.float32, device="cuda")
            y = torch.empty_like(x)
            r["remap_bytes"] = nbytes
            r["copy_same_bytes_us"] = events(lambda: y.copy_(x), a.reps)
            r["floor_us_at_6.3TBps"] = nbytes / (COPY_TBS * 1e6)
            img_dev = ds.loadImageDevice(i)
            r["index_us"], r["scatter_us"] = device_only(ds, i, img_dev, a.reps)
            # npz read, label PNG decode, host gather, packed upload, pmf_a2d2_index, meta read, pmf_project_v2_scatter
            r["project_device_ms"] = clock(lambda: ds.projectDevice(i, img_dev, 1.0), a.reps)
            r["label_png_decode_ms"] = clock(lambda: ds.loadSemImage(ds.label_files[i]), a.reps)
            r["validation_item_ms"] = clock(lambda: val[i], a.reps)
            r["training_item_ms"] = clock(lambda: trn[i], a.reps)
            if not a.no_host_baseline:
                d = np.load(ds.lidar_files[i])
                rows, cols = ds._pixel_index(d)
                sem_image = ds.loadSemImage(ds.label_files[i])
                t0 = time.perf_counter()
                und = A.undistorted_ref(cams, key, host)
                r["host_undistort_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                sem = A.lookup_loop(ds.class_index, sem_image, rows, cols)
                r["host_label_loop_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                pc = np.concatenate((d["points"], d["reflectance"][:, None]), 1)
                rp = A.frame_ref(pc, sem, rows, cols, und)[0]
                A.center_crop_ref(A.pad_ref(rp, 480, 1280), 480, 1280)
                r["host_frame_ms"] = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(img_dev.cpu().numpy(), und)
            out[key] = r
            print(key, json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}))
    print(json.dumps({"metric": "A2D2 loader stages, 1208 x 1920", **out}))


if __name__ == "__main__":
    main()
