#!/usr/bin/env python3
"""The nuScenes projection chain at nuScenes size (34 720 points per sweep, 900 x 1600 frames), per view and per sweep of
six views: the device path (one upload of the raw sweep, then per view pmf_nus_project, the meta read and
pmf_project_v2_scatter) next to the numpy composition of the reference's method (dataset_nuscenes_v2.py:301-375: per view
the sweep file is read again, four rotate / translate steps on the float32 [4, N] cloud, the pinhole, the masks), followed by
the host loader's upload + scatter (PerspectiveViewLoaderV2._nus_item) as it ran before.  nuscenes-devkit is not used: the
host baseline is its arithmetic written in numpy.
Device stages: HIP events around `reps` back-to-back calls; stages with a host part: a host clock around work that ends in a
synchronise, median of `reps`.
usage: python tools/bench_nus_loader.py [--points 34720] [--reps 20]"""
import argparse
import ctypes as C
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

import nus_tables_cases as N  # noqa: E402
from pmf_amd import _lib as L  # noqa: E402
from pmf_amd.dataset.nuScenes.tables import nus_project_gpu  # noqa: E402
from pmf_amd.dataset.perspective_view_loader import upload_packed  # noqa: E402

H, W = 900, 1600


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


def host_view(path, chain, fov, scales, min_dist=0.1):
    """mapLidar2CameraCropYaw as the reference runs it, numpy in the devkit's place"""
    c = chain
    pc = np.fromfile(path, dtype=np.float32).reshape((-1, 5))[:, :4].T.copy()          # LidarPointCloud.from_file
    for r, t, rot_first in ((c[0:9], c[9:12], True), (c[12:21], c[21:24], True), (c[27:36], c[24:27], False),
                            (c[39:48], c[36:39], False)):
        for step in ((0, 1) if rot_first else (1, 0)):
            if step == 0:
                pc[:3, :] = np.dot(r.reshape(3, 3), pc[:3, :])
            else:
                for i in range(3):
                    pc[i, :] = pc[i, :] + t[i]
    keep = pc[2, :] > min_dist
    yaw = -np.arctan2(pc[2, :], pc[0, :])
    keep = np.logical_and(keep, (yaw >= fov[0]) * (yaw <= fov[1]))
    crop = pc[:, keep]
    pts = np.dot(c[48:57].reshape(3, 3), crop[:3, :])
    pts = pts / pts[2:3, :]
    mapped = np.fliplr(pts.transpose(1, 0)[:, :2]).copy()
    mapped[:, 0] *= scales[0]
    mapped[:, 1] *= scales[1]
    return crop.transpose(1, 0), mapped, keep


def scatter(crop, sem_kept, ident, o, img, lut):
    h, w = o["x_max"] - o["x_min"] + 1, o["y_max"] - o["y_min"] + 1
    proj = torch.empty((10, h, w), dtype=torch.float32, device="cuda")
    pix = torch.empty(h * w, dtype=torch.int32, device="cuda")
    L.check(L.lib().pmf_project_v2_scatter(crop.data_ptr(), sem_kept.data_ptr(), ident.data_ptr(), o["x_data"].data_ptr(),
                                           o["y_data"].data_ptr(), o["depth"].data_ptr(), o["K"], img.data_ptr(), img.shape[0],
                                           img.shape[1], lut.data_ptr(), 256, o["x_min"], o["y_min"], h, w, proj.data_ptr(),
                                           pix.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "scatter")
    return proj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=34720)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    chains = []
    for cam in range(6):
        c = N.make_chain(rng, cam)
        c[48:54] *= 10.0                                  # the test tree's intrinsics are a tenth of the real ones
        chains.append(c)
    pts = N.make_points(rng, a.points)
    sem = rng.integers(0, 32, a.points).astype(np.int32)
    lut = torch.from_numpy(np.resize(np.array(N.CLASS_OF_INDEX, np.int32), 256)).cuda()
    frames = [torch.from_numpy(rng.integers(0, 256, ((H, W, 3) if cam == 3 else (H // 2, int(W * 0.6), 3))).astype(np.uint8))
              .cuda() for cam in range(6)]
    scales = [(1.0, 1.0) if cam == 3 else (0.5, 0.6) for cam in range(6)]
    fovs = [N.fov_bounds(ch) for ch in N.CHANNELS]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sweep.pcd.bin")
        pts.tofile(path)

        def upload():
            raw = np.fromfile(path, dtype=np.float32).reshape((-1, 5))
            return upload_packed([raw, sem], "cuda")

        dpts, dsem = upload()
        ident = torch.arange(a.points, dtype=torch.int32, device="cuda")

        def project(cam):
            return nus_project_gpu(dpts, chains[cam], 1, 0.1, fovs[cam][0], fovs[cam][1], 0.0, 0.0, scales[cam][0],
                                   scales[cam][1], 1.0)

        def device_view(cam):
            o = project(cam)
            return scatter(o["crop"], dsem[o["src"].long()], ident, o, frames[cam], lut)

        def device_sweep():
            nonlocal dpts, dsem
            dpts, dsem = upload()
            for cam in range(6):
                device_view(cam)

        def host_loader_view(cam):
            crop, mapped, keep = host_view(path, chains[cam], fovs[cam], scales[cam])
            xd, yd = mapped[:, 0].astype(np.int32), mapped[:, 1].astype(np.int32)
            depth = np.linalg.norm(crop[:, :3], 2, axis=1).astype(np.float32)
            up = upload_packed([np.ascontiguousarray(crop, np.float32), sem[keep], xd, yd, depth], "cuda")
            o = dict(x_data=up[2], y_data=up[3], depth=up[4], K=len(xd), x_min=int(xd.min()), x_max=int(xd.max()),
                     y_min=int(yd.min()), y_max=int(yd.max()))
            return scatter(up[0], up[1], ident, o, frames[cam], lut)

        print("points per sweep: %d, frames %d x %d (CAM_BACK) and %d x %d" % (a.points, H, W, H // 2, int(W * 0.6)))
        kept = [project(cam)["K"] for cam in range(6)]
        print("kept per view:", kept)
        n = a.points
        keep = torch.empty(n, dtype=torch.uint8, device="cuda")
        i32 = torch.empty((3, n), dtype=torch.int32, device="cuda")
        crop = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        xy = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        depth = torch.empty(n, dtype=torch.float32, device="cuda")
        meta = torch.zeros(5, dtype=torch.int32, device="cuda")
        blk = torch.empty(n // L.NUS_BLOCK + 2, dtype=torch.int32, device="cuda")

        def launches(cam):             # the three launches alone: no allocation, no meta read
            L.check(L.lib().pmf_nus_project(dpts.data_ptr(), n, 5, chains[cam].ctypes.data, 1, 0.1, fovs[cam][0], fovs[cam][1],
                                            0.0, 0.0, scales[cam][0], scales[cam][1], 1.0, keep.data_ptr(), i32[0].data_ptr(),
                                            crop.data_ptr(), xy.data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(),
                                            depth.data_ptr(), meta.data_ptr(), blk.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pmf_nus_project")
        print("%-58s %10s" % ("stage", "time"))
        for cam in (0, 3):
            print("%-58s %8.1f us" % ("view %d: pmf_nus_project, three launches (HIP events)" % cam,
                                      events(lambda: launches(cam), a.reps)))
            print("%-58s %8.3f ms" % ("view %d: pmf_nus_project + allocation + meta read" % cam,
                                      clock(lambda: project(cam), a.reps)))
            print("%-58s %8.3f ms" % ("view %d: device path, project + scatter" % cam, clock(lambda: device_view(cam), a.reps)))
            print("%-58s %8.3f ms" % ("view %d: numpy chain alone (file read included)" % cam,
                                      clock(lambda: host_view(path, chains[cam], fovs[cam], scales[cam]), a.reps)))
            print("%-58s %8.3f ms" % ("view %d: numpy chain + upload + scatter" % cam,
                                      clock(lambda: host_loader_view(cam), a.reps)))
        print("%-58s %8.3f ms" % ("sweep: read + one upload", clock(upload, a.reps)))
        print("%-58s %8.3f ms" % ("sweep: device path, upload + six views", clock(device_sweep, a.reps)))
        print("%-58s %8.3f ms" % ("sweep: numpy chain + upload + scatter, six views",
                                  clock(lambda: [host_loader_view(cam) for cam in range(6)], a.reps)))


if __name__ == "__main__":
    main()
