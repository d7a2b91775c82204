"""Shared pieces of the devkit-free nuScenes reader's tests (TEST INFRASTRUCTURE, not a conftest): a writer of a small
nuScenes tree (JSON tables, sweeps, lidarseg files, images) and the numpy restatement of pmf_nus_project as
include/pmf_amd_nus.h specifies it: element-wise float64 products in the stated order, astype(float32) after every step."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from a2d2_cases import center_crop_ref, pad_ref  # noqa: E402,F401  (the loader's tail is the same for every data set)

CHANNELS = ("CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_BACK_RIGHT", "CAM_BACK", "CAM_BACK_LEFT", "CAM_FRONT_LEFT")
# yaw of each camera's optical axis in the ego frame (degrees): with the reader's windows (+-35, 40, 45, 50, 45, 40 degrees)
# neighbours overlap, and a gap of about 5 degrees stays open on either side of the front camera
CAM_YAW = (0.0, -80.0, -150.0, 180.0, 150.0, 80.0)
FOV = {"CAM_FRONT": (-35, 35), "CAM_FRONT_RIGHT": (-40, 40), "CAM_BACK_RIGHT": (-45, 45), "CAM_BACK": (-50, 50),
       "CAM_BACK_LEFT": (-45, 45), "CAM_FRONT_LEFT": (-40, 40)}
H, W = 90, 160                      # a tenth of the 900 x 1600 frames, the intrinsics scaled with them
MINI_NAMES = ("scene-0061", "scene-0103")         # one of v1.0-mini's training scenes and one of its validation scenes
# the 32 classes of nuScenes-lidarseg in index order
CATEGORIES = (
    'noise', 'animal', 'human.pedestrian.adult', 'human.pedestrian.child', 'human.pedestrian.construction_worker',
    'human.pedestrian.personal_mobility', 'human.pedestrian.police_officer', 'human.pedestrian.stroller',
    'human.pedestrian.wheelchair', 'movable_object.barrier', 'movable_object.debris', 'movable_object.pushable_pullable',
    'movable_object.trafficcone', 'static_object.bicycle_rack', 'vehicle.bicycle', 'vehicle.bus.bendy', 'vehicle.bus.rigid',
    'vehicle.car', 'vehicle.construction', 'vehicle.emergency.ambulance', 'vehicle.emergency.police', 'vehicle.motorcycle',
    'vehicle.trailer', 'vehicle.truck', 'flat.driveable_surface', 'flat.other', 'flat.sidewalk', 'flat.terrain',
    'static.manmade', 'static.other', 'static.vegetation', 'vehicle.ego')
# what the reference's two dictionaries make of them (dataset_nuscenes.py:20-72)
CLASS_OF_INDEX = (0, 0, 7, 7, 7, 0, 7, 0, 0, 1, 0, 0, 8, 0, 2, 3, 3, 4, 5, 0, 0, 6, 9, 10, 11, 12, 13, 14, 15, 0, 16, 0)

YAW_EPS, DIST_EPS, PIX_EPS = 1e-4, 1e-4, 1e-6


# ---- quaternions of the tree (w, x, y, z) -------------------------------------------------------------------------------
def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


def qaxis(axis, deg):
    h = math.radians(deg) / 2.0
    v = [0.0, 0.0, 0.0]
    v[axis] = math.sin(h)
    return (math.cos(h), v[0], v[1], v[2])


Q_CAM = (0.5, -0.5, 0.5, -0.5)      # camera axes (x right, y down, z forward) -> ego axes (x forward, y left, z up)


def camera_rotation(yaw_deg, rng):
    """camera -> ego: the optical axis at ``yaw_deg`` in the ego frame, a degree or so of mounting error"""
    q = qmul(qaxis(2, yaw_deg), Q_CAM)
    for axis in range(3):
        q = qmul(q, qaxis(axis, float(rng.uniform(-1.5, 1.5))))
    return [float(v) for v in q]


def make_chain(rng, cam=0):
    """57 doubles of a plausible (lidar, camera) pair, laid out as include/pmf_amd_nus.h says"""
    from pmf_amd.dataset.nuScenes import quaternion_rotation_matrix as R
    cal = _calibration(rng)
    pose_l = _pose(rng)
    return chain_of(cal["LIDAR_TOP"], pose_l, _camera_pose(pose_l, cam), cal[CHANNELS[cam]], R)


def chain_of(cs_l, pose_l, pose_c, cs_c, R):
    t = lambda rec: np.asarray(rec["translation"], np.float64)
    parts = [R(*cs_l["rotation"]), t(cs_l), R(*pose_l["rotation"]), t(pose_l), -t(pose_c), R(*pose_c["rotation"]).T,
             -t(cs_c), R(*cs_c["rotation"]).T, np.asarray(cs_c["camera_intrinsic"], np.float64)]
    return np.concatenate([np.ravel(p) for p in parts])


def _calibration(rng):
    cal = {"LIDAR_TOP": dict(rotation=[float(v) for v in qmul(qaxis(2, -90.0 + float(rng.uniform(-1, 1))),
                                                                qaxis(0, float(rng.uniform(-1, 1))))],
                             translation=[0.94 + float(rng.uniform(-.05, .05)), float(rng.uniform(-.05, .05)), 1.84],
                             camera_intrinsic=[])}
    for ch, yaw in zip(CHANNELS, CAM_YAW):
        f = 126.6 + float(rng.uniform(-3, 3))
        a = math.radians(yaw)
        cal[ch] = dict(rotation=camera_rotation(yaw, rng),
                       translation=[1.0 + 0.6 * math.cos(a) + float(rng.uniform(-.05, .05)),
                                    0.5 * math.sin(a) + float(rng.uniform(-.05, .05)), 1.5 + float(rng.uniform(-.05, .05))],
                       camera_intrinsic=[[f, 0.0, 81.6 + float(rng.uniform(-2, 2))],
                                         [0.0, f, 49.1 + float(rng.uniform(-2, 2))], [0.0, 0.0, 1.0]])
    return cal


def _pose(rng):
    """an ego pose far from the map's origin: float32 rounding of the global coordinates matters there"""
    q = qmul(qaxis(2, float(rng.uniform(-180, 180))), qmul(qaxis(1, float(rng.uniform(-1, 1))), qaxis(0, float(rng.uniform(-1, 1)))))
    return dict(rotation=[float(v) for v in q],
                translation=[411.3 + float(rng.uniform(-50, 50)), 1180.9 + float(rng.uniform(-50, 50)),
                             float(rng.uniform(-.1, .1))])


def _camera_pose(pose_l, j):
    """the ego pose at camera j's time: a third of a metre on and slightly turned, so lidar and camera time differ"""
    a = 0.3 + 0.03 * j
    return dict(rotation=[float(v) for v in qmul(tuple(pose_l["rotation"]), qaxis(2, 0.5 + 0.1 * j))],
                translation=[pose_l["translation"][0] + a, pose_l["translation"][1] - 0.5 * a,
                             pose_l["translation"][2] + 0.01])


def make_points(rng, n, cols=5):
    """sweep rows f32[n, cols]: 3..40 m around the lidar, all azimuths, -2..3 m high, intensity 0..255, ring index"""
    r, az = rng.uniform(3.0, 40.0, n), rng.uniform(-math.pi, math.pi, n)
    rows = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 3.0, n), rng.integers(0, 256, n).astype(np.float64),
                     rng.integers(0, 32, n).astype(np.float64)], 1).astype(np.float32)
    return np.ascontiguousarray(rows[:, :cols])


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _rot(R, p):
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) for i in range(3)], 1).astype(np.float32)


def _tr(t, p):
    return (p.astype(np.float64) + t[None, :]).astype(np.float32)


def camera_frame(points, chain):
    """f32[P, 3]: the chain of the header, a float32 point after every step"""
    c = np.asarray(chain, np.float64)
    p = np.ascontiguousarray(points[:, :3], np.float32)
    p = _tr(c[9:12], _rot(c[0:9].reshape(3, 3), p))
    p = _tr(c[21:24], _rot(c[12:21].reshape(3, 3), p))
    p = _rot(c[27:36].reshape(3, 3), _tr(c[24:27], p))
    p = _rot(c[39:48].reshape(3, 3), _tr(c[36:39], p))
    return p


def pinhole(cam, chain):
    """(u, v) float64 of the float32 camera-frame points"""
    K = np.asarray(chain, np.float64)[48:57].reshape(3, 3)
    x, y, z = (cam[:, k].astype(np.float64) for k in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b, c = ((K[i, 0] * x + K[i, 1] * y) + K[i, 2] * z for i in range(3))
        return a / c, b / c


def _norm32(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.sqrt((x * x + y * y) + z * z)          # float32 throughout


def restate(points, chain, mode, min_dist, fov_lo=0.0, fov_hi=0.0, bound_h=0.0, bound_w=0.0, row_scale=1.0, col_scale=1.0,
            img_scale=1.0):
    """numpy for pmf_nus_project -> dict(keep bool[P], src i32[K], crop f32[K,4], xy f64[K,2], x_data, y_data i32[K], depth
    f32[K], meta [K, row_min, row_max, col_min, col_max] or [0] when nothing is kept)"""
    points = np.asarray(points, np.float32)
    cam = camera_frame(points, chain)
    u, v = pinhole(cam, chain)
    front = cam[:, 2] > np.float32(min_dist)
    if mode == 1:
        yaw = -np.arctan2(cam[:, 2], cam[:, 0])
        assert yaw.dtype == np.float32
        yaw = yaw.astype(np.float64)
        keep = front & (yaw >= float(np.float32(fov_lo))) & (yaw <= float(np.float32(fov_hi)))
        depth = _norm32(cam)
    else:
        with np.errstate(invalid="ignore"):
            keep = front & (u > 1) & (u < bound_h - 1) & (v > 1) & (v < bound_w - 1)
        depth = _norm32(points)
    xy = np.stack([(v * np.float64(row_scale)) * np.float64(img_scale), (u * np.float64(col_scale)) * np.float64(img_scale)],
                  1)[keep]
    x_data, y_data = xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32)
    K = int(keep.sum())
    meta = [K, int(x_data.min()), int(x_data.max()), int(y_data.min()), int(y_data.max())] if K else [0]
    return dict(keep=keep, src=np.flatnonzero(keep).astype(np.int32),
                crop=np.concatenate([cam, points[:, 3:4]], 1)[keep].astype(np.float32), xy=xy, x_data=x_data, y_data=y_data,
                depth=depth[keep].astype(np.float32), meta=meta)


def fov_bounds(channel):
    """(fov_lo, fov_hi) of dataset_nuscenes_v2.py:305-306,353-355, float64"""
    fov_delta = 90.0 / 180.0 * np.pi
    return FOV[channel][0] / 180.0 * np.pi - fov_delta, FOV[channel][1] / 180.0 * np.pi - fov_delta


def too_close(points, chain, mode, min_dist, fov_lo=0.0, fov_hi=0.0, bound_h=0.0, bound_w=0.0):
    """bool[P]: the points whose keep bit could depend on the last bit of atan2f, or that sit on a threshold: within
    YAW_EPS rad of a yaw bound, DIST_EPS of min_dist, PIX_EPS px of a mode-0 pixel bound"""
    cam = camera_frame(np.asarray(points, np.float32), chain)
    bad = np.abs(cam[:, 2].astype(np.float64) - float(np.float32(min_dist))) < DIST_EPS
    if mode == 1:
        yaw = (-np.arctan2(cam[:, 2], cam[:, 0])).astype(np.float64)
        for b in (fov_lo, fov_hi):
            bad |= np.abs(yaw - float(np.float32(b))) < YAW_EPS
    else:
        u, v = pinhole(cam, chain)
        with np.errstate(invalid="ignore"):
            for val, b in ((u, 1.0), (u, bound_h - 1.0), (v, 1.0), (v, bound_w - 1.0)):
                bad |= np.abs(val - b) < PIX_EPS
    return bad


def frame_ref(crop, labels_kept, xy, image_u8):
    """perspective_view_loader_v2.py:72-140 on what mapLidar2CameraCropYaw hands over -> (proj f32[10, h, w], depth f32[K]);
    ``labels_kept``: the mapped labels of the kept points, ``image_u8``: the (jittered / resized) frame"""
    image = np.asarray(image_u8).astype(np.float32) / 255.0
    x_data, y_data = xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32)
    x_min, x_max, y_min, y_max = x_data.min(), x_data.max(), y_data.min(), y_data.max()
    h, w = x_max - x_min + 1, y_max - y_min + 1
    depth = np.linalg.norm(crop[:, :3], 2, axis=1).astype(np.float32)
    xyzi = np.zeros((h, w, 4), np.float32)
    xyzi[x_data - x_min, y_data - y_min] = crop[:, :4]
    pdepth = np.zeros((h, w), np.float32)
    pdepth[x_data - x_min, y_data - y_min] = depth
    plabel = np.zeros((h, w), np.int32)
    plabel[x_data - x_min, y_data - y_min] = labels_kept
    pmask = np.zeros((h, w), np.int32)
    pmask[x_data - x_min, y_data - y_min] = 1
    rgb = np.zeros((h, w, 3), np.float32)
    rr, cc = np.arange(h)[:, None] + x_min, np.arange(w)[None, :] + y_min
    ok = (rr >= 0) & (rr < image.shape[0]) & (cc >= 0) & (cc < image.shape[1])
    rgb[ok] = image[np.broadcast_to(rr, ok.shape)[ok], np.broadcast_to(cc, ok.shape)[ok]]
    proj = np.concatenate([pdepth[None], xyzi.transpose(2, 0, 1), rgb.transpose(2, 0, 1), pmask[None].astype(np.float32),
                           plabel[None].astype(np.float32)], 0)
    return proj.astype(np.float32), depth


# ---- the tree -------------------------------------------------------------------------------------------------------
def write_tree(root, version="v1.0-mini", scene_names=MINI_NAMES, samples=2, npts=3000, seed=0, labels=True,
               category_index=True):
    """A nuScenes tree under ``root``: len(scene_names) scenes x ``samples`` key frames, LIDAR_TOP + six cameras, one
    calibration per scene and sensor, one ego pose per key frame record (the cameras' a third of a metre further along
    than the sweep's), sweeps of about ``npts`` rows x 5 floats (rows the restatement finds too close to a threshold of any of the six
    views, in either mode, are left out), uint8 lidarseg files, H x W PNG frames.  One extra camera record per
    sample is NOT a key frame.  Returns {lidar token: dict(points, labels, chains={channel: 57 doubles})}."""
    from PIL import Image
    from pmf_amd.dataset.nuScenes import quaternion_rotation_matrix as R
    rng = np.random.default_rng(seed)
    tabs = {k: [] for k in ("scene", "sample", "sample_data", "calibrated_sensor", "ego_pose", "sensor", "category",
                            "lidarseg")}
    for i, name in enumerate(CATEGORIES):
        c = dict(token="cat%02d" % i, name=name, description="")
        if category_index:
            c["index"] = i
        tabs["category"].append(c)
    for ch in ("LIDAR_TOP",) + CHANNELS:
        tabs["sensor"].append(dict(token="sensor_" + ch, channel=ch, modality="lidar" if ch == "LIDAR_TOP" else "camera"))
    truth = {}
    for s, name in enumerate(scene_names):
        cal = _calibration(rng)
        for ch, rec in cal.items():
            tabs["calibrated_sensor"].append(dict(token="cs_%d_%s" % (s, ch), sensor_token="sensor_" + ch, **rec))
        toks = ["sample_%d_%d" % (s, k) for k in range(samples)]
        tabs["scene"].append(dict(token="scene_%d" % s, name=name, description="scene %d of the test tree" % s,
                                  nbr_samples=samples, first_sample_token=toks[0], last_sample_token=toks[-1]))
        for k, tok in enumerate(toks):
            tabs["sample"].append(dict(token=tok, scene_token="scene_%d" % s, timestamp=1000 * (s * samples + k),
                                       prev=toks[k - 1] if k else "", next=toks[k + 1] if k + 1 < samples else ""))
            pose_l = _pose(rng)
            lidar_tok = "sd_%d_%d_LIDAR_TOP" % (s, k)
            tabs["ego_pose"].append(dict(token="pose_" + lidar_tok, timestamp=0, **pose_l))
            fname = "samples/LIDAR_TOP/s%d_k%d.pcd.bin" % (s, k)
            tabs["sample_data"].append(dict(token=lidar_tok, sample_token=tok, ego_pose_token="pose_" + lidar_tok,
                                            calibrated_sensor_token="cs_%d_LIDAR_TOP" % s, filename=fname,
                                            fileformat="pcd", is_key_frame=True, height=0, width=0))
            chains = {}
            for j, ch in enumerate(CHANNELS):
                pose = _camera_pose(pose_l, j)
                cam_tok = "sd_%d_%d_%s" % (s, k, ch)
                tabs["ego_pose"].append(dict(token="pose_" + cam_tok, timestamp=0, **pose))
                img_name = "samples/%s/s%d_k%d.png" % (ch, s, k)
                tabs["sample_data"].append(dict(token=cam_tok, sample_token=tok, ego_pose_token="pose_" + cam_tok,
                                                calibrated_sensor_token="cs_%d_%s" % (s, ch), filename=img_name,
                                                fileformat="png", is_key_frame=True, height=H, width=W))
                # an intermediate frame of the same camera: in the table, not in the reverse index
                tabs["sample_data"].append(dict(token=cam_tok + "_sweep", sample_token=tok, ego_pose_token="pose_" + cam_tok,
                                                calibrated_sensor_token="cs_%d_%s" % (s, ch),
                                                filename="sweeps/%s/s%d_k%d.png" % (ch, s, k), fileformat="png",
                                                is_key_frame=False, height=H, width=W))
                os.makedirs(os.path.dirname(os.path.join(root, img_name)), exist_ok=True)
                Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(root, img_name))
                chains[ch] = chain_of(cal["LIDAR_TOP"], pose_l, pose, cal[ch], R)
            pts = make_points(rng, npts)
            n = npts // 20
            pts[n:2 * n, :3] = pts[2 * n:3 * n, :3]         # equal pixels, other intensity: the scatter's order decides
            bad = np.zeros(len(pts), bool)
            for ch in CHANNELS:
                lo, hi = fov_bounds(ch)
                bad |= too_close(pts, chains[ch], 1, 0.1, lo, hi)
                bad |= too_close(pts, chains[ch], 0, 1.0, bound_h=float(W), bound_w=float(H))
            pts = np.ascontiguousarray(pts[~bad])
            lab = rng.integers(0, 32, len(pts)).astype(np.uint8)
            os.makedirs(os.path.dirname(os.path.join(root, fname)), exist_ok=True)
            pts.tofile(os.path.join(root, fname))
            if labels:
                seg = "lidarseg/%s/%s_lidarseg.bin" % (version, lidar_tok)
                os.makedirs(os.path.dirname(os.path.join(root, seg)), exist_ok=True)
                lab.tofile(os.path.join(root, seg))
                tabs["lidarseg"].append(dict(token=lidar_tok, sample_data_token=lidar_tok, filename=seg))
            truth[lidar_tok] = dict(points=pts, labels=lab, chains=chains)
    os.makedirs(os.path.join(root, version), exist_ok=True)
    for k, rows in tabs.items():
        if k == "lidarseg" and not labels:
            continue
        with open(os.path.join(root, version, k + ".json"), "w") as f:
            json.dump(rows, f)
    return truth
