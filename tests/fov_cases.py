"""Shared cases of the SemanticKITTI-FOV tests and the numpy restatement of the reference's method
(pc_processor/dataset/semantic_kitti/parser.py mapLidar2Camera + tasks/process_semantickitti_fov/create_fov_dataset.py):
keep = x > 0.5, float64 proj @ [x y z 1], u = a / c, v = b / c, 0 < u < w, 0 < v < h; then boolean indexing."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# u = y / x, v = z / x: exact at x = 1
EXACT_PROJ = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], np.float64)
EXACT_DIMS = [(4, 8), (8, 4), (6, 6)]               # (h, w) of the three frames that hold the same rows
SEAM_SIZES = [1, 1023, 0, 1025, 2049]               # an empty frame in the middle, frames straddling workgroups, one point
TREE = dict(seed=3, seqs=(0, 8), frames=5, npts=3000, h=24, w=80)


def uv(points, proj):
    """float64 (u, v) of every row (whatever its x), the reference's arithmetic"""
    hom = np.concatenate([points[:, :3].astype(np.float64), np.ones((points.shape[0], 1))], 1)
    with np.errstate(all="ignore"):
        m = (np.asarray(proj, np.float64).reshape(3, 4) @ hom.T).T
        return m[:, 0] / m[:, 2], m[:, 1] / m[:, 2]


def numpy_keep(points, proj, h, w):
    u, v = uv(points, proj)
    with np.errstate(invalid="ignore"):
        return (points[:, 0] > np.float32(0.5)) & (u > 0) & (u < w) & (v > 0) & (v < h)


def numpy_filter(frames, dims, proj_matrix, labels=None, device=None):
    """the signature of fov_filter_gpu: -> [(points[keep], labels[keep] or None, keep)]"""
    out = []
    for b, pts in enumerate(frames):
        keep = numpy_keep(pts, proj_matrix, dims[b][0], dims[b][1])
        out.append((pts[keep], None if labels is None else labels[b][keep], keep))
    return out


def border_distance(points, proj, h, w):
    """smallest distance (pixels) of a projected coordinate of a point in front of the vehicle from an image border"""
    u, v = uv(points, proj)
    front = points[:, 0] > np.float32(0.5)
    d = np.minimum.reduce([np.abs(u), np.abs(u - w), np.abs(v), np.abs(v - h)])
    return float(d[front].min())


def exact_rows():
    """rows on and next to every border of the keep rule under EXACT_PROJ, for every (h, w) of EXACT_DIMS; the fourth column is
    a distinct payload (one of them a NaN with a payload: rows are copied as bits)"""
    f = np.float32
    up, down = (lambda a: np.nextafter(f(a), f(np.inf))), (lambda a: np.nextafter(f(a), f(-np.inf)))
    rows = [(0.5, 0.25, 0.25), (up(0.5), 0.5, 0.5)]                      # x = 0.5 is out, its successor is in (u, v just below 1)
    for lim in sorted({d for hw in EXACT_DIMS for d in hw}):
        for edge in (0.0, lim, down(lim), -0.0):
            rows.append((1.0, edge, 1.0))                                 # u on / next to the border, v inside every frame
            rows.append((1.0, 1.0, edge))                                 # the same for v
    rows += [(np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.nan), (np.inf, 1.0, 1.0), (-np.inf, 1.0, 1.0)]
    rows += [(1.0, 5.0, 1.0), (1.0, 1.0, 5.0), (2.0, 10.0, 2.0)]          # kept under one frame's dims, dropped under another's
    pts = np.zeros((len(rows) + 1, 4), np.float32)
    pts[:-1, :3] = np.array(rows, np.float32)
    pts[-1] = (1.0, 1.0, 1.0, 0.0)                                        # NaN in the fourth coordinate: kept, bits intact
    pts[:, 3] = np.arange(len(pts), dtype=np.float32) / 64
    w = pts.view(np.uint32)
    w[-1, 3] = 0x7FC0BEEF
    w[-2, 3] = 0xFFC12345
    return pts


def seam_frames(mode, seed=5):
    """SEAM_SIZES frames under EXACT_PROJ and dims (8, 8): 'all' / 'none' / 'alt' rows kept, far from every border"""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames, labels, n0 = [], [], 0
    for n in SEAM_SIZES:
        idx = np.arange(n0, n0 + n)
        x = rng.uniform(1.0, 2.0, n).astype(np.float32)
        pts = np.stack([x, x * rng.uniform(1, 7, n).astype(np.float32), x * rng.uniform(1, 7, n).astype(np.float32),
                        rng.random(n).astype(np.float32)], 1).astype(np.float32)
        out = {"all": np.zeros(n, bool), "none": np.ones(n, bool), "alt": idx % 2 == 1}[mode]
        pts[out, 0] = -pts[out, 0]
        frames.append(pts)
        labels.append((rng.integers(0, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32))
        n0 += n
    return frames, labels, [(8, 8)] * len(SEAM_SIZES)
