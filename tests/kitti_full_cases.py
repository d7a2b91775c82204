"""Shared cases of the full-sweep SemanticKITTI tests and the numpy restatement of pmf_kitti_full_fill's rule
(include/pmf_amd_full.h), built on fov_cases: the keep mask is fov_cases.numpy_keep, the reference's float64 arithmetic."""
import numpy as np

import fov_cases as F

# annotation id -> class of the raw tests: 300 entries, seven classes; 0, 1 and 150 map to class 0, 300 and 5000 lie beyond
NLUT, NCLS = 300, 7
LUT = np.zeros(NLUT, np.int32)
LUT[[10, 40, 252, 257, 259, 299]] = [1, 2, 3, 4, 5, 6]
ID_POOL = np.array([0, 1, 10, 40, 150, 252, 257, 259, 299, 300, 5000], np.uint32)
FILL_ID = 40


def cls(ids, lut):
    """class of the low halves of `ids`: lut[id] inside the table, 0 at or beyond its end"""
    ids = (np.asarray(ids).astype(np.uint32) & 0xFFFF).astype(np.int64)
    lut = np.asarray(lut, np.int32)
    return np.where(ids < lut.shape[0], lut[np.minimum(ids, lut.shape[0] - 1)], 0).astype(np.int64)


def numpy_fill(frames, dims, proj, main, sub, lut, fill_id, nclasses, gt=None, keeps=None):
    """the rule, frame by frame -> dict(out=[u32[P_b]], keep=[bool[P_b]], source=[int[P_b]], kept_count i64[B],
    counts i64[3], conf i64[C, C] or None).  keeps: masks to use instead of numpy_keep (inputs on a border)."""
    B = len(frames)
    out, keep_l, src_l = [], [], []
    kept_count = np.zeros(B, np.int64)
    counts = np.zeros(3, np.int64)
    conf = np.zeros((nclasses, nclasses), np.int64) if gt is not None else None
    fill = np.uint32(int(fill_id) & 0xFFFF)
    for b, pts in enumerate(frames):
        keep = F.numpy_keep(pts, proj, dims[b][0], dims[b][1]) if keeps is None else np.asarray(keeps[b], bool)
        kept_count[b] = int(keep.sum())
        rank = np.cumsum(keep) - keep                               # kept rows of the frame in front of row i
        words = np.asarray(main[b]).astype(np.uint32) & 0xFFFF
        has = keep & (rank < words.shape[0])
        m = np.zeros(pts.shape[0], np.uint32)
        m[has] = words[rank[has]]
        s = np.asarray(sub[b]).astype(np.uint32) & 0xFFFF
        from_main = cls(m, lut) != 0
        from_sub = ~from_main & (cls(s, lut) != 0)
        pred = np.where(from_main, m, np.where(from_sub, s, fill)).astype(np.uint32)
        source = np.where(from_main, 0, np.where(from_sub, 1, 2))
        counts += np.bincount(source, minlength=3)
        if gt is not None:
            p, t = cls(pred, lut), cls(gt[b], lut)
            ok = (p >= 0) & (p < nclasses) & (t >= 0) & (t < nclasses)
            np.add.at(conf, (p[ok], t[ok]), 1)
        out.append(pred)
        keep_l.append(keep)
        src_l.append(source)
    return dict(out=out, keep=keep_l, source=src_l, kept_count=kept_count, counts=counts, conf=conf)


def words(rng, n):
    """n label words: a low half from ID_POOL, a random high half"""
    return (rng.choice(ID_POOL, n).astype(np.uint32) | (rng.integers(0, 2 ** 16, n).astype(np.uint32) << 16)).astype(np.uint32)


def random_case(sizes, seed, dims=(8, 8), short=None, extra=None):
    """frames of the given sizes under F.EXACT_PROJ, about half of the rows kept and all of them far from every border, with
    main (one word per kept row; frame `short` three words less, frame `extra` five more), sub and gt words"""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames, main, sub, gt = [], [], [], []
    for b, n in enumerate(sizes):
        x = rng.uniform(1.0, 2.0, n).astype(np.float32)
        pts = np.stack([x, x * rng.uniform(1, 7, n).astype(np.float32), x * rng.uniform(1, 7, n).astype(np.float32),
                        rng.random(n).astype(np.float32)], 1).astype(np.float32)
        behind = rng.random(n) < 0.5
        pts[behind, 0] = -pts[behind, 0]
        k = int(F.numpy_keep(pts, F.EXACT_PROJ, dims[0], dims[1]).sum())
        if b == short:
            k = max(k - 3, 0)
        if b == extra:
            k += 5
        frames.append(pts)
        main.append(words(rng, k))
        sub.append(words(rng, n))
        gt.append(words(rng, n))
    return frames, [tuple(dims)] * len(sizes), main, sub, gt


def is_rich(want):
    """all three sources occur, kept and unkept rows both occur"""
    src = np.concatenate(want["source"])
    keep = np.concatenate(want["keep"])
    return set(np.unique(src)) == {0, 1, 2} and bool(keep.any()) and not bool(keep.all())
