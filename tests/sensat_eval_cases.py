"""Shared pieces of the SensatUrban evaluation tests (TEST INFRASTRUCTURE, not a conftest): a synthetic SensatUrban tree
(.pth / .bin / .ply per block), probability maps by recipe, and torch-CPU / numpy statements of the per-frame composition of
the reference's tasks/sensat_urban/pmf_eval/infer.py:95-208.

What is pinned to a reference RUN: the tile enumeration and the zero-filled crops -- tests/golden/g19_sensat_tiles.npz holds
what the reference's own SensatUrban(use_crop=True) returned for two tiny frames (regenerate_g19 below; its loop is the same
loop as infer.py:95-118).  The reference's infer.py itself cannot run where this was written (torchvision, prettytable and
CUDA are missing), so everything else here -- normalise, the seven variants and their inverses, the sum order, accumulation,
argmax, gather or KNN, zero -> 1, confusion -- is a RESTATEMENT written from reading that file, in the same torch ops
(rot90, flip, permute, pad, centre crop) on the CPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NCLASSES = 14
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
MEAN = [27.47, 26.90, 27.22, 0.63, 0.81, 0, 0, 0]
STD = [18.43, 18.00, 18.21, 0.40, 0.39, 255.0, 255.0, 255.0]
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_sensat_tiles.npz")
# (name, h, w, points): the smallest shapes that can still go wrong -- 70 x 100 gives three shifted, overlapping rows and
# columns at S = 32 (two at 48) at unaligned w_start; 40 x 52 is smaller than a 48 tile in one dimension
FRAMES = (("birmingham_block_0", 70, 100, 9000), ("cambridge_block_9", 40, 52, 2500))
G19_SIZES = (32, 48)


def make_frame(seed, h, w, npts, quantise=False):
    """-> (frame dict as the dataset preparation writes it, uint8[P] point labels 0..12, xyz f32[P,3], rgb u8[P,3]).
    Several points share a pixel (npts > occupied pixels) and ~25 % of the pixels stay empty (mask 0, label -1).
    quantise: heights in steps of 1/4 (every value of the frame is then exact in float16: the fixture stores it so)."""
    rs = np.random.RandomState(seed)
    occupied = rs.rand(h, w) < 0.75
    occ = np.flatnonzero(occupied.reshape(-1))
    pix = np.concatenate([occ, occ[rs.randint(0, occ.size, max(npts - occ.size, 0))]])[:npts]
    rs.shuffle(pix)
    h_idx, w_idx = (pix // w).astype(np.int64), (pix % w).astype(np.int64)
    z = 5.0 + 45.0 * rs.rand(pix.size)
    if quantise:
        z = np.round(z * 4) / 4
    z = z.astype(np.float32)
    rgb = rs.randint(0, 256, (pix.size, 3)).astype(np.uint8)
    coarse = rs.randint(0, 13, (h // 8 + 1, w // 8 + 1))
    pix_label = np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:h, :w]
    labels = pix_label[h_idx, w_idx].astype(np.uint8)
    flip = rs.rand(pix.size) < 0.1
    labels[flip] = rs.randint(0, 13, int(flip.sum())).astype(np.uint8)
    fm = np.zeros((8, h, w), np.float64)
    zmax = np.full(h * w, -np.inf)
    zmin = np.full(h * w, np.inf)
    cnt = np.zeros(h * w)
    np.maximum.at(zmax, pix, z)
    np.minimum.at(zmin, pix, z)
    np.add.at(cnt, pix, 1)
    seen = cnt > 0
    fm[0].reshape(-1)[seen] = zmax[seen]
    fm[1].reshape(-1)[seen] = zmin[seen]
    fm[2].reshape(-1)[seen] = (zmax[seen] + zmin[seen]) / 2
    fm[3].reshape(-1)[seen] = np.minimum(cnt[seen], 8) / 8
    fm[4].reshape(-1)[seen] = 1.0
    for k in range(3):
        fm[5 + k].reshape(-1)[pix] = rgb[:, k]                 # the last point of a pixel wins
    label_map = np.full((h, w), -1, np.int64)
    label_map.reshape(-1)[pix] = labels
    xyz = np.stack([w_idx + rs.rand(pix.size), h_idx + rs.rand(pix.size), z], 1).astype(np.float32)
    return {"feature_map": fm, "label_map": label_map, "h_idx": h_idx, "w_idx": w_idx}, labels, xyz, rgb


def write_ply(path, xyz, rgb, cls=None):
    """binary little-endian PLY, the vertex layout of SensatUrban: x y z float, red green blue uchar[, class uchar]"""
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if cls is not None:
        fields.append(("class", "u1"))
    v = np.zeros(xyz.shape[0], dtype=fields)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if cls is not None:
        v["class"] = cls
    names = {"<f4": "float", "u1": "uchar"}
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % xyz.shape[0]
    head += "".join("property %s %s\n" % (names[t], n) for n, t in fields) + "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(v.tobytes())


def write_tree(root, split="val", frames=FRAMES, seed=0, quantise=False):
    """<root>/<split>/NAME.{pth,bin,ply} per block (+ a cambridge_block_1 the dataset must skip) -> {name: (frame, labels,
    xyz)}"""
    folder = os.path.join(root, split)
    os.makedirs(folder, exist_ok=True)
    out = {}
    todo = list(frames) + [("cambridge_block_1", 20, 24, 300)]
    for k, (name, h, w, npts) in enumerate(todo):
        frame, labels, xyz, rgb = make_frame(100 * seed + k, h, w, npts, quantise)
        torch.save(frame, os.path.join(folder, name + ".pth"))
        labels.tofile(os.path.join(folder, name + ".bin"))
        write_ply(os.path.join(folder, name + ".ply"), xyz, rgb, labels if split != "test" else None)
        out[name] = (frame, labels, xyz)
    return out


def prob_recipe(seed, n, S, C=NCLASSES):
    """f32[n,C,S,S]: blocks of 8 x 8 pixels share a dominant class (class 0 among them, so some points land on class 0) plus
    full-mantissa noise, so that the order of float additions shows in the last bit"""
    rs = np.random.RandomState(seed)
    coarse = rs.rand(n, C, S // 8 + 1, S // 8 + 1).astype(np.float32)
    p = np.repeat(np.repeat(coarse, 8, 2), 8, 3)[:, :, :S, :S] + np.float32(0.3) * rs.rand(n, C, S, S).astype(np.float32)
    return np.ascontiguousarray(p.astype(np.float32))


def windows_np(h, w, S):
    """the enumeration of infer.py:95-116, restated -> [(h_start, h_end, w_start, w_end)]"""
    out = []
    for r in range(-(-h // S)):
        hs, he = r * S, (r + 1) * S
        if he > h:
            he, hs = h, max(h - S, 0)
        for c in range(-(-w // S)):
            ws, we = c * S, (c + 1) * S
            if we > w:
                we, ws = w, max(w - S, 0)
            out.append((hs, he, ws, we))
    return out


def ref_tile_inputs(feature_map, win, S, mean=MEAN, std=STD, tta=False):
    """infer.py:117-147 for one tile -> ([pcd variants], [rgb variants]) as the reference feeds them to the model: the tile
    alone, or the tile + rot90 / rot180 / flip W / flip H / transpose + the 16-pixel zero pad (seven entries)"""
    hs, he, ws, we = win
    crop = np.zeros((8, S, S))
    crop[:, :he - hs, :we - ws] = feature_map[:, hs:he, ws:we]
    x = torch.from_numpy(crop).float().unsqueeze(0)
    m = torch.Tensor(mean).view(1, 8, 1, 1)
    s = torch.Tensor(std).view(1, 8, 1, 1)
    x = (x - m) / s * x[:, 4].unsqueeze(1)
    pcd, rgb = x[:, 0:5], x[:, 5:8]
    if not tta:
        return [pcd], [rgb]
    var = lambda t: [t, t.rot90(1, (2, 3)), t.rot90(2, (2, 3)), t.flip(3), t.flip(2), t.permute(0, 1, 3, 2),
                     torch.nn.functional.pad(t, (16, 16, 16, 16), mode="constant", value=0)]
    return var(pcd), var(rgb)


def ref_tile_sum(outs, S):
    """infer.py:158-170: the model outputs of one tile ([1,C,S,S] x 1, or x 6 + [1,C,S+32,S+32]) -> [C,S,S]"""
    if len(outs) == 1:
        return outs[0][0]
    p0, p1, p2, p3, p4, p5, p6 = outs
    return (p0 + p1.rot90(3, (2, 3)) + p2.rot90(2, (2, 3)) + p3.flip(3) + p4.flip(2) + p5.permute(0, 1, 3, 2)
            + p6[:, :, 16:16 + S, 16:16 + S])[0]


def ref_confidence_map(h, w, sizes, tile_outputs, C=NCLASSES):
    """infer.py:93-172: tile_outputs(S, k, win) -> the model outputs of tile k of size S (CPU tensors).  Only the part of a
    tile inside the frame is added (the reference raises on a frame smaller than the tile: the extension of the library)."""
    conf = torch.zeros((C, h, w)).float()
    for S in sizes:
        for k, win in enumerate(windows_np(h, w, S)):
            hs, he, ws, we = win
            conf[:, hs:he, ws:we] += ref_tile_sum(tile_outputs(S, k, win), S)[:, :he - hs, :we - ws]
    return conf


def np_conf(pred, gt, C=NCLASSES):
    pred, gt = np.asarray(pred, np.int64).reshape(-1), np.asarray(gt, np.int64).reshape(-1)
    return np.bincount(pred * C + gt, minlength=C * C).reshape(C, C)


def ref_finish(conf, frame, labels=None, z=None, knn_params=None, C=NCLASSES):
    """infer.py:174-215 -> dict(argmax int64[h,w], pixel_conf, pred uint8[P] (before the - 1), zero_num, point_conf)"""
    argmax = conf.unsqueeze(0).argmax(dim=1)[0]
    out = {"argmax": argmax.numpy(), "pixel_conf": np_conf(argmax.numpy(), np.asarray(frame["label_map"]) + 1, C)}
    h_idx, w_idx = frame["h_idx"], frame["w_idx"]
    if knn_params is not None:
        from oracle import knn_ref                      # numpy statement of knn.py: independent of the HIP vote
        pred = torch.from_numpy(knn_ref.knn_vote(
            torch.from_numpy(frame["feature_map"][0]).float().numpy(), np.asarray(z, np.float32), argmax.numpy(),
            w_idx, h_idx, nclasses=C, **knn_params)).long()
    else:
        pred = argmax[h_idx, w_idx]
    out["zero_num"] = int(pred.eq(0).sum())
    pred[pred.eq(0)] = 1
    out["pred"] = pred.numpy().astype(np.uint8)
    if labels is not None:
        out["point_conf"] = np_conf(out["pred"], labels + 1, C)
    return out


def regenerate_g19(reference_root, path=GOLDEN):
    """run the REFERENCE's SensatUrban(use_crop=True) on a synthetic tree of the two FRAMES (quantised: every value exact in
    float16) at img 32 and 48 and record the input frames and the crops it returns.  The reference calls torch.load without
    weights_only; newer torch refuses numpy arrays by default, so torch.load is wrapped for the duration of the call."""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location(
        "ref_sensat_urban", os.path.join(reference_root, "pc_processor", "dataset", "sensat_urban", "sensat_urban.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        tree = write_tree(tmp, "val", quantise=True)
        real_load = torch.load
        torch.load = lambda *a, **k: real_load(*a, **dict(k, weights_only=False))
        try:
            for S in G19_SIZES:
                ds = mod.SensatUrban(tmp, "val", keep_idx=False, img_h=S, img_w=S, use_crop=True)
                rec["order_%d" % S] = np.array([n.replace(".pth", "") for n in ds.data_split])
                rec["crop_feature_%d" % S] = np.stack([ds.readDataByIndex(i)["feature_map"] for i in range(len(ds))])
                rec["crop_label_%d" % S] = np.stack([ds.readDataByIndex(i)["label_map"] for i in range(len(ds))])
        finally:
            torch.load = real_load
    for name, _, _, _ in FRAMES:
        rec["%s.feature_map" % name] = tree[name][0]["feature_map"]
        rec["%s.label_map" % name] = tree[name][0]["label_map"]
    small = {}
    for k, v in rec.items():
        if v.dtype.kind == "f":
            assert np.array_equal(v.astype(np.float16).astype(v.dtype), v), k
            v = v.astype(np.float16)
        elif v.dtype.kind == "i":
            v = v.astype(np.int8)
        small[k] = v
    np.savez_compressed(path, **small)
    return path
