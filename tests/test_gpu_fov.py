"""pmf_fov_filter / fov_filter_gpu / create_fov_dataset on the GPU against the numpy restatement of the reference's method
(fov_cases) and against the loader's own projection kernel (project_frame_gpu), bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fov_cases as F

pytestmark = pytest.mark.gpu

PAT_PTS, PAT_LAB, PAT_KEEP, PAT_OFF = 0x7FC0BEEF, 0xDEADBEEF, 0xAB, -7777
TAIL = 64                                   # entries behind the capacity of every output: never written either


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Call:
    """one raw pmf_fov_filter call on pattern-filled outputs; `over` replaces arguments by name (error cases)"""

    def __init__(self, frames, dims, proj, labels=None, over=None):
        from pmf_amd import _lib as L
        self.B = B = len(frames)
        self.sizes = [len(f) for f in frames]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.P = P = int(self.offsets[-1])
        cap = max(P, 1)
        self.pts = _dev(np.concatenate(frames).astype(np.float32).reshape(-1, 4).view(np.int32))
        self.lab = None if labels is None else _dev(np.concatenate(labels).astype(np.uint32).view(np.int32))
        self.off_d, self.dim_d = _dev(self.offsets), _dev(np.asarray(dims, np.int32).reshape(B, 2))
        self.mat = _dev(np.asarray(proj, np.float64).reshape(12))
        self.keep = torch.full((cap + TAIL,), PAT_KEEP, dtype=torch.uint8).cuda()
        self.out_pts = _dev(np.full((cap + TAIL, 4), PAT_PTS, np.uint32).view(np.int32))
        self.out_lab = _dev(np.full(cap + TAIL, PAT_LAB, np.uint32).view(np.int32))
        self.out_off = torch.full((B + 1 + TAIL,), PAT_OFF, dtype=torch.int64).cuda()
        self.blk = torch.zeros((cap + L.FOV_BLOCK - 1) // L.FOV_BLOCK + 1, dtype=torch.int32).cuda()
        a = dict(points=self.pts.data_ptr(), labels=None if self.lab is None else self.lab.data_ptr(),
                 offsets=self.off_d.data_ptr(), dims=self.dim_d.data_ptr(), B=B, P=P, proj=self.mat.data_ptr(),
                 keep=self.keep.data_ptr(), out_points=self.out_pts.data_ptr(), out_labels=self.out_lab.data_ptr(),
                 out_offsets=self.out_off.data_ptr(), blk=self.blk.data_ptr())
        a.update(over or {})
        torch.cuda.synchronize()
        self.rc = L.lib().pmf_fov_filter(a["points"], a["labels"], a["offsets"], a["dims"], a["B"], a["P"], a["proj"], a["keep"],
                                         a["out_points"], a["out_labels"], a["out_offsets"], a["blk"],
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def host(self):
        return dict(keep=self.keep.cpu().numpy(), pts=self.out_pts.cpu().numpy().view(np.uint32),
                    lab=self.out_lab.cpu().numpy().view(np.uint32), off=self.out_off.cpu().numpy())

    def untouched(self):
        h = self.host()
        return ((h["keep"] == PAT_KEEP).all() and (h["pts"] == PAT_PTS).all() and (h["lab"] == PAT_LAB).all()
                and (h["off"] == PAT_OFF).all())


def _check(frames, dims, proj, labels, what):
    """the raw call against the restatement: keep, out_offsets, rows and label words as bits, pattern behind out_offsets[B]"""
    c = Call(frames, dims, proj, labels)
    assert c.rc == 0, what
    want = F.numpy_filter(frames, dims, proj, labels)
    h = c.host()
    keep = np.concatenate([w[2] for w in want])
    rows = np.concatenate([w[0] for w in want]).reshape(-1, 4).view(np.uint32)
    off = np.concatenate([[0], np.cumsum([len(w[0]) for w in want])])
    K = int(off[-1])
    assert np.array_equal(h["keep"][:c.P], keep.astype(np.uint8)), what
    assert np.array_equal(h["off"][:c.B + 1], off), what
    assert np.array_equal(h["pts"][:K], rows), what
    assert (h["keep"][c.P:] == PAT_KEEP).all() and (h["off"][c.B + 1:] == PAT_OFF).all(), what
    assert (h["pts"][K:] == PAT_PTS).all(), what
    if labels is None:
        assert (h["lab"] == PAT_LAB).all(), what
    else:
        assert np.array_equal(h["lab"][:K], np.concatenate([w[1] for w in want])), what
        assert (h["lab"][K:] == PAT_LAB).all(), what
    return want, K


def test_exact_boundary_cases():
    rows = F.exact_rows()
    rng = np.random.Generator(np.random.PCG64(1))
    labels = [rng.integers(0, 2 ** 32, len(rows), dtype=np.uint64).astype(np.uint32) for _ in F.EXACT_DIMS]
    want, K = _check([rows] * 3, F.EXACT_DIMS, F.EXACT_PROJ, labels, "exact")
    keeps = np.stack([w[2] for w in want])
    u, v = rows[:, 1], rows[:, 2]
    x1 = rows[:, 0] == 1
    # the restatement itself decides the borders as the issue states them
    for b, (h, w) in enumerate(F.EXACT_DIMS):
        pw, ph = np.nextafter(np.float32(w), np.float32(0)), np.nextafter(np.float32(h), np.float32(0))
        assert not keeps[b][x1 & ((u == 0) | (u == w) | (v == 0) | (v == h))].any()         # 0 and -0.0, w, h: out
        assert keeps[b][x1 & (u == pw) & (v == 1)].all() and keeps[b][x1 & (v == ph) & (u == 1)].all()
        assert (x1 & (u == pw) & (v == 1)).sum() == 1 and (x1 & (v == ph) & (u == 1)).sum() == 1
        assert not keeps[b][~np.isfinite(rows[:, :3]).all(1)].any()
        assert not keeps[b][0] and keeps[b][1]                                              # x = 0.5 and its successor
        assert keeps[b][-1]                                                                 # NaN intensity does not matter
    assert (keeps.any(0) & ~keeps.all(0)).sum() >= 3                                        # kept under one frame, not another
    assert 0 < K < 3 * len(rows)


@pytest.mark.parametrize("mode", ["all", "none", "alt"])
def test_block_and_frame_seams(mode):
    frames, labels, dims = F.seam_frames(mode)
    assert [len(f) for f in frames] == F.SEAM_SIZES
    want, K = _check(frames, dims, F.EXACT_PROJ, labels, mode)
    total = sum(F.SEAM_SIZES)
    assert K == {"all": total, "none": 0, "alt": total // 2}[mode]


def test_max_frames_of_three_points():
    from pmf_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(2))
    B = L.FOV_MAX_FRAMES
    frames = [np.stack([np.ones(3), rng.uniform(0.5, 7.5, 3), rng.uniform(0.5, 7.5, 3), rng.random(3)], 1).astype(np.float32)
              for _ in range(B)]
    dims = [(1 + b % 8, 8 - b % 8) for b in range(B)]
    labels = [rng.integers(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32) for _ in range(B)]
    want, K = _check(frames, dims, F.EXACT_PROJ, labels, "64 frames")
    assert 0 < K < 3 * B


def test_null_labels_leave_out_labels_untouched():
    frames, labels, dims = F.seam_frames("alt")
    _check(frames, dims, F.EXACT_PROJ, None, "no labels")
    c = Call(frames, dims, F.EXACT_PROJ, None, dict(out_labels=None))            # no labels: out_labels may be NULL as well
    assert c.rc == 0 and np.array_equal(c.host()["off"][:6], Call(frames, dims, F.EXACT_PROJ, labels).host()["off"][:6])


def test_every_error_returns_without_a_launch():
    from pmf_amd import _lib as L
    frames, labels, dims = F.seam_frames("all")
    bad = [dict(points=None), dict(offsets=None), dict(dims=None), dict(proj=None), dict(keep=None), dict(out_points=None),
           dict(out_offsets=None), dict(blk=None), dict(out_labels=None), dict(B=0), dict(B=-3), dict(B=L.FOV_MAX_FRAMES + 1),
           dict(P=0), dict(P=-1)]
    for kw in bad:
        c = Call(frames, dims, F.EXACT_PROJ, labels, kw)
        assert c.rc == L.PMF_E_ARG and c.untouched(), kw
    own = Call(frames, dims, F.EXACT_PROJ, labels)          # its buffers, 4 and 8 bytes in: real memory, off the 16-byte grid
    for off in (4, 8):
        for name, t in (("points", own.pts), ("out_points", own.out_pts)):
            e = Call(frames, dims, F.EXACT_PROJ, labels, {name: t.data_ptr() + off})
            assert e.rc == L.PMF_E_ARG and e.untouched(), (name, off)
    for P in (2 ** 31, 2 ** 33):
        c = Call(frames, dims, F.EXACT_PROJ, labels, dict(P=P))
        assert c.rc == L.PMF_E_UNSUPPORTED and c.untouched(), P


# ---- the synthetic tree ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from oracle.cases import kitti_tree
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    root = str(tmp_path_factory.mktemp("fov") / "sequences")
    cfg, data = kitti_tree(root, **F.TREE)
    return dict(root=root, cfg=cfg, data=data, ds=SemanticKitti(root, [0, 8], cfg))


def test_tree_against_the_loaders_kernel(tree):
    from pmf_amd.dataset import project_frame_gpu
    from pmf_amd.dataset.semantic_kitti import fov_filter_gpu
    ds, h, w = tree["ds"], F.TREE["h"], F.TREE["w"]
    for seq in ("00", "08"):
        M = ds.proj_matrix[seq]
        keys = sorted(k for k in tree["data"] if k[0] == seq)
        frames = [tree["data"][k][0] for k in keys]
        labels = [tree["data"][k][1] for k in keys]
        for k, pts in zip(keys, frames):        # the case is valid: see tests/test_fov_host.py::test_tree_is_a_valid_case
            assert 0.5 <= F.numpy_keep(pts, M, h, w).mean() <= 0.85 and F.border_distance(pts, M, h, w) > 1e-6, k
        got = fov_filter_gpu(frames, [(h, w)] * len(frames), M, labels)
        bare = fov_filter_gpu(frames, [(h, w)] * len(frames), M)
        want = F.numpy_filter(frames, [(h, w)] * len(frames), M, labels)
        for k, pts, raw, g, g0, r in zip(keys, frames, labels, got, bare, want):
            img = tree["data"][k][2]
            keep = project_frame_gpu(pts, (raw & 0xFFFF).astype(np.int32), img, M, ds.class_map_lut)[4].cpu().numpy()
            assert g[2].dtype == np.bool_ and np.array_equal(g[2], keep), k          # the existing kernel is the yardstick
            assert np.array_equal(keep, r[2]), k
            assert g[0].dtype == np.float32 and g[0].tobytes() == pts[keep].tobytes(), k
            assert g[1].dtype == np.uint32 and np.array_equal(g[1], raw[keep]), k
            assert g0[1] is None and g0[0].tobytes() == g[0].tobytes() and np.array_equal(g0[2], keep), k


def test_filter_on_the_seam_frames_and_on_an_empty_batch():
    from pmf_amd.dataset.semantic_kitti import fov_filter_gpu
    frames, labels, dims = F.seam_frames("alt")
    got = fov_filter_gpu(frames, dims, F.EXACT_PROJ, labels)
    want = F.numpy_filter(frames, dims, F.EXACT_PROJ, labels)
    assert len(got) == len(frames)
    for g, r in zip(got, want):
        assert g[0].tobytes() == r[0].tobytes() and np.array_equal(g[1], r[1]) and np.array_equal(g[2], r[2])
    empty = fov_filter_gpu([frames[2]], [dims[2]], F.EXACT_PROJ, [labels[2]])          # a batch without a point: no launch
    assert empty[0][0].shape == (0, 4) and empty[0][1].shape == (0,) and empty[0][2].shape == (0,)


def test_end_to_end_tree_through_the_loader(tree, tmp_path):
    from pmf_amd.dataset import PerspectiveViewLoader
    from pmf_amd.dataset.semantic_kitti import SemanticKitti, create_fov_dataset
    dst = str(tmp_path / "sequences")
    stats = create_fov_dataset(tree["root"], dst, [0, 8], config_path=tree["cfg"], batch_frames=3)
    raw_ds, fov_ds = tree["ds"], SemanticKitti(dst, [0, 8], tree["cfg"])
    assert len(fov_ds) == len(raw_ds) == 2 * F.TREE["frames"]
    cfg = {"sensor": dict(h_pad=0, w_pad=0, proj_h=F.TREE["h"], proj_w=F.TREE["w"], proj_ht=F.TREE["h"], proj_wt=F.TREE["w"])}
    raw_ld = PerspectiveViewLoader(raw_ds, cfg, is_train=False, return_uproj=True)
    fov_ld = PerspectiveViewLoader(fov_ds, cfg, is_train=False, return_uproj=True)
    kept = {"00": 0, "08": 0}
    for i in range(len(raw_ds)):
        assert fov_ds.parsePathInfoByIndex(i) == raw_ds.parsePathInfoByIndex(i)
        a = raw_ld[i]
        keep = raw_ld.last_keep
        b = fov_ld[i]
        assert bool(fov_ld.last_keep.all()) and fov_ld.last_keep.shape[0] == int(keep.sum()) > 0, i
        for name, x, y in zip(("feature", "mask", "label", "x_data", "y_data"), a[:5], b[:5]):
            assert x.shape == y.shape and torch.equal(x, y), (i, name)
        assert torch.equal(b[5], a[5][keep]), i
        kept[raw_ds.parsePathInfoByIndex(i)[0]] += int(keep.sum())
    assert {s: stats[s]["points_kept"] for s in stats} == kept
    for seq in ("00", "08"):
        for f in os.listdir(os.path.join(dst, seq, "image_2")):
            with open(os.path.join(dst, seq, "image_2", f), "rb") as g, open(os.path.join(tree["root"], seq, "image_2", f), "rb") as s:
                assert g.read() == s.read()
