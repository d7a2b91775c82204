"""SemanticKITTI-FOV, host side (no GPU): the sixth header's binding and argument guards, and create_fov_dataset driven by the
numpy restatement of the reference's method (fov_cases.numpy_filter) on the synthetic tree of oracle.cases.kitti_tree."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import fov_cases as F


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_sixth_header_binding():
    from pmf_amd import _lib
    assert _lib.EXPORTS_FOV == ["pmf_fov_filter"]
    assert (_lib.FOV_BLOCK, _lib.FOV_MAX_FRAMES) == (1024, 64)
    assert os.path.samefile(_lib.FOV_HEADER_PATH, os.path.join(F.ROOT, "include", "pmf_amd_fov.h"))
    assert not set(_lib.EXPORTS_FOV) & set(_lib.EXPORTS + _lib.EXPORTS_SENSAT + _lib.EXPORTS_WIDE + _lib.EXPORTS_A2D2
                                           + _lib.EXPORTS_NUS)
    lib = _lib.lib()
    V, I, Q = C.c_void_p, C.c_int32, C.c_int64
    assert lib.pmf_fov_filter.argtypes == [V, V, V, V, I, Q, V, V, V, V, V, V, V]
    assert lib.pmf_fov_filter.restype is C.c_int32


def test_build_checks_the_sixth_list(monkeypatch):
    import __graft_entry__ as g
    from pmf_amd import _lib
    assert _lib.lib() is not None
    monkeypatch.setattr(g.subprocess, "run", lambda *a, **kw: None)
    g.build()
    monkeypatch.setattr(_lib, "EXPORTS_FOV", _lib.EXPORTS_FOV + ["pmf_fov_not_there"])
    with pytest.raises(RuntimeError, match="pmf_fov_not_there"):
        g.build()


def test_missing_symbol_names_the_header(monkeypatch):
    from pmf_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXPORTS_FOV", _lib.EXPORTS_FOV + ["pmf_fov_not_there"])
    with pytest.raises(_lib.PMFLibraryError, match=r"pmf_fov_not_there, which include/pmf_amd_fov\.h declares"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib() is not None


def test_every_argument_guard_answers_before_a_launch():
    """the guards look at the pointers' values only: plausible numbers stand in for device memory"""
    from pmf_amd import _lib
    p = 4096
    names = ("points", "labels", "offsets", "dims", "B", "P", "proj", "keep", "out_points", "out_labels", "out_offsets", "blk")

    def call(**kw):
        a = dict(points=p, labels=p, offsets=p, dims=p, B=2, P=100, proj=p, keep=p, out_points=p, out_labels=p,
                 out_offsets=p, blk=p)
        a.update(kw)
        return _lib.lib().pmf_fov_filter(*[a[n] for n in names], None)
    E = _lib.PMF_E_ARG
    for name in ("points", "offsets", "dims", "proj", "keep", "out_points", "out_offsets", "blk"):
        assert call(**{name: None}) == E, name
    assert call(out_labels=None) == E                       # labels without a place for them
    for B in (0, -1, _lib.FOV_MAX_FRAMES + 1):
        assert call(B=B) == E
    for P in (0, -1):
        assert call(P=P) == E
    for off in (4, 8, 12, 1):
        assert call(points=p + off) == E and call(out_points=p + off) == E
    assert call(P=2 ** 31) == _lib.PMF_E_UNSUPPORTED and call(P=2 ** 40) == _lib.PMF_E_UNSUPPORTED
    assert call(P=2 ** 31, points=None) == E


def test_filter_checks_its_batch_on_the_host():
    """shape errors are found before the device is asked for: they raise ValueError with or without a GPU"""
    from pmf_amd.dataset.semantic_kitti import fov_filter_gpu
    pts = np.zeros((5, 4), np.float32)
    with pytest.raises(ValueError, match="frame 1 has 5 points but 4 labels"):
        fov_filter_gpu([pts, pts], [(4, 4)] * 2, F.EXACT_PROJ, [np.zeros(5, np.uint32), np.zeros(4, np.uint32)])
    with pytest.raises(ValueError, match="frame 0 must be a float32 array"):
        fov_filter_gpu([pts.astype(np.float64)], [(4, 4)], F.EXACT_PROJ)
    with pytest.raises(ValueError, match="image sizes"):
        fov_filter_gpu([pts, pts], [(4, 4)], F.EXACT_PROJ)
    with pytest.raises(ValueError, match="3 x 4"):
        fov_filter_gpu([pts], [(4, 4)], np.eye(4))
    from pmf_amd import _lib
    n = _lib.FOV_MAX_FRAMES + 1
    with pytest.raises(ValueError, match="65 frames, a batch holds 1 to 64"):
        fov_filter_gpu([pts] * n, [(4, 4)] * n, F.EXACT_PROJ)
    with pytest.raises(ValueError, match="0 frames"):
        fov_filter_gpu([], [], F.EXACT_PROJ)


def test_filter_has_no_host_path():
    import torch
    from pmf_amd.dataset.semantic_kitti import fov_filter_gpu
    with pytest.raises(RuntimeError, match="GPU only"):
        fov_filter_gpu([np.ones((5, 4), np.float32)], [(4, 4)], F.EXACT_PROJ, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            fov_filter_gpu([np.ones((5, 4), np.float32)], [(4, 4)], F.EXACT_PROJ)


def test_shim_names():
    import pc_processor
    from pmf_amd.dataset.semantic_kitti import fov
    assert pc_processor.dataset.semantic_kitti.fov_filter_gpu is fov.fov_filter_gpu
    assert pc_processor.dataset.semantic_kitti.create_fov_dataset is fov.create_fov_dataset
    import pc_processor.dataset.semantic_kitti.fov as shim
    assert shim is fov


# ---- create_fov_dataset with the numpy filter ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """kitti_tree + what it does not have: label words with the top bit set, a frame that keeps no point, poses.txt in one
    sequence only and times.txt in the other"""
    from oracle.cases import kitti_tree
    root = str(tmp_path_factory.mktemp("fov") / "sequences")
    cfg, data = kitti_tree(root, **F.TREE)
    lab = os.path.join(root, "00", "labels", "000001.label")
    words = np.fromfile(lab, np.uint32)
    words[::3] |= np.uint32(0x80000000)
    words[1::7] = np.uint32(0xFFFFFFFF)
    words.tofile(lab)
    pts = np.fromfile(os.path.join(root, "08", "velodyne", "000002.bin"), np.float32).reshape(-1, 4)
    pts[:, 0] = -np.abs(pts[:, 0])
    pts.tofile(os.path.join(root, "08", "velodyne", "000002.bin"))
    with open(os.path.join(root, "00", "poses.txt"), "w") as f:
        f.write("1 0 0 0 0 1 0 0 0 0 1 0\n" * F.TREE["frames"])
    with open(os.path.join(root, "08", "times.txt"), "w") as f:
        f.write("0.0\n0.1\n")
    return dict(root=root, cfg=cfg)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _snapshot(root):
    return {os.path.relpath(os.path.join(d, f), root): _bytes(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs}


@pytest.fixture(scope="module")
def built(tree, tmp_path_factory):
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    dst = str(tmp_path_factory.mktemp("fov_out") / "sequences")
    stats = create_fov_dataset(tree["root"], dst, [8, 0], config_path=tree["cfg"], batch_frames=3, io_threads=2,
                               filter_fn=F.numpy_filter)
    return dict(dst=dst, stats=stats)


def test_tree_layout_and_contents(tree, built):
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    src, dst = tree["root"], built["dst"]
    assert sorted(os.listdir(dst)) == ["00", "08"]
    assert sorted(os.listdir(os.path.join(dst, "00"))) == ["calib.txt", "image_2", "labels", "poses.txt", "velodyne"]
    assert sorted(os.listdir(os.path.join(dst, "08"))) == ["calib.txt", "image_2", "labels", "times.txt", "velodyne"]
    ds = SemanticKitti(src, [0, 8], tree["cfg"])
    top_bit = empty = 0
    for seq in ("00", "08"):
        frames = ["%06d" % i for i in range(F.TREE["frames"])]
        assert sorted(os.listdir(os.path.join(dst, seq, "velodyne"))) == [f + ".bin" for f in frames]
        assert sorted(os.listdir(os.path.join(dst, seq, "labels"))) == [f + ".label" for f in frames]
        assert sorted(os.listdir(os.path.join(dst, seq, "image_2"))) == [f + ".png" for f in frames]
        for name in ["calib.txt"] + [os.path.join("image_2", f + ".png") for f in frames]:
            assert _bytes(os.path.join(dst, seq, name)) == _bytes(os.path.join(src, seq, name)), (seq, name)
        n_read = n_kept = 0
        for f in frames:
            pts = np.fromfile(os.path.join(src, seq, "velodyne", f + ".bin"), np.float32).reshape(-1, 4)
            words = np.fromfile(os.path.join(src, seq, "labels", f + ".label"), np.uint32)
            keep = F.numpy_keep(pts, ds.proj_matrix[seq], F.TREE["h"], F.TREE["w"])
            assert _bytes(os.path.join(dst, seq, "velodyne", f + ".bin")) == pts[keep].tobytes(), (seq, f)
            assert _bytes(os.path.join(dst, seq, "labels", f + ".label")) == words[keep].tobytes(), (seq, f)
            # the reference's own label arithmetic on int32 gives the same words
            i32 = words.view(np.int32)
            assert np.array_equal((((i32 >> 16)[keep].astype(np.int32) << 16) + (i32 & 0xFFFF)[keep].astype(np.int32)),
                                  words[keep].view(np.int32))
            top_bit += int((words[keep] >> 31).sum())
            empty += int(keep.sum() == 0)
            n_read, n_kept = n_read + len(pts), n_kept + int(keep.sum())
        st = built["stats"][seq]
        assert (st["frames"], st["points_read"], st["points_kept"]) == (F.TREE["frames"], n_read, n_kept)
    assert top_bit > 100 and empty == 1                     # the cases are in the tree: not vacuous
    assert os.path.getsize(os.path.join(dst, "08", "velodyne", "000002.bin")) == 0
    assert os.path.getsize(os.path.join(dst, "08", "labels", "000002.label")) == 0
    # the written tree opens as a data set of its own, files line up one to one
    out = SemanticKitti(dst, [0, 8], tree["cfg"])
    assert len(out) == 2 * F.TREE["frames"]
    for i in range(len(out)):
        p, sem, inst = out.loadDataByIndex(i)
        assert p.shape[0] == sem.shape[0] == inst.shape[0]


@pytest.mark.parametrize("batch_frames,io_threads", [(1, 1), (4, 3), (64, 100)])
def test_result_does_not_depend_on_batch_or_threads(tree, built, tmp_path, batch_frames, io_threads):
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    dst = str(tmp_path / "sequences")
    calls = []

    def counting(frames, dims, proj, labels=None):
        calls.append(len(frames))
        assert all(d == (F.TREE["h"], F.TREE["w"]) for d in dims)
        return F.numpy_filter(frames, dims, proj, labels)
    stats = create_fov_dataset(tree["root"], dst, [0, 8], config_path=tree["cfg"], batch_frames=batch_frames,
                               io_threads=io_threads, filter_fn=counting)
    assert _snapshot(dst) == _snapshot(built["dst"])
    n = F.TREE["frames"]
    per_seq = [min(batch_frames, n - s) for s in range(0, n, batch_frames)]
    assert calls == per_seq * 2                           # batches never span sequences, the last one is short
    for seq in stats:
        assert {k: v for k, v in stats[seq].items() if k != "seconds"} == \
            {k: v for k, v in built["stats"][seq].items() if k != "seconds"}


def test_without_labels(tree, tmp_path):
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    dst = str(tmp_path / "sequences")
    seen = []

    def flt(frames, dims, proj, labels=None):
        seen.append(labels)
        return F.numpy_filter(frames, dims, proj, labels)
    create_fov_dataset(tree["root"], dst, [8], config_path=tree["cfg"], has_label=False, filter_fn=flt)
    assert seen == [None]
    assert sorted(os.listdir(os.path.join(dst, "08"))) == ["calib.txt", "image_2", "times.txt", "velodyne"]
    assert len(os.listdir(os.path.join(dst, "08", "velodyne"))) == F.TREE["frames"]


def test_existing_destination(tree, built, tmp_path):
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    dst = str(tmp_path / "sequences")
    os.makedirs(os.path.join(dst, "08", "velodyne"))
    with open(os.path.join(dst, "08", "velodyne", "000099.bin"), "wb") as f:
        f.write(b"stale")
    before = _snapshot(dst)
    with pytest.raises(FileExistsError, match="08"):
        create_fov_dataset(tree["root"], dst, [0, 8], config_path=tree["cfg"], filter_fn=F.numpy_filter)
    assert _snapshot(dst) == before and os.listdir(dst) == ["08"]           # nothing was written, sequence 00 included
    create_fov_dataset(tree["root"], dst, [0, 8], config_path=tree["cfg"], overwrite=True, filter_fn=F.numpy_filter)
    assert _snapshot(dst) == _snapshot(built["dst"])
    with pytest.raises(ValueError, match="same directory"):
        create_fov_dataset(tree["root"], tree["root"], [0], config_path=tree["cfg"], overwrite=True, filter_fn=F.numpy_filter)


def test_label_count_mismatch_and_missing_calib(tree, tmp_path):
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    src = str(tmp_path / "src")
    shutil.copytree(os.path.join(tree["root"], "00"), os.path.join(src, "00"))
    lab = os.path.join(src, "00", "labels", "000003.label")
    np.fromfile(lab, np.uint32)[:-1].tofile(lab)
    with pytest.raises(ValueError, match=r"000003\.label holds 3020 labels.*000003\.bin holds 3021 points"):
        create_fov_dataset(src, str(tmp_path / "dst"), [0], config_path=tree["cfg"], filter_fn=F.numpy_filter)
    os.remove(os.path.join(src, "00", "calib.txt"))
    with pytest.raises(FileNotFoundError, match="calib.txt"):
        create_fov_dataset(src, str(tmp_path / "dst2"), [0], config_path=tree["cfg"], filter_fn=F.numpy_filter)
    assert not os.path.exists(str(tmp_path / "dst2"))


def test_tree_is_a_valid_case(tree):
    """what tests/test_gpu_fov.py relies on: every frame of the untouched tree keeps 50 .. 85 % and no projected coordinate is
    within 1e-6 px of a border, so that float64 summation order cannot move a point across it"""
    from oracle.cases import kitti_tree
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cfg, data = kitti_tree(d, **F.TREE)
        ds = SemanticKitti(d, [0, 8], cfg)
        for (seq, frame), (pts, raw, img) in data.items():
            share = F.numpy_keep(pts, ds.proj_matrix[seq], F.TREE["h"], F.TREE["w"]).mean()
            assert 0.5 <= share <= 0.85, (seq, frame, share)
            assert F.border_distance(pts, ds.proj_matrix[seq], F.TREE["h"], F.TREE["w"]) > 1e-6
