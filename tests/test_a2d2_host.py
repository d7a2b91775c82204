"""A2D2 loader, host side (no GPU): the fourth header's binding and guards, file discovery, the label lookup's key scheme,
and the numpy restatements of tests/a2d2_cases.py against exact arithmetic."""
import json
import os

import numpy as np
import pytest

import a2d2_cases as A


def test_fourth_header_binding():
    from pmf_amd import _lib
    import ctypes as C
    assert _lib.EXPORTS_A2D2 == ["pmf_undistort_map", "pmf_remap_u8c3", "pmf_a2d2_index"]
    assert (_lib.LENS_TELECAM, _lib.LENS_FISHEYE) == (0, 1)
    assert not set(_lib.EXPORTS_A2D2) & set(_lib.EXPORTS + _lib.EXPORTS_SENSAT + _lib.EXPORTS_WIDE)
    lib = _lib.lib()
    V, I, D = C.c_void_p, C.c_int32, C.c_double
    assert lib.pmf_undistort_map.argtypes == [I, V, D, D, D, D, V, I, I, V, V]
    assert lib.pmf_remap_u8c3.argtypes == [V, I, I, V, I, I, V, V]
    assert lib.pmf_a2d2_index.argtypes == [V, V, V, V, V, I, V, V, I, D, V, V, V, V, V, V, V, V]
    for name in _lib.EXPORTS_A2D2:
        assert getattr(lib, name).restype is C.c_int32
    import __graft_entry__ as g
    import inspect
    assert "EXPORTS_A2D2" in inspect.getsource(g.build)


def test_missing_symbol_names_the_header(monkeypatch):
    """a library without one of the header's functions is refused with the header's name"""
    from pmf_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXPORTS_A2D2", _lib.EXPORTS_A2D2 + ["pmf_a2d2_not_there"])
    with pytest.raises(_lib.PMFLibraryError, match=r"pmf_a2d2_not_there, which include/pmf_amd_a2d2\.h declares"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib() is not None


def test_entry_point_guards():
    """every guard answers before a launch: the pointers below are never dereferenced"""
    from pmf_amd import _lib
    lib = _lib.lib()
    p, E, U = 4096, _lib.PMF_E_ARG, _lib.PMF_E_UNSUPPORTED
    m = lib.pmf_undistort_map
    assert m(0, 0, 1.0, 1.0, 0.0, 0.0, p, 4, 4, p, None) == E            # null inverse matrix
    assert m(0, p, 1.0, 1.0, 0.0, 0.0, 0, 4, 4, p, None) == E            # null coefficients
    assert m(1, p, 1.0, 1.0, 0.0, 0.0, p, 4, 4, 0, None) == E            # null map
    assert m(0, p, 1.0, 1.0, 0.0, 0.0, p, 0, 4, p, None) == E
    assert m(0, p, 1.0, 1.0, 0.0, 0.0, p, 4, -1, p, None) == E
    assert m(2, p, 1.0, 1.0, 0.0, 0.0, p, 4, 4, p, None) == E            # unknown lens kind
    assert m(-1, p, 1.0, 1.0, 0.0, 0.0, p, 4, 4, p, None) == E
    assert m(0, p, 1.0, 1.0, 0.0, 0.0, p, 65536, 32768, p, None) == U    # h * w = 2^31
    r = lib.pmf_remap_u8c3
    assert r(0, 4, 4, p, 4, 4, p, None) == E and r(p, 4, 4, 0, 4, 4, p, None) == E and r(p, 4, 4, p, 4, 4, 0, None) == E
    assert r(p, 0, 4, p, 4, 4, p, None) == E and r(p, 4, 0, p, 4, 4, p, None) == E
    assert r(p, 4, 4, p, 0, 4, p, None) == E and r(p, 4, 4, p, 4, -3, p, None) == E
    assert r(p, 4, 4, p, 65536, 32768, p, None) == U and r(p, 65536, 32768, p, 4, 4, p, None) == U
    assert r(p, 4, 4, p + 8, 4, 4, p, None) == E                          # map off its 16 bytes
    assert r(p, 4, 4, p, 4, 4, p + 2, None) == E                          # dst off its dword
    ix = lib.pmf_a2d2_index

    def call(**kw):
        a = dict(points=p, refl=p, rows=p, cols=p, rgb=p, P=10, keys=p, cls=p, n=55, sc=1.0, pts=p, depth=p, xy=p, xd=p, yd=p,
                 sem=p, meta=p)
        a.update(kw)
        return ix(a["points"], a["refl"], a["rows"], a["cols"], a["rgb"], a["P"], a["keys"], a["cls"], a["n"], a["sc"],
                  a["pts"], a["depth"], a["xy"], a["xd"], a["yd"], a["sem"], a["meta"], None)
    for name in ("points", "refl", "rows", "cols", "pts", "depth", "xy", "xd", "yd", "sem", "meta"):
        assert call(**{name: 0}) == E, name
    assert call(P=0) == E and call(P=-5) == E
    for sc in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sc=sc) == E
    assert call(keys=0) == E and call(cls=0) == E and call(n=0) == E and call(n=65) == E
    assert call(pts=p + 4) == E                                           # pts off its 16 bytes


def test_file_discovery_and_names(tmp_path):
    from pmf_amd.dataset.a2d2 import A2D2_PV
    import pc_processor
    assert pc_processor.dataset.a2d2.A2D2_PV is A2D2_PV
    cams, cidx, _ = A.build_tree(str(tmp_path / "tree"))
    root = str(tmp_path / "tree")
    kw = dict(unused_index=[], zero_size_index=[], split_bounds=(4, 6))
    every = A2D2_PV(root, cams, cidx, split="all", **kw)
    assert len(every) == 8 and every.lidar_files == sorted(every.lidar_files)
    assert [len(A2D2_PV(root, cams, cidx, split=s, **kw)) for s in ("train", "valid", "test")] == [4, 2, 2]
    assert A2D2_PV(root, cams, cidx, split="valid", **kw).lidar_files == every.lidar_files[4:6]
    assert A2D2_PV(root, cams, cidx, split="test", **kw).lidar_files == every.lidar_files[6:]
    # the two deletions act one after the other, as np.delete twice
    cut = A2D2_PV(root, cams, cidx, split="all", unused_index=[1, 2], zero_size_index=[0], split_bounds=(4, 6))
    assert cut.lidar_files == [every.lidar_files[i] for i in (3, 4, 5, 6, 7)]
    f = every.lidar_files[0]
    assert f.endswith("/20180807_145028/lidar/cam_front_center/20180807145028_lidar_frontcenter_000000001.npz")
    assert every.camera_files[0] == f.replace("/lidar/", "/camera/").replace("_lidar_", "_camera_").replace(".npz", ".png")
    assert every.label_files[0] == f.replace("/lidar/", "/label/").replace("_lidar_", "_label_").replace(".npz", ".png")
    assert all(os.path.isfile(x) for x in every.camera_files + every.label_files)
    assert A2D2_PV.get_save_file_name(every.label_files[0]) == "20180807145028_pred_frontcenter_000000001.label"
    assert every._camera_key(0) == "front_center" and every._camera_key(7) == "side_left"
    assert every.parsePathInfoByIndex(3) == (3, '')
    assert every.mapped_class_name[38] == "rain_dirt" and len(every.mapped_class_name) == 39
    assert every.cls_freq.shape == (39,) and every.cls_freq[0] == 0 and abs(every.cls_freq.sum() - 1.0) < 1e-12
    lab = np.arange(5)
    assert every.labelMapping(lab) is lab
    with pytest.raises(ValueError, match="invalid split"):
        A2D2_PV(root, cams, cidx, split="val", **kw)
    with pytest.raises(ValueError, match="dataset not found"):
        A2D2_PV(root + "_nowhere", cams, cidx, **kw)
    with pytest.raises(ValueError, match="parameter error"):
        A2D2_PV.extract_file_name_from_lidar_file_name(every.lidar_files, "lidar")
    with pytest.raises(IndexError):           # the reference's fixed indices on a small tree: why the keywords exist
        A2D2_PV(root, cams, cidx, split="all")
    # the defaults are the reference's
    from pmf_amd.dataset.a2d2 import unused_index, zero_size_index
    assert len(unused_index) == 26 and unused_index[0] == 942 and unused_index[-1] == 27428
    assert zero_size_index == [12907, 12908, 12909, 12910, 12911, 12912, 13649, 13650, 13651, 13652]
    mapped, keep = every.mapLidar2Camera(0, None, 48, 80)
    d = np.load(every.lidar_files[0])
    assert np.array_equal(mapped[:, 0], (d["row"] + 0.5).astype(np.int32)) and mapped.dtype == np.int32
    assert np.array_equal(mapped[:, 1], (d["col"] + 0.5).astype(np.int32)) and keep.all() and keep.shape == (300,)
    pc = np.zeros((300, 4))
    got = every.mapLidar2CameraCropYaw(0, pc)
    assert got[0] is pc and np.array_equal(got[1], mapped) and got[2].all()


def test_lookup_keys_equal_the_per_point_loop():
    """the u32 key scheme names the same dictionary entries as the reference's hex strings, on every colour of
    class_index.json and on channel values below 16 (where hex() has one digit and the loop patches an 'x' into a '0')"""
    from pmf_amd.dataset.a2d2 import A2D2_PV, colour_table
    with open(A.CLASS_INDEX) as f:
        class_index = json.load(f)
    keys, cls = colour_table(class_index)
    assert keys.dtype == np.uint32 and cls.dtype == np.int32 and len(keys) == len(class_index) == 55 <= 64
    assert len(set(keys.tolist())) == len(keys)
    colours = np.stack(((keys >> 16) & 255, (keys >> 8) & 255, keys & 255), 1).astype(np.uint8)
    assert (colours < 16).any()                                   # e.g. '#b65906', '#000064'
    extra = np.array([[0, 0, 0], [1, 2, 3], [15, 16, 9], [10, 255, 0], [255, 255, 255]], np.uint8)
    table = dict(zip(keys.tolist(), cls.tolist()))
    img = np.concatenate((colours, extra))[None]                  # a 1 x n label image
    rows, cols = np.zeros(img.shape[1], np.int32), np.arange(img.shape[1], dtype=np.int32)
    for c in range(img.shape[1]):
        px = img[0, c]
        key = (int(px[0]) << 16) | (int(px[1]) << 8) | int(px[2])
        hexs = A.rgb_to_hex(px)
        assert hexs == A2D2_PV.rgb_to_hex(px) == "#%06x" % key
        if hexs in class_index:
            assert table[key] == class_index[hexs] == A.lookup_loop(class_index, img, rows[c:c + 1], cols[c:c + 1])[0]
        else:
            assert key not in table
            with pytest.raises(KeyError, match=hexs):
                A.lookup_loop(class_index, img, rows[c:c + 1], cols[c:c + 1])
    assert np.array_equal(A.lookup_loop(class_index, img, rows[:55], cols[:55]), cls)


def _neigh_bound(n):
    """|bilinear(u + du, v + dv) - bilinear(u, v)| for |du|, |dv| <= 1/64 inside one (closed) cell, from its four corners:
    d/du = (n01 - n00)(1 - fy) + (n11 - n10) fy is a mean of two differences, d/dv likewise, and the bilinear form's only
    second-order term is (n00 - n01 - n10 + n11) du dv"""
    gx = np.maximum(np.abs(n[1] - n[0]), np.abs(n[3] - n[2]))
    gy = np.maximum(np.abs(n[2] - n[0]), np.abs(n[3] - n[1]))
    cross = np.abs(n[0] - n[1] - n[2] + n[3])
    return (gx + gy) / 64.0 + cross / 4096.0


def test_fixed_point_remap_against_exact_bilinear():
    """the 5-bit scheme vs float64 bilinear sampling at the unquantised coordinates.  Per pixel and channel: the coordinates
    are quantised by at most 1/64 px per axis, which moves the exact value by at most _neigh_bound -- integers are multiples
    of the 1/32 quantum, so the quantised point may land on an edge of the exact point's cell, never beyond it, and the
    bilinear form is continuous there; the result is then rounded once, <= 0.5; the weights (32-a)(32-b)/1024 are exact."""
    rng = np.random.RandomState(3)
    src = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    worst = 0.0
    for lens, dist in (("Telecam", [-0.26, 0.05, 0.001, -0.002, 0.01]), ("Fisheye", [-0.04, 0.01, 0.002, -0.001])):
        newm = [[30.0, 0, 26.2], [0, 31.0, 18.1], [0, 0, 1]]
        orig = [[36.0, 0, 26.9], [0, 35.5, 18.6], [0, 0, 1]]
        m, t = A.undistort_map(lens, newm, orig, dist, 37, 53)
        got = A.remap_u8c3(src, m).astype(np.float64)
        u, v = t[..., 0] / 32.0, t[..., 1] / 32.0
        exact, n, _, _ = A.bilinear_exact(src, u, v)
        bound = _neigh_bound(n) + 0.5 + 1e-9
        err = np.abs(got - exact)
        assert (np.abs(m - t) <= 0.5).all()                     # <= 1/64 px per axis
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print("%s: worst err %.4f, worst err / bound %.4f" % (lens, err.max(), ratio))
        assert (err <= bound).all()
        # the quantised coordinates sampled exactly differ from the integer form by the final rounding only
        q, _, _, _ = A.bilinear_exact(src, m[..., 0] / 32.0, m[..., 1] / 32.0)
        assert np.abs(got - q).max() <= 0.5 + 1e-9
    assert 0.0 < worst <= 1.0


def test_map_restatement_sanity():
    rng = np.random.RandomState(4)
    src = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    K = np.array([[41.3, 0, 25.7], [0, 40.2, 18.9], [0, 0, 1]])
    # (the fisheye model with all-zero coefficients is the equidistant projection, not the identity: Telecam throughout)
    m, t = A.undistort_map("Telecam", K, K, [0, 0, 0, 0, 0], 37, 53)
    jj, ii = np.meshgrid(np.arange(53), np.arange(37))
    assert np.array_equal(m[..., 0], 32 * jj) and np.array_equal(m[..., 1], 32 * ii)
    assert not A.near_half(t).any()
    assert np.array_equal(A.remap_u8c3(src, m), src)                           # identity
    mf, _ = A.undistort_map("Fisheye", K, K, [0, 0, 0, 0], 37, 53)
    assert np.array_equal(mf[19, 26], m[19, 26]) and (np.abs(mf[0, 0]) > np.abs(m[0, 0])).all()   # atan(r) / r < 1 off-centre
    # integer shift (3, -2): destination (i, j) reads source (i - 2, j + 3), zero outside
    Ks = K.copy()
    Ks[0, 2] += 3
    Ks[1, 2] -= 2
    m, t = A.undistort_map("Telecam", K, Ks, [0] * 5, 37, 53)
    assert np.array_equal(m[..., 0], 32 * (jj + 3)) and np.array_equal(m[..., 1], 32 * (ii - 2))
    want = np.zeros_like(src)
    want[2:, :50] = src[:35, 3:]
    assert np.array_equal(A.remap_u8c3(src, m), want) and not A.near_half(t).any()
    # half-pixel shift along x: (a + b + 1) >> 1 of horizontal neighbours, the last column pairs with the zero border
    Kh = K.copy()
    Kh[0, 2] += 0.5
    m, t = A.undistort_map("Telecam", K, Kh, [0] * 5, 37, 53)
    assert np.array_equal(m[..., 0], 32 * jj + 16) and not A.near_half(t).any()
    s = src.astype(np.int64)
    right = np.concatenate((s[:, 1:], np.zeros((37, 1, 3), np.int64)), 1)
    assert np.array_equal(A.remap_u8c3(src, m), ((s + right + 1) >> 1).astype(np.uint8))
    # saturation and NaN of the fixed-point conversion
    assert A.fix32([2.5, 3.5, -2.5, 1e30, -1e30, float("nan"), float("inf")]).tolist() == \
        [2, 4, -2, A.I32_MAX, A.I32_MIN, A.I32_MIN, A.I32_MAX]
    far = np.array([[[A.I32_MAX, 0], [A.I32_MIN, A.I32_MIN]]], np.int32)
    assert not A.remap_u8c3(src, far).any()


def test_cameras_of_the_gpu_map_test_stay_under_the_exemption_cap():
    """the share of map entries within 1e-6 of a rounding tie, for the cameras tests/test_gpu_a2d2.py builds maps for"""
    for name, (lens, newm, orig, dist, h, w) in A.map_cameras().items():
        _, t = A.undistort_map(lens, newm, orig, dist, h, w)
        share = float(A.near_half(t).mean())
        print("%s: %.6f %% of the entries near a tie" % (name, 100 * share))
        assert share <= 1e-3
