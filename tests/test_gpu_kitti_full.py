"""pmf_kitti_full_fill / fov_fill / the two SemanticKITTI full-sweep tasks on the GPU against the numpy restatement of the rule
(kitti_full_cases) and against pmf_fov_filter's keep mask.  Everything compared is integer data: bit equality throughout."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import fov_cases as F
import kitti_full_cases as K

pytestmark = pytest.mark.gpu

PAT_OUT, PAT_KEEP, PAT_KEPT, PAT_ACC = 0xDEADBEEF, 0xAB, -7777, 1000
PAT_MAIN = 0x0BAD0000 | 299                # in front of the main words: a word of class 6 that no case may pick up
TAIL = 64                                   # entries behind every output: never written
SALSA_TASK = os.path.join(F.ROOT, "tasks", "salsanext_eval_semantickitti")
FULL_TASK = os.path.join(F.ROOT, "tasks", "pmf_eval_semantickitti", "fullsweep_eval")
PMF_TASK = os.path.join(F.ROOT, "tasks", "pmf_eval_semantickitti")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return np.ascontiguousarray(a, np.uint32).view(np.int32)


class Call:
    """one raw pmf_kitti_full_fill call on pattern-filled outputs.  Every input sits in a tensor of exactly its size, the
    main words at the very end of one whose size is a whole number of the allocator's 512-byte granules; `over`
    replaces arguments by name (NULL optionals, error cases), `acc` = (conf, counts) tensors of an earlier call to add to."""

    def __init__(self, frames, dims, proj, main, sub, gt, lut=K.LUT, fill=K.FILL_ID, ncls=K.NCLS, over=None, acc=None,
                 main_off=None):
        from pmf_amd import _lib as L
        self.B = B = len(frames)
        self.offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
        self.P = P = int(self.offsets[-1])
        self.ncls = ncls
        cap = max(P, 1)
        self.moff = np.concatenate([[0], np.cumsum([len(m) for m in main])]).astype(np.int64) if main_off is None \
            else np.asarray(main_off, np.int64)
        Kt = int(sum(len(m) for m in main))
        self.pts = _dev(np.concatenate(frames).astype(np.float32).reshape(-1, 4))
        # the main words end where their allocation ends: a tensor of whole 512-byte granules, poison in front of the words
        self.main_buf = self.main = None
        if Kt:
            n = (Kt + 127) // 128 * 128
            self.main_buf = _dev(_i32(np.concatenate([np.full(n - Kt, PAT_MAIN, np.uint32), np.concatenate(main)])))
            self.main = self.main_buf[n - Kt:]
        self.sub = _dev(_i32(np.concatenate(sub)))
        self.gt = _dev(_i32(np.concatenate(gt))) if gt is not None else None
        self.off_d, self.moff_d = _dev(self.offsets), _dev(self.moff)
        self.dim_d = _dev(np.asarray(dims, np.int32).reshape(B, 2))
        self.mat, self.lut = _dev(np.asarray(proj, np.float64).reshape(12)), _dev(np.asarray(lut, np.int32))
        self.out = _dev(_i32(np.full(cap + TAIL, PAT_OUT, np.uint32)))
        self.keep = torch.full((cap + TAIL,), PAT_KEEP, dtype=torch.uint8).cuda()
        self.kept = torch.full((B + TAIL,), PAT_KEPT, dtype=torch.int64).cuda()
        if acc is None:
            self.conf = torch.full((ncls * ncls + TAIL,), PAT_ACC, dtype=torch.int64).cuda()
            self.counts = torch.full((3 + TAIL,), PAT_ACC, dtype=torch.int64).cuda()
        else:
            self.conf, self.counts = acc
        self.ws = torch.zeros(L.FULL_WS_PER_BLOCK * ((cap + L.FOV_BLOCK - 1) // L.FOV_BLOCK) + L.FULL_WS_FIXED,
                              dtype=torch.int32).cuda()
        ptr = lambda t: None if t is None else t.data_ptr()
        a = dict(points=ptr(self.pts), offsets=ptr(self.off_d), dims=ptr(self.dim_d), B=B, P=P,
                 proj=ptr(self.mat), main=ptr(self.main), main_off=ptr(self.moff_d), K=Kt, sub=ptr(self.sub),
                 gt=ptr(self.gt), lut=ptr(self.lut), nlut=int(self.lut.shape[0]), fill=fill, C=ncls, out=ptr(self.out),
                 keep=ptr(self.keep), kept=ptr(self.kept), counts=ptr(self.counts),
                 conf=ptr(self.conf) if gt is not None else None, ws=ptr(self.ws))
        a.update(over or {})
        self.args = a
        torch.cuda.synchronize()
        self.rc = L.lib().pmf_kitti_full_fill(
            a["points"], a["offsets"], a["dims"], a["B"], a["P"], a["proj"], a["main"], a["main_off"], a["K"], a["sub"],
            a["gt"], a["lut"], a["nlut"], a["fill"], a["C"], a["out"], a["keep"], a["kept"], a["counts"], a["conf"], a["ws"],
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def host(self):
        return dict(out=self.out.cpu().numpy().view(np.uint32), keep=self.keep.cpu().numpy(), kept=self.kept.cpu().numpy(),
                    counts=self.counts.cpu().numpy(), conf=self.conf.cpu().numpy())

    def untouched(self):
        h = self.host()
        return ((h["out"] == PAT_OUT).all() and (h["keep"] == PAT_KEEP).all() and (h["kept"] == PAT_KEPT).all()
                and (h["counts"] == PAT_ACC).all() and (h["conf"] == PAT_ACC).all())


def _compare(c, want, what, gt=True, keep=True, counts=True, conf=True, times=1):
    """one finished call against the restatement: every output that was asked for, and the pattern behind and beside them"""
    assert c.rc == 0, what
    h = c.host()
    n2 = c.ncls * c.ncls
    assert np.array_equal(h["out"][:c.P], np.concatenate(want["out"])), what
    assert (h["out"][:c.P] >> 16 == 0).all(), what
    assert np.array_equal(h["kept"][:c.B], want["kept_count"]), what
    assert (h["out"][c.P:] == PAT_OUT).all() and (h["kept"][c.B:] == PAT_KEPT).all(), what
    assert (h["keep"][c.P:] == PAT_KEEP).all() and (h["counts"][3:] == PAT_ACC).all() and (h["conf"][n2:] == PAT_ACC).all(), what
    if keep:
        assert np.array_equal(h["keep"][:c.P], np.concatenate(want["keep"]).astype(np.uint8)), what
    else:
        assert (h["keep"] == PAT_KEEP).all(), what
    if counts:
        assert np.array_equal(h["counts"][:3], PAT_ACC + times * want["counts"]), what
        assert int(want["counts"].sum()) == c.P, what
    else:
        assert (h["counts"] == PAT_ACC).all(), what
    if conf and gt:
        assert np.array_equal(h["conf"][:n2], PAT_ACC + times * want["conf"].reshape(-1)), what
        assert int(want["conf"].sum()) == c.P, what                  # every point is scored: LUT's classes all lie below NCLS
    else:
        assert (h["conf"] == PAT_ACC).all(), what


def _case(sizes, seed, rich=True, **kw):
    frames, dims, main, sub, gt = K.random_case(sizes, seed, **kw)
    for pts in frames:
        if (pts[:, 0] > 0.5).any():
            assert F.border_distance(pts, F.EXACT_PROJ, 8, 8) > 1e-6
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, K.NCLS, gt)
    assert K.is_rich(want) or not rich, "a degenerate case"
    return (frames, dims, F.EXACT_PROJ, main, sub, gt), want


# ---- raw ABI -------------------------------------------------------------------------------------------------------------
def test_frames_straddling_workgroups_and_an_empty_frame():
    args, want = _case(F.SEAM_SIZES, 11)
    assert (want["kept_count"] > 0).sum() >= 3 and want["kept_count"][2] == 0
    _compare(Call(*args), want, "seam sizes")


def test_one_frame_around_the_block_size():
    from pmf_amd import _lib as L
    for P in (L.FOV_BLOCK - 1, L.FOV_BLOCK, L.FOV_BLOCK + 1):
        args, want = _case([P], 20 + P)
        _compare(Call(*args), want, "P = %d" % P)
    seen = set()
    for seed in range(40, 48):                   # one point: it cannot show every source at once, the eight seeds together do
        args, want = _case([1], seed, rich=False)
        _compare(Call(*args), want, "P = 1, seed %d" % seed)
        seen.add((bool(want["keep"][0][0]), int(want["source"][0][0])))
    assert {s for _, s in seen} == {0, 1, 2} and {k for k, _ in seen} == {True, False}


def test_max_frames():
    from pmf_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(3))
    sizes = [int(n) for n in rng.integers(0, 41, L.FOV_MAX_FRAMES)]
    sizes[5] = sizes[63] = 0
    args, want = _case(sizes, 12)
    _compare(Call(*args), want, "64 frames")


def test_more_tiles_than_workgroups():
    """the fill kernel runs at most 512 workgroups and walks the tiles of FOV_BLOCK rows with that stride: 547 tiles"""
    from pmf_amd import _lib as L
    sizes = [300000, 1, 260000]
    assert sum(sizes) > 512 * L.FOV_BLOCK + 20000
    args, want = _case(sizes, 53)
    _compare(Call(*args), want, "547 tiles")


def _fov_keep(frames, dims, proj):
    from pmf_amd.dataset.semantic_kitti import fov_filter_gpu
    return [g[2] for g in fov_filter_gpu(frames, dims, proj)]


def test_keep_is_the_fov_filters_keep_on_any_input():
    """rows on the borders, NaN and infinite rows (exact_rows), and random rows with no distance kept from the border: the
    mask is pmf_fov_filter's bit for bit, and with that mask the outputs follow the rule"""
    rng = np.random.Generator(np.random.PCG64(7))
    rows = F.exact_rows()
    near = np.stack([np.ones(3000), rng.integers(0, 9, 3000) + rng.choice([0, 1e-7, -1e-7, 0.5], 3000),
                     rng.integers(0, 9, 3000) + rng.choice([0, 1e-7, -1e-7, 0.5], 3000), rng.random(3000)], 1).astype(np.float32)
    near[::97, rng.integers(0, 3)] = np.nan
    frames = [rows, rows, rows, near]
    dims = F.EXACT_DIMS + [(8, 8)]
    keeps = _fov_keep(frames, dims, F.EXACT_PROJ)
    assert any(k.any() and not k.all() for k in keeps)
    main = [K.words(rng, int(k.sum())) for k in keeps]
    sub, gt = [K.words(rng, len(f)) for f in frames], [K.words(rng, len(f)) for f in frames]
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, K.NCLS, gt, keeps=keeps)
    assert K.is_rich(want)
    c = Call(frames, dims, F.EXACT_PROJ, main, sub, gt)
    assert np.array_equal(c.host()["keep"][:c.P], np.concatenate(keeps).astype(np.uint8))
    _compare(c, want, "border rows")


# ---- corners ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "all"])
def test_a_view_that_keeps_nothing_and_one_that_keeps_all(mode):
    frames, _, dims = F.seam_frames(mode)
    rng = np.random.Generator(np.random.PCG64(13))
    n_kept = [len(f) if mode == "all" else 0 for f in frames]
    main = [K.words(rng, k) for k in n_kept]
    sub, gt = [K.words(rng, len(f)) for f in frames], [K.words(rng, len(f)) for f in frames]
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, K.LUT, K.FILL_ID, K.NCLS, gt)
    assert want["kept_count"].tolist() == n_kept
    assert (want["counts"][0] == 0) == (mode == "none")
    _compare(Call(frames, dims, F.EXACT_PROJ, main, sub, gt), want, mode)


def test_a_main_table_shorter_and_one_longer_than_the_kept_rows():
    """kept_count reports the kept rows whatever main holds; the rows behind a short table take the sub word, the words behind
    the kept rows of a long table are not used.  main_ids is a tensor of exactly K_total words."""
    args, want = _case(F.SEAM_SIZES, 17, short=1, extra=3)
    main = args[3]
    assert len(main[1]) == want["kept_count"][1] - 3 and len(main[3]) == want["kept_count"][3] + 5
    c = Call(*args)
    assert c.main.numel() == sum(len(m) for m in main) and c.main_buf.numel() * 4 % 512 == 0
    assert c.main.data_ptr() + 4 * c.main.numel() == c.main_buf.data_ptr() + 4 * c.main_buf.numel()
    _compare(c, want, "short and long main")
    none = [m[:0] for m in main]                                   # K_total = 0: main_ids NULL
    c = Call(args[0], args[1], args[2], none, args[4], args[5])
    assert c.args["main"] is None
    w0 = K.numpy_fill(args[0], args[1], args[2], none, args[4], K.LUT, K.FILL_ID, K.NCLS, args[5])
    assert w0["counts"][0] == 0 and np.array_equal(w0["kept_count"], want["kept_count"])
    _compare(c, w0, "no main word at all")


def test_main_offsets_that_break_every_assumption_stay_in_bounds():
    """a table that decreases, goes negative and far beyond K_total: the call answers, every word written is one the inputs
    hold (or the fill id), kept_count does not depend on the table, and nothing beside the outputs is touched"""
    args, want = _case(F.SEAM_SIZES, 19)
    Kt = sum(len(m) for m in args[3])
    for table in ([0, 2 ** 62, -5, 7, Kt + 10 ** 6, -2 ** 63], [Kt, Kt - 1, 0, 2 ** 40, 3, 2], [-3, -2, -1, 0, 1, 2]):
        c = Call(*args, main_off=table)
        assert c.rc == 0
        h = c.host()
        assert np.array_equal(h["kept"][:c.B], want["kept_count"]) and (h["kept"][c.B:] == PAT_KEPT).all()
        assert np.array_equal(h["keep"][:c.P], np.concatenate(want["keep"]).astype(np.uint8))
        assert (h["out"][c.P:] == PAT_OUT).all() and (h["keep"][c.P:] == PAT_KEEP).all()
        assert np.isin(h["out"][:c.P], K.ID_POOL).all()
        assert h["counts"][:3].sum() == 3 * PAT_ACC + c.P and (h["counts"][3:] == PAT_ACC).all()
        assert h["conf"][:K.NCLS ** 2].sum() == K.NCLS ** 2 * PAT_ACC + c.P and (h["conf"][K.NCLS ** 2:] == PAT_ACC).all()


def test_ids_beyond_the_table_and_a_short_table():
    """with a table of 41 entries the ids 150 .. 5000 are all class 0, on the prediction's side and on the label's"""
    frames, dims, main, sub, gt = K.random_case(F.SEAM_SIZES, 23)
    lut = K.LUT[:41].copy()
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, lut, K.FILL_ID, K.NCLS, gt)
    assert K.is_rich(want) and not np.isin(np.concatenate(want["out"]), [150, 252, 257, 259, 299, 300, 5000]).any()
    assert want["conf"][:, 0].sum() > 0.5 * sum(F.SEAM_SIZES)
    _compare(Call(frames, dims, F.EXACT_PROJ, main, sub, gt, lut=lut), want, "short table")
    one = np.array([3], np.int32)                                   # nlut = 1: only id 0 is inside, and it has a class
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, one, K.FILL_ID, K.NCLS, gt)
    assert want["counts"][2] > 0 and set(np.unique(np.concatenate(want["out"]))) == {0, K.FILL_ID}
    _compare(Call(frames, dims, F.EXACT_PROJ, main, sub, gt, lut=one), want, "table of one entry")
    # a table with classes outside 0 .. C-1: such rows are not counted, the labels do not change
    wide = K.LUT.copy()
    wide[252], wide[257] = K.NCLS, -2
    want = K.numpy_fill(frames, dims, F.EXACT_PROJ, main, sub, wide, K.FILL_ID, K.NCLS, gt)
    assert 0 < want["conf"].sum() < sum(F.SEAM_SIZES)
    c = Call(frames, dims, F.EXACT_PROJ, main, sub, gt, lut=wide)
    h = c.host()
    assert c.rc == 0 and np.array_equal(h["out"][:c.P], np.concatenate(want["out"]))
    assert np.array_equal(h["conf"][:K.NCLS ** 2], PAT_ACC + want["conf"].reshape(-1))


def test_high_halves_do_not_matter():
    (frames, dims, proj, main, sub, gt), want = _case(F.SEAM_SIZES, 29)
    assert all((np.concatenate(x) >> 16 != 0).any() for x in (main, sub, gt))
    low = lambda arrs: [a & 0xFFFF for a in arrs]
    _compare(Call(frames, dims, proj, main, sub, gt, fill=K.FILL_ID | 0x7FFF0000), want, "high halves set")
    _compare(Call(frames, dims, proj, low(main), low(sub), low(gt)), want, "high halves clear")


def test_every_optional_pointer_null():
    args, want = _case(F.SEAM_SIZES, 31)
    _compare(Call(*args, over=dict(keep=None)), want, "keep NULL", keep=False)
    _compare(Call(*args, over=dict(counts=None)), want, "counts NULL", counts=False)
    _compare(Call(*args, over=dict(conf=None)), want, "conf NULL", conf=False)
    _compare(Call(*args, over=dict(conf=None, gt=None)), want, "gt and conf NULL", conf=False)
    _compare(Call(*args[:5], None), want, "no gt array", gt=False)
    _compare(Call(*args, over=dict(keep=None, counts=None, conf=None, gt=None)), want, "all NULL", keep=False, counts=False,
             conf=False)


def test_two_calls_accumulate_and_give_identical_bits():
    args, want = _case(F.SEAM_SIZES, 37)
    a = Call(*args)
    b = Call(*args, acc=(a.conf, a.counts))
    ha, hb = a.host(), b.host()
    for key in ("out", "keep", "kept"):
        assert ha[key].tobytes() == hb[key].tobytes(), key
    _compare(b, want, "second call", times=2)
    c = Call(*args)                                                 # a third call on fresh accumulators: the first one's bits
    _compare(c, want, "third call")
    assert c.host()["out"].tobytes() == ha["out"].tobytes()


def test_every_error_returns_without_touching_the_outputs():
    from pmf_amd import _lib as L
    args, _ = _case(F.SEAM_SIZES, 41)
    bad = [dict(points=None), dict(offsets=None), dict(dims=None), dict(proj=None), dict(main=None), dict(main_off=None),
           dict(sub=None), dict(lut=None), dict(out=None), dict(kept=None), dict(ws=None), dict(gt=None), dict(B=0), dict(B=-3),
           dict(B=L.FOV_MAX_FRAMES + 1), dict(P=0), dict(P=-1), dict(K=-1), dict(C=0), dict(C=65), dict(C=-1), dict(nlut=0),
           dict(nlut=-4)]
    for kw in bad:
        c = Call(*args, over=kw)
        assert c.rc == L.PMF_E_ARG and c.untouched(), kw
    own = Call(*args)                       # its points, 4 and 8 bytes in: real memory, off the 16-byte grid
    for off in (4, 8):
        e = Call(*args, over=dict(points=own.pts.data_ptr() + off))
        assert e.rc == L.PMF_E_ARG and e.untouched(), off
    for P in (2 ** 31, 2 ** 33):
        c = Call(*args, over=dict(P=P))
        assert c.rc == L.PMF_E_UNSUPPORTED and c.untouched(), P


# ---- the wrapper ----------------------------------------------------------------------------------------------------------
def test_fov_fill_on_a_side_stream_and_its_length_check():
    from pmf_amd.postproc import fov_fill
    (frames, dims, proj, main, sub, gt), want = _case(F.SEAM_SIZES, 43)
    conf = torch.zeros((K.NCLS, K.NCLS), dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = fov_fill(frames, dims, proj, main, sub, K.LUT, K.FILL_ID, K.NCLS, gt=gt, conf=conf, counts=counts)
    side.synchronize()
    assert len(got) == len(frames)
    for g, w in zip(got, want["out"]):
        assert g.dtype == np.uint32 and np.array_equal(g, w)
    assert np.array_equal(conf.cpu().numpy(), want["conf"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
    bare = fov_fill((np.concatenate(frames), np.cumsum([0] + F.SEAM_SIZES)), dims, proj,
                    (np.concatenate(main), np.cumsum([0] + [len(m) for m in main])), np.concatenate(sub), K.LUT, K.FILL_ID,
                    K.NCLS)
    assert all(np.array_equal(g, w) for g, w in zip(bare, want["out"]))
    k3 = int(want["kept_count"][3])
    for wrong in (main[3][:-1], np.concatenate([main[3], main[3][:2]])):
        with pytest.raises(ValueError, match=r"frame 3: the camera sees %d of its 1025 points but the main prediction holds %d"
                           % (k3, len(wrong))):
            fov_fill(frames, dims, proj, main[:3] + [wrong] + main[4:], sub, K.LUT, K.FILL_ID, K.NCLS)
    before = (conf.clone(), counts.clone())                     # a refused batch leaves the caller's accumulators alone
    with pytest.raises(ValueError, match="frame 3"):
        fov_fill(frames, dims, proj, main[:3] + [main[3][:-1]] + main[4:], sub, K.LUT, K.FILL_ID, K.NCLS, gt=gt, conf=conf,
                 counts=counts)
    assert torch.equal(conf, before[0]) and torch.equal(counts, before[1])
    pair = fov_fill(tuple(frames[:2]), dims[:2], proj, tuple(main[:2]), tuple(sub[:2]), K.LUT, K.FILL_ID, K.NCLS)
    assert len(pair) == 2 and all(np.array_equal(g, w) for g, w in zip(pair, want["out"]))  # a tuple of two frames is two frames
    empty = fov_fill([frames[2]], [dims[2]], proj, [main[2]], [sub[2]], K.LUT, K.FILL_ID, K.NCLS)      # no point: no launch
    assert len(empty) == 1 and empty[0].shape == (0,)


# ---- the tasks -------------------------------------------------------------------------------------------------------------
def _load(name, path, option=None):
    saved = sys.modules.get("option")
    if option is not None:
        sys.modules["option"] = option
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            sys.modules.pop("option", None)
        else:
            sys.modules["option"] = saved
    return mod


def _task(tag, folder, script):
    opt = _load(tag + "_option", os.path.join(folder, "option.py"))
    return opt, _load(tag + "_" + script, os.path.join(folder, script + ".py"), opt)


def _write_words(folder, seq, frame, words):
    d = os.path.join(folder, "sequences", seq, "predictions")
    os.makedirs(d, exist_ok=True)
    np.ascontiguousarray(words, np.uint32).view(np.int32).tofile(os.path.join(d, frame + ".label"))


def _read_words(folder, seq, frame):
    return np.fromfile(os.path.join(folder, "sequences", seq, "predictions", frame + ".label"), dtype=np.uint32)


def _yaml(path, cfg):
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the synthetic raw tree of the FOV tests, its FOV tree, and a sub prediction for every raw point"""
    from oracle.cases import kitti_tree
    from pmf_amd.dataset.semantic_kitti import SemanticKitti, create_fov_dataset
    base = tmp_path_factory.mktemp("full")
    root, fov = str(base / "raw" / "sequences"), str(base / "fov" / "sequences")
    cfg, data = kitti_tree(root, **F.TREE)
    create_fov_dataset(root, fov, [0, 8], config_path=cfg, batch_frames=4)
    ds = SemanticKitti(root, [0, 8], cfg)
    ids = np.array(sorted(set(ds.data_config["learning_map_inv"].values())), np.uint32)   # what a prediction can hold
    assert ids[0] == 0 and len(ids) == 6
    rng = np.random.Generator(np.random.PCG64(5))
    sub = str(base / "sub")
    for (seq, frame), (pts, raw, img) in data.items():
        _write_words(sub, seq, frame, rng.choice(ids, pts.shape[0]))
    return dict(base=base, root=root, fov=fov, cfg=cfg, data=data, ds=ds, ids=ids, sub=sub)


def _expect(tree, main_folder, seqs, fill_class, ncls):
    """the restatement, frame by frame, on the files of main_folder and the tree's sub prediction"""
    ds, h, w = tree["ds"], F.TREE["h"], F.TREE["w"]
    out, conf, counts = {}, np.zeros((ncls, ncls), np.int64), np.zeros(3, np.int64)
    for (seq, frame), (pts, raw, img) in sorted(tree["data"].items()):
        if seq not in seqs:
            continue
        assert F.border_distance(pts, ds.proj_matrix[seq], h, w) > 1e-6
        want = K.numpy_fill([pts], [(h, w)], ds.proj_matrix[seq], [_read_words(main_folder, seq, frame)],
                            [_read_words(tree["sub"], seq, frame)], ds.class_map_lut, int(ds.class_map_lut_inv[fill_class]),
                            ncls, [raw])
        assert want["kept_count"][0] == _read_words(main_folder, seq, frame).shape[0]
        assert K.is_rich(want), (seq, frame)
        out[(seq, frame)] = want["out"][0]
        conf += want["conf"]
        counts += want["counts"]
    return out, conf, counts


def test_fullsweep_task_end_to_end(tree, tmp_path):
    """synthetic main predictions, one word per point of the FOV tree: every written file, the confusion matrix and the source
    counts equal the restatement, for every frame of both sequences; batches of 3 over 5 frames per sequence"""
    opt, main = _task("kitti_full", FULL_TASK, "main")
    rng = np.random.Generator(np.random.PCG64(9))
    main_dir = str(tmp_path / "main")
    for (seq, frame) in tree["data"]:
        k = os.path.getsize(os.path.join(tree["fov"], seq, "velodyne", frame + ".bin")) // 16
        _write_words(main_dir, seq, frame, rng.choice(tree["ids"], k))
    save = str(tmp_path / "out")
    conf = _yaml(str(tmp_path / "full.yaml"), dict(
        save_path=save, data_root=tree["root"], main_pred_folder=main_dir, sub_pred_folder=tree["sub"], sequences=[0, 8],
        has_label=True, merge_batch_size=3, fill_class=3, n_classes=6, data_config_path=tree["cfg"]))
    s = opt.Option(conf)
    assert [len(b) for b in main.batches(tree["ds"], 3)] == [3, 2, 3, 2]
    exp = main.Experiment(s)
    written = exp.run()
    want, wconf, wcounts = _expect(tree, main_dir, ("00", "08"), 3, 6)
    assert sorted(written) == sorted(want)
    for key, path in written.items():
        assert path == os.path.join(save, "sequences", key[0], "predictions", key[1] + ".label")
        assert np.array_equal(np.fromfile(path, dtype=np.uint32), want[key]), key
    assert np.array_equal(exp.merge_pred.evaluator.conf_matrix.cpu().numpy(), wconf)
    assert np.array_equal(exp.merge_pred.counts.cpu().numpy(), wcounts) and wcounts.min() > 0
    assert wconf.sum() == sum(v[0].shape[0] for v in tree["data"].values())
    chk = _load("kitti_full_check_valid", os.path.join(FULL_TASK, "check_valid.py"), opt)
    chk.Experiment(s).run()
    # a main prediction under another keep rule (one label short): refused, naming the frame
    short = _read_words(main_dir, "08", "000004")[:-1]
    _write_words(main_dir, "08", "000004", short)
    with pytest.raises(ValueError, match=r"sequence 08, frames 000003 \.\. 000004 .*: fov_fill: frame 1: the camera sees %d"
                       % (short.shape[0] + 1)):
        main.Experiment(s).run()


def test_fullsweep_from_the_pmf_evaluation_on_the_raw_tree(tmp_path):
    """tasks/pmf_eval_semantickitti on the FOV tree and on the raw tree write the same files (the loader's keep mask is the
    filter's: same K), so the full sweeps are the same; a 48 x 160 tree of one sequence and two frames"""
    from oracle.cases import kitti_tree
    from pmf_amd.dataset.semantic_kitti import create_fov_dataset
    root, fov = str(tmp_path / "raw" / "sequences"), str(tmp_path / "fov" / "sequences")
    cfg_path, data = kitti_tree(root, seed=6, seqs=(8,), frames=2, npts=3000, h=48, w=160)
    create_fov_dataset(root, fov, [8], config_path=cfg_path)
    popt, infer = _task("kitti_pmf_eval", PMF_TASK, "infer")
    with open(os.path.join(PMF_TASK, "config_server_kitti.yaml")) as f:
        icfg = yaml.safe_load(f)
    icfg.update(data_config_path=cfg_path, nclasses=6, sequences={"valid": [8]}, has_label=True)
    icfg["sensor"].update(proj_h=48, proj_w=160, h_pad=8, w_pad=0)
    preds, weights = {}, str(tmp_path / "pmf.pth")
    for name, where in (("fov", fov), ("raw", root)):
        icfg.update(save_path=str(tmp_path / ("eval_" + name)), data_root=where,
                    pretrained_model=weights if os.path.isfile(weights) else None)
        s = popt.Option(_yaml(str(tmp_path / (name + ".yaml")), icfg))
        exp = infer.Experiment(s)
        if not os.path.isfile(weights):
            torch.save(exp.model.state_dict(), weights)
        exp.run()
        preds[name] = os.path.join(s.save_path, "preds")
    rng = np.random.Generator(np.random.PCG64(2))
    ids = np.array([0, 1, 10, 11, 13, 30, 40, 44, 48, 50, 70, 72, 80, 252, 259], np.uint32)
    sub = str(tmp_path / "sub")
    for (seq, frame), (pts, raw, img) in data.items():
        a, b = _read_words(preds["fov"], seq, frame), _read_words(preds["raw"], seq, frame)
        assert a.shape[0] == os.path.getsize(os.path.join(fov, seq, "velodyne", frame + ".bin")) // 16 < pts.shape[0]
        assert a.tobytes() == b.tobytes(), frame
        _write_words(sub, seq, frame, rng.choice(ids, pts.shape[0]))
    opt, main = _task("kitti_full", FULL_TASK, "main")
    files = {}
    for name in ("fov", "raw"):
        save = str(tmp_path / ("out_" + name))
        s = opt.Option(_yaml(str(tmp_path / ("full_%s.yaml" % name)), dict(
            save_path=save, data_root=root, main_pred_folder=preds[name], sub_pred_folder=sub, sequences=[8],
            has_label=True, fill_class=3, n_classes=6, data_config_path=cfg_path)))
        written = main.Experiment(s).run()
        files[name] = {k: np.fromfile(p, dtype=np.uint32) for k, p in written.items()}
    assert sorted(files["raw"]) == sorted(data)
    for key, (pts, raw, img) in data.items():
        assert files["raw"][key].shape[0] == pts.shape[0] and np.array_equal(files["raw"][key], files["fov"][key]), key


def _salsa_tree(tmp_path):
    """one sequence of five sweeps whose label file also knows raw id 257; sweep 000001 carries 257 and 259"""
    from oracle.cases import kitti_tree
    from pmf_amd.dataset.semantic_kitti import SemanticKitti
    root = str(tmp_path / "sequences")
    cfg_path, data = kitti_tree(root, seed=8, seqs=(8,), frames=5, npts=1500)
    with open(cfg_path) as f:
        lab = yaml.safe_load(f)
    lab["learning_map"][257] = 4
    lab["color_map"][257] = [1, 2, 3]
    lab["content"][257] = 0.01
    _yaml(cfg_path, lab)
    path = os.path.join(root, "08", "labels", "000001.label")
    raw = np.fromfile(path, dtype=np.uint32)
    raw[::5] = (raw[::5] & 0xFFFF0000) | 257
    raw.tofile(path)
    assert (raw & 0xFFFF == 257).sum() >= 300 and (raw & 0xFFFF == 259).sum() > 0
    return root, cfg_path, SemanticKitti(root, [8], cfg_path, has_image=False)


@pytest.mark.parametrize("use_knn", [False, True])
def test_salsanext_eval_semantickitti_task(tmp_path, use_knn):
    """a random-initialised SalsaNext at 32 x 512, batches of 3 over 5 sweeps (a short last batch): every file equals
    class_map_lut_inv[argmax[py, px]] (or the per-sweep KNN vote) composed from torch ops on the network's own outputs, the
    point confusion equals numpy's with the WHOLE label table: raw ids 257 and 259 keep their classes"""
    import pc_processor
    from pmf_amd.models import SalsaNext
    from pmf_amd.utils.detinit import deterministic_init
    from tests import salsa_eval_cases as S
    root, cfg_path, ds = _salsa_tree(tmp_path)
    assert ds.class_map_lut.shape[0] > 259 and ds.class_map_lut[257] == 4 and ds.class_map_lut[259] == 2
    opt, infer = _task("kitti_salsa", SALSA_TASK, "infer")
    with open(os.path.join(SALSA_TASK, "config_server_kitti.yaml")) as f:
        cfg = yaml.safe_load(f)
    ncls = 6
    cfg.update(save_path=str(tmp_path / "out"), data_root=root, data_config_path=cfg_path, n_classes=ncls, sequences=[8],
               eval_batch_size=3, pretrained_model=None, print_frequency=1, sensor=dict(S.CONFIG["sensor"]))
    cfg["post"]["KNN"]["use"] = use_knn
    s = opt.Option(_yaml(str(tmp_path / "salsa.yaml"), cfg))
    exp = infer.Experiment(s, model=deterministic_init(SalsaNext(in_channels=5, nclasses=ncls)))
    outs = []
    exp.model.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()) and None)
    written = exp.run()
    assert [tuple(o.shape) for o in outs] == [(3, ncls, 32, 512), (2, ncls, 32, 512)]
    assert sorted(written) == [("08", "%06d" % i) for i in range(5)]
    loader = pc_processor.dataset.SalsaNextLoader(ds, cfg, is_train=False, return_uproj=True, label_lut=ds.class_map_lut)
    assert tuple(loader._label_lut().shape) == ds.class_map_lut.shape
    assert tuple(pc_processor.dataset.SalsaNextLoader(ds, cfg, is_train=False)._label_lut().shape) == (256,)
    knn = pc_processor.postproc.KNN(cfg["post"]["KNN"]["params"], ncls)
    lut_inv = torch.from_numpy(ds.class_map_lut_inv).cuda()
    conf = np.zeros((ncls, ncls), np.int64)
    for i in range(5):
        it = loader._eval_item(i)
        amap = outs[i // 3][i % 3].argmax(dim=0)
        px, py = it["px"].long(), it["py"].long()
        gather = amap[py, px]
        lab = knn(it["proj_range"], it["depth"], amap, px, py).reshape(-1).long() if use_knn else gather
        path = written[("08", "%06d" % i)]
        assert path == os.path.join(s.save_path, "preds", "sequences", "08", "predictions", "%06d.label" % i)
        got = np.fromfile(path, dtype=np.int32)
        assert got.shape[0] == ds.loadDataByIndex(i)[0].shape[0]
        assert np.array_equal(got, lut_inv[lab].cpu().numpy().astype(np.int32)), i
        raw = np.fromfile(ds.label_files[i], dtype=np.uint32) & 0xFFFF
        np.add.at(conf, (lab.cpu().numpy(), ds.class_map_lut[raw]), 1)
    got_conf = exp.inference.evaluator.conf_matrix.cpu().numpy()
    assert np.array_equal(got_conf, conf)
    raw1 = np.fromfile(ds.label_files[1], dtype=np.uint32) & 0xFFFF
    cut = ds.class_map_lut.copy()
    cut[256:] = 0                                                    # what a 256-entry table would have scored
    assert conf[:, 0].sum() < np.add.reduce([(cut[np.fromfile(f, dtype=np.uint32) & 0xFFFF] == 0).sum() for f in ds.label_files])
    assert conf[:, 4].sum() >= (raw1 == 257).sum() > 0 and (raw1 == 259).sum() > 0
