"""Forward / input-gradient convolution cases for tests/test_conv_reference_host.py and tests/test_gpu_conv.py (host only: numpy,
torch on the CPU, ctypes).

  * A case is ONE pmf_conv_desc_t (include/pmf_amd.h) in one of two forms.  "fwd": operands with views, the taps of taps_of,
    bias, activation, optional ep_pmask, optional stats.  "dgrad": exactly what plan_conv.py::_dgrad / _dgrad_launch /
    _dgrad_merged build -- ONE operand dz, negated taps (or the stride-2 parity sub-taps with out_sy = out_sx = 2 and
    out_oy / ox = py / px), a transposed pack addressed at the operand's column offset, ACT_NONE, accumulate, ep_cmul,
    ep_relu_x with or without ep_relu_scale / shift, stats with ep_stat_mean (with and without PMF_EP_STAT_X_ONLY), ndst
    destinations each with an epilogue of its own.  Both forms are the same GEMM: W[tap][k][column], k over the operands.
  * reference(): the GEMM sum in numpy float64 straight from the descriptor-shaped case (not autograd), with S = the same sum
    over absolute values + |bias| and M = the sum over the magnitudes the operand view can move (wgrad_cases.transformed: the
    view of pmf_src_t -- scale / shift in float32, ReLU, cmul, zero padding AFTER the transform, broadcast).
    epilogue(): conv_epi.h restated in float32 in its own operation order -- + bias, activation, * (ecm * pm), mask test
    !(x * rs + rt > 0), + old -- and the statistics expected from THOSE float32 outputs, folded in float64.
  * inputs(): "exact" inputs on which no summation order can round (exactness()), "random" full-mantissa operands / weights,
    and the two one-hot forms.
  * fill_desc(): ONE descriptor builder over raw device pointers; packs(): the fp32 pack, the split-bf16 pack and the stem
    format-2 pack made on the host (gpu_helpers.pack_fwd*_host).
  * CASES: the smallest shapes that still cross every seam of a 4 x 32-pixel segment tile (MT 1 and 2, output-channel tiles of
    32 and 64); LAUNCHES: every (case, weights form, cfg, ticket array) the GPU file runs, with the kernel it must reach."""
import ctypes as C
import zlib

import numpy as np
import torch

from pmf_amd import _lib as L
from tests.gpu_helpers import SENT, pack_fwd_host, pack_fwd_s3_host, pack_fwd_s3_stem_host, taps_of
from tests.wgrad_cases import Src, tap_view, transformed

F32, F64 = np.float32, np.float64
FAKE = 0x10000


def ru(v, m):
    return (v + m - 1) // m * m


def tile(bn, mt, ks=0):
    return bn | (mt << 8) | (ks << 16)


class Dst:
    """one destination and its epilogue.  relu: None / "plain" (ep_relu_x alone) / "affine" (+ ep_relu_scale / shift);
    stat: None / "sq" (sum, sum of squares) / "mean" (ep_stat_mean next to the ReLU mask) / "x_only" (PMF_EP_STAT_X_ONLY)"""

    def __init__(self, C_, ldc=None, acc=0, cmul=False, relu=None, stat=None):
        assert stat != "mean" or relu
        assert stat != "x_only" or not relu
        self.C, self.ldc, self.acc, self.cmul, self.relu, self.stat = C_, ldc or ru(C_, 8), acc, cmul, relu, stat
        self.rldc = ru(C_, 8) + 4


class Case:
    def __init__(self, name, form, N, OH, OW, srcs, Cout, taps, stride=1, gather=0, bias=False, act=L.ACT_NONE, pmask=False,
                 dsts=None, out_H=None, out_W=None, out_s=1, out_o=(0, 0), C_real=None, ldw=None, coloff=0, Ctot=None,
                 conv=None, stem=False, parent=None, force_s3=False):
        self.force_s3 = force_s3                   # split-bf16 weights although pmf_conv_s3_eligible says 0 (pmf_conv_fwd runs it)
        self.name, self.form, self.N, self.OH, self.OW, self.srcs, self.Cout = name, form, N, OH, OW, srcs, Cout
        self.taps, self.stride, self.gather, self.bias, self.act, self.pmask = list(taps), stride, gather, bias, act, pmask
        self.dsts = dsts or [Dst(Cout)]
        assert sum(d.C for d in self.dsts) == Cout
        self.out_H, self.out_W, self.out_s, self.out_o = out_H or OH, out_W or OW, out_s, out_o
        self.Ktot = sum(s.C for s in srcs)
        self.C_real = C_real or self.Ktot          # single operand: channels [C_real, C) are zero (or beyond the pitch)
        self.Ctot = Ctot or Cout                   # columns of the pack; this launch takes [coloff, coloff + Cout)
        self.coloff = coloff
        self.ldw = ldw or (ru(self.Ctot, 64) + (64 if form == "dgrad" else 0))
        self.conv, self.stem, self.parent = conv, stem, parent

    @property
    def npix(self):
        return self.N * self.OH * self.OW

    def rows_y(self):
        return slice(self.out_o[0], self.out_o[0] + (self.OH - 1) * self.out_s + 1, self.out_s)

    def rows_x(self):
        return slice(self.out_o[1], self.out_o[1] + (self.OW - 1) * self.out_s + 1, self.out_s)

    def single(self, k):
        """destination k of a merged launch as the per-operand launch _dgrad_launch builds: the same pack at the operand's
        column offset, the same epilogue"""
        c0 = sum(d.C for d in self.dsts[:k])
        return Case("%s.dst%d" % (self.name, k), self.form, self.N, self.OH, self.OW, self.srcs, self.dsts[k].C, self.taps,
                    self.stride, self.gather, False, self.act, False, [self.dsts[k]], self.out_H, self.out_W, self.out_s,
                    self.out_o, self.C_real, self.ldw, self.coloff + c0, self.Ctot, None, self.stem, (self, k))

    def plain(self):
        """the same GEMM without views, bias, activation or epilogue (the one-hot forms)"""
        srcs = [Src(s.C, s.H, s.W, s.ldc, bcast=s.bcast) for s in self.srcs]
        c = Case(self.name, self.form, self.N, self.OH, self.OW, srcs, self.Cout, self.taps, self.stride, self.gather, False,
                 L.ACT_NONE, False, [Dst(d.C, d.ldc) for d in self.dsts], self.out_H, self.out_W, self.out_s, self.out_o,
                 self.C_real, self.ldw, self.coloff, self.Ctot, self.conv, self.stem, None, self.force_s3)
        return c


# ------------------------------------------------------------------------------------------------ the case table
def fwd(name, N, H, W, cins, Cout, k, dil=1, stride=1, gather=0, raw=False, bias=True, act=L.ACT_LRELU, pmask=False, stat="sq",
        bcast=(), ldc_pad=0, out_pad=0, C_real=None, stem=False, force_s3=False):
    """an ordinary convolution (`same` padding; k = 2: dilation 2, padding 1).  Operand i gets scale / shift unless raw, ReLU
    on every other operand, cmul on the first"""
    pad = 1 if k == 2 else dil * (k - 1) // 2
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    srcs = []
    for i, c in enumerate(cins):
        b = i in bcast
        srcs.append(Src(c, 1 if b else H, 1 if b else W, c + ldc_pad, aff=not raw, relu=(not raw) and i % 2 == 1,
                        cmul=(not raw) and i == 0, bcast=b))
    return Case(name, "fwd", N, OH, OW, srcs, Cout, taps_of(k, k, dil, pad), stride, gather, bias, act, pmask,
                [Dst(Cout, ru(Cout, 8) + out_pad, stat=stat)], C_real=C_real, stem=stem,
                conv=dict(k=k, dil=dil, pad=pad, stride=stride), force_s3=force_s3)


def dgrad(name, N, H, W, cins, Cf, k, dil=1, stride=1, gather=0, which=0, dsts=None, Kd=None, dz_ldc=None, merged=False,
          cls=None):
    """the input gradient of Conv2d(sum(cins) -> Cf, k, dil, stride) on an H x W map with respect to operand `which` (or, merged,
    all operands in one launch); cls = (py, px): one parity class of a stride-2 layer"""
    pad = 1 if k == 2 else dil * (k - 1) // 2
    zH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    zW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    full = [(dy, dx, i) for i, (dy, dx) in enumerate(taps_of(k, k, dil, pad))]
    py, px = cls or (0, 0)
    if stride == 1:
        sub, mh, mw = [(-dy, -dx, wi) for dy, dx, wi in full], H, W
    else:
        sub = [((py - dy) // 2, (px - dx) // 2, wi) for dy, dx, wi in full if (py - dy) % 2 == 0 and (px - dx) % 2 == 0]
        mh, mw = (H - py + 1) // 2, (W - px + 1) // 2
    assert sub
    Kd = Kd or ru(Cf, 8)
    coloff = 0 if merged else sum(cins[:which])
    Cout, Ctot, col0 = sum(cins) if merged else cins[which], sum(cins), 0
    if coloff % 32:      # an operand that does not start on a 32-column fragment gets a pack of its own channel range (_dgrad)
        Ctot, col0, coloff = Cout, coloff, 0
    dsts = dsts or ([Dst(c) for c in cins] if merged else [Dst(Cout)])
    return Case(name, "dgrad", N, mh, mw, [Src(Kd, zH, zW, dz_ldc or Kd)], Cout, [(dy, dx) for dy, dx, _ in sub], 1, gather,
                False, L.ACT_NONE, False, dsts, H, W, stride, (py, px), min(Cf, Kd), None, coloff, Ctot,
                conv=dict(k=k, dil=dil, pad=pad, stride=stride, H=H, W=W, cins=list(cins), Cf=Cf, widx=[wi for _, _, wi in sub],
                          col0=col0))


def _cases():
    A, R, N_ = L.ACT_LRELU, L.ACT_RELU, L.ACT_NONE
    out = [
        # ---- forward: one tap
        fwd("f_1x1_16_20", 2, 5, 33, [16], 20, 1, act=A),                                  # Cout < out_ldc, ragged 32-tile
        fwd("f_1x1_8_32_raw", 2, 3, 31, [8], 32, 1, raw=True, C_real=5, ldc_pad=4),        # generic loop: 8-channel operand
        fwd("f_1x1_16+64_48", 2, 9, 37, [16, 64], 48, 1, act=R, out_pad=8),                # 5 K steps, two operands with views
        fwd("f_1x1_3x64_80_full", 2, 4, 32, [64, 64, 64], 80, 1, raw=True, act=N_),        # full 4 x 32 tiles: 64-channel stages
        fwd("f_1x1_s2_64_128", 2, 9, 65, [64], 128, 1, stride=2, raw=True, act=R),         # 5 x 33 outputs of a 9 x 65 map
        fwd("f_1x1_32+bcast_24", 2, 5, 33, [32, 16], 24, 1, bcast=(1,), act=A),
        # one tap on split-bf16 weights, either side of conv_direct_lds's 96 KiB: 448 channels = 28 K steps x 3 KiB + 7424 B of
        # tables = 93440 B stay resident in LDS, 512 channels = 32 x 3 KiB + 8448 B = 106752 B stream in chunks of 8 K steps (the
        # form of the network's 768-channel 1x1 layers); the launch table pins the LDS size, which tells the two apart
        fwd("f_1x1_448_48_resident", 2, 4, 32, [448], 48, 1, raw=True, act=A),
        fwd("f_1x1_512_48_stream", 2, 4, 32, [512], 48, 1, raw=True, act=A),
        dgrad("d_1x1_64_from512_stream", 2, 4, 32, [64], 512, 1, dsts=[Dst(64, cmul=True, relu="plain")]),
        # one tap on split-bf16 weights whose fragments neither fit LDS nor stream in chunks: four 16-channel slabs per stage
        fwd("f_1x1_1792_32", 1, 4, 32, [1792], 32, 1, raw=True, act=N_, force_s3=True),
        # ---- forward: windows
        fwd("f_2x2d2_16+64_48", 2, 5, 37, [16, 64], 48, 2, 2, act=A),
        fwd("f_2x2d2_64_64", 2, 9, 33, [64], 64, 2, 2, raw=True, act=R),
        fwd("f_3x3_16_24_pmask", 2, 9, 31, [16], 24, 3, act=R, pmask=True),
        fwd("f_3x3_64_128", 2, 5, 65, [64], 128, 3, act=A),
        fwd("f_3x3d2_32_32", 2, 9, 33, [32], 32, 3, 2, raw=True, act=N_, stat=None),
        fwd("f_3x3d6_16_16", 2, 9, 37, [16], 16, 3, 6, act=A),
        fwd("f_3x3d18_16_20_gather", 2, 5, 37, [16], 20, 3, 18, gather=1, raw=True, act=A),
        fwd("f_3x3_s2_64_128", 2, 9, 65, [64], 128, 3, stride=2, raw=True, act=A),
        fwd("f_3x3_256_32_ksplit", 2, 3, 31, [256], 32, 3, raw=True, act=A),
        fwd("f_7x7_8_64_stem", 2, 9, 37, [8], 64, 7, raw=True, C_real=3, act=R, stem=True),
        fwd("f_7x7_8_32_stem_view", 2, 5, 33, [8], 32, 7, C_real=5, act=A, stem=True),
        # ---- input gradient: stride 1
        dgrad("d_1x1_32_from20_k32", 2, 5, 33, [32], 20, 1, Kd=32, dz_ldc=24,               # the 24 -> 32 case
              dsts=[Dst(32, relu="plain", stat="mean")]),
        dgrad("d_1x1_16+64_from48", 2, 9, 37, [16, 64], 48, 1, which=1, dsts=[Dst(64, 72, acc=1, cmul=True, relu="affine")]),
        dgrad("d_1x1_3x64_from64_full", 2, 4, 32, [192], 64, 1, dsts=[Dst(192, stat="x_only")]),
        dgrad("d_2x2d2_32_from32", 2, 5, 37, [32], 32, 2, 2, dsts=[Dst(32, 40, relu="plain")]),
        dgrad("d_3x3_32_from64", 2, 9, 31, [32], 64, 3, dsts=[Dst(32, cmul=True, relu="affine", stat="mean", acc=1)]),
        dgrad("d_3x3_128_from64", 2, 5, 65, [128], 64, 3, dsts=[Dst(128, stat="x_only")]),
        dgrad("d_3x3d6_16_from16", 2, 9, 37, [16], 16, 3, 6, dsts=[Dst(16, 24, acc=1)]),
        dgrad("d_3x3d18_16_from24_gather", 2, 5, 37, [16], 24, 3, 18, gather=1, dsts=[Dst(16, relu="plain")]),
        dgrad("d_3x3_256_from256_ksplit", 2, 3, 31, [256], 256, 3, dsts=[Dst(256, cmul=True, relu="affine", stat="mean")]),
        dgrad("d_3x3_merged_32+64+32", 2, 9, 33, [32, 64, 32], 64, 3, merged=True,
              dsts=[Dst(32, 40, relu="affine", stat="mean"), Dst(64, acc=1, cmul=True), Dst(32, stat="x_only")]),
        dgrad("d_2x2d2_merged_64+64", 2, 5, 37, [64, 64], 32, 2, 2, merged=True,
              dsts=[Dst(64, acc=1, relu="plain"), Dst(64, 72, cmul=True, stat="x_only")]),
        dgrad("d_1x1_s2_64_from128", 2, 9, 65, [64], 128, 1, stride=2, cls=(0, 0), dsts=[Dst(64, acc=1, relu="plain")]),
    ]
    # ---- input gradient of a stride-2 3x3: the four parity classes, in the order the plan issues them
    for py in range(2):
        for px in range(2):
            out.append(dgrad("d_3x3_s2_64_from128.p%d%d" % (py, px), 2, 9, 65, [64], 128, 3, stride=2, cls=(py, px),
                             dsts=[Dst(64, 72, acc=1, cmul=True, relu="affine")]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PARITY = ["d_3x3_s2_64_from128.p%d%d" % (py, px) for py in range(2) for px in range(2)]
MERGED = [c.name for c in CASES if len(c.dsts) > 1]
SIGMOID = "f_1x1_16_20"             # the precision test also runs this case with PMF_ACT_SIGMOID


# ------------------------------------------------------------------------------------------------ inputs
def _rng(name, mode, salt=0):
    return np.random.RandomState(zlib.crc32(("%s/%s/%d" % (name, mode, salt)).encode()) & 0x7FFFFFFF)


def sentinel(shape):
    return np.full(shape, SENT, np.uint32).view(F32)


def lattice(case):
    """(Ly, Lx): two operand pixels this far apart never meet in one output's window"""
    dys, dxs = [t[0] for t in case.taps], [t[1] for t in case.taps]
    return max(dys) - min(dys) + 1, max(dxs) - min(dxs) + 1


def inputs(case, mode, salt=0):
    """dict(x = [N, H, W, ldc] per operand with NaN in the pitch padding and ZERO in the channels [C_real, C) of a single operand,
    scale / shift [C] or None, cmul [N, C + 8] or None, W [ntaps, Ktot, Ctot] (Wwin: the layer's whole window), bias [Cout] or None, pmask [N, out_H, out_W] or
    None, dst = [dict(out0 [N, out_H, out_W, ldc]: the sentinel, or integers in [0, C) under accumulate; cmul [N, C + 8],
    relu_x [N, out_H, out_W, rldc], rs, rt, mean [C] -- or None)]).
    mode "exact": see exactness().  "random": operands in [-1, 1), scale in [0.5, 1.5), shift in [-0.5, 0.5), weights in
    [-0.2, 0.2), bias in [-1, 1); the epilogue's own inputs stay as in "exact" (no mask decision on a rounding).
    "onehot_w" (case.plain()): ONE power of two per output column, at tap (column + salt) % ntaps and a K position whose
    place in the 16-deep step is (column + 8 salt) % 16 -- over two salts every column meets both halves of its B fragment
    and the columns together all 16 places --, operands with full mantissas.  "onehot_x": ONE power of two per operand pixel
    on the lattice() grid (shifted by sample and salt), at channel (3 y + 5 x + n + 8 salt) % C_real; weights with full
    mantissas."""
    if case.parent is not None:
        par, k = case.parent
        inp = dict(inputs(par, mode, salt))
        inp["dst"] = [inp["dst"][k]]
        return inp
    group = case.name.split(".p")[0]                 # the parity classes of one layer share dz, weights and the gradient map
    g = _rng(group, mode, salt)
    N, exact = case.N, mode == "exact"
    wscale = 4 if any(d.cmul for d in case.dsts) else 1          # the GEMM sums are multiples of 4 where ep_cmul multiplies them
    xs, scs, shs, cms = [], [], [], []
    single = len(case.srcs) == 1
    for i, s in enumerate(case.srcs):
        cols = min(s.C, s.ldc)
        shape = (N, s.H, s.W, cols)
        if exact:
            if s.cmul:
                sc = g.choice([1.0, 2.0], s.C).astype(F32)
                sh = (4 * g.randint(-1, 2, s.C)).astype(F32)
                v = (4 * g.randint(-2, 3, shape)).astype(F32)
            else:
                sc = g.choice([0.5, 1.0, 2.0], s.C).astype(F32)
                sh = g.randint(-2, 3, s.C).astype(F32)
                v = g.randint(-4, 5, shape).astype(F32)
                if s.aff:
                    v = np.where(sc[:cols] == 0.5, np.trunc(v / 2) * 2, v).astype(F32)
        else:
            sc = g.uniform(0.5, 1.5, s.C).astype(F32)
            sh = g.uniform(-0.5, 0.5, s.C).astype(F32)
            v = g.uniform(-1, 1, shape).astype(F32)
        if mode == "onehot_x":
            Ly, Lx = lattice(case)
            v = np.zeros(shape, F32)
            full = [j for j, o in enumerate(case.srcs) if not o.bcast]       # (a broadcast operand stays zero)
            for n in range(N if not s.bcast else 0):
                for y in range((n + salt) % Ly, s.H, Ly):
                    for x in range((n + 2 * salt) % Lx, s.W, Lx):
                        if full[(y + x + n) % len(full)] != i:                # ONE operand holds the pixel's value
                            continue
                        c = (3 * y + 5 * x + n + 8 * salt) % (case.C_real if single else s.C)
                        v[n, y, x, c] = 2.0 ** ((y + x) % 5 - 2) * (-1) ** (x + n)
        x = np.full((N, s.H, s.W, s.ldc), np.nan, F32)
        x[..., :cols] = v
        if single and case.C_real < cols:
            x[..., case.C_real:cols] = 0.0
        xs.append(x)
        aff = s.aff and mode in ("exact", "random")
        scs.append(sc if aff else None)
        shs.append(sh if aff else None)
        cms.append((g.rand(N, s.C + 8) > 0.25).astype(F32) * F32(1.25) if s.cmul and mode in ("exact", "random") else None)
    nt, K, Ct = len(case.taps), case.Ktot, case.Ctot
    widx = case.conv.get("widx", list(range(nt)))    # the launch's taps in the layer's window (drawn whole, for all classes)
    nwin = case.conv["k"] ** 2
    Wwin = None
    if exact:
        Wwin = (wscale * g.randint(-2, 3, (nwin, K, Ct))).astype(F32)
        Wm = Wwin[widx]
    elif mode == "onehot_w":
        Wm = np.zeros((nt, K, Ct), F32)
        for co in range(Ct):
            k16 = case.C_real // 16
            kk = (co + 8 * salt) % 16 + 16 * ((3 * co + salt) % k16) if k16 else (co + 4 * salt) % case.C_real
            Wm[(co + salt) % nt, kk, co] = 2.0 ** (co % 7 - 3) * (-1) ** co
    else:
        Wwin = g.uniform(-0.2, 0.2, (nwin, K, Ct)).astype(F32)
        Wm = Wwin[widx]
    if single:
        Wm[:, case.C_real:, :] = 0.0
        if Wwin is not None:
            Wwin[:, case.C_real:, :] = 0.0
    bias = None
    if case.bias:
        bias = (wscale * g.randint(-8, 9, case.Cout)).astype(F32) if exact else g.uniform(-1, 1, case.Cout).astype(F32)
    ge = _rng(group, "epilogue")                 # the epilogue's own inputs: the same in every mode
    pmask = (ge.rand(N, case.out_H, case.out_W) > 0.3).astype(F32) if case.pmask else None
    dst = []
    for d in case.dsts:
        e = dict(cmul=None, relu_x=None, rs=None, rt=None, mean=None)
        out0 = sentinel((N, case.out_H, case.out_W, d.ldc)).copy()
        pre = ge.randint(-8, 9, (N, case.out_H, case.out_W, d.C)).astype(F32)
        if d.acc:
            out0[..., :d.C] = pre
        e["out0"] = out0
        if d.cmul:
            e["cmul"] = (ge.rand(N, d.C + 8) > 0.25).astype(F32) * F32(1.25)
        if d.relu or d.stat == "x_only":
            rx = np.full((N, case.out_H, case.out_W, d.rldc), np.nan, F32)
            rx[..., :d.C] = 2 * ge.randint(-3, 4, (N, case.out_H, case.out_W, d.C))
            e["relu_x"] = rx
        if d.relu == "affine":
            e["rs"] = ge.choice([0.5, 1.0, 2.0], d.C).astype(F32)
            e["rt"] = ge.randint(-2, 3, d.C).astype(F32)
        if d.stat in ("mean", "x_only"):
            e["mean"] = ge.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], d.C).astype(F32)
        dst.append(e)
    return dict(x=xs, scale=scs, shift=shs, cmul=cms, W=Wm, Wwin=Wwin, bias=bias, pmask=pmask, dst=dst)


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(case, inp):
    """(G, S, M), each [N, OH, OW, Cout] float64: the GEMM sum WITHOUT the bias, the sum of |in_t| |w| + |bias|, and the sum of
    mag_t |w| + |bias| (mag_t = (|x scale| + |shift|) cmul: what an fma in place of the reference's float32 product and sum can
    move in_t by, in units of 2^-24)"""
    tr = [transformed(case, inp, i) for i in range(len(case.srcs))]
    Kr = case.C_real
    Wm = inp["W"][:, :Kr, case.coloff:case.coloff + case.Cout].astype(F64)
    G, S, M = (np.zeros((case.npix, case.Cout), F64) for _ in range(3))
    for t, (dy, dx) in enumerate(case.taps):
        a = np.concatenate([tap_view(v, case, dy, dx) for v, _ in tr], -1).reshape(case.npix, -1)[:, :Kr]
        m = np.concatenate([tap_view(mg, case, dy, dx) for _, mg in tr], -1).reshape(case.npix, -1)[:, :Kr]
        G += a @ Wm[t]
        S += np.abs(a) @ np.abs(Wm[t])
        M += m @ np.abs(Wm[t])
    if inp["bias"] is not None:
        S += np.abs(inp["bias"].astype(F64))
        M += np.abs(inp["bias"].astype(F64))
    sh = (case.N, case.OH, case.OW, case.Cout)
    return G.reshape(sh), S.reshape(sh), M.reshape(sh)


def f32_of(ref64):
    return (ref64 + 0.0).astype(F32)          # (+ 0.0: a float32 accumulator that starts at +0 never ends at -0)


def _class(case, a):
    return a[:, case.rows_y(), case.rows_x()]


def epilogue(case, inp, acc, dtype=F32, act=None):
    """conv_epi.h on the accumulators acc [N, OH, OW, Cout], per destination: dict(full = the destination tensor
    [N, out_H, out_W, ldc] as it must read afterwards (float32; everything the launch does not own keeps its initial bits),
    stat [2, C] float64 = (sum v, sum v^2 or sum v (x - mean)) over the launch's pixels, statabs [2, C] = the same sums over
    absolute values, or None).  dtype float32: the kernel's own operation order, one rounding per operation; float64: the
    exact epilogue of the precision test."""
    act = case.act if act is None else act
    res, c0 = [], 0
    for d, e in zip(case.dsts, inp["dst"]):
        v = acc[..., c0:c0 + d.C].astype(dtype)
        if inp["bias"] is not None:
            v = v + inp["bias"][c0:c0 + d.C].astype(dtype)
        if act == L.ACT_SIGMOID:
            v = (1 / (1 + np.exp(-v.astype(F64)))).astype(dtype)
        elif act != L.ACT_NONE:
            slope = dtype(0.01 if act == L.ACT_LRELU else 0.0) if dtype is F32 else F64(F32(0.01) if act == L.ACT_LRELU else 0.0)
            v = np.where(v > 0, v, v * slope).astype(dtype)
        ecm = e["cmul"][:, None, None, :d.C].astype(dtype) if e["cmul"] is not None else dtype(1)
        pm = _class(case, inp["pmask"])[..., None].astype(dtype) if inp["pmask"] is not None else dtype(1)
        v = (v * (ecm * pm).astype(dtype)).astype(dtype)
        xr = _class(case, e["relu_x"])[..., :d.C] if e["relu_x"] is not None else None
        if d.relu:
            t = xr
            if e["rs"] is not None:
                t = ((xr * e["rs"]).astype(F32) + e["rt"]).astype(F32)
            v = np.where(t > 0, v, dtype(0)).astype(dtype)
        # (+ old also without accumulate, where old = +0: a -0 -- 0 * a negative sum, ReLU's 0 * v -- leaves as +0)
        old = _class(case, e["out0"])[..., :d.C].astype(dtype) if d.acc else dtype(0)
        v = (v + old).astype(dtype)
        full = None
        if dtype is F32:
            full = e["out0"].copy()
            full[:, case.rows_y(), case.rows_x(), :d.C] = v
        stat = statabs = None
        if d.stat:
            v64 = v.astype(F64)
            second = v64 if d.stat == "sq" else (xr - e["mean"]).astype(F32).astype(F64)
            stat = np.stack([v64.sum((0, 1, 2)), (v64 * second).sum((0, 1, 2))])
            statabs = np.stack([np.abs(v64).sum((0, 1, 2)), np.abs(v64 * second).sum((0, 1, 2))])
        res.append(dict(full=full, v=v, stat=stat, statabs=statabs))
        c0 += d.C
    return res


def integer_outputs(case):
    """every output is an integer on the exact inputs (ACT_NONE, ACT_RELU; cmul 1.25 on multiples of 4): the statistics are
    owed exactly.  LeakyReLU's 0.01 v is a float32 number, not an integer: the float64 fold may round"""
    return case.act in (L.ACT_NONE, L.ACT_RELU)


def exactness(case, inp):
    """the conditions under which bit equality with the float64 reference is OWED in every summation order, as a list of
    violations (empty = they hold):
      1. every transformed operand value and every weight is an integer of at most 8 significant bits -- ONE bf16 plane, so the
         mid and lo planes are zero and the split products lose nothing; bias and the pre-filled output are integers;
      2. S < 2^24 - 2^10 for every output: every partial sum in every order is an integer below 2^24, also with the bias and
         the pre-filled gradient (|.| <= 32 + 8) on top;
      3. the view's scale and shift, ep_relu_scale / shift and the mean are integers or powers of two and x * s + t is exact
         without an fma as with one; cmul (operand and epilogue) is 0 or 1.25 and multiplies multiples of 4; pmask is 0 or 1."""
    bad = []

    def one_plane(a, what):
        a = np.asarray(a, F64)
        if not (np.isfinite(a).all() and (a == np.round(a)).all()):
            bad.append(what + ": not integers")
        elif not (a.astype(F32).astype(F64) == torch.from_numpy(a.astype(F32)).to(torch.bfloat16).double().numpy()).all():
            bad.append(what + ": more than one bf16 plane")
    for i, s in enumerate(case.srcs):
        v, _ = transformed(case, inp, i)
        one_plane(v[..., :case.C_real] if len(case.srcs) == 1 else v, "operand %d" % i)
        cols = min(s.C, s.ldc)
        x = inp["x"][i][..., :cols].astype(F64)
        if inp["scale"][i] is not None:
            sc, sh = inp["scale"][i].astype(F64), inp["shift"][i].astype(F64)
            if not (sc * x == (sc * x).astype(F32)).all() or not (sc * x + sh == (sc * x + sh).astype(F32)).all():
                bad.append("operand %d: the affine map rounds" % i)
            if not np.isin(np.abs(sc), [0.5, 1, 2]).all() or not (sh == np.round(sh)).all():
                bad.append("operand %d: scale / shift off the grid" % i)
        if inp["cmul"][i] is not None:
            if not np.isin(inp["cmul"][i], [0, 1.25]).all():
                bad.append("operand %d: cmul" % i)
            pre = x * inp["scale"][i] + inp["shift"][i] if inp["scale"][i] is not None else x
            if not (pre % 4 == 0).all():
                bad.append("operand %d: cmul multiplies a value that is no multiple of 4" % i)
    one_plane(inp["W"], "weights")
    if len(case.srcs) == 1 and np.any(inp["W"][:, case.C_real:, :] != 0):
        bad.append("weight rows beyond C_real are not zero")
    if inp["bias"] is not None:
        one_plane(inp["bias"], "bias")
    G, S, _ = reference(case, inp)
    if not S.max() < 2 ** 24 - 2 ** 10:
        bad.append("S = %g reaches 2^24" % S.max())
    if inp["pmask"] is not None and not np.isin(inp["pmask"], [0, 1]).all():
        bad.append("pmask")
    c0 = 0
    for k, (d, e) in enumerate(zip(case.dsts, inp["dst"])):
        if d.acc and not (e["out0"][..., :d.C] == np.round(e["out0"][..., :d.C])).all():
            bad.append("dst %d: the pre-filled output is no integer" % k)
        if e["cmul"] is not None:
            if not np.isin(e["cmul"], [0, 1.25]).all() or not (G[..., c0:c0 + d.C] % 4 == 0).all() or case.act != L.ACT_NONE:
                bad.append("dst %d: ep_cmul multiplies a value that is no multiple of 4" % k)
        if e["relu_x"] is not None:
            x = e["relu_x"][..., :d.C].astype(F64)
            if e["rs"] is not None:
                t = x * e["rs"] + e["rt"]
                if not (np.isin(e["rs"], [0.5, 1, 2]).all() and (t == np.round(t)).all()):
                    bad.append("dst %d: ep_relu_scale / shift round" % k)
            if e["mean"] is not None and not ((x - e["mean"]) * 2 == np.round((x - e["mean"]) * 2)).all():
                bad.append("dst %d: x - mean rounds" % k)
        c0 += d.C
    return bad


# ------------------------------------------------------------------------------------------------ weight packs
def wforms(case):
    """the weight forms a case is run with: "f32" always; "s3" (split-bf16 fragments; "stem": pack format 2) where
    pmf_conv_s3_eligible allows"""
    e = L.lib().pmf_conv_s3_eligible(C.byref(host_desc(case, "f32")))
    assert not (e and case.force_s3)
    return ["f32"] + ((["s3"] if case.force_s3 else []) if not e else (["stem"] if e == 3 else ["s3"]))


def packs(case, inp, wform):
    """the whole pack [ntaps][Ktot][ldw] (all Ctot columns; a launch addresses it at its column offset) as an array of 32-bit
    words: fp32, split-bf16 fragments [ntaps][Ktot / 16][ldw / 32][3][64][8] or the stem's format 2"""
    wv = torch.from_numpy(np.ascontiguousarray(inp["W"].transpose(2, 1, 0)))[..., None]       # a virtual OIHW of ntaps x 1
    if wform == "f32":
        return pack_fwd_host(wv, case.Ktot, case.ldw).numpy().view(np.int32).reshape(-1)
    if wform == "stem":
        assert case.Ktot == 8 and case.coloff == 0
        return pack_fwd_s3_stem_host(wv, case.ldw).numpy().reshape(-1).view(np.int32)
    assert case.Ktot % 16 == 0 and case.ldw % 32 == 0 and case.coloff % 32 == 0
    return pack_fwd_s3_host(wv, case.Ktot, case.ldw).numpy().reshape(-1).view(np.int32)


# ------------------------------------------------------------------------------------------------ descriptor
def _ep(e, d, p):
    e.out, e.out_ldc, e.accumulate = p["out"], d.ldc, d.acc
    if d.cmul:
        e.ep_cmul, e.ep_cmul_ld = p["cmul"], d.C + 8
    if d.relu or d.stat == "x_only":
        e.ep_relu_x, e.ep_relu_ldc = p["relu_x"], d.rldc
    if d.relu == "affine":
        e.ep_relu_scale, e.ep_relu_shift = p["rs"], p["rt"]
    if d.stat:
        e.stats = p["stats"]
    if d.stat in ("mean", "x_only"):
        e.ep_stat_mean = p["mean"]
    e.ep_flags = L.EP_STAT_X_ONLY if d.stat == "x_only" else 0


def fill_desc(case, ptr, wform, cfg=0, act=None):
    """pmf_conv_desc_t of `case` over device pointers: ptr = dict(x, scale, shift, cmul = [..] (0 / None: absent), w (the pack's
    first byte), bias, pmask, dst = [dict(out, cmul, relu_x, rs, rt, stats, mean)], ws, ws_bytes, tickets)"""
    d = L.ConvDesc()
    d.N, d.OH, d.OW, d.Cout, d.nsrc = case.N, case.OH, case.OW, case.Cout, len(case.srcs)
    for i, s in enumerate(case.srcs):
        e = d.src[i]
        e.x, e.C, e.ldc, e.H, e.W = ptr["x"][i], s.C, s.ldc, s.H, s.W
        e.scale, e.shift = ptr["scale"][i] or None, ptr["shift"][i] or None
        if ptr["cmul"][i]:
            e.cmul, e.cmul_ld = ptr["cmul"][i], s.C + 8
        e.flags = (L.SRC_RELU if s.relu else 0) | (L.SRC_BCAST if s.bcast else 0)
    d.ntaps = len(case.taps)
    for t, (dy, dx) in enumerate(case.taps):
        d.tdy[t], d.tdx[t] = dy, dx
    d.in_stride, d.gather, d.ldw = case.stride, case.gather, case.ldw
    if wform == "f32":
        d.w = ptr["w"] + 4 * case.coloff
    else:
        d.w_s3 = ptr["w"] + (case.coloff // 32) * 3 * 1024
    d.bias = ptr.get("bias") or None
    d.act = case.act if act is None else act
    d.out_H, d.out_W, d.out_sy, d.out_sx, (d.out_oy, d.out_ox) = case.out_H, case.out_W, case.out_s, case.out_s, case.out_o
    if len(case.dsts) == 1:
        _ep(d, case.dsts[0], ptr["dst"][0])
    else:
        d.ndst = len(case.dsts)
        d.out, d.out_ldc = ptr["dst"][0]["out"], case.dsts[0].ldc
        for k, dd in enumerate(case.dsts):
            d.dst[k].C = dd.C
            _ep(d.dst[k], dd, ptr["dst"][k])
    d.ep_pmask = ptr.get("pmask") or None
    d.splitk_ws, d.splitk_ws_bytes = ptr.get("ws") or None, ptr.get("ws_bytes") or 0
    d.splitk_tickets = ptr.get("tickets") or None
    d.cfg = cfg
    return d


def host_desc(case, wform, cfg=0, ws_bytes=0, tickets=False):
    """the descriptor over made-up non-null pointers: for the host-side queries and the refusals, which launch nothing"""
    ptr = dict(x=[FAKE] * len(case.srcs), scale=[FAKE if s.aff else 0 for s in case.srcs],
               shift=[FAKE if s.aff else 0 for s in case.srcs], cmul=[FAKE if s.cmul else 0 for s in case.srcs], w=FAKE,
               bias=FAKE if case.bias else 0, pmask=FAKE if case.pmask else 0,
               dst=[dict(out=FAKE, cmul=FAKE, relu_x=FAKE, rs=FAKE, rt=FAKE, stats=FAKE, mean=FAKE) for _ in case.dsts],
               ws=FAKE if ws_bytes else 0, ws_bytes=ws_bytes, tickets=FAKE if tickets else 0)
    return fill_desc(case, ptr, wform, cfg)


def variant(d):
    """(family or negative return code, [BN, MT, K splits, combine, stat rows, K stages, LDS, grid x, y, z, NCO, A-slab form])"""
    info = (C.c_int32 * 12)()
    fam = L.lib().pmf_conv_fwd_variant(C.byref(d), C.cast(info, C.c_void_p))
    return fam, list(info)


def slab_bytes(case):
    """one partial slab of a K split (conv_epi.h: [N][OH][OW][Cout rounded up to 4] float32 per split)"""
    return case.npix * ru(case.Cout, 4) * 4


def pick(case, wform, cfg, tickets):
    """(family, BN, MT, K splits, combine form, statistics rows, workspace bytes, ticket entries) of a launch whose K-split
    workspace is exactly as large as the split count it would choose with room to spare"""
    fam, info = variant(host_desc(case, wform, cfg, 1 << 40, tickets))
    ks = info[2]
    need = ks * slab_bytes(case) if ks > 1 else 0
    return dict(family=fam, BN=info[0], MT=info[1], ksplit=ks, combine=info[3], rows=info[4], ws_bytes=need,
                tickets=info[7] * info[9] * (info[8] // max(ks, 1)), nco=info[10], lds=info[6])


# ------------------------------------------------------------------------------------------------ the launches of the GPU file
TILES = [tile(32, 1), tile(64, 1), tile(32, 2), tile(64, 2)]
SPLITS = [tile(32, 1, 4), tile(64, 2, 2), tile(64, 1, 8)]
WS_CFGS = [L.CFG_WS | (code << 26) | tile(32, 1) for code in (0, 1, 2, 3)]


def launches(case):
    """[(weights form, cfg, K-split workspace given)] of one case: cfg 0 and the four tiles without a workspace; three K-split
    requests with one (kept where the library does split); on split-bf16 weights the direct-taps bit on two tiles and the
    wave-scheduled kernel with NCO 1, 2, 4 (cfg bits 26 and 27) -- each kept where it changes the kernel.  Environment
    switches select nothing here: cfg, w against w_s3 and the ticket pointer do."""
    out = []
    for wf in wforms(case):
        seen = set()
        cand = [(c, False) for c in [0] + TILES] + [(c, True) for c in SPLITS]
        if wf == "s3":
            cand += [(tile(32, 1) | L.CFG_DIRECT_TAPS, False), (tile(64, 2) | L.CFG_DIRECT_TAPS, False)]
            cand += [(c, False) for c in WS_CFGS]
        for cfg, split in cand:
            p = pick(case, wf, cfg, False) if split else variant(host_desc(case, wf, cfg))
            key = (p["family"], p["BN"], p["MT"], p["ksplit"], p["nco"]) if split else (p[0], p[1][0], p[1][1], 1, p[1][10])
            if key[0] < 0 or (split and p["ksplit"] < 2) or (key in seen and cfg != 0):
                continue
            seen.add(key)
            out.append((wf, cfg, split))
    return out


def launch_table():
    """{"case/form/cfg/split": [family, BN, MT, K splits, combine form with a ticket array, combine form without, dynamic LDS
    bytes (the one-tap direct kernel: resident fragments or streamed chunks), NCO of the wave-scheduled kernel]}"""
    tab = {}
    for c in CASES:
        for wf, cfg, split in launches(c):
            if split:
                a, b = pick(c, wf, cfg, True), pick(c, wf, cfg, False)
                row = [a["family"], a["BN"], a["MT"], a["ksplit"], a["combine"], b["combine"], a["lds"]]
            else:
                fam, info = variant(host_desc(c, wf, cfg))
                row = [fam, info[0], info[1], info[2], info[3], info[3], info[6]]
            tab["%s/%s/%#x/%d" % (c.name, wf, cfg, split)] = row + ([pick(c, wf, cfg, False)["nco"]] if row[0] == 100 else [])
    return tab


if __name__ == "__main__":          # python -m tests.conv_cases OUT.json: the table of the library built in the tree
    import json
    import sys
    with open(sys.argv[1], "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in launch_table().items()))
