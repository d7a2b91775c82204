"""Weight-gradient cases for tests/test_wgrad_reference_host.py and tests/test_gpu_wgrad.py (host only: numpy, ctypes).

  * reference(): a float64 restatement of the formula of pmf_wgrad_desc_t (include/pmf_amd.h), straight from a descriptor-shaped
    case -- not autograd:
        dW[co, k, tap_widx[t]] (+)= sum_{n,oy,ox} in_t(n, oy*s + tdy[t], ox*s + tdx[t], k) * dz[n, oy, ox, co]
    in_t = the operand transform of pmf_src_t (scale / shift evaluated in float32 like every kernel does, then PMF_SRC_RELU, then
    cmul; zero outside the map AFTER the transform; PMF_SRC_BCAST), k over the concatenated operands; next to it the abs-sum
    S[co, k, t] = sum |in_t| * |dz| and dbias[co] = sum_r rows[r][co].  mag_sum(): sum mag_t * |dz| with mag_t = (|x * scale| +
    |shift|) * cmul, the one place it is used is the fma allowance of the worst-case bound (a kernel may contract the affine map
    into one fma, which moves in_t by eps32 * mag_t at most, also where the ReLU leaves |in_t| = 0).
  * fill_desc(): ONE descriptor builder over device pointers (several operands, transforms, stride, gather, pitches ldc > C and
    dz_ldc > Cout, Cin_real < C, tap subsets, dbias rows).
  * CASES: the smallest shapes at which each kernel family of conv_wgrad.hip can still go wrong, with the family expected under
    PMF_WGRAD_S3 set / clear and the environments of WGRAD_VARIANT_ENVS; instantiation() restates wg_pick()'s template
    parameters (KG, NCO, RAG, XSL, NT).
  * inputs(): "exact" inputs on which no summation order can round (see exactness()), "random" full-mantissa inputs in the
    det_tensor ranges of tests/test_gpu_ops.py::_conv_case, and the two one-hot forms."""
import ctypes as C
import zlib

import numpy as np

from pmf_amd import _lib as L
from tests.gpu_helpers import taps_of

F32, F64 = np.float32, np.float64
ENVS = {"default": {}, "swp_pixel_split": {"PMF_WG_S3N": "0"}, "nsplit_two_tiles": {"PMF_WG_S3N": "2"}}   # = WGRAD_VARIANT_ENVS
FAM = {"UNIT": 0, "PIPE": 1, "SWP": 3, "NSPLIT": 5, "DIRECT": 6, "DIRECT_S3": 7, "STREAM": 8, "FEWC": 9}   # = PMF_WG_*
FAM_NAME = {v: k for k, v in FAM.items()}
LSB = 1.0 / 16          # least significant bit of every product of the exact inputs (operand: 1/4, dz: 1/4)


class Src:
    def __init__(self, C_, H, W, ldc=None, aff=False, relu=False, cmul=False, bcast=False):
        self.C, self.H, self.W, self.ldc = C_, H, W, ldc or C_
        self.aff, self.relu, self.cmul, self.bcast = aff, relu, cmul, bcast


class Case:
    """one descriptor shape.  fam: {(s3, env name): family name}."""

    def __init__(self, name, N, OH, OW, srcs, Cout, taps, KHW, widx=None, stride=1, gather=0, dz_ldc=None, Cin_real=None,
                 fam=None, conv=None, dbias=False):
        self.name, self.N, self.OH, self.OW, self.srcs, self.Cout = name, N, OH, OW, srcs, Cout
        self.taps, self.KHW, self.widx = list(taps), KHW, list(widx if widx is not None else range(len(taps)))
        self.stride, self.gather = stride, gather
        self.dz_ldc = dz_ldc or Cout
        self.Ktot = sum(s.C for s in srcs)
        self.Cin_real = Cin_real or self.Ktot
        self.fam = fam or {}
        self.conv = conv                    # (k, dil, pad) when the case is an ordinary nn.Conv2d
        self.dbias = dbias                  # the case carries dbias rows (dbias_ld > Cout)
        self.dbias_nrows, self.dbias_ld = 5, (Cout + 3) // 4 * 4 + 4

    @property
    def npix(self):
        return self.N * self.OH * self.OW

    def tap_subset(self):
        """the same case without the taps of the LAST window row and the FIRST window column; tap_widx from the full window"""
        k = self.conv[0]
        keep = [i for i in range(k * k) if i // k != k - 1 and i % k != 0]
        c = Case(self.name + ".sub", self.N, self.OH, self.OW, self.srcs, self.Cout, [self.taps[i] for i in keep], self.KHW,
                 keep, self.stride, self.gather, self.dz_ldc, self.Cin_real, None, None, self.dbias)
        c.dropped = [i for i in range(k * k) if i not in keep]
        return c


def conv(name, N, H, W, cins, Cout, k, dil=1, stride=1, gather=0, dz_ldc=None, Cin_real=None, raw=False, bcast=(), ldc_pad=0,
         fam=None, dbias=False, variant=0):
    """an ordinary convolution (`same` padding; k = 2: dilation 2, padding 1 -- the 2x2 d2 layers of the network).  Operand i
    gets scale / shift unless raw, ReLU on every other operand, cmul on the first operand of every other case."""
    pad = 1 if k == 2 else dil * (k - 1) // 2
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    srcs = []
    for i, c in enumerate(cins):
        b = i in bcast
        srcs.append(Src(c, 1 if b else H, 1 if b else W, c + ldc_pad, aff=not raw, relu=(not raw) and (i + variant) % 2 == 1,
                        cmul=(not raw) and i == 0 and variant % 2 == 0, bcast=b))
    return Case(name, N, OH, OW, srcs, Cout, taps_of(k, k, dil, pad), k * k, None, stride, gather, dz_ldc, Cin_real, fam,
                (k, dil, pad), dbias)


def _all(s3, f32, swp=None, two=None):
    """family table: S3 set / clear under the default environment; S3 set under PMF_WG_S3N=0 / =2 (default: as `s3`).  With the
    flag clear no environment of ENVS changes the selection."""
    f = {(1, "default"): s3, (0, "default"): f32, (1, "swp_pixel_split"): swp or s3, (1, "nsplit_two_tiles"): two or s3}
    f[(0, "swp_pixel_split")] = f[(0, "nsplit_two_tiles")] = f32
    return f


def _cases():
    out = []
    # ---- WG_FEWC: <= 4 real input channels of one raw 8-channel operand, >= 9 taps, full tiles, Cout % 64 == 0
    fe = _all("FEWC", "FEWC")
    out += [conv("fewc_3x3_c3", 1, 8, 64, [8], 64, 3, Cin_real=3, raw=True, fam=fe),              # 27 rows: KG 1
            conv("fewc_3x3_c4", 1, 8, 64, [8], 64, 3, Cin_real=4, raw=True, fam=fe),              # 36: KG 2
            conv("fewc_5x5_c3", 1, 8, 64, [8], 64, 5, Cin_real=3, raw=True, fam=fe),              # 75: KG 3
            conv("fewc_7x7_c3", 1, 8, 64, [8], 64, 7, Cin_real=3, raw=True, fam=fe, dbias=True),  # 147 of 160: KG 5, zero-word rows
            conv("fewc_5x5_c4_2pairs", 2, 12, 32, [8], 128, 5, Cin_real=4, raw=True, fam=fe)]     # 100 -> four row tiles run as KG 5
    # ---- WG_UNIT
    un = _all("UNIT", "UNIT")
    out += [conv("unit_1x1_32_20", 2, 16, 72, [32], 20, 1, dz_ldc=24, fam=un, dbias=True),          # U = 1: rows dealt to the waves
            conv("unit_1x1_32_64", 2, 16, 72, [32], 64, 1, fam=un, variant=1),                     # U = 2
            conv("unit_1x1_32_128", 1, 12, 40, [32], 128, 1, fam=un),                              # NT = 4
            conv("unit_3x3d18_gather", 1, 20, 40, [24], 40, 3, dil=18, gather=1, Cin_real=21, fam=un, variant=1),
            conv("unit_3x3_s2_odd", 1, 15, 33, [32], 64, 3, stride=2, fam=un),
            conv("unit_1x1_s2_odd", 1, 63, 131, [32], 64, 1, stride=2, ldc_pad=4, fam=un, variant=1),
            conv("unit_7x7_c8", 1, 8, 40, [8], 32, 7, fam=un),                                     # ragged last tap batch (49 = 5 x 9 + 4)
            conv("unit_3x3_bcast", 2, 10, 40, [32, 32], 32, 3, bcast=(0,), fam=un)]
    # ---- WG_PIPE / WG_SWP / WG_NSPLIT: 3x3, 3x3 d2, 2x2 d2
    for kn, k, dil in (("3x3", 3, 1), ("3x3d2", 3, 2), ("2x2d2", 2, 2)):
        v = len(kn)
        full = [("64_64", [64], 64, _all("NSPLIT", "PIPE", "SWP")), ("64_128", [64], 128, _all("NSPLIT", "PIPE", "SWP")),
                ("32+16_256", [32, 16], 256, _all("NSPLIT", "UNIT", "SWP"))]
        for cn, cins, co, fam in full:
            out.append(conv("tile_%s_%s_8x64" % (kn, cn), 2 if co == 64 else 1, 8, 64, cins, co, k, dil, fam=fam, variant=v,
                            dbias=(cn == "64_128" and k == 2)))
        rag = _all("NSPLIT", "UNIT", "UNIT")
        out += [conv("tile_%s_32_32_30x40" % kn, 1, 30, 40, [32], 32, k, dil, fam=rag, variant=v),
                conv("tile_%s_64_64_15x80" % kn, 2, 15, 80, [64], 64, k, dil, fam=rag, variant=v + 1),
                conv("tile_%s_32_128_5x33" % kn, 1, 5, 33, [32], 128, k, dil, ldc_pad=8, fam=rag, variant=v),
                conv("tile_%s_16_20_8x64" % kn, 1, 8, 64, [16], 20, k, dil, dz_ldc=24, fam=_all("NSPLIT", "UNIT", "UNIT"), variant=v),
                conv("tile_%s_8_32_8x64" % kn, 1, 8, 64, [8], 32, k, dil, Cin_real=5, fam=_all("NSPLIT", "UNIT", "UNIT"), variant=v + 1)]
    # a one-tap layer on full tiles runs the pipelined kernels with TB = 1 (and never the N-split form)
    out.append(conv("tile_1x1_32_64_8x64", 1, 8, 64, [32], 64, 1, fam=_all("SWP", "PIPE")))
    # ---- WG_DIRECT (fp32): >= 16384 pixels, Ktot >= 96; 129 x 129 = 16641 pixels: odd, and a ragged last 16-pixel group
    out += [conv("direct_96_32", 1, 129, 129, [96], 32, 1, fam=_all("DIRECT", "DIRECT"), variant=1),
            conv("direct_128_20", 1, 129, 129, [128], 20, 1, dz_ldc=24, Cin_real=125, fam=_all("DIRECT", "DIRECT")),
            conv("direct_64+128_80", 1, 129, 129, [64, 128], 80, 1, dz_ldc=88, fam=_all("DIRECT_S3", "DIRECT"))]
    # ---- WG_DIRECT_S3: Cout >= 64, operands multiples of 64 channels, >= 4096 pixels (or >= 1024 with Ktot >= 512)
    out += [conv("ds3_64_64_floor", 2, 32, 64, [64], 64, 1, fam=_all("DIRECT_S3", "PIPE"), variant=1),
            conv("ds3_512_64", 1, 32, 32, [512], 64, 1, fam=_all("DIRECT_S3", "PIPE")),
            conv("ds3_64+128_80_odd", 1, 65, 65, [64, 128], 80, 1, dz_ldc=84, fam=_all("DIRECT_S3", "UNIT")),   # 4225 pixels
            # (65 x 63 = 4095 pixels is ONE below the selector's floor: the unit-dealing kernel with four output tiles)
            conv("unit_64+128_80_below_floor", 1, 65, 63, [64, 128], 80, 1, dz_ldc=84, fam=_all("UNIT", "UNIT")),
            conv("ds3_64_128_s2", 2, 64, 128, [64], 128, 1, stride=2, fam=_all("DIRECT_S3", "UNIT"), variant=1, dbias=True)]
    # ---- WG_STREAM: one tap, Ktot <= 96, Cout <= 64, >= 32768 pixels
    stf = _all("STREAM", "STREAM")
    out += [conv("stream_32_20", 2, 64, 256, [32], 20, 1, dz_ldc=24, fam=stf),
            conv("stream_64+16_16_odd", 1, 129, 257, [64, 16], 16, 1, fam=stf, variant=1),
            conv("stream_3x32_32", 2, 128, 129, [32, 32, 32], 32, 1, fam=stf),                      # KT 3
            conv("stream_8_64", 2, 64, 256, [8], 64, 1, Cin_real=5, fam=stf, variant=1)]           # NTL 2
    # ---- stage 2, tiled form (kind 1: ntaps * Ktot * Cout32 >= 131072, nsplit <= 32); the flat form (kind 0) serves the rest
    out += [conv("red_tile_256_256", 2, 4, 16, [256], 256, 3, fam=_all("NSPLIT", "UNIT", "UNIT")),
            conv("red_tile_250_200", 2, 4, 16, [256], 200, 3, Cin_real=250, fam=_all("NSPLIT", "UNIT", "UNIT"), variant=1, dbias=True)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SUBSET_CASES = ["fewc_5x5_c3", "unit_3x3_s2_odd", "tile_3x3_64_64_8x64", "tile_3x3d2_32_32_30x40", "red_tile_250_200"]
RED_MULTI = ["red_tile_256_256", "red_tile_250_200", "unit_1x1_32_20", "tile_2x2d2_64_128_8x64", "fewc_7x7_c3"]
PRECISION = ["fewc_7x7_c3", "unit_3x3_s2_odd", "tile_3x3_64_64_8x64", "tile_3x3d2_64_64_15x80", "tile_2x2d2_32+16_256_8x64",
             "direct_64+128_80", "ds3_512_64", "ds3_64_128_s2", "stream_3x32_32"]


# ------------------------------------------------------------------------------------------------ wg_pick()'s template parameters
def instantiation(case, s3, env="default"):
    """restates wg_pick() of conv_wgrad.hip for the parameters pmf_conv_wgrad_variant does not export: a dict with the family
    name and, per family, KG (few-channel), NT (unit-dealing), NCO / RAG / XSL (N-split), XSL (pipelined)"""
    fam = case.fam[(s3, env)]
    r = {"family": fam}
    dys, dxs = [t[0] for t in case.taps], [t[1] for t in case.taps]
    if fam == "FEWC":
        kg = -(-len(case.taps) * case.Cin_real // 32)
        r["KG"] = kg if kg <= 3 else 5
    if fam in ("PIPE", "SWP", "NSPLIT"):
        slots = (4 + max(dys) - min(dys)) * (32 + max(dxs) - min(dxs)) * 8
        r["XSL"] = 7 if slots <= 256 * 7 else 9
    if fam == "NSPLIT":
        mode = int(ENVS[env].get("PMF_WG_S3N", "4"))
        r["NCO"] = 1 if case.Cout % 32 else (4 if mode >= 4 and case.Cout % 128 == 0 else (2 if case.Cout % 64 == 0 else 1))
        r["RAG"] = bool(case.OH % 4 or case.OW % 32)
    if fam == "UNIT":
        wide = len(case.taps) == 1 and case.Cout > 64
        r["NT"] = 4 if wide else (2 if case.Cout > 32 else 1)
        # (NT = 1 is also what a descriptor gets whose pipelined conditions hold: none of the UNIT rows of the table does)
    return r


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case, mode, salt=0):
    return np.random.RandomState(zlib.crc32(("%s/%s/%d" % (case.name, mode, salt)).encode()) & 0x7FFFFFFF)


def special_pixels(case, nsplit):
    """flat pixel indices (n, oy, ox row-major) where a kernel can lose a pixel: the four corners of the first sample, the last
    pixel of the last sample, both sides of the 4 x 32 tile seams, the ragged remainder, and the first / last pixel of a split
    (contiguous pixel-pair ranges in the direct fp32 kernel, 16-pixel groups in the direct split-bf16 kernel, per-sample pair
    ranges in the streaming kernel; the tiled kernels deal whole tiles: their seams are the tile seams)"""
    N, OH, OW = case.N, case.OH, case.OW
    hw = OH * OW
    px = {0, OW - 1, (OH - 1) * OW, hw - 1, N * hw - 1, (N - 1) * hw}
    for y in (3, 4, OH - 1, OH - OH % 4 - 1, OH - OH % 4):
        for x in (31, 32, OW - 1, OW - OW % 32 - 1, OW - OW % 32):
            if 0 <= y < OH and 0 <= x < OW:
                px.add(y * OW + x)
                px.add((N - 1) * hw + y * OW + x)
    npix = N * hw
    ns = max(nsplit, 1)
    per_pair = -(-((npix + 1) // 2) // ns) * 2
    per_grp = -(-((npix + 15) // 16) // ns) * 16
    S = max(ns // N, 1)
    per_str = -(-((hw + 1) // 2) // S) * 2
    for b in (per_pair, per_grp, per_str, (N - 1) * hw + per_str):
        for p in (b - 1, b, b + 1):
            if 0 <= p < npix:
                px.add(p)
    return sorted(px)


def inputs(case, mode, nsplit=1):
    """dict(x=[N,H,W,ldc] per operand with NaN in the pitch padding -- and in the channels [Cin_real, C) of a single operand --,
    scale / shift [C] or None, cmul [N, cmul_ld] or None, dz [N,OH,OW,dz_ldc] with NaN in [Cout, dz_ldc), rows [nrows, dbias_ld],
    dw0 / db0: pre-filled gradient and bias gradient).
    mode "exact": operands integers in [-4, 4] (even under scale 0.5), scale in {0.5, 1, 2}, shift an integer in [-2, 2], cmul in
    {0, 1.25}: every transformed value is a multiple of 1/4 below 2^8 quarters; dz a multiple of 1/4 in [-2, 2].
    mode "random": det_tensor's ranges in _conv_case (x, dz in [-1, 1), scale in [0.5, 1.5), shift in [-0.5, 0.5), cmul {0, 1.25}).
    mode "onehot_dz": dz zero but for ONE pixel per output channel (special_pixels, a power of two), operands random without
    scale / shift; "onehot_x": one pixel per input channel holds a power of two, dz random."""
    g = _rng(case, mode)
    N = case.N
    exact = mode == "exact"
    xs, scs, shs, cms = [], [], [], []
    for i, s in enumerate(case.srcs):
        shape = (N, s.H, s.W, s.C)
        aff = s.aff and mode in ("exact", "random")
        if exact:
            sc = g.choice([0.5, 1.0, 2.0], s.C).astype(F32)
            sh = g.randint(-2, 3, s.C).astype(F32)
            v = g.randint(-4, 5, shape).astype(F32)
            if aff:
                v = np.where(sc == 0.5, np.trunc(v / 2) * 2, v).astype(F32)
        else:
            sc = g.uniform(0.5, 1.5, s.C).astype(F32)
            sh = g.uniform(-0.5, 0.5, s.C).astype(F32)
            v = g.uniform(-1, 1, shape).astype(F32)
        if mode == "onehot_x":
            v = np.zeros(shape, F32)
            sp = special_pixels(Case("x", N, s.H, s.W, [], 1, [], 1), nsplit)
            for c in range(s.C):
                p = sp[(c * 5 + i) % len(sp)]
                v.reshape(N * s.H * s.W, s.C)[p, c] = 2.0 ** ((c % 5) - 2) * (1 if s.relu else (-1) ** c)
        x = np.full((N, s.H, s.W, s.ldc), np.nan, F32)
        x[..., :s.C] = v
        if len(case.srcs) == 1 and case.Cin_real < s.C:
            x[..., case.Cin_real:] = np.nan
        xs.append(x)
        scs.append(sc if aff else None)
        shs.append(sh if aff else None)
        # (one-hot operands: no multiplier -- 1.25 x a 24-bit dz is no float32 number)
        cms.append((g.rand(N, s.C + 8) > 0.25).astype(F32) * F32(1.25) if s.cmul and mode != "onehot_x" else None)
    dz = np.full((N, case.OH, case.OW, case.dz_ldc), np.nan, F32)
    if exact:
        z = g.randint(-8, 9, (N, case.OH, case.OW, case.Cout)).astype(F32) / 4
    elif mode == "onehot_dz":
        z = np.zeros((N, case.OH, case.OW, case.Cout), F32)
        sp = special_pixels(case, nsplit)
        for co in range(case.Cout):
            z.reshape(case.npix, case.Cout)[sp[co % len(sp)], co] = 2.0 ** ((co % 5) - 2) * (-1) ** co
    else:
        z = g.uniform(-1, 1, (N, case.OH, case.OW, case.Cout)).astype(F32)
    dz[..., :case.Cout] = z
    rows = np.full((case.dbias_nrows, case.dbias_ld), np.nan, F32)
    rows[:, :case.Cout] = g.randint(-8, 9, (case.dbias_nrows, case.Cout)) / 4 if exact else g.uniform(-1, 1, (case.dbias_nrows, case.Cout))
    dw0 = g.randint(-8, 9, (case.Cout, case.Cin_real, case.KHW)).astype(F32)
    db0 = g.randint(-8, 9, case.Cout).astype(F32)
    return dict(x=xs, scale=scs, shift=shs, cmul=cms, dz=dz, rows=rows, dw0=dw0, db0=db0)


# ------------------------------------------------------------------------------------------------ float64 reference
def transformed(case, inp, i):
    """(in, mag) of operand i as float64 [N, H', W', C]: the transform of pmf_src_t with the affine map evaluated in float32;
    a PMF_SRC_BCAST operand is expanded to the (OH * stride) x (OW * stride) map the kernels give it"""
    s = case.srcs[i]
    x = inp["x"][i][..., :s.C]
    if inp["scale"][i] is not None:
        v = (x * inp["scale"][i]).astype(F32) + inp["shift"][i]                     # float32, as the kernels evaluate it
        mag = np.abs(x.astype(F64) * inp["scale"][i]) + np.abs(inp["shift"][i].astype(F64))
    else:
        v, mag = x, np.abs(x.astype(F64))
    if s.relu:
        v = np.maximum(v, F32(0))
    if inp["cmul"][i] is not None:
        cm = inp["cmul"][i][:, None, None, :s.C]
        v, mag = (v * cm).astype(F32), mag * cm.astype(F64)                         # (one float32 product, like the kernels)
    v = v.astype(F64)
    if s.bcast:
        sh = (case.N, case.OH * case.stride, case.OW * case.stride, s.C)
        v, mag = np.broadcast_to(v, sh), np.broadcast_to(mag, sh)
    return v, mag


def tap_view(a, case, dy, dx):
    """a[n, oy*s + dy, ox*s + dx, :] for every output pixel, zero outside the map"""
    N, H, W, C_ = a.shape
    s = case.stride
    out = np.zeros((N, case.OH, case.OW, C_), F64)
    oy, ox = np.arange(case.OH) * s + dy, np.arange(case.OW) * s + dx
    my, mx = (oy >= 0) & (oy < H), (ox >= 0) & (ox < W)
    if my.any() and mx.any():
        out[:, np.nonzero(my)[0][:, None], np.nonzero(mx)[0][None, :], :] = a[:, oy[my][:, None], ox[mx][None, :], :]
    return out


def reference(case, inp, dtype=F64):
    """(dW [Cout, Cin_real, KHW] with NaN where no tap writes, S [Cout, Cin_real, ntaps], dbias [Cout]); dtype float32: the
    same sum evaluated in float32 (the fp32 CPU yardstick of the precision test)"""
    tr = [transformed(case, inp, i) for i in range(len(case.srcs))]
    dz = inp["dz"][..., :case.Cout].astype(F64).reshape(-1, case.Cout)
    dw = np.full((case.Cout, case.Cin_real, case.KHW), np.nan, F64)
    S = np.zeros((case.Cout, case.Cin_real, len(case.taps)), F64)
    for t, (dy, dx) in enumerate(case.taps):
        a = np.concatenate([tap_view(v, case, dy, dx) for v, _ in tr], -1).reshape(-1, case.Ktot)[:, :case.Cin_real]
        if dtype is F64:
            dw[:, :, case.widx[t]] = dz.T @ a
        else:
            dw[:, :, case.widx[t]] = (dz.astype(F32).T @ a.astype(F32)).astype(F64)
        S[:, :, t] = np.abs(dz).T @ np.abs(a)
    dbias = inp["rows"][:, :case.Cout].astype(F64).sum(0)
    return dw, S, dbias


def mag_sum(case, inp):
    """sum_pixels mag_t * |dz| [Cout, Cin_real, ntaps], mag_t = (|x * scale| + |shift|) * cmul taken BEFORE the ReLU: what an
    fma in place of the reference's float32 product and sum can move in_t by, in units of eps32"""
    tr = [transformed(case, inp, i)[1] for i in range(len(case.srcs))]
    dz = np.abs(inp["dz"][..., :case.Cout].astype(F64)).reshape(-1, case.Cout)
    M = np.zeros((case.Cout, case.Cin_real, len(case.taps)), F64)
    for t, (dy, dx) in enumerate(case.taps):
        m = np.concatenate([tap_view(mg, case, dy, dx) for mg in tr], -1).reshape(-1, case.Ktot)[:, :case.Cin_real]
        M[:, :, t] = dz.T @ m
    return M


def exactness(case, inp):
    """the two conditions under which bit equality with the float64 reference is OWED in every summation order, as a list of
    violations (empty = they hold):
      1. every transformed operand value and every dz value is a multiple of 1/4 with at most 8 significant bits -- ONE bf16
         plane, so the split products lose nothing and every product is a multiple of LSB = 1/16;
      2. S / LSB < 2^24 for every weight: every partial sum in every order is an integer below 2^24 in units of LSB, hence a
         float32 number."""
    bad = []
    for i in range(len(case.srcs)):
        v, _ = transformed(case, inp, i)
        v = v[..., :case.Cin_real] if len(case.srcs) == 1 else v
        q = v * 4
        if not (np.isfinite(q).all() and (q == np.round(q)).all() and np.abs(q).max() < 256):
            bad.append("operand %d is not on the quarter grid below 2^8" % i)
        if inp["scale"][i] is not None:          # the float32 affine map itself is exact: an fma and mul + add agree
            x = inp["x"][i][..., :case.srcs[i].C].astype(F64)
            e = x * inp["scale"][i].astype(F64) + inp["shift"][i].astype(F64)
            if not (np.nan_to_num(e) == np.nan_to_num(e.astype(F32).astype(F64))).all():
                bad.append("operand %d: the affine map rounds" % i)
    z = inp["dz"][..., :case.Cout].astype(F64) * 4
    if not ((z == np.round(z)).all() and np.abs(z).max() < 256):
        bad.append("dz is not on the quarter grid")
    _, S, _ = reference(case, inp)
    if not S.max() / LSB + 16 * 16 < 2 ** 24:      # (+ the pre-filled gradient of the accumulate variant, |dw0| <= 8)
        bad.append("S = %g LSB reaches 2^24" % (S.max() / LSB))
    return bad


# ------------------------------------------------------------------------------------------------ descriptor
def fill_desc(case, ptr, s3, nsplit=1, accumulate=0, dbias=False):
    """pmf_wgrad_desc_t of `case` over device pointers: ptr = dict(x=[..], scale=[..], shift=[..], cmul=[..] (0 / None: absent),
    dz, partial, dw, rows, db)"""
    d = L.WgradDesc()
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
        d.tdy[t], d.tdx[t], d.tap_widx[t] = dy, dx, case.widx[t]
    d.in_stride, d.gather = case.stride, case.gather
    d.dz, d.dz_ldc = ptr["dz"], case.dz_ldc
    d.partial, d.nsplit, d.dw_oihw = ptr["partial"], nsplit, ptr["dw"]
    d.Cin_real, d.KHW, d.accumulate = case.Cin_real, case.KHW, accumulate
    if dbias:
        d.dbias_rows, d.dbias_nrows, d.dbias_ld, d.dbias_out = ptr["rows"], case.dbias_nrows, case.dbias_ld, ptr["db"]
    d.flags = L.WGRAD_S3 if s3 else 0
    return d


def host_desc(case, s3, nsplit=1, dbias=False, transforms=True):
    """the descriptor over made-up non-null pointers: for the host-side queries and the guards, which launch nothing"""
    fake = 0x10000
    n = len(case.srcs)
    ptr = dict(x=[fake] * n, scale=[fake if (s.aff and transforms) else 0 for s in case.srcs],
               shift=[fake if (s.aff and transforms) else 0 for s in case.srcs],
               cmul=[fake if (s.cmul and transforms) else 0 for s in case.srcs], dz=fake, partial=fake, dw=fake, rows=fake, db=fake)
    return fill_desc(case, ptr, s3, nsplit, 0, dbias)


def default_nsplit(case, s3):
    lib = L.lib()
    return lib.pmf_conv_wgrad_nsplit(C.byref(host_desc(case, s3)))


def pixel_tiles(case):
    return -(-case.OH // 4) * -(-case.OW // 32) * case.N


def empty_split_count(case, s3, fam):
    """a split count with splits that get no pixel at all (every family writes such a slab as zeros: the tile / pair / group
    loops of conv_wgrad.hip start beyond their end and the accumulators are stored as they were cleared).  The streaming
    kernel needs a multiple of N."""
    if fam in ("DIRECT", "STREAM", "DIRECT_S3"):
        # contiguous ranges of per = ceil(units / n) units (pixel pairs; 16-pixel groups; pixel pairs of ONE sample): the
        # smallest n whose last range starts at or beyond the end, (n - 1) * per >= units -- about sqrt(units)
        units = {"DIRECT": (case.npix + 1) // 2, "DIRECT_S3": (case.npix + 15) // 16, "STREAM": (case.OH * case.OW + 1) // 2}[fam]
        n = 2
        while (n - 1) * -(-units // n) < units:
            n += 1
        return n * case.N if fam == "STREAM" else n
    return pixel_tiles(case) + 3
