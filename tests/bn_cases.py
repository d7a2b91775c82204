"""CPU side of tests/test_gpu_bn.py and tests/test_bn_reference_host.py: input builders, the float64 references of the
BatchNorm backward and of the statistics finalisation (csrc/bn.hip), the float32 restatement of the kernels' coefficient
form, the rounding counts (table ``K``) and the case lists.  Nothing here touches the GPU or the built library, except the
double-precision guarded buffer DBuf, which the GPU tests alone construct.

Layer order is conv -> act -> BatchNorm: ``a = act(z)`` is what BatchNorm normalises, ``gy`` the gradient of its output and
``dz = dL/dz`` what the kernels write.  The slope of act is taken from the sign of ``a`` (a > 0 ? 1 : slope), so 0.0 and -0.0
are on the non-positive branch."""
import math

import torch
import torch.nn.functional as F

from pmf_amd import _lib as L
from tests.test_gpu_elementwise import BAND, DEV, EPS, SENT, gen, rnd

EPS64 = float(torch.finfo(torch.float64).eps)
SENT64 = (0x7FF8BEEF << 32) | SENT                 # a quiet float64 NaN with a payload
BN_EPS = 1e-5
COL_CAP = 512                                      # PMF_COL_ROWS (csrc/common.h); the GPU tests hold it to pmf_debug_col(0, 0)
HARD = 1                                           # index of the hard channel
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU)
COMBOS = [(act, train) for train in (1, 0) for act in ACTS]

# what measure_restate_units() / measure_chain_units() return on the CPU, worst element in units of eps32 * mag_dz;
# tests/test_bn_reference_host.py holds these figures to the helpers
MEASURED = {
    "restate": 1.49,
    "chain": 41.36,
}

# K = 2 * (float32 roundings on the longest path to one output).  save_mean, save_invstd, gamma and gy are inputs (exact).
# Sums that a kernel accumulates in float64 and casts once count from the cast; f64_floor() adds the float64 sum itself.
R_COEF1 = 6     # x - mean per term, the cast of the sum, r * sgc, r * dgam, 1/npix (npix < 2^24 is exact), * invM
R_DZ = R_COEF1 + 1 + 1 + 1 + 2 + 2    # ... (x - MU) and its product with K, the outer subtraction, A = g*r and the product
#                                       with it, the slope 0.01f (a rounded constant) and the product with it: 13
K = {
    "coef0": 2 * 1,                   # gamma * r
    "coef1": 2 * R_COEF1,
    "coef2": 2 * 3,                   # the cast of the sum, 1/npix, the product
    "dgamma": 2 * 4,                  # x - mean per term, the cast, r * sgc, += prefill
    "dbeta": 2 * 2,                   # the cast, += prefill
    "dz": 2 * R_DZ,
    "acc": 2 * 1,                     # prefill + the result onto zeros: one more rounding
    # dz, then as K["act_bwd_rows"] of the element-wise suite: a thread's sequential sum over the pixels it visits and the
    # sequential LDS fold over `rows`
    "dbias_rows": lambda visits, rows: 2 * (R_DZ + visits + rows),
    # dz, the thread's PPT terms, 5 shuffle levels, 16 wave terms
    "dbias_small": lambda ppt: 2 * (R_DZ + ppt + 5 + 16),
    # finalize: mean, var, invstd in float64, rounded once
    "save_mean": 2 * 1,
    "save_invstd": 2 * 1,
    "scale": 2 * 2,                   # invstd, gamma * invstd
    "shift": 2 * 5,                   # (float)mean, scale (2), their product, beta - product
    "running": 2 * 3,                 # 1 - momentum and (float)stat in parallel, the two products in parallel, the sum
    # eval affine: rv + eps, sqrtf, 1/ (all correctly rounded)
    "eval_invstd": 2 * 3,
    "eval_scale": 2 * 4,
    "eval_shift": 2 * 6,              # rm * scale, beta - product
    # MEASURED (measure_chain_units): torch's float32 CPU batch_norm forward + backward against float64 on the chain test's
    # inputs; the rounding of the mean to float32 perturbs a - mean, which no count covers; 4 x the figure, rounded up
    "chain": math.ceil(4 * MEASURED["chain"]),
}


class DBuf:
    """the float64 sibling of Buf: rows x ld doubles between two guard bands, [:, :C] the kernel's (or `fill`), everything
    else a NaN-payload sentinel that must be bit-unchanged afterwards"""

    def __init__(self, rows, C, ld=None, fill=None):
        self.rows, self.C, self.ld = rows, C, ld or C
        self.n = rows * self.ld
        self.lo = (max(BAND, min(2 * self.ld, 4096)) + 63) // 64 * 64
        self.raw = torch.full((self.lo + self.n + self.lo,), SENT64, dtype=torch.int64, device=DEV)
        if fill is not None:
            self._body(self.raw)[:, :C] = fill.reshape(rows, C).double().to(DEV)
        self.before = self.raw.cpu()
        self.ptr = self.raw.data_ptr() + 8 * self.lo
        assert (self.raw.data_ptr() & 255) == 0

    def _body(self, raw):
        return raw[self.lo:self.lo + self.n].view(torch.float64).view(self.rows, self.ld)

    def check(self, what, rows_written=None):
        now = self.raw.cpu()
        own = torch.zeros(now.shape, dtype=torch.bool)
        own[self.lo:self.lo + self.n].view(self.rows, self.ld)[:self.rows if rows_written is None else rows_written, :self.C] = True
        stray = (now != self.before) & ~own
        assert not stray.any(), "%s: %d stray writes outside the output, first at double %d of the body" % (
            what, int(stray.sum()), int(stray.nonzero()[0]) - self.lo)
        return self._body(now)[:, :self.C].clone()


def slope_of(a, act):
    """act'(z) from the sign of a = act(z), float64"""
    one = torch.ones_like(a, dtype=torch.float64)
    if act == L.ACT_NONE:
        return one
    return torch.where(a > 0, one, one * (0.01 if act == L.ACT_LRELU else 0.0))


def act_fwd(z, act):
    if act == L.ACT_RELU:
        return F.relu(z)                                      # (its gradient at 0 is 0; clamp_min's is 1)
    return F.leaky_relu(z, 0.01) if act == L.ACT_LRELU else z.clone()


def bn_inputs(npix, C, act, seed, hard=True):
    """the inputs of one backward case, float32: z, a = act(z), gy, gamma and the saved statistics of a.  Every fifth row
    of z (hence of a) is exactly 0.0 and one element is -0.0.  The hard channel (mu 100, sd 0.01) keeps its rows: zeros in
    it would turn its standard deviation into 40 and it would no longer show a kernel that multiplies before it centres."""
    g = gen(seed)
    mu, sd = rnd(g, C) * 8, torch.rand(C, generator=g) * 4 + 0.05
    hard = hard and C > HARD
    if hard:
        mu[HARD], sd[HARD] = 100.0, 0.01
    z = torch.randn(npix, C, generator=g) * sd + mu
    keep = z[:, HARD].clone() if hard else None
    z[::5] = 0.0
    if hard:
        z[:, HARD] = keep
    z[npix // 2, 0] = -0.0
    a = act_fwd(z, act)
    a[npix // 2, 0] = -0.0                                    # (whatever the act makes of the sign of a zero)
    gy = rnd(g, npix, C)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1
    a64 = a.double()
    mean = a64.mean(0)
    var = (a64 - mean).pow(2).mean(0)
    return {"z": z, "a": a, "gy": gy, "gamma": gamma, "mean": mean.float(), "invstd": (1 / (var + BN_EPS).sqrt()).float(),
            "g": g}


def bn_bwd_ref(a, gy, gamma, mean, invstd, act, train):
    """float64 reference of the backward from the BatchNorm definition; mean and invstd are taken as given.  Returns the
    values and, under 'mag_*', the same formulas on absolute values."""
    a, gy, gm, mean, r = (t.double() for t in (a, gy, gamma, mean, invstd))
    M = a.shape[0]
    d = a - mean
    xhat = d * r
    dbeta = gy.sum(0)
    dgamma = (gy * xhat).sum(0)
    sl = slope_of(a, act)
    ag, ad = gy.abs(), d.abs()
    if train:
        dz = gm * r * (gy - dbeta / M - xhat * dgamma / M) * sl
        mag = (gm * r).abs() * ((ag + ag.mean(0)) + ad * r * r * (ag * ad).mean(0)) * sl
        coef = torch.stack([gm * r, r * r * (gy * d).mean(0), gy.mean(0)])
        mcoef = torch.stack([(gm * r).abs(), r * r * (ag * ad).mean(0), ag.mean(0)])
    else:
        dz = gm * r * gy * sl
        mag = (gm * r).abs() * ag * sl
        coef = torch.stack([gm * r, torch.zeros_like(r), torch.zeros_like(r)])
        mcoef = torch.stack([(gm * r).abs(), torch.zeros_like(r), torch.zeros_like(r)])
    return {"dz": dz, "dgamma": dgamma, "dbeta": dbeta, "dbias": dz.sum(0), "coef": coef,
            "mag_dz": mag, "mag_dgamma": r * (ag * ad).sum(0), "mag_dbeta": ag.sum(0), "mag_dbias": mag.sum(0),
            "mag_coef": mcoef}


def f64_floor(n, mag):
    """what a float64 sum of n terms of total magnitude `mag` may be off by"""
    return n * EPS64 * mag


def restate32(a, gy, gamma, mean, invstd, act, train):
    """the kernels' coefficient form in float32 torch, in the kernels' order: float64 sums cast once, then invM, coef0..2 and
    A*((g - MG) - (x - MU)*K)"""
    f = torch.float32
    assert all(t.dtype == f for t in (a, gy, gamma, mean, invstd))
    xc = a - mean
    sg = gy.double().sum(0).float()
    sgc = (gy.double() * xc.double()).sum(0).float()
    invM = torch.tensor(1.0, dtype=f) / torch.tensor(float(a.shape[0]), dtype=f)
    dgam = invstd * sgc
    A = gamma * invstd
    zero = torch.zeros_like(A)
    Kc = invstd * dgam * invM if train else zero
    MG = sg * invM if train else zero
    dz = A * ((gy - MG) - (a - mean) * Kc)
    if act != L.ACT_NONE:
        sl = torch.tensor(0.01 if act == L.ACT_LRELU else 0.0, dtype=f)
        dz = dz * torch.where(a > 0, torch.ones((), dtype=f), sl)
    return {"dz": dz, "dgamma": dgam, "dbeta": sg, "coef": torch.stack([A, Kc, MG])}


# ------------------------------------------------------------------------------------------------ case lists
BWD_C = [4, 12, 20, 96, 1028]
SMALL_NPIX = [1, 2, 511, 512, 513, 1024, 1025, 2047, 2048]
CHAIN = [(513, 12), (4099, 20)]


def col_npix_host(C, cap=COL_CAP):
    rows = 256 // min(C // 4, 256)
    return [1, rows * 4 - 1, 4 * rows * cap * 2 + 3]


def reduce_cases(C):
    """(npix, act, train) of the three-launch tests at C: every combination at the two small maps, one rotated pair at the
    largest; the last C, whose largest map is the smallest, takes the sixth pair too, so that all six appear"""
    n, i = col_npix_host(C), BWD_C.index(C)
    last = [COMBOS[i]] + ([COMBOS[5]] if i == len(BWD_C) - 1 else [])
    return [(npix, act, train) for npix in n[:2] for act, train in COMBOS] + [(n[2],) + c for c in last]


def small_cases(C):
    out = []
    for i, npix in enumerate(SMALL_NPIX):
        if npix <= 513:
            out += [(npix, act, train) for act, train in COMBOS]
        else:
            out.append((npix,) + COMBOS[(BWD_C.index(C) + i) % 6])
    return out


def case_seed(npix, C, act):
    return 1000 + 7 * (npix % 9973) + 13 * C + act


def units(got, ref, mag):
    return ((got.double() - ref).abs() / (EPS * mag).clamp_min(1e-300))[mag > 0].max().item() if (mag > 0).any() else 0.0


def measure_restate_units(Cs=BWD_C):
    """how MEASURED['restate'] was measured: restate32 against bn_bwd_ref, worst dz element in units of eps32 * mag_dz, over
    the inputs of every backward case of the GPU tests (no kernel runs), with and without the hard channel"""
    worst = 0.0
    for C in Cs:
        for npix, act, train in sorted(set(reduce_cases(C) + small_cases(C))):
            for hard in (True, False):
                if not hard and npix > 4099:
                    continue
                x = bn_inputs(npix, C, act, case_seed(npix, C, act), hard=hard)
                args = (x["a"], x["gy"], x["gamma"], x["mean"], x["invstd"], act, train)
                ref = bn_bwd_ref(*args)
                worst = max(worst, units(restate32(*args)["dz"], ref["dz"], ref["mag_dz"]))
    return worst


def chain_ref(a, gy, gamma, act, dtype):
    """autograd through F.batch_norm on a (training), times act'(a): dz in `dtype`"""
    x = a.to(dtype).clone().requires_grad_(True)
    y = F.batch_norm(x, None, None, gamma.to(dtype), torch.zeros_like(gamma, dtype=dtype), True, 0.1, BN_EPS)
    (y * gy.to(dtype)).sum().backward()
    return x.grad * slope_of(a, act).to(dtype)


def chain_case(npix, C):
    """the inputs of one chain case, the float64 autograd dz and its magnitude (from the float64 statistics)"""
    act = L.ACT_LRELU
    x = bn_inputs(npix, C, act, case_seed(npix, C, act))
    a64 = x["a"].double()
    mean = a64.mean(0)
    r = 1 / ((a64 - mean).pow(2).mean(0) + BN_EPS).sqrt()
    mag = bn_bwd_ref(x["a"], x["gy"], x["gamma"], mean, r, act, 1)["mag_dz"]
    return x, chain_ref(x["a"], x["gy"], x["gamma"], act, torch.float64), mag


def measure_chain_units():
    """how MEASURED['chain'] was measured: torch's float32 CPU batch_norm forward + backward against the float64 one on the
    chain test's inputs, worst element in units of eps32 * mag_dz (mag_dz from the float64 statistics)"""
    worst = 0.0
    for npix, C in CHAIN:
        x, ref, mag = chain_case(npix, C)
        worst = max(worst, units(chain_ref(x["a"], x["gy"], x["gamma"], L.ACT_LRELU, torch.float32), ref, mag))
    return worst


# ------------------------------------------------------------------------------------------------ finalisation
def stat_rows(x, nrows):
    """[npix, C] float32 -> float64 partial rows [nrows][2][C]: the map split into nrows chunks, each summed in float64"""
    x = x.double()
    rows = torch.zeros(nrows, 2, x.shape[1], dtype=torch.float64)
    for i, ch in enumerate(torch.tensor_split(x, nrows)):
        rows[i, 0], rows[i, 1] = ch.sum(0), (ch * ch).sum(0)
    return rows


def finalize_ref(rows, count, gamma, beta, rm, rv, momentum, eps):
    """float64 reference of pmf_bn_finalize over partial rows [nrows][2][C].  momentum and eps are the float32 values the
    kernel receives.  The running variance takes the unbiased estimate var * count / (count - 1) for count > 1 and var itself
    for count == 1: the project's rule (bn_finalize_k), where torch would divide by zero."""
    momentum, eps = (float(torch.tensor(v, dtype=torch.float32)) for v in (momentum, eps))
    gamma, beta = gamma.double(), beta.double()
    nrows = rows.shape[0]
    s1, s2 = rows[:, 0].sum(0), rows[:, 1].sum(0)
    a1, a2 = rows[:, 0].abs().sum(0), rows[:, 1].abs().sum(0)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    invstd = 1 / (var + eps).sqrt()
    scale = gamma * invstd
    unb = var * count / (count - 1) if count > 1 else var
    # the float64 part: the two sums of nrows terms, the division, the product and the difference of var
    dmean = f64_floor(nrows + 2, a1 / count)
    dvar = f64_floor(nrows + 4, a2 / count + 2 * mean.abs() * a1 / count)
    dinv = 0.5 * invstd * dvar / (var + eps)
    out = {"mean": mean, "invstd": invstd, "scale": scale, "shift": beta - mean * scale,
           "mag_mean": mean.abs(), "mag_invstd": invstd, "mag_scale": scale.abs(), "mag_shift": beta.abs() + (mean * scale).abs(),
           "floor_mean": dmean, "floor_invstd": dinv, "floor_scale": gamma.abs() * dinv,
           "floor_shift": dmean * scale.abs() + mean.abs() * gamma.abs() * dinv}
    if rm is not None:
        rm, rv = rm.double(), rv.double()
        out.update({"rm": (1 - momentum) * rm + momentum * mean, "rv": (1 - momentum) * rv + momentum * unb,
                    "mag_rm": (1 - momentum) * rm.abs() + momentum * mean.abs(), "mag_rv": (1 - momentum) * rv.abs() + momentum * unb,
                    "floor_rm": momentum * dmean, "floor_rv": momentum * dvar * (count / (count - 1) if count > 1 else 1.0)})
    return out


def finalize_inputs(npix, C, seed):
    """a float32 map [npix, C] with |mean| / std <= 160 (far below the 1e3 at which the float64 cancellation of
    sumsq/count - mean^2, eps64 * 1e6, would come near eps32), and the per-channel vectors"""
    g = gen(seed)
    mu, sd = rnd(g, C) * 8, torch.rand(C, generator=g) * 4 + 0.05
    x = torch.randn(npix, C, generator=g) * sd + mu
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1
    return {"x": x, "gamma": gamma, "beta": rnd(g, C), "rm": rnd(g, C) * 4, "rv": torch.rand(C, generator=g) * 4 + 0.1, "g": g}
