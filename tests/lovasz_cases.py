"""CPU side of tests/test_gpu_lovasz.py and tests/test_lovasz_reference_host.py: the inputs, the float64 reference of the
Lovasz stage of csrc/loss.hip (in-library radix sort, Jaccard first differences scattered through the permutation, fold),
the float32 restatement of the kernels' arithmetic, the derived bounds and the case lists.  Nothing here touches the GPU or
the built library, except the guarded word buffer WBuf, which the GPU tests alone construct.

The stage.  Rows r = head * C + cls of the key matrix f32[2C][P] hold the errors |fg - p| of one class and one head, -1 at
unlabelled pixels (label 0).  For every row whose class is not 0 and occurs among the labels, the m = P - cnt[0] labelled
pixels are ranked by DESCENDING error, equal errors in ascending pixel order; along that order, with fg_i = [label = cls],
    G = sum fg,  jaccard_i = 1 - (G - cumsum(fg)_i) / (G + cumsum(1 - fg)_i),  grad_i = jaccard_i - jaccard_{i-1}  (jaccard_-1 = 0)
    value = dot(err, grad),   gl / gc [n][cls][hw] += lam_head / n_present * grad_i * (fg_i ? -1 : +1)  where err_i != 0
and the fold turns the row values and the per-pixel partial sums `rows` f64[nrows][4] = {foc, foc_cam, per_p, per_q} into
    out8 = {total, foc, lov, foc_cam, lov_cam, per_p + per_q, per_p, per_q},  lov = sum of the head's row values / n_present,
    total = foc + foc_cam + lambda (lov + lov_cam) + gamma_per (per_p + per_q)       or      sum_i w6[i] * term_i.

Derived bounds (u = 2^-24, the unit roundoff of float32).  The kernels keep G, the running count and the rank in float32;
all three are integers below 2^24, so G - run and the union are exact, the (correctly rounded) division loses u / 2 relative
to a quotient <= 1 (u / 2 absolute), its rounding and that of the subtraction from 1 (a result <= 1) another u / 2 each, hence
|d jaccard| <= 1.5 u (the restatement finds 0.75 u, MEASURED['djac']).
  * grad_i: two Jaccard values, 3 u, plus the rounding of their difference, u |grad_i| <= u:  3 u + u = 4 u;
    pmf_lovasz_grad is held to 3 u per element (the difference is exact or its rounding is far below u wherever both
    Jaccard errors are at their worst: adjacent values in [1/2, 1) differ exactly).
  * an element of gl / gc:  lam / n_present * 4 u  +  2 u |expected element|  (the float32 product with the rounded weight
    and the read-modify-write add onto the prefill).
  * a row value: the errors are sorted descending and the Jaccard errors telescope,
    |sum e_i d grad_i| <= max |d jaccard| * (e_first - e_last) + the roundings of the differences <= 2 u per row whatever its
    length; the dot product itself is float64 (f64_floor).
  * out8[2], out8[4]: the mean of such rows, 2 u, plus the cast to float32, u |value|.
  * out8[1, 3, 5, 6, 7]: float64 sums of `rows` cast once: u |value| + n eps64 sum |terms|.
  * out8[0]: |w_lov| 2 u + |w_lov_cam| 2 u + u |value| + the float64 floor of the weighted sum.
restate32() evaluates the kernels' float32 formulas on the host over every GPU case; MEASURED records the worst error / bound
it finds for each quantity (tests/test_lovasz_reference_host.py keeps them below 1 and equal to what the helper returns)."""
import functools

import numpy as np

U = 2.0 ** -24
EPS64 = float(np.finfo(np.float64).eps)
CHUNK = 4096
P_MAX = 1 << 24                                    # pixels the Lovasz entry points accept (include/pmf_amd.h)

# worst error / bound of restate32() over CASES (measure()), and of the float32 first differences over GRAD_CASES
# (measure_grad()); 'djac' is the worst Jaccard error in units of u
MEASURED = {
    "grad": 0.47,
    "row": 0.31,
    "out8": 0.91,               # (a single cast to float32 loses between u / 2 and u of the value: this figure is near 1 by nature)
    "lovasz_grad": 0.50,
    "djac": 0.75,
}

LAMBDA, GAMMA_PER = 0.75, 0.375                    # (lambda != 1, gamma_per != 0.5)
W6 = (0.5, 1.25, 0.75, 0.625, 0.25, 1.5)           # (w6[1] != w6[3], w6[4] != w6[5]); exact in float32


# ------------------------------------------------------------------------------------------------ key patterns
def _bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def pattern(name, n, rng, row):
    """n float32 keys in [0, 1]"""
    if name == "uniform":
        return rng.random(n, dtype=np.float32)
    if name == "eighths":
        return (rng.integers(0, 9, n) / 8.0).astype(np.float32)
    if name == "saturated":
        return rng.integers(0, 2, n).astype(np.float32)
    if name == "equal":
        return np.full(n, (row + 1) / 64.0, dtype=np.float32)
    if name in ("descending", "ascending"):
        v = (np.arange(n, 0, -1) / float(n)).astype(np.float32)      # n <= 2^23: all distinct
        return v if name == "descending" else v[::-1].copy()
    if name.startswith("byte"):
        # float bit patterns that differ in ONE byte only: that counting pass alone orders the row.  Pass 3 sees bits 24-29
        # only (errors <= 1.0 = 0x3F800000; the sort key is 0x3FFFFFFF - bits)
        k = int(name[4])
        base, hi = ((0x3F000000, 256), (0x3E800000, 256), (0, 256), (0, 64))[k]
        return _bits(base | (rng.integers(0, hi, n).astype(np.uint32) << np.uint32(8 * k)))
    if name == "special":
        v = rng.random(n, dtype=np.float32)
        exact = _bits([0x00000000, 0x3F800000, 0x00000001, 0x3F7FFFFF, 0x00800000])   # 0, 1, denormal min, 1 - 2^-24, 2^-126
        pick = rng.integers(0, 20, n)
        for i, e in enumerate(exact):
            v[pick == i] = e
        return v
    raise KeyError(name)


PATTERNS = ["uniform", "eighths", "saturated", "equal", "descending", "ascending", "byte0", "byte1", "byte2", "byte3", "special"]
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8229]
MAKEUPS = ["full", "absent_single", "owner"]


def _case(name, N, HW, C, m, makeup, pats):
    return {"name": name, "N": N, "HW": HW, "C": C, "m": m, "makeup": makeup, "pats": pats}


def _cases():
    out = [
        _case("wave", 1, 35, 3, 20, "full", ("uniform", "eighths")),
        _case("ragged3", 3, 2743, 5, 5000, "full", ("uniform", "saturated")),
        _case("exact", 2, 4096, 14, 6000, "absent_single", ("eighths", "uniform")),
        _case("exact_all", 2, 4096, 14, 8192, "full", ("uniform", "special")),
        _case("r4", 1, 8229, 2, 8229, "full", ("saturated", "uniform")),
        _case("r40", 1, 8229, 20, 4097, "absent_single", ("special", "eighths")),
    ]
    n = len(PATTERNS)
    for i, m in enumerate(COUNTS):
        out.append(_case("count%d" % m, 3, 2743, 5, m, MAKEUPS[i % 3], (PATTERNS[i % n], PATTERNS[(i + 3) % n])))
        out.append(_case("count%d_r4" % m, 1, 8229, 2, m, "full", (PATTERNS[(i + 1) % n], PATTERNS[(i + 5) % n])))
    for m in (1, 4096, 8229):
        out.append(_case("count%d_r40" % m, 1, 8229, 20, m, MAKEUPS[m % 3], ("eighths", "uniform")))
    for i, p in enumerate(PATTERNS):
        out.append(_case("pat_" + p, 3, 2743, 5, 8229 if i % 2 else 5000, "full", (p, PATTERNS[(i + 1) % n])))
    return out


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]


def labels_of(P, C, m, makeup, rng):
    """int64[P] with exactly m labelled pixels (label != 0) at random positions.  full: every class 1..C-1 occurs (as far as m
    allows); absent_single: class 1 has one pixel and the last class none (C >= 4; with C = 3 class 2 owns the rest);
    owner: one class owns every labelled pixel"""
    lab = np.zeros(P, dtype=np.int64)
    where = rng.permutation(P)[:m]
    if m == 0:
        return lab
    if C == 2 or makeup == "owner":
        lab[where] = 1 if C == 2 else 2
        return lab
    if makeup == "full":
        cls = rng.integers(1, C, m)
        cls[:min(m, C - 1)] = np.arange(1, C)[:min(m, C - 1)]
    else:
        hi = C - 1 if C >= 4 else C
        cls = rng.integers(2, hi, m)
        cls[0] = 1
    lab[where] = cls
    return lab


@functools.lru_cache(None)
def inputs(name):
    """the inputs of one case: key f32[2C][P], label i64[P], cnt i64[C], rows f64[nrows][4], the prefills of gl and gc
    f32[N][C][HW]"""
    cs = CASES[CASE_NAMES.index(name)]
    N, HW, C, m = cs["N"], cs["HW"], cs["C"], cs["m"]
    P = N * HW
    rng = np.random.default_rng(1000 + CASE_NAMES.index(name))
    label = labels_of(P, C, m, cs["makeup"], rng)
    assert int((label != 0).sum()) == m
    key = np.empty((2 * C, P), dtype=np.float32)
    for r in range(2 * C):
        key[r] = pattern(cs["pats"][r // C], P, rng, r)
    key[:, label == 0] = -1.0
    nrows = (P + 255) // 256
    return dict(cs, P=P, key=key, label=label, cnt=np.bincount(label, minlength=C).astype(np.int64),
                rows=rng.random((nrows, 4)) * 2 - 1, nrows=nrows,
                pre_gl=(rng.random((N, C, HW), dtype=np.float32) * 2 - 1), pre_gc=(rng.random((N, C, HW), dtype=np.float32) * 2 - 1))


# ------------------------------------------------------------------------------------------------ float64 reference
def jaccard_grad(fg):
    """float64 first differences of the Jaccard index along one sorted 0/1 row"""
    fg = np.asarray(fg, dtype=np.float64)
    G = fg.sum()
    jac = 1.0 - (G - np.cumsum(fg)) / np.maximum(G + np.cumsum(1.0 - fg), 1e-12)
    return np.diff(jac, prepend=0.0), jac


def weights_of(lam, gamma_per, w6):
    """the six weights of {foc, lov, foc_cam, lov_cam, per_p, per_q} as the kernels receive them (float32)"""
    f = np.float32
    if w6 is not None:
        return [float(f(w)) for w in w6]
    return [1.0, float(f(lam)), 1.0, float(f(lam)), float(f(gamma_per)), float(f(gamma_per))]


def reference(key, label, N, HW, C, rows, pre_gl, pre_gc, lam=LAMBDA, gamma_per=GAMMA_PER, w6=None):
    """float64, from the definition.  key [2C][P] (float32 or float64).  Returns per present row the permutation, the sorted
    errors, the foreground flags, the first differences and the value; the full-length permutation / sorted keys of EVERY row
    (labelled pixels first, unlabelled at the tail: what the int64 entry points are fed); the expected gl / gc with the
    mask of the elements the stage may touch and their bound; out8 with its bound."""
    P = N * HW
    label = np.asarray(label)
    cnt = np.bincount(label, minlength=C)
    m = P - int(cnt[0])
    present = [c for c in range(1, C) if cnt[c] > 0]
    npres = max(len(present), 1)
    w = weights_of(lam, gamma_per, w6)
    k64 = np.asarray(key, dtype=np.float64)
    perm_full = np.empty((2 * C, P), dtype=np.int64)
    out = {"m": m, "present": present, "rows": {}, "perm_full": perm_full}
    exp = [np.asarray(pre_gl, dtype=np.float64).copy(), np.asarray(pre_gc, dtype=np.float64).copy()]
    touched = [np.zeros((N, C, HW), dtype=bool), np.zeros((N, C, HW), dtype=bool)]
    lov = [0.0, 0.0]
    alov = [0.0, 0.0]
    for r in range(2 * C):
        head, cls = divmod(r, C)
        order = np.argsort(-k64[r], kind="stable")                   # equal keys: ascending pixel order
        perm_full[r] = order
        if cls == 0 or cnt[cls] == 0:
            continue
        perm = order[label[order] != 0]
        assert perm.shape[0] == m and np.array_equal(perm, order[:m])
        err = np.asarray(key)[r, perm]
        fg = label[perm] == cls
        grad, jac = jaccard_grad(fg)
        e64 = err.astype(np.float64)
        value = float(np.dot(e64, grad))
        lam_np = w[1 + 2 * head] / npres
        nz = err != 0
        n_, hw_ = np.divmod(perm[nz], HW)
        exp[head][n_, cls, hw_] += lam_np * grad[nz] * np.where(fg[nz], -1.0, 1.0)
        touched[head][n_, cls, hw_] = True
        lov[head] += value
        alov[head] += float(np.dot(e64, np.abs(grad)))
        out["rows"][r] = {"perm": perm, "err": err, "fg": fg, "grad": grad, "jac": jac, "value": value,
                          "floor": m * EPS64 * float(np.dot(e64, np.abs(grad)))}
    out["val_full"] = np.take_along_axis(np.asarray(key), perm_full, 1)
    out["gl"], out["gc"], out["touched"] = exp[0], exp[1], touched
    out["lam_np"] = [w[1] / npres, w[3] / npres]
    out["grad_bound"] = [abs(out["lam_np"][h]) * 4 * U + 2 * U * np.abs(exp[h]) for h in (0, 1)]
    rows = np.asarray(rows, dtype=np.float64)
    s, a = rows.sum(0), np.abs(rows).sum(0)
    nr = rows.shape[0] + 8
    terms = [s[0], lov[0] / npres, s[1], lov[1] / npres, s[2], s[3]]             # foc, lov, foc_cam, lov_cam, per_p, per_q
    aterms = [a[0], alov[0] / npres, a[1], alov[1] / npres, a[2], a[3]]
    nterm = [nr, m + nr, nr, m + nr, nr, nr]
    floor = [nterm[i] * EPS64 * aterms[i] for i in range(6)]
    total = sum(w[i] * terms[i] for i in range(6))
    o8 = np.array([total, terms[0], terms[1], terms[2], terms[3], terms[4] + terms[5], terms[4], terms[5]])
    b8 = np.array([
        (abs(w[1]) + abs(w[3])) * 2 * U + U * abs(total) + sum(abs(w[i]) * (floor[i] + 8 * EPS64 * aterms[i]) for i in range(6)),
        U * abs(o8[1]) + floor[0],
        2 * U + U * abs(o8[2]) + floor[1],
        U * abs(o8[3]) + floor[2],
        2 * U + U * abs(o8[4]) + floor[3],
        U * abs(o8[5]) + floor[4] + floor[5] + EPS64 * (aterms[4] + aterms[5]),
        U * abs(o8[6]) + floor[4],
        U * abs(o8[7]) + floor[5],
    ])
    out["out8"], out["out8_bound"] = o8, b8
    return out


ROW_BOUND = 2 * U


@functools.lru_cache(None)
def case_ref(name, weighted):
    x = inputs(name)
    return reference(x["key"], x["label"], x["N"], x["HW"], x["C"], x["rows"], x["pre_gl"], x["pre_gc"],
                     w6=W6 if weighted else None)


# ------------------------------------------------------------------------------------------------ float32 restatement
def jaccard_grad32(fg, n_valid=None):
    """lovasz_grad_k / lovasz2_grad_k on one sorted 0/1 row: run, G and the rank in float32,
    uni = G + ((float)(i + 1) - run), j = 1.f - (G - run) / max(uni, 1e-12f), gr = j - jprev; 0 from n_valid on"""
    f = np.float32
    fg = np.asarray(fg, dtype=f)
    run = np.cumsum(fg, dtype=f)                                     # (integers below 2^24: exact)
    G = f(run[-1]) if fg.size else f(0)
    uni = G + (np.arange(1, fg.size + 1, dtype=f) - run)
    j = f(1) - (G - run) / np.maximum(uni, f(1e-12))
    assert j.dtype == f
    gr = np.empty_like(j)
    gr[:1] = j[:1]
    gr[1:] = j[1:] - j[:-1]
    if n_valid is not None:
        gr[n_valid:] = 0
    return gr, j


def restate32(x, ref, weighted):
    """the Lovasz stage in the kernels' arithmetic on the reference's permutation: float32 Jaccard, float64 dot product, the
    float32 product lam / n_present * gr and the float32 add onto the prefill, the fold in float64 cast once"""
    f = np.float32
    N, HW, C = x["N"], x["HW"], x["C"]
    w = weights_of(LAMBDA, GAMMA_PER, W6 if weighted else None)
    npres = max(len(ref["present"]), 1)
    g = [x["pre_gl"].copy(), x["pre_gc"].copy()]
    vals, djac = {}, 0.0
    lov = [0.0, 0.0]
    for r, row in ref["rows"].items():
        head, cls = divmod(r, C)
        gr, j = jaccard_grad32(row["fg"])
        djac = max(djac, float(np.abs(j.astype(np.float64) - row["jac"]).max()) / U) if j.size else djac
        vals[r] = float(np.dot(row["err"].astype(np.float64), gr.astype(np.float64)))
        lov[head] += vals[r]
        wcls = f(w[1 + 2 * head]) / f(npres)
        nz = row["err"] != 0
        n_, hw_ = np.divmod(row["perm"][nz], HW)
        d = (wcls * gr[nz]) * np.where(row["fg"][nz], f(-1), f(1))
        assert d.dtype == f
        g[head][n_, cls, hw_] = g[head][n_, cls, hw_] + d
    s = x["rows"].sum(0)
    t = [s[0], lov[0] / npres, s[1], lov[1] / npres, s[2], s[3]]
    total = sum(w[i] * t[i] for i in range(6))
    o8 = np.array([total, t[0], t[1], t[2], t[3], t[4] + t[5], t[4], t[5]]).astype(f)
    return {"gl": g[0], "gc": g[1], "values": vals, "out8": o8, "djac": djac}


def ratios(got, ref):
    """worst error / bound of one run (restated or from the GPU) per quantity: got = {gl, gc, values {r: v}, out8}"""
    out = {"grad": 0.0, "row": 0.0, "out8": 0.0}
    for h, name in enumerate(("gl", "gc")):
        t = ref["touched"][h]
        if t.any():
            e = np.abs(got[name].astype(np.float64) - ref[name])[t] / ref["grad_bound"][h][t]
            out["grad"] = max(out["grad"], float(e.max()))
    for r, row in ref["rows"].items():
        out["row"] = max(out["row"], abs(got["values"][r] - row["value"]) / (ROW_BOUND + row["floor"]))
    out["out8"] = float((np.abs(got["out8"].astype(np.float64) - ref["out8"]) / ref["out8_bound"]).max())
    return out


def measure(names=None):
    """how MEASURED['grad' / 'row' / 'out8' / 'djac'] were measured: restate32 against the reference over the GPU cases"""
    worst = {"grad": 0.0, "row": 0.0, "out8": 0.0, "djac": 0.0}
    for name in names or CASE_NAMES:
        for weighted in (False, True):
            x, ref = inputs(name), case_ref(name, weighted)
            got = restate32(x, ref, weighted)
            rt = dict(ratios(got, ref), djac=got["djac"])
            worst = {k: max(worst[k], rt[k]) for k in worst}
    return worst


# ------------------------------------------------------------------------------------------------ pmf_lovasz_grad
GRAD_P = [1, 35, 4095, 4096, 4097, 8229]
GRAD_BOUND = 3 * U


def grad_nvalid(P):
    return sorted({v for v in (0, 1, P // 2, P, 4095, 4096, 4097, 8191, 8192, 8193) if v <= P})


GRAD_CASES = [(P, nv) for P in GRAD_P for nv in grad_nvalid(P)]


@functools.lru_cache(None)
def grad_inputs(P, nv):
    """fg f32[3][P], rows all 0, all 1 and random over the first nv slots; the ignored tail holds 0 (as a sorted row does)"""
    rng = np.random.default_rng(7 * P + nv)
    fg = np.zeros((3, P), dtype=np.float32)
    fg[1, :nv] = 1
    fg[2, :nv] = rng.integers(0, 2, nv)
    return fg


def grad_ref(fg, nv):
    out = np.stack([jaccard_grad(row)[0] for row in fg])
    out[:, nv:] = 0
    return out


def measure_grad():
    worst = 0.0
    for P, nv in GRAD_CASES:
        fg = grad_inputs(P, nv)
        got = np.stack([jaccard_grad32(row, nv)[0] for row in fg])
        worst = max(worst, float(np.abs(got.astype(np.float64) - grad_ref(fg, nv)).max()) / GRAD_BOUND)
    return worst


# ------------------------------------------------------------------------------------------------ device side
class WBuf:
    """a tensor of 4- or 8-byte elements (int64 labels, counts and permutations; the sort's workspace as int32 words) between
    two guard bands of the sentinel the float buffers use; `t` None: n words of sentinel"""

    def __init__(self, t=None, words=0):
        import torch
        from tests.test_gpu_elementwise import BAND, DEV, SENT
        self.dtype = torch.int32 if t is None else t.dtype
        self.shape = (words,) if t is None else tuple(t.shape)
        body = None if t is None else t.contiguous().view(-1).view(torch.int32)
        self.n = words if t is None else body.numel()
        self.lo = max(BAND, 4096)
        self.raw = torch.full((self.lo + self.n + self.lo,), SENT, dtype=torch.int32, device=DEV)
        if body is not None:
            self.raw[self.lo:self.lo + self.n] = body.to(DEV)
        self.before = self.raw.cpu()
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        assert (self.raw.data_ptr() & 255) == 0

    def check(self, what, written=False):
        """bands bit-unchanged (and the body too unless `written`); returns the body on the CPU in its own type"""
        now = self.raw.cpu()
        stray = now != self.before
        if written:
            stray[self.lo:self.lo + self.n] = False
        assert not stray.any(), "%s: %d stray writes, first at word %d of the body" % (
            what, int(stray.sum()), int(stray.nonzero()[0]) - self.lo)
        return now[self.lo:self.lo + self.n].view(self.dtype).view(self.shape).clone()
