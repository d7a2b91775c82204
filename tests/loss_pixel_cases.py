"""CPU side of tests/test_gpu_loss_pixel.py and tests/test_loss_pixel_reference_host.py: the inputs, the float64 reference of
the per-pixel stage of csrc/loss.hip (loss_count_k, loss_pixel_k<false / true>, loss_dice_sums_k, loss_dice_fold_k), the
float32 restatement of the kernel's arithmetic, the derived bounds, the gate margins, the mutants and the case lists.  Nothing
here touches the GPU or the built library.

The stage.  p / q = LiDAR / camera probabilities of one pixel (float32 [N][C][HW]), t its label, P = N HW, M = P C:
    plog_c = ln max(p_c, 1e-8),  e_p = -sum_c p_c plog_c / ln C,  conf_p = 1 - e_p,  d = conf_p - conf_q
    gate_p = [d > 0][conf_p >= tau],  gate_q = [d < 0][conf_q >= tau],  w_pcd = gate_p |d|,  w_img = gate_q |d|
    Lp = sum_c xlogy(q_c, q_c) - q_c plog_c,  Lq = sum_c xlogy(p_c, p_c) - p_c qlog_c
    per_p = sum_pixels w_img Lp / M,  per_q = sum_pixels w_pcd Lq / M            (the weights are NOT detached)
    foc = sum_{0 < t < C} -(1 - p_t)^g ln max(p_t, 1e-6) alpha_t / (P - cnt[0])
    dice: see pmf_amd/loss/dice_loss.py explog_dice_closed_form
core() evaluates these formulas and every piece of their analytic gradient in the order the kernel does, in the dtype it is
given: in float64 it IS the reference (tests/test_loss_pixel_reference_host.py holds it to float64 autograd through the
project's own loss modules, term by term), in float32 it is the restatement of the kernel's arithmetic (logf / powf stand in
as the correctly rounded float32 value of the float64 function, so that the figures do not depend on the host's libm).
The thresholds 1e-8, 1e-6, 1e-38 and tau are the float32-rounded constants in both: a float32 p equal to float32(1e-8) is
NOT clamped.

Where the stage deviates from the torch modules (pinned by the tests, stated in include/pmf_amd.h):
  * a batch without a labelled pixel: the modules give 0 / 0 = NaN for the focal terms, the kernel 0 and finite gradients;
  * p_c = 0 under an open gate: d xlogy(p, p) / dp = ln 0 + 1 = -inf in autograd; the kernel takes ln max(p_c, 1e-38).

Derived bounds (u = 2^-24; first order in u).  A float32 +, -, *, / loses u relative.  What the device's logf / powf lose is
NOT KNOWN on the machine these bounds were written on: 4 ulp = 8 u relative per call is ALLOWED (LU), an unmeasured figure.
  * plog_c: LU |plog_c|.
  * e_p: the C products lose (LU + u) each, their sequential sum C u of sum |p_c plog_c| =: A_p; 1 / logf(C) and the product
    with it (LU + 2 u) |e_p|:   de_p = (LU + (C + 1) u) A_p / ln C + (LU + 2 u) |e_p|,   dconf_p = de_p + u.
  * d = conf_p - conf_q is a cancellation: dd = dconf_p + dconf_q + u |d| is an ABSOLUTE error, and it is what w_pcd / w_img
    inherit (dw = gate dd): relative to a small |d| it is large, and the bounds below carry it as such.
  * Lp: 2C terms, each a product with a logarithm:  dLp = (LU + (2C + 1) u) sum_c |q_c ln q_c| + |q_c plog_c|.
  * dd/dp_c = (plog_c + [p_c >= 1e-8]) / ln C:  ddd = (LU |plog_c| + (LU + 3 u) |plog_c + i_c|) / ln C.
  * the gradient of one pixel and class is  spa (a + b) + spb (e + f) + [c = t] dfoc + dice_c  with
        a = -w_img q_c / p_c                    da = dw q_c / p_c + 3 u |a|
        b = -Lp gate_q dd/dp_c                  db = dLp |dd/dp_c| + |Lp| ddd + 2 u |b|
        e = w_pcd (ln max(p_c, 1e-38) + 1 - qlog_c) =: w_pcd s       de = dw |s| + w_pcd ds + u |e|,
                                                                     ds = LU (|ln p_c| + |qlog_c|) + 2 u (|ln p_c| + 1 + |qlog_c|)
        f = Lq gate_p dd/dp_c                   as b
    (and the mirror image for q), by the product rule; the sum of a pair and the product with spa = w / (float) M lose 4 u of
    |a| + |b|;  dfoc = w alpha_t (g o^(g-1) ln p_t - o^g / p_t) / (P - cnt[0]), o = 1 - p_t, loses
    ((|g - 1| + 2) u + 2 LU) |T1| + ((g + 1) u + LU) |T2| + 6 u (|T1| + |T2|);  the Dice term K/C (2 [t = c] - dice_c) / D_c,
    three casts from float64, a difference and two products: 7 u of |K/C| (2 [t = c] + dice_c) / D_c;  the final additions 3 u
    of the sum of the magnitudes.
  * a pixel's per_p value: (dw |Lp| + w_img dLp) / M;  its focal value ((g + 3) u + 2 LU) |value|;  a row of `rows` is a
    float64 sum of 256 of these.
  * parts and dice are float64 throughout: n eps64 sum |terms|.
Gate margins.  A generated pixel is left out of the value and gradient comparison only if |d| <= dd, |conf_p - tau| <= dconf_p
or |conf_q - tau| <= dconf_q: there float32 may take the other branch.  Hand-made edge pixels that sit exactly ON a branch
(d = 0 by construction: identical heads, one-hot rows) are compared by branch: the reference is evaluated on the side the
float32 restatement took, which the kernel must take too.  Caps (conditions, held by the host test): at most 5 % of a case's
pixels left out; at least 10 % of them in each open-gate state after the exclusion -- except in the case p1, whose single
pixel has one gate state.  restate32 runs over every case; MEASURED records its worst error / bound per quantity."""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
LU = 8 * U                    # ALLOWED, not measured: 4 ulp of float32 per logf / powf call on the device
EPS64 = float(np.finfo(np.float64).eps)
F32, F64 = np.float32, np.float64
T8, T6, T38 = F32(1e-8), F32(1e-6), F32(1e-38)
BLOCK = 256                   # LP_BLOCK and DS_TILE of csrc/loss.hip
BOOSTS = (0.0, 3.0, 6.0, 9.0, 14.0)
PARAMS = [(2.0, 0.7, 0.375), (1.0, 0.3, 0.375), (1.5, 0.7, 0.25)]     # (focal_gamma, tau, gamma_per); gamma_per != 0.5
W6 = (0.5, 1.25, 0.75, 0.625, 0.25, 1.5)              # {foc, lov, foc_cam, lov_cam, per_p, per_q}; exact in float32
W6_OTHER_LOV = (0.5, -3.0, 0.75, 7.0, 0.25, 1.5)      # differs in w6[1], w6[3] alone: the stage must not notice
UNIT = {"foc": (1, 0, 0, 0, 0, 0), "foc_cam": (0, 0, 1, 0, 0, 0), "per_p": (0, 0, 0, 0, 1, 0), "per_q": (0, 0, 0, 0, 0, 1)}
W_LOV_ONLY = (0, 1, 0, 1, 0, 0)

# worst error / bound of the float32 restatement over CASES and DICE_CASES (measure()); tests/test_loss_pixel_reference_host.py
# holds these figures to what the helper returns
MEASURED = {
    "grad_foc": 0.19,
    "grad_per": 0.49,
    "grad_total": 0.49,
    "grad_dice": 0.49,
    "rows": 0.13,
}

MUTANTS = ["detached", "ddq_sign", "ip_one", "clamp6_for_8", "clamp8_for_6", "w45_swap", "per_over_P", "focal_over_P", "pow_g",
           "dice_one"]


# ------------------------------------------------------------------------------------------------ cases
def _case(name, N, C, HW, labels="mixed", edges=False, par=0):
    return {"name": name, "N": N, "C": C, "HW": HW, "labels": labels, "edges": edges, "par": par}


CASES = [
    _case("c2", 1, 2, 77, edges=True, par=0),
    _case("c5", 2, 5, 333, edges=True, par=1),
    _case("c14", 3, 14, 527, labels="absent", par=2),
    _case("c20", 2, 20, 1031, edges=True, par=0),
    _case("c32", 1, 32, 300, edges=True, par=1),
    _case("p1", 1, 5, 1, labels="nounlab", par=0),
    _case("p255", 1, 5, 255, par=2),
    _case("p256", 1, 5, 256, labels="nounlab", par=1),
    _case("p257", 1, 5, 257, par=0),
    _case("n2c2", 2, 2, 131, par=2),
    _case("n3c32", 3, 32, 70, par=0),
    _case("allunlab", 2, 5, 133, labels="allunlab", par=1),
    _case("dicezero", 1, 5, 300, labels="dicezero", par=0),
]
CASE_NAMES = [c["name"] for c in CASES]
DICE_NPARTS = (1, 15, 16, 17, 127, 128, 129, 300)
DICE_C = (2, 14, 32)
DICE_CASES = [_case("dice%d_c%d" % (nparts, C), 1, C, nparts * BLOCK - (0 if nparts % 2 == 0 else 3 if nparts > 1 else 99),
                    par=(nparts + C) % 3) for nparts in DICE_NPARTS for C in DICE_C]
DICE_NAMES = [c["name"] for c in DICE_CASES]
COUNT_CASE = _case("count", 1, 2, 2048 * 1024 + 2049)        # beyond loss_count_k's 1024 workgroups x 8 pixels per thread
_ALL = {c["name"]: c for c in CASES + DICE_CASES + [COUNT_CASE]}


def _soft(C, k=0):
    """an unsure row without ties"""
    v = np.roll(1.0 + 0.37 * np.arange(C), k)
    return (v / v.sum()).astype(F32)


def _sharp(C, big, special, fill=True):
    """nearly one-hot at `big`; special {class: float32 value} is stored exactly; the other classes hold small distinct
    values (fill) or exact zeros"""
    r = np.zeros(C)
    if fill:
        r[:] = 1e-3 * (1 + np.arange(C)) / C
    for i, v in special.items():
        r[i] = float(v)
    r[big] = 0.0
    r[big] = 1.0 - r.sum()
    r = r.astype(F32)
    for i, v in special.items():
        r[i] = F32(v)
    return r


def _onehot(C, k):
    r = np.zeros(C, dtype=F32)
    r[k] = 1
    return r


def _tie(C, i, j):
    r = _soft(C).astype(F64)
    r[i] = r[j] = r.max() * 1.25
    r = (r / r.sum()).astype(F32)
    assert r[i] == r[j] == r.max()
    return r


SPECIALS = [F32(0), np.nextafter(T8, F32(0)), T8, np.nextafter(T8, F32(1)), np.nextafter(T6, F32(0)), T6, np.nextafter(T6, F32(1))]
_ON_THRESHOLD = (F32(0), T8, T6)


def edge_pixels(C):
    """[(p row, q row, label, exact)]: `exact` marks rows with a 0 or a value exactly on a clamp, where float64 autograd
    through the torch modules (thresholds 1e-8 / 1e-6 as doubles, ln 0) is not the reference"""
    out = []
    both = lambda a, b, t, ex: out.extend([(a, b, t, ex), (b, a, t, ex)])                                   # noqa: E731
    for s in SPECIALS:
        ex = any(s == v for v in _ON_THRESHOLD)
        both(_sharp(C, 0, {1: s}), _soft(C), 1, ex)                       # p_t = s; the sharp head's gate is open
    both(_onehot(C, 1), _soft(C), 1, True)                                # p_t = 1
    out.append((_onehot(C, 1), _onehot(C, 1), 1, True))                   # d = 0, every p_c in {0, 1}
    out.append((_onehot(C, 0), _onehot(C, 1), 1, True))
    out.append((_soft(C, 1), _soft(C, 1), 1, False))                      # identical heads: d = 0
    ties = [(0, 1), (C - 2, C - 1)] + ([(1, 2)] if C >= 3 else [])
    for k, (i, j) in enumerate(ties):
        for t in (0, 1):
            out.append((_tie(C, i, j), _tie(C, *ties[(k + 1) % len(ties)]), t, False))
    if C >= 3:
        for s in SPECIALS:      # the UNSURE head holds the tiny value: the other head's gate is open, q_c / p_c is guarded
            r = np.zeros(C)
            r[:] = 1e-3 * (1 + np.arange(C)) / C
            r[0], r[1], r[2] = 0.5, 0.0, 0.0
            r[2] = 1.0 - r.sum()
            r = r.astype(F32)
            r[1] = s
            both(r, _sharp(C, 0, {1: F32(1e-3)}), 1, any(s == v for v in _ON_THRESHOLD))
    return out


def _labels(kind, P, C, rng):
    if kind == "allunlab":
        return np.zeros(P, dtype=np.int64)
    hi = C - 1 if (kind == "absent" and C >= 3) else C
    lab = rng.integers(1, hi, P)
    if kind in ("mixed", "absent", "dicezero"):
        lab[rng.random(P) < 0.3] = 0
    if kind == "dicezero":
        lab[:C] = np.arange(C)                                            # every class present, class 0 too
    return lab.astype(np.int64)


def _head(P, C, rng):
    """float32 probabilities [P][C]: logits uniform in [-2, 2], a boost from BOOSTS on one random class per pixel, softmax
    (evaluated in float64 and rounded once, so that every host builds the same float32 inputs)"""
    z = rng.random((P, C)) * 4 - 2
    z[np.arange(P), rng.integers(0, C, P)] += np.asarray(BOOSTS)[rng.integers(0, len(BOOSTS), P)]
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def to_nchw(a, x):
    return np.ascontiguousarray(a.reshape(x["N"], x["HW"], x["C"]).transpose(0, 2, 1))


def to_pix(a, x):
    return np.ascontiguousarray(np.asarray(a).reshape(x["N"], x["C"], x["HW"]).transpose(0, 2, 1)).reshape(x["P"], x["C"])


def make_inputs(cs, edges=None, safe_only=False):
    """edges: None = as the case says.  safe_only: leave out the edge pixels marked `exact`"""
    N, C, HW = cs["N"], cs["C"], cs["HW"]
    P = N * HW
    rng = np.random.default_rng(zlib.crc32(cs["name"].encode()))      # (a case's inputs depend on its own name alone)
    pp, qq = _head(P, C, rng), _head(P, C, rng)
    label = _labels(cs["labels"], P, C, rng)
    edge, exact = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    if cs["labels"] == "dicezero":                # the true-class probability is exactly 0 in both heads
        on = label > 0
        pp[on, label[on]] = 0
        qq[on, label[on]] = 0
        edge[on] = exact[on] = True
    if cs["edges"] if edges is None else edges:
        rows = [r for r in edge_pixels(C) if not (safe_only and r[3])]
        assert len(rows) < P
        for k, (a, b, t, ex) in enumerate(rows):
            i = P - len(rows) + k
            pp[i], qq[i], label[i], edge[i], exact[i] = a, b, t, True, ex
    fg, tau, gper = PARAMS[cs["par"]]
    alpha = (0.25 + rng.random(C)).astype(F32)
    return dict(cs, P=P, pp=pp, qq=qq, p=to_nchw(pp, cs), q=to_nchw(qq, cs), label=label, alpha=alpha, fg=fg, tau=tau, gper=gper,
                edge=edge, exact=exact, nrows=-(-P // BLOCK))


@functools.lru_cache(None)
def inputs(name):
    return make_inputs(_ALL[name])


# ------------------------------------------------------------------------------------------------ the formulas, in any dtype
def _lg(a, dt):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(a, dtype=F64)).astype(dt)


def _pw(a, e, dt):
    return np.power(np.asarray(a, dtype=F64), float(e)).astype(dt)


def histogram(label, C):
    label = np.asarray(label)
    return np.bincount(label[(label >= 0) & (label < C)], minlength=C).astype(np.int64)


def core(x, dt, mut=None, gates=None, clamps=(T8, T6)):
    """every per-pixel quantity of loss_pixel_k in dtype dt, in the kernel's order of operations.  gates: (gate_p, gate_q)
    to take instead of the ones dt's own d and confidences give.  mut: one of MUTANTS (a deliberately WRONG variant).
    clamps: the two thresholds; the kernel's are float32(1e-8), float32(1e-6), the torch modules' the doubles 1e-8, 1e-6"""
    f = dt
    P, C = x["P"], x["C"]
    p, q = x["pp"].astype(f), x["qq"].astype(f)
    lab = x["label"]
    t8 = f(clamps[1] if mut == "clamp6_for_8" else clamps[0])
    t6 = f(clamps[0] if mut == "clamp8_for_6" else clamps[1])
    t38, one, zero = f(T38), f(1), f(0)
    logC = _lg(f(C), f)
    ilogC = one / logC
    plog, qlog = _lg(np.maximum(p, t8), f), _lg(np.maximum(q, t8), f)
    xlp = np.where(p > 0, p * _lg(np.where(p > 0, p, one), f), zero)
    xlq = np.where(q > 0, q * _lg(np.where(q > 0, q, one), f), zero)
    ep, eq, Lp, Lq = (np.zeros(P, dtype=f) for _ in range(4))
    for c in range(C):
        ep = ep - p[:, c] * plog[:, c]
        eq = eq - q[:, c] * qlog[:, c]
        Lp = Lp + (xlq[:, c] - q[:, c] * plog[:, c])
        Lq = Lq + (xlp[:, c] - p[:, c] * qlog[:, c])
    ep, eq = ep * ilogC, eq * ilogC
    conf_p, conf_q = one - ep, one - eq
    d = conf_p - conf_q
    tau = f(F32(x["tau"]))
    if gates is None:
        gp, gq = (d > 0) & (conf_p >= tau), (d < 0) & (conf_q >= tau)
    else:
        gp, gq = gates
    gpf, gqf = gp.astype(f), gq.astype(f)
    ad = np.abs(d)
    wp, wi = gpf * ad, gqf * ad
    ip = np.ones_like(p) if mut == "ip_one" else (p >= t8).astype(f)
    iq = np.ones_like(q) if mut == "ip_one" else (q >= t8).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        rp, rq = np.where(ip > 0, one / p, zero), np.where(iq > 0, one / q, zero)
        ddp = (plog + ip) * ilogC
        ddq = (qlog + iq) * ilogC if mut == "ddq_sign" else -(qlog + iq) * ilogC
        det = zero if mut == "detached" else one
        l38p, l38q = _lg(np.maximum(p, t38), f), _lg(np.maximum(q, t38), f)
        col = lambda v: v[:, None]                                                                          # noqa: E731
        K = {
            "a1": -col(wi) * q * rp, "b1": -(col(Lp * gqf) * ddp) * det,
            "e1": col(wp) * (l38p + one - qlog), "f1": (col(Lq * gpf) * ddp) * det,
            "a2": col(wi) * (l38q + one - plog), "b2": -(col(Lp * gqf) * ddq) * det,
            "e2": -col(wp) * p * rq, "f2": (col(Lq * gpf) * ddq) * det,
        }
    # focal
    cnt = histogram(lab, C)
    valid = (lab > 0) & (lab < C)
    tt = np.where(valid, lab, 0)
    ar = np.arange(P)
    al = x["alpha"].astype(f)[tt]
    fg = f(F32(x["fg"]))
    msum = float(P if mut == "focal_over_P" else P - cnt[0])
    M = float(P if mut == "per_over_P" else P * C)
    for name, r in (("l", p), ("c", q)):
        pt = r[ar, tt]
        ll, o = _lg(np.maximum(pt, t6), f), one - pt
        pw = _pw(o, fg, f)
        if mut == "pow_g":
            pw1 = _pw(o, fg, f)
        else:
            pw1 = np.ones_like(o) if fg == 1 else _pw(o, fg - one, f)
        with np.errstate(divide="ignore", invalid="ignore"):
            T2 = np.where(pt >= t6, pw / pt, zero)
        K["T1" + name], K["T2" + name] = fg * pw1 * ll, T2
        K["foc" + name] = np.where(valid, (-pw * ll * al).astype(F64) / max(msum, 1.0), 0.0)
    K["perp"], K["perq"] = wi.astype(F64) * Lp.astype(F64) / M, wp.astype(F64) * Lq.astype(F64) / M
    K.update(p=p, q=q, plog=plog, qlog=qlog, xlp=xlp, xlq=xlq, ep=ep, eq=eq, Lp=Lp, Lq=Lq, conf_p=conf_p, conf_q=conf_q, d=d,
             tau=tau, gp=gp, gq=gq, wp=wp, wi=wi, ip=ip, iq=iq, rp=rp, rq=rq, ddp=ddp, ddq=ddq, l38p=l38p, l38q=l38q,
             cnt=cnt, valid=valid, tt=tt, al=al, fg=fg, msum=msum, M=M, dt=f, mut=mut)
    for k in ("a1", "e2", "ep", "d", "wp", "ddp", "T1l"):
        assert K[k].dtype == f, k
    return K


def weights4(x, w6):
    """(w_foc, w_foc_cam, w_per_p, w_per_q) as loss_pixel_k uses them: from w6, or (1, 1, gamma_per, gamma_per)"""
    if w6 is None:
        return (1.0, 1.0, x["gper"], x["gper"])
    return (w6[0], w6[2], w6[4], w6[5])


def combine(x, K, w6, dice=None):
    """gl, gc [P][C] in K's dtype from its pieces: spa (a + b) + spb (e + f), the focal gradient at c = t, the Dice term"""
    f = K["dt"]
    w_fl, w_fc, wa, wb = (f(F32(v)) for v in weights4(x, w6))
    if K["mut"] == "w45_swap":
        wa, wb = wb, wa
    Mf = f(F32(K["M"]))
    spa, spb = wa / Mf, wb / Mf
    valid, tt = K["valid"], K["tt"]
    ar = np.arange(x["P"])[valid]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for h, (s, w_f) in enumerate((("1", w_fl), ("2", w_fc))):
            g = spa * (K["a" + s] + K["b" + s]) + spb * (K["e" + s] + K["f" + s])
            n = "lc"[h]
            if valid.any():
                df = w_f * K["al"] * (K["T1" + n] - K["T2" + n]) / f(F32(K["msum"]))
                g[ar, tt[valid]] = g[ar, tt[valid]] + df[valid]
            if dice is not None:
                C = x["C"]
                row = dice[h]
                two = np.where(np.arange(C)[None, :] == tt[:, None], f(1 if K["mut"] == "dice_one" else 2), f(0))
                add = f(row[1]) * (two - row[2:2 + C].astype(f)[None, :]) * row[2 + C:].astype(f)[None, :]
                g = g + np.where(valid[:, None], add, f(0))
            assert g.dtype == f
            out.append(g)
    return out


def dice_ref(x):
    """float64: parts [nparts][4C] = per tile of 256 pixels {S_lidar, I_lidar, S_camera, I_camera}, dice [2][2 + 2C] = per head
    {L, K / C, dice_c, 1 / D_c}, and their bounds n eps64 sum |terms|"""
    P, C, lab = x["P"], x["C"], x["label"]
    valid = (lab > 0) & (lab < C)
    onehot = (lab[:, None] == np.arange(C)[None, :]) & valid[:, None]
    cols = []
    for r in (x["pp"], x["qq"]):
        s = r.astype(F64) * valid[:, None]
        cols += [s, s * onehot]
    per_pixel = np.concatenate(cols, 1)                                   # [P][4C]
    parts = np.add.reduceat(per_pixel, np.arange(0, P, BLOCK), 0)
    tot = parts.sum(0)
    cnt = histogram(lab, C).astype(F64)
    n = (P + 64) * EPS64
    dice, bound = np.zeros((2, 2 + 2 * C)), np.zeros((2, 2 + 2 * C))
    for h in range(2):
        S, I = tot[2 * C * h:2 * C * h + C], tot[2 * C * h + C:2 * C * h + 2 * C]
        D = S + cnt + 1e-6
        dc = (2 * I + 1e-6) / D
        m = dc.mean()
        nl = -np.log(max(m, 1e-6))
        dice[h, 0] = nl ** 0.3
        dice[h, 1] = 0.0 if m < 1e-6 else -0.3 * nl ** -0.7 / m / C
        dice[h, 2:2 + C], dice[h, 2 + C:] = dc, 1.0 / D
        dnl = (n + 8 * EPS64) * (1.0 + abs(nl))
        bound[h, 0] = 0.3 * nl ** -0.7 * dnl + 8 * EPS64 * dice[h, 0]
        bound[h, 1] = abs(dice[h, 1]) * (0.7 * dnl / nl + n + 16 * EPS64)
        bound[h, 2:2 + C], bound[h, 2 + C:] = n * dc, n / D
    return {"parts": parts, "parts_bound": BLOCK * EPS64 * parts, "dice": dice, "dice_bound": bound, "below": [
        bool(dice[h, 2:2 + C].mean() < 1e-6) for h in range(2)]}


# ------------------------------------------------------------------------------------------------ bounds and margins
def margins(x, K):
    """(dconf_p, dconf_q, dd): the derived absolute errors of a float32 evaluation of the confidences and their difference"""
    C = x["C"]
    logC = float(np.log(C))
    kE = LU + (C + 1) * U
    dcp = kE * np.abs(K["p"] * K["plog"]).sum(1) / logC + (LU + 2 * U) * np.abs(K["ep"]) + U
    dcq = kE * np.abs(K["q"] * K["qlog"]).sum(1) / logC + (LU + 2 * U) * np.abs(K["eq"]) + U
    return dcp, dcq, dcp + dcq + U * np.abs(K["d"])


def in_margin(x, K):
    dcp, dcq, dd = margins(x, K)
    return (np.abs(K["d"]) <= dd) | (np.abs(K["conf_p"] - K["tau"]) <= dcp) | (np.abs(K["conf_q"] - K["tau"]) <= dcq)


def grad_bound(x, K, w6, dice=None, magnitudes=False):
    """the derived bound of every element of gl, gc [P][C] for the weights w6 (module docstring); K: the float64 core.
    magnitudes: return instead the sum of the magnitudes of the element's pieces, (wa (|a| + |b|) + wb (|e| + |f|)) / M +
    w alpha_t (|T1| + |T2|) / (P - cnt[0]) + the Dice term's"""
    C = x["C"]
    logC, M, msum = float(np.log(C)), K["M"], max(K["msum"], 1.0)
    w_fl, w_fc, wa, wb = (abs(float(F32(v))) for v in weights4(x, w6))
    dd = margins(x, K)[2]
    col = lambda v: v[:, None]                                                                              # noqa: E731
    ab = np.abs
    kL = LU + (2 * C + 1) * U
    dLp = kL * (ab(K["xlq"]) + ab(K["q"] * K["plog"])).sum(1)
    dLq = kL * (ab(K["xlp"]) + ab(K["p"] * K["qlog"])).sum(1)
    dddp = (LU * ab(K["plog"]) + (LU + 3 * U) * ab(K["plog"] + K["ip"])) / logC
    dddq = (LU * ab(K["qlog"]) + (LU + 3 * U) * ab(K["qlog"] + K["iq"])) / logC
    gp, gq = K["gp"].astype(F64), K["gq"].astype(F64)

    def ratio_term(w_open, num, rec, t):             # w num / den
        return col(w_open * dd) * num * rec + 3 * U * ab(t)

    def through_weight(gate, dL, L, ddx, dddx, t):   # L gate dd/dx
        return col(gate) * (col(dL) * ab(ddx) + col(ab(L)) * dddx) + 2 * U * ab(t)

    def log_term(gate, w, lx, other, t):             # w (ln x + 1 - other)
        s = lx + 1.0 - other
        ds = LU * (ab(lx) + ab(other)) + 2 * U * (ab(lx) + 1.0 + ab(other))
        return col(gate * dd) * ab(s) + col(w) * ds + U * ab(t)

    out = []
    for h in range(2):
        if h == 0:
            da = ratio_term(gq, K["q"], K["rp"], K["a1"])
            db = through_weight(gq, dLp, K["Lp"], K["ddp"], dddp, K["b1"])
            de = log_term(gp, K["wp"], K["l38p"], K["qlog"], K["e1"])
            df = through_weight(gp, dLq, K["Lq"], K["ddp"], dddp, K["f1"])
            mA, mB = ab(K["a1"]) + ab(K["b1"]), ab(K["e1"]) + ab(K["f1"])
        else:
            da = log_term(gq, K["wi"], K["l38q"], K["plog"], K["a2"])
            db = through_weight(gq, dLp, K["Lp"], K["ddq"], dddq, K["b2"])
            de = ratio_term(gp, K["p"], K["rq"], K["e2"])
            df = through_weight(gp, dLq, K["Lq"], K["ddq"], dddq, K["f2"])
            mA, mB = ab(K["a2"]) + ab(K["b2"]), ab(K["e2"]) + ab(K["f2"])
        b = (wa * (da + db + 4 * U * mA) + wb * (de + df + 4 * U * mB)) / M
        mag = (wa * mA + wb * mB) / M
        n, w_f = "lc"[h], (w_fl, w_fc)[h]
        valid, tt = K["valid"], K["tt"]
        if valid.any():
            fgv = float(K["fg"])
            T1, T2 = ab(K["T1" + n]), ab(K["T2" + n])
            dT = ((abs(fgv - 1) + 2) * U + 2 * LU) * T1 + ((fgv + 1) * U + LU) * T2 + 6 * U * (T1 + T2)
            s = w_f * K["al"].astype(F64) / msum
            ar = np.arange(x["P"])[valid]
            b[ar, tt[valid]] += (s * dT)[valid]
            mag[ar, tt[valid]] += (s * (T1 + T2))[valid]
        if dice is not None:
            row = dice[h]
            two = np.where(np.arange(C)[None, :] == tt[:, None], 2.0, 0.0)
            t = np.where(valid[:, None], abs(row[1]) * (two + row[2:2 + C][None, :]) * row[2 + C:][None, :], 0.0)
            b += 7 * U * t
            mag += t
        out.append(mag if magnitudes else b + 3 * U * mag)
    return out


def instantiation_bound(x, ref):
    """the bound of  <true> gradient - (<false> gradient + Dice term)  per element of gl, gc.  loss_pixel_k<true> and <false>
    are compiled apart, and the compiler may fuse a product into the addition that follows it in one and not in the other
    (a fused product is not rounded), so the part the two share need not come out bit-equal.  What CANNOT differ: the logf /
    powf calls (same function, operands that are inputs or fmaxf of inputs), hence no LU here; and the per-pixel leaves Lp, Lq,
    w_pcd, w_img, which the test sees bit-equal through `rows` (float64 sums of w L).  From equal leaves, one evaluation of
        spa (a + b) + spb (e + f) + dfoc
    rounds: a = (w q) (1 / p) twice, b, e, f once each (dd/dp_c and ln p + 1 - qlog hold no product that feeds an addition:
    the same instructions on the same operands in both), a pair's sum once, the product with spa once: 4 u of |a| + |b|; the
    sum of the two groups and the addition of dfoc once each: 6 u in all.  dfoc = w alpha (T1 - T2) / msum: T1 = g o^(g-1) ln p_t
    two products, the difference (which may take the second product fused), the product with w alpha (itself a product of
    leaves), the division, the addition to the rest: 6 u of w alpha (|T1| + |T2|) / msum.  Two evaluations differ by at most
    twice that: 12 u of the magnitudes grad_bound(magnitudes=True) returns.  The Dice term itself: 7 u of its magnitude
    (module docstring); the addition of it: u of the result, which the caller adds"""
    mags = grad_bound(x, ref["K"], None, magnitudes=True)
    term = grad_bound(x, ref["K"], (0, 0, 0, 0, 0, 0), ref["dice"]["dice"], magnitudes=True)
    return [12 * U * m + 7 * U * t for m, t in zip(mags, term)]


def rows_of(x, K):
    """rows f64[nrows][4] = per block of 256 pixels {foc, foc_cam, per_p, per_q}"""
    v = np.stack([K["focl"], K["focc"], K["perp"], K["perq"]], 1)
    return np.add.reduceat(v, np.arange(0, x["P"], BLOCK), 0)


def rows_bound(x, K, left_out):
    C = x["C"]
    dd = margins(x, K)[2]
    ab = np.abs
    kL = LU + (2 * C + 1) * U
    dLp = kL * (ab(K["xlq"]) + ab(K["q"] * K["plog"])).sum(1)
    dLq = kL * (ab(K["xlp"]) + ab(K["p"] * K["qlog"])).sum(1)
    kf = (float(K["fg"]) + 3) * U + 2 * LU
    gp, gq = K["gp"].astype(F64), K["gq"].astype(F64)
    M = K["M"]
    other = left_out * ab(K["d"]) * (ab(K["Lp"]) + ab(K["Lq"])) / M       # a pixel left out may sit on either side of its gate
    e = np.stack([kf * ab(K["focl"]), kf * ab(K["focc"]),
                  (gq * dd * ab(K["Lp"]) + K["wi"] * dLp) / M + 4 * EPS64 * ab(K["perp"]) + other,
                  (gp * dd * ab(K["Lq"]) + K["wp"] * dLq) / M + 4 * EPS64 * ab(K["perq"]) + other], 1)
    v = np.stack([K["focl"], K["focc"], K["perp"], K["perq"]], 1)
    idx = np.arange(0, x["P"], BLOCK)
    return np.add.reduceat(e, idx, 0) + 2 * BLOCK * EPS64 * np.add.reduceat(ab(v), idx, 0)


# ------------------------------------------------------------------------------------------------ the reference of one case
def keys_of(x):
    """f32 [2C][P]: |fg - p| in float32 (exact: the kernel's own two operations), -1 where the label is 0"""
    lab, C = x["label"], x["C"]
    fg = ((lab[:, None] == np.arange(C)[None, :]) & (lab[:, None] != 0)).astype(F32)
    k = np.concatenate([np.abs(fg - x["pp"]).T, np.abs(fg - x["qq"]).T], 0)
    k[:, lab == 0] = -1
    assert k.dtype == F32
    return np.ascontiguousarray(k)


def confusion_of(x):
    """int64 [2][C][C] (prediction, label) counts over the pixels with 0 <= label < C; the FIRST maximum is the prediction"""
    lab, C = x["label"], x["C"]
    ok = (lab >= 0) & (lab < C)
    out = np.zeros((2, C, C), dtype=np.int64)
    for h, r in enumerate((x["pp"], x["qq"])):
        np.add.at(out[h], (np.argmax(r, 1)[ok], lab[ok]), 1)
    return out


def reference(x, mut=None):
    """the float64 reference of one set of inputs: the float32 restatement's gates (asserted equal to float64's own outside the
    margins by the host test), the pixels that are compared, cnt, keys, confusion matrices, rows and their bound, Dice"""
    K32 = core(x, F32)
    K = core(x, F64, mut=mut, gates=(K32["gp"], K32["gq"]))
    own = core(x, F64)
    mg = in_margin(x, own)
    left_out = mg & ~x["edge"]
    dr = dice_ref(x)
    return {"K": K, "K32": K32, "own_gates": (own["gp"], own["gq"]), "margin": mg, "left_out": left_out, "cmp": ~left_out,
            "cnt": K["cnt"], "rows": rows_of(x, K), "rows_bound": rows_bound(x, own, left_out), "dice": dr, "d_own": own["d"]}


@functools.lru_cache(None)
def case_ref(name):
    ref = reference(inputs(name))
    ref["key"], ref["conf"] = keys_of(inputs(name)), confusion_of(inputs(name))
    return ref


WSPECS = {"foc": UNIT["foc"], "foc_cam": UNIT["foc_cam"], "per_p": UNIT["per_p"], "per_q": UNIT["per_q"], "w6": W6, "plain": None}


def grad_ref(x, ref, spec, mutant=None):
    """(gl, gc, bound_gl, bound_gc) [P][C] float64 for one of WSPECS, or 'dice' (the unweighted call with the Dice term) or
    'dice_term' (the Dice term alone).  mutant: a reference() of a MUTANT, evaluated under the true reference's bounds"""
    K = (mutant or ref)["K"]
    dice = ref["dice"]["dice"] if spec in ("dice", "dice_term") else None
    w6 = (0, 0, 0, 0, 0, 0) if spec == "dice_term" else WSPECS["plain" if spec == "dice" else spec]
    gl, gc = combine(x, K, w6, dice)
    bl, bc = grad_bound(x, ref["K"], w6, dice)
    return gl, gc, bl, bc


def worst_ratio(got, want, bound, rows=None):
    """max |got - want| / bound over the compared rows; an element whose bound is 0 must be exact; anything not finite: inf"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    if rows is not None:
        got, want, bound = got[rows], want[rows], bound[rows]
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    e = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e == 0, 0.0, e / bound)
    return float(r.max())


def restate32(x, ref, spec):
    """gl, gc of the float32 restatement for one spec"""
    dice = ref["dice"]["dice"] if spec in ("dice", "dice_term") else None
    w6 = (0, 0, 0, 0, 0, 0) if spec == "dice_term" else WSPECS["plain" if spec == "dice" else spec]
    return combine(x, ref["K32"], w6, dice)


QUANTITY = {"foc": "grad_foc", "foc_cam": "grad_foc", "per_p": "grad_per", "per_q": "grad_per", "w6": "grad_total",
            "plain": "grad_total", "dice": "grad_dice", "dice_term": "grad_dice"}


def measure(name):
    """worst error / bound of the float32 restatement on one case, per quantity of MEASURED"""
    x, ref = inputs(name), case_ref(name)
    out = dict.fromkeys(MEASURED, 0.0)
    for spec, qty in QUANTITY.items():
        if name in DICE_NAMES and spec != "dice":             # (the Dice cases are there for the Dice term)
            continue
        gl, gc, bl, bc = grad_ref(x, ref, spec)
        rl, rc = restate32(x, ref, spec)
        out[qty] = max(out[qty], worst_ratio(rl, gl, bl, ref["cmp"]), worst_ratio(rc, gc, bc, ref["cmp"]))
    out["rows"] = worst_ratio(rows_of(x, ref["K32"]), ref["rows"], ref["rows_bound"])
    return out


def mutant_ratio(name, mut):
    """how far (in bounds) the wrong variant `mut` of the reference is from the reference on one case, worst quantity"""
    x, ref = inputs(name), case_ref(name)
    wrong = reference(x, mut)
    worst = worst_ratio(wrong["rows"], ref["rows"], ref["rows_bound"])
    for spec in QUANTITY:
        gl, gc, bl, bc = grad_ref(x, ref, spec)
        ml, mc, _, _ = grad_ref(x, ref, spec, mutant=wrong)
        worst = max(worst, worst_ratio(ml, gl, bl, ref["cmp"]), worst_ratio(mc, gc, bc, ref["cmp"]))
    return worst
