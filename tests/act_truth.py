"""Float64 truth, cases and per-element bars for gsrast.activations.gaussian_activations (csrc/gsr_extra.hip k_gauss_act_fwd / k_gauss_act_bwd):

    scaling = exp(s)      rotation = q / max(|q|, 1e-12f)      opacity = 1 / (1 + exp(-o))
    d s = g_s * scaling   d q = (g_q - r <r, g_q>) / |q|   (|q| > 1e-12f;  g_q / 1e-12f where the norm is clamped)   d o = g_o * a * (1 - a)

Truth is numpy float64 on the float32 inputs.  The clamp DECISION is taken from the float32 norm, computed op by op as the kernel does (four
squares, three additions left to right, a square root): a row whose float64 norm lies within 8 float32 steps of 1e-12f is "fragile" and may take
either branch (whole row); the builder keeps such rows to at most 4 per case.

Bars, per element:  |cand - truth| <= K * max(2^-24 * scale, 2^-149),  scale = the sum of the magnitudes of the formula's terms, K = twice the number
of float32 roundings on the path.  A rounding is half an ulp, 2^-24 relative; expf, the division and sqrt are taken as 1 ulp, that is as two
roundings each.  2^-149 is the spacing of the float32 denormals, below which no scale can push a rounding.
    scaling      K = 4   (expf: 2)                                                            scale |e^s|
    opacity      K = 10  (expf: 2, the addition, the division: 2)                             scale a
    d scaling    K = 6   (expf: 2, the product)                                               scale |g| e^s
    d opacity    K = 16  (a: 5, 1 - a, two products)                                          scale |g| a (1 + a)     [g a - g a a]
    rotation     K = 22  (4 squares, 3 additions, sqrt: 2, the division: 2)                   scale |r_i|
    d rotation   K = 62  (r: 11; <r,g>: 4 products, 3 additions; r_i dot; the difference; |q| again: 9; the division: 2)
                                                                                              scale (|g_i| + |r_i| |<r,g>|) / |q|
A truth beyond the float32 range (exp(89)) demands the infinity of its sign, and so does the gradient of such an element (g * inf: the
backward multiplies by the float32 output, as the reference's exp does).  Where the yardstick -- torch's own float32 exp / F.normalize /
sigmoid and their autograd on the same device -- itself misses K / 2 against the same truth, the bar of that element is twice the yardstick's
error (check() prints the element); a fragile row's bars are never widened.  On the MI355X no element's bar was.

Worst observed error in units of the bars, all cases of tests/test_gpu_activations.py on the MI355X (kernel | torch's formulation):
    scaling 0.32 | 0.32    opacity 0.19 | 0.19    d scaling 0.35 | 0.35    d opacity 0.21 | 0.18    rotation 0.13 | 0.11    d rotation 0.56 | 0.31"""
import numpy as np

EPS = np.float32(1e-12)
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
K = {"scaling": 4, "opacity": 10, "d_scaling": 6, "d_opacity": 16, "rotation": 22, "d_rotation": 62}
SIZES = (1, 255, 256, 257, 4099)
FRAGILE_STEPS = 8
SCALING_SPECIAL = (-87.0, 88.0, 89.0, -104.0, 0.0, -86.5, 87.5)
OPACITY_SPECIAL = (0.0, 1e-8, -1e-8, 16.6, -16.6, 17.4, -17.4, 88.0, -88.0, 104.0, -104.0)


def norm_f32(q):
    """|q| as the kernel computes it: every operation rounded to float32, the additions left to right."""
    q = q.astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        sq = (q * q).astype(np.float32)
        return np.sqrt(((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32) + sq[:, 3]).astype(np.float32)


def make_case(P, S, seed, absent=None):
    """Float32 inputs and upstream gradients built from the seed.  The special rows come first, rotated by the seed so that P = 1 sees a different
    one per seed.  absent: the name of an upstream gradient that the loss does not produce ("scaling" | "rotation" | "opacity")."""
    r = np.random.default_rng(seed)
    s = r.uniform(-87.0, 88.0, (P, S))
    o = r.normal(0.0, 4.0, (P, 1))
    d = r.normal(size=(P, 4)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    q = d * r.uniform(0.5, 2.0, (P, 1))
    quats = []
    for k, n in enumerate((np.nextafter(EPS, np.float32(0)), EPS, np.nextafter(EPS, np.float32(1)))):        # the clamp and its two neighbours, on an axis
        v = np.zeros(4); v[k + 1] = float(n) * (-1.0) ** k
        quats.append(v)
    quats.append(np.zeros(4))
    for n in (1e-18, 1e18):                                          # the ends of the range in which the squares stay normal
        v = r.normal(size=4)
        quats.append(v / np.linalg.norm(v) * n)
    shift = seed % 7
    for i in range(P):
        j = i + shift
        if j < len(SCALING_SPECIAL):
            s[i, i % S] = SCALING_SPECIAL[j]
        if j < len(OPACITY_SPECIAL):
            o[i, 0] = OPACITY_SPECIAL[j]
        if j < len(quats):
            q[i] = quats[j]
    s, q, o = s.astype(np.float32), q.astype(np.float32), o.astype(np.float32)
    g = {"scaling": r.normal(size=(P, S)).astype(np.float32), "rotation": r.normal(size=(P, 4)).astype(np.float32), "opacity": r.normal(size=(P, 1)).astype(np.float32)}
    row = P - 1                                                       # one upstream gradient parallel to r: the projection cancels
    n = norm_f32(q[row:row + 1])[0]
    if n > EPS:
        g["rotation"][row] = (np.float32(3.0) * (q[row] / n)).astype(np.float32)
    if absent is not None:
        g[absent] = None
    return {"s": s, "q": q, "o": o, "g": g, "P": P, "S": S}


def truth(c):
    """-> {output: (truth float64, scale float64)}, clamped [P] (the float32 decision), fragile [P], and for fragile rows the other branch:
    other = {"rotation": ..., "d_rotation": ...} (truth, scale) evaluated with the opposite decision."""
    s, q, o = (c[k].astype(np.float64) for k in ("s", "q", "o"))
    g = {k: (None if v is None else v.astype(np.float64)) for k, v in c["g"].items()}
    zero = lambda a: np.zeros_like(a)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(s)
        a = 1.0 / (1.0 + np.exp(-o))
        out = {"scaling": (e, np.abs(e)), "opacity": (a, a)}
        e_out = np.where(e > FLT_MAX * (1.0 + U), np.inf, e)      # d s = g * scaling, scaling the float32 OUTPUT: an overflowed exp gives g * inf
        out["d_scaling"] = (zero(e), zero(e)) if g["scaling"] is None else (g["scaling"] * e_out, np.abs(g["scaling"]) * e_out)
        out["d_opacity"] = (zero(a), zero(a)) if g["opacity"] is None else (g["opacity"] * a * (1.0 - a), np.abs(g["opacity"]) * a * (1.0 + a))
        n64 = np.sqrt((q * q).sum(1))
        clamped = ~(norm_f32(c["q"]) > EPS)
        step = float(np.nextafter(EPS, np.float32(1)) - EPS)
        fragile = np.abs(n64 - float(EPS)) <= FRAGILE_STEPS * step

        def rot(cl):
            den = np.where(cl, float(EPS), n64)[:, None]
            rr = q / den
            if g["rotation"] is None:
                return (rr, np.abs(rr)), (zero(q), zero(q))
            gq = g["rotation"]
            dot = (rr * gq).sum(1, keepdims=True)
            full = ((gq - rr * dot) / den, (np.abs(gq) + np.abs(rr) * np.abs(dot)) / den)
            flat = (gq / float(EPS), np.abs(gq) / float(EPS))
            pick = lambda x, y: np.where(cl[:, None], x, y)
            return (rr, np.abs(rr)), (pick(flat[0], full[0]), pick(flat[1], full[1]))
        out["rotation"], out["d_rotation"] = rot(clamped)
        other = dict(zip(("rotation", "d_rotation"), rot(~clamped)))
    return out, clamped, fragile, other


def eval_f32(c, defect=None):
    """The kernels' formulas in numpy float32, op by op.  defect: None | "no_projection" | "clamp_1e-6" | "a_not_a(1-a)" (planted, for the CPU test)."""
    f = np.float32
    s, q, o, g = c["s"], c["q"], c["o"], c["g"]
    eps = f(1e-6) if defect == "clamp_1e-6" else EPS
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(s).astype(f)
        a = (f(1.0) / (f(1.0) + np.exp(-o).astype(f)).astype(f)).astype(f)
        n = norm_f32(q)
        rr = (q / np.maximum(n, eps)[:, None]).astype(f)
        out = {"scaling": e, "opacity": a, "rotation": rr}
        out["d_scaling"] = np.zeros_like(e) if g["scaling"] is None else (g["scaling"] * e).astype(f)
        if g["opacity"] is None:
            out["d_opacity"] = np.zeros_like(a)
        elif defect == "a_not_a(1-a)":
            out["d_opacity"] = (g["opacity"] * a).astype(f)
        else:
            out["d_opacity"] = ((g["opacity"] * a).astype(f) * (f(1.0) - a).astype(f)).astype(f)
        if g["rotation"] is None:
            out["d_rotation"] = np.zeros_like(q)
        else:
            gq = g["rotation"]
            pr = (rr * gq).astype(f)
            dot = (((pr[:, 0] + pr[:, 1]).astype(f) + pr[:, 2]).astype(f) + pr[:, 3]).astype(f)[:, None]
            if defect == "no_projection":
                dot = np.zeros_like(dot)
            full = ((gq - (rr * dot).astype(f)).astype(f) / n[:, None]).astype(f)
            flat = (gq * f(1e12)).astype(f) if defect != "clamp_1e-6" else (gq * f(1e6)).astype(f)
            out["d_rotation"] = np.where((n > eps)[:, None], full, flat)
    return out


def _units(cand, tr, scale, k, yard=None, what="", firm=None):
    """|cand - tr| in units of the element's bar (inf where an infinity or a NaN is missed).  firm [P]: rows whose bar the yardstick never widens."""
    cand = cand.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        bar = k * np.maximum(U * scale, TINY)
        if yard is not None:
            yerr = np.abs(yard.astype(np.float64) - tr)
            wide = np.isfinite(yerr) & (yerr > 0.5 * bar)
            if firm is not None:
                wide &= ~firm.reshape((-1,) + (1,) * (wide.ndim - 1))
            for i in np.argwhere(wide)[:8]:
                print(f"  yardstick beyond K/2 at {what}{tuple(i)}: truth {tr[tuple(i)]!r} torch {yard[tuple(i)]!r} ({yerr[tuple(i)] / bar[tuple(i)] * k:.1f} of {k}): bar doubled to its error")
            bar = np.where(wide, 2.0 * yerr, bar)
        over = np.abs(tr) > FLT_MAX * (1.0 + U)
        units = np.abs(cand - tr) / bar
        units = np.where(over, np.where(cand == np.sign(tr) * np.inf, 0.0, np.inf), units)
        units = np.where(np.isfinite(cand) | over, units, np.inf)
    return units


def check(c, cand, yard=None, raise_on_miss=True):
    """cand / yard: {output: float32 array}.  -> {output: worst |error| in units of its bar}; raises AssertionError on the first output that misses."""
    tr, clamped, fragile, other = truth(c)
    assert int(fragile.sum()) <= 4, f"the builder made {int(fragile.sum())} fragile rows"
    worst, missed = {}, []
    for name, (t, scale) in tr.items():
        y = None if yard is None or yard.get(name) is None else yard[name]
        u = _units(cand[name], t, scale, K[name], y, what=name, firm=fragile)      # a fragile row has its own rule: the yardstick may sit on its other branch
        if name in other and fragile.any():                        # a fragile row may take the other branch, as a whole
            u2 = _units(cand[name], other[name][0], other[name][1], K[name])
            row, row2 = u.max(1), u2.max(1)
            u = np.where((fragile & (row2 < row))[:, None], u2, u)
        worst[name] = float(u.max()) if u.size else 0.0
        if not worst[name] <= 1.0:
            i = np.unravel_index(int(np.argmax(u)), u.shape)
            missed.append(f"{name}{tuple(int(v) for v in i)}: got {cand[name][i]!r}, truth {t[i]!r}, {worst[name]:.3g} bars (K = {K[name]})")
    if missed and raise_on_miss:
        raise AssertionError("; ".join(missed))
    return worst
