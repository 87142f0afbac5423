"""The PGSR multi-view losses (geometric consistency + patch NCC) stated in float64, with every decision a float32 rounding can flip named and
measured, and the checker that holds a float32 result -- the HIP kernels', the C oracle's -- to it element by element.

The truth is tests/ref_mv_torch.py in float64 (the reference's formulas, through world coordinates, torch autograd for the gradients, masks and
weights detached) on the float32 inputs widened exactly.  `evaluate` adds, per pixel, the distance from every gate:
  frustum  min(|u|, |u - Wn|, |v|, |v - Hn|)      pixels       feeds d_mask, weight, count, sum, the pixel's gradients
  qz       |q.z - 0.1|                                          the same
  th       |noise - noise_th|                     pixels       the same
  noise0   noise itself                           pixels       feeds the gradients only: the direction e / noise loses its digits
  clamp    min(|u|, |u - (Wn-1)|, |v|, |v - (Hn-1)|)            gradients only: mu / mv switch, the value is continuous
  cell     |uc - rint(uc)|, |vc - rint(vc)| (not where the coordinate is clamped: there it IS the integer, on both sides)   gradients only: the
           tap set and the coordinate gradient change, the value does not
and per sample:
  kappa    max(sum r^2 / rvar, sum n^2 / nvar): the cancellation factor of the two variances (1 for a single tap and for a patch with every tap
           beyond doubt in the zero padding: both variances are 0 in any arithmetic).  unit = kappa ntap 2^-24 + WARP_ERR * sum |d ncc / d tap
           coordinate|: what one float32 summation of the patch costs ncc, plus what the float32 error of the warped coordinates costs it (autograd
           of the truth; it matters for a tap in the padding strip, where the bilinear value falls from the texel to 0 within one cell)
  0.9      |ncc - 0.9| / unit        feeds ncc_mask, count, sum, the sample's gradients
  clamp02  min(|raw|, |raw - 2|) / unit with raw = 1 - cc before the clamp      gradients only
  tap      the distance of any warped tap near the image from a cell edge (the padding edges -1, W-1, H-1 are cell edges)   gradients only
  g2       min over taps of |g2|, the homography's third row                    value and gradients
A pixel / sample is ROBUST when every margin exceeds its bound, FRAGILE otherwise, with the name of the closest gate.  Non-finite u, v, q.z or
noise switch a pixel off beyond doubt (comparisons with NaN are false): such a pixel is robust and off.  A near-map texel is robust when no
fragile pixel can scatter into it.

BOUND is measured, never taken from the HIP library: per quantity, the largest deviation of the float32 C oracle (oracle/gsm_oracle.c, the
-ffp-contract=off build and its FMA twin; for ncc also a numpy float32 evaluation in the kernel's summation order: taps strided over 16 lanes,
then a four-level pairwise tree) from this truth over every case of mv_cases.NAMES, times 4, rounded up to a round figure.
tests/test_mv_truth_cpu.py measures them again on every run and fails if 4 x a deviation exceeds its bound.

Units.  u, v, noise, warp: pixels.  weight: absolute.  ncc: ratio to unit.  The gradients are not proportional to their own size: the geometric
loss differentiates |e|, whose direction e / noise carries the ABSOLUTE float32 error of e (a few ulps of a pixel coordinate) divided by noise,
and e . J cancels.  So
  g_depth[p] is held to   BOUND['g_geo'] * w (|d ex / d depth| + |d ey / d depth|) / min(noise, 1), each derivative taken as the sum of the
                          magnitudes of its two paths (direct, and through the sampled depth mz: they nearly cancel where the two views agree)
  g_near[t]  is held to   BOUND['g_geo'] * sum over the pixels that tap t of tapweight * w (|d ex / d mz| + |d ey / d mz|) / min(noise, 1) + |dmz|
                          (the second term: the tap weight itself carries the error of u, v, also where it is almost 0)
(BOUND['g_geo'] is in pixels, like the error of e), and the NCC gradients of a sample, four numbers, to
  BOUND['g_ncc'] * unit * (max |truth| + floor)   with floor = the case's median of max |truth| over its gradient-robust samples.
"""
import numpy as np
import torch

import oracle
import oracle_multiview as om
import ref_mv_torch

EPS24 = 2.0 ** -24
NOISE0_FACTOR = 16           # noise <= 16 x BOUND['noise']: the first-order bound on the direction's error (error of e / noise) no longer holds
# quantity -> largest measured oracle deviation (test_mv_truth_cpu.py -s prints them; EXPERIMENTS.md keeps the table) and bound >= 4 x that
MEASURED = dict(u=1.43e-5, qz=4.3e-7, noise=1.77e-5, weight=1.66e-5, warp=2.91e-5, g2=2.2e-7, ncc=0.39, ncc_device_order=0.38, g_geo=1.06e-5, g_ncc=4.4)
BOUND = dict(u=6e-5, qz=2e-6, noise=8e-5, weight=7e-5, warp=1.2e-4, g2=1e-6, ncc=1.6, g_geo=4.5e-5, g_ncc=20.0)
WARP_ERR = 3e-5              # pixels: what a float32 evaluation of a warped tap coordinate is off by (MEASURED['warp']; the CPU test holds it)
GEO_VALUE_GATES, GEO_GRAD_GATES = ("frustum", "qz", "th"), ("noise0", "clamp", "cell")


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=grad)


def evaluate(case, indices="case"):
    """-> dict of numpy arrays: the truth, its margins and the scales of the per-element bounds (module text).  indices: int32 sample slots,
    None = every pixel of the truth's d_mask, 'case' = the case's own list."""
    W, H = case["W"], case["H"]
    patch, th, s = int(case.get("patch", 3)), float(case.get("noise_th", 1.0)), float(case.get("ncc_scale", 1.0))
    Hn, Wn = case["near_plane_depth"].shape[-2:]
    Hg, Wg = case["gray"].shape[-2:]
    lv = {k: _t64(case[k], True) for k in ("plane_depth", "near_plane_depth", "rendered_normal", "rendered_distance")}
    if isinstance(indices, str):
        indices = case.get("indices")
    parts = {}
    idx_t = None if indices is None else torch.tensor(np.asarray(indices, np.int64))
    with np.errstate(all="ignore"):
        ref_mv_torch.multiview_loss(lv["plane_depth"], lv["near_plane_depth"], lv["rendered_normal"], lv["rendered_distance"], _t64(case["gray"]),
                                    _t64(case["near_gray"]), case["view"], case["near"], patch=patch, th=th, indices=idx_t, dtype=torch.float64,
                                    ncc_scale=s, parts=parts, guarded=True)
    grad = lambda out, inp: torch.autograd.grad(out, inp, retain_graph=True, allow_unused=True)
    zero_like = lambda g, like: (torch.zeros_like(like) if g is None else g).detach().numpy()
    HW = W * H
    g_depth, g_near = grad(parts["geo_sum"], [lv["plane_depth"], lv["near_plane_depth"]])
    ex, ey = parts["err"][:, 0], parts["err"][:, 1]
    fin_e = torch.isfinite(ex) & torch.isfinite(ey)
    exs, eys = torch.where(fin_e, ex, torch.zeros_like(ex)).sum(), torch.where(fin_e, ey, torch.zeros_like(ey)).sum()
    jxd, jxm = grad(exs, [lv["plane_depth"], parts["map_z"]])
    jyd, jym = grad(eys, [lv["plane_depth"], parts["map_z"]])
    (dmz,) = grad(parts["geo_sum"], [parts["map_z"]])
    pu, pv = parts["proj"][:, 0], parts["proj"][:, 1]
    fin_p = torch.isfinite(pu) & torch.isfinite(pv)
    (du_dd,) = grad(torch.where(fin_p, pu, torch.zeros_like(pu)).sum(), [lv["plane_depth"]])
    (dv_dd,) = grad(torch.where(fin_p, pv, torch.zeros_like(pv)).sum(), [lv["plane_depth"]])
    n = lambda a: a.detach().numpy().reshape(-1)
    u, v, qz, noise = n(parts["proj"][:, 0]), n(parts["proj"][:, 1]), n(parts["qz"]), n(parts["noise"])
    frustum, d_mask, w = n(parts["frustum"]), n(parts["d_mask"]), n(parts["weights"])
    with np.errstate(all="ignore"):
        finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(qz)
        inf = np.full(HW, np.inf)
        m = {}
        m["frustum"] = np.where(finite, np.minimum(np.minimum(np.abs(u), np.abs(u - Wn)), np.minimum(np.abs(v), np.abs(v - Hn))), inf)
        m["qz"] = np.where(finite, np.abs(qz - float(np.float32(0.1))), inf)
        # a pixel beyond doubt outside the frustum never reaches the later gates
        out_sure = ~finite | (~frustum & ((m["frustum"] > BOUND["u"]) | ~(qz > 0.1)) & (m["qz"] > BOUND["qz"]))
        noise_ok = np.isfinite(noise)
        m["th"] = np.where(out_sure | ~noise_ok, inf, np.abs(noise - float(np.float32(th))))
        off_sure = out_sure | ~noise_ok | (~d_mask & (m["th"] > BOUND["noise"]) & (m["frustum"] > BOUND["u"]) & (m["qz"] > BOUND["qz"]))
        m["noise0"] = np.where(off_sure, inf, noise)
        cu, cv = (u < 0) | (u > Wn - 1), (v < 0) | (v > Hn - 1)
        m["clamp"] = np.where(off_sure, inf, np.minimum(np.minimum(np.abs(u), np.abs(u - (Wn - 1))), np.minimum(np.abs(v), np.abs(v - (Hn - 1)))))
        uc, vc = np.clip(np.nan_to_num(u), 0, Wn - 1), np.clip(np.nan_to_num(v), 0, Hn - 1)
        m["cell"] = np.where(off_sure, inf, np.minimum(np.where(cu, np.inf, np.abs(uc - np.rint(uc))), np.where(cv, np.inf, np.abs(vc - np.rint(vc)))))
    bound_of = dict(frustum=BOUND["u"], qz=BOUND["qz"], th=BOUND["noise"], noise0=NOISE0_FACTOR * BOUND["noise"], clamp=BOUND["u"], cell=BOUND["u"])
    value_robust = np.all([m[g] > bound_of[g] for g in GEO_VALUE_GATES], axis=0)
    grad_robust = value_robust & np.all([m[g] > bound_of[g] for g in GEO_GRAD_GATES], axis=0)
    rel = np.stack([m[g] / bound_of[g] for g in GEO_VALUE_GATES + GEO_GRAD_GATES], 1)
    closest = np.array(GEO_VALUE_GATES + GEO_GRAD_GATES)[np.argmin(rel, axis=1)]
    # scales of the per-element gradient bounds
    wj = np.where(d_mask, w / np.minimum(np.where(noise > 0, noise, 1.0), 1.0), 0.0)
    nz = lambda g, like: np.nan_to_num(zero_like(g, like).reshape(-1))
    # d e / d depth is a direct path plus one through the sampled depth mz; with consistent geometry the two nearly cancel, the errors do not
    (dmz_dd,) = grad(torch.where(torch.isfinite(parts["map_z"]), parts["map_z"], torch.zeros_like(parts["map_z"])).sum(), [lv["plane_depth"]])
    via_x, via_y = nz(jxm, parts["map_z"]) * nz(dmz_dd, lv["plane_depth"]), nz(jym, parts["map_z"]) * nz(dmz_dd, lv["plane_depth"])
    tot_x, tot_y = nz(jxd, lv["plane_depth"]), nz(jyd, lv["plane_depth"])
    scale_depth = wj * (np.abs(tot_x - via_x) + np.abs(via_x) + np.abs(tot_y - via_y) + np.abs(via_y))
    dmz_n = nz(dmz, parts["map_z"])
    per_mz = wj * (np.abs(nz(jxm, parts["map_z"])) + np.abs(nz(jym, parts["map_z"])))
    x0, y0 = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
    ax, ay = uc - x0, vc - y0
    scale_near = np.zeros(Wn * Hn)
    touched = np.zeros(Wn * Hn, bool)                # by a pixel that is not gradient-robust and may be on: conservative footprint
    live = d_mask | ~off_sure
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            ok = d_mask & (x0 + dx < Wn) & (y0 + dy < Hn)
            np.add.at(scale_near, ((y0 + dy) * Wn + x0 + dx)[ok], (per_mz * wx * wy + np.abs(dmz_n))[ok])
    frag = np.nonzero(live & ~grad_robust)[0]
    for p in frag:
        xs = np.arange(max(x0[p] - 1, 0), min(x0[p] + 3, Wn)); ys = np.arange(max(y0[p] - 1, 0), min(y0[p] + 3, Hn))
        touched[(ys[:, None] * Wn + xs[None, :]).reshape(-1)] = True
    out = dict(W=W, H=H, Wn=Wn, Hn=Hn, Wg=Wg, Hg=Hg, patch=patch, u=u, v=v, qz=qz, noise=noise, frustum=frustum, d_mask=d_mask, weights=w,
               geo_sum=float(parts["geo_sum"].detach()), geo_count=int(parts["geo_count"]), g_depth=zero_like(g_depth, lv["plane_depth"]).reshape(-1),
               g_near=zero_like(g_near, lv["near_plane_depth"]).reshape(-1), margins=m, value_robust=value_robust, grad_robust=grad_robust,
               closest=closest, dmz=dmz_n, du_dd=nz(du_dd, lv["plane_depth"]), dv_dd=nz(dv_dd, lv["plane_depth"]), scale_depth=scale_depth, scale_near=scale_near, near_robust=~touched, x0=x0, y0=y0, in_frustum=int(frustum.sum()))
    # ------------------------------------------------------------------------------------------------------------------------- samples
    if indices is None:
        indices = np.nonzero(d_mask)[0]
    idx = np.asarray(indices, np.int64).reshape(-1)
    N, ntap = idx.size, (2 * patch + 1) ** 2
    used = np.nonzero(idx >= 0)[0]
    z = lambda fill=0.0, dt=np.float64: np.full(N, fill, dt)
    ncc, raw, nmask, kappa, wsens = z(), z(1.0), z(False, bool), z(np.inf), z()
    m09, mcl, mtap, mg2 = z(np.inf), z(np.inf), z(np.inf), z(np.inf)
    gN, gD = np.zeros((3, HW)), np.zeros(HW)
    defined = np.zeros(N, bool)
    if used.size and "ncc" in parts:
        gn_, gd_ = grad(parts["ncc_sum"], [lv["rendered_normal"], lv["rendered_distance"]])
        gN, gD = zero_like(gn_, lv["rendered_normal"]).reshape(3, HW), zero_like(gd_, lv["rendered_distance"]).reshape(-1)
        with np.errstate(all="ignore"):
            ncc[used], raw[used], nmask[used] = n(parts["ncc"]), n(parts["ncc_raw"]), n(parts["ncc_mask"])
            fin_r = torch.isfinite(parts["ncc_raw"])
            (dw_,) = grad(torch.where(fin_r, parts["ncc_raw"], torch.zeros_like(parts["ncc_raw"])).sum(), [parts["warp"]])
            wsens[used] = 0.0 if dw_ is None else np.nan_to_num(np.abs(dw_.numpy()).sum(axis=(1, 2)))
            r2, n2, rvar, nvar = (n(parts[k]) for k in ("r2", "n2", "rvar", "nvar"))
            kr = np.where(rvar > 0, r2 / rvar, np.inf); kn = np.where(nvar > 0, n2 / nvar, np.inf)
            kappa[used] = 1.0 if ntap == 1 else np.maximum(np.maximum(kr, kn), 1.0)      # one tap: both variances are r r - r r, the 1e-8 rules
            warp, g2 = parts["warp"].detach().numpy(), parts["g2"].numpy()
            defined[used] = np.isfinite(warp).all(axis=(1, 2)) & np.isfinite(g2).all(axis=1) & np.isfinite(n(parts["ncc_raw"]))
            near_img = (warp[..., 0] > -1.5) & (warp[..., 0] < Wg + 0.5) & (warp[..., 1] > -1.5) & (warp[..., 1] < Hg + 0.5)
            dist_edge = np.minimum(np.abs(warp[..., 0] - np.rint(warp[..., 0])), np.abs(warp[..., 1] - np.rint(warp[..., 1])))
            mtap[used] = np.where(near_img, dist_edge, np.inf).min(axis=1)
            b = BOUND["warp"]                        # every tap beyond doubt in the zero padding: all n are 0 exactly, ncc == 1 in any arithmetic
            all_out = ((warp[..., 0] < -1 - b) | (warp[..., 0] > Wg + b) | (warp[..., 1] < -1 - b) | (warp[..., 1] > Hg + b)).all(axis=1)
            kappa[used] = np.where(all_out, 1.0, kappa[used])
            mg2[used] = np.abs(g2).min(axis=1)
    unit = kappa * ntap * EPS24 + WARP_ERR * wsens
    with np.errstate(all="ignore"):
        m09 = np.where(np.isfinite(unit), np.abs(ncc - float(np.float32(0.9))) / unit, 0.0)
        mcl = np.where(np.isfinite(unit), np.minimum(np.abs(raw), np.abs(raw - 2.0)) / unit, 0.0)
    m09[idx < 0] = np.inf; mcl[idx < 0] = np.inf
    pix = np.where(idx >= 0, idx, 0)
    weight_robust = (idx < 0) | value_robust[pix]
    s_value_robust = (idx < 0) | (defined & (m09 > BOUND["ncc"]) & (mg2 > BOUND["g2"]))
    s_grad_robust = s_value_robust & weight_robust & (mcl > BOUND["ncc"]) & (mtap > BOUND["warp"])
    gmax = np.abs(np.concatenate([gN[:, pix], gD[None, pix]], 0)).max(axis=0)
    live_s = (idx >= 0) & s_grad_robust & nmask & (w[pix] > 0) & (raw > 0) & (raw < 2)
    floor = float(np.median(gmax[live_s])) if live_s.any() else 0.0
    out.update(indices=idx.astype(np.int32), N=N, ntap=ntap, ncc=ncc, ncc_raw=raw, ncc_mask=nmask, kappa=kappa, unit=unit, defined=defined,
               s_margins=dict(gate09=m09, clamp02=mcl, tap=mtap, g2=mg2), s_value_robust=s_value_robust, s_grad_robust=s_grad_robust,
               weight_robust=weight_robust, g_normal=gN, g_dist=gD, grad_floor=floor, ncc_sum=float(parts["ncc_sum"].detach()), ncc_count=int(parts["ncc_count"]),
               warp=parts.get("warp").detach().numpy() if "warp" in parts else None, warp_sens=wsens, g2=parts.get("g2").numpy() if "g2" in parts else None, used=used,
               ref_val=parts["ref_val"].numpy() if "ref_val" in parts else None, samp=parts["samp"].numpy() if "samp" in parts else None)
    return out


# ------------------------------------------------------------------------------------------------------------- float32 candidates (CPU)
def oracle_cfg(case):
    Hn, Wn = case["near_plane_depth"].shape[-2:]
    Hg, Wg = case["gray"].shape[-2:]
    return om.make_cfg(case["W"], case["H"], case["view"], case["near"], Wn=Wn, Hn=Hn, Wg=Wg, Hg=Hg, ncc_scale=float(case.get("ncc_scale", 1.0)),
                       noise_th=float(case.get("noise_th", 1.0)), patch=int(case.get("patch", 3)))


def oracle_candidate(case, indices, fma=False):
    """The C oracle's result in the layout `deviations` takes (its NCC on its own geo weights, as the device does), plus its float32 u, v, q.z
    and warped taps."""
    def run():
        cfg = oracle_cfg(case)
        g = om.geo(cfg, case["plane_depth"], case["near_plane_depth"])
        idx = np.asarray(indices, np.int32)
        c = om.ncc(cfg, idx, g["weight"], case["rendered_normal"], case["rendered_distance"], case["gray"], case["near_gray"])
        u, v, qz = om.proj(cfg, case["plane_depth"])
        wp = om.warp(cfg, idx, case["rendered_normal"], case["rendered_distance"])
        return dict(noise=g["noise"], d_mask=g["dmask"].astype(bool), weights=g["weight"], geo_sum=float(g["stats"][0]), geo_count=int(g["stats"][1]),
                    g_depth=g["g_depth"], g_near=g["g_near"], ncc=c["ncc"], ncc_mask=c["mask"].astype(bool), ncc_sum=float(c["stats"][0]),
                    ncc_count=int(c["stats"][1]), g_normal=c["g_normal"], g_dist=c["g_dist"], u=u, v=v, qz=qz, warp=wp)
    if fma:
        with oracle.fma_twin():
            return run()
    return run()


def device_order_ncc(truth):
    """ncc per used sample from the truth's taps rounded to float32, the five sums in the kernel's order (lane l adds taps l, l + 16, ... in
    turn; the 16 lane sums meet in a four-level pairwise tree), the rest in float32 as the kernel writes it.  -> float32 [N] (0 in unused slots)"""
    f = np.float32
    r, nn = truth["ref_val"].astype(f), truth["samp"].astype(f)
    ntap = r.shape[1]

    def sum16(a):
        lanes = np.zeros((a.shape[0], 16), f)
        for j in range(ntap):
            lanes[:, j % 16] = lanes[:, j % 16] + a[:, j]
        for step in (1, 2, 4, 8):
            lanes = lanes + lanes[:, np.arange(16) ^ step]
        return lanes[:, 0]
    Sr, Sn, Srr, Snn, Srn = sum16(r), sum16(nn), sum16(r * r), sum16(nn * nn), sum16(r * nn)
    tps = f(ntap)
    ravg, navg = Sr / tps, Sn / tps
    cross, rvar, nvar = Srn - navg * Sr, Srr - ravg * Sr, Snn - navg * Sn
    with np.errstate(all="ignore"):
        ncc = np.clip(f(1) - cross * cross / (rvar * nvar + f(1e-8)), f(0), f(2)).astype(f)
    out = np.zeros(truth["N"], f)
    out[truth["used"]] = ncc
    return out


# ----------------------------------------------------------------------------------------------------------------------- the checker
def deviations(got, truth):
    """got: dict(noise, d_mask, weights, geo_sum, geo_count, g_depth, g_near, ncc, ncc_mask, ncc_sum, ncc_count, g_normal [3,HW], g_dist) with the
    UNSCALED gradients (of the two sums).  -> (worst, report, problems): worst = per quantity the largest deviation in the units of BOUND,
    report = counts (robust, fragile, flips by gate), problems = list of strings: what no bound forgives (a mask differing on a robust
    element, a gradient where there must be none, a count that the flips do not explain)."""
    t = truth
    a = lambda k: np.asarray(got[k], np.float64).reshape(-1)
    problems, worst, rep = [], {}, {}
    gm = np.asarray(got["d_mask"]).astype(bool).reshape(-1)
    vr, gr = t["value_robust"], t["grad_robust"]
    flips = gm != t["d_mask"]
    bad = np.nonzero(flips & vr)[0]
    if bad.size:
        problems.append(f"d_mask differs on {bad.size} robust pixels, first {bad[:6].tolist()} (closest gate {t['closest'][bad[:6]].tolist()})")
    rep["pixels"], rep["in_frustum"] = int(vr.size), t["in_frustum"]
    rep["fragile_pixels"] = int((~gr).sum())
    rep["flipped_pixels"] = {g: int((flips & (t["closest"] == g)).sum()) for g in GEO_VALUE_GATES if (flips & (t["closest"] == g)).any()}
    on = vr & t["d_mask"]
    with np.errstate(all="ignore"):
        worst["noise"] = float(np.abs(a("noise") - t["noise"])[vr & t["frustum"] & np.isfinite(t["noise"])].max(initial=0.0))
        worst["weight"] = float(np.abs(a("weights") - t["weights"])[vr].max(initial=0.0))
        gd, gn = a("g_depth"), a("g_near")
        if not np.isfinite(gd).all() or not np.isfinite(gn).all():
            problems.append("non-finite geometric gradient")
        off = vr & ~t["d_mask"]
        if np.abs(gd[off]).max(initial=0.0) != 0 or np.abs(a("weights")[off]).max(initial=0.0) != 0:
            problems.append("a pixel that is off beyond doubt has a weight or a gradient")
        sel = gr & t["d_mask"] & (t["scale_depth"] > 0)
        worst["g_geo"] = float((np.abs(gd - t["g_depth"])[sel] / t["scale_depth"][sel]).max(initial=0.0))
        nr = t["near_robust"]
        sel_n = nr & (t["scale_near"] > 0)
        worst["g_geo"] = max(worst["g_geo"], float((np.abs(gn - t["g_near"])[sel_n] / t["scale_near"][sel_n]).max(initial=0.0)))
        if np.abs(gn[nr & (t["scale_near"] == 0)]).max(initial=0.0) != 0:
            problems.append("g_near holds a contribution in a texel no valid pixel taps")
        l2 = lambda x, y: float(np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-300))
        keep_d = gr | ~(gm | t["d_mask"])
        worst["l2_depth"], worst["l2_near"] = l2(gd[keep_d], t["g_depth"][keep_d]), l2(gn[nr], t["g_near"][nr])
    want_count = t["geo_count"] + int((flips & gm).sum()) - int((flips & ~gm).sum())
    if int(got["geo_count"]) != want_count or int(gm.sum()) != want_count:
        problems.append(f"geo count {got['geo_count']} (mask {int(gm.sum())}) != truth {t['geo_count']} corrected for the flips: {want_count}")
    tw = np.where(vr, t["weights"] * np.nan_to_num(t["noise"]), a("weights") * np.nan_to_num(a("noise")))
    want_sum = float(tw[gm].sum())
    tol = max(want_count, 1) * (2 * BOUND["noise"] + 4 * EPS24)
    worst["geo_sum"] = abs(float(got["geo_sum"]) - want_sum) / tol                  # in units of its tolerance: must stay <= 1
    # ------------------------------------------------------------------------------------------------------------------------- samples
    idx, N = t["indices"], t["N"]
    used = idx >= 0
    pix = np.where(used, idx, 0)
    gncc, gmask = a("ncc")[:N], np.asarray(got["ncc_mask"]).astype(bool).reshape(-1)[:N]
    if np.abs(gncc[~used]).max(initial=0.0) != 0 or gmask[~used].any():
        problems.append("an unused slot (-1) has an ncc value or a mask")
    svr, sgr = t["s_value_robust"] & used, t["s_grad_robust"] & used
    cmp_v = used & t["defined"] & (t["s_margins"]["g2"] > BOUND["g2"]) & np.isfinite(t["unit"])
    with np.errstate(all="ignore"):
        worst["ncc"] = float((np.abs(gncc - t["ncc"])[cmp_v] / t["unit"][cmp_v]).max(initial=0.0))
    sflip = (gmask != t["ncc_mask"]) & used & t["defined"]
    bad = np.nonzero(sflip & svr)[0]
    if bad.size:
        problems.append(f"ncc_mask differs on {bad.size} robust samples, first slots {bad[:6].tolist()}")
    rep["samples"], rep["value_fragile_samples"], rep["grad_fragile_samples"] = int(used.sum()), int((used & ~t["s_value_robust"]).sum()), int((used & ~t["s_grad_robust"]).sum())
    rep["flipped_samples"] = int(sflip.sum())
    gN, gD = np.asarray(got["g_normal"], np.float64).reshape(3, -1), a("g_dist")
    if not np.isfinite(gN).all() or not np.isfinite(gD).all():
        problems.append("non-finite NCC gradient")
    g4, t4 = np.concatenate([gN[:, pix], gD[None, pix]], 0), np.concatenate([t["g_normal"][:, pix], t["g_dist"][None, pix]], 0)
    tw_s = t["weights"][pix]
    sends = t["ncc_mask"] & (t["ncc_raw"] > 0) & (t["ncc_raw"] < 2) & (tw_s > 0)
    live = sgr & sends
    with np.errstate(all="ignore"):
        dev = np.abs(g4 - t4).max(axis=0) / (t["unit"] * (np.abs(t4).max(axis=0) + t["grad_floor"]))
        worst["g_ncc"] = float(dev[live].max(initial=0.0))
        worst["l2_ncc"] = float(np.linalg.norm((g4 - t4)[:, live]) / (np.linalg.norm(t4[:, live]) + 1e-300))
    none = used & t["weight_robust"] & ((svr & ~t["ncc_mask"]) | (tw_s == 0))
    sampled = np.zeros(gD.size, bool); sampled[pix[used]] = True
    if np.abs(g4[:, none]).max(initial=0.0) != 0:
        problems.append("a sample whose mask is off beyond doubt, or whose weight is 0, sends a gradient")
    if np.abs(gN[:, ~sampled]).max(initial=0.0) != 0 or np.abs(gD[~sampled]).max(initial=0.0) != 0:
        problems.append("a pixel that was not sampled has an NCC gradient")
    undefined = used & ~t["defined"]
    want_c = t["ncc_count"] + int((sflip & gmask).sum()) - int((sflip & ~gmask).sum()) + int((gmask & undefined).sum())
    if int(got["ncc_count"]) != want_c or int(gmask.sum()) != want_c:
        problems.append(f"ncc count {got['ncc_count']} (mask {int(gmask.sum())}) != truth {t['ncc_count']} corrected for the flips: {want_c}")
    gw = a("weights")[pix]
    contrib = np.where(svr & t["weight_robust"], t["ncc"] * tw_s, gncc * gw)
    want_s = float(contrib[gmask & used].sum())
    with np.errstate(all="ignore"):
        tol_s = float((BOUND["ncc"] * np.where(np.isfinite(t["unit"]), t["unit"], 0.0) * tw_s + 2 * BOUND["weight"])[gmask & used].sum()) + 4 * EPS24 * max(want_c, 1)
    worst["ncc_sum"] = abs(float(got["ncc_sum"]) - want_s) / tol_s
    return worst, rep, problems


CHECKED = ("noise", "weight", "g_geo", "ncc", "g_ncc")


def check(got, truth, label=""):
    """deviations() held to BOUND: raises AssertionError naming the first miss.  -> (worst, report)"""
    worst, rep, problems = deviations(got, truth)
    assert not problems, f"{label}: " + "; ".join(problems)
    for k in CHECKED:
        assert worst[k] <= BOUND[k], f"{label}: {k} deviates by {worst[k]:.3e}, bound {BOUND[k]:.3e}"
    assert worst["geo_sum"] <= 1.0 and worst["ncc_sum"] <= 1.0, f"{label}: sums off by {worst['geo_sum']:.2f} / {worst['ncc_sum']:.2f} of their tolerance"
    return worst, rep


def unscale(grad, up, lam, count):
    """the unscaled gradient of the sum from the gradient of up * lam * mean (zero maps when the count is 0)"""
    return np.asarray(grad, np.float64) / (up * lam / max(float(count), 1.0))
