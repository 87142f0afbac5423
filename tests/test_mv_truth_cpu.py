"""tests/mv_truth.py (the float64 statement of the PGSR multi-view losses) held to the reference-run fixture and to the float32 C oracle (plain
and FMA builds, and a float32 evaluation of the patch sums in the kernel's order); its bounds measured again; its checker shown to accept every
correct float32 evaluation and to refuse planted errors; the cases held to their caps on fragile elements.  No GPU."""
import functools

import numpy as np
import pytest

import golden_ref
import mv_cases as MC
import mv_truth as MT
import sampler_truth as ST


@functools.lru_cache(maxsize=None)
def truth_of(name):
    return MT.evaluate(MC.make(name))


@functools.lru_cache(maxsize=None)
def candidate_of(name, fma):
    return MT.oracle_candidate(MC.make(name), truth_of(name)["indices"], fma)


def term_deviations(c, t):
    """the float32 oracle's u, v, q.z, warped taps and g2 against the truth's: the bounds of the gates"""
    with np.errstate(all="ignore"):
        live = np.isfinite(t["u"]) & np.isfinite(t["v"]) & (np.abs(t["u"]) < 4 * t["Wn"]) & (np.abs(t["v"]) < 4 * t["Hn"]) & (t["qz"] > 0.05)
        du = max(np.abs(c["u"] - t["u"])[live].max(initial=0.0), np.abs(c["v"] - t["v"])[live].max(initial=0.0))
        dq = np.abs(c["qz"] - t["qz"])[live].max(initial=0.0)
        dw = dg = 0.0
        if t["warp"] is not None:
            cw = c["warp"][t["used"]].astype(np.float64)
            near = (np.abs(t["warp"][..., 0]) < 2 * t["Wg"]) & (np.abs(t["warp"][..., 1]) < 2 * t["Hg"]) & (np.abs(t["g2"]) > 0.05) & np.isfinite(cw).all(axis=-1)
            dw = np.abs(cw[..., :2] - t["warp"])[near].max(initial=0.0)
            dg = np.abs(cw[..., 2] - t["g2"])[np.isfinite(cw[..., 2]) & np.isfinite(t["g2"])].max(initial=0.0)
    return dict(u=float(du), qz=float(dq), warp=float(dw), g2=float(dg))


@functools.lru_cache(maxsize=None)
def measure():
    """-> (worst over all cases {quantity: deviation}, per-case rows)"""
    worst, rows = dict.fromkeys(MT.MEASURED, 0.0), []
    for name in MC.NAMES:
        t = truth_of(name)
        for fma in (False, True):
            c = candidate_of(name, fma)
            w, rep, problems = MT.deviations(c, t)
            assert not problems, (name, fma, problems)
            w.update(term_deviations(c, t))
            rows.append((name, "fma" if fma else "plain", w, rep))
            for k in worst:
                if k in w:
                    worst[k] = max(worst[k], w[k])
        if t["ref_val"] is not None:
            d = np.abs(MT.device_order_ncc(t).astype(np.float64) - t["ncc"])
            ok = (t["indices"] >= 0) & t["defined"] & np.isfinite(t["unit"])
            worst["ncc_device_order"] = max(worst["ncc_device_order"], float((d[ok] / t["unit"][ok]).max(initial=0.0)))
    return worst, rows


def test_bounds_cover_the_oracle_deviation():
    """Every bound of mv_truth is at least 4 x the largest deviation of a float32 evaluation from the truth, and not idly wide: at most 4.8 x."""
    worst, rows = measure()
    for name, build, w, rep in rows:
        print(f"{name:22s} {build:5s} " + " ".join(f"{k}={w[k]:.2e}" for k in ("u", "noise", "weight", "g_geo", "warp", "ncc", "g_ncc", "l2_depth", "l2_near", "l2_ncc"))
              + f" | pixels fragile {rep['fragile_pixels']} flipped {rep['flipped_pixels']} samples {rep['samples']} vf {rep['value_fragile_samples']} "
              f"gf {rep['grad_fragile_samples']} flipped {rep['flipped_samples']}")
    for k, v in worst.items():
        print(f"quantity {k}: largest float32 deviation {v:.3e}, x4 = {4 * v:.3e}, bound {MT.BOUND.get('ncc' if k == 'ncc_device_order' else k):.3e}, recorded {MT.MEASURED[k]:.3e}")
    for k, v in worst.items():
        b = MT.BOUND["ncc" if k == "ncc_device_order" else k]
        assert 4 * v <= b, (k, v, b)
    for k, b in MT.BOUND.items():                # a round figure above 4 x the deviation measured NOW, never more than a fifth above it
        top = max(worst[k], worst["ncc_device_order"] if k == "ncc" else 0.0)
        assert b <= 1.2 * 4 * top, (k, b, top)
    for k, v in worst.items():                   # and the recorded figures are these measurements, to the digits kept
        assert abs(MT.MEASURED[k] - v) <= 0.03 * v, (k, MT.MEASURED[k], v)


@pytest.mark.parametrize("name", MC.NAMES)
def test_cases_stay_under_their_caps(name):
    """Conditions on the inputs, not tolerances: a case with too many elements near a decision checks too little."""
    t = truth_of(name)
    case = MC.make(name)
    tied = MC.tied_pixels(case)
    frag = ~t["grad_robust"] & ~tied & (t["frustum"] | ~t["value_robust"])
    used = (t["indices"] >= 0) & ~tied[np.where(t["indices"] >= 0, t["indices"], 0)]        # a sample on a tied pixel is exempt with it
    vf, gf = int((used & ~t["s_value_robust"]).sum()), int((used & ~t["s_grad_robust"]).sum())
    print(f"{name}: fragile pixels {int(frag.sum())} / {t['in_frustum']} in frustum ({int(tied.sum())} tied by construction), samples {int(used.sum())}: "
          f"value-fragile {vf}, gradient-fragile {gf}, kappa median {np.median(t['kappa'][used]) if used.any() else 0:.1f} max finite "
          f"{np.max(t['kappa'][used & np.isfinite(t['kappa'])], initial=0):.1f}")
    if name == "identical":          # every pixel has noise ~ 0 and projects onto a texel centre on purpose: the case has its own assertions
        assert (t["margins"]["noise0"][t["frustum"]] < 1e-4).all() and t["value_robust"].mean() > 0.9
        return
    assert frag.sum() <= max(MC.MAX_FRAGILE * t["in_frustum"], 2)
    n = max(int(used.sum()), 1)
    planted = 1 if name == "constant_patch" else 0
    assert vf - planted <= max(MC.MAX_VALUE_FRAGILE_SAMPLES * n, 1) and gf - planted <= max(MC.MAX_GRAD_FRAGILE_SAMPLES * n, 2)


def test_cases_reach_the_paths_they_are_named_for():
    t = truth_of("low_contrast")
    assert np.median(t["kappa"]) > 1000
    t = truth_of("constant_patch")
    assert np.isinf(t["kappa"][9]) or t["kappa"][9] > 1e9
    for name in ("patch2_n15", "n4097", "shifted_near"):
        t = truth_of(name)
        used = t["indices"] >= 0
        assert (t["indices"] < 0).any() and (used & (t["weights"][np.where(used, t["indices"], 0)] == 0)).any(), name
    t = truth_of("shifted_near")
    wx = t["warp"][..., 0]
    outside = (wx < -1) | (wx > t["Wg"])
    assert outside.all(axis=1).any() and (outside.any(axis=1) & ~outside.all(axis=1)).any()
    for name in ("border_u", "border_v"):
        t, case = truth_of(name), MC.make(name)
        line, tied = MC.border_line(case, np.arange(t["u"].size)), MC.tied_pixels(case)
        for col, gate in case["ties"].items():
            sel = (line == col) & tied
            assert (~t["grad_robust"][sel]).all() and (t["closest"][sel] == gate).all(), (name, col, gate, t["closest"][sel][:4])
        assert t["grad_robust"][~tied].mean() > 0.95
        clamped = line == 27                                       # Wn - 0.5: inside the frustum, coordinate clamped
        assert t["frustum"][clamped].all()
    base, planted, rows = MC.degenerate()
    clean = dict(planted, near_plane_depth=base["near_plane_depth"])            # the planted scene without its NaN texel
    tc, tp = MT.evaluate(clean), MT.evaluate(planted)
    feeders = rows["near_nan_feeders"]
    assert tc["d_mask"][feeders].any() and not tp["d_mask"][feeders].any()      # valid pixels tap the texel; the NaN switches them off
    geo_rows = [rows[k] for k in ("depth_zero", "depth_negative", "depth_nan", "depth_inf", "qz_zero", "qz_below")]
    assert not tp["d_mask"][geo_rows].any() and tp["value_robust"][geo_rows].all()           # off beyond doubt in the truth too
    assert tp["geo_count"] == MT.evaluate(base)["geo_count"]
    t = truth_of("patch0")
    assert (t["ncc"][t["indices"] >= 0] == 1).all() and not t["ncc_mask"].any() and not t["g_normal"].any()


def test_truth_matches_the_reference_run():
    z = golden_ref.load("ref_loss_plane_multiview")
    cam = lambda pre: {k: (z[f"{pre}_{k}"] if k in ("R", "T") else float(z[f"{pre}_{k}"])) for k in ("R", "T", "Fx", "Fy", "Cx", "Cy")}
    case = dict(W=int(z["W"]), H=int(z["H"]), view=cam("v"), near=cam("n"), patch=int(z["patch_size"]), noise_th=float(z["pixel_noise_threshold"]),
                **{k: z[k] for k in ("plane_depth", "near_plane_depth", "rendered_normal", "rendered_distance", "gray", "near_gray")})
    t = MT.evaluate(case, None)
    lg, ln = float(z["lambda_geo"]), float(z["lambda_ncc"])
    np.testing.assert_allclose(lg * t["geo_sum"] / t["geo_count"], float(z["geo_loss"]), rtol=2e-5)
    np.testing.assert_allclose(ln * t["ncc_sum"] / t["ncc_count"], float(z["ncc_loss"]), rtol=2e-4)
    # the reference ran in float32: its own gradients carry the direction noise of pixels with a tiny reprojection error (mv_truth's noise0 gate)
    keep_d, keep_n = t["grad_robust"] | ~t["d_mask"], t["near_robust"]
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel((lg / t["geo_count"] * t["g_depth"])[keep_d], z["d_plane_depth"].reshape(-1)[keep_d]) < 1e-4
    assert rel((lg / t["geo_count"] * t["g_near"])[keep_n], z["d_near_plane_depth"].reshape(-1)[keep_n]) < 1e-4
    assert rel(ln / t["ncc_count"] * t["g_normal"], z["d_rendered_normal"].reshape(3, -1)) < 2e-3
    assert rel(ln / t["ncc_count"] * t["g_dist"], z["d_rendered_distance"].reshape(-1)) < 2e-3


# ------------------------------------------------------------------------------------------------------------------- the checker itself
@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("name", MC.NAMES)
def test_checker_accepts_the_oracle(name, fma):
    t = truth_of(name)
    c = dict(candidate_of(name, fma))
    MT.check(c, t, name)
    if t["ref_val"] is not None:                 # the kernel's summation order: its own values, its own mask, count and sum, through the whole checker
        used = t["indices"] >= 0
        ncc = MT.device_order_ncc(t)
        w = c["weights"][np.where(used, t["indices"], 0)]
        # the truth's guarded taps are 0 where a coordinate is not finite; no case of NAMES has such a sample
        assert t["defined"][used].all()
        mask = used & (ncc < np.float32(0.9))
        flipped = mask != c["ncc_mask"]
        assert not (flipped & t["s_value_robust"]).any()
        c.update(ncc=ncc, ncc_mask=mask, ncc_count=int(mask.sum()), ncc_sum=float((ncc.astype(np.float64) * w)[mask].sum()))
        if flipped.any():                        # a sample whose mask the other order flips has the oracle's gradient for the other decision: take its pixel's out
            gN, gD = c["g_normal"].copy(), c["g_dist"].copy()
            px = t["indices"][flipped]
            gN[:, px], gD[px] = t["g_normal"][:, px] * (mask[flipped]), t["g_dist"][px] * (mask[flipped])
            c.update(g_normal=gN, g_dist=gD)
        MT.check(c, t, name + " device order")


def test_mv_expf_is_within_an_ulp_of_exp():
    """The exp that k_mv_geo and the oracle share (mv_expf, the same float32 sequence in both) against float64 exp: a dense grid over the
    arguments a weight can see, [0, 30], and over negative ones; the float32 overflow edge; the explicit branches (x >= 100, NaN, x < -110)."""
    import oracle_multiview as om
    f = np.float32
    x = np.concatenate([np.linspace(0, 30, 2000001), np.linspace(-87, 0, 500001), np.linspace(30, 88.7, 500001)]).astype(f)
    y = om.mv_expf(x).astype(np.float64)
    want = np.exp(x.astype(np.float64))
    ulp = np.abs(y - want) / np.spacing(want.astype(f)).astype(np.float64)
    worst = {k: float(ulp[m].max()) for k, m in (("[0,30]", (x >= 0) & (x <= 30)), ("[-87,0)", x < 0), ("(30,88.7]", x > 30))}
    print("mv_expf against float64 exp, ulps:", worst)
    assert worst["[0,30]"] <= 0.96 and max(worst.values()) <= 1.0
    assert om.mv_expf([0.0])[0] == 1.0 and om.mv_expf([np.log(2.0)])[0] == f(2.0)
    edge = om.mv_expf(np.array([88.72, 88.73, 89.0, 99.99, 100.0, 1e9, np.inf, -104.0, -111.0, -1e9, -np.inf], f))
    assert np.isfinite(edge[0]) and np.isinf(edge[1:7]).all() and (edge[1:7] > 0).all()          # FLT_MAX = exp(88.7228...)
    assert (edge[7:] >= 0).all() and (edge[8:] == 0).all() and edge[7] <= f(1e-44)
    assert np.isnan(om.mv_expf([np.nan])[0])
    assert (1.0 / om.mv_expf(np.array([1e9, 200.0], f)) == 0).all()                                # the weight of a huge reprojection error


def _planted(defect, c, t, case):
    """a copy of the candidate's arrays with one error"""
    c = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    Wn, Hn = t["Wn"], t["Hn"]
    on = t["d_mask"] & t["grad_robust"]
    near = np.asarray(case["near_plane_depth"], np.float64).reshape(-1)
    if defect == "tap_weight_swapped_on_clamped":           # k_mv_geo's first atomic with ax in place of wx0, seen only where u is clamped (ax == 0)
        p = np.nonzero(on & (t["u"] > Wn - 1))[0]
        wy0 = 1.0 - (np.clip(t["v"][p], 0, Hn - 1) - t["y0"][p])
        g = c["g_near"].astype(np.float64)
        np.add.at(g, t["y0"][p] * Wn + t["x0"][p], -t["dmz"][p] * wy0)
        c["g_near"] = g
    elif defect == "mu_dropped":                              # the coordinate gradient of a clamped coordinate kept: dmz * dmz_dv * dv/ddepth arrives
        p = np.nonzero(on & (t["v"] > Hn - 1))[0]
        ax = np.clip(t["u"][p], 0, Wn - 1) - t["x0"][p]
        k0 = t["y0"][p] * Wn + t["x0"][p]
        dmz_dv = -near[k0] * (1 - ax) - near[np.minimum(k0 + 1, Wn * Hn - 1)] * ax      # the bottom taps are out of range
        c["g_depth"] = c["g_depth"].astype(np.float64)
        c["g_depth"][p] += t["dmz"][p] * dmz_dv * t["dv_dd"][p]
    elif defect == "adjoint_row_1pc":                         # 1 % in one row of the 3x3 adjoint: the y component of every normal gradient
        c["g_normal"] = c["g_normal"].astype(np.float64); c["g_normal"][1] *= 1.01
    elif defect == "sample_index_shifted":                    # every NCC result one slot late
        c["ncc"] = np.roll(c["ncc"], 1); c["ncc_mask"] = np.roll(c["ncc_mask"], 1)
    elif defect == "ncc_3_bounds":
        i = int(np.nonzero((t["indices"] >= 0) & t["s_value_robust"] & np.isfinite(t["unit"]))[0][3])
        c["ncc"] = c["ncc"].astype(np.float64); c["ncc"][i] = t["ncc"][i] + 3 * MT.BOUND["ncc"] * t["unit"][i]
    elif defect == "count_off_by_one":
        c["geo_count"] += 1
    elif defect == "ncc_count_off_by_one":
        c["ncc_count"] -= 1
    return c


DEFECT_CASE = {"tap_weight_swapped_on_clamped": "border_u", "mu_dropped": "border_v", "adjoint_row_1pc": "default", "sample_index_shifted": "patch3_n16",
               "ncc_3_bounds": "scale1p5_near_50x38", "count_off_by_one": "near_50x38", "ncc_count_off_by_one": "n4097"}


@pytest.mark.parametrize("defect", list(DEFECT_CASE))
def test_a_planted_error_trips_the_checker(defect):
    name = DEFECT_CASE[defect]
    t, case = truth_of(name), MC.make(name)
    c = candidate_of(name, False)
    MT.check(dict(c), t, "clean")
    if defect in ("tap_weight_swapped_on_clamped", "mu_dropped"):
        assert (t["d_mask"] & t["grad_robust"] & (t["u" if name == "border_u" else "v"] > (t["Wn"] if name == "border_u" else t["Hn"]) - 1)).any()
    with pytest.raises(AssertionError):
        MT.check(_planted(defect, c, t, case), t, defect)


# ------------------------------------------------------------------------------------------------------------------------- the sampler
def test_the_tied_seeds_still_tie():
    m = ST.tie_mask()
    assert m.size == 20011 and m.size % 256 != 0
    for seed in ST.TIE_SEEDS:
        assert ST.fills_from_ties(m, ST.TIE_NUM, seed), seed
    assert ST.find_tied_seeds(2) == list(ST.TIE_SEEDS[:2]) and ST.TIE_SEEDS[2] >> 32 == 0xDEADBEEF
    assert not ST.fills_from_ties(m, ST.TIE_NUM, 5)


def test_sampler_restatement_is_the_num_smallest_keys():
    """select() against a plain sort of (key, index) pairs, and key24 against the hash written out with Python integers"""
    def key_py(p, seed):
        s0, s1, M = seed & 0xFFFFFFFF, seed >> 32, 0xFFFFFFFF
        x = (p * 0x9E3779B1 + s0) & M
        x ^= x >> 16; x = (x * 0x85EBCA6B) & M; x ^= x >> 13; x = (x + s1) & M; x = (x * 0xC2B2AE35) & M; x ^= x >> 16
        return x >> 8
    for seed in (0, 5, 0x9E3779B97F4A7C15, ST.TIE_SEEDS[2]):
        assert [key_py(p, seed) for p in (0, 1, 4095, 20010, 2 ** 31 - 1)] == ST.key24(np.array([0, 1, 4095, 20010, 2 ** 31 - 1]), seed).tolist()
    m = ST.tie_mask()
    for seed, num in ((5, 100), (ST.TIE_SEEDS[0], ST.TIE_NUM), (7, 1)):
        idx = np.nonzero(m)[0]
        pairs = sorted(zip(ST.key24(idx, seed).tolist(), idx.tolist()))[:num]
        T = pairs[-1][0] if len(pairs) == num else None
        got = ST.select(m, num, seed)
        assert sorted(got.tolist()) == sorted(p for _, p in pairs)
        k = ST.key24(got.astype(np.uint32), seed)
        below = k < sorted(ST.key24(idx, seed).tolist())[num]
        assert (np.diff(got[below]) > 0).all() and (np.diff(got[~below]) > 0).all() and below[:below.sum()].all()
    few = np.zeros(5003, bool); few[[7, 4100, 5002]] = True
    assert ST.select(few, 100, 3).tolist() == [7, 4100, 5002] + [-1] * 97
    assert ST.select(few[:50], 100, 3).tolist() == [7 if i == 7 else -1 for i in range(50)]
