"""The multi-view loss kernels (k_mv_geo, k_mv_ncc<CACHE>, k_mv_values, k_mv_scale) and the pixel sampler (gsr_sample_mask) at their edges,
against the float64 truth of tests/mv_truth.py element by element, and against the host restatement of the sampler slot for slot.

Paths and where they are reached (test id in brackets):
  near size and intrinsics of their own, y0 * Wn addressing with Wn != W          [near_50x38, near_64x48_of_33x17, scale1p5_near_50x38, border_*]
  ncc_scale 2.0 / 1.5: px = x / s, K_near(s), Kinv_view(s), gray smaller than the render      [scale2_patch2, scale1p5_near_50x38]
  patch 0 (one tap), 1, 2 (25 taps: lanes 9-15 one tap, 0-8 two), 3, 4 and 8 (re-gathering variant, 289 taps), 9 refused
                                                                                   [patch0 .. patch8_n17, test_patch_9_is_refused]
  sample lists of 1, 15, 16, 17, 4097 slots (N % 16 != 0), idx == -1 slots, sampled pixels with weight 0, image corners and edges (reference
  taps in the zero padding)                                                        [patch1_n1 .. patch8_n17, n4097]
  warped patches partly and wholly outside the gray image (mv_bilerp0's fu == -1 and fu == W-1 strips)     [shifted_near]
  a constant reference patch (rvar == 0), kappa in the thousands                   [constant_patch, low_contrast]
  u in (Wn-1, Wn): mask true, coordinate clamped, mu = 0, xr false; u at Wn-1, on a cell edge (ax == 0), at 0, at Wn, just outside; the same in v
                                                                                   [border_u, border_v]
  noise == 0 (the noise > 0 branch)                                               [identical]
  the isfinite guard, q.z <= 0.1, NaN / 0 inputs                                  [test_degenerate_inputs_switch_off_only_themselves]
  the `clamped` branch of k_mv_ncc (reachable through rounding only)             [identical]
  k_mv_scale with device upstream scalars, out_all_map                            [test_plane_losses_scales_by_float64_factors]
  the sampler's tie-fill branch, the `all` path, valid counts around num, block edges     [test_sampler_*]"""
import numpy as np
import pytest
import torch

import mv_cases as MC
import mv_truth as MT
import oracle_multiview as om
import sampler_truth as ST

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LG, LN = 0.03, 0.15
LEAVES = ("plane_depth", "near_plane_depth", "rendered_normal", "rendered_distance")


def _cfg(case):
    from gsrast.losses import multiview_cfg
    s = float(case.get("ncc_scale", 1.0))
    Hn, Wn = case["near_plane_depth"].shape[-2:]
    Hg, Wg = case["gray"].shape[-2:]
    return multiview_cfg(MC.cam_ns(case["view"], s), MC.cam_ns(case["near"], s), case["W"], case["H"], near_size=(Wn, Hn), gray_size=(Wg, Hg),
                         patch_size=int(case.get("patch", 3)), pixel_noise_threshold=float(case.get("noise_th", 1.0)))


def run_device(case, indices, up=(2.0, 3.0)):
    """-> `got` in the layout of mv_truth.deviations: the gradients divided by the float64 factor up * lambda / max(count, 1) they must carry"""
    from gsrast.losses import plane_multiview_loss
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    lv = {k: t(case[k]).requires_grad_(True) for k in LEAVES}
    geo, ncc, aux = plane_multiview_loss(*[lv[k] for k in LEAVES], t(case["gray"]), t(case["near_gray"]), _cfg(case), LG, LN,
                                         indices=t(np.asarray(indices, np.int32)), return_aux=True)
    (up[0] * geo + up[1] * ncc).backward()
    return _got(aux, {k: v.grad for k, v in lv.items()}, geo, ncc, up)


def _got(aux, grads, geo, ncc, up):
    a = {k: v.detach().cpu().numpy() for k, v in aux.items()}
    st = a["stats"].astype(np.float64)
    g = {k: (np.zeros(1) if v is None else v.cpu().numpy()) for k, v in grads.items()}
    return dict(noise=a["pixel_noise"].reshape(-1), d_mask=a["d_mask"].reshape(-1), weights=a["weights"].reshape(-1), geo_sum=st[0], geo_count=int(st[1]),
                g_depth=MT.unscale(g["plane_depth"], up[0], LG, st[1]).reshape(-1), g_near=MT.unscale(g["near_plane_depth"], up[0], LG, st[1]).reshape(-1),
                ncc=a["ncc"], ncc_mask=a["ncc_mask"], ncc_sum=st[3], ncc_count=int(st[4]),
                g_normal=MT.unscale(g["rendered_normal"], up[1], LN, st[4]).reshape(3, -1), g_dist=MT.unscale(g["rendered_distance"], up[1], LN, st[4]).reshape(-1),
                stats=st, geo=float(geo), ncc_loss=float(ncc))


def _hold(name, got, truth, case):
    worst, rep = MT.check(got, truth, name)
    # second line of defence: whole-tensor relative L2 over the robust elements, at most 4 x what the float32 oracle shows on the same case
    orc = [MT.deviations(MT.oracle_candidate(case, truth["indices"], fma), truth)[0] for fma in (False, True)]
    for k in ("l2_depth", "l2_near", "l2_ncc"):
        bar = 4 * max(o[k] for o in orc)
        print(f"{name}: {k} device {worst[k]:.3e} oracle {max(o[k] for o in orc):.3e}")
        assert worst[k] <= bar, (name, k, worst[k], bar)
    print(f"{name}: " + " ".join(f"{k}={worst[k]:.2e}" for k in MT.CHECKED) + f" | oracle " + " ".join(f"{k}={max(o[k] for o in orc):.2e}" for k in MT.CHECKED)
          + f" | pixels {rep['pixels']} fragile {rep['fragile_pixels']} flipped {rep['flipped_pixels']} samples {rep['samples']} value-fragile "
          f"{rep['value_fragile_samples']} gradient-fragile {rep['grad_fragile_samples']} flipped {rep['flipped_samples']}")
    on = got["d_mask"]                             # the weight is 1 / mv_expf(noise) of the device's own noise, the bits of the sequence that
    assert np.array_equal(got["weights"][on], np.float32(1) / om.mv_expf(got["noise"][on])) and not got["weights"][~on].any()      # test_mv_truth_cpu holds to exp
    st = got["stats"]
    assert st[2] == (np.float32(st[0]) / np.float32(st[1]) if st[1] > 0 else 0.0) and st[5] == (np.float32(st[3]) / np.float32(st[4]) if st[4] > 0 else 0.0)
    assert np.float32(got["geo"]) == np.float32(LG) * np.float32(st[2]) and np.float32(got["ncc_loss"]) == np.float32(LN) * np.float32(st[5])
    return worst, rep


@pytest.mark.parametrize("name", MC.NAMES)
def test_case_matches_the_float64_truth(name):
    """Robust pixels and samples: masks equal to the truth, every value and every gradient element within its measured bound (mv_truth.BOUND);
    fragile ones may differ only in what their gate feeds, and are counted in the output."""
    case = MC.make(name)
    truth = MT.evaluate(case)
    got = run_device(case, truth["indices"])
    _hold(name, got, truth, case)
    if name.startswith("border"):
        clamped = (MC.border_line(case, np.arange(truth["u"].size)) == 27) & truth["grad_robust"]
        assert clamped.any() and got["d_mask"][clamped].all()                  # Wn - 0.5: inside the frustum with a clamped coordinate
    if name == "identical":
        fr = truth["frustum"] & truth["value_robust"]
        assert got["d_mask"][fr].all() and got["geo_count"] >= fr.sum()
        assert np.isfinite(got["g_depth"]).all() and np.isfinite(got["g_near"]).all()
        zero = got["noise"] == 0
        print(f"identical: {int(zero.sum())} of {zero.size} pixels have noise == 0 exactly, the largest is {got['noise'][truth['frustum']].max():.2e}")
        assert zero.any() and not got["g_depth"][zero].any()
        # the `clamped` branch of k_mv_ncc (1 - cc outside [0, 2]: no gradient) can only be reached through rounding (cc <= 1 by Cauchy-Schwarz):
        # here, where both patches are the same image, samples round below 0 (on one MI355X all 13 read ncc == 0, 12 send nothing).  Which ones do
        # is not pinned: the truth's gradient vanishes there and every such sample is gradient-fragile.  Reported, and held to be finite
        used = truth["indices"] >= 0
        at0 = used & (got["ncc"] == 0)
        pix = truth["indices"][at0]
        silent = int((~got["g_normal"][:, pix].any(axis=0) & (got["g_dist"][pix] == 0)).sum())
        print(f"identical: {int(at0.sum())} of {int(used.sum())} samples have ncc == 0 on the device, {silent} of them send no gradient at all (clamped, or weight 0)")
        assert np.isfinite(got["g_normal"]).all() and np.isfinite(got["g_dist"]).all()
    if name == "patch0":
        used = truth["indices"] >= 0
        assert (got["ncc"][used] == 1).all() and not got["ncc_mask"].any() and got["ncc_loss"] == 0 and not got["g_normal"].any() and not got["g_dist"].any()
    if name == "constant_patch":
        p = int(truth["indices"][9])
        assert not got["ncc_mask"][9] and not got["g_normal"][:, p].any() and got["g_dist"][p] == 0


@pytest.mark.parametrize("name", ["border_u", "border_v"])
def test_tied_border_pixels_equal_the_float32_oracle_bit_for_bit(name):
    """The pixels placed on a decision (u or v at 0, Wn - 1, Wn, on a cell edge, a few ulps outside) are fragile by construction: no truth can
    say which way they fall.  There the device is held to the float32 oracle, which follows the kernel's operation order in a build without
    contraction: noise, d_mask and the weight bit for bit.

    The weight is 1 / exp(noise).  With the library expf the device and the host agreed to an ulp, not to the bit (one weight of the 56 tied pixels
    of border_v was an ulp off): a library function is outside the argument from the operation order.  The kernel and the oracle now both state
    exp as the same fixed sequence of float32 operations (mv_expf), and the weight is bit-equal like the rest."""
    case = MC.make(name)
    truth = MT.evaluate(case)
    got = run_device(case, truth["indices"])
    tied = MC.tied_pixels(case)
    orc = MT.oracle_candidate(case, truth["indices"])
    assert (~truth["grad_robust"][tied]).all()
    assert np.array_equal(got["d_mask"][tied], orc["d_mask"][tied])
    assert np.array_equal(got["noise"][tied], orc["noise"][tied])
    assert np.array_equal(got["weights"][tied] == 0, orc["weights"][tied] == 0)
    ulps = np.abs(got["weights"][tied].astype(np.float64) - orc["weights"][tied]) / np.spacing(np.maximum(orc["weights"][tied], np.float32(1e-30)))
    print(f"{name}: weights of the {int(tied.sum())} tied pixels differ from the oracle by at most {ulps.max():.0f} ulps, bit-equal on {int((ulps == 0).sum())}")
    assert np.array_equal(got["weights"][tied], orc["weights"][tied])


def test_patch_9_is_refused():
    case = dict(MC.make("patch1_n1")); case["patch"] = 9
    with pytest.raises(RuntimeError, match="loss_plane_mv_geo: bad configuration"):
        run_device(case, np.array([5], np.int32))


def test_degenerate_inputs_switch_off_only_themselves():
    """plane_depth 0 / negative / NaN / +inf, a depth that puts q.z at 0 and at 0.05, a NaN texel of the neighbour's depth map under valid pixels;
    rendered_distance 0 and a NaN normal at sampled pixels.  The same scene with those pixels switched off by ordinary means (depth -1, the
    sample slot unused) must give the same sums, counts and gradients, bit for bit outside the planted pixels.

    For the geometric rows the reference's behaviour is defined (a comparison with NaN is false).  For the two NCC rows it is not (grid_sample
    on NaN coordinates): asserted is only what the kernel documents -- the sample's mask is off, it sends no gradient, it is not counted.

    Why every row addresses in range (csrc/gsr_mvloss.hip): k_mv_geo clamps u, v with fminf(fmaxf(., 0), Wn - 1): fmaxf returns the other operand
    for a NaN, so uc, vc lie in [0, Wn-1] x [0, Hn-1] for NaN and for both infinities, before floorf and the int conversion; the right / bottom tap
    is read only if x0 + 1 < Wn / y0 + 1 < Hn; the four loads are further under isfinite(u) && isfinite(v).  The atomics run under `dm`, which needs
    mask (false for NaN u, v, q.z) and noise < th (false for a NaN noise, which a NaN texel or mz gives), and use the same x0, y0.  depth 0 gives
    q = b, finite.  k_mv_ncc reads normal / dist at the sampled pixel p itself (0 <= p < W H by the list); a zero distance or NaN normal makes Hk
    and every warped coordinate NaN or infinite, and mv_bilerp0 tests floorf(u) in [-1, W) and floorf(v) in [-1, H) BEFORE any int conversion:
    the test is false for NaN and +-inf, the tap is 0 and no address is formed.  The reference taps do not depend on normal / dist."""
    base, planted, rows = MC.degenerate()
    gb, gp = run_device(base, base["indices"]), run_device(planted, planted["indices"])
    geo_rows = np.array([rows[k] for k in ("depth_zero", "depth_negative", "depth_nan", "depth_inf", "qz_zero", "qz_below")] + rows["near_nan_feeders"].tolist())
    assert not gp["d_mask"][geo_rows].any() and not gp["weights"][geo_rows].any() and not gp["g_depth"][geo_rows].any()
    assert gp["geo_count"] == gb["geo_count"] and gp["geo_sum"] == gb["geo_sum"] and gp["geo"] == gb["geo"]
    other = np.ones(gp["noise"].size, bool); other[geo_rows] = False
    for k in ("noise", "d_mask", "weights", "g_depth"):
        assert np.array_equal(gp[k][other], gb[k][other]), k
    # no contribution reaches g_near: the texel under the NaN included.  Its float atomics arrive in a different order from run to run
    assert np.isfinite(gp["g_near"]).all()
    assert np.abs(gp["g_near"] - gb["g_near"]).max() <= 1e-5 * np.abs(gb["g_near"]).max()
    truth = MT.evaluate(base)                     # and the base run itself is right
    MT.check(gb, truth, "degenerate base")
    for slot in (rows["dist_zero_slot"], rows["normal_nan_slot"]):
        p = int(planted["indices"][slot])
        assert not gp["ncc_mask"][slot] and np.isfinite(gp["ncc"][slot]) and not gp["g_normal"][:, p].any() and gp["g_dist"][p] == 0
    assert gp["ncc_count"] == gb["ncc_count"] and gp["ncc_sum"] == gb["ncc_sum"] and gp["ncc_loss"] == gb["ncc_loss"]
    keep = np.ones(gp["ncc"].size, bool); keep[[rows["dist_zero_slot"], rows["normal_nan_slot"]]] = False
    assert np.array_equal(gp["ncc"][keep], gb["ncc"][keep]) and np.array_equal(gp["ncc_mask"][keep], gb["ncc_mask"][keep])
    assert np.array_equal(gp["g_normal"], gb["g_normal"]) and np.array_equal(gp["g_dist"], gb["g_dist"])


def test_plane_losses_scales_by_float64_factors():
    """plane_losses with out_all_map, explicit indices and upstream scalars 2.5 / 0.7 (the normal loss unused): the gradients that leave
    k_mv_scale, divided by the float64 factor up * lambda / max(count, 1), meet the truth's unscaled gradients within the per-element bounds;
    the alpha channel of the out_all_map gradient is zero."""
    from gsrast.losses import plane_losses
    case = MC.make("scale1p5_near_50x38")
    truth = MT.evaluate(case)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    H, W = case["H"], case["W"]
    pd, nd = t(case["plane_depth"]).requires_grad_(True), t(case["near_plane_depth"]).requires_grad_(True)
    oam = torch.cat([t(case["rendered_normal"]), torch.full((1, H, W), 0.9, device=DEV), t(case["rendered_distance"])], 0).requires_grad_(True)
    K = torch.tensor([[80.0, 0, W / 2], [0, 80.0, H / 2], [0, 0, 1]], device=DEV)
    rm = torch.inverse(K.double().t()).float()
    up = (2.5, 0.7)
    from gsrast.losses import plane_multiview_loss
    gray, ngray, idx = t(case["gray"]), t(case["near_gray"]), t(truth["indices"])
    # the per-pixel and per-sample outputs come from the public two-loss call on the same inputs (they do not depend on which entry point ran: no
    # atomics feed them); values and gradients from plane_losses
    with torch.no_grad():
        g0, n0, aux = plane_multiview_loss(pd, nd, None, None, gray, ngray, _cfg(case), LG, LN, indices=idx, return_aux=True, out_all_map=oam)
    nrm, geo, ncc = plane_losses(pd, nd, oam, gray, ngray, _cfg(case), rm, None, 0.015, LG, LN, indices=idx)
    assert float(g0) == float(geo) and float(n0) == float(ncc) and float(nrm) > 0
    (up[0] * geo + up[1] * ncc).backward()
    ga = oam.grad
    assert ga.shape == (5, H, W) and ga[3].abs().max() == 0
    got = _got(aux, {"plane_depth": pd.grad, "near_plane_depth": nd.grad, "rendered_normal": ga[0:3], "rendered_distance": ga[4]}, geo, ncc, up)
    _hold("plane_losses", got, truth, case)


# ---------------------------------------------------------------------------------------------------------------------------- the sampler
def _sample(mask, num, seed):
    from gsrast.losses import sample_valid_pixels
    return sample_valid_pixels(torch.tensor(mask, device=DEV), num, seed=seed).cpu().numpy()


def _mask_with(n, count, seed):
    m = np.zeros(n, bool)
    m[np.random.default_rng(seed).permutation(n)[:count]] = True
    return m


@pytest.mark.parametrize("valid", ["num-1", "num", "num+1", "1", "0"])
@pytest.mark.parametrize("num", [1, 100, 3000])
def test_sampler_valid_counts_around_num(num, valid):
    """the exact output array at valid counts of num - 1, num (the `all` path of k_sm_pick: no bin's prefix exceeds num) and num + 1, 1 and 0"""
    count = {"num-1": num - 1, "num": num, "num+1": num + 1, "1": 1, "0": 0}[valid]
    m = _mask_with(5003, count, 3 * num + count)
    got = _sample(m, num, 11)
    assert np.array_equal(got, ST.select(m, num, 11)), (got[:8], ST.select(m, num, 11)[:8])


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8191, 8193, 20011])
@pytest.mark.parametrize("num", [1, 100, 3000])
def test_sampler_equals_the_host_restatement(n, num):
    """slot for slot, at the block edges of SM_BLOCK = 4096 and at an n that is no multiple of 256; seeds with and without high bits"""
    m = np.random.default_rng(n + num).random(n) < 0.7
    for seed in (5, 0x9E3779B97F4A7C15):
        want = ST.select(m, num, seed)
        got = _sample(m, num, seed)
        assert np.array_equal(got, want), (n, num, seed, np.nonzero(got != want)[0][:8])
        taken = want[want >= 0]
        assert taken.size == min(num, int(m.sum())) and np.unique(taken).size == taken.size and m[taken].all()


@pytest.mark.parametrize("seed", ST.TIE_SEEDS)
def test_sampler_fills_from_the_threshold_ties(seed):
    """seeds whose threshold key is shared by several entries, found by a host search (sampler_truth.find_tied_seeds): the last slots are filled
    from the ties in ascending index, k_sm_write's second branch"""
    m = ST.tie_mask()
    T, c_lt, c_eq = ST.threshold(m, ST.TIE_NUM, seed)
    assert c_eq >= 2 and c_lt < ST.TIE_NUM
    got = _sample(m, ST.TIE_NUM, seed)
    assert np.array_equal(got, ST.select(m, ST.TIE_NUM, seed))
    k = ST.key24(got.astype(np.uint32), seed)
    assert (k[:c_lt] < T).all() and (k[c_lt:] == T).all() and (np.diff(got[:c_lt]) > 0).all() and (np.diff(got[c_lt:]) > 0).all()


@pytest.mark.parametrize("where", ["one_block", "last_partial_block"])
def test_sampler_with_all_set_entries_in_one_block(where):
    n = 20011
    lo, hi = (2 * 4096, 3 * 4096) if where == "one_block" else (4 * 4096, n)
    m = np.zeros(n, bool)
    m[lo:hi] = np.random.default_rng(9).random(hi - lo) < 0.8
    for num in (100, 3000):
        got = _sample(m, num, 21)
        assert np.array_equal(got, ST.select(m, num, 21)), (where, num)
