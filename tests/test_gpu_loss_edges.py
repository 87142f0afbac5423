"""The fused image-space loss kernels (k_ssim_fwd, k_ssim_bwd, k_surfel_geo, k_plane_geo) at their edges, against the float64 truth of
tests/loss_truth.py element by element: every loss scalar, every gradient channel and every optional map within K[quantity] * 2^-24 * scale of
the truth, exact zeros exact, nothing non-finite; a fragile element on one side of its gate or the other.

Paths and where they are reached (cases of tests/loss_cases.py, test id in brackets):
  SSIM tiles of 30 / 30 / 1 rows and 32 / 32 / 1 columns: the SS_VROW clamp and the rows masked by ly0 + o < SS_TY      [*-1x61x65-*]
  exactly one tile; one more row and column; images smaller than the window; one row, one column          [*-3x30x32-*, *-1x31x33-*, *-2x5x11-*, *-1x11x4-*, *-1x1x70-*, *-1x70x1-*]
  E[x^2] - mu^2 cancelling against C2: smooth images with a small residual, constants, a bright near-converged pair, near-black     [smooth_*, affine, constant, bright, black]
  img == gt (the four terms of dS/dmu1 cancel; L1 sign 0), a bit-equal block, values clipped to 0 and 1, values up to 1.5     [identical, bit_equal, over_one]
  geo tiles of 4 / 4 / 1 rows and 64 / 64 / 1 columns, one tile, one more row and column, 3 x 3, four shapes without an interior pixel     [*-9x129-*, ...]
  rendered normal ~ depth normal: 1 - dot and dn - n (n . dn) cancel; in k_plane_geo sgn_ near 0, exactly 0, within a few ulps     [converged, conv_pert, conv_zero, conv_ulps]
  an empty rectangle over the seams: P = 0, len = 0, the 1e-12 clamp and the len > 1e-12 gate          [empty, depth0]
  nan0's inf branch (allmap0 != 0 at alpha 0; a quotient that overflows float32 only), median depth inf / -inf / nan, alpha 2^-126 and 2^-130     [specials]
  alpha = 0 blocks, weight None / random / with a zero region                                           [alpha0, *-None, *-zero_region]"""
import functools

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_truth as LT
from test_loss_truth_cpu import ALL, IDS, case_of, exempt, truth_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = 2.0                 # the upstream factor of every backward here: a power of two, so dividing it out again is exact


def _t(a, grad=False):
    t = torch.tensor(np.ascontiguousarray(a), device=DEV)
    return t.requires_grad_(True) if grad else t


def _n(t):
    return t.detach().cpu().numpy()


def run_device(kind, c, up=UP, unit=False, maps=True):
    """-> the candidate in the layout of loss_truth.check (gradients with the upstream factor divided out), plus 'raw': the gradient tensors as
    autograd returned them"""
    from gsrast.losses import l1_ssim, plane_geo_loss, surfel_geo_loss
    if kind == "ssim":
        x = _t(c["img"], True)
        loss, parts = l1_ssim(x, _t(c["gt"]), c["lam"], return_parts=True, unit_upstream=unit)
        (loss * up).backward()
        p = _n(parts)
        return dict(l1=p[0], ssim=p[1], loss=loss.item(), dL_dimg=_n(x.grad).astype(np.float64) / up, raw=(x.grad,))
    if kind == "surfel":
        x = _t(c["allmap"], True)
        out = surfel_geo_loss(x, _t(c["ray_mat"]), _t(c["normal_rot"]), c["depth_ratio"], c["lambda_normal"], c["lambda_dist"], return_maps=maps, unit_upstream=unit)
        (out[0] * up).backward()
        p = _n(out[1])
        cand = dict(err=p[0], dist=p[1], loss=out[0].item(), raw=(x.grad,), **LT.split_allmap_grad(_n(x.grad).astype(np.float64) / up))
        if maps:
            cand.update(surf_depth=_n(out[2])[0], normal_world=_n(out[3]), surf_normal=_n(out[4]))
        return cand
    d, a = _t(c["depth"][None], True), _t(c["all_map"], True)
    w = None if c["weight"] is None else _t(c["weight"])
    out = plane_geo_loss(d, a, _t(c["ray_mat"]), w, c["lam"], return_map=maps, unit_upstream=unit)
    (out[0] * up).backward()
    ga = _n(a.grad).astype(np.float64) / up
    cand = dict(l1=_n(out[1])[0], loss=out[0].item(), dL_ddepth=_n(d.grad)[0].astype(np.float64) / up, dL_dnormal=ga[0:3], dA_rest=ga[3:], raw=(d.grad, a.grad))
    if maps:
        cand["depth_normal"] = _n(out[2])
    return cand


@functools.lru_cache(maxsize=None)
def device_of(kind, name):
    return run_device(kind, case_of(kind, name))


def _report(tag, rep):
    print(f"HIP {tag} " + " ".join(f"{k}={v['worst']:.4g}" for k, v in rep.items() if k != "fragile_share")
          + f" | fragile share {rep['fragile_share']:.4f} took the other side " + str({k: v["took_other_side"] for k, v in rep.items() if k != "fragile_share" and v["took_other_side"]}))


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_case_matches_the_float64_truth(kind, name):
    """Values, parts, maps and gradients (backward with an upstream factor of 2) through loss_truth.check: no problem, and the fragile cap."""
    t = truth_of(kind, name)
    cand = device_of(kind, name)
    rep, problems = LT.check(cand, t, name)
    _report(f"{kind}:{name}", rep)
    assert not problems, problems
    if not exempt(kind, name):
        assert rep["fragile_share"] <= LC.MAX_FRAGILE
    if kind == "plane":
        assert not cand["dA_rest"].any()                       # alpha and distance get no gradient here
    if kind != "ssim":                                         # without the optional maps: the same loss and the same gradients, bit for bit
        bare = run_device(kind, case_of(kind, name), maps=False)
        assert bare["loss"] == cand["loss"] and all(torch.equal(a, b) for a, b in zip(bare["raw"], cand["raw"]))


def _first_of_each_regime():
    seen, out = set(), []
    for k, n in ALL:
        if (k, n.split("-")[0]) not in seen:
            seen.add((k, n.split("-")[0]))
            out.append((k, n))
    return out


FIRST = _first_of_each_regime()


@pytest.mark.parametrize("kind,name", FIRST, ids=[f"{k}:{n}" for k, n in FIRST])
def test_unit_upstream_is_bit_equal_to_an_upstream_of_one(kind, name):
    c = case_of(kind, name)
    a, b = run_device(kind, c, up=1.0, unit=False), run_device(kind, c, up=1.0, unit=True)
    assert a["loss"] == b["loss"]
    for x, y in zip(a["raw"], b["raw"]):
        assert torch.equal(x, y)
    assert any(x.abs().max() > 0 for x in a["raw"]) or c["regime"] == "identical"


@pytest.mark.parametrize("kind,name", [(k, n) for k, n in ALL if k != "ssim"], ids=[i for i, (k, _) in zip(IDS, ALL) if k != "ssim"])
def test_exact_zeros(kind, name):
    """What is 0 in every arithmetic is 0 on the device: allmap channels 7-10, dA[3:], the border of the normal maps, and on an image without
    interior pixels every gradient but the ones the truth names (channel 6; dL_dnormal = -w sign(0 - normal))."""
    c, t, cand = case_of(kind, name), truth_of(kind, name), device_of(kind, name)
    H, W = c["shape"]
    border = np.ones((H, W), bool); border[1:-1, 1:-1] = False
    if kind == "surfel":
        assert not cand["g_zero"].any() and not cand["surf_normal"][:, border].any()
        if c["shape"] in LC.NO_INTERIOR:
            assert not cand["g_depth"].any() and not cand["g_normal"].any() and not cand["surf_normal"].any()
            assert (cand["g_dist"] != 0).all() == (c["lambda_dist"] != 0)
    else:
        assert not cand["dA_rest"].any() and not cand["depth_normal"][:, border].any()
        if c["shape"] in LC.NO_INTERIOR:
            assert not cand["dL_ddepth"].any() and not cand["depth_normal"].any()
            assert np.array_equal(cand["dL_dnormal"] != 0, t["out"]["dL_dnormal"] != 0)


OLD_SURFEL = [(23, 31, 0.0, 0), (17, 40, 1.0, 1), (30, 22, 0.3, 2), (3, 3, 0.0, 3), (2, 5, 0.0, 4), (16, 16, 0.0, 5), (33, 49, 0.0, 6), (200, 333, 0.0, 7), (32772, 3, 0.0, 8)]
OLD_PLANE = [(23, 31, 0, True), (17, 40, 1, False), (3, 3, 2, True), (2, 6, 3, True), (100, 161, 4, True), (32772, 3, 5, True)]


@pytest.mark.parametrize("H,W,ratio,seed", OLD_SURFEL)
def test_old_surfel_inputs_under_the_per_channel_bound(H, W, ratio, seed):
    """The inputs of test_gpu_loss.py::test_surfel_geo_matches_oracle (lambda_dist = 100), every channel group held to its own bound."""
    import test_gpu_loss
    from gsrast.losses import camera_ray_matrices
    am, wvt, fpt = test_gpu_loss._geo_inputs(H, W, seed)
    rm, nr = camera_ray_matrices(wvt.to(DEV), fpt.to(DEV), W, H)
    c = dict(allmap=am, ray_mat=_n(rm), normal_rot=_n(nr), depth_ratio=ratio, lambda_normal=0.05, lambda_dist=100.0)
    t = LT.surfel_truth(c["allmap"], c["ray_mat"], c["normal_rot"], ratio, 0.05, 100.0)
    rep, problems = LT.check(run_device("surfel", c), t, f"old surfel {H}x{W}")
    _report(f"old-surfel:{H}x{W}", rep)
    assert not problems, problems


@pytest.mark.parametrize("H,W,seed,use_w", OLD_PLANE)
def test_old_plane_inputs_under_the_per_channel_bound(H, W, seed, use_w):
    """The inputs of test_gpu_loss.py::test_plane_geo_matches_oracle; a sign within its bound of 0 may fall on either side, nothing else may."""
    import test_loss_cpu
    depth, am, Kc, weight = test_loss_cpu._plane_case(H, W, seed)
    rm = torch.inverse(torch.tensor(Kc, dtype=torch.float64).t()).float().numpy()
    c = dict(depth=depth, all_map=am, weight=weight if use_w else None, ray_mat=rm, lam=0.015)
    t = LT.plane_truth(depth, am[3], am[0:3], c["weight"], rm, 0.015)
    rep, problems = LT.check(run_device("plane", c), t, f"old plane {H}x{W}")
    _report(f"old-plane:{H}x{W}", rep)
    assert not problems, problems
