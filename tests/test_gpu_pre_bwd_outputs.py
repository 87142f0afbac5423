"""GPU: what the preprocess backward writes, and from where.

k_preprocess_bwd_surfel takes Tw.z (transMat[8]) of the forward from a packed [P] array of the geometry arena instead of gathering it out of the
80-byte blend records, and both preprocess backward kernels skip the dL_dcov3D (surfel: dL_dtransMat) store when the caller passes a null pointer,
which the autograd bridge does exactly when no cov3D_precomp / transMat_precomp was supplied.  Every check runs on a 64x48 image at the sizes around
the kernels' 64-lane waves and 256-thread workgroups, two seeds, a quarter of the Gaussians behind the camera (radii == 0 rows).  Gradient bounds are
those of the small cases of tests/test_gpu_parity.py against tests/oracle.py (_grad_close, imported)."""
import functools

import numpy as np
import pytest
import torch

import oracle
import scenes
from test_gpu_parity import _grad_close, _hiprun

pytestmark = pytest.mark.gpu

W, H = 64, 48
SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
SEEDS = [0, 1]
VARIANTS = ["ewa", "surfel", "plane"]
CASES = [(v, P, s) for v in VARIANTS for P in SIZES for s in SEEDS]


@functools.lru_cache(maxsize=None)
def _case(variant, P, seed):
    """-> (scene, upstream gradients, the oracle's gradients, the oracle's radii); computed once per case and left unchanged."""
    sc = scenes.make_scene(variant, P, W, H, seed=seed, bg=(0.2, 0.4, 0.6))
    behind = (np.arange(P) + seed) % 4 == 1          # pose 0: world space is camera space, z > 0 in front
    sc["means3D"][behind, 2] *= -1.0
    if variant == "plane":
        sc["all_map"] = scenes.plane_all_map(sc)
    og = scenes.random_out_grads(variant, W, H, seed=seed, scale=1.0)
    with oracle.Forward(sc, variant) as f:
        g = f.backward(**og)
        radii = f.radii.copy()
    assert (radii[behind] == 0).all() and (P == 1 or (radii == 0).any())
    return sc, og, g, radii


def _pairs(variant):
    pairs = [("dL_dmeans3D", "dL_dmeans3D"), ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations"), ("dL_dopacities", "dL_dopacity"),
             ("dL_dmeans2D", "dL_dmeans2D"), ("dL_dcolors_precomp", "dL_dcolors")]
    if variant == "plane":
        pairs += [("dL_dall_map", "dL_dall_map"), ("dL_dmeans2D_abs", "dL_dmeans2D_abs")]
    return pairs


def _spy_backward(monkeypatch):
    """Records what gsrast.rasterize.backward was asked for and what it returned."""
    from gsrast import rasterize as rz
    seen = []
    real = rz.backward

    def spy(*a, **kw):
        g = real(*a, **kw)
        seen.append((kw.get("want_dcov3D"), g["dL_dcov3D"]))
        return g
    monkeypatch.setattr(rz, "backward", spy)
    return seen


@pytest.mark.parametrize("variant,P,seed", CASES)
def test_bridge_without_precomp_returns_none_for_the_slot_and_every_other_gradient(variant, P, seed, monkeypatch):
    """Through gsrast.runner.run = the autograd bridge, no cov3D_precomp: the library is handed a null dL_dcov3D, the slot comes back None, and the
    leaves' gradients stay within the bounds of the small parity cases."""
    hr = _hiprun()
    sc, og, g, radii = _case(variant, P, seed)
    seen = _spy_backward(monkeypatch)
    res = hr.run(variant, sc, og)
    assert len(seen) == 1 and seen[0][0] is False and seen[0][1] is None
    assert np.array_equal(res["radii"], radii)
    for a, b in _pairs(variant):
        print(variant, P, seed, a, float(np.abs(res["grads"][a]).max()), float(np.abs(np.asarray(res["grads"][a], np.float64).reshape(g[b].shape) - g[b]).max()))
        assert np.isfinite(res["grads"][a]).all()
        _grad_close(res["grads"][a], g[b])


def _raw(variant, sc, og, want_dcov3D=True, backwards=1):
    """gsrast.rasterize.forward, then `backwards` calls of gsrast.rasterize.backward on the same arenas -> list of gradient dicts (numpy)."""
    hr = _hiprun()
    from gsrast import rasterize as rz
    t = hr.to_dev(sc, "cuda")
    rs = hr.settings(variant, t)
    args = (t["means3D"], t.get("shs"), t.get("colors_precomp"), t["opacities"], t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"),
            t.get("all_map") if variant == "plane" else None)
    R, outs, radii, geom, binning, img = rz.forward(hr.VID[variant], *args, rs)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    kw = dict(grad_color=dev(og["dL_dcolor"]))
    if variant == "surfel":
        kw.update(grad_others=dev(og["dL_dothers"]))
    if variant == "plane":
        kw.update(grad_all_map=dev(og["dL_dout_all_map"]), grad_plane_depth=dev(og["dL_dplane_depth"]), all_map_pixels=outs["all_map"])
    out = []
    for _ in range(backwards):
        g = rz.backward(hr.VID[variant], R, rs, radii, *args, geom, binning, img, want_dcov3D=want_dcov3D, **kw)
        out.append({k: (None if v is None else v.cpu().numpy()) for k, v in g.items()})
    return out


@pytest.mark.parametrize("P,seed", [(P, s) for P in SIZES for s in SEEDS])
def test_surfel_means2D_is_the_transmat_gradient_times_the_forwards_depth(P, seed):
    """dL_dmeans2D[:, 0|1] of a visible surfel = dL_dtransMat[:, 2|5] * Tw.z * 0.5 * W|H (SURFEL backward.cu:633-636) with Tw.z the float the blend
    used -- read here from the record array -- and W, H as the kernel re-derives them in float32: bit for bit.  The kernel and the reference form the
    first product in float32 and the rest in float64; the same expression with every product in float64 rounds once instead of twice and may differ
    from it by one unit in the last place, no more.  Invisible rows are exactly 0."""
    hr = _hiprun()
    sc, og, g, radii = _case("surfel", P, seed)
    T8 = hr.run_raw("surfel", sc)["rec"][:, 8].astype(np.float32)
    got = _raw("surfel", sc, og)[0]
    assert got["dL_dcov3D"].shape == (P, 9)
    _grad_close(got["dL_dcov3D"], g["dL_dcov3D"])
    f32 = np.float32
    tanx, tany = f32(sc["tanfovx"]), f32(sc["tanfovy"])
    fx, fy = f32(W) / (f32(2.0) * tanx), f32(H) / (f32(2.0) * tany)
    Wb, Hb = int(f32(f32(fx * tanx) * f32(2.0))), int(f32(f32(fy * tany) * f32(2.0)))
    vis = radii > 0
    for col, k, n in ((0, 2, Wb), (1, 5, Hb)):
        dT = got["dL_dcov3D"][:, k].astype(np.float32)
        want = ((dT * T8).astype(np.float32).astype(np.float64) * 0.5 * float(f32(n))).astype(np.float32)
        have = got["dL_dmeans2D"][:, col]
        assert np.array_equal(have[vis].view(np.uint32), want[vis].view(np.uint32)), (col, int((have[vis] != want[vis]).sum()))
        once = (dT.astype(np.float64) * T8.astype(np.float64) * 0.5 * float(f32(n))).astype(np.float32)
        assert (np.abs(have[vis].astype(np.float64) - once[vis]) <= np.spacing(np.abs(once[vis]))).all()
        assert not have[~vis].any()
    assert not got["dL_dmeans2D"][:, 2].any()


@functools.lru_cache(maxsize=None)
def _precomp_case(variant, P, seed):
    """The case with its covariances (surfel: transMats) precomputed by the oracle and handed in through the cov3D_precomp slot."""
    sc, og, _, radii = _case(variant, P, seed)
    with oracle.Forward(sc, variant) as f:
        cov = f.geom()["cov"].copy()
    cov[radii == 0] = 0.0
    s2 = {k: v for k, v in sc.items() if k not in ("scales", "rotations")}
    s2["cov3D_precomp"] = cov
    if variant == "surfel":
        # a transMat of zeros is no surfel: the few rows the forward rejected in front of the camera go behind it too (culled by their depth before T is read)
        s2["means3D"] = sc["means3D"].copy()
        s2["means3D"][radii == 0, 2] = -np.abs(sc["means3D"][radii == 0, 2])
    with oracle.Forward(s2, variant) as f:
        g = f.backward(**og)
        r2 = f.radii.copy()
    return s2, og, g, r2


@pytest.mark.parametrize("variant,P,seed", CASES)
def test_bridge_with_precomp_delivers_its_gradient(variant, P, seed, monkeypatch):
    hr = _hiprun()
    s2, og, g, r2 = _precomp_case(variant, P, seed)
    seen = _spy_backward(monkeypatch)
    res = hr.run(variant, s2, og)
    assert len(seen) == 1 and seen[0][0] is True and seen[0][1] is not None
    assert np.array_equal(res["radii"], r2)
    got = res["grads"]["dL_dcov3D_precomp"]
    assert got is not None and got.shape == g["dL_dcov3D"].shape and np.isfinite(got).all()
    _grad_close(got, g["dL_dcov3D"])
    for a, b in (("dL_dmeans3D", "dL_dmeans3D"), ("dL_dopacities", "dL_dopacity"), ("dL_dmeans2D", "dL_dmeans2D"), ("dL_dcolors_precomp", "dL_dcolors")):
        _grad_close(res["grads"][a], g[b])


@pytest.mark.parametrize("want", [True, False])
@pytest.mark.parametrize("variant,P,seed", CASES)
def test_two_backwards_on_the_same_arenas_agree(variant, P, seed, want):
    """The second call adds into the accumulator rows the first one left behind: they agree only if the preprocess backward still clears every row it
    read, with and without the dL_dcov3D store."""
    sc, og, g, radii = _case(variant, P, seed)
    one, two = _raw(variant, sc, og, want_dcov3D=want, backwards=2)
    assert (one["dL_dcov3D"] is None) == (not want)
    for k in one:
        if one[k] is None or one[k].size == 0:      # (no SH coefficients in these scenes: dL_dsh is [P,0,3])
            continue
        assert np.isfinite(two[k]).all(), k
        _grad_close(two[k], one[k])
    for a, b in _pairs(variant):
        _grad_close(two[b], g[b])
