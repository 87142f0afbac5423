"""GPU: the plane rasterizer's per-Gaussian `all_map` prepare (csrc/gsr_extra.hip gsr_plane_allmap[_backward]) and the densification statistics
(gsr_densify_stats) at their decision and block edges.

all_map reference: tests/glue_truth.plane_allmap_autograd (float64 torch, gradients from autograd).  Bounds are tests/test_gpu_golden_ref.py's: values
rtol 1e-5 / atol 1e-6; gradients max |d| <= 1e-5 max |ref| for means3D, 5e-5 for rotations.  The random inputs stay clear of every decision (asserted on
the truth's intermediates); the decisions themselves -- equal scales, the camera centre in the Gaussian's plane, a signed distance of exactly 0 -- are
taken on rows of exactly representable numbers, where the values are compared exactly.
Statistics reference: tests/glue_truth.densify_stats."""
import numpy as np
import pytest
import torch

import glue_cases
import glue_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _allmap(xyz, q, sc, V, cp, dL):
    from gsrast.plane_prep import plane_input_all_map
    x = _t(xyz).requires_grad_(True); qq = _t(q).requires_grad_(True); s = _t(sc).requires_grad_(True)
    am = plane_input_all_map(x, qq, s, _t(V), _t(cp))
    (am * _t(dL)).sum().backward()
    assert s.grad is None                                                           # argmin: the scales get no gradient
    return am.detach().cpu().numpy(), x.grad.cpu().numpy(), qq.grad.cpu().numpy()


def _grad_close(got, ref, bar, what):
    e = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"PLANE-EDGE {what}: max|d| / max|ref| {e:.2e} (bar {bar:.0e})")
    assert e <= bar, (what, e)


@pytest.mark.parametrize("cols", [3, 6])
@pytest.mark.parametrize("P", glue_cases.PLANE_SIZES)
def test_allmap_against_float64_autograd(P, cols):
    xyz, q, sc, V, cp, dL = glue_cases.plane_random(P, cols)
    t = glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp, dL)
    assert glue_cases.plane_margins_ok(t, sc).all()                                  # no float32 / float64 decision can differ
    norms = np.linalg.norm(q.astype(np.float64), axis=1)
    assert norms.min() >= 0.29 and norms.max() <= 3.01 and (P < 255 or (norms.min() < 0.5 and norms.max() > 2.5))
    am, dx, dq = _allmap(xyz, q, sc, V, cp, dL)
    np.testing.assert_allclose(am, t["all_map"], rtol=1e-5, atol=1e-6)
    assert (am[:, 3] == 1).all()
    _grad_close(dx, t["d_xyz"], 1e-5, f"P={P} cols={cols} d_means3D")
    _grad_close(dq, t["d_q"], 5e-5, f"P={P} cols={cols} d_rotations")


def test_scale_stride_reads_the_first_three_columns():
    """(P,6) scales whose last three columns would pick another axis: same output as their first three columns alone."""
    P = 257
    xyz, q, sc, V, cp, dL = glue_cases.plane_random(P, 6)
    sc[:, 3:] = sc[:, :3].min(axis=1, keepdims=True) * 0.5
    a = _allmap(xyz, q, sc, V, cp, dL)
    b = _allmap(xyz, q, np.ascontiguousarray(sc[:, :3]), V, cp, dL)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_edge_rows_exactly():
    """First minimum among equal scales; dot == 0: no flip; signed distance == 0: distance 0 and nothing sent back through |.|."""
    xyz, q, sc, V, camposes, tags, want_k = glue_cases.plane_edge_rows()
    n = xyz.shape[0]
    dL = np.random.default_rng(4).normal(0, 1, (n, 5)).astype(np.float32)
    g4 = np.zeros((n, 5), np.float32); g4[:, 4] = 1.0
    seen = {"dot0": 0, "sd0": 0, "flip": 0}
    for cp in camposes:
        t = glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp, dL)
        assert np.array_equal(t["k"], want_k)
        am, dx, dq = _allmap(xyz, q, sc, V, cp, dL)
        bad = np.nonzero((am.astype(np.float64) != t["all_map"]).any(axis=1))[0]
        assert bad.size == 0, ([tags[i] for i in bad[:6]], am[bad[:6]], t["all_map"][bad[:6]])
        _grad_close(dx, t["d_xyz"], 1e-5, "edge rows d_means3D")
        _grad_close(dq, t["d_q"], 5e-5, "edge rows d_rotations")
        zero = t["sd"] == 0
        seen["dot0"] += int(((t["dot"] == 0) & ~zero).sum()); seen["sd0"] += int((zero & (t["dot"] != 0)).sum()); seen["flip"] += int((t["dot"] < 0).sum())
        assert (am[zero, 4] == 0).all()
        _, dx4, dq4 = _allmap(xyz, q, sc, V, cp, g4)                                 # only the distance carries a gradient
        assert not dx4[zero].any() and not dq4[zero].any()
        assert dx4[~zero].any(axis=1).all()
    assert all(v > 0 for v in seen.values()), seen


def test_misaligned_rotations_are_refused_on_the_host():
    """The kernels read rotations as float4: a view one float into its storage is refused before any launch, and the next valid call is right."""
    from gsrast.plane_prep import plane_input_all_map
    P = 257
    xyz, q, sc, V, cp, dL = glue_cases.plane_random(P, 3)
    buf = torch.empty(4 * P + 1, device=DEV)
    qv = buf[1:].view(P, 4)
    qv.copy_(_t(q))
    assert qv.data_ptr() % 16 == 4 and qv.is_contiguous()
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        plane_input_all_map(_t(xyz), qv, _t(sc), _t(V), _t(cp))
    am, _, _ = _allmap(xyz, q, sc, V, cp, dL)
    np.testing.assert_allclose(am, glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp)["all_map"], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------ densification statistics
NAMES = ("max_radii2D", "accum", "denom", "accum_abs", "denom_abs")


@pytest.mark.parametrize("filt", ["none", "all", "random"])
@pytest.mark.parametrize("P", glue_cases.DENSIFY_SIZES)
def test_densify_stats(P, filt):
    """Block edge (256 threads), the three filters, out_observe absent or present (with zeros), grad_stride 2 / 3 / 4 over a gradient whose columns past
    the second hold 1e30, with and without the _abs pair, two consecutive calls.  denom and max_radii2D exactly; accumulators rtol 1e-6 (the fixture's)."""
    from gsrast.stats import densification_stats_
    for stride in (2, 3, 4):
        for use_obs in (False, True):
            for use_abs in (False, True):
                c = glue_cases.densify_case(P, filt)
                assert (c["observe"] == 0).any() or P == 1
                g = np.ascontiguousarray(c["grad"][:, :stride]); ga = np.ascontiguousarray(c["grad_abs"][:, :stride]) if use_abs else None
                ob = c["observe"] if use_obs else None
                ref = {n: c[n].copy() for n in NAMES}
                dev = {n: _t(c[n]) for n in NAMES}
                for _ in range(2):
                    glue_truth.densify_stats(c["filter"], c["radii"], g, ref["max_radii2D"], ref["accum"], ref["denom"], ob, ga,
                                             ref["accum_abs"] if use_abs else None, ref["denom_abs"] if use_abs else None)
                    densification_stats_(dev["max_radii2D"], dev["accum"], dev["denom"], _t(g), torch.from_numpy(c["filter"]).to(DEV),
                                         torch.from_numpy(c["radii"]).to(DEV), None if ob is None else torch.from_numpy(ob).to(DEV),
                                         None if ga is None else _t(ga), dev["accum_abs"] if use_abs else None, dev["denom_abs"] if use_abs else None)
                key = (P, filt, stride, use_obs, use_abs)
                got = {n: dev[n].cpu().numpy() for n in NAMES}
                for n in ("denom", "max_radii2D", "denom_abs"):
                    assert np.array_equal(got[n], ref[n]), (key, n)
                for n in ("accum", "accum_abs"):
                    np.testing.assert_allclose(got[n], ref[n], rtol=1e-6, atol=0, err_msg=str((key, n)))
                if not use_abs or filt == "none":
                    assert np.array_equal(got["accum_abs"], c["accum_abs"]) and np.array_equal(got["denom_abs"], c["denom_abs"])
                if filt == "none":
                    assert all(np.array_equal(got[n], c[n]) for n in NAMES)
