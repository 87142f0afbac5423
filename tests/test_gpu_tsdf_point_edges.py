"""GPU: the per-point TSDF update (csrc/gsr_extra.hip gsr_tsdf_integrate) on each of its paths: the float4 kernel with and without a scalar tail,
the scalar kernel as the whole job (V < 4, or any buffer off a 16-byte boundary), per-point truncation through both, and the fetch without the packed
(r,g,b,d) scratch.

Scene (tests/glue_cases.py): one or two 48 x 32 frames into one state; points in front of, around and far behind a smooth surface, outside the
frustum, behind the camera, and on the last texel column, where the right-hand corners of the bilinear stencil fall outside the image.
Reference: tests/glue_truth.tsdf_frame, float64, its mask decisions made in float32 with the kernel's expressions.  Weights are exact; TSDF and colour
within 1e-4, the project's bound for this update (tests/test_gpu_parity.py): the float32 cancellation in depth(u, v) - z at depth 5 is a few ulps of
4.8e-7, the depth map moves by at most 0.06 per pixel so a pixel coordinate off by 1e-5 adds < 1e-6, and the smallest truncation dividing it is 0.1."""
import numpy as np
import pytest
import torch

import glue_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = glue_cases.TSDF_W, glue_cases.TSDF_H


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _shift(t):
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _integrate(pts, cams, depth, rgb, trunc, frames, shift=False, scratch=True):
    """-> (tsdf, weight, rgb) device tensors after `frames` frames from (1, 1, 0).  shift: every per-point buffer one float off alignment.
    scratch=False: the C entry directly with rgbd_scratch = NULL (three single-channel fetches per colour)."""
    import gsrast
    from gsrast.tsdf import tsdf_integrate_
    V = pts.shape[0]
    place = _shift if shift else (lambda t: t)
    p = place(_t(pts)); ts = place(torch.ones(V, device=DEV)); w = place(torch.ones(V, device=DEV)); c = place(torch.zeros(V, 3, device=DEV))
    tp = place(_t(trunc)) if np.ndim(trunc) else None
    for fr in range(frames):
        F, d, col = _t(cams[fr]["projmatrix"]), _t(depth[fr]), _t(rgb[fr])
        if scratch:
            tsdf_integrate_(p, F, d, col, tp if tp is not None else float(trunc), ts, c, w)
        else:
            rc = gsrast.lib().gsr_tsdf_integrate(V, p.data_ptr(), F.data_ptr(), W, H, d.data_ptr(), col.data_ptr(), 0.0 if tp is not None else float(trunc),
                                                 None if tp is None else tp.data_ptr(), ts.data_ptr(), w.data_ptr(), c.data_ptr(), None,
                                                 gsrast.stream_ptr(torch.device(DEV)))
            assert rc == 0, gsrast.last_error()
    if shift:
        assert all(x.data_ptr() % 16 == 4 for x in (p, ts, w, c) + ((tp,) if tp is not None else ()))
    return ts, w, c


def _check_kinds(state, info):
    t, w, c = state
    upd = info["updated"]
    assert np.array_equal(w > 1, upd) and upd.mean() >= 0.25
    assert info["behind"].any() and (~info["in_frustum"] & ~info["behind"]).any()
    assert (info["in_frustum"] & ~(info["sdf32"] > -info["trunc32"])).any()
    assert (upd & (info["x_pix"] == W - 1)).any()


def _trunc(V, per_point):
    return glue_cases.tsdf_trunc_pp(V) if per_point else glue_cases.TSDF_TRUNC


@pytest.mark.parametrize("per_point", [False, True], ids=["scalar", "perpoint"])
@pytest.mark.parametrize("frames", [1, 2])
@pytest.mark.parametrize("V", glue_cases.TSDF_SIZES)
def test_against_float64_truth(V, frames, per_point):
    trunc = _trunc(V, per_point)
    pts, cams, depth, rgb, truth, info = glue_cases.tsdf_truth(V, frames, trunc)
    if V >= 8:
        _check_kinds(glue_cases.tsdf_truth(V, 1, trunc)[4], info)
    ts, w, c = (x.cpu().numpy() for x in _integrate(pts, cams, depth, rgb, trunc, frames))
    et, ec = np.abs(ts - truth[0]).max(), np.abs(c - truth[2]).max()
    print(f"TSDF-EDGE V={V} frames={frames} per_point={per_point}: max |tsdf - truth| {et:.2e}, |rgb - truth| {ec:.2e}, updated {(truth[1] > 1).mean():.2f}")
    assert np.array_equal(w, truth[1])
    assert et < 1e-4 and ec < 1e-4, (et, ec)


@pytest.mark.parametrize("per_point", [False, True], ids=["scalar", "perpoint"])
@pytest.mark.parametrize("V", [3, 5, 1027])
def test_unaligned_buffers_against_float64_truth(V, per_point):
    """Every per-point buffer one float off: the scalar kernel is the whole job, with its own read of the per-point truncation."""
    trunc = _trunc(V, per_point)
    pts, cams, depth, rgb, truth, info = glue_cases.tsdf_truth(V, 2, trunc)
    ts, w, c = (x.cpu().numpy() for x in _integrate(pts, cams, depth, rgb, trunc, 2, shift=True))
    assert np.array_equal(w, truth[1])
    assert np.abs(ts - truth[0]).max() < 1e-4 and np.abs(c - truth[2]).max() < 1e-4


def test_paths_give_the_same_bits():
    """V = 1027 (256 float4 groups and a 3-point tail), two frames.  All paths run tsdf_point, and bilinear_border4 is bit-identical per channel to
    bilinear_border: aligned == every buffer shifted one float; scalar truncation == a per-point tensor filled with that value; packed scratch == the
    direct call without it."""
    V = 1027
    trunc = glue_cases.TSDF_TRUNC
    pts, cams, depth, rgb, truth, info = glue_cases.tsdf_truth(V, 2, trunc)
    _check_kinds(glue_cases.tsdf_truth(V, 1, trunc)[4], info)
    base = _integrate(pts, cams, depth, rgb, trunc, 2)
    assert (base[1] > 1).float().mean().item() >= 0.25
    full = np.full(V, trunc, np.float32)
    tpp = glue_cases.tsdf_trunc_pp(V)
    base_pp = _integrate(pts, cams, depth, rgb, tpp, 2)
    assert not torch.equal(base_pp[0], base[0])
    for what, got, ref in (("shifted", _integrate(pts, cams, depth, rgb, trunc, 2, shift=True), base),
                           ("per-point tensor of one value", _integrate(pts, cams, depth, rgb, full, 2), base),
                           ("per-point tensor of one value, shifted", _integrate(pts, cams, depth, rgb, full, 2, shift=True), base),
                           ("no scratch", _integrate(pts, cams, depth, rgb, trunc, 2, scratch=False), base),
                           ("no scratch, shifted", _integrate(pts, cams, depth, rgb, trunc, 2, shift=True, scratch=False), base),
                           ("varying truncation, shifted", _integrate(pts, cams, depth, rgb, tpp, 2, shift=True), base_pp),
                           ("varying truncation, no scratch", _integrate(pts, cams, depth, rgb, tpp, 2, scratch=False), base_pp)):
        for name, a, b in zip(("tsdf", "weight", "rgb"), got, ref):
            diff = torch.nonzero((a != b).reshape(V, -1).any(dim=1)).reshape(-1)
            assert diff.numel() == 0, (what, name, diff[:8].tolist(), a.reshape(V, -1)[diff[:8]].tolist(), b.reshape(V, -1)[diff[:8]].tolist())
