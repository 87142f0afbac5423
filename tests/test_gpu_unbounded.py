"""GPU tests (pytest -m gpu) of gsrast.unbounded (gsr_unbounded_* of the C ABI, csrc/gsr_unbounded.hip): the lattice against the numpy restatement of
the contract (bit for bit), the frame-fused passes against the chain of the per-frame op gsrast.tsdf.tsdf_integrate_ (bit for bit) and against the
reference's own run (1e-4), marching cubes against the restatement on the same device-computed values (bit for bit, in canonical order, whatever the
slab), and the public entry point against the composition of its pieces."""
import functools
import os

import numpy as np
import pytest
import torch

import ref_unbounded_numpy as ref
from test_unbounded_cpu import GOLDEN, sphere_field

pytestmark = pytest.mark.gpu
CENTER, RADIUS = (0.1, -0.05, 2.6), 1.7


@functools.lru_cache(None)
def _fx():
    fx = np.load(os.path.join(GOLDEN, "ref_unbounded_lattice.npz")); fr = np.load(os.path.join(GOLDEN, "ref_tsdf_unbounded.npz"))
    dev = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).cuda() for k in ("full_proj", "depth", "rgb", "verts")}
    return fx, fr, dev


@functools.lru_cache(None)
def _axes_mixed():
    """(19, 33, 45) planes with |c| up to 1.6: mag covers < 1, (1, 1.9), > 1.9 and > 2."""
    return tuple(np.linspace(lo, hi, n).astype(np.float32) for lo, hi, n in ((-1.6, 1.55, 19), (-1.5, 1.6, 33), (-1.6, 1.6, 45)))


def _chain(pts, tr, P, depth, rgb):
    """The per-frame op, once per frame, on materialised points: the way the parent commit runs the pass."""
    from gsrast.tsdf import tsdf_integrate_
    V = int(pts.shape[0])
    t, c, w = torch.ones(V, device="cuda"), torch.zeros((V, 3), device="cuda"), torch.ones(V, device="cuda")
    for f in range(len(P)):
        tsdf_integrate_(pts, P[f], depth[f], rgb[f], tr, t, c, w)
    return t, c, w


def test_lattice_points_bit_exact():
    from gsrast.unbounded import lattice_points
    axes = _axes_mixed()
    vox = np.float32(RADIUS * 2 / 64)
    pts, tr = lattice_points(*axes, CENTER, RADIUS, vox)
    wp, wt = ref.lattice_points(*axes, CENTER, RADIUS, vox)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    mag = np.sqrt(X.astype(np.float64) ** 2 + Y ** 2 + Z ** 2).ravel()
    for lo, hi in ((0, 1), (1, 1.9), (1.9, 2), (2, 9)):
        assert ((mag > lo) & (mag < hi)).sum() > 50
    assert pts.shape == (19 * 33 * 45, 3) and tr.shape == (19 * 33 * 45,)
    assert pts.cpu().numpy().tobytes() == wp.tobytes()
    assert tr.cpu().numpy().tobytes() == wt.tobytes()


@pytest.mark.parametrize("F", [1, 3])
def test_lattice_tsdf_equals_the_per_frame_chain(F):
    from gsrast.unbounded import lattice_points, lattice_tsdf
    _, _, d = _fx()
    axes = _axes_mixed()                                              # 19 * 33 * 45 samples: rows of 45 and a total that is no multiple of 4
    vox = np.float32(RADIUS * 2 / 64)
    pts, tr = lattice_points(*axes, CENTER, RADIUS, vox)
    want, _, _ = _chain(pts, tr, d["full_proj"][:F], d["depth"][:F], d["rgb"][:F])
    got = lattice_tsdf(*axes, CENTER, RADIUS, vox, d["full_proj"][:F], d["depth"][:F])
    assert got.shape == (19, 33, 45) and (got != 1).sum() > 500
    assert torch.equal(got.reshape(-1), want)
    # one more frame that no sample projects into (w = -1 whatever the point): nothing changes
    away = d["full_proj"][:1].clone()
    away[0, :, 3] = torch.tensor([0.0, 0.0, 0.0, -1.0], device="cuda")
    P2 = torch.cat([d["full_proj"][:F], away]); D2 = torch.cat([d["depth"][:F], d["depth"][:1]])
    assert torch.equal(lattice_tsdf(*axes, CENTER, RADIUS, vox, P2, D2), got)


def test_lattice_tsdf_ragged_frames_carry_the_state():
    """Frames of three sizes in a row: one launch per run of equal sizes with (tsdf, weight) carried, equal to the chain frame by frame."""
    from gsrast.unbounded import lattice_points, lattice_tsdf
    _, _, d = _fx()
    axes = tuple(a[:n] for a, n in zip(_axes_mixed(), (7, 9, 45)))
    vox = np.float32(RADIUS * 2 / 64)
    depth = [d["depth"][0], d["depth"][1][:, :40, :52].contiguous(), d["depth"][2]]
    rgb = [d["rgb"][0], d["rgb"][1][:, :40, :52].contiguous(), d["rgb"][2]]
    pts, tr = lattice_points(*axes, CENTER, RADIUS, vox)
    want, _, ww = _chain(pts, tr, d["full_proj"], depth, rgb)
    got = lattice_tsdf(*axes, CENTER, RADIUS, vox, d["full_proj"], depth)
    assert torch.equal(got.reshape(-1), want)
    t0 = torch.ones((7, 9, 45), device="cuda"); w0 = torch.ones((7, 9, 45), device="cuda")
    t1, w1 = lattice_tsdf(*axes, CENTER, RADIUS, vox, d["full_proj"], depth, state=(t0, w0))
    assert torch.equal(t1.reshape(-1), want) and torch.equal(w1.reshape(-1), ww)


def test_lattice_tsdf_meets_the_reference_run():
    from gsrast.unbounded import lattice_axes, lattice_tsdf
    fx, _, d = _fx()
    R, st, res = float(fx["R"]), int(fx["stride"]), int(fx["resolution"])
    sub = [a[::st] for a in lattice_axes((-R,) * 3, (R,) * 3, res, int(fx["crop"]))]
    got = lattice_tsdf(*sub, fx["center"], float(fx["radius"]), np.float32(float(fx["radius"]) * 2 / res), d["full_proj"], d["depth"]).cpu().numpy()
    want = fx["volume"]
    assert got.shape == want.shape
    err = np.abs(got - want)
    print(f"lattice vs reference: max error {err.max():.2e}")
    assert err.max() <= 1e-4 and np.array_equal(got < 0, want < 0)


@functools.lru_cache(None)
def _scene33():
    """The fixture scene at crop 17, resolution 34: a 33^3 lattice whose surface crosses the block plane; values computed on the device."""
    from gsrast.unbounded import lattice_axes, lattice_tsdf
    fx, _, d = _fx()
    R = float(fx["R"])
    axes = lattice_axes((-R,) * 3, (R,) * 3, 34, 17)
    f = lattice_tsdf(*axes, CENTER, RADIUS, np.float32(RADIUS * 2 / 34), d["full_proj"], d["depth"])
    return axes, f


def _hand_set():
    rng = np.random.default_rng(11)
    f = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 1.0], np.float32), size=(9, 6, 7)).astype(np.float32)
    f[-1] = np.where((np.arange(6)[:, None] + np.arange(7)[None, :]) % 2 == 0, -0.75, 0.5)          # a sign change on the last plane of every axis
    f[:, -1, :] = -f[:, -2, :] - np.float32(0.125)
    f[:, :, -1] = np.where(f[:, :, -2] < 0, 0.5, -0.5)
    axes = (np.cumsum(rng.uniform(0.1, 0.3, 9)).astype(np.float32), np.cumsum(rng.uniform(0.1, 0.3, 6)).astype(np.float32),
            np.cumsum(rng.uniform(0.1, 0.3, 7)).astype(np.float32))
    assert (f == 0).sum() > 20
    return axes, f


def _mc_case(name):
    if name == "scene33":
        axes, f = _scene33()
        return axes, f
    if name == "sphere":
        axes = _axes_mixed()
        return axes, torch.from_numpy(sphere_field(axes, centre=(0.2, -0.1, 0.05), r=0.9)).cuda()
    if name == "hand":
        axes, f = _hand_set()
        return axes, torch.from_numpy(f).cuda()
    return _axes_mixed(), torch.ones((19, 33, 45), device="cuda")


@pytest.mark.parametrize("name", ["scene33", "sphere", "hand", "ones"])
def test_marching_cubes_equals_the_restatement(name):
    from gsrast.unbounded import lattice_marching_cubes
    axes, f = _mc_case(name)
    wv, wt = ref.marching_cubes(f.cpu().numpy(), *axes)
    if name == "ones":
        assert len(wv) == 0 and len(wt) == 0
    else:
        assert len(wv) > 100 and len(wt) > 100
    if name == "scene33":                          # the surface crosses the block plane (index 16) of the x axis
        gx = np.searchsorted(axes[0], wv[:, 0], side="right") - 1
        assert (gx == 15).any() and (gx == 16).any()
    for slab in (None, 2, 7):
        v, t = lattice_marching_cubes(f, *axes, slab=slab)
        assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape == (len(wv), 3) and t.shape == (len(wt), 3), (slab, v.shape, t.shape)
        assert v.cpu().numpy().tobytes() == wv.tobytes(), slab
        assert t.cpu().numpy().tobytes() == wt.tobytes(), slab


def test_marching_cubes_scans_more_than_1024_workgroups():
    """A 68 x 64 x 64 lattice: a plane is 16 workgroups of 256 points, so the one-workgroup scan over the workgroups' sums takes a second chunk of
    1024 and carries the first chunk's total into it.  One slab: 1088 workgroups.  slab=66: the first slab owns 65 planes, and its first point
    that is not owned, whose prefix is the slab's vertex count, lies in workgroup 1040, past the first chunk.  slab=64: exactly 1024 workgroups."""
    from gsrast.unbounded import lattice_marching_cubes, slab_plan
    rng = np.random.default_rng(5)
    axes = tuple(np.cumsum(rng.uniform(0.03, 0.06, n)).astype(np.float32) - np.float32(0.045 * n / 2) for n in (68, 64, 64))
    f = sphere_field(axes, centre=(0.1, -0.05, 0.02), r=1.38)
    groups = lambda slab: [(min(own + 1, planes) * 64 * 64 // 256, own * 64 * 64 // 256) for _, own, planes in slab_plan(68, slab)]
    assert groups(None) == [(1088, 1088)]
    assert groups(66)[0] == (1056, 1040) and groups(64)[0] == (1024, 1008)
    wv, wt = ref.marching_cubes(f, *axes)
    gx = np.searchsorted(axes[0], wv[:, 0], side="right") - 1
    assert len(wv) > 10000 and gx.min() < 10 and (gx >= 65).sum() > 100      # the surface has vertices in the workgroups of both chunks: planes up to 63, and 64 on
    ft = torch.from_numpy(f).cuda()
    for slab in (None, 66, 64):
        v, t = lattice_marching_cubes(ft, *axes, slab=slab)
        assert v.shape == (len(wv), 3) and t.shape == (len(wt), 3), (slab, v.shape, t.shape)
        assert v.cpu().numpy().tobytes() == wv.tobytes(), slab
        assert t.cpu().numpy().tobytes() == wt.tobytes(), slab


@pytest.mark.parametrize("V", [1, 5, 3000])
def test_texture_equals_the_per_frame_chain(V):
    from gsrast.unbounded import texture_vertices
    _, fr, d = _fx()
    vox = np.float32(fr["voxel_size"])
    verts = d["verts"][:V].contiguous()
    _, want, _ = _chain(verts, float(np.float32(5) * vox), d["full_proj"], d["depth"], d["rgb"])
    got = texture_vertices(verts, vox, d["full_proj"], d["depth"], d["rgb"])
    assert got.shape == (V, 3) and torch.equal(got, want)
    if V == 3000:
        err = np.abs(got.cpu().numpy() - fr["vert_rgb"]).max()
        print(f"texture vs reference: max error {err:.2e}")
        assert err <= 1e-4 and (got != 0).any()


def test_contraction_bound():
    from gsrast.unbounded import contraction_bound
    fx, _, _ = _fx()
    got = contraction_bound(torch.from_numpy(fx["xyz"]).cuda(), fx["center"], float(fx["radius"]))
    assert abs(got - float(fx["R"])) <= 1e-6


def test_extract_mesh_unbounded_end_to_end(tmp_path):
    import gsrast
    from gsrast import ply, unbounded as ub
    fx, _, d = _fx()
    xyz = torch.from_numpy(fx["xyz"]).cuda()
    args = (d["full_proj"], d["depth"], d["rgb"], xyz, CENTER, RADIUS)
    mesh = gsrast.extract_mesh_unbounded(*args, resolution=34, crop=17, slab=7)
    # the composition of the pieces
    R = ub.contraction_bound(xyz, CENTER, RADIUS)
    vox = np.float32(RADIUS * 2 / 34)
    axes = ub.lattice_axes((-R,) * 3, (R,) * 3, 34, 17)
    f = ub.lattice_tsdf(*axes, CENTER, RADIUS, vox, d["full_proj"], d["depth"])
    v, t = ub.lattice_marching_cubes(f, *axes)
    contracted = v.cpu().numpy().copy()
    v = ub.finish_vertices(v, CENTER, RADIUS, 32.0)
    assert v.cpu().numpy().tobytes() == ref.finish(contracted, CENTER, RADIUS, 32.0).tobytes()
    c = ub.texture_vertices(v, vox, d["full_proj"], d["depth"], d["rgb"])
    assert len(v) > 100 and len(t) > 100
    assert torch.equal(mesh.vertices, v) and torch.equal(mesh.triangles, t) and torch.equal(mesh.vertex_colors, c)
    assert torch.equal(gsrast.extract_mesh_unbounded(*args, resolution=34, crop=17, slab=None).vertices, v)
    # the clip acts on world coordinates
    clipped = gsrast.extract_mesh_unbounded(*args, resolution=34, crop=17, slab=7, max_range=0.5)
    assert float(clipped.vertices.abs().max()) == 0.5 and float(v.abs().max()) > 0.5 and torch.equal(clipped.triangles, t)
    assert clipped.vertices.cpu().numpy().tobytes() == ref.finish(contracted, CENTER, RADIUS, 0.5).tobytes()
    # the result feeds the post-processing and the PLY writer unchanged
    post = gsrast.post_process_mesh(mesh, cluster_to_keep=1)
    assert 0 < post.triangles.shape[0] <= t.shape[0] and post.vertices.shape[0] <= v.shape[0]
    path = os.path.join(tmp_path, "unbounded.ply")
    ply.write_triangle_mesh(path, mesh)
    back = ply.read_triangle_mesh(path)
    assert torch.equal(back.vertices, mesh.vertices.cpu()) and torch.equal(back.triangles, mesh.triangles.cpu())
    assert float((back.vertex_colors - mesh.vertex_colors.cpu().clamp(0, 1)).abs().max()) <= 1.0 / 255.0
