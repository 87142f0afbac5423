"""CPU checks of the unbounded mesh path (gsrast.unbounded, gsr_unbounded_* of include/gsrast.h): the numpy float32 restatement of the contract
(ref_unbounded_numpy) against the lattice the reference's own extract_mesh_unbounded produced (tests/golden/ref_unbounded_lattice.npz), the lattice
axes, the restatement's marching cubes on an analytic sphere that crosses the block planes, and the C entry points' argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_mesh_numpy as mesh_ref
import ref_unbounded_numpy as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ["gsr_unbounded_lattice_points", "gsr_unbounded_lattice_tsdf", "gsr_unbounded_mc_scratch_bytes", "gsr_unbounded_mc_count", "gsr_unbounded_mc_emit",
       "gsr_unbounded_finish", "gsr_unbounded_texture"]


def test_restatement_matches_the_reference_lattice():
    """The reference ran extract_mesh_unbounded(resolution=512) through its real marching_cubes_with_contraction; the fixture keeps every 9th plane of
    its 512^3 volume.  The restatement of include/gsrast.h's formulas on those planes: within 1e-4 absolute (the bar of
    test_tsdf_matches_reference_run), every sample compared, no sign disagreement."""
    from gsrast.unbounded import lattice_axes
    fx = np.load(os.path.join(GOLDEN, "ref_unbounded_lattice.npz")); fr = np.load(os.path.join(GOLDEN, "ref_tsdf_unbounded.npz"))
    R, st, res = float(fx["R"]), int(fx["stride"]), int(fx["resolution"])
    axes = lattice_axes((-R,) * 3, (R,) * 3, res, int(fx["crop"]))
    sub = [a[::st] for a in axes]
    want = fx["volume"]
    assert want.shape == tuple(len(a) for a in sub) == (57, 57, 57)
    got = ref.lattice_tsdf(*sub, fx["center"], float(fx["radius"]), np.float32(float(fx["radius"]) * 2 / res), fr["full_proj"], fr["depth"])
    err = np.abs(got - want)
    print(f"lattice: max error {err.max():.2e}, {float((want != 1).mean()):.4f} of the samples off 1, {int((want < 0).sum())} negative")
    assert np.isfinite(got).all() and got.shape == want.shape
    assert err.max() <= 1e-4
    assert np.array_equal(got < 0, want < 0)
    assert (want != 1).sum() > 1000          # the comparison is not one of untouched samples only
    # the strided planes hold 2 negative samples; the fixture also keeps, by index, every negative sample of the reference's volume and a share of the
    # small positive ones: the same bar there, and the sign of every one of them
    idx, bval = fx["band_index"].astype(np.int64), fx["band_value"]
    assert (bval < 0).sum() > 1000 and (bval >= 0).sum() > 1000
    pts, tr = ref.uncontract(np.stack([axes[a][idx[:, a]] for a in range(3)], 1), fx["center"], float(fx["radius"]), np.float32(float(fx["radius"]) * 2 / res))
    bgot = ref.fuse(pts, tr, fr["full_proj"], fr["depth"])
    print(f"band: {len(bval)} samples, {int((bval < 0).sum())} negative, max error {np.abs(bgot - bval).max():.2e}")
    assert np.abs(bgot - bval).max() <= 1e-4
    assert np.array_equal(bgot < 0, bval < 0)


def test_lattice_axes():
    from gsrast.unbounded import lattice_axes
    for lo, hi, res, crop in (((-1.4723, -1.4723, -1.4723), (1.4723, 1.4723, 1.4723), 1024, 512), ((-1.0, -0.7, 0.1), (1.3, 0.9, 1.9), 36, 9),
                              ((-1.9, -1.9, -1.9), (1.9, 1.9, 1.9), 17, 17)):
        N = res // crop
        axes = lattice_axes(lo, hi, res, crop)
        for a in range(3):
            ax = axes[a]
            assert ax.dtype == np.float32 and len(ax) == N * (crop - 1) + 1 and (np.diff(ax) > 0).all()
            edges = np.linspace(lo[a], hi[a], N + 1)
            import torch
            for b in range(N):
                blk = torch.linspace(edges[b], edges[b + 1], crop).numpy()
                assert blk.tobytes() == ax[b * (crop - 1):b * (crop - 1) + crop].tobytes()          # every crop of the reference, duplicates bit-equal
    with pytest.raises(RuntimeError):
        lattice_axes((-1,) * 3, (1,) * 3, 30, 17)


def _warped_axes():
    from gsrast.unbounded import lattice_axes
    axes = lattice_axes((-1.0, -0.9, -1.1), (1.2, 1.0, 0.9), 26, 13)          # two blocks per axis, 25 planes
    return [(a + np.float32(0.15) * a * a * a).astype(np.float32) for a in axes]          # monotone warp: non-uniform spacing


def sphere_field(axes, centre=(0.13, 0.02, -0.07), r=0.55, band=0.3):
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in axes], indexing="ij")
    sdf = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    return np.minimum(1.0, sdf / band).astype(np.float32)


def test_restatement_on_a_sphere_across_the_block_planes():
    axes = _warped_axes()
    f = sphere_field(axes)
    for a, ax in enumerate(axes):                  # the surface crosses the block plane (index 12) of every axis
        assert (np.take(f, 12, axis=a) < 0).any() and (np.take(f, 12, axis=a) > 0).any()
    v, t = ref.marching_cubes(f, *axes)
    topo = mesh_ref.topology(t, len(v))
    assert topo == dict(watertight=True, euler=2, unused=0)
    sv, st = mesh_ref.extract(*mesh_ref.sphere(), 0.05)[0::2]
    vol = mesh_ref.signed_volume(v, t)
    assert vol * mesh_ref.signed_volume(sv, st) > 0          # the same orientation as the bounded path's sphere
    assert 0.9 < vol / (4.0 / 3.0 * np.pi * 0.55 ** 3) < 1.0
    assert np.abs(np.linalg.norm(v.astype(np.float64) - np.array((0.13, 0.02, -0.07)), axis=1) - 0.55).max() < 0.02
    # canonical order: vertices ascend in (gx, gy, gz, axis) -- their lower lattice point never decreases
    key = [np.searchsorted(ax, v[:, a], side="right") - 1 for a, ax in enumerate(axes)]
    flat = (key[0] * 25 + key[1]) * 25 + key[2]
    assert (np.diff(flat) >= 0).all()


def test_finish_and_texture_restatement_against_the_reference_run():
    """The un-contraction without truncation inverts the reference's contraction, and the texturing pass meets ref_tsdf_unbounded.npz's colours."""
    fr = np.load(os.path.join(GOLDEN, "ref_tsdf_unbounded.npz"))
    col = ref.texture(fr["verts"], np.float32(fr["voxel_size"]), fr["full_proj"], fr["depth"], fr["rgb"])
    assert np.abs(col - fr["vert_rgb"]).max() <= 1e-4
    c = np.array([[0.2, -0.1, 0.3], [0.9, 0.8, -0.7], [1.2, 0.1, 0.0]], np.float32)
    w = ref.finish(c, (0.1, -0.05, 2.6), 1.7, max_range=3.0)
    mag = np.linalg.norm(c.astype(np.float64), axis=1, keepdims=True)
    want = np.where(mag < 1, c, c / mag / (2 - mag)) * 1.7 + np.array((0.1, -0.05, 2.6))
    assert np.allclose(w, np.clip(want, -3.0, 3.0), atol=1e-5) and (np.abs(w) <= 3.0).all() and (np.abs(want) > 3.0).any()


def test_new_symbols_are_exported_and_the_abi_version_stays():
    import gsrast
    L = gsrast.lib()
    for s in NEW:
        assert s in gsrast.EXPORTS and hasattr(L, s)
    assert gsrast.ABI_VERSION == 8 and L.gsr_abi_version() == 8
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "gsrast.h")).read()
    assert "#define GSR_ABI_VERSION 8" in hdr
    assert gsrast.extract_mesh_unbounded is gsrast.unbounded.extract_mesh_unbounded


def test_argument_errors_without_a_device():
    """gsr_unbounded_* validate sizes, pointers, alignment and scratch before touching the device."""
    import gsrast
    L = gsrast.lib()
    buf = (C.c_float * 256)()
    a = C.addressof(buf)
    a += (-a) % 16                                   # a 16-byte aligned address inside buf
    ctr = (C.c_float * 3)(0.0, 0.0, 0.0)

    def err(rc, word):
        return rc != 0 and word in gsrast.last_error()
    tsdf = lambda **k: L.gsr_unbounded_lattice_tsdf(k.get("nx", 4), 4, 4, k.get("xs", a), a, a, k.get("ctr", ctr), 1.0, 0.1, k.get("F", 2), a, 8, 8, a,
                                                    k.get("out", a), k.get("w", None), None)
    assert err(tsdf(nx=1), "at least 2 planes")
    assert err(tsdf(xs=None), "null pointer")
    assert err(tsdf(ctr=None), "null pointer")
    assert err(tsdf(out=None), "null pointer")
    assert err(tsdf(out=a + 4), "aligned")
    assert err(tsdf(w=a + 8), "aligned")
    assert err(tsdf(F=0), "bad sizes")
    assert err(L.gsr_unbounded_lattice_points(4, 1, 4, a, a, a, ctr, 1.0, 0.1, a, a, None), "at least 2 planes")
    assert err(L.gsr_unbounded_lattice_points(4, 4, 4, a, a, a, ctr, 1.0, 0.1, None, a, None), "null pointer")
    assert err(L.gsr_unbounded_lattice_points(4, 4, 4, a, a, a, ctr, -1.0, 0.1, a, a, None), "positive")
    need = L.gsr_unbounded_mc_scratch_bytes(4, 4, 4)
    assert 4 * 64 <= need <= 4 * 64 + 4096
    cnt = (C.c_uint64 * 2)()
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 4, a, a, need - 1, 0, 0, cnt, None), "scratch")
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 4, a, a + 4, need, 0, 0, cnt, None), "scratch")
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 4, None, a, need, 0, 0, cnt, None), "null pointer")
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 4, a, a, need, 0, 0, None, None), "null pointer")
    assert err(L.gsr_unbounded_mc_count(1, 4, 4, 1, a, a, need, 0, 0, cnt, None), "at least 2 planes")
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 3, a, a, need, 0, 0, cnt, None), "owns")          # a slab that does not end the lattice needs two planes behind
    assert err(L.gsr_unbounded_mc_count(4, 4, 4, 0, a, a, need, 0, 0, cnt, None), "owns")
    assert err(L.gsr_unbounded_mc_count(1024, 1024, 1024, 1024, a, a, 1 << 40, 0, 0, cnt, None), "smaller slab")
    assert err(L.gsr_unbounded_mc_emit(4, 4, 4, 4, a, a, a, a, a, need, 0, 5, 5, None, a, None), "null pointer")
    assert err(L.gsr_unbounded_mc_emit(4, 4, 4, 4, a, None, a, a, a, need, 0, 5, 5, a, a, None), "null pointer")
    assert err(L.gsr_unbounded_mc_emit(4, 4, 4, 4, a, a, a, a, a, need, (1 << 31) - 3, 5, 5, a, a, None), "bad counts")
    assert err(L.gsr_unbounded_finish(5, ctr, 1.0, 32.0, None, None), "null pointer")
    assert err(L.gsr_unbounded_finish(-1, ctr, 1.0, 32.0, a, None), "bad sizes")
    assert err(L.gsr_unbounded_texture(5, a, 0.1, 0, a, 8, 8, a, a, a, None), "bad sizes")
    assert err(L.gsr_unbounded_texture(5, a, 0.1, 2, a, 8, 8, a, None, a, None), "null pointer")
    assert err(L.gsr_unbounded_texture(5, None, 0.1, 2, a, 8, 8, a, a, a, None), "null pointer")
    # nothing to do is no error and touches no device
    assert L.gsr_unbounded_finish(0, ctr, 1.0, 32.0, None, None) == 0 and L.gsr_unbounded_texture(0, None, 0.1, 2, a, 8, 8, a, a, None, None) == 0


def test_slab_plan_covers_every_plane_once():
    from gsrast.unbounded import slab_plan
    for nx in (2, 3, 9, 33, 45):
        for slab in (None, 2, 3, 7, 32, nx, nx + 5):
            plan = slab_plan(nx, slab)
            x = 0
            for x0, own, np_ in plan:
                assert x0 == x and own >= 1 and x0 + np_ <= nx and (own == np_ or own + 2 <= np_)
                assert slab is None or np_ <= max(int(slab), 2) + 1
                x += own
            assert x == nx and plan[-1][1] == plan[-1][2]
