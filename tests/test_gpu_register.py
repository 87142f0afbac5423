"""GPU tests (pytest -m gpu) of gsrast.register and chamfer.NearestGrid (the "registration" section of the C ABI, csrc/gsr_register.hip, and the
build / query halves of gsr_nearest_points) against the restatements of tests/register_truth.py on the named inputs of tests/register_cases.py.

Compared with np.array_equal: NearestGrid against nearest_points, transform_points, crop_polygon_volume, the counts of the sums, and solve_transform
against truth.solve fed with the device's own record (float64 division and square root are IEEE, contraction is off: the same operations give the
same bits).

The sums: means and raw sums against math.fsum at rtol = 1e-12 on clouds with positive coordinates, the bar of test_gpu_chamfer.  The order of the
float64 additions is the only difference from math.fsum, and a value passes through few of them: at most 5 in its thread (4 elements a thread
while the grid of blocks grows, 1024 blocks of 256 threads at the most, so 5 at the one size past that), 6 + 2 in the block's butterfly and wave
sum, then in the finish kernel 4 in a thread (1024 partials over 256 threads) and 6 + 2 again: 25 roundings of 2^-53 on non-negative terms, 3e-15
relative, and one more for the mean's division.  The centred sums are recomputed by the truth WITH THE DEVICE'S OWN MEANS (read back) -- every term
is then the same float64 number on both sides -- and held to 1e-12 x the sum of the absolute values of the terms: the same 25 roundings.

icp: iterations, converged, status, n_inliers and fitness equal the truth's exactly, inlier_rmse at rtol 1e-9, and the transformation within
TRANSFORM_BAR = 6.0e-12 per element: 8 x the 7.4e-13 by which the truth's own final transformation moves (largest over the four main cases, the
partial-overlap one) when every sum of every iteration is moved by a relative 1e-12, the bar the sums are held to; test_register_cpu measures it
again on every run and holds the constant to it."""
import math
import warnings

import numpy as np
import pytest
import torch

import chamfer_cases
import register_cases as cases
import register_truth as truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def count_syncs(fn):
    """Host synchronisations of fn() as torch's sync debug mode reports them (tests/test_gpu_create_anchors.py's way)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower()), out


def _views(a):
    """The three layouts of test_gpu_chamfer._views: packed, a view one float into its storage, the first three columns of [P,4]."""
    P = a.shape[0]
    buf = torch.empty(3 * P + 1, device=DEV)
    view = buf[1:].view(P, 3)
    view.copy_(torch.from_numpy(a))
    wide = torch.full((P, 4), 1e30, device=DEV)
    wide[:, :3] = torch.from_numpy(a).to(DEV)
    assert P == 0 or (view.data_ptr() % 16 == 4 and view.is_contiguous() and (P == 1 or not wide[:, :3].is_contiguous()))
    return _dev(a), view, wide[:, :3]


# ---------------------------------------------------------------------------------------------------------------- build once, query many times
@pytest.mark.parametrize("name", sorted(chamfer_cases.NEAREST))
def test_nearest_grid_equals_nearest_points(name):
    from gsrast import chamfer
    q, t, m = chamfer_cases.NEAREST[name]
    dq, dt = _dev(q), _dev(t)
    want = chamfer.nearest_points(dq, dt, m)
    grid = chamfer.NearestGrid(dt, m)
    dt.fill_(7.0)                                         # the grid keeps its own copy of the targets
    first = grid.query(dq)
    other = grid.query(torch.flip(dq, [0]))               # a second query against the same build
    again = grid.query(dq)
    for got in (first, again, tuple(torch.flip(x, [0]) for x in other)):
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
        assert np.array_equal(got[1].cpu().numpy(), want[1].cpu().numpy()) and np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy()), name
    d2 = torch.full_like(first[0], -7.0); idx = torch.full_like(first[1], -9)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    grid.query(dq, skip=skip, out=(d2, idx))              # the word is set: every workgroup returns at once
    assert bool((d2 == -7.0).all()) and bool((idx == -9).all())
    skip.zero_()
    grid.query(dq, skip=skip, out=(d2, idx))
    assert torch.equal(d2, want[0]) and torch.equal(idx, want[1])


# ---------------------------------------------------------------------------------------------------------------- transform_points
@pytest.mark.parametrize("n", cases.SIZES)
def test_transform_points_sizes_and_layouts(n):
    from gsrast import register
    pts = cases.sheet(n, 3)
    for name, M in cases.TRANSFORMS.items():
        want = truth.transform(pts, M)
        for k, view in enumerate(_views(pts)):
            got = register.transform_points(view, torch.from_numpy(M))
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3) and got.is_contiguous()
            assert np.array_equal(got.cpu().numpy(), want), (name, n, k)
    assert np.array_equal(register.transform_points(_dev(pts), cases.MOTION.tolist()).cpu().numpy(), truth.transform(pts, cases.MOTION))      # a nested list is a matrix too


def test_transform_points_far_cloud_and_non_finite_rows():
    from gsrast import register
    far = cases.sheet(257, 4) + F(1e4)
    rows = np.concatenate([cases.NONFINITE_ROWS, far[:5]])
    for M in cases.TRANSFORMS.values():
        assert np.array_equal(register.transform_points(_dev(far), M).cpu().numpy(), truth.transform(far, M))
        got, want = register.transform_points(_dev(rows), M).cpu().numpy(), truth.transform(rows, M)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True) and np.isnan(want).any() and np.isinf(want).any()
    M = np.eye(4); M[0, 0] = 1 + 2.0 ** -30                                   # float64 inside: the float32 product would lose the 2^-6
    assert register.transform_points(_dev(cases.a3([[2.0 ** 24, 0, 0]])), M).cpu().numpy()[0, 0] == F(2.0 ** 24 + 2.0 ** -6)


def test_triangle_mesh_transform():
    from gsrast import register
    from gsrast.tsdf import TriangleMesh
    v = cases.sheet(65, 8)
    tri = np.random.default_rng(1).integers(0, 65, (40, 3)).astype(np.int32)
    col = np.random.default_rng(2).uniform(0, 1, (65, 3)).astype(F)
    mesh = TriangleMesh(_dev(v), _dev(col), _dev(tri), vertex_normals=_dev(col), triangle_normals=_dev(col[:40]))
    out = mesh.transform(cases.MOTION)
    assert torch.equal(out.vertices, register.transform_points(_dev(v), cases.MOTION)) and np.array_equal(out.vertices.cpu().numpy(), truth.transform(v, cases.MOTION))
    assert torch.equal(out.triangles, _dev(tri)) and torch.equal(out.vertex_colors, _dev(col)) and out.vertex_normals is None and out.triangle_normals is None
    assert torch.equal(mesh.vertices, _dev(v)) and mesh.vertex_normals is not None and mesh.triangle_normals is not None


# ---------------------------------------------------------------------------------------------------------------- correspondence_sums
def _sum_inputs(n, seed=0):
    """Clouds with positive coordinates (the rtol of the raw sums means something), T = 300 targets."""
    r = np.random.default_rng(seed + n)
    return r.uniform(1, 3, (n, 3)).astype(F), r.uniform(2, 5, (300, 3)).astype(F)


def _patterns(n, T, seed=0):
    r = np.random.default_rng(seed)
    one = np.full(n, -1, np.int32)
    if n:
        one[n // 2] = T - 1
    alt = np.where(np.arange(n) % 2 == 0, r.integers(0, T, n), -1).astype(np.int32)
    perm = (r.permutation(max(n, 1))[:n] % T).astype(np.int32)
    return {"none": np.full(n, -1, np.int32), "one": one, "alternating": alt, "permutation": perm}


def _check_sums(s, t, idx, label):
    from gsrast import register
    ds, dt, di = _dev(s), _dev(t), _dev(idx)
    record = register.correspondence_sums(ds, dt, di)
    assert torch.equal(record, register.correspondence_sums(ds, dt, di)), "two runs, the same bits"
    got = register.read_record(record)
    p, q, status = truth.pairs(s, t, idx)
    assert status == 0 and got["status"] == 0 and got["n"] == len(p), label
    assert np.array_equal(got["transformation"].numpy(), np.eye(4))
    if len(p) == 0:
        assert all(not got[k].numpy().any() for k in ("sum_p", "sum_q", "mean_p", "mean_q", "H")) and got["spp"] == 0.0 and got["sqq"] == 0.0
        return
    for key, cloud in (("sum_p", p), ("sum_q", q)):
        want = np.array([math.fsum(cloud[:, a].tolist()) for a in range(3)])
        rel = np.abs(got[key].numpy() - want) / want
        mean_rel = np.abs(got["mean_" + key[-1]].numpy() - want / len(p)) / (want / len(p))
        print(f"{label} {key}: rel {rel.max():.1e}, mean rel {mean_rel.max():.1e}")
        assert rel.max() <= 1e-12 and mean_rel.max() <= 1e-12, (label, key)
        assert np.array_equal(got["mean_" + key[-1]].numpy(), got[key].numpy() / float(len(p)))                  # one float64 division each
    H, spp, sqq, Habs = truth.centred(p, q, got["mean_p"].numpy(), got["mean_q"].numpy())                            # with the device's own means
    errs = (np.abs(got["H"].numpy() - H) / np.maximum(Habs, 1e-300)).max(), abs(got["spp"] - spp) / max(spp, 1e-300), abs(got["sqq"] - sqq) / max(sqq, 1e-300)
    print(f"{label} centred: H {errs[0]:.1e} spp {errs[1]:.1e} sqq {errs[2]:.1e} of the sum of |term|")
    assert (np.abs(got["H"].numpy() - H) <= 1e-12 * Habs).all() and abs(got["spp"] - spp) <= 1e-12 * spp and abs(got["sqq"] - sqq) <= 1e-12 * sqq, label


@pytest.mark.parametrize("n", cases.SUM_SIZES)
def test_correspondence_sums(n):
    s, t = _sum_inputs(n)
    for name, idx in _patterns(n, len(t)).items():
        _check_sums(s, t, idx, f"N={n} {name}")


def test_correspondence_sums_past_the_largest_grid_of_blocks():
    """One size past RG_BLOCKS * RG_PER_BLOCK elements, where the grid of blocks stops growing and a thread takes a fifth element."""
    n = cases.SUM_PAST_GRID
    s, t = _sum_inputs(n)
    _check_sums(s, t, _patterns(n, len(t))["alternating"], f"N={n} alternating")


def test_correspondence_sums_far_cloud_and_bad_index():
    from gsrast import register
    s, t = cases.OFFSET_1E4
    _check_sums(s, t, np.arange(len(s), dtype=np.int32), "offset 1e4")
    back = register.read_record(register.correspondence_sums(_dev(s - F(1e4)), _dev(t - F(1e4)), _dev(np.arange(len(s), dtype=np.int32))))
    far = register.read_record(register.correspondence_sums(_dev(s), _dev(t), _dev(np.arange(len(s), dtype=np.int32))))
    assert np.abs(far["H"].numpy() - back["H"].numpy()).max() < 1e-11           # the two passes keep the digits (one pass loses 1e-6: test_register_cpu)
    s, t = _sum_inputs(257)
    for bad in (len(t), -2, 1 << 30):
        idx = _patterns(257, len(t))["permutation"]; idx[100] = bad
        record = register.correspondence_sums(_dev(s), _dev(t), _dev(idx))
        assert int(record[register.R_STATUS].item()) & register.ERR_INDEX and int(record[register.R_N].item()) == 256
        with pytest.raises(RuntimeError, match="index"):
            register.read_record(record)
        with pytest.raises(RuntimeError, match="index"):
            register.solve_transform(record)
    ds, dt, di = _dev(s), _dev(t), _dev(_patterns(257, len(t))["permutation"])
    syncs, _ = count_syncs(lambda: register.correspondence_sums(ds, dt, di))
    assert syncs == 0, "the record stays on the device"


# ---------------------------------------------------------------------------------------------------------------- solve_transform
@pytest.mark.parametrize("name", sorted(cases.SOLVE))
def test_solve_transform(name):
    from gsrast import register
    s, t, scaling = cases.SOLVE[name]
    record = register.correspondence_sums(_dev(s), _dev(t), _dev(np.arange(len(s), dtype=np.int32)))
    got = register.solve_transform(record, with_scaling=scaling)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 4) and not got.is_cuda
    rec = register.read_record(record)                    # the device's own sums: the truth solves exactly what the device solved
    want, status = truth.solve({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}, scaling)
    assert rec["status"] == status and np.array_equal(rec["transformation"].numpy(), got.numpy())
    if name in cases.SOLVE_DEGENERATE:
        assert status == register.ERR_DEGENERATE and np.array_equal(got.numpy(), np.eye(4))
        with pytest.raises(RuntimeError, match="degenerate"):
            register.fit_transform(_dev(s), _dev(t), with_scaling=scaling)
        return
    M = got.numpy()
    print(f"{name}: {int((M != want).sum())} of 16 elements differ, largest {np.abs(M - want).max():.1e}")
    assert status == 0 and np.array_equal(M, want), name
    R = M[:3, :3] / (np.cbrt(np.linalg.det(M[:3, :3])) if scaling else 1.0)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0.999999      # a proper rotation: the reflection and the collinear case too
    assert np.array_equal(register.fit_transform(_dev(s), _dev(t), with_scaling=scaling).numpy(), M)
    if name == "half_turn":
        assert np.abs(M - np.diag([-1.0, -1, 1, 1])).max() < 1e-15
    if name in ("scale_half", "scale_three"):
        assert abs(np.cbrt(np.linalg.det(M[:3, :3])) - {"scale_half": 0.5, "scale_three": 3.0}[name]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- icp
def _check_icp(got, want, label):
    print(f"{label}: iterations {got.iterations}/{want['iterations']} converged {got.converged} status {got.status} inliers {got.n_inliers}/{want['n_inliers']} "
          f"rmse {got.inlier_rmse!r}/{want['inlier_rmse']!r} |dM| {np.abs(got.transformation.numpy() - want['transformation']).max():.2e}")
    assert (got.iterations, got.converged, got.status, got.n_inliers) == (want["iterations"], want["converged"], want["status"], want["n_inliers"]), label
    assert got.fitness == want["fitness"] and got.inlier_rmse == pytest.approx(want["inlier_rmse"], rel=1e-9, abs=0), label
    assert got.transformation.dtype == torch.float64 and tuple(got.transformation.shape) == (4, 4)
    assert np.abs(got.transformation.numpy() - want["transformation"]).max() <= cases.TRANSFORM_BAR, label


@pytest.mark.parametrize("name", sorted(cases.ICP))
def test_icp(name):
    from gsrast import register
    c = cases.ICP[name]
    want = cases.icp_truth(name)
    got = register.icp(_dev(c["source"]), _dev(c["target"]), c["cap"], **c["kw"])
    _check_icp(got, want, name)
    if want["status"]:                                    # stopped before any solve: the matrix is the init, bit for bit
        init = c["kw"].get("init")
        assert np.array_equal(got.transformation.numpy(), np.eye(4) if init is None else init)


def test_icp_with_init_evaluation_and_empty_target():
    from gsrast import register
    c = cases.ICP["exact_copy"]
    ds, dt = _dev(c["source"]), _dev(c["target"])
    init = cases.icp_truth("exact_copy")["transformation"]
    want = truth.icp(c["source"], c["target"], c["cap"], init=init, **c["kw"])
    assert want["iterations"] == 1 and want["converged"]
    _check_icp(register.icp(ds, dt, c["cap"], init=init, **c["kw"]), want, "with_init")
    zero = register.icp(ds, dt, c["cap"], max_iteration=0)
    ev = register.evaluate_registration(ds, dt, c["cap"], np.eye(4))
    _check_icp(ev, cases.icp_truth("max_iteration_0"), "evaluate_registration")
    assert (ev.fitness, ev.inlier_rmse, ev.n_inliers, ev.iterations, ev.converged, ev.status) == \
        (zero.fitness, zero.inlier_rmse, zero.n_inliers, zero.iterations, zero.converged, zero.status) and torch.equal(ev.transformation, zero.transformation)
    ev = register.evaluate_registration(ds, dt, c["cap"], init)
    assert ev.fitness == 1.0 and ev.inlier_rmse == pytest.approx(want["trace"][0][2], rel=1e-9) and np.array_equal(ev.transformation.numpy(), init)
    none = register.icp(ds, torch.empty((0, 3), device=DEV), 0.5)
    assert (none.fitness, none.n_inliers, none.inlier_rmse, none.iterations, none.converged, none.status) == (0.0, 0, 0.0, 0, False, register.ERR_DEGENERATE)
    a, b = register.icp(ds, dt, c["cap"], **c["kw"]), register.icp(ds, dt, c["cap"], **c["kw"])
    assert torch.equal(a.transformation, b.transformation) and a.inlier_rmse == b.inlier_rmse      # two runs, the same bits
    for k, view in enumerate(zip(_views(c["source"]), _views(c["target"]))):
        assert torch.equal(register.icp(view[0], view[1], c["cap"], **c["kw"]).transformation, a.transformation), k


# ---------------------------------------------------------------------------------------------------------------- synchronisations
def test_host_synchronisations():
    from gsrast import chamfer, register
    c = cases.ICP["exact_copy"]
    ds, dt = _dev(c["source"]), _dev(c["target"])
    for max_iteration in (3, 30):
        syncs, r = count_syncs(lambda: register.icp(ds, dt, c["cap"], max_iteration=max_iteration, **c["kw"]))
        assert syncs == 1 and r.iterations == min(max_iteration, 10), f"one host read, whatever max_iteration ({max_iteration})"
    syncs, _ = count_syncs(lambda: register.transform_points(ds, cases.MOTION))
    assert syncs == 0
    syncs, grid = count_syncs(lambda: chamfer.NearestGrid(dt, 0.15))
    assert syncs == 0
    syncs, _ = count_syncs(lambda: grid.query(ds))
    assert syncs == 0
    syncs, _ = count_syncs(lambda: register.crop_polygon_volume(ds, cases.POLYGONS["K1024"], "Z", -0.1, 0.1))
    assert syncs == 0
    syncs, _ = count_syncs(lambda: register.fit_transform(ds, dt))
    assert syncs == 1


# ---------------------------------------------------------------------------------------------------------------- crop_polygon_volume
@pytest.mark.parametrize("name", sorted(cases.POLYGONS))
def test_crop_polygon_volume(name):
    from gsrast import register
    poly = cases.POLYGONS[name]
    lo, hi = -0.5, 0.25
    for axis in "XYZ":
        pts = cases.crop_points(poly, axis, lo, hi)
        want = truth.crop(pts, poly, axis, lo, hi)
        got = register.crop_polygon_volume(_dev(pts), poly, axis, lo, hi)
        assert got.dtype == torch.bool and tuple(got.shape) == (257,) and got.is_cuda
        print(f"{name} {axis}: {int(want.sum())} of 257 kept, {int((got.cpu().numpy() != want).sum())} differ")
        assert np.array_equal(got.cpu().numpy(), want) and want.any() and not want.all(), (name, axis)
        ax = "XYZ".index(axis)
        three = np.insert(poly, ax, 123.0, axis=1)        # the [K,3] form of the crop file: the coordinate along the axis is ignored
        assert torch.equal(register.crop_polygon_volume(_dev(pts), three.tolist(), axis.lower(), lo, hi), got)
        for n in (0, 1):
            small = register.crop_polygon_volume(_dev(pts[250:250 + n]), torch.from_numpy(poly), axis, lo, hi)
            assert np.array_equal(small.cpu().numpy(), want[250:250 + n]) and small.dtype == torch.bool
    views = _views(cases.crop_points(poly, "Z", lo, hi))
    assert all(torch.equal(register.crop_polygon_volume(v, poly, "Z", lo, hi), register.crop_polygon_volume(views[0], poly, "Z", lo, hi)) for v in views[1:])
