"""GPU tests (pytest -m gpu) of gsrast.rasterize_mesh, triangle_view_counts and cull_unseen_triangles (gsr_mesh_rasterize of the C ABI,
csrc/gsr_mesh_raster.hip) against the restatement of tests/raster_truth.py on the named inputs of tests/raster_cases.py.

triangle_id, dropped and counts are integers and compared with np.array_equal.  depth and barycentric are compared as BYTES: the path is + - x /
and rint in float64 on widened float32 inputs and one rounding to float32, all IEEE operations without FMA contraction -- the ground on which
test_gpu_smooth.test_filter_smooth_simple_is_bit_equal_to_the_truth already asserts bytes on this device.  Every comparison prints the number of
components that are not bit-equal first.

Observed on an MI355X: every count printed is 0 -- all maps of all 23 named cases are bit-equal to the truth."""
import numpy as np
import pytest
import torch

import raster_cases as cases
import raster_truth as truth
from test_gpu_smooth import _syncs, _views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_I32 = 2 ** 31 - 1


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(DEV)        # a copy: the cases are read-only


def _mesh(k):
    from gsrast.tsdf import TriangleMesh
    return TriangleMesh(_dev(k["v"]), _dev(k["c"]), _dev(k["t"]))


def _raster(k, mesh=None, mats=None, **kw):
    import gsrast
    return gsrast.rasterize_mesh(mesh or _mesh(k), _dev(k["mats"] if mats is None else mats), k["W"], k["H"], near=k["near"], cull_sign=k["cull_sign"], **kw)


def _counts(k, tol=None, mesh=None, **kw):
    import gsrast
    return gsrast.triangle_view_counts(mesh or _mesh(k), _dev(k["mats"]), k["W"], k["H"], near=k["near"], cull_sign=k["cull_sign"], depth_tolerance=tol, **kw)


def _bytes(r):
    return [x.cpu().numpy().tobytes() for x in (r.depth, r.triangle_id, r.barycentric, r.dropped)]


def _bits_differ(got, want):
    return int((got.view(np.int32) != want.view(np.int32)).sum()) if got.size else 0


@pytest.mark.parametrize("name", cases.NAMES)
def test_against_the_truth(name):
    k = cases.CASES[name]
    r = _raster(k)
    depth, tid, bary, dropped = cases.truth_maps(name)
    n = len(k["mats"])
    assert r.depth.dtype == r.barycentric.dtype == torch.float32 and r.triangle_id.dtype == r.dropped.dtype == torch.int32
    assert all(x.is_cuda for x in (r.depth, r.triangle_id, r.barycentric, r.dropped))
    assert tuple(r.depth.shape) == tuple(r.triangle_id.shape) == (n, k["H"], k["W"]) and tuple(r.barycentric.shape) == (n, k["H"], k["W"], 2)
    assert tuple(r.dropped.shape) == (n, 3)
    gd, gb = r.depth.cpu().numpy(), r.barycentric.cpu().numpy()
    print(f"{name}: {_bits_differ(gd, depth)} depth and {_bits_differ(gb, bary)} barycentric components not bit-equal, "
          f"{int((r.triangle_id.cpu().numpy() != tid).sum())} ids differ")
    assert np.array_equal(r.triangle_id.cpu().numpy(), tid)
    assert np.array_equal(r.dropped.cpu().numpy(), dropped)
    assert gd.tobytes() == depth.tobytes()
    assert gb.tobytes() == bary.tobytes()
    for tol in (None, cases.TOLERANCE):
        c = _counts(k, tol)
        assert c.dtype == torch.int32 and c.is_cuda and tuple(c.shape) == (len(k["t"]),)
        assert np.array_equal(c.cpu().numpy(), cases.truth_counts(name, tol)), tol
    assert _raster(k, want_barycentric=False).barycentric is None


@pytest.mark.parametrize("name", cases.SPHERES + ("whole_image",))
def test_both_paths_give_the_same_bytes(name):
    k = cases.CASES[name]
    _, t, b = cases.named_triangle(name)
    assert b >= 2 and cases.truth_views(name)[0]["box"][t] == b
    mesh = _mesh(k)
    base = _bytes(_raster(k, mesh))
    depth, tid, _, _ = cases.truth_maps(name)
    assert base[0] == depth.tobytes() and base[1] == tid.tobytes()
    for large_from in (0, b - 1, b, MAX_I32):
        assert _bytes(_raster(k, mesh, _large_from=large_from)) == base, large_from
        for tol in (None, cases.TOLERANCE):
            assert np.array_equal(_counts(k, tol, mesh, _large_from=large_from).cpu().numpy(), cases.truth_counts(name, tol)), (large_from, tol)


def test_eight_views_equal_eight_calls_and_a_second_run_gives_the_same_bytes():
    k = cases.CASES["sphere_33x31"]
    assert len(k["mats"]) == 8
    mesh = _mesh(k)
    whole = _raster(k, mesh)
    assert _bytes(_raster(k, mesh)) == _bytes(whole)
    assert _counts(k, cases.TOLERANCE, mesh).cpu().numpy().tobytes() == _counts(k, cases.TOLERANCE, mesh).cpu().numpy().tobytes()
    for i in range(8):
        one = _raster(k, mesh, mats=k["mats"][i])                                            # a single [4,4] matrix is one view
        assert tuple(one.depth.shape) == (1, k["H"], k["W"])
        for a, b in zip((one.depth, one.triangle_id, one.barycentric, one.dropped), (whole.depth, whole.triangle_id, whole.barycentric, whole.dropped)):
            assert a[0].cpu().numpy().tobytes() == b[i].cpu().numpy().tobytes(), i
    assert mesh.vertices.cpu().numpy().tobytes() == k["v"].tobytes() and mesh.triangles.cpu().numpy().tobytes() == k["t"].tobytes()
    assert mesh.vertex_colors.cpu().numpy().tobytes() == k["c"].tobytes()


def test_1030_views_equal_the_calls_on_the_first_1024_and_the_last_6():
    """More views than a chunk takes (test_raster_cpu holds the rule): the second turn offsets the matrices, the maps and `dropped` by 1024 views,
    clears the key buffer, the lists and the owner bytes again and adds its views to the counts.  test_against_the_truth holds the case's maps,
    `dropped` and counts to the truth; here the whole call against the two calls either side of the chunk edge, the cull, and a second run."""
    import gsrast
    name = "box_1030_views"
    k = cases.CASES[name]
    cut, n = cases.CHUNK_MAX, len(k["mats"])
    assert n == 1030 > cut == 1024
    mesh = _mesh(k)
    whole = _raster(k, mesh)
    assert whole.triangle_id.cpu().numpy()[cut:].tobytes() == cases.truth_maps(name)[1][cut:].tobytes() and int((whole.triangle_id[cut:] >= 0).sum()) > 6 * 20
    first, last = _raster(k, mesh, mats=k["mats"][:cut]), _raster(k, mesh, mats=k["mats"][cut:])
    assert tuple(last.depth.shape) == (n - cut, k["H"], k["W"])
    for a, b, c in zip(_bytes(whole), _bytes(first), _bytes(last)):
        assert a == b + c
    assert _bytes(_raster(k, mesh)) == _bytes(whole)
    for tol in (None, cases.TOLERANCE):
        counts = _counts(k, tol, mesh).cpu().numpy()
        parts = [gsrast.triangle_view_counts(mesh, _dev(m), k["W"], k["H"], near=k["near"], cull_sign=k["cull_sign"], depth_tolerance=tol).cpu().numpy()
                 for m in (k["mats"][:cut], k["mats"][cut:])]
        assert parts[1].max() > 0 and counts.tobytes() == (parts[0] + parts[1]).tobytes() and np.array_equal(counts, cases.truth_counts(name, tol)), tol
        assert _counts(k, tol, mesh).cpu().numpy().tobytes() == counts.tobytes()
    want_counts = cases.truth_counts(name, cases.TOLERANCE)
    out, counts = gsrast.cull_unseen_triangles(mesh, _dev(k["mats"]), k["W"], k["H"], min_views=1000, depth_tolerance=cases.TOLERANCE, near=k["near"], return_counts=True)
    v, c, t = truth.cull(k["v"], k["c"], k["t"], want_counts, 1000)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and 0 < len(t) < len(k["t"])
    assert np.array_equal(out.triangles.cpu().numpy(), t) and out.vertices.cpu().numpy().tobytes() == v.tobytes() and out.vertex_colors.cpu().numpy().tobytes() == c.tobytes()


def test_input_layout():
    from gsrast.tsdf import TriangleMesh
    k = cases.CASES["sphere_64x48"]
    base = None
    for vv, cc, tt in zip(_views(k["v"]), _views(k["c"]), _views(k["t"])):
        mesh = TriangleMesh(vv, cc, tt)
        got = _bytes(_raster(k, mesh)) + [_counts(k, cases.TOLERANCE, mesh).cpu().numpy().tobytes()]
        base = base or got
        assert got == base
        assert vv.cpu().numpy().tobytes() == k["v"].tobytes() and tt.cpu().numpy().tobytes() == k["t"].tobytes()
    assert base[1] == cases.truth_maps("sphere_64x48")[1].tobytes()


def test_visibility_of_the_fine_sphere():
    k = cases.CASES["sphere_128x96"]
    plain, tol = _counts(k).cpu().numpy(), _counts(k, cases.TOLERANCE).cpu().numpy()
    assert np.array_equal(plain, cases.truth_counts("sphere_128x96")) and np.array_equal(tol, cases.truth_counts("sphere_128x96", cases.TOLERANCE))
    ids = _raster(k).triangle_id.cpu().numpy()
    owners = np.zeros(len(k["t"]), bool)
    owners[ids[ids >= 0]] = True
    assert ((~owners) & (tol > 0)).sum() > 1000            # they own no pixel in any view and are seen by the vertex test
    assert np.array_equal(plain > 0, owners) and (tol >= plain).all() and (tol == 0).sum() > 0


@pytest.mark.parametrize("min_views", [1, 2])
@pytest.mark.parametrize("tol", [None, cases.TOLERANCE])
def test_cull_unseen_triangles_against_the_truth(min_views, tol):
    import gsrast
    k = cases.CASES["sphere_33x31"]
    mesh = _mesh(k)
    out, counts = gsrast.cull_unseen_triangles(mesh, _dev(k["mats"]), k["W"], k["H"], min_views=min_views, depth_tolerance=tol, near=k["near"], return_counts=True)
    want_counts = cases.truth_counts("sphere_33x31", tol)
    v, c, t = truth.cull(k["v"], k["c"], k["t"], want_counts, min_views)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and 0 < len(t) == (want_counts >= min_views).sum()
    assert tol is not None or len(t) < len(k["t"])         # without the vertex test some triangles own no pixel in any of the eight views
    assert out.triangles.dtype == torch.int32 and np.array_equal(out.triangles.cpu().numpy(), t)
    assert out.vertices.cpu().numpy().tobytes() == v.tobytes() and out.vertex_colors.cpu().numpy().tobytes() == c.tobytes()
    assert out is not mesh and out.vertex_normals is None and out.triangle_normals is None
    assert out.vertices.data_ptr() != mesh.vertices.data_ptr() and out.triangles.data_ptr() != mesh.triangles.data_ptr()
    assert mesh.vertices.cpu().numpy().tobytes() == k["v"].tobytes() and mesh.triangles.cpu().numpy().tobytes() == k["t"].tobytes()
    assert mesh.vertex_colors.cpu().numpy().tobytes() == k["c"].tobytes()


def test_the_methods_and_the_functions_agree_and_interpolate_reproduces_the_depth():
    import gsrast
    k = cases.CASES["sphere_64x48"]
    mesh, M = _mesh(k), _dev(k["mats"])
    r = mesh.rasterize(M, k["W"], k["H"], near=k["near"])
    assert isinstance(r, gsrast.MeshRaster) and _bytes(r) == _bytes(gsrast.rasterize_mesh(mesh, M, k["W"], k["H"], near=k["near"]))
    assert mesh.rasterize(M, k["W"], k["H"], 0.01, 0, False).barycentric is None
    a = mesh.cull_unseen_triangles(M, k["W"], k["H"], 2, cases.TOLERANCE)
    b = gsrast.cull_unseen_triangles(mesh, M, k["W"], k["H"], min_views=2, depth_tolerance=cases.TOLERANCE)
    assert isinstance(a, type(mesh)) and a is not mesh
    for x, y in ((a.vertices, b.vertices), (a.vertex_colors, b.vertex_colors), (a.triangles, b.triangles)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # the interpolated positions are points whose own w is the depth
    p = r.interpolate(mesh.triangles, mesh.vertices)
    assert tuple(p.shape) == (len(k["mats"]), k["H"], k["W"], 3) and p.dtype == torch.float32
    hit = (r.triangle_id >= 0).cpu().numpy()
    assert (p.cpu().numpy()[~hit] == 0).all() and hit.sum() > 1000
    for i, Mi in enumerate(k["mats"]):
        q = p[i].cpu().numpy().astype(np.float64).reshape(-1, 3)
        w = (q @ Mi.astype(np.float64)[:3, 3] + float(Mi[3, 3])).reshape(k["H"], k["W"])
        d = r.depth[i].cpu().numpy().astype(np.float64)
        assert np.abs(w - d)[hit[i]].max() <= 1e-5 * d[hit[i]].max(), i


def test_one_host_synchronisation_per_call():
    """Counted the way test_gpu_smooth counts them: the same for 1 view and for 8, at 33 x 31 and at 128 x 96."""
    import gsrast
    for name in ("sphere_33x31", "sphere_128x96"):
        k = cases.CASES[name]
        mesh = _mesh(k)
        eight = _dev(np.concatenate([k["mats"]] * 3)[:8])
        for M in (eight[:1].contiguous(), eight):
            assert _syncs(lambda: gsrast.rasterize_mesh(mesh, M, k["W"], k["H"])) == 1, (name, len(M))
            assert _syncs(lambda: gsrast.triangle_view_counts(mesh, M, k["W"], k["H"], depth_tolerance=cases.TOLERANCE)) == 1, (name, len(M))
            assert _syncs(lambda: gsrast.cull_unseen_triangles(mesh, M, k["W"], k["H"])) == 2, (name, len(M))


def test_status_words_raise_the_documented_errors():
    """Input checks: a refused index is never dereferenced, a non-finite coordinate is data that fails the near or the guard test."""
    import gsrast
    match = {"nonfinite": "non-finite", "index": r"outside \[0, number of vertices\)"}
    for name, (k, kind) in cases.errors().items():
        mesh, M = _mesh(k), _dev(k["mats"])
        for f in (gsrast.rasterize_mesh, gsrast.triangle_view_counts, gsrast.cull_unseen_triangles):
            with pytest.raises(RuntimeError, match=match[kind]):
                f(mesh, M, k["W"], k["H"])
        with pytest.raises(RuntimeError, match=match[kind]):                                  # whatever the number of views
            gsrast.rasterize_mesh(mesh, M[:0], k["W"], k["H"])
    k = cases.CASES["whole_image"]
    host = _mesh(k).cpu()
    for f in (gsrast.rasterize_mesh, gsrast.triangle_view_counts, gsrast.cull_unseen_triangles):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f(host, _dev(k["mats"]), 32, 32)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f(_mesh(k), torch.from_numpy(k["mats"]), 32, 32)
        with pytest.raises(RuntimeError, match=r"shape \[4, 4\]"):
            f(_mesh(k), _dev(k["mats"])[:, :3], 32, 32)
        with pytest.raises(RuntimeError, match="torch.float32"):
            f(_mesh(k), _dev(k["mats"]).double(), 32, 32)


def test_culling_takes_the_inner_sphere_out_and_improves_the_accuracy():
    import gsrast
    k = cases.nested_spheres()
    mesh, M = _mesh(k), _dev(k["mats"])
    outer = _mesh(dict(k, t=k["t"][:1024]))
    gt = gsrast.sample_surface(outer, 0.05)
    before = gsrast.surface_distance(gsrast.post_process_mesh(mesh, cluster_to_keep=2), gt, spacing=0.05)
    culled, counts = gsrast.cull_unseen_triangles(mesh, M, k["W"], k["H"], depth_tolerance=0.02, return_counts=True)
    counts = counts.cpu().numpy()
    assert (counts[1024:] == 0).all() and (counts[:1024] > 0).all()                          # no camera sees the inner sphere, every outer triangle is seen
    assert culled.triangles.shape[0] == 1024 and int(culled.triangles.max()) < culled.vertices.shape[0] == len(k["v"]) // 2
    assert np.array_equal(culled.triangles.cpu().numpy(), k["t"][:1024])
    after = gsrast.surface_distance(gsrast.post_process_mesh(culled, cluster_to_keep=1), gt, spacing=0.05)
    print(f"accuracy before {before['accuracy']:.4g}, after {after['accuracy']:.4g}")
    assert after["accuracy"] < before["accuracy"] and after["accuracy"] < 1e-3 < before["accuracy"]
