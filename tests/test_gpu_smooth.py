"""GPU tests (pytest -m gpu) of gsrast.mesh.vertex_adjacency, compute_triangle_normals / compute_vertex_normals and filter_smooth_simple /
_laplacian / _taubin (gsr_mesh_adjacency_*, gsr_mesh_normals, gsr_mesh_smooth of the C ABI, csrc/gsr_mesh_smooth.hip) against the restatement
of tests/smooth_truth.py on the named inputs of tests/smooth_cases.py.

The adjacency is integer and compared with np.array_equal.  The simple filter uses only float64 + and /, which are exact operations without FMA
contraction: bit-equal.  The normals, the Laplacian and the Taubin filter pass through a float64 sqrt, and whether the device's sqrt is correctly
rounded has not been established: bit equality is the expectation, every test prints how many components are not bit-equal, and the bar asserted per
component is one float32 ulp of M (the largest absolute coordinate among input and truth output) for positions and 2^-23 for normals and colours.
Why that bar: degree <= 64 with <= 10 iterations, or degree <= 5000 with <= 2, means a few hundred to a few thousand float64 roundings per step,
each <= a few 2^-53 relative; the mu step amplifies at most 2.06 x per iteration; the state error stays below 2^-30 M, far under half a float32 ulp of
M, so the two final roundings differ by at most one such ulp.

Observed on an MI355X: every count printed below is 0 -- all outputs are bit-equal to the truth."""
import numpy as np
import pytest
import torch

import smooth_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORMAL_BAR = 2.0 ** -23


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mesh(v, c, t):
    from gsrast.tsdf import TriangleMesh
    return TriangleMesh(_dev(v), _dev(c), _dev(t))


def _case(name):
    return _mesh(*cases.CASES[name])


def _bits_differ(got, want):
    return int((got.view(np.int32) != want.view(np.int32)).sum()) if got.size else 0


def _ulp_of(m):
    """One float32 ulp of the magnitude m."""
    return float(np.spacing(np.float32(m))) if m > 0 else float(np.spacing(np.float32(0)))


def _smooth(mesh, kind, n, scope):
    import gsrast
    f = {"simple": lambda: gsrast.filter_smooth_simple(mesh, n, scope),
         "laplacian": lambda: gsrast.filter_smooth_laplacian(mesh, n, cases.LAMBDA, scope),
         "taubin": lambda: gsrast.filter_smooth_taubin(mesh, n, cases.LAMBDA, cases.MU, scope)}[kind]
    out = f()
    assert out.vertices.dtype == out.vertex_colors.dtype == torch.float32 and out.triangles.dtype == torch.int32
    return out.vertices.cpu().numpy(), out.vertex_colors.cpu().numpy(), out


@pytest.mark.parametrize("name", cases.NAMES)
def test_vertex_adjacency_against_the_truth(name):
    import gsrast
    start, nb = gsrast.vertex_adjacency(_case(name))
    want_start, want_nb = cases.truth_adjacency(name)
    assert start.dtype == nb.dtype == torch.int32 and start.is_cuda and nb.is_cuda
    assert np.array_equal(start.cpu().numpy(), want_start) and np.array_equal(nb.cpu().numpy(), want_nb)


@pytest.mark.parametrize("scope", cases.SCOPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_filter_smooth_simple_is_bit_equal_to_the_truth(name, scope):
    v, c, t = cases.CASES[name]
    mesh = _mesh(v, c, t)
    for n in cases.iterations(name):
        gv, gc, out = _smooth(mesh, "simple", n, scope)
        wv, wc = cases.truth_smooth(name, "simple", n, scope)
        print(f"{name} simple {scope} x{n}: {_bits_differ(gv, wv)} position and {_bits_differ(gc, wc)} colour components not bit-equal")
        assert gv.shape == wv.shape and gv.tobytes() == wv.tobytes(), (name, n)
        assert gc.shape == wc.shape and gc.tobytes() == wc.tobytes(), (name, n)
        assert out.triangles.cpu().numpy().tobytes() == t.tobytes() and out.triangles is not mesh.triangles
        assert not t.size or out.triangles.data_ptr() != mesh.triangles.data_ptr()
        if scope == "vertex":
            assert gc.tobytes() == c.tobytes()


@pytest.mark.parametrize("scope", cases.SCOPES)
@pytest.mark.parametrize("kind", ["laplacian", "taubin"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_laplacian_and_taubin_against_the_truth(name, kind, scope):
    v, c, t = cases.CASES[name]
    mesh = _mesh(v, c, t)
    for n in cases.iterations(name):
        gv, gc, out = _smooth(mesh, kind, n, scope)
        wv, wc = cases.truth_smooth(name, kind, n, scope)
        M = max(float(np.abs(v).max()) if v.size else 0.0, float(np.abs(wv).max()) if wv.size else 0.0)
        print(f"{name} {kind} {scope} x{n}: {_bits_differ(gv, wv)} position and {_bits_differ(gc, wc)} colour components not bit-equal")
        assert gv.shape == wv.shape and gc.shape == wc.shape
        if gv.size:
            assert np.abs(gv.astype(np.float64) - wv.astype(np.float64)).max() <= _ulp_of(M), (name, kind, n)
            assert np.abs(gc.astype(np.float64) - wc.astype(np.float64)).max() <= NORMAL_BAR, (name, kind, n)
        if scope == "vertex":
            assert gc.tobytes() == c.tobytes()
        assert out.triangles.cpu().numpy().tobytes() == t.tobytes()
        assert out.vertex_normals is None and out.triangle_normals is None


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("name", cases.NAMES)
def test_normals_against_the_truth(name, normalized):
    import gsrast
    mesh = _case(name)
    for which, f in (("triangle", gsrast.compute_triangle_normals), ("vertex", gsrast.compute_vertex_normals)):
        got = f(mesh, normalized=normalized)
        want = cases.truth_normals(name, which, normalized)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
        g = got.cpu().numpy()
        print(f"{name} {which} normals normalized={normalized}: {_bits_differ(g, want)} components not bit-equal")
        if normalized:
            if g.size:
                assert np.abs(g.astype(np.float64) - want.astype(np.float64)).max() <= NORMAL_BAR, (name, which)
        else:                                             # the unnormalised normal is products and sums alone: exact operations
            assert g.tobytes() == want.tobytes(), (name, which)


def test_fallback_normals():
    import gsrast
    n = gsrast.compute_vertex_normals(_case("cancelling")).cpu().numpy()
    assert (n == np.array([0, 0, 1], np.float32)).all()
    v, _, t = cases.CASES["isolated"]
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    mesh = _case("isolated")
    assert (gsrast.compute_vertex_normals(mesh).cpu().numpy()[~used] == np.array([0, 0, 1], np.float32)).all()
    assert (gsrast.compute_vertex_normals(mesh, normalized=False).cpu().numpy()[~used] == 0).all()
    tn = gsrast.compute_triangle_normals(_case("degenerate")).cpu().numpy()
    assert (tn[:3] == np.array([0, 0, 1], np.float32)).all() and (tn[5] == np.array([0, 0, 1], np.float32)).all()


@pytest.mark.parametrize("name", ["torus_noisy", "size_V1025", "fan_1025_closed"])
def test_a_second_run_gives_identical_bits_and_the_input_is_unchanged(name):
    import gsrast
    v, c, t = cases.CASES[name]
    mesh = _mesh(v, c, t)
    n = cases.iterations(name)[1]

    def run():
        out = [x.cpu().numpy().tobytes() for x in gsrast.vertex_adjacency(mesh)]
        out += [gsrast.compute_vertex_normals(mesh).cpu().numpy().tobytes(), gsrast.compute_triangle_normals(mesh).cpu().numpy().tobytes()]
        for kind in cases.FILTERS:
            gv, gc, _ = _smooth(mesh, kind, n, "all")
            out += [gv.tobytes(), gc.tobytes()]
        return out
    assert run() == run()
    assert mesh.vertices.cpu().numpy().tobytes() == v.tobytes() and mesh.vertex_colors.cpu().numpy().tobytes() == c.tobytes()
    assert mesh.triangles.cpu().numpy().tobytes() == t.tobytes()


@pytest.mark.parametrize("kind", cases.FILTERS)
def test_zero_iterations_return_the_inputs_bits_in_new_tensors(kind):
    v, c, t = cases.CASES["far_from_origin"]
    mesh = _mesh(v, c, t)
    for scope in cases.SCOPES:
        gv, gc, out = _smooth(mesh, kind, 0, scope)
        assert gv.tobytes() == v.tobytes() and gc.tobytes() == c.tobytes() and out.triangles.cpu().numpy().tobytes() == t.tobytes()
        assert out is not mesh and out.vertices.data_ptr() != mesh.vertices.data_ptr() and out.vertex_colors.data_ptr() != mesh.vertex_colors.data_ptr()
        assert out.triangles.data_ptr() != mesh.triangles.data_ptr()


def _views(a):
    """The three layouts of test_gpu_simplify._views: packed, a view one element into its storage, the first three columns of [P,4]."""
    P, dt = a.shape[0], torch.from_numpy(a).dtype
    buf = torch.empty(3 * P + 1, device=DEV, dtype=dt)
    view = buf[1:].view(P, 3)
    view.copy_(torch.from_numpy(a))
    wide = torch.full((P, 4), 7, device=DEV, dtype=dt)
    wide[:, :3] = torch.from_numpy(a).to(DEV)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and not wide[:, :3].is_contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV), view, wide[:, :3]


@pytest.mark.parametrize("name", ["size_V257", "cube"])
def test_input_layout(name):
    import gsrast
    v, c, t = cases.CASES[name]
    base = None
    for vv, cc, tt in zip(_views(v), _views(c), _views(t)):
        mesh = _mesh(vv, cc, tt)
        got = [x.cpu().numpy().tobytes() for x in gsrast.vertex_adjacency(mesh)]
        got += [gsrast.compute_vertex_normals(mesh).cpu().numpy().tobytes(), gsrast.compute_triangle_normals(mesh, False).cpu().numpy().tobytes()]
        for kind in cases.FILTERS:
            gv, gc, _ = _smooth(mesh, kind, 3, "all")
            got += [gv.tobytes(), gc.tobytes()]
        base = base or got
        assert got == base
        assert vv.cpu().numpy().tobytes() == v.tobytes() and tt.cpu().numpy().tobytes() == t.tobytes()


def test_the_methods_and_the_functions_agree():
    import gsrast
    mesh = _case("sphere")
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert mesh.vertex_normals is None and not mesh.has_vertex_normals() and not mesh.has_triangle_normals()
    assert mesh.compute_vertex_normals() is mesh and mesh.compute_triangle_normals() is mesh
    assert mesh.has_vertex_normals() and mesh.has_triangle_normals()
    assert same(mesh.vertex_normals, gsrast.compute_vertex_normals(mesh)) and same(mesh.triangle_normals, gsrast.compute_triangle_normals(mesh))
    assert same(mesh.compute_vertex_normals(normalized=False).vertex_normals, gsrast.mesh.compute_vertex_normals(mesh, False))
    pairs = ((mesh.filter_smooth_simple(3, "vertex"), gsrast.filter_smooth_simple(mesh, number_of_iterations=3, filter_scope="vertex")),
             (mesh.filter_smooth_laplacian(2, 0.4), gsrast.filter_smooth_laplacian(mesh, 2, lambda_filter=0.4)),
             (mesh.filter_smooth_taubin(2, 0.5, -0.53, "all"), gsrast.filter_smooth_taubin(mesh, 2)))
    for a, b in pairs:
        assert a is not mesh and b is not mesh and isinstance(a, type(mesh)) and isinstance(b, type(mesh))
        assert same(a.vertices, b.vertices) and same(a.vertex_colors, b.vertex_colors) and same(a.triangles, mesh.triangles)
        assert a.vertex_normals is None and a.triangle_normals is None and not same(a.vertices, mesh.vertices)
    assert mesh.has_vertex_normals()                      # the filters left the input alone
    assert mesh.remove_degenerate_triangles() is mesh and mesh.vertex_normals is None and mesh.triangle_normals is None      # an in-place filter drops them


def _syncs(f):
    import warnings
    f()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            f()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower())


def test_one_host_synchronisation_per_call():
    """Counted the way test_gpu_simplify.py counts them; the same for 1 and 10 iterations."""
    import gsrast
    mesh = _case("torus_noisy")
    assert _syncs(lambda: gsrast.vertex_adjacency(mesh)) == 1
    assert _syncs(lambda: gsrast.compute_vertex_normals(mesh)) == 1 and _syncs(lambda: gsrast.compute_triangle_normals(mesh)) == 1
    for scope in cases.SCOPES:
        for f in (gsrast.filter_smooth_simple, gsrast.filter_smooth_laplacian, gsrast.filter_smooth_taubin):
            one, ten = _syncs(lambda: f(mesh, number_of_iterations=1, filter_scope=scope)), _syncs(lambda: f(mesh, number_of_iterations=10, filter_scope=scope))
            assert one == ten == 1, (f.__name__, scope, one, ten)


def test_the_pipeline_runs_end_to_end(tmp_path):
    import gsrast
    from gsrast import ply
    mesh = _case("torus_noisy")
    post = gsrast.post_process_mesh(mesh, cluster_to_keep=1)
    small = gsrast.simplify_vertex_clustering(post, 0.12)
    smooth = gsrast.filter_smooth_taubin(small, 5)
    assert smooth.vertex_normals is None
    smooth.compute_vertex_normals()
    path = str(tmp_path / "fuse_post.ply")
    ply.write_triangle_mesh(path, smooth)
    back = ply.read_triangle_mesh(path, device=DEV)
    assert back.has_vertex_normals() and back.vertex_normals.cpu().numpy().tobytes() == smooth.vertex_normals.cpu().numpy().tobytes()
    assert back.vertices.cpu().numpy().tobytes() == smooth.vertices.cpu().numpy().tobytes()
    assert back.triangles.cpu().numpy().tobytes() == smooth.triangles.cpu().numpy().tobytes()
    n = back.vertex_normals.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    clusters, counts, _ = gsrast.cluster_connected_triangles(back, with_area=False)
    assert clusters.shape[0] == back.triangles.shape[0] > 0 and counts.numel() >= 1 and int(counts.sum()) == back.triangles.shape[0]
    assert 0 < small.vertices.shape[0] < mesh.vertices.shape[0]


def test_status_words_raise_the_documented_errors():
    """Input checks: every kernel treats such a value as data (a key, a refused index), nothing is dereferenced through it."""
    import gsrast
    match = {"nonfinite": "non-finite", "index": r"outside \[0, number of vertices\)"}
    filters = (gsrast.filter_smooth_simple, gsrast.filter_smooth_laplacian, gsrast.filter_smooth_taubin)
    for name, (v, c, t, kind) in cases.errors().items():
        mesh = _mesh(v, c, t)
        for f in filters:
            for scope in cases.SCOPES:
                with pytest.raises(RuntimeError, match=match[kind]):
                    f(mesh, 2, filter_scope=scope)
        if kind == "index":
            for f in (gsrast.vertex_adjacency, gsrast.compute_triangle_normals, gsrast.compute_vertex_normals):
                with pytest.raises(RuntimeError, match=match[kind]):
                    f(mesh)
    host = _case("alone").cpu()
    for f in filters + (gsrast.vertex_adjacency, gsrast.compute_triangle_normals, gsrast.compute_vertex_normals):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f(host)
    empty_v = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match=match["index"]):                                  # triangles without vertices: every index is out of range
        gsrast.vertex_adjacency(_mesh(empty_v, empty_v, cases.CASES["alone"][2]))
