"""GPU tests (pytest -m gpu) of gsrast.mesh.simplify_vertex_clustering (gsr_mesh_simplify_* of the C ABI, csrc/gsr_mesh_simplify.hip) against the
restatement of tests/simplify_truth.py on the named inputs of tests/simplify_cases.py.  Both sides evaluate the same float64 operations in the same
order with FMA contraction off, so vertices, colours, triangles, vertex_map and the record's counts are compared with np.array_equal."""
import numpy as np
import pytest
import torch

import simplify_cases as cases
import simplify_truth as truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("average", "quadric")


def _mesh(v, c, t):
    from gsrast.tsdf import TriangleMesh
    d = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return TriangleMesh(d(v), d(c), d(t))


def _run(mesh, vs, mode):
    """-> dict like the truth's, through the one-read-back path that also hands out the record."""
    from gsrast import mesh as M
    nv, nc, tris, vmap, rec = M._simplify(mesh, vs, mode, True)
    assert nv.dtype == nc.dtype == torch.float32 and tris.dtype == vmap.dtype == torch.int32
    assert nv.shape == nc.shape == (rec[1], 3) and tris.shape == (rec[2], 3) and vmap.shape == (mesh.vertices.shape[0],)
    return dict(vertices=nv.cpu().numpy(), colors=nc.cpu().numpy(), triangles=tris.cpu().numpy(), vertex_map=vmap.cpu().numpy(), record=tuple(rec))


def _same(got, want, name):
    for k in ("vertex_map", "triangles", "vertices", "colors"):
        g, w = got[k], want[k]
        bad = np.flatnonzero((g.view(np.int32) != w.view(np.int32)).reshape(len(g), -1).any(1)) if g.shape == w.shape and len(g) else []
        print(f"{name} {k}: {w.shape}, {len(bad)} rows differ")
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (name, k, bad[:8], g[bad[:8]], w[bad[:8]])
    print(f"{name} record: {got['record']}")
    assert got["record"] == want["record"], name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_against_the_truth(name, mode):
    v, c, t, vs = cases.CASES[name]
    _same(_run(_mesh(v, c, t), vs, mode), cases.truth(name, mode), f"{name} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["torus", "size_V1025", "strip_z_65536"])
def test_a_second_run_gives_identical_bits_and_the_input_is_unchanged(name, mode):
    v, c, t, vs = cases.CASES[name]
    mesh = _mesh(v, c, t)
    a, b = _run(mesh, vs, mode), _run(mesh, vs, mode)
    for k in ("vertices", "colors", "triangles", "vertex_map"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["record"] == b["record"]
    assert mesh.vertices.cpu().numpy().tobytes() == v.tobytes() and mesh.vertex_colors.cpu().numpy().tobytes() == c.tobytes()
    assert mesh.triangles.cpu().numpy().tobytes() == t.tobytes()


def _views(a):
    """The three layouts of test_gpu_chamfer._views: packed, a view one element into its storage, the first three columns of [P,4]."""
    P, dt = a.shape[0], torch.from_numpy(a).dtype
    buf = torch.empty(3 * P + 1, device=DEV, dtype=dt)
    view = buf[1:].view(P, 3)
    view.copy_(torch.from_numpy(a))
    wide = torch.full((P, 4), 7, device=DEV, dtype=dt)
    wide[:, :3] = torch.from_numpy(a).to(DEV)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and not wide[:, :3].is_contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV), view, wide[:, :3]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["size_V257", "cube"])
def test_input_layout(name, mode):
    v, c, t, vs = cases.CASES[name]
    want = cases.truth(name, mode)
    for i, (vv, cc, tt) in enumerate(zip(_views(v), _views(c), _views(t))):
        _same(_run(_mesh(vv, cc, tt), vs, mode), want, f"{name} {mode} layout {i}")
        assert vv.cpu().numpy().tobytes() == v.tobytes() and tt.cpu().numpy().tobytes() == t.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_the_method_and_the_function_agree(mode):
    import gsrast
    v, c, t, vs = cases.CASES["sphere"]
    mesh = _mesh(v, c, t)
    a = mesh.simplify_vertex_clustering(vs, mode)
    b, vmap = gsrast.simplify_vertex_clustering(mesh, vs, contraction=mode, return_map=True)
    assert a is not mesh and isinstance(a, type(mesh)) and isinstance(gsrast.simplify_vertex_clustering(mesh, vs), type(mesh))
    want = cases.truth("sphere", mode)
    for x in (a, b):
        assert x.vertices.cpu().numpy().tobytes() == want["vertices"].tobytes() and x.vertex_colors.cpu().numpy().tobytes() == want["colors"].tobytes()
        assert x.triangles.cpu().numpy().tobytes() == want["triangles"].tobytes()
    assert np.array_equal(vmap.cpu().numpy(), want["vertex_map"])


@pytest.mark.parametrize("mode", MODES)
def test_one_host_read_back_per_call(mode):
    """The record between count and emit is the call's only synchronisation (the way test_gpu_post_mesh counts them)."""
    import warnings
    import gsrast
    v, c, t, vs = cases.CASES["torus"]
    mesh = _mesh(v, c, t)
    gsrast.simplify_vertex_clustering(mesh, vs, mode, return_map=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            gsrast.simplify_vertex_clustering(mesh, vs, mode, return_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum(1 for x in w if "synchroniz" in str(x.message).lower()) == 1


@pytest.mark.parametrize("mode", MODES)
def test_torus_invariants(mode):
    v, c, t, vs = cases.CASES["torus"]
    out = _run(_mesh(v, c, t), vs, mode)
    n, tr, vm = out["record"][1], out["triangles"].astype(np.int64), out["vertex_map"]
    assert tr.min() >= 0 and tr.max() < n
    assert ((tr[:, 0] != tr[:, 1]) & (tr[:, 1] != tr[:, 2]) & (tr[:, 2] != tr[:, 0])).all()
    assert (tr[:, 0] < tr[:, 1]).all() and (tr[:, 0] < tr[:, 2]).all()                     # rotated: the smallest first
    assert len(np.unique(tr, axis=0)) == len(tr)                                             # no rotated triple twice
    assert np.array_equal(np.unique(vm), np.arange(n))                                       # onto [0, V')
    first = np.full(n, len(vm), np.int64)
    np.minimum.at(first, vm, np.arange(len(vm)))
    assert (np.diff(first) > 0).all()                                                        # numbered by the lowest member
    assert np.isfinite(out["vertices"]).all() and n < len(v) // 4 and len(tr) < len(t) // 4


def test_components_survive_and_post_process_mesh_runs_on_the_result():
    import gsrast
    v, c, t, vs = cases.CASES["two_components"]
    mesh = _mesh(v, c, t)
    before = gsrast.cluster_connected_triangles(mesh, with_area=False)[1]
    small = gsrast.simplify_vertex_clustering(mesh, vs)
    after = gsrast.cluster_connected_triangles(small, with_area=False)[1]
    assert before.numel() == after.numel() == 2
    v, c, t, vs = cases.CASES["torus"]
    small = gsrast.simplify_vertex_clustering(_mesh(v, c, t), vs, "quadric")
    post = gsrast.post_process_mesh(small, cluster_to_keep=1)
    assert post.triangles.shape[0] > 0 and post.triangles.shape[0] <= small.triangles.shape[0]
    assert int(post.triangles.max()) < post.vertices.shape[0]


def test_edge_shapes():
    import gsrast
    e = lambda dt: torch.empty((0, 3), dtype=dt, device=DEV)
    out, vmap = gsrast.simplify_vertex_clustering(_mesh(e(torch.float32), e(torch.float32), e(torch.int32)), 0.5, return_map=True)
    assert out.vertices.shape == out.vertex_colors.shape == out.triangles.shape == (0, 3) and vmap.shape == (0,) and out.vertices.is_cuda
    v, c, t, vs = cases.CASES["no_triangles"]
    for mode in MODES:
        _same(_run(_mesh(v, c, t), vs, mode), cases.truth("no_triangles", mode), f"no_triangles {mode}")
    span = np.array([(0, 0, 0), (2097150.5, 0, 0), (1, 1, 0)], dtype=np.float32)            # cells 0 .. 2^21 - 1: the last extent that fits
    got = _run(_mesh(span, c[:3], np.array([(0, 1, 2)], np.int32)), 1.0, "average")
    _same(got, truth.simplify(span, c[:3], np.array([(0, 1, 2)], np.int32), 1.0), "span")


def test_status_words_raise_the_documented_errors():
    """Input checks: every kernel treats such a value as data (a key, a refused index), nothing is dereferenced through it."""
    import gsrast
    match = {"nonfinite": "non-finite", "range": r"extent .* voxel_size .* 2\^21", "index": r"outside \[0, number of vertices\)"}
    for name, (v, c, t, vs, kind) in cases.errors().items():
        for mode in MODES:
            with pytest.raises(RuntimeError, match=match[kind]):
                gsrast.simplify_vertex_clustering(_mesh(v, c, t), vs, mode)
    v, c, t, _ = cases.CASES["alone"]
    mesh = _mesh(v, c, t)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            gsrast.simplify_vertex_clustering(mesh, bad)
    with pytest.raises(ValueError, match="contraction"):
        gsrast.simplify_vertex_clustering(mesh, 0.5, "edge_collapse")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        gsrast.simplify_vertex_clustering(mesh.cpu(), 0.5)
    empty_v = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match=match["index"]):                                  # triangles without vertices: every index is out of range
        gsrast.simplify_vertex_clustering(_mesh(empty_v, empty_v, t), 0.5)
