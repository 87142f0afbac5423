"""CPU tests of the mesh smoothing / normals feature: the restatement of tests/smooth_truth.py against an independent dense-matrix formulation and
against what the filters are for, the structure of the named cases, the TriangleMesh and PLY behaviour that needs no device, the argument errors
raised before any device call, and the header, the table and the library's exports."""
import copy
import os

import numpy as np
import pytest
import torch

import smooth_cases as cases
import smooth_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gsr_mesh_adjacency_scratch_bytes", "gsr_mesh_adjacency_count", "gsr_mesh_adjacency_emit", "gsr_mesh_normals_scratch_bytes", "gsr_mesh_normals",
         "gsr_mesh_smooth_scratch_bytes", "gsr_mesh_smooth"]


# ---------------------------------------------------------------------------------------------------------------- the truth
def _dense_adjacency(t, V):
    A = np.zeros((V, V), bool)
    for tri in np.asarray(t, dtype=np.int64):
        for a in tri:
            for b in tri:
                if a != b:
                    A[a, b] = True
    return A


def _dense_step(p, A, lam):
    """One step as matrix products: another order of the additions, so equal to the truth up to float64 round-off only."""
    deg = A.sum(1)
    if lam is None:
        return (p + A.astype(np.float64) @ p) / (deg + 1.0)[:, None]
    d = np.linalg.norm(p[:, None, :3] - p[None, :, :3], axis=2)
    Wm = np.where(A, 1.0 / (d + 1e-12), 0.0)
    W = Wm.sum(1)
    with np.errstate(all="ignore"):
        q = p + lam * ((Wm @ p) / W[:, None] - p)
    q[deg == 0] = p[deg == 0]
    return q


@pytest.mark.parametrize("name", cases.SMALL)
def test_truth_against_a_dense_matrix_formulation(name):
    v, c, t = cases.CASES[name]
    V = len(v)
    A = _dense_adjacency(t, V)
    start, nb = cases.truth_adjacency(name)
    assert np.array_equal(np.diff(start), A.sum(1)) and np.array_equal(nb, np.nonzero(A)[1])
    p0 = np.concatenate([v.astype(np.float64), c.astype(np.float64)], axis=1)
    for kind in cases.FILTERS:
        p = p0.copy()
        for _ in range(3):
            p = _dense_step(p, A, None if kind == "simple" else cases.LAMBDA)
            if kind == "taubin":
                p = _dense_step(p, A, cases.MU)
        gv, gc = truth.smooth(v, c, t, kind, 3, cases.LAMBDA, cases.MU, "all")
        scale = max(1.0, float(np.abs(p0).max())) if V else 1.0
        assert gv.shape == (V, 3) and gc.shape == (V, 3) and gv.dtype == gc.dtype == np.float32
        if V:                                             # float64 round-off, then one rounding to float32 on either side
            assert np.abs(gv - p[:, :3].astype(np.float32)).max() <= 2.0 ** -22 * scale and np.abs(gc - p[:, 3:].astype(np.float32)).max() <= 2.0 ** -22
        only_v, same_c = truth.smooth(v, c, t, kind, 3, cases.LAMBDA, cases.MU, "vertex")
        assert only_v.tobytes() == gv.tobytes() and same_c.tobytes() == c.tobytes()       # the colours never feed the positions
    # the normals: per-vertex sums of np.cross, another order of the operations
    n = np.cross(v.astype(np.float64)[t[:, 1]] - v.astype(np.float64)[t[:, 0]], v.astype(np.float64)[t[:, 2]] - v.astype(np.float64)[t[:, 0]]) if len(t) else np.zeros((0, 3))
    s = np.zeros((V, 3))
    for k in range(3):
        np.add.at(s, t[:, k], n)
    got = truth.vertex_normals(v, t, normalized=False).astype(np.float64)
    assert np.abs(got - s).max(initial=0.0) <= 1e-6 * max(1.0, np.abs(s).max(initial=0.0))
    assert truth.triangle_normals(v, t, normalized=False).tobytes() == n.astype(np.float32).tobytes() or np.allclose(truth.triangle_normals(v, t, False), n, rtol=1e-6, atol=1e-30)


def test_zero_iterations_and_isolated_vertices():
    v, c, t = cases.CASES["isolated"]
    for kind in cases.FILTERS:
        gv, gc = truth.smooth(v, c, t, kind, 0)
        assert gv.tobytes() == v.tobytes() and gc.tobytes() == c.tobytes()
        gv, gc = truth.smooth(v, c, t, kind, 4)
        used = np.zeros(len(v), bool)
        used[t.reshape(-1)] = True
        assert (~used).sum() == 4 and gv[~used].tobytes() == v[~used].tobytes() and gc[~used].tobytes() == c[~used].tobytes()       # N(i) empty: q = p
        assert not np.array_equal(gv[used], v[used]) and np.isfinite(gv).all()
    n = truth.vertex_normals(v, t)
    assert (n[~used] == (0, 0, 1)).all() and (truth.vertex_normals(v, t, normalized=False)[~used] == 0).all()


def test_an_interior_vertex_of_the_flat_sheet_does_not_move():
    v, c, t = cases.CASES["sheet_17x17"]
    i, j = np.meshgrid(np.arange(17), np.arange(17), indexing="ij")
    ring = np.minimum(np.minimum(i, 16 - i), np.minimum(j, 16 - j)).ravel()         # steps to the boundary
    for kind in cases.FILTERS:
        for n, steps in ((1, 1 if kind != "taubin" else 2), (3, 3 if kind != "taubin" else 6)):
            gv, _ = truth.smooth(v, c, t, kind, n, cases.LAMBDA, cases.MU)
            still = ring >= steps + 1                     # a step moves the influence of the boundary one ring inwards
            assert still.sum() > 0 and np.array_equal(gv[still], v[still]), (kind, n)
            assert not np.array_equal(gv[ring == 0], v[ring == 0])
    assert (truth.vertex_normals(v, t) == (0, 0, 1)).all() and (truth.triangle_normals(v, t) == (0, 0, 1)).all()


def test_torus_normals_are_close_to_the_analytic_ones():
    """Within one degree: the 32 x 16 torus has facets of 11 to 22 degrees, the area-weighted mean of the six around a vertex is far closer (the minimum dot
    product is 0.99993, 0.7 degrees)."""
    _, analytic = cases.torus_points()
    n = cases.truth_normals("torus", "vertex", True).astype(np.float64)
    dots = (n * analytic).sum(1)
    print("torus: minimum dot product", dots.min())
    assert dots.min() > np.cos(np.radians(1.0)) and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(np.diff(cases.truth_adjacency("torus")[0]), np.full(512, 6))


def _volume(v, t):
    v = v.astype(np.float64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def _roughness(v, t):
    start, nb = truth.adjacency(t, len(v))
    v = v.astype(np.float64)
    centroid = np.add.reduceat(v[nb], start[:-1].astype(np.int64)) / np.diff(start)[:, None]
    return float(np.linalg.norm(v - centroid, axis=1).mean())


def test_taubin_keeps_the_volume_and_every_filter_smooths():
    """torus_noisy, 10 iterations: volume 3.046 -> 3.113 (Taubin), 1.645 (Laplacian); roughness 0.0305 -> 0.0273 / 0.0199 / 0.0160."""
    v, c, t = cases.CASES["torus_noisy"]
    vol0, rough0 = _volume(v, t), _roughness(v, t)
    out = {k: cases.truth_smooth("torus_noisy", k, 10, "all")[0] for k in cases.FILTERS}
    vol = {k: _volume(out[k], t) for k in out}
    rough = {k: _roughness(out[k], t) for k in out}
    print("volume", vol0, vol, "roughness", rough0, rough)
    assert vol0 > 0 and abs(vol["taubin"] - vol0) < abs(vol["laplacian"] - vol0) and abs(vol["taubin"] - vol0) < 0.05 * vol0
    assert all(rough[k] < rough0 for k in out) and rough["simple"] < rough["laplacian"] < rough["taubin"]


def test_cases_have_the_structure_they_are_named_for():
    deg = {n: np.diff(cases.truth_adjacency(n)[0]) for n in cases.NAMES}
    for n in cases.NAMES:
        start, nb = cases.truth_adjacency(n)
        V = len(cases.CASES[n][0])
        assert start.shape == (V + 1,) and start[0] == 0 and start[-1] == len(nb) and start.dtype == nb.dtype == np.int32
        for i in range(0, V, max(1, V // 50)):
            row = nb[start[i]:start[i + 1]]
            assert (np.diff(row) > 0).all() and i not in row
        if not n.startswith("fan"):
            assert deg[n].max(initial=0) <= 64, n                                     # what the bars of the GPU tests are derived for
    assert [len(cases.CASES[f"size_V{k}"][0]) for k in (255, 256, 257, 1025)] == [255, 256, 257, 1025]
    for k in (1025, 5000):
        for tail in ("", "_closed"):
            d = deg[f"fan_{k}{tail}"]
            assert d[7] == k == d.max() and np.delete(d, 7).max() <= 3
    assert len(cases.CASES["empty"][0]) == 0 and len(cases.CASES["no_triangles"][2]) == 0 and len(cases.CASES["alone"][2]) == 1
    assert np.array_equal(deg["duplicates"], [2, 4, 3, 3, 2]) and np.array_equal(deg["degenerate"], [3, 4, 2, 3, 3, 0, 1])
    assert (cases.truth_normals("cancelling", "vertex", True) == (0, 0, 1)).all()
    assert (cases.truth_normals("cancelling", "vertex", False) == 0).all()
    far = cases.CASES["far_from_origin"][0]
    assert far.min() > 9999.0 and far.max() < 10002.0 and len(np.unique(far[:, 2])) == 3      # the detail is one float32 ulp (2^-10) either way
    assert len(cases.CASES["strip_z_65536"][0]) == 52000


def test_error_inputs_raise_in_the_truth():
    for name, (v, c, t, kind) in cases.errors().items():
        with pytest.raises(truth.MeshError) as e:
            truth.smooth(v, c, t, "taubin", 1)
        assert e.value.status == {"index": truth.ERR_INDEX, "nonfinite": truth.ERR_NONFINITE}[kind], name
        if kind == "index":
            for f in (lambda: truth.adjacency(t, len(v)), lambda: truth.vertex_normals(v, t), lambda: truth.triangle_normals(v, t)):
                with pytest.raises(truth.MeshError):
                    f()


# ---------------------------------------------------------------------------------------------------------------- TriangleMesh and PLY
def _host(name="sphere"):
    from gsrast.tsdf import TriangleMesh
    v, c, t = cases.CASES[name]
    return TriangleMesh(torch.from_numpy(v.copy()), torch.from_numpy(c.copy()), torch.from_numpy(t.copy()))


def test_triangle_mesh_carries_its_normals(monkeypatch):
    from gsrast import mesh as M
    from gsrast.tsdf import TriangleMesh
    m = _host()
    assert m.vertex_normals is None and m.triangle_normals is None and not m.has_vertex_normals() and not m.has_triangle_normals()
    vn = torch.from_numpy(cases.truth_normals("sphere", "vertex", True).copy())
    tn = torch.from_numpy(cases.truth_normals("sphere", "triangle", True).copy())
    m = TriangleMesh(m.vertices, m.vertex_colors, m.triangles, vn, tn)       # the fourth and fifth constructor arguments
    assert m.vertex_normals is vn and m.triangle_normals is tn and m.has_vertex_normals() and m.has_triangle_normals()
    for other in (m.cpu(), m.clone(), copy.deepcopy(m)):
        assert other is not m and torch.equal(other.vertex_normals, vn) and torch.equal(other.triangle_normals, tn)
        assert torch.equal(other.vertices, m.vertices) and torch.equal(other.triangles, m.triangles)
    for other in (m.clone(), copy.deepcopy(m)):
        assert other.vertex_normals.data_ptr() != vn.data_ptr() and other.triangle_normals.data_ptr() != tn.data_ptr()
    half = TriangleMesh(m.vertices, m.vertex_colors, m.triangles, vn)
    assert half.clone().triangle_normals is None and half.cpu().has_vertex_normals() and not half.has_triangle_normals()
    # the in-place filters drop them (the device pass is stood in for: what it returns is not the point here)
    monkeypatch.setattr(M, "_filter", lambda mesh, **kw: (mesh.vertices, mesh.vertex_colors, mesh.triangles[:5], [0] * 8))
    monkeypatch.setattr(M, "_arrays", lambda mesh: (mesh.vertices, mesh.vertex_colors, mesh.triangles))
    for call in (lambda x: x.remove_degenerate_triangles(), lambda x: x.remove_unreferenced_vertices(),
                 lambda x: x.remove_triangles_by_mask(np.zeros(len(x.triangles), bool))):
        x = m.clone()
        assert call(x) is x and x.vertex_normals is None and x.triangle_normals is None and x.triangles.shape[0] == 5
    assert m.has_vertex_normals()


def _parent_writer_bytes(v, c, t):
    """The file the writer produced before vertex normals existed, built by hand."""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    c8 = np.clip(np.rint(c.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    body = b"".join(v[i].astype("<f4").tobytes() + c8[i].tobytes() for i in range(len(v)))
    body += b"".join(b"\x03" + t[i].astype("<i4").tobytes() for i in range(len(t)))
    return head, ("\n".join(head) + "\n").encode("ascii") + body


def _header(path):
    with open(path, "rb") as f:
        return f.read().split(b"end_header\n")[0].decode("ascii").split("\n")[:-1] + ["end_header"]


def test_ply_with_and_without_normals(tmp_path):
    from gsrast import ply
    v, c, t = cases.CASES["sphere"]
    m = _host()
    plain = str(tmp_path / "plain.ply")
    ply.write_triangle_mesh(plain, m)
    head, want = _parent_writer_bytes(v, c, t)
    assert _header(plain) == head
    with open(plain, "rb") as f:
        assert f.read() == want
    back = ply.read_triangle_mesh(plain)
    assert back.vertex_normals is None and back.triangle_normals is None and back.vertices.numpy().tobytes() == v.tobytes()
    m.vertex_normals = torch.from_numpy(cases.truth_normals("sphere", "vertex", True).copy())
    m.triangle_normals = torch.from_numpy(cases.truth_normals("sphere", "triangle", True).copy())      # not part of the file
    with_n = str(tmp_path / "normals.ply")
    ply.write_triangle_mesh(with_n, m)
    assert _header(with_n) == head[:6] + ["property float nx", "property float ny", "property float nz"] + head[6:]
    back = ply.read_triangle_mesh(with_n)
    assert back.has_vertex_normals() and back.vertex_normals.dtype == torch.float32 and back.triangle_normals is None
    assert back.vertex_normals.numpy().tobytes() == m.vertex_normals.numpy().tobytes()
    assert back.vertices.numpy().tobytes() == v.tobytes() and back.triangles.numpy().tobytes() == t.tobytes()
    assert np.abs(back.vertex_colors.numpy() - c).max() <= 0.5 / 255 + 1e-7
    m.vertex_normals = m.vertex_normals[:-1]
    with pytest.raises(ValueError, match="normals"):
        ply.write_triangle_mesh(str(tmp_path / "bad.ply"), m)
    # a file with only two of the three columns has no normals
    two = str(tmp_path / "two.ply")
    with open(with_n, "rb") as f:
        data = f.read()
    with open(two, "wb") as f:
        f.write(data.replace(b"property float nz", b"property float qz"))
    assert ply.read_triangle_mesh(two).vertex_normals is None


# ---------------------------------------------------------------------------------------------------------------- refusals, header, binding
def test_argument_errors_are_raised_before_any_device_call():
    import gsrast
    host = _host("alone")                                 # a host mesh: anything that got as far as the arrays would raise RuntimeError instead
    filters = (gsrast.filter_smooth_simple, gsrast.filter_smooth_laplacian, gsrast.filter_smooth_taubin)
    for f in filters:
        for bad in (-1, 1.5, 2.0, "3", None, True):
            with pytest.raises(ValueError, match="number_of_iterations"):
                f(host, bad)
        with pytest.raises(ValueError, match="filter_scope"):
            f(host, 1, filter_scope="normal")
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lambda_filter"):
            gsrast.filter_smooth_laplacian(host, 1, bad)
        with pytest.raises(ValueError, match="lambda_filter"):
            gsrast.filter_smooth_taubin(host, 1, lambda_filter=bad)
        with pytest.raises(ValueError, match="mu"):
            gsrast.filter_smooth_taubin(host, 1, mu=bad)
        with pytest.raises(ValueError, match="mu"):
            host.filter_smooth_taubin(1, 0.5, bad)
    for f in filters + (gsrast.vertex_adjacency, gsrast.compute_triangle_normals, gsrast.compute_vertex_normals):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f(host)
    for f in (host.compute_vertex_normals, host.compute_triangle_normals, host.filter_smooth_simple, host.filter_smooth_laplacian, host.filter_smooth_taubin):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f()
    assert host.vertex_normals is None


def test_header_constants_match_gsrast_mesh():
    import abi_header
    from gsrast import mesh
    consts = abi_header.constants(abi_header.source("gsrast.h"))
    assert consts["GSR_SMOOTH_SIMPLE"] == mesh.SMOOTH_SIMPLE == 0 and consts["GSR_SMOOTH_LAPLACIAN"] == mesh.SMOOTH_LAPLACIAN == 1
    assert consts["GSR_SMOOTH_TAUBIN"] == mesh.SMOOTH_TAUBIN == 2
    assert consts["GSR_SMOOTH_SCOPE_ALL"] == mesh.SCOPES["all"] == 0 and consts["GSR_SMOOTH_SCOPE_VERTEX"] == mesh.SCOPES["vertex"] == 1
    assert consts["GSR_MESH_ERR_INDEX"] == mesh.ERR_INDEX == truth.ERR_INDEX and consts["GSR_MESH_ERR_NONFINITE"] == mesh.ERR_NONFINITE == truth.ERR_NONFINITE
    assert consts["GSR_ABI_VERSION"] == 8
    with open(os.path.join(ROOT, "include", "gsrast.h")) as f:
        text = f.read()
    for words in ("PARITY IS UNPINNED", "DEPARTURE from the model", "the only further channel that is filtered", "ascending\n *      corner index 3 t + k"):
        assert words in text, words


def test_library_exports_the_entry_points_and_the_abi_stays_8():
    import abi_header
    import gsrast
    from gsrast import _abi
    L = gsrast.lib()
    assert L.gsr_abi_version() == 8 == gsrast.ABI_VERSION
    rows = {name for name, _, _ in _abi.FUNCTIONS}
    declared = abi_header.functions(abi_header.source("gsrast.h"))
    for name in NAMES:
        assert name in rows and name in declared and name in gsrast.EXPORTS and getattr(L, name).argtypes is not None, name
    for name in ("vertex_adjacency", "compute_triangle_normals", "compute_vertex_normals", "filter_smooth_simple", "filter_smooth_laplacian", "filter_smooth_taubin"):
        assert getattr(gsrast, name) is getattr(gsrast.mesh, name), name
    for name in ("compute_triangle_normals", "compute_vertex_normals", "filter_smooth_simple", "filter_smooth_laplacian", "filter_smooth_taubin",
                 "has_vertex_normals", "has_triangle_normals"):
        assert callable(getattr(gsrast.tsdf.TriangleMesh, name)), name


def test_scratch_queries_refuse_what_the_kernels_cannot_index():
    import gsrast
    L = gsrast.lib()
    # V = 2^31 - 1 and 6T = 2^32 - 4096 are the last sizes that fit: the 6T pairs go through grids and block counts that round their number up by as
    # much as 4096 (the sort's largest block) in 32-bit arithmetic, and from 6T = 2^32 - 4095 on that sum wraps -- 3T < 2^31 alone let 682 sizes through
    last_T, last_V = ((1 << 32) - 4096) // 6, (1 << 31) - 1
    assert 6 * last_T + 4095 < 1 << 32 <= 6 * (last_T + 1) + 4095 and 3 * (last_T + 1) < 1 << 31
    for q in (L.gsr_mesh_adjacency_scratch_bytes, L.gsr_mesh_normals_scratch_bytes, lambda T, V: L.gsr_mesh_smooth_scratch_bytes(T, V, 0),
              lambda T, V: L.gsr_mesh_smooth_scratch_bytes(T, V, 1)):
        assert q(0, 0) > 0 and q(1000, 600) > q(10, 600) > 0
        assert q(last_T + 1, 10) == 0 and q(10, last_V + 1) == 0 and q(-1, 10) == 0 and q(10, -1) == 0
        assert q(last_T, last_V) > 0
    s = L.gsr_mesh_smooth_scratch_bytes
    assert s(1000, 600, 2) == 0 and s(1000, 600, -1) == 0
    assert s(1000, 600, 0) - s(1000, 600, 1) >= 2 * 600 * 24 - 2 * 256                # two states of six doubles against two of three, 256-byte carving
    assert s(1000, 600, 0) > L.gsr_mesh_adjacency_scratch_bytes(1000, 600)
