"""GPU tests (pytest -m gpu) of gsrast.mesh (gsr_mesh_* of the C ABI, csrc/gsr_mesh_post.hip) against the numpy / scipy restatement of the mesh
filter's definition (ref_post_mesh_numpy) and the hand-written answers of post_mesh_cases.  Every comparison is exact (array or byte equality)
but the cluster areas, whose bound is derived in _check_area."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import post_mesh_cases as cases
import ref_post_mesh_numpy as ref

pytestmark = pytest.mark.gpu


def _mesh(v, c, t):
    from gsrast.tsdf import TriangleMesh
    return TriangleMesh(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (v, c, t)))


def _bytes(m):
    return tuple(x.cpu().numpy().tobytes() for x in (m.vertices, m.vertex_colors, m.triangles))


def _check_area(got, tris, verts, clusters, counts):
    """|got - want| <= n 2^-52 want + 16 2^-52 sum |e1| |e2| per cluster of n triangles, want = the float64 sum of numpy.
    Summation order: any order of n non-negative terms is within (n - 1) u sum of the exact sum, u = 2^-53, and so is numpy's: 2 (n - 1) u <= n 2^-52.
    A term: e1, e2 are exact in double (differences of float32 values); each of the 3 components of the cross product carries 2 rounded products
    and a rounded difference (<= 3 u |e1| |e2| each), the norm and the halving add a few u of the value <= |e1| |e2| / 2: well below
    16 2^-52 |e1| |e2| for both sides together."""
    want = np.zeros(len(counts)); slack = np.zeros(len(counts))
    p = verts.astype(np.float64)[tris.astype(np.int64)]
    np.add.at(want, clusters, ref.triangle_areas(verts, tris))
    np.add.at(slack, clusters, np.linalg.norm(p[:, 1] - p[:, 0], axis=1) * np.linalg.norm(p[:, 2] - p[:, 0], axis=1))
    bound = counts * 2.0 ** -52 * want + 16 * 2.0 ** -52 * slack
    err = np.abs(got - want)
    print(f"area: {len(counts)} clusters, largest error / bound {np.max(err / np.maximum(bound, 1e-300)) if len(counts) else 0:.3f}")
    assert (err <= bound).all()


def _check_clusters(v, c, t):
    from gsrast import mesh
    rc, rn, _ = ref.cluster_connected_triangles(t)
    tc, cn, area = mesh.cluster_connected_triangles(_mesh(v, c, t))
    assert tc.dtype == torch.int32 and cn.dtype == torch.int32 and area.dtype == torch.float64 and tc.is_cuda and cn.is_cuda and area.is_cuda
    assert np.array_equal(tc.cpu().numpy(), rc) and np.array_equal(cn.cpu().numpy(), rn)
    _check_area(area.cpu().numpy(), t, v, rc, rn)
    tc2, cn2, none = mesh.cluster_connected_triangles(_mesh(v, c, t), with_area=False)
    assert none is None and torch.equal(tc, tc2) and torch.equal(cn, cn2)
    return rn


def _check_post(v, c, t, k):
    from gsrast import mesh
    want = ref.post_process_mesh(v, c, t, cluster_to_keep=k)[:3]
    m = _mesh(v, c, t)
    before = _bytes(m)
    out = mesh.post_process_mesh(m, k)
    assert _bytes(m) == before                                           # the input is left untouched
    assert out.vertices.is_cuda and out.triangles.dtype == torch.int32 and tuple(out.triangles.shape) == want[2].shape
    assert tuple(out.vertices.shape) == want[0].shape and tuple(out.vertex_colors.shape) == want[1].shape
    assert _bytes(out) == tuple(np.ascontiguousarray(a).tobytes() for a in want)
    return out


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 1025, 70001])
def test_t_sweep(T):
    """Scan-block edges (256 threads a block in the unit's kernels, 1024 in the keep scan) and a multi-block scan of block sums."""
    v, c, t = cases.mixed_mesh(T, seed=T)
    counts = _check_clusters(v, c, t)
    for k in sorted({1, min(2, len(counts)), len(counts)}):
        _check_post(v, c, t, k)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_adversarial_grids(seed):
    """Long union chains and hooking races: two 64 x 64 grids joined at one vertex, triangle order and corner order scrambled."""
    from gsrast import mesh
    v, c, t, which = cases.adversarial_grids(64, seed)
    assert len(t) == 2 * 8192
    tc, cn, _ = mesh.cluster_connected_triangles(_mesh(v, c, t))
    tc, cn = tc.cpu().numpy(), cn.cpu().numpy()
    assert cn.tolist() == [8192, 8192]
    assert np.array_equal(tc, (which != which[0]).astype(np.int32))      # the grid of triangle 0 is cluster 0
    _check_clusters(v, c, t)
    out = _check_post(v, c, t, 1)                                        # a tie: both grids stay, no vertex goes
    assert out.triangles.shape[0] == len(t) and out.vertices.shape[0] == len(v)


@pytest.mark.parametrize("name,tris,clusters,counts", cases.HAND_CLUSTERS, ids=[c[0] for c in cases.HAND_CLUSTERS])
def test_hand_written_clusters(name, tris, clusters, counts):
    from gsrast import mesh
    v, c, t = cases.with_attributes(np.array(tris, np.int32), int(np.max(tris)) + 1)
    tc, cn, _ = mesh.cluster_connected_triangles(_mesh(v, c, t))
    assert tc.tolist() == clusters and cn.tolist() == counts


def test_degenerate_triangle_survives_the_vertex_pass():
    from gsrast import mesh
    v, c, t, want = cases.degenerate_case()
    out = mesh.post_process_mesh(_mesh(v, c, t), 1)
    assert _bytes(out) == (want["vertices"].tobytes(), want["colors"].tobytes(), want["triangles"].tobytes())
    _check_post(v, c, t, 1)


@pytest.mark.parametrize("case", [cases.TIES, cases.FLOOR_CASE], ids=["ties", "floor"])
def test_ties_and_floor(case):
    from gsrast import mesh
    v, c, t = cases.clusters_mesh(case["sizes"], seed=1, shuffle=False)
    out = _check_post(v, c, t, case["k"])
    _, cn, _ = mesh.cluster_connected_triangles(out)
    assert cn.tolist() == case["kept_sizes"]


@functools.lru_cache(maxsize=None)
def _matrix_mesh():
    return cases.clusters_mesh(cases.MATRIX_SIZES, seed=3, shuffle=True, spare_vertices=3)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7])
def test_threshold_matrix(k):
    from gsrast import mesh
    v, c, t = _matrix_mesh()
    out = _check_post(v, c, t, k)
    _, cn, _ = mesh.cluster_connected_triangles(out)
    assert sorted(cn.tolist()) == sorted(cases.MATRIX[k][1])


SELECT_SIZES = [1, 2, 255, 256, 257, 65536, 65537]


@functools.lru_cache(maxsize=None)
def _select_mesh():
    return cases.clusters_mesh(SELECT_SIZES, seed=5, shuffle=True, spare_vertices=2)


def test_select_decided_in_every_byte(monkeypatch):
    """Seven strips whose sizes part in different passes of the radix select of the k-th largest count: 1, 2 and 255 share everything but the lowest
    byte, 256 and 257 are told from them by the second byte and from each other by the lowest, 65536 and 65537 by the third and the lowest (a top
    byte other than 0 would take 2^24 triangles).  Every k from 1 to 7 through post_process_mesh, where the floor of 50 hides the thresholds 1 and 2;
    and with the floor at 0, in the restatement and in the filter, so that each of the seven thresholds is the one applied."""
    from gsrast import mesh
    v, c, t = _select_mesh()
    for k in range(1, 8):
        _check_post(v, c, t, k)
    with pytest.raises(IndexError, match="index -8 is out of bounds for axis 0 with size 7"):
        mesh.post_process_mesh(_mesh(v, c, t), 8)
    monkeypatch.setattr(mesh, "FLOOR", 0)
    monkeypatch.setattr(ref, "FLOOR", 0)
    m = _mesh(v, c, t)
    for k in range(1, 8):
        want = ref.post_process_mesh(v, c, t, cluster_to_keep=k)[:3]
        nv, nc, tris, rec = mesh._filter(m, cluster_to_keep=k, flags=mesh.DROP_UNREFERENCED | mesh.DROP_DEGENERATE)
        assert rec[:3] == [0, 7, sorted(SELECT_SIZES)[-k]], (k, rec)
        assert tuple(x.cpu().numpy().tobytes() for x in (nv, nc, tris)) == tuple(np.ascontiguousarray(a).tobytes() for a in want), k
        assert int(tris.shape[0]) == sum(n for n in SELECT_SIZES if n >= sorted(SELECT_SIZES)[-k])


def test_errors():
    from gsrast import mesh
    v, c, t = _matrix_mesh()
    m = _mesh(v, c, t)
    with pytest.raises(IndexError):
        mesh.post_process_mesh(m, 8)
    with pytest.raises(IndexError):
        mesh.post_process_mesh(_mesh(v[:0], c[:0], t[:0]), 1)
    for k in (0, -1):
        with pytest.raises(ValueError):
            mesh.post_process_mesh(m, k)
    tc, cn, area = mesh.cluster_connected_triangles(_mesh(v, c, t[:0]))
    assert tc.shape[0] == 0 and cn.shape[0] == 0 and area.shape[0] == 0
    from gsrast.tsdf import TriangleMesh
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh.post_process_mesh(TriangleMesh(m.vertices, m.vertex_colors, m.triangles.cpu()), 1)


def test_index_out_of_range_is_an_error_not_a_fault():
    from gsrast import mesh
    v, c, t = _matrix_mesh()
    for bad in (len(v), -1, 2 ** 31 - 1):
        t2 = t.copy()
        t2[len(t2) // 2, 1] = bad
        m = _mesh(v, c, t2)
        with pytest.raises(RuntimeError, match="outside"):
            mesh.post_process_mesh(m, 1)
        with pytest.raises(RuntimeError, match="outside"):
            mesh.cluster_connected_triangles(m)
        with pytest.raises(RuntimeError, match="outside"):
            m.remove_unreferenced_vertices()
        assert np.array_equal(m.triangles.cpu().numpy(), t2)             # a refused in-place call leaves the mesh as it was
    _check_post(v, c, t, 2)                                              # and the next call is served


def test_large_indices_through_the_c_abi():
    """Null vertices, V = 2^31 - 1: nothing of that size is allocated, the edge keys use all of their 62 bits."""
    import gsrast
    from gsrast import check, ptr, stream_ptr
    _, _, t = cases.mixed_mesh(3000, seed=11)
    r = np.random.default_rng(12)
    nv = int(t.max()) + 1
    ends = np.array([0, 2 ** 30, 2 ** 31 - 2])
    pool = np.setdiff1d(np.concatenate([r.integers(0, 20000, nv), 2 ** 30 + r.integers(-20000, 20000, nv), 2 ** 31 - 2 - r.integers(0, 20000, nv)]), ends)
    spread = r.permutation(np.concatenate([ends, r.permutation(pool)[:nv - 3]]))      # vertex id -> index: near 0, near 2^30, up to 2^31 - 2
    big = spread[t].astype(np.int32)
    assert big.max() <= 2 ** 31 - 2 and big.min() >= 0 and len(np.unique(spread)) == nv
    rc, rn, _ = ref.cluster_connected_triangles(big)
    assert np.array_equal(rn, ref.cluster_connected_triangles(t)[1])
    T, V = len(big), 2 ** 31 - 1
    L = gsrast.lib()
    tris = torch.from_numpy(big).cuda()
    tc, cn = torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda")
    nbytes = L.gsr_mesh_post_scratch_bytes(T, 0)
    scratch, status = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    check(L.gsr_mesh_cluster_triangles(ptr(tris), T, V, None, ptr(tc), ptr(cn), None, ptr(scratch), nbytes, ptr(status), stream_ptr()), "cluster")
    st, n = status.tolist()
    assert st == 0 and n == len(rn)
    assert np.array_equal(tc.cpu().numpy(), rc) and np.array_equal(cn[:n].cpu().numpy(), rn) and not cn[n:].any()


def test_step_by_step_equals_one_call():
    """The body of the reference's post_process_mesh (gssr/utils/mesh_utils.py:33-45), run against TriangleMesh's four methods."""
    from gsrast import mesh
    v, c, t0 = _matrix_mesh()
    t = np.concatenate([t0, [[3, 3, 4], [10, 11, 11]]]).astype(np.int32)             # two index-degenerate triangles on the strip of 200
    m = _mesh(v, c, t)
    before = _bytes(m)
    for k in (2, 5):
        mesh_0 = copy.deepcopy(m)
        triangle_clusters, cluster_n_triangles, cluster_area = (mesh_0.cluster_connected_triangles())
        triangle_clusters = np.asarray(triangle_clusters)
        cluster_n_triangles = np.asarray(cluster_n_triangles)
        cluster_area = np.asarray(cluster_area)
        n_cluster = np.sort(cluster_n_triangles.copy())[-k]
        n_cluster = max(n_cluster, 50)
        triangles_to_remove = cluster_n_triangles[triangle_clusters] < n_cluster
        mesh_0.remove_triangles_by_mask(triangles_to_remove)
        n_after_mask = int(mesh_0.triangles.shape[0])
        mesh_0.remove_unreferenced_vertices()
        mesh_0.remove_degenerate_triangles()
        assert int(mesh_0.triangles.shape[0]) == n_after_mask - 2 and mesh_0.vertices.shape[0] < len(v)
        one = mesh.post_process_mesh(m, k)
        assert _bytes(one) == _bytes(mesh_0) and _bytes(m) == before
        assert _bytes(one) == tuple(np.ascontiguousarray(a).tobytes() for a in ref.post_process_mesh(v, c, t, k)[:3])
    # a torch mask on the device serves as well as a numpy one
    a, b = copy.deepcopy(m), copy.deepcopy(m)
    mask = np.arange(len(t)) % 3 == 0
    a.remove_triangles_by_mask(mask); b.remove_triangles_by_mask(torch.from_numpy(mask).cuda())
    assert _bytes(a) == _bytes(b) and np.array_equal(a.triangles.cpu().numpy(), t[~mask]) and a.vertices.shape[0] == len(v)


def test_one_host_read_back_per_call():
    import warnings
    from gsrast import mesh
    m = _mesh(*_matrix_mesh())
    mesh.post_process_mesh(m, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            mesh.post_process_mesh(m, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum(1 for x in w if "synchroniz" in str(x.message).lower()) == 1


def test_end_to_end_from_a_volume(tmp_path):
    """One sphere and three small separate blobs in a ScalableTSDFVolume -> extract_triangle_mesh -> post_process_mesh(., 1) -> PLY and back."""
    import ref_mesh_numpy as rm
    from gsrast import mesh, ply
    from gsrast.tsdf import ScalableTSDFVolume
    n, h = 48, 0.05
    g = (np.arange(n, dtype=np.float64) + 0.5) * h
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    balls = [((0.8131, 0.7877, 0.8023), 0.41), ((2.01, 0.52, 0.49), 0.09), ((1.97, 1.93, 0.61), 0.11), ((0.55, 2.02, 1.96), 0.08)]
    sdf = np.minimum.reduce([np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r for (cx, cy, cz), r in balls])
    tsdf = np.minimum(1.0, sdf / (5 * h)).astype(np.float32)
    col = (np.stack([X, Y, Z], axis=-1) / (n * h) * 255.0).astype(np.float32)
    vol = ScalableTSDFVolume(h, 5 * h, capacity_units=32)
    vol.merge_units_(*(torch.from_numpy(a).cuda() for a in rm.units_from_dense(tsdf, np.ones_like(tsdf), col, (0, 0, 0))), assume_unique=True)
    raw = vol.extract_triangle_mesh()
    rv, rc, rt = (x.cpu().numpy() for x in (raw.vertices, raw.vertex_colors, raw.triangles))
    _, counts, _ = ref.cluster_connected_triangles(rt)
    assert len(counts) == 4 and sorted(counts.tolist())[-2] < counts.max()
    post = mesh.post_process_mesh(raw, 1)
    want = ref.post_process_mesh(rv, rc, rt, 1)[:3]
    assert _bytes(post) == tuple(np.ascontiguousarray(a).tobytes() for a in want)
    tc, cn, _ = mesh.cluster_connected_triangles(post)
    assert cn.tolist() == [int(counts.max())] and not tc.any()
    top = rm.topology(post.triangles.cpu().numpy(), int(post.vertices.shape[0]))
    assert top["watertight"] and top["euler"] == 2 and top["unused"] == 0
    path = str(tmp_path / "fuse_post.ply")
    ply.write_triangle_mesh(path, post)
    back = ply.read_triangle_mesh(path)
    assert np.array_equal(back.triangles.numpy(), want[2]) and back.vertices.numpy().tobytes() == want[0].tobytes()
