"""The mesh filter without a GPU: the numpy restatement (ref_post_mesh_numpy) against hand-written answers -- the same cases the device is then
held to in test_gpu_post_mesh.py -- and gsrast.mesh's behaviour where there is no device."""
import numpy as np
import pytest
import torch

import post_mesh_cases as cases
import ref_post_mesh_numpy as ref


@pytest.mark.parametrize("name,tris,clusters,counts", cases.HAND_CLUSTERS, ids=[c[0] for c in cases.HAND_CLUSTERS])
def test_hand_written_clusters(name, tris, clusters, counts):
    tc, cn, area = ref.cluster_connected_triangles(np.array(tris, np.int32))
    assert tc.dtype == np.int32 and cn.dtype == np.int32 and area is None
    assert tc.tolist() == clusters and cn.tolist() == counts


def test_cluster_area_is_the_float64_sum():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 5], [5, 5, 7], [5, 8, 5]], np.float32)
    tc, cn, area = ref.cluster_connected_triangles([[0, 1, 2], [4, 5, 6], [2, 1, 3]], v)
    assert tc.tolist() == [0, 1, 0] and cn.tolist() == [2, 1]
    assert area.dtype == np.float64 and area.tolist() == [1.0, 3.0]


def test_degenerate_triangle_survives_the_vertex_pass():
    v, c, t, want = cases.degenerate_case()
    tc, cn, _ = ref.cluster_connected_triangles(t)
    assert sorted(cn.tolist()) == [3, 52]
    gv, gc, gt, (v3, c3, t3) = ref.post_process_mesh(v, c, t, cluster_to_keep=1)
    assert len(t3) == want["step3_triangles"] and len(v3) == 53                 # D1 and D2 are still there and hold vertex 55
    assert np.array_equal(gt, want["triangles"]) and gt.dtype == np.int32
    assert gv.tobytes() == want["vertices"].tobytes() and gc.tobytes() == want["colors"].tobytes()
    assert not (gt == 52).any()                                                 # old vertex 55: kept, referenced by nothing any more


def _sizes_after(v, c, t, k):
    gv, gc, gt, _ = ref.post_process_mesh(v, c, t, cluster_to_keep=k)
    _, cn, _ = ref.cluster_connected_triangles(gt)
    assert len(gv) == len(gc) == (int(gt.max()) + 1 if len(gt) else 0)
    return cn.tolist()


def test_ties_at_the_threshold_are_kept():
    v, c, t = cases.clusters_mesh(cases.TIES["sizes"], seed=1, shuffle=False)
    _, cn, _ = ref.cluster_connected_triangles(t)
    assert ref.threshold(cn, cases.TIES["k"]) == cases.TIES["threshold"]
    assert _sizes_after(v, c, t, cases.TIES["k"]) == cases.TIES["kept_sizes"]


def test_floor_of_50():
    v, c, t = cases.clusters_mesh(cases.FLOOR_CASE["sizes"], seed=2, shuffle=False)
    _, cn, _ = ref.cluster_connected_triangles(t)
    assert ref.threshold(cn, cases.FLOOR_CASE["k"]) == cases.FLOOR_CASE["threshold"]
    assert _sizes_after(v, c, t, cases.FLOOR_CASE["k"]) == cases.FLOOR_CASE["kept_sizes"]


@pytest.mark.parametrize("k", sorted(cases.MATRIX))
def test_threshold_matrix(k):
    v, c, t = cases.clusters_mesh(cases.MATRIX_SIZES, seed=3, shuffle=False)
    _, cn, _ = ref.cluster_connected_triangles(t)
    thr, kept = cases.MATRIX[k]
    assert ref.threshold(cn, k) == thr and _sizes_after(v, c, t, k) == kept


def test_survivors_keep_their_order_and_colours_move_with_vertices():
    v, c, t = cases.clusters_mesh([3, 70, 2, 55], seed=4, spare_vertices=2)
    gv, gc, gt, _ = ref.post_process_mesh(v, c, t, cluster_to_keep=2)
    big = np.isin(t[:, 0], np.r_[np.arange(2 + 5, 2 + 5 + 72), np.arange(2 + 5 + 72 + 4, 2 + 5 + 72 + 4 + 57)])
    assert len(gt) == 125 and big.sum() == 125
    assert np.array_equal(gv[gt], v[t[big]]) and np.array_equal(gc[gt], c[t[big]])       # the same corners, in the same triangle order
    assert len(gv) == 72 + 57


def test_errors():
    v, c, t = cases.clusters_mesh([60, 3], seed=0)
    with pytest.raises(IndexError):
        ref.post_process_mesh(v, c, t, cluster_to_keep=3)
    with pytest.raises(IndexError):
        ref.post_process_mesh(v[:0], c[:0], t[:0], cluster_to_keep=1)
    for k in (0, -1):
        with pytest.raises(ValueError):
            ref.post_process_mesh(v, c, t, cluster_to_keep=k)


def test_no_cpu_path():
    """gsrast.mesh fails loudly for a host mesh, as ScalableTSDFVolume does for a host device; argument errors come first."""
    import gsrast
    from gsrast import mesh
    from gsrast.tsdf import TriangleMesh
    assert gsrast.post_process_mesh is mesh.post_process_mesh and gsrast.cluster_connected_triangles is mesh.cluster_connected_triangles
    v, c, t = (torch.from_numpy(a) for a in cases.clusters_mesh([60, 3]))
    m = TriangleMesh(v, c, t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh.post_process_mesh(m, 1)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh.cluster_connected_triangles(m)
    for call in (m.cluster_connected_triangles, m.remove_unreferenced_vertices, m.remove_degenerate_triangles, lambda: m.remove_triangles_by_mask(np.zeros(63, bool))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    for k in (0, -3, 1.5):
        with pytest.raises(ValueError, match="cluster_to_keep"):
            mesh.post_process_mesh(m, k)
    assert torch.equal(m.triangles, t) and m.vertices is v
    import copy
    d = copy.deepcopy(m)
    assert torch.equal(d.triangles, t) and d.triangles.data_ptr() != t.data_ptr() and torch.equal(m.clone().vertices, v)


def test_argument_errors_of_the_c_abi_without_a_device():
    import ctypes as C
    import gsrast
    from gsrast import mesh
    L = gsrast.lib()
    buf = (C.c_uint32 * 64)()
    a = C.addressof(buf)
    assert L.gsr_mesh_post_scratch_bytes(1 << 30, 10) == 0 and L.gsr_mesh_post_scratch_bytes(-1, 10) == 0           # 3T >= 2^31
    small, big = L.gsr_mesh_post_scratch_bytes(1000, 0), L.gsr_mesh_post_scratch_bytes(1000, 1 << 20)
    assert 0 < small < big and big - small >= 9 << 20
    assert L.gsr_mesh_post_scratch_bytes(10 ** 7, 0) <= 10 ** 7 * (16 * 12 + 32)                                   # at most 16 table slots per triangle
    assert L.gsr_mesh_cluster_triangles(a, 1 << 30, 10, None, a, a, None, a, 1 << 20, a, None) != 0 and "2^31" in gsrast.last_error()
    assert L.gsr_mesh_cluster_triangles(a, 4, 10, None, a, a, None, a, 16, a, None) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_mesh_cluster_triangles(a, 4, 10, None, a, a, a, a, 1 << 20, a, None) != 0 and "vertices" in gsrast.last_error()
    f = mesh.Filter(a, a, 4, 10, 3, 50, 0, 0)
    assert L.gsr_mesh_filter_count(C.byref(f), a, 1 << 20, a, None) != 0 and "exclude" in gsrast.last_error()
    f = mesh.Filter(a, None, 4, 10, 0, 50, 8, 0)
    assert L.gsr_mesh_filter_count(C.byref(f), a, 1 << 20, a, None) != 0 and "flags" in gsrast.last_error()
    f = mesh.Filter(a, None, 4, 10, 1, 50, 3, 0)
    rec = (C.c_uint32 * 8)(1, 0, 0, 0, 0)
    assert L.gsr_mesh_filter_emit(C.byref(f), a, 1 << 20, rec, 0, None, a, None) != 0 and "status" in gsrast.last_error()
