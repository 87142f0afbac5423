"""CPU tests of the surface-distance feature (gsrast.chamfer): the restatements of tests/chamfer_truth.py on hand-worked inputs, the structure the
named cases of tests/chamfer_cases.py rest on (under the documented cell rule), and what can be held without a GPU of the binding: the exports, the
ABI version, the host-side argument errors."""
import math
import os
import re

import numpy as np
import pytest

import chamfer_cases as cases
import chamfer_truth as truth

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-sr_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------- the truth, by hand
def test_nearest_by_hand():
    t = cases.a3([[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 3, 0]])
    q = cases.a3([[1.5, 0, 0], [1, 0, 0], [0, 2, 0]])
    d2, i = truth.nearest(q, t)
    assert d2.dtype == np.float32 and i.dtype == np.int32
    assert d2.tolist() == [0.25, 1.0, 1.0] and i.tolist() == [1, 0, 3]           # duplicate 1 / 2 -> 1; tie 0 / 1 at d2 = 1 -> 0; (0,3,0) beats (0,0,0)
    d2, i = truth.nearest(q, t, max_dist=0.75)                                  # 0.5625: only the first query keeps its target
    assert d2.tolist() == [0.25, np.inf, np.inf] and i.tolist() == [1, -1, -1]
    d2, i = truth.nearest(q, t, max_dist=1.0)                                   # equality stays in
    assert d2.tolist() == [0.25, 1.0, 1.0] and i.tolist() == [1, 0, 3]


def test_nearest_rounds_every_operation_in_float32():
    q = cases.a3([[0, 0, 0]]); t = cases.a3([[1 + 2 ** -12, 2 ** -12, 1]])
    dx = F(1 + 2 ** -12)
    want = F(F(F(dx * dx) + F(F(2 ** -12) * F(2 ** -12))) + F(1))
    assert truth.nearest(q, t)[0][0] == want and float(want) != (1 + 2 ** -12) ** 2 + 2 ** -24 + 1


def test_nearest_non_finite_and_empty():
    t = cases.a3([[np.nan, 0, 0], [0, np.inf, 0], [5, 0, 0]])
    q = cases.a3([[0, 0, 0], [np.nan, 0, 0], [0, 0, -np.inf]])
    d2, i = truth.nearest(q, t)
    assert d2.tolist() == [25.0, np.inf, np.inf] and i.tolist() == [2, -1, -1]
    for qq, tt in ((q, t[:2]), (q, t[:0])):
        d2, i = truth.nearest(qq, tt)
        assert np.isinf(d2).all() and (i == -1).all()
    assert truth.nearest(q[:0], t)[0].shape == (0,)


def test_cap_identity():
    """nearest(., ., m) is nearest(., ., None) with the rows beyond the cap voided: what the 20 000-point GPU cases use for their capped runs."""
    q, t = cases.NEAREST["size_Q257_T257"][:2]
    free = truth.nearest(q, t)
    for m in (0.05, 0.1, 0.2, float(np.sqrt(free[0][3]))):
        got, want = truth.cap(*free, m), truth.nearest(q, t, m)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (truth.nearest(q, t, 0.1)[1] == -1).any() and (truth.nearest(q, t, 0.1)[1] >= 0).any()


def test_sampler_by_hand():
    v = [[0, 0, 0], [3, 0, 0], [0, 3, 0]]
    p = truth.sample_surface(v, [[0, 1, 2]], 10.0)                              # n = 1: the centroid
    assert p.tolist() == [[1.0, 1.0, 0.0]]
    p = truth.sample_surface(v, [[0, 1, 2]], 3.0)                               # longest edge sqrt(18) = 4.24: n = 2
    want = np.array([[0.5, 0.5, 0], [0.5, 2.0, 0], [1.0, 1.0, 0], [2.0, 0.5, 0]])      # row 0: up j = 0, 1, down j = 0; row 1: up
    assert p.shape == (4, 3) and np.abs(p - want).max() < 1e-6
    two = truth.sample_surface(v + [[3, 3, 0]], [[0, 1, 2], [1, 3, 2]], 3.0)
    assert two.shape == (8, 3) and np.array_equal(two[:4], p)
    assert len({tuple(r) for r in two.tolist()}) == 8                           # no sample on the shared edge: none is shared
    assert truth.sample_surface(v, np.zeros((0, 3), np.int32), 1.0).shape == (0, 3)
    for bad, word in (((v, [[0, 1, 3]], 1.0), "index"), ((v, [[0, -1, 2]], 1.0), "index"), ((v, [[0, 1, 2]], 1e-3), "cap")):
        with pytest.raises(ValueError, match=word):
            truth.sample_surface(*bad)


@pytest.mark.parametrize("name", sorted(cases.MESH_N))
def test_sampler_cases_have_the_n_they_are_named_for(name):
    v, t, s = cases.MESHES[name]
    assert truth.triangle_n(v[t[0, 0]], v[t[0, 1]], v[t[0, 2]], s) == cases.MESH_N[name]
    assert len(truth.sample_surface(v, t, s)) == cases.MESH_N[name] ** 2


def test_sampler_case_structure():
    v, t, s = cases.MESHES["edge_one_ulp_above"]
    assert v[1, 0] == np.nextafter(F(3), F(4)) and math.sqrt(float(F(v[1, 0] * v[1, 0]))) / s > 3.0
    v, t, s = cases.MESHES["zero_area"]
    p = truth.sample_surface(v, t, s)
    assert len(p) == 16 and (p[:, 1:] == 0).all()                               # collinear: n = 4 from the longest edge, every sample on the line
    v, t, s = cases.MESH_ABOVE_CAP
    assert truth.triangle_n(v[0], v[1], v[2], s) == 2000 > truth.MAX_N
    v, t, s = cases.MESHES["T65"]
    ns = [truth.triangle_n(v[a], v[b], v[c], s) for a, b, c in t]
    assert min(ns) >= 1 and max(ns) >= 3 and len(set(ns)) >= 3                  # the block scan meets different counts
    # more than one block of the sampler: the count writes one sum per SS_BLOCK triangles, the emit searches their scanned sums first
    B = cases.SAMPLER_BLOCK
    src = open(os.path.join(CSRC, "gsr_chamfer.hip")).read()
    assert re.search(r"^#define SS_BLOCK %d\s" % B, src, flags=re.M) and "gsr_div_up(a.T, SS_BLOCK)" in src
    for name, blocks in cases.MESH_BLOCKS.items():
        v, t, s = cases.MESHES[name]
        ns = np.array([truth.triangle_n(v[a], v[b], v[c], s) for a, b, c in t])
        assert -(-len(t) // B) == blocks and (blocks > 1) == (len(t) > B), name
        sums = [int((ns[k * B:(k + 1) * B] ** 2).sum()) for k in range(blocks)]
        prefix = np.cumsum([0] + sums)
        p = truth.sample_surface(v, t, s)
        assert len(p) == prefix[-1] and min(sums) >= 1, name
        for k in range(1, blocks):                                              # sample prefix[k] exists and is the first of block k's first triangle
            assert prefix[k] < len(p) and np.array_equal(p[prefix[k]], truth.sample_surface(v, t[k * B:k * B + 1], s)[0]), (name, k)
            assert not np.array_equal(p[prefix[k]], p[prefix[k] - 1])
        if name == "T2048_uneven":
            assert (ns[:B] == 1).all() and ns[B:].min() >= 5 and sums[0] == B and sums[1] >= 25 * B
    assert len(truth.sample_surface(*cases.MESHES["T3077"])) == 33324


def test_samples_are_sub_triangle_centroids_of_equal_weight():
    v, t, s = cases.MESHES["n17"]
    p = truth.sample_surface(v, t, s).astype(np.float64)
    a, b, c = v[t[0]].astype(np.float64)
    assert len(p) == 17 * 17 and np.allclose(p.mean(axis=0), (a + b + c) / 3.0, rtol=0, atol=1e-5)      # equal weights reproduce the centroid
    M = np.stack([b - a, c - a], 1)
    uv = np.linalg.lstsq(M, (p - a).T, rcond=None)[0].T
    assert (uv > 1e-3).all() and (uv.sum(axis=1) < 1 - 1e-3).all()              # strictly inside: never on an edge


def test_thinning_by_hand():
    pts, cell = cases.VOXELS["negative"]
    kept, idx = truth.voxel_downsample(pts, cell)
    c = np.floor(pts.astype(np.float64) / cell)[:, 0]
    assert c.tolist() == [-1, -1, 0, -1, -2, 0]                                 # floor, not truncation: -0.5, -0.25 and -1.0 share cell -1; -0.0 is cell 0
    assert idx.tolist() == [0, 2, 4] and np.array_equal(kept, pts[idx])
    pts, cell = cases.VOXELS["on_multiples"]
    assert truth.voxel_downsample(pts, cell)[1].tolist() == [0, 2, 4, 5]        # 0.25 starts cell 1 and 0.26 shares it; 0.5 starts cell 2; 0.49999997 stays in cell 1
    assert truth.voxel_downsample(cases.VOXELS["one_cell"][0], 1.0)[1].tolist() == [0]
    pts, cell = cases.VOXELS["one_per_cell"]
    assert truth.voxel_downsample(pts, cell)[1].tolist() == list(range(len(pts))) and len(pts) == 48
    assert truth.voxel_downsample(*cases.VOXELS["nonfinite"])[1].tolist() == [0, 4]
    assert truth.voxel_downsample(*cases.VOXELS["edge_of_range"])[1].tolist() == [0, 1, 2]
    for bad in (cases.VOXEL_OUT_OF_RANGE, cases.VOXEL_JUST_OUT_OF_RANGE):
        with pytest.raises(ValueError, match="range"):
            truth.voxel_downsample(*bad)


def test_statistics_by_hand():
    pred = cases.a3([[0, 0, 0], [1, 0, 0], [5, 0, 0]])
    gt = cases.a3([[0, 0, 1], [1, 0, 1]])
    r = truth.surface_distance(pred, gt, thresholds=(1.0, 1.5))
    assert r["accuracy"] == math.fsum([1, 1, math.sqrt(17.0)]) / 3 and r["completeness"] == 1.0 and r["chamfer"] == 0.5 * (r["accuracy"] + 1.0)
    assert r["precision"] == [0.0, 2 / 3] and r["recall"] == [0.0, 1.0] and r["fscore"] == [0.0, 2 * (2 / 3) / (2 / 3 + 1)]      # d < tau is strict
    assert (r["n_pred"], r["n_gt"]) == (3, 2)
    r = truth.surface_distance(pred, gt, max_dist=2.0, thresholds=(1.5,))       # the far sample counts as max_dist
    assert r["accuracy"] == (1 + 1 + 2.0) / 3
    r = truth.surface_distance(pred[:0], gt, max_dist=2.0, thresholds=(1.5,))
    assert math.isnan(r["accuracy"]) and r["completeness"] == 2.0 and math.isnan(r["precision"][0]) and r["recall"] == [0.0] and r["n_pred"] == 0


# ---------------------------------------------------------------------------------------------------------------- the structure of the cases
def test_lattice_case_structure():
    q, t, _ = cases.NEAREST["lattice"]
    g = truth.grid_rule(t)
    assert g["h"] == 1.0 and g["inv_h"] == 1.0 and g["mn"].tolist() == [0, 0, 0] and g["n"].tolist() == [9, 9, 1] and g["dense"] and g["Tf"] == 64
    on_face = q[list(cases.Q_FACE)].astype(np.float64)
    assert ((on_face == np.floor(on_face)).sum(axis=1) >= 2).all()                # x (and y) on a face of the cells
    qd = q[cases.Q_DIAGONAL]
    d2, i = truth.nearest(q, t)
    own, diag = truth.cell_of(g, t[2]), truth.cell_of(g, t[3])
    assert truth.cell_of(g, qd).tolist() == own.tolist() == [3, 3, 0] and diag.tolist() == [2, 2, 0]
    assert abs(math.sqrt(truth.pair_d2(qd[None], t[2:3])[0, 0]) - 0.9) < 1e-3 and abs(math.sqrt(truth.pair_d2(qd[None], t[3:4])[0, 0]) - 0.2) < 5e-3
    assert i[cases.Q_DIAGONAL] == 3
    for k in cases.Q_SHELLS:
        shells = np.abs(truth.cell_of(g, t) - truth.cell_of(g, q[k])).max(axis=1)
        assert i[k] == 4 and shells[i[k]] >= 3 and shells.min() == shells[i[k]]   # nothing nearer in cells either: shells 0..2 are empty


def test_one_cell_and_flat_case_structure():
    for name, dims in (("one_cell_capped", [1, 1, 1]), ("one_cell_pair", [1, 1, 1]), ("flat_three_axes", [1, 1, 1])):
        q, t, m = cases.NEAREST[name]
        assert truth.grid_rule(t, m)["n"].tolist() == dims, name
    g = truth.grid_rule(*cases.NEAREST["flat_one_axis"][1:])
    assert g["n"][2] == 1 and g["n"][0] > 4 and g["n"][1] > 4
    g = truth.grid_rule(*cases.NEAREST["flat_two_axes"][1:])
    assert g["n"][1] == 1 and g["n"][2] == 1 and 100 < g["n"][0] <= 151         # a line: about one target per cell
    assert (truth.nearest(*cases.NEAREST["flat_three_axes"])[1] == 0).all()     # 40 copies of one point: the first wins


def test_two_clusters_force_the_sparse_table():
    q, t, _ = cases.NEAREST["two_clusters"]
    g = truth.grid_rule(t)
    c = truth.cell_of(g, t)
    assert not g["dense"] and g["n"][0] > 100000 and g["n"][1] == 1 and g["n"][2] == 1
    assert c[100:, 0].min() - c[:100, 0].max() >= 99000 and abs(g["h"] - 0.01) < 1e-4
    mid = truth.cell_of(g, q[29])                                              # (500, 0, 0)
    assert np.abs(c - mid).max(axis=1).min() > truth.RINGS                     # its shells run out: the box scan answers


@pytest.mark.parametrize("name,cells,chunks", [("ring_400", 21, 2), ("ring_1024", 33, 4)])
def test_rings_leave_the_dense_table_for_the_box_scan(name, cells, chunks):
    """k_np_query walks shells 0..CF_RINGS of the dense table and then falls back to cf_box_scan: the queries named in Q_RING_FAR find every one of
    those shells empty, the rim queries are answered inside them."""
    src = open(os.path.join(CSRC, "gsr_chamfer.hip")).read()
    assert re.search(r"^#define CF_RINGS %d\s" % truth.RINGS, src, flags=re.M) and re.search(r"^#define CF_CHUNK 256\s", src, flags=re.M)
    q, t, m = cases.NEAREST[name]
    assert m is None and q is cases.RING_QUERIES
    g = truth.grid_rule(t)
    assert g["dense"] and g["n"].tolist() == [cells, cells, 1] and -(-g["Tf"] // 256) == chunks
    c = truth.cell_of(g, t)
    shell = lambda k: int(np.abs(c - truth.cell_of(g, q[k])).max(axis=1).min())
    for k in cases.Q_RING_FAR[name]:
        assert shell(k) > truth.RINGS, (name, k, shell(k))
        assert truth.RINGS + 1 <= truth.cell_of(g, q[k])[0] < cells - truth.RINGS - 1         # the grid goes on beyond the last shell: the walk does not end for lack of cells
    assert cases.Q_RING_CENTRE in cases.Q_RING_FAR[name]
    for k in cases.Q_RING_RIM:
        assert shell(k) <= truth.RINGS, (name, k, shell(k))
    d = truth.pair_d2(q[cases.Q_RING_CENTRE][None], t)[0]
    d2, i = truth.nearest(q, t)
    assert (d == d.min()).sum() >= 2 and d2[cases.Q_RING_CENTRE] == d.min() and i[cases.Q_RING_CENTRE] == np.flatnonzero(d == d.min())[0]
    assert np.abs(d.astype(np.float64) - 1.0).max() <= 4 * 2.0 ** -24 and len(np.unique(d)) >= 2     # every target within a few ulps of d2 = 1, not all equal
    assert (i >= 0).all()


def test_far_and_cap_case_structure():
    q, t, _ = cases.NEAREST["far_query"]
    g = truth.grid_rule(t)
    inside = ((q.astype(np.float64) >= g["mn"]) & (q.astype(np.float64) <= g["mn"] + g["h"] * g["n"])).all(axis=1)
    assert not inside.any() and g["n"].min() > truth.RINGS + 2
    d2, i = truth.nearest(q, t)
    assert (i >= 0).all() and np.isfinite(d2).all() and d2[2] > 1e29
    assert truth.nearest(*cases.NEAREST["far_query_capped"])[1].tolist() == [-1, -1, -1, -1, int(i[4])]
    assert truth.nearest(*cases.NEAREST["cap_equal"])[1].tolist() == [0] and truth.nearest(*cases.NEAREST["cap_equal"])[0].tolist() == [25.0]
    assert truth.md2_of(cases.NEAREST["cap_one_ulp_less"][2]) < 25.0 and truth.nearest(*cases.NEAREST["cap_one_ulp_less"])[1].tolist() == [-1]


def test_tie_offset_and_density_case_structure():
    assert truth.nearest(*cases.NEAREST["equal_d2"])[1].tolist() == [0] and truth.nearest(*cases.NEAREST["equal_d2_reversed"])[1].tolist() == [0]
    q, t, _ = cases.NEAREST["equal_d2"]
    assert (truth.pair_d2(q, t) == 9.0).all() and len({tuple(r) for r in t.tolist()}) == 5
    g = truth.grid_rule(t)
    assert len({tuple(r) for r in truth.cell_of(g, t).tolist()}) >= 3           # the tied targets sit in different cells
    assert (truth.nearest(*cases.NEAREST["duplicates"])[1] < 20).all()
    q, t, _ = cases.NEAREST["offset_1e4"]
    g = truth.grid_rule(t)
    assert g["h"] < 4 * float(np.spacing(F(1e4))) and len(np.unique(t[:, 0])) < 30      # cells of a few ulps: a float32 cell index would merge them
    qc, tc = cases.big("clustered")
    dense_part = ((tc >= 0.3) & (tc <= 0.3 + 0.01 ** (1 / 3))).all(axis=1)
    assert 100 <= dense_part.sum() / 0.01 / ((~dense_part).sum() / 0.99) <= 103 and len(tc) == len(qc) == 20000


def test_nonfinite_case_structure():
    q, t, _ = cases.NEAREST["nonfinite"]
    d2, i = truth.nearest(q, t)
    bad_t = np.flatnonzero(~np.isfinite(t).all(axis=1))
    assert bad_t.tolist() == [3, 10, 11, 40] and not np.isin(i, bad_t).any()
    assert i[[0, 5, 6]].tolist() == [-1, -1, -1] and i[7] == 12 and d2[7] == 0
    assert (truth.nearest(*cases.NEAREST["nonfinite_targets_only"])[1] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- the binding, without a GPU
NAMES = ["gsr_nearest_points_scratch_bytes", "gsr_nearest_points", "gsr_sample_surface_scratch_bytes", "gsr_sample_surface_count", "gsr_sample_surface_emit",
         "gsr_voxel_downsample_scratch_bytes", "gsr_voxel_downsample_count", "gsr_voxel_downsample_emit", "gsr_distance_stats_scratch_bytes", "gsr_distance_stats"]


def test_library_exports_the_entry_points_and_the_abi_stays_8():
    import gsrast
    L = gsrast.lib()
    assert L.gsr_abi_version() == 8 == gsrast.ABI_VERSION
    for name in NAMES:
        assert name in gsrast.EXPORTS and getattr(L, name).argtypes is not None, name
    assert gsrast.nearest_points is gsrast.chamfer.nearest_points and gsrast.surface_distance is gsrast.chamfer.surface_distance
    assert gsrast.sample_surface is gsrast.chamfer.sample_surface and gsrast.voxel_downsample is gsrast.chamfer.voxel_downsample


def test_constants_equal_the_header():
    import abi_header as H
    from gsrast import chamfer
    c = H.constants(H.source("gsrast.h"))
    assert (chamfer.ERR_INDEX, chamfer.ERR_CAP, chamfer.ERR_RANGE) == (c["GSR_CHAMFER_ERR_INDEX"], c["GSR_CHAMFER_ERR_CAP"], c["GSR_CHAMFER_ERR_RANGE"])
    assert chamfer.MAX_N == c["GSR_SAMPLE_MAX_N"] == truth.MAX_N and chamfer.MAX_THRESHOLDS == c["GSR_CHAMFER_MAX_THRESHOLDS"]
    assert chamfer.CELL_RANGE == truth.CELL_RANGE


def test_scratch_queries_and_host_side_refusals():
    """What the library answers before it touches a device: sizes, and the argument errors of every entry point."""
    import ctypes as C
    import gsrast
    L = gsrast.lib()
    assert L.gsr_nearest_points_scratch_bytes(10, 1 << 31) == 0 and L.gsr_nearest_points_scratch_bytes(-1, 5) == 0
    small, large = L.gsr_nearest_points_scratch_bytes(1000, 1000), L.gsr_nearest_points_scratch_bytes(1000, 1000000)
    assert 0 < small < large and large / 1000000 < 96                           # under 96 bytes per target
    assert L.gsr_nearest_points_scratch_bytes(10, 0) > 0 and L.gsr_sample_surface_scratch_bytes(0) > 0
    assert L.gsr_sample_surface_scratch_bytes(1 << 31) == 0 and L.gsr_voxel_downsample_scratch_bytes(-1) == 0 and L.gsr_distance_stats_scratch_bytes(1 << 31) == 0
    assert 0 < L.gsr_voxel_downsample_scratch_bytes(1000000) / 1000000 < 48
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    for refused, word in ((lambda: L.gsr_nearest_points(p, 1 << 31, p, 1, -1.0, p, p, p, 4096, None), "out of range"),
                          (lambda: L.gsr_nearest_points(p, 1, p, 1, float("nan"), p, p, p, 4096, None), "NaN"),
                          (lambda: L.gsr_nearest_points(None, 1, p, 1, -1.0, p, p, p, 4096, None), "null"),
                          (lambda: L.gsr_nearest_points(p, 1, p, 1, -1.0, p, p, p, 16, None), "scratch too small"),
                          (lambda: L.gsr_sample_surface_count(p, 3, p, 1, 0.0, p, 4096, p, None), "spacing"),
                          (lambda: L.gsr_sample_surface_count(p, 3, p, 1, float("inf"), p, 4096, p, None), "spacing"),
                          (lambda: L.gsr_sample_surface_count(p, 3, p, 1, 1.0, p, 4096, None, None), "null record"),
                          (lambda: L.gsr_sample_surface_emit(p, 3, p, 1, 1.0, p, 4096, 1 << 31, p, None), "2\\^31"),
                          (lambda: L.gsr_voxel_downsample_count(p, 1, -1.0, p, 4096, p, None), "cell size"),
                          (lambda: L.gsr_voxel_downsample_emit(p, 4, p, 4096, 5, p, p, None), "out of range"),
                          (lambda: L.gsr_distance_stats(p, 1, -1.0, None, 9, p, p, 1 << 20, None), "thresholds"),
                          (lambda: L.gsr_distance_stats(p, 1, float("nan"), None, 0, p, p, 1 << 20, None), "NaN")):
        assert refused() == 1
        assert re.search(word, gsrast.last_error()), (word, gsrast.last_error())


def test_python_argument_errors():
    import torch
    from gsrast import chamfer
    pts = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        chamfer.nearest_points(pts, pts)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        chamfer.voxel_downsample(pts, 1.0)

    class Mesh:
        vertices, triangles = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        chamfer.sample_surface(Mesh(), 1.0)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spacing"):
            chamfer.sample_surface(Mesh(), s)
        with pytest.raises(ValueError, match="cell"):
            chamfer.voxel_downsample(pts, s)
    for m in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            chamfer.nearest_points(pts, pts, max_dist=m)
    with pytest.raises(ValueError, match="spacing is required"):
        chamfer.surface_distance(Mesh(), pts)
    with pytest.raises(ValueError, match="thresholds"):
        chamfer.surface_distance(pts, pts, thresholds=range(9))
    with pytest.raises(RuntimeError, match="shape"):
        chamfer.nearest_points(torch.zeros((4, 2)), pts)
