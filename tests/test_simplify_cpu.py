"""CPU tests of the mesh simplification: by-hand results of tests/simplify_truth.py, the truth against an independent dict-of-cells restatement,
the structure of the named cases of tests/simplify_cases.py (each has what it is named for, and meets the truth's conditions under the quadric
contraction), the header's constants against gsrast.mesh, the binding, and the refusals that need no device."""
import math
import os
import re

import numpy as np
import pytest

import simplify_cases as cases
import simplify_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gsr_mesh_simplify_scratch_bytes", "gsr_mesh_simplify_count", "gsr_mesh_simplify_emit"]


# ---------------------------------------------------------------------------------------------------------------- the truth, by hand
def test_two_triangles_in_one_cell_leave_one_vertex_and_no_triangle():
    v, c, t, vs = cases.CASES["two_in_one_cell"]
    out = truth.simplify(v, c, t, vs)
    assert out["record"] == (0, 1, 0, 0) and out["triangles"].shape == (0, 3) and out["vertex_map"].tolist() == [0, 0, 0, 0]
    want = np.array([[(0 + 0.1 + 0 + 0.1) / 4, (0 + 0 + 0.1 + 0.1) / 4, 0.05 / 4]], dtype=np.float64)
    assert np.abs(out["vertices"] - want).max() < 1e-7
    assert np.abs(out["colors"][0] - c.astype(np.float64).mean(0)).max() < 1e-7


def test_every_vertex_alone_comes_back_bit_for_bit():
    v, c, t, vs = cases.CASES["alone"]
    out = truth.simplify(v, c, t, vs)
    assert out["vertices"].tobytes() == v.tobytes() and out["colors"].tobytes() == c.tobytes()
    assert out["vertex_map"].tolist() == list(range(len(v))) and out["members"] == 1
    base = cases.grid_triangles(9, 7)                     # the sheet's own triangles come first and are distinct: they stay, rotated; the copies go
    assert len(out["triangles"]) == len(base)
    for got, src in zip(out["triangles"].tolist(), base.tolist()):
        k = src.index(min(src))
        assert got == src[k:] + src[:k]


def test_fan_keeps_the_lowest_of_a_triple_and_both_orientations():
    v, c, t, vs = cases.CASES["fan"]
    out = truth.simplify(v, c, t, vs)
    assert out["vertex_map"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    # t0 (A,B,C) stays, t1 (A,C,B) its mirror stays, t2 / t5 repeat t0, t3 is degenerate, t4 repeats t1, t6 (A,B,D) stays, t7 (D,A,B) repeats t6
    assert out["triangles"].tolist() == [[0, 1, 2], [0, 2, 1], [0, 1, 3]]


def test_unreferenced_vertices_are_clustered_like_any_other():
    v, c, t, vs = cases.CASES["unreferenced"]
    out = truth.simplify(v, c, t, vs)
    referenced = np.zeros(len(v), bool)
    referenced[t.ravel()] = True
    vm = out["vertex_map"]
    assert not referenced[0] and vm[0] == 0               # the first vertex of all is unreferenced and defines the origin
    only_unref = set(vm[~referenced].tolist()) - set(vm[referenced].tolist())
    shared = set(vm[~referenced].tolist()) & set(vm[referenced].tolist())
    assert len(only_unref) >= 3 and len(shared) >= 2      # cells of their own, and cells shared with the sheet
    assert vm[-3] == vm[-2]                               # (9, 9, 5) and (9.1, 9.2, 5.1) share one
    p = int(vm[-2])
    assert np.array_equal(out["vertices"][p], ((v[-3].astype(np.float64) + v[-2].astype(np.float64)) / 2.0).astype(np.float32))


def test_cube_corner_goes_to_the_corner_by_hand():
    v, c, t, vs = cases.CASES["cube"]
    avg, quad = truth.simplify(v, c, t, vs, "average"), truth.simplify(v, c, t, vs, "quadric")
    corner0 = int(np.flatnonzero((v == 0).all(1))[0])
    corner1 = int(np.flatnonzero((v == 1).all(1))[0])
    p0, p1 = int(avg["vertex_map"][corner0]), int(avg["vertex_map"][corner1])
    members = np.flatnonzero(avg["vertex_map"] == p0)
    assert len(members) == 7 and set(np.unique(v[members]).tolist()) == {0.0, 0.125}
    assert np.array_equal(avg["vertices"][p0], np.full(3, np.float32(3 * 0.125 / 7)))      # 3 of the 7 members have 0.125 on an axis
    assert quad["vertices"][p0].tolist() == [0.0, 0.0, 0.0] and quad["vertices"][p1].tolist() == [1.0, 1.0, 1.0]
    assert quad["record"] == (0, 26, 48, 8) and int(quad["quadric"].sum()) == 8             # the eight corner cells; edge and face cells fall back
    rest = ~quad["quadric"]
    assert np.array_equal(quad["vertices"][rest], avg["vertices"][rest]) and np.array_equal(quad["colors"], avg["colors"])
    assert np.array_equal(quad["triangles"], avg["triangles"])


def test_flat_sheet_falls_back_everywhere():
    v, c, t, vs = cases.CASES["flat_sheet"]
    avg, quad = cases.truth("flat_sheet", "average"), cases.truth("flat_sheet", "quadric")
    assert quad["record"][3] == 0 and quad["record"] == avg["record"]
    for k in ("vertices", "colors", "triangles", "vertex_map"):
        assert avg[k].tobytes() == quad[k].tobytes(), k


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_curved_shapes_mix_accepted_and_rejected_cells(name):
    q = cases.truth(name, "quadric")
    n, took = q["record"][1], q["record"][3]
    print(f"{name}: {n} cells, {took} took the quadric position")
    assert 0 < took < n and n - took >= 10
    v, _, _, vs = cases.CASES[name]
    o, cells = truth.cells_of(v, vs)
    first = {}
    for i, cell in enumerate(cells):
        first.setdefault(cell, i)
    cell_of_new = sorted(first, key=first.get)
    for p in np.flatnonzero(q["quadric"])[:200]:          # an accepted position lies in its cell's closed box, up to the float32 rounding
        x = q["vertices"][p].astype(np.float64) - np.array(o)
        assert ((x >= np.array(cell_of_new[p]) * vs - 1e-6) & (x <= (np.array(cell_of_new[p]) + 1) * vs + 1e-6)).all()


# ---------------------------------------------------------------------------------------------------------------- an independent restatement
def _restated(v, c, t, vs):
    """Dict of cells, Python loops, numpy for the cells, math.fsum for the means: -> (vertex_map, mean positions float64, mean colours float64,
    sum of |x| per element, counts, triangles)."""
    lo = np.array([min(float(x) for x in v[:, a]) for a in range(3)])
    cell = np.floor((v.astype(np.float64) - (lo - vs / 2.0)) / vs).astype(np.int64)
    members = {}
    for i in range(len(v)):
        members.setdefault(tuple(cell[i]), []).append(i)
    order = sorted(members.values(), key=lambda m: m[0])
    vmap = np.empty(len(v), np.int64)
    for p, m in enumerate(order):
        vmap[m] = p
    both = np.concatenate([v, c], axis=1).astype(np.float64)
    mean = np.array([[math.fsum(both[m, k]) / len(m) for k in range(6)] for m in order])
    mag = np.array([[math.fsum(np.abs(both[m, k])) for k in range(6)] for m in order])
    count = np.array([len(m) for m in order])
    best = {}
    for i, tri in enumerate(t.tolist()):
        n = [int(vmap[x]) for x in tri]
        if len(set(n)) < 3:
            continue
        k = n.index(min(n))
        best.setdefault(tuple(n[k:] + n[:k]), i)
    tris = [key for key, _ in sorted(best.items(), key=lambda kv: kv[1])]
    return vmap, mean, mag, count, np.array(tris, dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_truth_against_the_restatement(name):
    """Cells, numbering and triangles must agree exactly.  The means: the sequential float64 sum of n terms differs from the exact sum by at most
    (n - 1) 2^-53 sum|x| to first order, and math.fsum is the exact sum rounded once, so before the division the two differ by at most n 2^-53 sum|x|;
    dividing by n (>= 1) does not widen that.  Both sides then round to float32: half a float32 ulp of the mean on top."""
    v, c, t, vs = cases.CASES[name]
    out = cases.truth(name, "average")
    vmap, mean, mag, count, tris = _restated(v, c, t, vs)
    assert np.array_equal(out["vertex_map"], vmap) and out["record"] == (0, len(mean), len(tris), 0) and out["members"] == count.max()
    assert np.array_equal(out["triangles"], tris)
    got = np.concatenate([out["vertices"], out["colors"]], axis=1).astype(np.float64)
    bound = count[:, None] * 2.0 ** -53 * mag + np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64) * 0.5000001
    assert (np.abs(got - mean) <= bound).all(), name


@pytest.mark.parametrize("mode", ["average", "quadric"])
def test_the_benchmark_baseline_is_the_definition(mode):
    """tools/bench_simplify.host_simplify, the vectorised numpy path the benchmark times and compares the device with, gives the truth's bits."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_simplify
    for name in sorted(cases.CASES):
        v, c, t, vs = cases.CASES[name]
        want = cases.truth(name, mode)
        got = bench_simplify.host_simplify(v, c, t, vs, mode)
        for g, k in zip(got[:4], ("vertices", "colors", "triangles", "vertex_map")):
            assert g.tobytes() == want[k].tobytes(), (name, k)
        assert got[4] == want["record"][3] and got[5] == want["members"], name


# ---------------------------------------------------------------------------------------------------------------- the structure of the cases
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_meets_the_conditions_of_the_quadric_truth(name):
    q = cases.truth(name, "quadric")                      # asserts inside: no x within 2^-30 voxel of a face, no exact-zero det of a non-flat cell
    a = cases.truth(name, "average")
    assert np.array_equal(q["vertex_map"], a["vertex_map"]) and np.array_equal(q["triangles"], a["triangles"]) and np.array_equal(q["colors"], a["colors"])
    rest = ~q["quadric"]
    assert np.array_equal(q["vertices"][rest], a["vertices"][rest])


def test_sizes_stand_at_the_edges():
    for n in cases.EDGES:
        assert len(cases.CASES[f"size_V{n}"][0]) == n and len(cases.CASES[f"size_T{n}"][2]) == n
        assert cases.truth(f"cells_{n}", "average")["record"][1] == n
    # the soups really carry degenerate triangles, equal triples and unreferenced vertices
    v, c, t, vs = cases.CASES["size_T1025"]
    out = cases.truth("size_T1025", "average")
    n = out["vertex_map"][t]
    degenerate = (n[:, 0] == n[:, 1]) | (n[:, 1] == n[:, 2]) | (n[:, 2] == n[:, 0])
    assert degenerate.sum() > 10 and out["record"][2] < len(t) - degenerate.sum()
    assert len(np.unique(cases.CASES["size_V1025"][2])) < 1025      # and unreferenced vertices
    assert out["members"] >= 3


@pytest.mark.parametrize("name", ["lattice", "lattice_negative", "lattice_1e4"])
def test_lattice_vertices_sit_on_cell_faces(name):
    v, c, t, vs = cases.CASES[name]
    o, cells = truth.cells_of(v, vs)
    rel = (v.astype(np.float64) - np.array(o)) / vs
    on_face = rel == np.floor(rel)
    assert on_face.any(axis=1).sum() > 100 and (np.array(cells)[on_face] == rel[on_face]).all()      # on a face: the cell above it
    base = cases.truth("lattice", "average")
    out = cases.truth(name, "average")
    assert np.array_equal(out["vertex_map"], base["vertex_map"]) and np.array_equal(out["triangles"], base["triangles"])
    shift = {"lattice": 0.0, "lattice_negative": -8.0, "lattice_1e4": 1.0e4}[name]
    assert np.array_equal(out["vertices"], (base["vertices"].astype(np.float64) + shift).astype(np.float32))      # dyadic: the shift is exact


@pytest.mark.parametrize("name,axis,least", [("strip_x_256", 0, 256), ("strip_x_65536", 0, 65536), ("strip_y_65536", 1, 65536), ("strip_z_65536", 2, 65536)])
def test_strips_cross_the_digits_of_the_sort_key(name, axis, least):
    v, c, t, vs = cases.CASES[name]
    _, cells = truth.cells_of(v, vs)
    cc = np.array(cells)
    assert cc[:, axis].max() > least and cc[:, (axis + 1) % 3].max() == 1 and cc[:, (axis + 2) % 3].max() == 0
    key = cc[:, 0] | (cc[:, 1] << 21) | (cc[:, 2] << 42)
    lo_bit = 21 * axis
    for byte in range(lo_bit // 8, (lo_bit + (17 if least > 256 else 9)) // 8 + 1):      # every byte the axis reaches takes more than one value
        assert len(np.unique((key >> (8 * byte)) & 0xFF)) > 1, (name, byte)
    out = cases.truth(name, "average")
    assert 1 < out["members"] and out["record"][1] < len(v)      # some neighbouring columns share a cell


def test_the_three_long_strips_change_every_byte_of_the_key():
    seen = np.zeros(8, bool)
    for name in ("strip_x_65536", "strip_y_65536", "strip_z_65536"):
        v, _, _, vs = cases.CASES[name]
        cc = np.array(truth.cells_of(v, vs)[1])
        key = cc[:, 0] | (cc[:, 1] << 21) | (cc[:, 2] << 42)
        for byte in range(8):
            seen[byte] |= len(np.unique((key >> (8 * byte)) & 0xFF)) > 1
    assert seen.all()


def test_two_components_stay_two():
    v, c, t, vs = cases.CASES["two_components"]
    gap = v[144:].min(0)[0] - v[:144].max(0)[0]
    assert gap > 10 * vs
    out = cases.truth("two_components", "average")
    side = out["vertex_map"] >= out["vertex_map"][144]    # new vertices are numbered by their lowest member: the second sheet's come after the first's
    assert not side[:144].any() and side[144:].all()
    tri_side = out["triangles"] >= out["vertex_map"][144]
    assert (tri_side.all(1) | ~tri_side.any(1)).all() and tri_side.all(1).any() and (~tri_side.any(1)).any()      # no triangle bridges the gap


def test_error_inputs_raise_in_the_truth():
    want = {"nonfinite": truth.ERR_NONFINITE, "range": truth.ERR_RANGE, "index": truth.ERR_INDEX}
    for name, (v, c, t, vs, kind) in cases.errors().items():
        with pytest.raises(truth.SimplifyError) as e:
            truth.simplify(v, c, t, vs)
        assert e.value.status & want[kind], name
    v, c, t, _ = cases.CASES["alone"]
    span = np.array([(0, 0, 0), (2097150.5, 0, 0), (1, 1, 0)], dtype=np.float32)      # cells 0 .. 2^21 - 1: the last one that fits
    assert truth.simplify(span, c[:3], np.array([(0, 1, 2)]), 1.0)["record"] == (0, 3, 1, 0)


# ---------------------------------------------------------------------------------------------------------------- header, binding, refusals
def test_header_constants_match_gsrast_mesh():
    import abi_header
    from gsrast import mesh
    consts = abi_header.constants(abi_header.source("gsrast.h"))
    assert consts["GSR_SIMPLIFY_AVERAGE"] == mesh.SIMPLIFY_AVERAGE == mesh.CONTRACTIONS["average"] == 0
    assert consts["GSR_SIMPLIFY_QUADRIC"] == mesh.SIMPLIFY_QUADRIC == mesh.CONTRACTIONS["quadric"] == 1
    assert consts["GSR_MESH_ERR_RANGE"] == mesh.ERR_RANGE == truth.ERR_RANGE == 8
    assert consts["GSR_MESH_ERR_NONFINITE"] == mesh.ERR_NONFINITE == truth.ERR_NONFINITE == 16
    assert consts["GSR_MESH_ERR_INDEX"] == mesh.ERR_INDEX == truth.ERR_INDEX
    bits = [consts[k] for k in ("GSR_MESH_ERR_INDEX", "GSR_MESH_ERR_INTERNAL", "GSR_MESH_ERR_KEEP", "GSR_MESH_ERR_RANGE", "GSR_MESH_ERR_NONFINITE")]
    assert len(set(bits)) == 5 and all(b & (b - 1) == 0 for b in bits)
    assert mesh.CELL_LIMIT == truth.AXIS_CELLS == 1 << 21 and consts["GSR_ABI_VERSION"] == 8
    with open(os.path.join(ROOT, "gs-sr_amd", "csrc", "gsr_mesh_simplify.hip")) as f:
        src = f.read()
    assert re.search(r"#define MS_AXIS_BITS 21\b", src) and "2097152.0" in src


def test_library_exports_the_entry_points_and_the_abi_stays_8():
    import gsrast
    from gsrast import _abi
    L = gsrast.lib()
    assert L.gsr_abi_version() == 8 == gsrast.ABI_VERSION
    rows = {name for name, _, _ in _abi.FUNCTIONS}
    for name in NAMES:
        assert name in rows and name in gsrast.EXPORTS and getattr(L, name).argtypes is not None, name
    assert gsrast.simplify_vertex_clustering is gsrast.mesh.simplify_vertex_clustering
    assert callable(gsrast.tsdf.TriangleMesh.simplify_vertex_clustering)


def test_scratch_query_refuses_what_the_kernels_cannot_index():
    import gsrast
    L = gsrast.lib()
    q = L.gsr_mesh_simplify_scratch_bytes
    assert q(0, 0, 0) > 0 and q(1000, 600, 1) > q(1000, 600, 0) > 0
    assert q((1 << 31) // 3 + 1, 10, 0) == 0 and q(10, 1 << 31, 0) == 0 and q(-1, 10, 0) == 0 and q(10, -1, 1) == 0 and q(10, 10, 2) == 0
    assert q((1 << 31) // 3, (1 << 31) - 1, 1) > 0        # 3T = 2^31 - 2 and V = 2^31 - 1 are the last sizes that fit


def test_python_refusals_without_a_device():
    import torch
    from gsrast import mesh
    from gsrast.tsdf import TriangleMesh
    v, c, t, _ = cases.CASES["alone"]
    host = TriangleMesh(torch.from_numpy(v), torch.from_numpy(c), torch.from_numpy(t))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            mesh.simplify_vertex_clustering(host, bad)
    with pytest.raises(ValueError, match="contraction"):
        mesh.simplify_vertex_clustering(host, 0.5, contraction="median")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh.simplify_vertex_clustering(host, 0.5)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        host.simplify_vertex_clustering(0.5, "quadric")
