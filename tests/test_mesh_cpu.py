"""CPU checks of the TSDF mesh extraction's fixed parts (no GPU): the generated marching-cubes table, the numpy restatement of the mesh
(ref_mesh_numpy) on an analytic sphere, the PLY mesh container, and the C ABI's bookkeeping."""
import os
import re

import numpy as np
import torch

import ref_mesh_numpy as ref
from ref_mesh_numpy import gen_mc_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_matches_committed_header():
    assert open(gen_mc_table.HEADER).read() == gen_mc_table.header_text()
    t = ref.TABLE
    assert t.shape == (256, 16) and t[0, 15] == 0 and t[255, 15] == 0 and t[:, 15].max() == 5
    assert [int((t[:, 15] == k).sum()) for k in range(6)] == [2, 16, 50, 80, 76, 32]
    for row in t:
        n = int(row[15])
        assert (row[:3 * n] < 12).all() and (row[3 * n:15] == 255).all()
    assert gen_mc_table.EDGES == [(0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)]


def test_table_closes_a_random_field():
    """Every directed mesh edge of a random 12^3 field inside a positive border has its opposite exactly once: the cases agree across shared faces."""
    rng = np.random.default_rng(5)
    f = np.ones((12, 12, 12), np.float32)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (10, 10, 10)).astype(np.float32)
    v, c, t = ref.extract(f, np.ones_like(f), np.zeros(f.shape + (3,), np.float32), 1.0)
    top = ref.topology(t, len(v))
    assert len(t) > 500 and top["watertight"] and top["unused"] == 0


def test_single_corner_normals_point_away_from_the_corner():
    for i in range(8):
        f = np.ones((2, 2, 2), np.float32)
        o = gen_mc_table.CORNERS[i]
        f[o] = -1.0
        v, c, t = ref.extract(f, np.ones_like(f), np.zeros(f.shape + (3,), np.float32), 1.0)
        assert t.shape == (1, 3) and v.shape == (3, 3)
        p = v[t[0]].astype(np.float64)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        corner = np.array(o, np.float64) + 0.5
        assert np.dot(n, p.mean(axis=0) - corner) > 0, i


def test_reference_on_analytic_sphere():
    """Linear interpolation of a function whose second derivative along an edge is at most 1 / (r - h) is off by at most h^2 / (8 (r - h))."""
    n, h, centre, r = 32, 0.05, (0.8131, 0.7877, 0.8023), 0.41
    tsdf, w, col = ref.sphere(n, h, centre, r)
    v, c, t = ref.extract(tsdf, w, col, h)
    top = ref.topology(t, len(v))
    assert top["watertight"] and top["euler"] == 2 and top["unused"] == 0
    vol = ref.signed_volume(v, t)
    assert 0.97 < vol / (4.0 / 3.0 * np.pi * r ** 3) < 1.0
    dev = np.abs(np.linalg.norm(v.astype(np.float64) - np.array(centre), axis=1) - r).max()
    bound = h * h / (8 * (r - h))
    print(f"sphere: {len(v)} vertices, {len(t)} triangles, volume ratio {vol / (4.0 / 3.0 * np.pi * r ** 3):.4f}, deviation {dev:.3e} (bound {bound:.3e})")
    assert abs(bound - 8.68e-4) < 1e-6 and dev <= bound
    assert c.min() >= 0.0 and c.max() <= 1.0
    # the colour ramp is linear in space, so an interpolated colour is the ramp at the vertex
    assert np.abs(c - v / np.float32(n * h)).max() < 1e-5


def test_reference_does_not_depend_on_the_array_cut():
    """The same field given as a larger array with another origin: the same mesh (units order the output, not the array)."""
    rng = np.random.default_rng(2)
    f = rng.uniform(-1, 1, (20, 18, 17)).astype(np.float32)
    w = (rng.uniform(0, 1, f.shape) > 0.1).astype(np.float32)
    col = rng.uniform(0, 255, f.shape + (3,)).astype(np.float32)
    a = ref.extract(f, w, col, 0.02, origin=(-7, 3, 12))
    pad = ((5, 2), (1, 3), (0, 4))
    b = ref.extract(np.pad(f, pad), np.pad(w, pad), np.pad(col, pad + ((0, 0),)), 0.02, origin=(-12, 2, 12))
    assert len(a[2]) > 1000
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_a_row_cut_inside_a_run_of_fillers_gives_two_independent_meshes():
    """What the 4100-unit GPU test builds its truth on.  A filler unit (tsdf 0.5, weight 1) has no sign change inside it or against another filler, so
    no vertex and no triangle lies in a cube between two fillers: the mesh of the row is the mesh of the units up to a cut inside a run of fillers,
    followed by the mesh of the units behind a cut further on in the same run (vertices, colours and triangles in unit order; the second part's
    indices behind the first's).  12 units, field units at 0, 1, 8 and 11; cut after unit 3 and before unit 6."""
    rng = np.random.default_rng(21)
    fields = {u: ref.field_unit(rng) for u in (0, 1, 8, 11)}
    whole = ref.extract_row(fields, 0, 12, 0.02)
    first, second = ref.extract_row(fields, 0, 4, 0.02), ref.extract_row(fields, 6, 12, 0.02)
    assert len(first[2]) > 5000 and len(second[2]) > 5000 and second[0][:, 0].min() > 0.02 * 16 * 7 - 0.02 > first[0][:, 0].max()
    assert (whole[0][:, 0] > 0.02 * 16 * 2).any() and (second[0][:, 0] < 0.02 * 16 * 8).any()      # a surface inside the fillers next to a field unit
    for got, want in zip(ref.concat([first, second]), whole):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    again = ref.concat([first, ref.extract_row(fields, 4, 12, 0.02)])                         # wherever the run is cut
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, whole))
    # a cut next to a field unit is NOT free: the cubes across it are lost
    assert len(ref.concat([ref.extract_row(fields, 0, 8, 0.02), ref.extract_row(fields, 8, 12, 0.02)])[2]) < len(whole[2])


def test_the_grid_of_the_mesh_kernels_is_capped_at_4096_units():
    """k_tm_count and k_tm_emit run min(n_units, TM_GRID) workgroups that walk k = blockIdx.x, += gridDim.x: a workgroup stages a second unit only
    past TM_GRID units, which test_gpu_mesh.test_more_than_4096_units crosses with 4100."""
    import test_gpu_mesh as G
    src = open(os.path.join(ROOT, "gs-sr_amd", "csrc", "gsr_tsdf_mesh.hip")).read()
    assert re.search(r"^#define TM_GRID %d\s" % G.TM_GRID, src, flags=re.M)
    assert len(re.findall(r"for \(int k = blockIdx\.x; k < a\.n; k \+= gridDim\.x\)", src)) == 2
    assert len(re.findall(r"dim3\(\(uint32_t\)std::min\(n_units, TM_GRID\)\)", src)) == 2
    assert G.ROW_UNITS > G.TM_GRID and all(0 <= u < G.ROW_UNITS for u in G.ROW_FIELDS)
    assert {G.TM_GRID - 1, G.TM_GRID, 0, G.ROW_UNITS - 1} <= set(G.ROW_FIELDS)                 # either side of the turn and both ends


def test_ply_triangle_mesh_round_trip(tmp_path):
    from gsrast import ply
    from gsrast.tsdf import TriangleMesh
    rng = np.random.default_rng(0)
    m = TriangleMesh(torch.tensor(rng.normal(size=(7, 3)).astype(np.float32)), torch.tensor((rng.integers(0, 256, (7, 3)) / 255.0).astype(np.float32)),
                     torch.tensor(rng.integers(0, 7, (9, 3)).astype(np.int32)))
    path = str(tmp_path / "mesh.ply")
    ply.write_triangle_mesh(path, m)
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert head[3:] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
                        "element face 9", "property list uchar int vertex_indices", ""]
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 7 * 15 + 9 * 13
    r = ply.read_triangle_mesh(path)
    assert r.vertices.dtype == torch.float32 and r.triangles.dtype == torch.int32
    assert torch.equal(r.vertices, m.vertices) and torch.equal(r.triangles, m.triangles) and torch.equal(r.vertex_colors, m.vertex_colors)
    empty = TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    ply.write_triangle_mesh(path, empty)
    r = ply.read_triangle_mesh(path)
    assert tuple(r.vertices.shape) == (0, 3) and tuple(r.triangles.shape) == (0, 3) and r.cpu().triangles.dtype == torch.int32


def test_mesh_entry_points_in_header_exports_and_library():
    import ctypes as C
    import gsrast
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    L = gsrast.lib()
    for s in ("gsr_tsdf_sparse_mesh_scratch_bytes", "gsr_tsdf_sparse_mesh_count", "gsr_tsdf_sparse_mesh_emit"):
        assert re.search(r"\b" + s + r"\s*\(", src) and s in gsrast.EXPORTS and hasattr(L, s)
    assert re.search(r"#define GSR_ABI_VERSION 8\b", src) and gsrast.ABI_VERSION == 8 and L.gsr_abi_version() == 8
    # scratch besides the outputs: under 4 KB per unit (1/20 of a unit's record)
    assert L.gsr_tsdf_sparse_mesh_scratch_bytes(100000) < 4096 * 100000
    assert L.gsr_tsdf_sparse_mesh_scratch_bytes(1) < 4096
    # arguments are validated before anything is launched
    counts = (C.c_uint64 * 2)()
    assert L.gsr_tsdf_sparse_mesh_count(None, 1, None, 0.0, None, 0, counts, None) != 0 and "null volume" in gsrast.last_error()
