"""Named inputs of the gsrast.chamfer tests (numpy only).  NEAREST[name] = (query [Q,3], target [T,3], max_dist or None); the structure a case
rests on (which cell holds what under the documented cell rule) is asserted in test_chamfer_cpu.py."""
import numpy as np

F = np.float32
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _u(seed, n, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def a3(rows):
    return np.asarray(rows, F).reshape(-1, 3)


SIZES = (0, 1, 63, 64, 65, 257)


def lattice_targets():
    """64 targets in the plane z = 0 whose box is [0,8] x [0,8]: the cell rule gives h = sqrt(64 / 64) = 1 and faces on the integers.  Targets 2
    and 3 are the 0.9-cell / 0.2-cell pair around the query (3.05, 3.05); the fillers keep to x >= 5, target 4 = (5, 6.5) in front."""
    fill = np.random.default_rng(11).uniform([5.25, 0.0, 0.0], [8.0, 8.0, 0.0], (59, 3))
    return a3(np.concatenate([[[0, 0, 0], [8, 8, 0], [3.95, 3.05, 0], [2.9, 2.92, 0], [5.0, 6.5, 0]], fill]))


LATTICE_QUERIES = a3([[3.0, 2.5, 0], [3.0, 4.0, 0], [6.0, 6.0, 0], [8, 8, 0], [0, 0, 0],      # on a face, an edge, corners of cells
                      [3.05, 3.05, 0],                                                    # own cell 0.9 away, diagonal neighbour 0.2 away
                      [2.5, 6.5, 0], [1.5, 7.5, 0.25]])                                   # the nearest target is three shells away
Q_FACE, Q_DIAGONAL, Q_SHELLS = (0, 1, 2, 3, 4), 5, (6, 7)


def two_clusters():
    """200 targets in two clusters 1000 apart in x, 1e-5 wide in y and z: h = sqrt(2 * 1000 * 1e-5 / 200) = 0.01, the clusters 1e5 cells apart
    and the 1e5 cells beyond the dense table.  Queries at both, between them (the shells run out: box scan) and beside them."""
    r = np.random.default_rng(12)
    c = r.uniform([0, 0, 0], [0.05, 1e-5, 1e-5], (200, 3))
    c[100:, 0] += 1000.0
    c[0] = [0, 0, 0]; c[199] = [1000.05, 1e-5, 1e-5]
    q = np.concatenate([c[::7] + r.normal(0, 0.003, (29, 3)), [[500.0, 0, 0], [499.99, 0.3, -0.2], [250.0, 0, 0], [1000.2, 0, 0], [-0.2, 0, 0], [1000.02, 5e-6, 0]]])
    return a3(q), a3(c)


def ring(n):
    """n targets on the unit circle of the plane z = 0, (cos, sin, 0) of 2 pi k / n rounded to float32: the box is [-1,1] x [-1,1], the cell rule gives
    h = sqrt(4 / n) and floor(2 / h) + 1 cells along x and y -- a dense table whose middle is empty.  From the centre every target is within a few
    ulps of d2 = 1 and many d2 are equal: the lowest index among the smallest has to survive."""
    a = 2.0 * np.pi * np.arange(n) / n
    return a3(np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1))


RING_QUERIES = a3([[0, 0, 0], [0.05, -0.02, 0], [0.3, 0.1, 0],      # the centre and near it: the shells of the dense table run out, the box scan answers
                   [0.97, 0.05, 0], [-0.6, -0.78, 0]])             # just inside the rim: answered within the shells
Q_RING_CENTRE, Q_RING_RIM = 0, (3, 4)
Q_RING_FAR = {"ring_400": (0, 1), "ring_1024": (0, 1, 2)}          # the queries whose nearest target is more than CF_RINGS shells away


def _clustered(seed, n):
    """A 100:1 density contrast: half of the points in the unit cube, half in a cube of a hundredth of its volume."""
    r = np.random.default_rng(seed)
    side = 0.01 ** (1.0 / 3.0)
    return a3(np.concatenate([r.uniform(0, 1, (n // 2, 3)), 0.3 + r.uniform(0, side, (n - n // 2, 3))]))


def _nonfinite():
    t = _u(21, 80)
    t[3, 0] = NAN; t[10, 1] = INF; t[11, 2] = -INF; t[40] = NAN
    q = _u(22, 70)
    q[0, 0] = NAN; q[5, 2] = INF; q[6] = -INF
    q[7] = t[12]
    return q, t


def _build():
    c = {}
    for Q in SIZES:
        for T in SIZES:
            c[f"size_Q{Q}_T{T}"] = (_u(100 + Q, Q), _u(200 + T, T), None)
    c["one_cell_capped"] = (_u(1, 90, -0.5, 0.6), _u(2, 50, 0.0, 0.1), 1.0)                # max_dist clamps the cell to 1 >= the extent
    c["one_cell_pair"] = (_u(3, 40, -1, 2), a3([[0, 0, 0], [1, 1, 1]]), None)              # h = sqrt(3 / 2) > 1
    flat = _u(4, 150); flat[:, 2] = F(0.5)
    line = _u(5, 150); line[:, 1] = F(0.25); line[:, 2] = F(-2.0)
    c["flat_one_axis"] = (_u(6, 120, -0.2, 1.2), flat, None)
    c["flat_two_axes"] = (_u(7, 120, -0.2, 1.2), line, None)
    c["flat_three_axes"] = (_u(8, 50, -1, 1), np.tile(a3([[0.25, -0.5, 0.125]]), (40, 1)), None)
    c["lattice"] = (LATTICE_QUERIES, lattice_targets(), None)
    cube = _u(9, 500)
    far = a3([[100, 0.5, 0.5], [-1e6, 3, 7], [0.5, 0.5, 1e15], [1.5, 0.5, 0.5], [0.5, -0.01, 0.5]])
    c["far_query"] = (far, cube, None)
    c["far_query_capped"] = (far, cube, 0.5)
    five = a3([[0, 0, 0], [100, 100, 100]])
    c["cap_equal"] = (a3([[3, 4, 0]]), five, 5.0)                                          # d2 = 25 = 5 * 5: equality stays in
    c["cap_one_ulp_less"] = (a3([[3, 4, 0]]), five, float(np.nextafter(F(5), F(0))))
    base = _u(10, 20)
    c["duplicates"] = (_u(13, 64), np.concatenate([base, base, base]), None)
    ties = a3([[-3, 0, 0], [1, 2, 2], [2, 2, 1], [0, 0, 3], [2, 1, 2]])                     # every d2 from the origin is 9
    c["equal_d2"] = (a3([[0, 0, 0]]), ties, None)
    c["equal_d2_reversed"] = (a3([[0, 0, 0]]), ties[::-1].copy(), None)
    off = F(1e4)
    c["offset_1e4"] = (off + _u(14, 300, 0, 0.02), off + _u(15, 300, 0, 0.02), None)       # an ulp at 1e4 is 9.8e-4: a few ulps of structure
    c["two_clusters"] = two_clusters() + (None,)
    c["ring_400"] = (RING_QUERIES, ring(400), None)                                       # 21 x 21 x 1 cells, 2 chunks of the box scan
    c["ring_1024"] = (RING_QUERIES, ring(1024), None)                                     # 33 x 33 x 1 cells, 4 chunks
    q, t = _nonfinite()
    c["nonfinite"] = (q, t, None)
    c["nonfinite_capped"] = (q, t, 0.1)
    c["nonfinite_targets_only"] = (_u(16, 10), np.full((7, 3), NAN, F), None)
    return c


NEAREST = _build()
LAYOUT = ("size_Q63_T257", "duplicates", "flat_one_axis")       # run again in the three layouts of test_gpu_knn_edges.test_input_layout


def big(name):
    """The 20 000 x 20 000 inputs, built on demand: (query, target)."""
    if name == "uniform":
        return _u(31, 20000), _u(32, 20000)
    return _clustered(33, 20000), _clustered(34, 20000)


# ---- meshes: (vertices [V,3], triangles [T,3] int32, spacing)
def _mesh(v, t, s):
    return a3(v), np.asarray(t, np.int32).reshape(-1, 3), s


TRI = [[0, 0, 0], [3, 0, 0], [1.5, 1, 0]]                 # longest edge 3


def random_mesh(T, seed=41):
    r = np.random.default_rng(seed)
    return a3(r.uniform(-1, 1, (40, 3))), r.integers(0, 40, (T, 3)).astype(np.int32), 0.6


def uneven_mesh():
    """2048 triangles, spacing 0.6: the first 1024 inside a cube of edge 0.3 (n = 1, one sample each), the next 1024 with an edge from a cluster at
    x = +1.6 to one at x = -1.6 (n >= 5, 25 samples or more each): the sums of the two blocks of 1024 triangles differ by more than 25 times."""
    r = np.random.default_rng(43)
    v = np.concatenate([r.uniform(-0.15, 0.15, (20, 3)), r.uniform(-0.15, 0.15, (10, 3)) + [1.6, 0, 0], r.uniform(-0.15, 0.15, (10, 3)) - [1.6, 0, 0]])
    small = r.integers(0, 20, (1024, 3))
    wide = np.stack([r.integers(20, 30, 1024), r.integers(30, 40, 1024), r.integers(0, 40, 1024)], 1)
    return a3(v), np.concatenate([small, wide]).astype(np.int32), 0.6


SAMPLER_BLOCK = 1024                                      # csrc/gsr_chamfer.hip SS_BLOCK: triangles per workgroup of the count, one scanned sum each
MESHES = {
    "edge_exactly_3_spacings": _mesh(TRI, [[0, 1, 2]], 1.0),                                         # n = 3
    "edge_exactly_4_spacings": _mesh(TRI, [[0, 1, 2]], 0.75),                                        # n = 4
    "edge_one_ulp_above": _mesh([[0, 0, 0], [np.nextafter(F(3), F(4)), 0, 0], [1.5, 1, 0]], [[0, 1, 2]], 1.0),      # n = 4
    "zero_area": _mesh([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0, 1, 2]], 0.5),
    "all_equal": _mesh([[0.5, 0.25, -1]] * 3, [[0, 1, 2]], 0.1),                                     # n = 1
    "n1": _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], 2.0),
    "n2": _mesh([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0.5]], [[0, 1, 2]], 0.5),
    "n3": _mesh([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0.5]], [[2, 0, 1]], 1.0 / 3.0),
    "n17": _mesh([[0, 0, 0], [17, 0, 0], [3, 5, 1]], [[0, 1, 2]], 1.0),
    "T1": random_mesh(1),
    "T65": random_mesh(65),
    "T1023": random_mesh(1023),                                                                      # one block of the sampler, one short of full
    "T1024": random_mesh(1024),                                                                      # one full block
    "T1025": random_mesh(1025),                                                                      # a second block of one triangle
    "T3077": random_mesh(3077),                                                                      # four blocks, the last partial
    "T2048_uneven": uneven_mesh(),
    "two_triangles": _mesh([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]], 0.3),
}
MESH_BLOCKS = {"T1023": 1, "T1024": 1, "T1025": 2, "T3077": 4, "T2048_uneven": 2}
MESH_N = {"edge_exactly_3_spacings": 3, "edge_exactly_4_spacings": 4, "edge_one_ulp_above": 4, "all_equal": 1, "n1": 1, "n2": 2, "n3": 3, "n17": 17}
MESH_BAD_INDEX = _mesh(TRI, [[0, 1, 2], [0, 1, 3]], 1.0)
MESH_NEGATIVE_INDEX = _mesh(TRI, [[0, -1, 2]], 1.0)
MESH_ABOVE_CAP = _mesh([[0, 0, 0], [2000, 0, 0], [1, 1, 0]], [[0, 1, 2]], 1.0)           # n = 2000 > 1024


# ---- thinning: (points [N,3], cell)
def _one_per_cell():
    g = np.stack(np.meshgrid(np.arange(-2, 2), np.arange(-2, 2), np.arange(0, 3), indexing="ij"), -1).reshape(-1, 3)
    return a3((g + np.random.default_rng(51).uniform(0.1, 0.9, g.shape)) * 0.5)


VOXELS = {
    "negative": (a3([[-0.5, 0.5, 0.5], [-0.25, 0.25, 0.75], [0.5, 0.5, 0.5], [-1.0, 0.5, 0.5], [-1.5, 0.5, 0.5], [-0.0, 0.1, 0.1]]), 1.0),      # floor: -1, not 0
    "on_multiples": (a3([[0.25, 0.5, -0.25], [0.26, 0.6, -0.2], [0.5, 0.5, -0.25], [0.49999997, 0.5, -0.25], [-0.25, -0.5, 0], [0, 0, 0]]), 0.25),
    "one_cell": (_u(52, 65, 0.01, 0.99), 1.0),
    "one_per_cell": (_one_per_cell(), 0.5),
    "N1": (_u(53, 1), 0.1),
    "N65": (_u(54, 65, -1, 1), 0.4),
    "nonfinite": (a3([[0.1, 0.1, 0.1], [NAN, 0, 0], [0.2, 0.2, 0.2], [0, INF, 0], [5, 5, 5]]), 1.0),
    "edge_of_range": (a3([[-1048576.0, 0, 0], [1048575.5, 0, 0], [0, 0, 0]]), 1.0),
}
VOXEL_OUT_OF_RANGE = (a3([[0, 0, 0], [1.0e7, 0, 0]]), 1.0)
VOXEL_JUST_OUT_OF_RANGE = (a3([[0, 0, 1048576.0]]), 1.0)
