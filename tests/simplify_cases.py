"""Named inputs for the tests of gsrast.mesh.simplify_vertex_clustering: CASES[name] = (vertices float32 [V,3], colors float32 [V,3], triangles int32
[T,3], voxel_size).  Every case is small enough that a GPU run takes well under a second; the strips that cross 65 536 cells carry 52 000 vertices
because the crossing needs them.  tests/test_simplify_cpu.py checks that each case has the structure it is named for, and that every case meets
the conditions of tests/simplify_truth.py under contraction="quadric"."""
import functools

import numpy as np

EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def _colors(n, seed):
    return np.random.default_rng(1000 + seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def _pack(v, t, voxel, seed=0):
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    return v, _colors(len(v), seed), np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3), float(voxel)


def grid_triangles(nu, nv, wrap_u=False, wrap_v=False):
    """Two triangles per quad of an nu x nv vertex grid, vertex (i, j) = i * nv + j; wrapping welds the last row / column to the first."""
    t = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            a, b = i * nv + j, i * nv + (j + 1) % nv
            c, d = ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
            t += [(a, c, b), (b, c, d)]
    return np.array(t, dtype=np.int32).reshape(-1, 3)


def soup(V, T, seed, side=4.0, voxel=0.5):
    """V random vertices in a cube and T random index triples: degenerate triangles, equal triples and unreferenced vertices all occur."""
    r = np.random.default_rng(seed)
    return _pack(r.uniform(-side / 2, side / 2, (V, 3)), r.integers(0, V, (T, 3)), voxel, seed)


def occupied(n_cells, seed):
    """Exactly n_cells occupied cells: cell k of a 3-d walk gets 1 to 3 vertices well inside it, shuffled; triangles at random."""
    r = np.random.default_rng(seed)
    k = np.arange(n_cells)
    cell = np.stack([k % 37, (k // 37) % 29, k // (37 * 29)], axis=1).astype(np.float64)
    reps = r.integers(1, 4, n_cells)
    which = np.repeat(k, reps)
    # vertex 0 of cell 0 sits at (0, 0, 0) and is the minimum on every axis: origin = -voxel / 2 and cell j covers [(j - 0.5), (j + 0.5)) voxels.  Every
    # other vertex lies at least 0.1 of a cell inside its cell, and not below 0 where its cell index is 0.
    inside = np.where(cell[which] == 0.0, r.uniform(0.5, 0.9, (len(which), 3)), r.uniform(0.1, 0.9, (len(which), 3)))
    v = (cell[which] + inside - 0.5) * 0.25
    v[0] = 0.0
    perm = r.permutation(len(which))
    v, which = v[perm], which[perm]
    T = 2 * len(v) + 1
    return _pack(v, r.integers(0, len(v), (T, 3)), 0.25, seed), which


def two_in_one_cell():
    v = [(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (0.1, 0.1, 0.05)]
    return _pack(v, [(0, 1, 2), (1, 3, 2)], 1.0)


def alone():
    """A 9 x 7 sheet with unit spacing and a voxel of 0.5: every vertex alone in its cell."""
    i, j = np.meshgrid(np.arange(9), np.arange(7), indexing="ij")
    v = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, 0.25 * np.sin(i.ravel() + 2.0 * j.ravel())], axis=1)
    t = grid_triangles(9, 7)
    t = np.concatenate([t, t[::3, [1, 2, 0]], t[1::4, [2, 0, 1]]])      # some start with another corner: they come back rotated, duplicates go
    return _pack(v, t, 0.5, 3)


def fan():
    """Three cells A, B, C (+ a fourth, D) with several vertices each.  Triangles 0, 2, 5 collapse to the triple (A, B, C) in its three rotations: the
    lowest stays.  Triangles 1 and 4 collapse to its mirror (A, C, B): another triple, the lower one stays.  Triangle 3 is degenerate (two corners in A)."""
    A, B, C, D = (0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2)
    off = [(0.0, 0.0, 0.0), (0.2, 0.1, 0.0), (0.1, 0.3, 0.2)]
    v = [(c[0] + o[0], c[1] + o[1], c[2] + o[2]) for c in (A, B, C, D) for o in off]      # vertex 3 k + m: cell k, member m
    a, b, c, d = 0, 3, 6, 9
    t = [(a, b, c), (a + 1, c + 1, b + 1), (b + 2, c, a + 2), (a, a + 1, b), (c + 2, b, a), (c + 1, a + 1, b + 2), (a, b, d), (d + 1, a + 2, b + 1)]
    return _pack(v, t, 1.0, 4)


def unreferenced():
    """A 6 x 6 sheet (voxel = 2 spacings) plus unreferenced vertices: some inside cells of the sheet, some in cells of their own, one first of all."""
    i, j = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    sheet = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, np.zeros(36)], axis=1)
    extra = np.array([(-3.0, -3.0, -1.0), (0.3, 0.4, 0.1), (2.6, 2.7, 0.2), (9.0, 9.0, 5.0), (9.1, 9.2, 5.1), (2.5, 8.0, 3.0)])
    v = np.concatenate([extra[:1], sheet, extra[1:]])
    return _pack(v, grid_triangles(6, 6) + 1, 2.0, 5)


def lattice(shift):
    """7 x 7 x 3 vertices at multiples of 0.25 under a voxel of 0.5: origin = lo - 0.25, so every vertex with an odd multiple sits exactly ON a cell
    face and belongs to the cell above it (floor).  Everything is dyadic, at shift 0, -8 and 1e4 alike."""
    i, j, k = np.meshgrid(np.arange(7), np.arange(7), np.arange(3), indexing="ij")
    v = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) * 0.25 + shift
    t = np.concatenate([grid_triangles(7, 7) * 3 + k for k in range(3)])      # three sheets, vertex (i, j, k) = (i * 7 + j) * 3 + k
    return _pack(v, t, 0.5, 6)


def strip(axis, columns, seed):
    """A two-row strip along `axis`: column steps of 0.5 .. 0.9 or 3 .. 4 voxels at random (neighbouring columns sometimes share a cell), rows 1.3
    voxels apart.  The voxel is not dyadic: far out a float32 coordinate is a multiple of 2^-10 and would sit exactly on the faces of a dyadic lattice."""
    r = np.random.default_rng(seed)
    u = r.uniform(size=columns - 1)
    along = np.concatenate([[0.0], np.cumsum(np.where(u < 0.3, r.uniform(0.5, 0.9, columns - 1), r.uniform(3.0, 4.0, columns - 1)))])
    v = np.zeros((columns, 2, 3))
    v[:, :, axis] = along[:, None]
    v[:, 1, (axis + 1) % 3] = 1.3
    v[:, :, (axis + 2) % 3] = r.uniform(0.0, 0.3, (columns, 2))
    return _pack(v.reshape(-1, 3) * 0.1237, grid_triangles(columns, 2), 0.1237, seed)


def two_components():
    """Two 12 x 12 sheets 40 units apart; voxel = 2 spacings, far below the gap."""
    i, j = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    a = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, 0.3 * np.cos(0.7 * i.ravel())], axis=1)
    t = grid_triangles(12, 12)
    return _pack(np.concatenate([a, a + (40.0, 3.0, 1.0)]), np.concatenate([t, t + 144]), 2.0, 7)


def cube():
    """The surface of [0, 1]^3, 8 x 8 quads per face, welded; voxel 0.5 -> origin -0.25: the cell of corner (0, 0, 0) holds the seven surface vertices
    with coordinates in {0, 0.125}.  Everything is dyadic: the three face planes meet in (0, 0, 0) exactly, the average is (3/7 * 0.125, ...)."""
    n = 8
    index, v, t = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(v)
            v.append(p)
        return index[p]
    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, i + di, j + dj
                        q.append(vid(tuple(p)))
                    if side == 0:
                        q = q[::-1]                       # outward orientation
                    t += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return _pack(np.array(v, dtype=np.float64) / n, t, 0.5, 8)


def flat_sheet():
    """A 40 x 40 sheet in the plane z = 0.75, jittered inside the plane: every normal is (0, 0, +-1) exactly, every cell's determinant an exact 0."""
    r = np.random.default_rng(9)
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    v = np.stack([i.ravel() + r.uniform(-0.3, 0.3, 1600), j.ravel() + r.uniform(-0.3, 0.3, 1600), np.full(1600, 0.75)], axis=1)
    return _pack(v, grid_triangles(40, 40), 3.0, 9)


def sphere(seed=10):
    """A UV sphere, 100 rings x 200 segments, welded around, jittered: ~20 000 vertices; the voxel is about three edge lengths."""
    r = np.random.default_rng(seed)
    th, ph = np.meshgrid(np.pi * (np.arange(100) + 0.5) / 100, 2 * np.pi * np.arange(200) / 200, indexing="ij")
    rad = 1.0 + r.normal(0.0, 0.004, th.shape)
    v = np.stack([rad * np.sin(th) * np.cos(ph), rad * np.sin(th) * np.sin(ph), rad * np.cos(th)], axis=-1).reshape(-1, 3)
    return _pack(v, grid_triangles(100, 200, wrap_v=True), 0.1, seed)


def torus(seed=11):
    """A torus (R = 1, r = 0.35), 200 x 100, welded both ways, jittered: 20 000 vertices, cells on convex and saddle regions."""
    r = np.random.default_rng(seed)
    u, w = np.meshgrid(2 * np.pi * np.arange(200) / 200, 2 * np.pi * np.arange(100) / 100, indexing="ij")
    rr = 0.35 + r.normal(0.0, 0.003, u.shape)
    v = np.stack([(1.0 + rr * np.cos(w)) * np.cos(u), (1.0 + rr * np.cos(w)) * np.sin(u), rr * np.sin(w)], axis=-1).reshape(-1, 3)
    return _pack(v, grid_triangles(200, 100, wrap_u=True, wrap_v=True), 0.09, seed)


@functools.lru_cache(maxsize=None)
def _all():
    c = {"two_in_one_cell": two_in_one_cell(), "alone": alone(), "fan": fan(), "unreferenced": unreferenced(),
         "lattice": lattice(0.0), "lattice_negative": lattice(-8.0), "lattice_1e4": lattice(1.0e4),
         "strip_x_256": strip(0, 150, 20), "strip_x_65536": strip(0, 26000, 21), "strip_y_65536": strip(1, 26000, 22), "strip_z_65536": strip(2, 26000, 23),
         "two_components": two_components(), "cube": cube(), "flat_sheet": flat_sheet(), "sphere": sphere(), "torus": torus(),
         "no_triangles": _pack(np.random.default_rng(30).uniform(0, 3, (300, 3)), np.zeros((0, 3)), 0.5, 30)}
    for n in EDGES:
        c[f"size_V{n}"] = soup(n, 2 * n + 3, 100 + n, side=4.0, voxel=0.5 if n > 1 else 1.0)
        c[f"size_T{n}"] = soup(90, n, 200 + n + RESEED.get(f"size_T{n}", 0), side=3.0, voxel=0.75)
        c[f"cells_{n}"] = occupied(n, 300 + n + RESEED.get(f"cells_{n}", 0))[0]
    return c


# The first seed of these cases gives a cell whose quadric minimiser lies ON a face of its box (x = 0 of a one-triangle cell, say), which the conditions
# of simplify_truth.py rule out: the next seed in line does not.  test_simplify_cpu.py checks every case against the conditions.
RESEED = {"size_T63": 5000, "size_T65": 5000, "cells_257": 5000, "cells_1024": 5000}


CASES = _all()
QUADRIC_SHAPES = ("cube", "flat_sheet", "sphere", "torus")


@functools.lru_cache(maxsize=None)
def truth(name, contraction):
    """The truth of a case, computed once and shared; the arrays are not to be modified."""
    import simplify_truth
    out = simplify_truth.simplify(*CASES[name], contraction=contraction)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def errors():
    """name -> (vertices, colors, triangles, voxel_size, the status bit or exception the call must raise)."""
    v, c, t, _ = CASES["alone"]
    nan, inf, far = v.copy(), v.copy(), v.copy()
    nan[17, 1] = np.nan
    inf[40, 2] = -np.inf
    far[5, 0] = 3.0e6                                     # extent / voxel = 2^21 * 1.43 with voxel 1
    bad = t.copy()
    bad[7, 2] = len(v)
    neg = t.copy()
    neg[0, 0] = -1
    edge = np.array([(0, 0, 0), (2097151.5, 0, 0), (1, 1, 0)], dtype=np.float32)      # cells 0 .. 2^21: one too many (origin = -0.5)
    return {"nan": (nan, c, t, 0.5, "nonfinite"), "inf": (inf, c, t, 0.5, "nonfinite"), "range": (far, c, t, 1.0, "range"),
            "range_edge": (edge, c[:3], np.array([(0, 1, 2)], np.int32), 1.0, "range"),
            "index": (v, c, bad, 0.5, "index"), "index_negative": (v, c, neg, 0.5, "index")}
