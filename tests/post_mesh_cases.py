"""Meshes for the mesh filter's tests (test_post_mesh_cpu.py checks the numpy restatement against the hand-written answers, test_gpu_post_mesh.py
the device against both).  Plain numpy: vertices / colours float32 [V,3], triangles int32 [T,3]."""
import numpy as np


def strip(n, v0=0):
    """n triangles (v0 + i, v0 + i + 1, v0 + i + 2): one cluster over n + 2 vertices."""
    i = np.arange(n, dtype=np.int64)[:, None] + v0
    return (i + np.arange(3)).astype(np.int32)


def tetrahedron(v0=0):
    return np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32) + v0


def with_attributes(triangles, n_vertices, seed=0):
    r = np.random.default_rng(seed)
    return (r.uniform(-2, 2, (n_vertices, 3)).astype(np.float32), r.uniform(0, 1, (n_vertices, 3)).astype(np.float32),
            np.ascontiguousarray(triangles, np.int32).reshape(-1, 3))


def clusters_mesh(sizes, seed=0, shuffle=True, spare_vertices=0):
    """One strip per entry of `sizes` on vertices of its own, `spare_vertices` that nothing references in front, the triangle order shuffled."""
    parts, v0 = [], spare_vertices
    for n in sizes:
        parts.append(strip(n, v0))
        v0 += n + 2
    t = np.concatenate(parts) if parts else np.zeros((0, 3), np.int32)
    if shuffle:
        t = t[np.random.default_rng(seed).permutation(len(t))]
    return with_attributes(t, v0, seed)


def mixed_mesh(T, seed=0, shuffle=True):
    """Exactly T triangles: isolated triangles, tetrahedra and strips of 2..7, from T = 255 on also a strip of 60 and one of 50 (what survives the
    floor of 50); every piece on vertices of its own."""
    r = np.random.default_rng(seed)
    parts, n, v0 = [], 0, 0
    if T >= 255:
        for m in (60, 50):
            parts.append(strip(m, v0)); n += m; v0 += m + 2
    while n < T:
        kind = int(r.integers(0, 3))
        p = strip(1, v0) if kind == 0 else (tetrahedron(v0) if kind == 1 else strip(int(r.integers(2, 8)), v0))
        p = p[:T - n]
        parts.append(p); n += len(p); v0 += int(p.max()) - v0 + 1
    t = np.concatenate(parts)
    if shuffle:
        t = t[r.permutation(T)]
    return with_attributes(t, v0, seed)


def grid(n, v0=0):
    """n x n quads on (n + 1)^2 welded vertices, two triangles each."""
    i, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    a = (i * (n + 1) + j + v0).reshape(-1)
    b, c, d = a + 1, a + n + 1, a + n + 2
    return np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


def adversarial_grids(n=64, seed=0):
    """Two n x n grids that share ONE vertex (the last of the first = the first of the second), triangles in random order, the indices of every
    triangle rotated and flipped at random -> (vertices, colours, triangles, the grid of every triangle)."""
    r = np.random.default_rng(seed)
    nv = (n + 1) ** 2
    t = np.concatenate([grid(n), grid(n, nv - 1)])
    which = np.repeat(np.arange(2), 2 * n * n)
    p = r.permutation(len(t))
    t, which = t[p], which[p]
    rot = r.integers(0, 3, len(t))
    t = np.stack([t[np.arange(len(t)), (rot + k) % 3] for k in range(3)], 1)
    flip = r.integers(0, 2, len(t)).astype(bool)
    t[flip] = t[flip][:, ::-1]
    return with_attributes(t, 2 * nv - 1, seed) + (which,)


# ---- hand-written answers: (name, triangles, triangle_clusters, cluster_n_triangles)
HAND_CLUSTERS = [
    ("two triangles sharing one vertex only", [[0, 1, 2], [2, 3, 4]], [0, 1], [1, 1]),
    ("two triangles sharing an edge", [[0, 1, 2], [2, 1, 3]], [0, 0], [2]),
    ("three triangles on one edge", [[0, 1, 2], [0, 1, 3], [1, 0, 4]], [0, 0, 0], [3]),
    ("a duplicate joins its twin", [[0, 1, 2], [5, 6, 7], [2, 0, 1]], [0, 1, 0], [2, 1]),
    ("(a,a,b) joins its neighbour through (a,b)", [[5, 6, 7], [0, 1, 3], [1, 1, 3]], [0, 1, 1], [1, 2]),
    ("(a,a,b) and (a,a,c) share the edge (a,a)", [[1, 1, 3], [5, 6, 7], [1, 1, 4]], [0, 1, 0], [2, 1]),
    ("(a,a,a)", [[2, 2, 2], [2, 2, 5], [0, 1, 2]], [0, 0, 1], [2, 1]),
    ("numbered by the smallest triangle", [[6, 7, 8], [0, 1, 2], [3, 4, 5], [2, 1, 9], [8, 7, 10]], [0, 1, 2, 1, 0], [2, 2, 1]),
]


def degenerate_case():
    """A strip of 50 on vertices 2..53; D1 = (2,2,3) joins it through (2,3), D2 = (2,2,55) joins D1 through (2,2): one cluster of 52.  A floater of 3
    triangles on 56..60.  Vertices 0, 1 and 54 are referenced by nobody, 55 by D2 alone.
    -> (vertices, colours, triangles, expected): step 3 keeps vertices 2..53 and 55 (D2 still references it), step 4 then drops D1 and D2, so the
    result keeps vertex 55 although no triangle of the result references it."""
    t = np.concatenate([strip(20, 2), [[2, 2, 3]], strip(3, 56), strip(30, 22), [[2, 2, 55]]]).astype(np.int32)
    v, c, t = with_attributes(t, 61, seed=5)
    kept = np.r_[np.arange(2, 54), 55]
    tris = np.concatenate([strip(20, 0), strip(30, 20)]).astype(np.int32)            # 2 -> 0, ...: every index drops by 2
    return v, c, t, dict(vertices=v[kept], colors=c[kept], triangles=tris, step3_triangles=52)


TIES = dict(sizes=[55, 60, 52, 55], k=2, threshold=55, kept_sizes=[55, 60, 55])        # sorted 52 55 55 60: n[-2] = 55, both 55s stay
FLOOR_CASE = dict(sizes=[60, 49], k=2, threshold=50, kept_sizes=[60])                     # n[-2] = 49 < 50
MATRIX_SIZES = [200, 120, 120, 60, 49, 3, 1]
MATRIX = {1: (200, [200]), 2: (120, [200, 120, 120]), 3: (120, [200, 120, 120]), 4: (60, [200, 120, 120, 60]), 5: (50, [200, 120, 120, 60]),
          7: (50, [200, 120, 120, 60])}                                                  # k -> (threshold, sizes that stay)
