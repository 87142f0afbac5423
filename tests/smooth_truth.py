"""The definition of gsrast.mesh.vertex_adjacency, compute_triangle_normals, compute_vertex_normals and filter_smooth_simple / _laplacian / _taubin
(include/gsrast.h, "mesh smoothing and normals"), restated in plain numpy float64, operation by operation in the stated order.
Nothing here adds up a list with np.sum: a sum over the neighbours (or the corners) of a vertex is one addition after another in ascending order --
the k-th term of every vertex at once, which is the same chain of roundings per vertex.  numpy's elementwise + - * / and sqrt are IEEE operations
rounded on their own, which is what the kernels compute with FMA contraction off.

  adjacency   N(i) = the j != i that share at least one triangle with i, distinct and ascending: start int32 [V + 1], neighbours int32 [E].
  normals     n_t = (v1 - v0) x (v2 - v0) in float64; normalised: n / sqrt((nx nx + ny ny) + nz nz), (0, 0, 1) where that is 0 or not finite;
              a vertex normal is the sum of the unnormalised n_t over its corners in ascending corner index 3 t + k.
  smoothing   float64 state from the first step to the last, rounded to float32 once."""
import numpy as np

ERR_INDEX, ERR_NONFINITE = 1, 16
SIMPLE, LAPLACIAN, TAUBIN = "simple", "laplacian", "taubin"


class MeshError(ValueError):
    def __init__(self, status):
        super().__init__(f"status {status}")
        self.status = status


def _check_index(triangles, V):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= V):
        raise MeshError(ERR_INDEX)
    return t


def adjacency(triangles, V):
    """-> (start int32 [V + 1], neighbours int32 [E])."""
    t = _check_index(triangles, V)
    pairs = np.concatenate([t[:, [a, b]] for a in range(3) for b in range(3) if a != b]) if len(t) else np.zeros((0, 2), np.int64)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    pairs = np.unique(pairs, axis=0) if len(pairs) else pairs             # sorted by (src, dst), every pair once
    start = np.zeros(V + 1, np.int64)
    np.add.at(start, pairs[:, 0] + 1, 1)
    return np.cumsum(start).astype(np.int32), pairs[:, 1].astype(np.int32)


def _cross(vertices, t):
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    v0, v1, v2 = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _unit(n):
    with np.errstate(all="ignore"):
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (L > 0.0) & np.isfinite(L)
        out = n / np.where(ok, L, 1.0)[:, None]
    out[~ok] = (0.0, 0.0, 1.0)
    return out


def _round(x):
    with np.errstate(all="ignore"):
        return x.astype(np.float32)


def triangle_normals(vertices, triangles, normalized=True):
    t = _check_index(triangles, len(vertices))
    n = _cross(vertices, t)
    return _round(_unit(n) if normalized else n)


def vertex_normals(vertices, triangles, normalized=True):
    V = len(vertices)
    t = _check_index(triangles, V)
    n = _cross(vertices, t)
    corner_vertex = t.reshape(-1)                                         # corner h = 3 t + k
    order = np.argsort(corner_vertex, kind="stable")                      # ascending h inside a vertex
    count = np.bincount(corner_vertex, minlength=V)[:V] if len(corner_vertex) else np.zeros(V, np.int64)
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    s = np.zeros((V, 3))
    with np.errstate(all="ignore"):
        for k in range(int(count.max()) if V and len(corner_vertex) else 0):
            who = np.flatnonzero(count > k)
            s[who] = s[who] + n[order[first[who] + k] // 3]
    return _round(_unit(s) if normalized else s)


def _step(p, start, nb, lam):
    """One step on the float64 state p [V, C] (columns 0..2 the positions).  lam None: the simple filter."""
    V = len(p)
    deg = (start[1:] - start[:-1]).astype(np.int64)
    s = p.copy() if lam is None else np.zeros_like(p)
    W = np.zeros(V)
    with np.errstate(all="ignore"):
        for k in range(int(deg.max()) if V else 0):
            who = np.flatnonzero(deg > k)
            r = p[nb[start[who] + k]]
            if lam is None:
                s[who] = s[who] + r
            else:
                d = p[who, :3] - r[:, :3]
                w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
                W[who] = W[who] + w
                s[who] = s[who] + w[:, None] * r
        if lam is None:
            return s / (deg + 1).astype(np.float64)[:, None]
        q = p + lam * (s / W[:, None] - p)
    q[deg == 0] = p[deg == 0]
    return q


def smooth(vertices, colors, triangles, kind, iterations=1, lam=0.5, mu=-0.53, scope="all"):
    """-> (vertices float32 [V,3], colors float32 [V,3]) of the smoothed mesh."""
    v32, c32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3), np.asarray(colors, dtype=np.float32).reshape(-1, 3)
    if iterations == 0:
        return v32.copy(), c32.copy()
    start, nb = adjacency(triangles, len(v32))
    if not np.isfinite(v32).all():
        raise MeshError(ERR_NONFINITE)
    start, nb = start.astype(np.int64), nb.astype(np.int64)
    p = np.concatenate([v32.astype(np.float64), c32.astype(np.float64)], axis=1) if scope == "all" else v32.astype(np.float64)
    for _ in range(iterations):
        if kind == SIMPLE:
            p = _step(p, start, nb, None)
        else:
            p = _step(p, start, nb, lam)
            if kind == TAUBIN:
                p = _step(p, start, nb, mu)
    return _round(p[:, :3]), (_round(p[:, 3:]) if scope == "all" else c32.copy())
