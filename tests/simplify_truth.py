"""The definition of gsrast.mesh.simplify_vertex_clustering (include/gsrast.h, "mesh simplification") as plain numpy float64 and Python
numbers, operation by operation, in the kernel's order.  A Python float is an IEEE double and +, -, *, /, math.sqrt and math.floor round as the
device's float64 operations do with FMA contraction off, so the GPU tests compare with np.array_equal.

  1. lo = per-axis float32 minimum over ALL vertices; origin = float64(lo) - 0.5 * voxel_size
  2. cell of a vertex: floor((float64(v) - origin) / voxel_size) per axis, inside [0, 2^21)
  3. one new vertex per occupied cell, numbered in ascending order of the cell's lowest member; vertex_map[v] = the new index of v
  4. average: float64 sum of the members in ascending vertex index, from 0.0, divided by float64(count), rounded to float32 (positions and colours)
  5. quadric: per triangle (a, b, c), everything relative to origin:
         a' = a - origin ...; e1 = b' - a', e2 = c' - a'; N = e1 x e2; L = sqrt((Nx Nx + Ny Ny) + Nz Nz); L == 0 or non-finite: nothing
         n = N / L; d = -((nx a'x + ny a'y) + nz a'z); p = (n, d); w = L * 0.5; q_ij = w * (p_i * p_j), i <= j
     every corner adds q to its cell, ascending (triangle, corner); A = Q[:3,:3], r = -Q[:3,3]; cofactors, det and x as written in solve();
     taken iff det finite and > 0, x finite and c * voxel <= x <= (c + 1.0) * voxel per axis; the position is float32(origin + x)
  6. triangles: mapped, degenerate ones dropped, rotated smallest first, of equal triples the lowest original index stays, order kept

CONDITIONS ON THE INPUTS (checked here, on the CPU, for every case run with contraction="quadric"; the number of cells excused from the comparison
is zero): no component of x of a cell with det > 0 lies within 2^-30 * voxel_size of a face of the cell's box, and no determinant is exactly 0 for a
non-flat cell.  A cell counts as non-flat when its planes span three dimensions: the smallest singular value of A is above 1e-9 of the largest
(numpy's SVD; only this classification uses it).  The determinant of a flat or edge-like cell -- one or two plane directions -- is rounding noise
around 0, often exactly 0, and such a cell is compared like any other: both sides evaluate the same operations."""
import math

import numpy as np

AXIS_CELLS = 1 << 21
ERR_INDEX, ERR_RANGE, ERR_NONFINITE = 1, 8, 16
MARGIN = 2.0 ** -30


class SimplifyError(Exception):
    def __init__(self, status):
        super().__init__(f"status {status}")
        self.status = status


def origin_of(vertices, voxel_size):
    lo = vertices.min(axis=0)                             # float32, exact in any order
    return [float(lo[a]) - 0.5 * voxel_size for a in range(3)]


def cells_of(vertices, voxel_size):
    """-> (origin [3 floats], cells: list of V (cx, cy, cz) Python integers); raises SimplifyError as the status word would."""
    vs = float(voxel_size)
    if not np.isfinite(vertices).all():
        raise SimplifyError(ERR_NONFINITE)
    o = origin_of(vertices, vs)
    cells = []
    for p in vertices.tolist():                           # float32 -> Python float is exact
        c = tuple(math.floor((p[a] - o[a]) / vs) for a in range(3))
        if not all(0 <= x < AXIS_CELLS for x in c):
            raise SimplifyError(ERR_RANGE)
        cells.append(c)
    return o, cells


def triangle_quadric(pa, pb, pc, o):
    """The ten entries 00 01 02 03 11 12 13 22 23 33 of (L / 2) p p^T, or None where the triangle contributes nothing."""
    A = [pa[k] - o[k] for k in range(3)]
    e1 = [(pb[k] - o[k]) - A[k] for k in range(3)]
    e2 = [(pc[k] - o[k]) - A[k] for k in range(3)]
    N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    s = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    if not math.isfinite(s):
        return None
    L = math.sqrt(s)
    if not L > 0.0:
        return None
    p = [N[0] / L, N[1] / L, N[2] / L, 0.0]
    p[3] = -((p[0] * A[0] + p[1] * A[1]) + p[2] * A[2])
    w = L * 0.5
    return [w * (p[i] * p[j]) for i in range(4) for j in range(i, 4)]


def solve(Q):
    """-> (det, x or None, the three terms of det)."""
    a00, a01, a02, a11, a12, a22 = Q[0], Q[1], Q[2], Q[4], Q[5], Q[7]
    r0, r1, r2 = -Q[3], -Q[6], -Q[8]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    terms = (a00 * c00, a01 * c01, a02 * c02)
    det = (terms[0] + terms[1]) + terms[2]
    if not (math.isfinite(det) and det > 0.0):
        return det, None, terms
    with np.errstate(all="ignore"):
        x = [float(np.float64((c00 * r0 + c01 * r1) + c02 * r2) / np.float64(det)),      # numpy: an overflowing quotient is inf, not an exception
             float(np.float64((c01 * r0 + c11 * r1) + c12 * r2) / np.float64(det)),
             float(np.float64((c02 * r0 + c12 * r1) + c22 * r2) / np.float64(det))]
    return det, x, terms


def non_flat(Q):
    A = np.array([[Q[0], Q[1], Q[2]], [Q[1], Q[4], Q[5]], [Q[2], Q[5], Q[7]]], dtype=np.float64)
    if not np.isfinite(A).all():
        return False
    sv = np.linalg.svd(A, compute_uv=False)
    return bool(sv[2] > 1.0e-9 * sv[0])


def simplify(vertices, colors, triangles, voxel_size, contraction="average", check_conditions=True):
    """-> dict(vertices float32 [V',3], colors float32 [V',3], triangles int32 [T',3], vertex_map int32 [V], record (0, V', T', quadric cells),
    members: the largest cell population, quadric: bool [V'] the cells that took the quadric position)."""
    assert contraction in ("average", "quadric")
    vs = float(voxel_size)
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    colors = np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    V, T = len(vertices), len(triangles)
    if T and (V == 0 or triangles.min() < 0 or triangles.max() >= V):
        if V and not np.isfinite(vertices).all():
            raise SimplifyError(ERR_NONFINITE | ERR_INDEX)
        raise SimplifyError(ERR_INDEX)
    if V == 0:
        return dict(vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32), triangles=np.zeros((0, 3), np.int32),
                    vertex_map=np.zeros(0, np.int32), record=(0, 0, 0, 0), members=0, quadric=np.zeros(0, bool))
    o, cells = cells_of(vertices, vs)
    index, vmap, cell_of_new = {}, [], []
    for v, c in enumerate(cells):                         # ascending v: a cell is numbered when its lowest member comes by
        if c not in index:
            index[c] = len(index)
            cell_of_new.append(c)
        vmap.append(index[c])
    n_new = len(index)
    # 4. the sums, one member after another in ascending vertex index
    sums = [[0.0] * 6 for _ in range(n_new)]
    count = [0] * n_new
    vl, cl = vertices.tolist(), colors.tolist()
    for v in range(V):
        s, p, q = sums[vmap[v]], vl[v], cl[v]
        for a in range(3):
            s[a] += p[a]
            s[3 + a] += q[a]
        count[vmap[v]] += 1
    with np.errstate(all="ignore"):
        mean = np.array(sums, dtype=np.float64) / np.array(count, dtype=np.float64)[:, None]
        new_v, new_c = mean[:, :3].astype(np.float32), mean[:, 3:].astype(np.float32)
    took = np.zeros(n_new, bool)
    if contraction == "quadric":
        Q = [None] * n_new
        tl = triangles.tolist()
        for t in range(T):
            i = tl[t]
            q = triangle_quadric(vl[i[0]], vl[i[1]], vl[i[2]], o)
            if q is None:
                continue
            for corner in range(3):                       # ascending (triangle, corner)
                p = vmap[i[corner]]
                if Q[p] is None:
                    Q[p] = [0.0] * 10
                acc = Q[p]
                for k in range(10):
                    acc[k] += q[k]
        for p in range(n_new):
            if Q[p] is None:
                continue
            det, x, terms = solve(Q[p])
            if check_conditions:
                assert not (det == 0.0 and non_flat(Q[p])), ("the determinant of a non-flat cell is exactly 0", p, terms)
            if x is None:
                continue
            ok = all(math.isfinite(xa) for xa in x)
            for a in range(3):
                lo_, hi_ = float(cell_of_new[p][a]) * vs, (float(cell_of_new[p][a]) + 1.0) * vs
                if ok and check_conditions:
                    assert abs(x[a] - lo_) > MARGIN * vs and abs(x[a] - hi_) > MARGIN * vs, ("x within 2^-30 voxel of a box face", p, a, x[a], lo_, hi_)
                ok = ok and lo_ <= x[a] <= hi_
            if ok:
                took[p] = True
                new_v[p] = [np.float32(o[a] + x[a]) for a in range(3)]
    # 6. triangles
    out, seen = [], set()
    for i in triangles.tolist():
        a, b, c = vmap[i[0]], vmap[i[1]], vmap[i[2]]
        if a == b or b == c or c == a:
            continue
        if b < a and b < c:
            a, b, c = b, c, a
        elif c < a and c < b:
            a, b, c = c, a, b
        if (a, b, c) in seen:
            continue
        seen.add((a, b, c))
        out.append((a, b, c))
    new_t = np.array(out, dtype=np.int32).reshape(-1, 3)
    return dict(vertices=new_v, colors=new_c, triangles=new_t, vertex_map=np.array(vmap, dtype=np.int32), record=(0, n_new, len(out), int(took.sum())),
                members=max(count), quadric=took)
