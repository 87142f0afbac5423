"""The numpy restatement of include/gsrast.h, "mesh rasterization and visibility": what gsrast.rasterize_mesh, triangle_view_counts and
cull_unseen_triangles are held to, operation by operation.

Everything is float64 arithmetic on widened float32 inputs, each expression evaluated operation by operation in the order written (numpy contracts
nothing), integers are int64 and exact:
  view        c_k = ((x M[0,k] + y M[1,k]) + z M[2,k]) + M[3,k], w = c_3 (row-vector convention, gssr/utils/mesh_utils.py:199-201)
  pixels      ndc_x = c_0 / w, px = ((ndc_x + 1) W - 1) 0.5, likewise py with H (ndc2Pix: centres at integers); X = rint(px 256), Y = rint(py 256)
  dropped     near: some vertex has !(w > near) (no clipping); guard: otherwise some !(|X| <= 2^24); zero_area: otherwise
              area2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) == 0.  cull_sign != 0 keeps only triangles whose area2 has that sign (not counted).
  coverage    area2 < 0: vertices 1 and 2 exchanged.  E_k(P) = dx (Py - Yi) - dy (Px - Xi), i = (k + 1) % 3, j = (k + 2) % 3, d = (Xj - Xi, Yj - Yi),
              P = (256 col, 256 row); covered iff every E_k > 0 or E_k == 0 and (dy < 0 or (dy == 0 and dx > 0)): top-left, watertight.
              Candidates ceil(Xmin / 256) .. floor(Xmax / 256), the same in y, clamped to the image.
  depth       l_k = E_k / |area2|, iw = (l0 (1/w0) + l1 (1/w1)) + l2 (1/w2) in the exchanged order, z64 = 1 / iw, z = float32(z64)
  winner      the minimum of (float32 bits of z) << 32 | triangle over the covering triangles, as uint64
  outputs     depth (0 where empty), triangle_id (-1), barycentric = float32((l_k (1/w_k)) z64) of the triangle's vertices 1 and 2 in the index
              buffer's order (0)
  seen        not dropped or culled, and owner of a pixel or -- with a tolerance -- a vertex with (rint(px), rint(py)) inside the image whose pixel
              is empty or has w <= float64(depth) + tolerance
The OUTSIDE of this repository's marching-cubes output (signed volume > 0: counter-clockwise seen from outside, like the spheres of
tests/raster_cases.py) under the reference's camera convention (+z forward, y down in the image) is area2 < 0, cull_sign = -1: on the sphere of
tests/ref_mesh_numpy.py every triangle that owns a pixel has area2 < 0 (test_raster_cpu.test_the_outside_of_a_marching_cubes_mesh_is_cull_sign_minus_one)."""
import numpy as np

ERR_INDEX, ERR_NONFINITE = 1, 16                      # GSR_MESH_ERR_*
GUARD = float(1 << 24)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
OK, NEAR, GUARDED, ZERO, CULLED = 0, 1, 2, 3, 4


def status(vertices, triangles):
    st = 0
    if vertices.size and not np.isfinite(vertices).all():
        st |= ERR_NONFINITE
    if triangles.size and ((triangles < 0) | (triangles >= len(vertices))).any():
        st |= ERR_INDEX
    return st


def project(vertices, M, W, H):
    """-> px, py, w of every vertex (float64)."""
    v, M = vertices.astype(np.float64), np.asarray(M, np.float32).astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        c = [((x * M[0, k] + y * M[1, k]) + z * M[2, k]) + M[3, k] for k in (0, 1, 3)]
        w = c[2]
        px = ((c[0] / w + 1.0) * float(W) - 1.0) * 0.5
        py = ((c[1] / w + 1.0) * float(H) - 1.0) * 0.5
    return px, py, w


def setup(vertices, triangles, M, W, H, near, cull_sign):
    """Per triangle: state, X [T,3], Y [T,3] (int64, in the order of the coverage test), rw [T,3] (that order), |area2|, swapped, and the
    per-vertex px, py, w."""
    px, py, w = project(vertices, M, W, H)
    t = triangles.astype(np.int64)
    with np.errstate(all="ignore"):
        Xd, Yd = np.rint(px * 256.0), np.rint(py * 256.0)
        near_v, guard_v = ~(w > near), ~(np.abs(Xd) <= GUARD) | ~(np.abs(Yd) <= GUARD)
    safe = lambda a: np.where(np.abs(a) <= GUARD, a, 0.0).astype(np.int64)
    X, Y = safe(Xd)[t], safe(Yd)[t]
    with np.errstate(all="ignore"):
        rw = (1.0 / w)[t]
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    state = np.full(len(t), OK)
    if cull_sign:
        state[(area2 > 0) != (cull_sign > 0)] = CULLED
    state[area2 == 0] = ZERO
    state[guard_v[t].any(1)] = GUARDED
    state[near_v[t].any(1)] = NEAR
    sw = area2 < 0
    for a in (X, Y, rw):
        a[sw] = a[sw][:, [0, 2, 1]]
    return state, X, Y, rw, np.abs(area2), sw, (px, py, w)


def rasterize(vertices, triangles, M, W, H, near=0.01, cull_sign=0):
    """One view -> dict(depth, triangle_id, barycentric, dropped, keys, state, box).  Raises ValueError on a status."""
    if status(vertices, triangles):
        raise ValueError(status(vertices, triangles))
    state, X, Y, rw, A, sw, vert = setup(vertices, triangles, M, W, H, near, cull_sign)
    T = len(triangles)
    keys = np.full((H, W), EMPTY, np.uint64)
    c0, c1 = np.maximum(-((-X.min(1)) // 256), 0), np.minimum(X.max(1) // 256, W - 1)
    r0, r1 = np.maximum(-((-Y.min(1)) // 256), 0), np.minimum(Y.max(1) // 256, H - 1)
    live = (state == OK) & (c0 <= c1) & (r0 <= r1)
    box = np.where(live, (c1 - c0 + 1) * (r1 - r0 + 1), 0)
    ties = 0                                              # E_k == 0 at a candidate centre, over all live triangles

    def edges(t, Px, Py):
        E, ok = [], True
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            dx, dy = int(X[t, j] - X[t, i]), int(Y[t, j] - Y[t, i])
            e = dx * (Py - int(Y[t, i])) - dy * (Px - int(X[t, i]))
            ok = ok & ((e > 0) | ((e == 0) & bool(dy < 0 or (dy == 0 and dx > 0))))
            E.append(e)
        return E, ok

    for t in np.nonzero(live)[0]:
        Py, Px = np.meshgrid(256 * np.arange(r0[t], r1[t] + 1, dtype=np.int64), 256 * np.arange(c0[t], c1[t] + 1, dtype=np.int64), indexing="ij")
        E, ok = edges(t, Px, Py)
        ties += int(sum((e == 0).sum() for e in E))
        if not ok.any():
            continue
        lam = [e.astype(np.float64) / float(A[t]) for e in E]
        iw = (lam[0] * rw[t, 0] + lam[1] * rw[t, 1]) + lam[2] * rw[t, 2]
        z = (1.0 / iw).astype(np.float32)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        sub = keys[r0[t]:r1[t] + 1, c0[t]:c1[t] + 1]
        sub[ok] = np.minimum(sub[ok], key[ok])
    hit = keys != EMPTY
    tid = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    bary = np.zeros((H, W, 2), np.float32)
    rows, cols = np.nonzero(hit)
    for r, c in zip(rows, cols):
        t = int(tid[r, c])
        E, _ = edges(t, 256 * int(c), 256 * int(r))
        lam = [np.float64(e) / np.float64(A[t]) for e in E]
        z64 = 1.0 / ((lam[0] * rw[t, 0] + lam[1] * rw[t, 1]) + lam[2] * rw[t, 2])
        q1, q2 = np.float32((lam[1] * rw[t, 1]) * z64), np.float32((lam[2] * rw[t, 2]) * z64)
        bary[r, c] = (q2, q1) if sw[t] else (q1, q2)
    dropped = np.array([(state == NEAR).sum(), (state == GUARDED).sum(), (state == ZERO).sum()], np.int32)
    return dict(depth=depth, triangle_id=tid, barycentric=bary, dropped=dropped, keys=keys, state=state, box=box, ties=ties, vert=vert)


def seen(vertices, triangles, view, W, H, depth_tolerance=None):
    """bool [T] of one rasterize() result."""
    T = len(triangles)
    own = np.zeros(T, bool)
    ids = view["triangle_id"]
    own[ids[ids >= 0]] = True
    if depth_tolerance is not None and T:
        px, py, w = view["vert"]
        with np.errstate(all="ignore"):
            fx, fy = np.rint(px), np.rint(py)
            inside = (fx >= 0.0) & (fx <= float(W - 1)) & (fy >= 0.0) & (fy <= float(H - 1))
        ix, iy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
        d = view["depth"][iy, ix].astype(np.float64)
        with np.errstate(all="ignore"):
            ok = inside & ((view["triangle_id"][iy, ix] < 0) | (w <= d + float(depth_tolerance)))
        own |= ok[triangles.astype(np.int64)].any(1)
    return own & (view["state"] == OK)


def view_counts(vertices, triangles, mats, W, H, near=0.01, cull_sign=0, depth_tolerance=None, views=None):
    """int32 [T]; `views`: the rasterize() results where the caller has them."""
    n = np.zeros(len(triangles), np.int32)
    for k, M in enumerate(mats):
        r = views[k] if views is not None else rasterize(vertices, triangles, M, W, H, near, cull_sign)
        n += seen(vertices, triangles, r, W, H, depth_tolerance)
    return n


def cull(vertices, colors, triangles, counts, min_views=1):
    """The triangles with counts >= min_views in their order, unreferenced vertices dropped, order kept -> vertices, colors, triangles."""
    keep_t = triangles[counts >= min_views]
    used = np.zeros(len(vertices), bool)
    used[keep_t.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return vertices[used], colors[used], new[keep_t].astype(np.int32).reshape(-1, 3)
