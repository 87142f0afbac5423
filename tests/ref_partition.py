"""The VastGaussian scene split restated over arrays (split_scene.py:39-53, gssr/utils/vastgaussian_utils.py:89-286).  TEST INFRASTRUCTURE ONLY.

Written from the reference's formulas in numpy; nothing here imports gsrast.  tests/test_partition_cpu.py holds every function to what the reference's
own four functions produced (tests/golden/ref_partition_*.npz) exactly, before a GPU result is read against it.

    centres            np.linalg.inv(w2c)[:3, -1], as get_cam_center: NOT -R^T t (the two differ in the last bits, and a camera on its own tile's edge
                       must compare equal to the box that was made from it)
    region_division    quadtree (stable sorted, the longer extent, ties to axis 1, a half is final when len < max_num_images) or grid (integer-division
                       slices; the leftovers at the end of a column or row belong to no tile)
    data_selection     inclusive float64 comparisons against the box expanded by ratio / 2 of its extent per side
    z_range            glue_truth.dist2_bruteforce on the float32 subset, numpy's own float32 mean() and std(), strict inequalities
    visibility         dtype float64, or np.longdouble for the floor of float64's own error: projection operation by operation, hull by
                       scipy.spatial.ConvexHull (always on the float64 points), an exact convex clip against the image rectangle, shoelace area
    coverage           np.unique of the tile's images' ids != -1; an id without a table row is a KeyError"""
import numpy as np

import glue_truth


def rotmat(q):
    w, x, y, z = (np.float64(v) for v in q)
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


def w2c(q, t):
    m = np.zeros((4, 4))
    m[:3, :3] = rotmat(q)
    m[:3, -1] = np.array(t)
    m[3, 3] = 1.0
    return m


def centres(qvecs, tvecs):
    return np.array([np.linalg.inv(w2c(q, t))[:3, -1] for q, t in zip(qvecs, tvecs)], np.float64).reshape(-1, 3)


def look_at(centre, target, roll=0.0):
    """-> (qvec, tvec) of a camera at `centre` whose +z axis points at `target` (scene construction only)."""
    f = np.asarray(target, np.float64) - np.asarray(centre, np.float64)
    f /= np.linalg.norm(f)
    up = np.array([np.sin(roll), np.cos(roll), 0.0]) if abs(f[2]) > 0.9 else np.array([0.0, 0.0, -1.0])
    r = np.cross(up, f); r /= np.linalg.norm(r)
    u = np.cross(f, r)
    R = np.stack([r, u, f])                               # rows: the camera's axes in world coordinates
    t = -R @ np.asarray(centre, np.float64)
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2; q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (R[j, i] + R[i, j]) / s; q[1 + k] = (R[k, i] + R[i, k]) / s
    return np.array(q, np.float64), t


# ---------------------------------------------------------------------------------------------------------------- step 1
def region_division(cen, num_col=None, num_row=None, max_num_images=150):
    """-> (tiles: list of lists of image indices in the reference's order, boxes float64 [T,4])."""
    cen = np.asarray(cen, np.float64).reshape(-1, 3)
    tiles = []
    if num_col is None or num_row is None:
        def split(idx):
            c = cen[idx]
            axis = 0 if (c[:, 0].max() - c[:, 0].min()) > (c[:, 1].max() - c[:, 1].min()) else 1
            srt = sorted(idx, key=lambda i: cen[i, axis])
            for part in (srt[:len(srt) // 2], srt[len(srt) // 2:]):
                if len(part) < max_num_images:
                    tiles.append(part)
                else:
                    split(part)
        split(list(range(len(cen))))
    else:
        n = len(cen)
        per_col = n // num_col
        srt = sorted(range(n), key=lambda i: cen[i, 0])
        for i in range(num_col):
            col = srt[i * per_col:((i + 1) * per_col if (i + 1) * per_col < n else n)]
            per_tile = len(col) // num_row
            cs = sorted(col, key=lambda i: cen[i, 1])
            for j in range(num_row):
                tiles.append(cs[j * per_tile:((j + 1) * per_tile if (j + 1) * per_tile < len(col) else len(col))])
    boxes = np.array([[cen[t, 0].min(), cen[t, 0].max(), cen[t, 1].min(), cen[t, 1].max()] for t in tiles], np.float64).reshape(-1, 4)
    return tiles, boxes


# ---------------------------------------------------------------------------------------------------------------- step 2
def expand(boxes, ratio):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    dw = (b[:, 1] - b[:, 0]) * ratio / 2.0
    dh = (b[:, 3] - b[:, 2]) * ratio / 2.0
    return np.stack([b[:, 0] - dw, b[:, 1] + dw, b[:, 2] - dh, b[:, 3] + dh], axis=1)


def inside(xy, boxes):
    """bool [T, n]: inclusive, float64."""
    x, y = np.asarray(xy, np.float64)[:, 0][None], np.asarray(xy, np.float64)[:, 1][None]
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return (x >= b[:, 0:1]) & (x <= b[:, 1:2]) & (y >= b[:, 2:3]) & (y <= b[:, 3:4])


def data_selection(boxes, cen, xyz, ratio=0.2):
    nb = expand(boxes, ratio)
    return [np.nonzero(m)[0] for m in inside(cen, nb)], [np.nonzero(m)[0] for m in inside(xyz, nb)]


# ---------------------------------------------------------------------------------------------------------------- step 3
def z_range(xyz):
    """-> dict(mz, Mz python floats of the float32 values, dist, lo, hi float32)."""
    pts = np.asarray(xyz, np.float64).reshape(-1, 3).astype(np.float32)
    dist = glue_truth.dist2_bruteforce(pts)
    lo, hi = dist.mean() - 3 * dist.std(), dist.mean() + 3 * dist.std()
    mask = (dist > lo) & (dist < hi)
    z = pts[mask][:, -1]
    return dict(mz=float(z.min()), Mz=float(z.max()), dist=dist, lo=lo, hi=hi, mask=mask)


def corners(box, mz, Mz, dtype=np.float64):
    mx, Mx, my, My = (dtype(v) for v in box)
    mz, Mz = dtype(mz), dtype(Mz)
    return np.array([[mx, my, mz], [mx, my, Mz], [mx, My, mz], [mx, My, Mz], [Mx, my, mz], [Mx, my, Mz], [Mx, My, mz], [Mx, My, Mz]], dtype)


def clip_convex(poly, w, h):
    """The convex polygon `poly` [n,2] (either orientation) cut to [0, w] x [0, h], exactly (Sutherland-Hodgman) -> [m,2] in poly's dtype."""
    pts = [tuple(p) for p in poly]
    one = poly.dtype.type
    for axis, bound, ge in ((0, one(0), True), (0, one(w), False), (1, one(0), True), (1, one(h), False)):
        out = []
        for i, cur in enumerate(pts):
            prev = pts[i - 1]
            cin = cur[axis] >= bound if ge else cur[axis] <= bound
            pin = prev[axis] >= bound if ge else prev[axis] <= bound
            if cin != pin:
                f = (bound - prev[axis]) / (cur[axis] - prev[axis])
                o = prev[1 - axis] + f * (cur[1 - axis] - prev[1 - axis])
                out.append((bound, o) if axis == 0 else (o, bound))
            if cin:
                out.append(cur)
        pts = out
    return np.array(pts, poly.dtype).reshape(-1, 2)


def area(poly):
    if len(poly) < 3:
        return poly.dtype.type(0)
    x, y = poly[:, 0], poly[:, 1]
    s = poly.dtype.type(0)
    for i in range(len(poly)):
        j = (i + 1) % len(poly)
        s = s + (x[i] * y[j] - x[j] * y[i])
    return abs(s) * poly.dtype.type(0.5)


def project(cor, E, fx, fy, w, h):
    """The reference's projection(): w2c then K with the principal point at the image's middle; no test of the sign of z.  -> (uv [8,2], zc [8])."""
    t = cor.dtype.type
    E = np.asarray(E).astype(cor.dtype)
    X, Y, Z = cor[:, 0], cor[:, 1], cor[:, 2]
    xc = ((E[0, 0] * X + E[0, 1] * Y) + E[0, 2] * Z) + E[0, 3]
    yc = ((E[1, 0] * X + E[1, 1] * Y) + E[1, 2] * Z) + E[1, 3]
    zc = ((E[2, 0] * X + E[2, 1] * Y) + E[2, 2] * Z) + E[2, 3]
    u = (t(fx) * xc + (t(w) / t(2)) * zc) / zc
    v = (t(fy) * yc + (t(h) / t(2)) * zc) / zc
    return np.stack([u, v], axis=1), zc


def visibility(boxes, zr, E, cen, intr, members, threshold, dtype=np.float64):
    """boxes [T,4]; zr [T,2] (mz, Mz); E [C,3or4,4] w2c; cen [C,3]; intr [C,4] = (fx, fy, width, height); members: per tile the image indices.
    -> dict(ratio [T,C], d [T,C], md [T], add bool [T,C], zc [T,C,8]) in dtype; member images are evaluated too (their add is False)."""
    from scipy.spatial import ConvexHull, QhullError
    T, C = len(boxes), len(cen)
    cen_t = np.asarray(cen).astype(dtype)
    ratio = np.zeros((T, C), dtype); d = np.zeros((T, C), dtype); md = np.zeros(T, dtype); add = np.zeros((T, C), bool); zcs = np.zeros((T, C, 8), dtype)
    for t in range(T):
        cor = corners(boxes[t], zr[t][0], zr[t][1], dtype)
        mem = np.asarray(members[t], np.int64)
        far = np.zeros(len(mem), dtype)
        for p in cor:
            dx, dy, dz = cen_t[mem, 0] - p[0], cen_t[mem, 1] - p[1], cen_t[mem, 2] - p[2]
            far = np.maximum(far, np.sqrt((dx * dx + dy * dy) + dz * dz))
        md[t] = far.mean() * dtype(1.2) if len(mem) else dtype(np.nan)
        for c in range(C):
            fx, fy, w, h = intr[c]
            uv, zc = project(cor, E[c], fx, fy, w, h)
            zcs[t, c] = zc
            try:
                hull = ConvexHull(uv.astype(np.float64)).vertices
                a = area(clip_convex(uv[hull], w, h))
            except QhullError:
                a = dtype(0)                              # all projections collinear: the reference raises, the project says ratio 0
            ratio[t, c] = a / (dtype(w) * dtype(h))
            l1 = (np.abs(cor[:, 0] - cen_t[c, 0]) + np.abs(cor[:, 1] - cen_t[c, 1])) + np.abs(cor[:, 2] - cen_t[c, 2])
            d[t, c] = (((l1[0] + l1[1]) + (l1[2] + l1[3])) + ((l1[4] + l1[5]) + (l1[6] + l1[7]))) / dtype(8)
            add[t, c] = bool(ratio[t, c] > threshold and d[t, c] < md[t]) and c not in set(mem.tolist())
    return dict(ratio=ratio, d=d, md=md, add=add, zc=zcs)


# ---------------------------------------------------------------------------------------------------------------- step 4
def coverage(tile_images, obs_offsets, obs_ids, point_ids):
    """-> per tile the rows of point_ids (ascending strictly) its images observe, ascending.  KeyError for an id without a row."""
    table = {int(i): r for r, i in enumerate(point_ids)}
    out = []
    for imgs in tile_images:
        ids = [obs_ids[obs_offsets[a]:obs_offsets[a + 1]] for a in imgs]
        ids = np.unique(np.concatenate([i[i != -1] for i in ids])) if len(ids) else np.zeros(0, np.int64)
        out.append(np.array([table[int(i)] for i in ids], np.int64))
    return out


def partition(qvecs, tvecs, intr, obs_offsets, obs_ids, point_ids, xyz, num_col=None, num_row=None, max_num_images=150, ratio=0.2, threshold=0.25):
    """The four steps.  -> dict(boxes, first (step 1's tiles), members (after step 2), in_box, zr, vis, images (final, the added ones in front), points)."""
    cen = centres(qvecs, tvecs)
    E = np.array([w2c(q, t) for q, t in zip(qvecs, tvecs)])
    first, boxes = region_division(cen, num_col, num_row, max_num_images)
    members, in_box = data_selection(boxes, cen, xyz, ratio)
    zrs = [z_range(xyz[p]) for p in in_box]
    zr = np.array([[z["mz"], z["Mz"]] for z in zrs], np.float64)
    vis = visibility(boxes, zr, E, cen, intr, members, threshold)
    images = [np.concatenate([np.nonzero(vis["add"][t])[0], members[t]]).astype(np.int64) for t in range(len(boxes))]
    table = np.sort(np.asarray(point_ids, np.int64))      # point_ids, xyz: in the order of the reference's dict, which need not ascend
    points = [table[rows] for rows in coverage(images, obs_offsets, obs_ids, table)]      # the tiles' point IDS, ascending
    return dict(cen=cen, E=E, boxes=boxes, first=first, members=members, in_box=in_box, zr=zr, zstats=zrs, vis=vis, images=images, points=points)
