"""Restatements of gsrast.chamfer in numpy, operation by operation (no torch): what include/gsrast.h defines under "surface distance".
nearest(): the float32 all-pairs search; sample_surface(), voxel_downsample(), statistics(): the rules of the header; grid_rule() / cell_of():
the cell-size rule of csrc/gsr_chamfer.hip, which no result depends on but the structure of the test cases does."""
import math

import numpy as np

INF = np.float32(np.inf)
AXIS_MAX = 1 << 21                                        # CF_AXIS_MAX
RINGS = 6                                                 # CF_RINGS: shells before the box scan with the dense table (CF_RINGS_SPARSE = 2 without)
MAX_N = 1024                                              # GSR_SAMPLE_MAX_N
CELL_RANGE = 1 << 20


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def md2_of(max_dist):
    """The float32 bound on d2: float32(max_dist) * float32(max_dist), +inf for None."""
    if max_dist is None:
        return INF
    m = np.float32(max_dist)
    return np.float32(m * m)


def pair_d2(q, t):
    """[Q,T] float32: (dx*dx + dy*dy) + dz*dz with dx = t.x - q.x, every operation rounded on its own (the order of glue_truth._pair_d2)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = t[None, :, 0] - q[:, None, 0]; dy = t[None, :, 1] - q[:, None, 1]; dz = t[None, :, 2] - q[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def nearest(query, target, max_dist=None, chunk=128):
    """-> (d2 float32 [Q], index int32 [Q]).  A target counts iff its coordinates are finite and d2 <= md2; the smallest d2 wins, among equal d2
    the lowest index; no counting target, or a non-finite query: (+inf, -1)."""
    q, t = _f32(query), _f32(target)
    Q, T = len(q), len(t)
    d2 = np.full(Q, INF, np.float32); idx = np.full(Q, -1, np.int32)
    if T == 0 or Q == 0:
        return d2, idx
    md2 = md2_of(max_dist)
    t_ok = np.isfinite(t).all(axis=1)
    q_ok = np.isfinite(q).all(axis=1)
    for a in range(0, Q, chunk):
        d = pair_d2(q[a:a + chunk], t)
        with np.errstate(invalid="ignore"):
            counts = t_ok[None, :] & (d <= md2)
        key = np.where(counts, d, INF)
        i = np.argmin(key, axis=1)                        # the first of the smallest: the lowest index
        rows = np.arange(len(i))
        some = counts.any(axis=1)
        far = some & ~counts[rows, i]                     # every counting d2 is +inf and an earlier target that does not count shares it
        i[far] = np.argmax(counts[far], axis=1)
        ok = some & q_ok[a:a + chunk]
        d2[a:a + chunk][ok] = key[rows, i][ok]
        idx[a:a + chunk][ok] = i[ok]
    return d2, idx


def cap(d2, idx, max_dist):
    """nearest(q, t, max_dist) from nearest(q, t, None): the nearest target counts or none does (test_chamfer_cpu holds the identity)."""
    keep = d2 <= md2_of(max_dist)
    return np.where(keep, d2, INF).astype(np.float32), np.where(keep, idx, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the grid (structure only)
def grid_rule(target, max_dist=None):
    """The grid k_np_grid decides on, in float64: dict(Tf, mn [3], h, inv_h, n [3], dense)."""
    t = _f32(target)
    fin = t[np.isfinite(t).all(axis=1)] + np.float32(0)
    Tf = len(fin)
    if Tf == 0:
        return dict(Tf=0, mn=np.zeros(3), h=1.0, inv_h=1.0, n=np.zeros(3, np.int64), dense=False)
    mn, mx = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    e = mx - mn
    emax = e.max()
    A = (e[0] * e[1] + e[1] * e[2]) + e[2] * e[0]
    h = math.sqrt(A / Tf) if A > 0 else (emax / Tf if emax > 0 else 1.0)
    if max_dist is not None and h < float(np.float32(max_dist)):
        h = float(np.float32(max_dist))
    if h < emax / 1048576.0:
        h = emax / 1048576.0
    if not (0.0 < h < 1e300):
        h = 1.0
    inv_h = 1.0 / h
    if not inv_h < 1e300:
        h = inv_h = 1.0
    n = np.minimum(np.floor(e * inv_h) + 1.0, float(AXIS_MAX)).astype(np.int64)
    dense = int(n[0]) * int(n[1]) * int(n[2]) <= min(max(4 * len(t), 4096), 1 << 30)
    return dict(Tf=Tf, mn=mn, h=h, inv_h=inv_h, n=n, dense=dense)


def cell_of(g, p):
    """int64 [..., 3]: the cell of float32 points under grid g (queries are clamped into the grid like this too)."""
    v = np.floor((np.asarray(p, np.float32).astype(np.float64) - g["mn"]) * g["inv_h"])
    return np.clip(v, 0, g["n"] - 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- samples
def triangle_n(a, b, c, spacing):
    a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))

    def e2(p, q):
        d = p - q
        return np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    with np.errstate(over="ignore"):
        L2 = max(e2(b, a), e2(c, b), e2(a, c))
    r = math.sqrt(float(L2)) / float(spacing)
    return max(1, math.ceil(r)) if math.isfinite(r) else MAX_N + 1


def sample_surface(vertices, triangles, spacing):
    """-> float32 [S,3]; raises ValueError("index") / ValueError("cap") as the device sets its status bits."""
    v = _f32(vertices); tr = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = []
    if len(tr) and ((tr < 0) | (tr >= len(v))).any():
        raise ValueError("index")
    for i0, i1, i2 in tr:
        n = triangle_n(v[i0], v[i1], v[i2], spacing)
        if n > MAX_N:
            raise ValueError("cap")
        A, B, C = (v[k].astype(np.float64) for k in (i0, i1, i2))
        for i in range(n):
            for third, count in ((1.0 / 3.0, n - i), (2.0 / 3.0, n - i - 1)):
                j = np.arange(count, dtype=np.float64)
                u = (float(i) + third) / float(n)
                w = (j + third) / float(n)
                out.append(((A[None, :] + u * (B - A)[None, :]) + w[:, None] * (C - A)[None, :]).astype(np.float32))
    return np.concatenate(out).reshape(-1, 3) if out else np.zeros((0, 3), np.float32)


# ---------------------------------------------------------------------------------------------------------------- thinning
def voxel_downsample(points, cell):
    """-> (points_kept, kept_index int32): the lowest index of every occupied cell of floor(float64(p) / float64(cell)); ValueError("range")."""
    p = _f32(points)
    seen, keep = set(), []
    for i, row in enumerate(p):
        if not np.isfinite(row).all():
            continue
        c = np.floor(row.astype(np.float64) / float(cell))
        if ((c < -CELL_RANGE) | (c >= CELL_RANGE)).any():
            raise ValueError("range")
        k = tuple(int(x) for x in c)
        if k not in seen:
            seen.add(k); keep.append(i)
    keep = np.asarray(keep, np.int32)
    return p[keep.astype(np.int64)], keep


# ---------------------------------------------------------------------------------------------------------------- statistics
def direction(src, dst, max_dist, thresholds):
    """(mean of d, [share of d < tau], n): d = sqrt(float64(d2)) clamped to float32(max_dist); the mean is math.fsum / n."""
    d2, _ = nearest(src, dst, max_dist)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2.astype(np.float64))
    if max_dist is not None:
        d = np.minimum(d, float(np.float32(max_dist)))
    n = len(d)
    nan = float("nan")
    return (math.fsum(d.tolist()) / n if n else nan), [(int((d < float(t)).sum()) / n if n else nan) for t in thresholds], n


def surface_distance(pred, gt, max_dist=None, thresholds=()):
    """The dictionary of gsrast.chamfer.surface_distance for two point clouds (sampling and thinning are the caller's)."""
    acc, P, n_p = direction(pred, gt, max_dist, thresholds)
    comp, R, n_g = direction(gt, pred, max_dist, thresholds)
    f = [(2.0 * p * r / (p + r) if p + r > 0 else (0.0 if p + r == 0 else float("nan"))) for p, r in zip(P, R)]
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "thresholds": [float(t) for t in thresholds], "precision": P,
            "recall": R, "fscore": f, "n_pred": n_p, "n_gt": n_g}
