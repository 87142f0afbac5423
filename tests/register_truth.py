"""Restatements of gsrast.register in numpy and plain Python floats, operation by operation (no torch): what include/gsrast.h defines under
"registration".  transform(), solve() and crop() restate the device's arithmetic exactly (IEEE float64, one rounding per operation, no fused
multiply-add) and are compared for equality; sums() is the exact sum (math.fsum) the device's fixed-order sums are held to within a tolerance; icp()
is the loop of the header around them and chamfer_truth.nearest."""
import math

import numpy as np

import chamfer_truth

ERR_INDEX, ERR_DEGENERATE = 1, 2
SWEEPS = 32                                               # GSR_REG_SWEEPS
MAX_POLYGON = 1024
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
AXES = {"X": 0, "Y": 1, "Z": 2}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def transform(points, M):
    """float32 [N,3]: ((m00 x + m01 y) + m02 z) + m03 in float64, rounded to float32 once."""
    p = _f32(points).astype(np.float64)
    M = np.asarray(M, np.float64)
    with np.errstate(all="ignore"):
        cols = [((M[a, 0] * p[:, 0] + M[a, 1] * p[:, 1]) + M[a, 2] * p[:, 2]) + M[a, 3] for a in range(3)]
        return np.stack(cols, axis=1).astype(np.float32).reshape(-1, 3)


def pairs(source, target, index):
    """(p float64 [n,3], q float64 [n,3], status): the pairs with index >= 0; an index outside [-1, T) sets ERR_INDEX and is no pair."""
    s, t = _f32(source), _f32(target)
    idx = np.asarray(index, np.int64).reshape(-1)
    bad = (idx < -1) | (idx >= len(t))
    ok = (idx >= 0) & ~bad
    return s[ok].astype(np.float64), t[idx[ok]].astype(np.float64), (ERR_INDEX if bad.any() else 0)


def _fsum_cols(a):
    return np.array([math.fsum(a[:, k].tolist()) for k in range(a.shape[1])], np.float64)


def centred(p, q, mean_p, mean_q):
    """(H [3,3], spp, sqq, and the sums of the absolute values of their terms) about the GIVEN means: every term is formed as the header forms it, the
    terms are added exactly."""
    dp, dq = p - np.asarray(mean_p, np.float64)[None, :], q - np.asarray(mean_q, np.float64)[None, :]
    H, Habs = np.zeros((3, 3)), np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            term = dp[:, a] * dq[:, b]
            H[a, b] = math.fsum(term.tolist()); Habs[a, b] = math.fsum(np.abs(term).tolist())
    spp = math.fsum(((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]).tolist())
    sqq = math.fsum(((dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2]).tolist())
    return H, spp, sqq, Habs


def sums(source, target, index):
    """The record of correspondence_sums as a dict: status, n, sum_p, sum_q, mean_p, mean_q, H, spp, sqq -- two passes, exact sums."""
    p, q, status = pairs(source, target, index)
    n = len(p)
    sum_p, sum_q = (_fsum_cols(p), _fsum_cols(q)) if n else (np.zeros(3), np.zeros(3))
    mean_p, mean_q = (sum_p / float(n), sum_q / float(n)) if n else (np.zeros(3), np.zeros(3))
    H, spp, sqq, _ = centred(p, q, mean_p, mean_q)
    return dict(status=status, n=n, sum_p=sum_p, sum_q=sum_q, mean_p=mean_p, mean_q=mean_q, H=H, spp=spp, sqq=sqq)


def sums_one_pass(source, target, index):
    """H, spp, sqq from raw moments in one pass, H = sum p q^T - n pm qm^T: what the two passes are there to avoid."""
    p, q, _ = pairs(source, target, index)
    n = float(len(p))
    pm, qm = p.sum(axis=0) / n, q.sum(axis=0) / n
    return p.T @ q - n * np.outer(pm, qm), float((p * p).sum() - n * (pm * pm).sum()), float((q * q).sum() - n * (qm * qm).sum())


def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))      # a float product overflows to inf without raising: t = 0
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = A[p][p] - t * apq
    A[q][q] = A[q][q] + t * apq
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r != p and r != q:
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
        vrp, vrq = V[r][p], V[r][q]
        V[r][p] = c * vrp - s * vrq
        V[r][q] = s * vrp + c * vrq


def solve(rec, with_scaling=False):
    """(M float64 [4,4] or None, status): the header's gsr_solve_transform on a record (a dict with n, H, spp, sqq, mean_p, mean_q) in Python floats.
    Degenerate: (None, ERR_DEGENERATE) -- the device leaves its matrix as it is."""
    n, spp, sqq = int(rec["n"]), float(rec["spp"]), float(rec["sqq"])
    if n < 3 or spp == 0.0 or sqq == 0.0:
        return None, ERR_DEGENERATE
    H = [[float(x) for x in row] for row in np.asarray(rec["H"], np.float64).reshape(3, 3)]
    pm, qm = [float(x) for x in rec["mean_p"]], [float(x) for x in rec["mean_q"]]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (H[0][0] + H[1][1]) + H[2][2]
    A[1][1] = (H[0][0] - H[1][1]) - H[2][2]
    A[2][2] = (H[1][1] - H[0][0]) - H[2][2]
    A[3][3] = (H[2][2] - H[0][0]) - H[1][1]
    A[0][1] = A[1][0] = H[1][2] - H[2][1]
    A[0][2] = A[2][0] = H[2][0] - H[0][2]
    A[0][3] = A[3][0] = H[0][1] - H[1][0]
    A[1][2] = A[2][1] = H[0][1] + H[1][0]
    A[1][3] = A[3][1] = H[2][0] + H[0][2]
    A[2][3] = A[3][2] = H[1][2] + H[2][1]
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    for _ in range(SWEEPS):
        if all(A[p][q] == 0.0 for p, q in PAIRS):
            break
        for p, q in PAIRS:
            _rotate(A, V, p, q)
    best = 0
    for a in range(1, 4):
        if A[a][a] > A[best][best]:
            best = a
    e = [V[a][best] for a in range(4)]
    norm = math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
    e = [x / norm for x in e]
    for a in range(4):
        if e[a] == 0.0:
            continue
        if e[a] < 0.0:
            e = [-x for x in e]
        break
    w, x, y, z = e
    ww, xx, yy, zz, xy, xz, yz, wx, wy, wz = w * w, x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [[((ww + xx) - yy) - zz, 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), ((ww - xx) + yy) - zz, 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), ((ww - xx) - yy) + zz]]
    scale = 1.0
    if with_scaling:
        acc = 0.0
        for a in range(3):
            for b in range(3):
                acc += R[a][b] * H[b][a]
        scale = acc / spp
    M = np.zeros((4, 4), np.float64)
    for a in range(3):
        rp = (R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2]
        for b in range(3):
            M[a, b] = scale * R[a][b] if with_scaling else R[a][b]
        M[a, 3] = qm[a] - (scale * rp if with_scaling else rp)
    M[3, 3] = 1.0
    return M, 0


def fit(source, target, with_scaling=False):
    s = _f32(source)
    return solve(sums(s, target, np.arange(len(s))), with_scaling)


def evaluate(d2, idx):
    """(n, fitness, rmse) of one query result."""
    ok = idx >= 0
    n = int(ok.sum())
    return n, n / float(len(idx)), (math.sqrt(math.fsum(d2[ok].astype(np.float64).tolist()) / float(n)) if n else 0.0)


def icp(source, target, cap, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, with_scaling=False, perturb=0.0):
    """The loop of the header -> dict(transformation, fitness, inlier_rmse, n_inliers, iterations, converged, status, trace), trace = one
    (n_k, fitness_k, rmse_k) per evaluation.  perturb: every sum of every record is multiplied by 1 + perturb * (+1 or -1, alternating by its place
    in the record) before the solve -- how far a transformation moves when its sums move by that relative amount."""
    s, t = _f32(source), _f32(target)
    M = np.eye(4) if init is None else np.array(init, np.float64)
    trace, k, converged, status = [], 0, False, 0
    while True:
        d2, idx = chamfer_truth.nearest(transform(s, M), t, cap)
        trace.append(evaluate(d2, idx))
        if k > 0 and abs(trace[-1][1] - trace[-2][1]) < relative_fitness and abs(trace[-1][2] - trace[-2][2]) < relative_rmse:
            converged = True
            break
        if k == max_iteration:
            break
        rec = sums(s, t, idx)
        if perturb:
            sign = iter([1.0, -1.0] * 16)
            for key in ("mean_p", "mean_q", "H"):
                rec[key] = rec[key] * (1.0 + perturb * np.array([next(sign) for _ in range(rec[key].size)]).reshape(rec[key].shape))
            rec["spp"] *= 1.0 + perturb; rec["sqq"] *= 1.0 - perturb
        Mn, st = solve(rec, with_scaling)
        if st:
            status = st
            break
        M, k = Mn, k + 1
    n, fitness, rmse = trace[-1]
    return dict(transformation=M, fitness=fitness, inlier_rmse=rmse, n_inliers=n, iterations=k, converged=converged, status=status, trace=trace)


def crop(points, polygon, axis, axis_min, axis_max):
    """bool [N]: finite, axis_min <= w <= axis_max, and an odd number of crossed edges a -> b (vertex k - 1 to vertex k):
    (a.v > v) != (b.v > v) and u < ((b.u - a.u) * (v - a.v)) / (b.v - a.v) + a.u, in float64.  polygon: [K,2] (u, v) or [K,3]."""
    ax = AXES[axis]
    p = _f32(points)
    poly = np.asarray(polygon, np.float64)
    if poly.shape[1] == 3:
        poly = poly[:, [a for a in range(3) if a != ax]]
    iu, iv = [a for a in range(3) if a != ax]
    w, u, v = (p[:, k].astype(np.float64) for k in (ax, iu, iv))
    with np.errstate(all="ignore"):
        inside = np.isfinite(p).all(axis=1) & (axis_min <= w) & (w <= axis_max)
        odd = np.zeros(len(p), bool)
        K = len(poly)
        for k in range(K):
            a, b = poly[k - 1], poly[k]
            straddles = (a[1] > v) != (b[1] > v)
            x = ((b[0] - a[0]) * (v - a[1])) / (b[1] - a[1]) + a[0]
            odd ^= straddles & (u < x)
    return inside & odd


def crop_by_angles(points, polygon, axis, axis_min, axis_max):
    """The same set by another route, for points that are not on the boundary: the winding of the polygon about the point, summed from the signed
    angles its edges subtend; inside under the even-odd rule for a simple polygon iff the winding number is odd."""
    ax = AXES[axis]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    poly = np.asarray(polygon, np.float64)
    if poly.shape[1] == 3:
        poly = poly[:, [a for a in range(3) if a != ax]]
    iu, iv = [a for a in range(3) if a != ax]
    d = poly[None, :, :] - p[:, None, [iu, iv]]
    e = np.roll(d, -1, axis=1)
    ang = np.arctan2(d[..., 0] * e[..., 1] - d[..., 1] * e[..., 0], d[..., 0] * e[..., 0] + d[..., 1] * e[..., 1]).sum(axis=1)
    wind = np.rint(ang / (2.0 * math.pi)).astype(np.int64)
    return (wind % 2 != 0) & (p[:, ax] >= axis_min) & (p[:, ax] <= axis_max)


def kabsch(p, q, with_scaling=False):
    """The SVD solution (Kabsch / Umeyama) of the same least-squares problem, for comparison with solve(): an independent formulation."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    dp, dq = p - pm, q - qm
    U, S, Vt = np.linalg.svd(dq.T @ dp)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = float((S * np.diag(D)).sum() / (dp * dp).sum()) if with_scaling else 1.0
    M = np.eye(4)
    M[:3, :3] = s * R
    M[:3, 3] = qm - s * R @ pm
    return M
