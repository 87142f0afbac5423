"""A reconstruction registered to its ground-truth scan on the device, the step between gsrast.mesh.cull_unseen_triangles and
gsrast.chamfer.surface_distance for a scene that lives in an arbitrary similarity frame (COLMAP poses, Tanks and Temples): the similarity fit of
corresponding points, point-to-point ICP, the crop to the scene's polygon volume (include/gsrast.h, "registration"; kernels in
csrc/gsr_register.hip; the whole recipe in INTEGRATION.md 4g).  Open3D 0.18's registration_icp,
TransformationEstimationPointToPoint and SelectionPolygonVolume are the model; parity with them is not pinned: every result is DEFINED in
include/gsrast.h and held to an operation-by-operation restatement (tests/register_truth.py).

    transform_points       p' = M p in float64, rounded to float32 once
    correspondence_sums    the two-pass float64 sums of corresponding pairs, in a fixed order -> a record on the device
    solve_transform        the record -> the least-squares rotation (Horn's quaternion method), translation and, where asked for, scale
    fit_transform          the two over rows i <-> i: the alignment of camera centres
    icp                    point-to-point ICP, the whole loop enqueued at once, one host read-back
    evaluate_registration  its evaluation alone
    crop_polygon_volume    the mask of the points inside a polygon extruded along an axis

A transformation is a float64 [4,4] in Open3D's COLUMN-vector convention, p' = M[:3,:3] p + M[:3,3] with the bottom row (0,0,0,1).  This is NOT
the row-vector convention of the cameras' full_proj_transform / world_view_transform in this repository (p' = p M): transpose those before they
meet these functions.  There is no CPU path: tensors that are not on a HIP device raise, like gsrast.chamfer."""
import ctypes as C
import math
import operator

import torch

from . import call, lib, scratch
from .chamfer import NearestGrid, _max_dist, _points  # noqa: F401  (NearestGrid is the search an ICP runs on)

ERR_INDEX, ERR_DEGENERATE = 1, 2                          # include/gsrast.h GSR_REG_ERR_*
SWEEPS = 32                                               # GSR_REG_SWEEPS: Jacobi sweeps at most
MAX_POLYGON = 1024                                        # GSR_REG_MAX_POLYGON
MAX_ITERATION = 4096                                      # GSR_REG_MAX_ITERATION
RECORD_WORDS = 48                                         # GSR_REG_RECORD_WORDS, and the GSR_REG_R_* indices of its 64-bit words:
R_STATUS, R_N, R_SUM_P, R_SUM_Q, R_MEAN_P, R_MEAN_Q, R_H, R_SPP, R_SQQ, R_M = 0, 1, 2, 5, 8, 11, 14, 23, 24, 25
R_FITNESS, R_RMSE, R_INLIERS, R_ITERATIONS, R_CONVERGED, R_STOP, R_SUM_D2 = 41, 42, 43, 44, 45, 46, 47
LAUNCHES_PER_ITERATION = 9                                # transform, query, evaluation (2), sums (4), solve


def _host_f64(x):
    """A tensor, an array or nested lists -> a float64 host tensor; lists of Python floats keep their 53 bits (torch.as_tensor alone would make them float32)."""
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", torch.float64)
    return torch.as_tensor(x, dtype=torch.float64)


def _matrix(M, name="transformation"):
    """A finite float64-convertible [4,4] -> (ctypes double[16], host float64 tensor); anything else is a ValueError."""
    try:
        m = _host_f64(M)
    except Exception as e:
        raise ValueError(f"{name} must be convertible to a float64 [4, 4] matrix: {e}") from None
    if tuple(m.shape) != (4, 4):
        raise ValueError(f"{name}: expected shape [4, 4] but found {list(m.shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError(f"{name} has a non-finite element")
    m = m.contiguous()
    return (C.c_double * 16)(*m.reshape(-1).tolist()), m


def transform_points(points, transformation):
    """-> float32 [N,3]: x' = ((m00 x + m01 y) + m02 z) + m03, likewise y' and z', in float64 on the widened float32 input, every operation rounded
    on its own and the result rounded to float32 once; non-finite coordinates come out as the arithmetic gives them.  transformation: float64 [4,4]
    in the column-vector convention of the module docstring (NOT the row-vector one of full_proj_transform); its bottom row is not read.  points:
    float32 [N,3] on a HIP device, any strides and any 4-byte alignment.  Host synchronisations per call: 0."""
    m, _ = _matrix(transformation)
    p = _points(points, "points")
    N, dev = int(p.shape[0]), p.device
    out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    call("gsr_transform_points", dev, p if N else None, N, m, out if N else None)
    return out


def _index(index, n, dev):
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or int(index.shape[0]) != n:
        raise RuntimeError(f"index: expected an int32 tensor of shape [{n}]")
    if index.device != dev:
        raise RuntimeError("index must be on the device of source")
    return index.contiguous()


def correspondence_sums(source, target, index):
    """-> the record, an int64 [RECORD_WORDS] tensor on the device (read_record() reads it): over the pairs (p, q) = (source[i], target[index[i]])
    with index[i] >= 0, float64 in two passes so that a cloud at 1e4 with an extent of 1 keeps its digits:
        n, sum p, sum q, the means pm = sum p / n and qm = sum q / n;   then with those means
        H[a][b] = sum (p - pm)_a (q - qm)_b,   Spp = sum |p - pm|^2,   Sqq = sum |q - qm|^2.
    The additions run in a fixed order that depends on N alone and there are no float atomics: two runs give the same bits.  index: int32 [N];
    -1 = no pair; any other value outside [0, T) sets ERR_INDEX, which read_record() and solve_transform() raise on.
    Host synchronisations per call: 0 (the record stays on the device)."""
    s, t = _points(source, "source"), _points(target, "target")
    if s.device != t.device:
        raise RuntimeError("source and target must be on one device")
    N, T, dev = int(s.shape[0]), int(t.shape[0]), s.device
    idx = _index(index, N, dev)
    record = torch.empty(RECORD_WORDS, dtype=torch.int64, device=dev)
    nbytes = int(lib().gsr_correspondence_sums_scratch_bytes(N))
    if nbytes == 0:
        raise RuntimeError(f"gsrast.register: {N} points out of range: every count must stay below 2^31")
    call("gsr_correspondence_sums", dev, s if N else None, N, t if T else None, T, idx if N else None, record, scratch(nbytes, dev), nbytes)
    return record


def read_record(record):
    """The record of correspondence_sums / solve_transform / icp on the host, as a dict (one host synchronisation).  Raises on ERR_INDEX."""
    host = record.cpu()                                   # the host read-back
    f = host.view(torch.float64)
    status = int(host[R_STATUS]) & 0xFFFFFFFF
    if status & ERR_INDEX:
        raise RuntimeError("gsrast.register: an index lies outside [-1, number of targets)")
    v3 = lambda k: f[k:k + 3].clone()
    return {"status": status, "n": int(host[R_N]), "sum_p": v3(R_SUM_P), "sum_q": v3(R_SUM_Q), "mean_p": v3(R_MEAN_P), "mean_q": v3(R_MEAN_Q),
            "H": f[R_H:R_H + 9].reshape(3, 3).clone(), "spp": float(f[R_SPP]), "sqq": float(f[R_SQQ]), "transformation": f[R_M:R_M + 16].reshape(4, 4).clone(),
            "fitness": float(f[R_FITNESS]), "inlier_rmse": float(f[R_RMSE]), "n_inliers": int(host[R_INLIERS]), "iterations": int(host[R_ITERATIONS]),
            "converged": bool(int(host[R_CONVERGED])), "sum_d2": float(f[R_SUM_D2])}


def solve_transform(record, with_scaling=False):
    """-> float64 [4,4] on the host: the M that takes the sources of the record onto its targets in the least-squares sense, q ~ s R p + t, written into
    the record too.  Horn's method: the symmetric 4x4 matrix of H is diagonalised by cyclic Jacobi rotations in a fixed pair order (at most SWEEPS
    sweeps), the eigenvector of its largest eigenvalue is the rotation's quaternion, so R is always a proper rotation (no determinant fix-up as after
    an SVD); s = 1, or with with_scaling Umeyama's sum_ab R_ab H_ba / Spp; t = qm - s R pm.  One wave, float64, no FMA contraction: the header
    writes every formula out and the result is reproducible bit for bit.
    Degenerate records (n < 3, Spp == 0 or Sqq == 0) set ERR_DEGENERATE in the record's status and leave its matrix as it is (the identity after
    correspondence_sums), which is returned.  Collinear pairs are NOT flagged: the rotation about their line is whatever the fixed order gives, and
    the result is still a rotation.  Host synchronisations per call: 1 (the record)."""
    if not isinstance(record, torch.Tensor) or not record.is_cuda or record.dtype != torch.int64 or tuple(record.shape) != (RECORD_WORDS,) or not record.is_contiguous():
        raise RuntimeError(f"record: expected the contiguous int64 [{RECORD_WORDS}] device tensor of correspondence_sums")
    call("gsr_solve_transform", record.device, record, int(bool(with_scaling)))
    return read_record(record)["transformation"]


def fit_transform(source, target, with_scaling=False):
    """-> float64 [4,4]: correspondence_sums + solve_transform over corresponding rows, source[i] <-> target[i]: the alignment of a
    reconstruction's camera centres with the ground truth's (with_scaling=True for a COLMAP frame).  Raises where the fit is degenerate (fewer
    than 3 rows, or all rows of a side equal).  Host synchronisations per call: 1."""
    s = _points(source, "source")
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != tuple(s.shape):
        raise RuntimeError(f"target: expected the shape of source, {list(s.shape)}")
    N = int(s.shape[0])
    record = correspondence_sums(s, target, torch.arange(N, dtype=torch.int32, device=s.device))
    call("gsr_solve_transform", record.device, record, int(bool(with_scaling)))
    r = read_record(record)
    if r["status"] & ERR_DEGENERATE:
        raise RuntimeError(f"fit_transform: degenerate: {N} rows, of which a fit needs at least 3 that are not all equal on either side")
    return r["transformation"]


class RegistrationResult:
    """What icp() and evaluate_registration() return: transformation (float64 [4,4], host), fitness (inliers / sources), inlier_rmse, n_inliers --
    the last three evaluated WITH that transformation --, iterations (solves done), converged, status (0 or ERR_DEGENERATE)."""

    def __init__(self, transformation, fitness, inlier_rmse, n_inliers, iterations, converged, status):
        self.transformation, self.fitness, self.inlier_rmse, self.n_inliers = transformation, fitness, inlier_rmse, n_inliers
        self.iterations, self.converged, self.status = iterations, converged, status

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.6g}, inlier_rmse={self.inlier_rmse:.6g}, n_inliers={self.n_inliers}, iterations={self.iterations}, "
                f"converged={self.converged}, status={self.status})")


def _threshold(x, name):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number but found {x!r}") from None
    if not (v >= 0.0) or math.isinf(v):
        raise ValueError(f"{name} must be a non-negative finite number but found {x}")
    return v


def icp(source, target, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, with_scaling=False):
    """Point-to-point ICP of source [N,3] against target [T,3] -> RegistrationResult.
        M_0 = init or the identity; the grid over target is built ONCE, with the cap float32(max_correspondence_distance)
        k = 0, 1, ...:  P_k = transform_points(source, M_k)   -- always of the ORIGINAL source: no drift, no composition
                        (d2, idx) = the nearest target of every P_k within the cap; n_k = #{idx >= 0}; fitness_k = n_k / N;
                        rmse_k = sqrt(sum float64(d2) / n_k) over them (0 where n_k = 0)
                        k > 0 and |fitness_k - fitness_(k-1)| < relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse  -> converged, stop
                        k == max_iteration                                                                                  -> stop, not converged
                        record = correspondence_sums(source, target, idx); degenerate -> stop with status ERR_DEGENERATE
                        M_(k+1) = solve_transform(record, with_scaling)
    The result's transformation is the M_k at the stop, and fitness, inlier_rmse and n_inliers were evaluated with it.  Solving the absolute
    transformation from the original source, where Open3D composes increments onto a moved copy, is a stated departure; the fixed points are the
    same.  max_iteration=0 is the evaluation alone (evaluate_registration).
    The whole loop is enqueued at once: the build, then LAUNCHES_PER_ITERATION = 9 launches per iteration and 4 for the last evaluation, a number
    fixed by max_iteration; after the stop the remaining launches return at their first instruction on a flag in the record.
    Host synchronisations per call: exactly 1, whatever max_iteration (the record).
    ValueError before any launch: a negative or non-finite distance or threshold, a max_iteration that is negative, not an integer or above
    MAX_ITERATION = 4096, an init that is not a finite float64-convertible [4,4], an empty source."""
    md = _max_dist(max_correspondence_distance)
    if md < 0:
        raise ValueError("max_correspondence_distance must be a non-negative finite number, not None")
    rf, rr = _threshold(relative_fitness, "relative_fitness"), _threshold(relative_rmse, "relative_rmse")
    try:
        max_iteration = operator.index(max_iteration) if not isinstance(max_iteration, bool) else None
    except TypeError:
        max_iteration = None
    if max_iteration is None or not 0 <= max_iteration <= MAX_ITERATION:
        raise ValueError(f"max_iteration must be an integer in [0, {MAX_ITERATION}]")
    m0, _ = _matrix(init if init is not None else torch.eye(4, dtype=torch.float64), "init")
    s, t = _points(source, "source"), _points(target, "target")
    if s.device != t.device:
        raise RuntimeError("source and target must be on one device")
    N, T, dev = int(s.shape[0]), int(t.shape[0]), s.device
    if N == 0:
        raise ValueError("source is empty")
    nbytes = int(lib().gsr_icp_scratch_bytes(N, T))
    if nbytes == 0:
        raise RuntimeError(f"gsrast.register: sizes {(N, T)} out of range: every count must stay below 2^31")
    record = torch.empty(RECORD_WORDS, dtype=torch.int64, device=dev)
    call("gsr_icp", dev, s, N, t if T else None, T, md, m0, max_iteration, rf, rr, int(bool(with_scaling)), record, scratch(nbytes, dev), nbytes)
    r = read_record(record)                               # the host read-back
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["n_inliers"], r["iterations"], r["converged"], r["status"])


def evaluate_registration(source, target, max_correspondence_distance, transformation=None):
    """icp(..., init=transformation, max_iteration=0): fitness, inlier_rmse and n_inliers of a given transformation.  1 host synchronisation."""
    return icp(source, target, max_correspondence_distance, init=transformation, max_iteration=0)


_AXES = {"X": 0, "Y": 1, "Z": 2}


def crop_polygon_volume(points, bounding_polygon, orthogonal_axis, axis_min, axis_max):
    """-> bool [N] on the device: the points inside the polygon extruded along an axis, the SelectionPolygonVolume of a Tanks-and-Temples crop
    JSON (its fields are the arguments).  bounding_polygon: float64-convertible [K,2], or [K,3] as the JSON stores it, where the coordinate along
    the axis is ignored; 3 <= K <= MAX_POLYGON = 1024.  orthogonal_axis: "X", "Y" or "Z"; the in-plane axes (u, v) are the other two in
    ascending order.  A point is kept iff it is finite, axis_min <= w <= axis_max and the even-odd crossing number over the K edges is odd; an edge
    a -> b is crossed iff (a.v > v) != (b.v > v) and u < ((b.u - a.u) (v - a.v)) / (b.v - a.v) + a.u, in float64 -- half-open in v, so that a vertex
    two edges share counts once.  The polygon is held in LDS.  Host synchronisations per call: 0."""
    axis = _AXES.get(orthogonal_axis.upper() if isinstance(orthogonal_axis, str) else orthogonal_axis)
    if axis is None:
        raise ValueError(f"orthogonal_axis must be 'X', 'Y' or 'Z' but found {orthogonal_axis!r}")
    lo, hi = float(axis_min), float(axis_max)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError("axis_min or axis_max is NaN")
    try:
        poly = _host_f64(bounding_polygon)
    except Exception as e:
        raise ValueError(f"bounding_polygon must be convertible to float64 [K, 2] or [K, 3]: {e}") from None
    if poly.dim() != 2 or poly.shape[1] not in (2, 3):
        raise ValueError(f"bounding_polygon: expected shape [K, 2] or [K, 3] but found {list(poly.shape)}")
    if poly.shape[1] == 3:
        poly = poly[:, [a for a in range(3) if a != axis]]
    K = int(poly.shape[0])
    if not 3 <= K <= MAX_POLYGON:
        raise ValueError(f"bounding_polygon has {K} vertices: 3 to {MAX_POLYGON} are possible")
    if not bool(torch.isfinite(poly).all()):
        raise ValueError("bounding_polygon has a non-finite coordinate")
    p = _points(points, "points")
    N, dev = int(p.shape[0]), p.device
    keep = torch.empty(N, dtype=torch.bool, device=dev)
    nbytes = int(lib().gsr_crop_polygon_scratch_bytes())
    call("gsr_crop_polygon_volume", dev, p if N else None, N, (C.c_double * (2 * K))(*poly.reshape(-1).tolist()), K, axis, lo, hi, keep if N else None,
         scratch(nbytes, dev), nbytes)
    return keep
