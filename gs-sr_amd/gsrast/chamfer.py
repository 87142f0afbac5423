"""An extracted mesh held against a ground-truth cloud on the device: accuracy, completeness, Chamfer distance and F-score, the DTU /
Tanks-and-Temples shape of evaluation (include/gsrast.h, "surface distance"; kernels in csrc/gsr_chamfer.hip).  The reference
tree ships no evaluation -- the 2DGS and PGSR repositories do, as host scripts over a KD-tree -- so nothing here has a line to be held against
there: every result is DEFINED in include/gsrast.h and held to an operation-by-operation restatement (tests/chamfer_truth.py).

    nearest_points     exact cross-set nearest neighbour (float32 d2, lowest index among ties) through a uniform grid over the targets
    NearestGrid        that grid built once and queried many times
    sample_surface     deterministic samples of a triangle mesh: n^2 sub-triangle centroids per triangle
    voxel_downsample   one point per occupied cell, the one with the lowest index
    surface_distance   the four figures and the F-score per threshold, float64 sums in a fixed order

voxel_downsample stands where the host scripts thin a cloud greedily by radius (a point stays iff no point kept before it lies within the
radius): that rule is sequential by definition and is NOT reproduced; the cell rule gives the same even density and does not depend on an order
of visits.  There is no CPU path: tensors that are not on a HIP device raise, like gsrast.mesh."""
import ctypes as C
import math

import torch

from . import call, lib, scratch

ERR_INDEX, ERR_CAP, ERR_RANGE = 1, 2, 4                   # include/gsrast.h GSR_CHAMFER_ERR_*
MAX_N = 1024                                              # GSR_SAMPLE_MAX_N: sub-divisions of one triangle's edges at most
MAX_THRESHOLDS = 8                                        # GSR_CHAMFER_MAX_THRESHOLDS
CELL_RANGE = 1 << 20                                      # voxel_downsample: cells per axis inside [-2^20, 2^20)


def _points(t, name):
    """A float32 [n,3] tensor on a HIP device, any strides and any 4-byte alignment (what distCUDA2 accepts) -> its packed form."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected scalar type Float but found {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{name}: expected shape [n, 3] but found {list(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor: gsrast.chamfer has no CPU path")
    return t.detach().contiguous()


def _max_dist(max_dist):
    """None -> -1.0 (the library's "no cap"); else the float32 the kernels compare with, as a Python float."""
    if max_dist is None:
        return -1.0
    m = float(max_dist)
    if not (m >= 0.0) or math.isinf(m):
        raise ValueError(f"max_dist must be a non-negative finite number or None but found {max_dist}")
    return C.c_float(m).value


def _scratch(query_fn, dev, *n):
    nbytes = int(getattr(lib(), query_fn)(*n))
    if nbytes == 0:
        raise RuntimeError(f"gsrast.chamfer: sizes {n} out of range: every count must stay below 2^31")
    return scratch(nbytes, dev), nbytes


def nearest_points(query, target, max_dist=None):
    """-> (d2 float32 [Q], index int32 [Q]): for every row of query [Q,3] the nearest row of target [T,3], bit for bit what the float32 all-pairs
    search gives: d2 = (dx*dx + dy*dy) + dz*dz with dx = t.x - q.x, every operation rounded on its own; among equal d2 the lowest target index.
    max_dist: a target counts only if d2 <= float32(max_dist)^2 (equality stays in).  A target with a non-finite coordinate never counts; a query
    with one, or with no counting target (T == 0 included), gets (+inf, -1).
    The search is a uniform grid over the targets (cell size from their extent and count, decided on the device, at least max_dist), shells of
    cells outward from the query's cell with conservative pruning; a query whose shells run out (far outside the targets' box with max_dist=None,
    say) falls back to a scan of the targets' 256-point boxes, so its cost is bounded and its result exact.
    Host synchronisations per call: 0."""
    md = _max_dist(max_dist)
    q, t = _points(query, "query"), _points(target, "target")
    if q.device != t.device:
        raise RuntimeError("query and target must be on one device")
    Q, T, dev = int(q.shape[0]), int(t.shape[0]), q.device
    d2 = torch.empty(Q, dtype=torch.float32, device=dev)
    index = torch.empty(Q, dtype=torch.int32, device=dev)
    work, nbytes = _scratch("gsr_nearest_points_scratch_bytes", dev, Q, T)
    call("gsr_nearest_points", dev, q if Q else None, Q, t if T else None, T, md, d2 if Q else None, index if Q else None, work, nbytes)
    return d2, index


class NearestGrid:
    """The search of nearest_points in its two halves: NearestGrid(target, max_dist) builds the grid over the targets once, .query(points) asks it any
    number of times -- what an ICP against a fixed scan needs (gsrast.register).  query(q) gives the bits of nearest_points(q, target, max_dist):
    the launches are the same.  The cap of a query is the cap of the build, because the cell size depends on it.  The grid keeps its own sorted copy
    of the targets: the tensor handed in is not read again.  Host synchronisations: 0, build and query."""

    def __init__(self, target, max_dist=None):
        self.max_dist = _max_dist(max_dist)
        t = _points(target, "target")
        self.n_target, self.device = int(t.shape[0]), t.device
        self._work, self._nbytes = _scratch("gsr_nearest_grid_scratch_bytes", self.device, self.n_target)
        call("gsr_nearest_grid_build", self.device, t if self.n_target else None, self.n_target, self.max_dist, self._work, self._nbytes)

    def query(self, points, skip=None, out=None):
        """-> (d2 float32 [Q], index int32 [Q]) as nearest_points gives them.  skip: an int32 [1] tensor on the device; while its word is non-zero every
        workgroup returns at once and the outputs stay as they are -- `out`, a (d2, index) pair of a former call, is then where they are."""
        q = _points(points, "points")
        if q.device != self.device:
            raise RuntimeError("points must be on the device of the grid's targets")
        Q = int(q.shape[0])
        if out is None:
            out = (torch.empty(Q, dtype=torch.float32, device=self.device), torch.empty(Q, dtype=torch.int32, device=self.device))
        d2, index = out
        if d2.dtype != torch.float32 or index.dtype != torch.int32 or tuple(d2.shape) != (Q,) or tuple(index.shape) != (Q,):
            raise RuntimeError(f"out: expected a float32 [{Q}] and an int32 [{Q}] tensor")
        if skip is not None and (not isinstance(skip, torch.Tensor) or skip.dtype != torch.int32 or skip.numel() != 1):
            raise RuntimeError("skip: expected an int32 tensor of one element")
        if Q >= 1 << 31:
            raise RuntimeError(f"gsrast.chamfer: {Q} points out of range: every count must stay below 2^31")
        call("gsr_nearest_grid_query", self.device, q if Q else None, Q, self.n_target, self.max_dist, self._work, self._nbytes, d2 if Q else None,
             index if Q else None, skip)
        return d2, index


def _mesh_arrays(mesh):
    """(vertices, triangles) of a TriangleMesh or of any object with those two tensors, checked as gsrast.mesh._arrays checks them; colours
    are not needed."""
    v, t = getattr(mesh, "vertices", None), getattr(mesh, "triangles", None)
    for x, name, dt in ((v, "vertices", torch.float32), (t, "triangles", torch.int32)):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"mesh.{name} must be a tensor")
        if not x.is_cuda:
            raise RuntimeError(f"mesh.{name} must be a CUDA tensor: gsrast.chamfer has no CPU path")
        if x.dtype != dt or x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError(f"mesh.{name}: expected a {dt} tensor of shape [n, 3] but found {x.dtype} {list(x.shape)}")
    if v.device != t.device:
        raise RuntimeError("mesh: vertices and triangles must be on one device")
    return v.detach().contiguous(), t.contiguous()


def _spacing(spacing):
    s = float(spacing)
    if not (s > 0.0) or math.isinf(s):
        raise ValueError(f"spacing must be a positive finite number but found {spacing}")
    return s


def sample_surface(mesh, spacing):
    """-> float32 [S,3] deterministic samples of a mesh (gsrast.tsdf.TriangleMesh, or anything with `vertices` float32 [V,3] and `triangles`
    int32 [T,3] on a HIP device).  Per triangle (a, b, c): L2 = its largest float32 squared edge length, n = max(1, ceil(sqrt(float64(L2)) /
    float64(spacing))), and exactly n^2 points, the centroids of its n^2 congruent sub-triangles: row i = 0..n-1 holds the n - i "up" centroids at
    barycentric u = (i + 1/3) / n, v = (j + 1/3) / n, then the n - i - 1 "down" ones at u = (i + 2/3) / n, v = (j + 2/3) / n;
    p = a + u (b - a) + v (c - a) in float64, rounded to float32 once.  Triangle-major, then row, then that order.  No sample lies on an edge, and
    each stands for area / n^2.
    Raises (nothing is clamped): a triangle index outside [0, V); a triangle whose n exceeds MAX_N = 1024; 2^31 samples or more.
    spacing <= 0 or non-finite raises ValueError.  T == 0 gives an empty tensor.  Host synchronisations per call: 1 (status and total)."""
    s = _spacing(spacing)
    v, t = _mesh_arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    if T == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    work, nbytes = _scratch("gsr_sample_surface_scratch_bytes", dev, T)
    record = torch.empty(4, dtype=torch.int32, device=dev)
    call("gsr_sample_surface_count", dev, v if V else None, V, t, T, s, work, nbytes, record)
    rec = [x & 0xFFFFFFFF for x in record.tolist()]       # the host read-back
    if rec[0] & ERR_INDEX:
        raise RuntimeError("sample_surface: a triangle index lies outside [0, number of vertices)")
    if rec[0] & ERR_CAP:
        raise RuntimeError(f"sample_surface: a triangle's longest edge is more than {MAX_N} x spacing (or not finite): subdivide the mesh or sample it more coarsely")
    total = rec[2] | (rec[3] << 32)
    if total >= 1 << 31:
        raise RuntimeError(f"sample_surface: {total} samples reach 2^31: sample the mesh in parts or more coarsely")
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    call("gsr_sample_surface_emit", dev, v if V else None, V, t, T, s, work, nbytes, total, points)
    return points


def voxel_downsample(points, cell):
    """-> (points_kept float32 [K,3], kept_index int32 [K]): one point per occupied cell, the one with the lowest index; the cell of a point is
    floor(float64(p) / float64(cell)) per axis.  The output keeps the input order; kept_index points into the input.  Points with a non-finite
    coordinate are dropped; a cell coordinate outside [-2^20, 2^20) raises.  This is the even-density step of the evaluation; the host scripts'
    greedy radius thinning is sequential by definition and is not reproduced (module docstring).
    Host synchronisations per call: 1 (status and count)."""
    c = float(cell)
    if not (c > 0.0) or math.isinf(c):
        raise ValueError(f"cell must be a positive finite number but found {cell}")
    p = _points(points, "points")
    N, dev = int(p.shape[0]), p.device
    if N == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    work, nbytes = _scratch("gsr_voxel_downsample_scratch_bytes", dev, N)
    record = torch.empty(2, dtype=torch.int32, device=dev)
    call("gsr_voxel_downsample_count", dev, p, N, c, work, nbytes, record)
    status, kept = (x & 0xFFFFFFFF for x in record.tolist())          # the host read-back
    if status & ERR_RANGE:
        raise RuntimeError(f"voxel_downsample: a cell coordinate lies outside [-2^20, 2^20): the cell size {c} is too small for this cloud")
    out = torch.empty((kept, 3), dtype=torch.float32, device=dev)
    index = torch.empty(kept, dtype=torch.int32, device=dev)
    call("gsr_voxel_downsample_emit", dev, p, N, work, nbytes, kept, out if kept else None, index if kept else None)
    return out, index


def _direction(src, dst, md, taus):
    """(sum of d, [number of d < tau]) over the points of src against dst: one launch sequence, one read-back."""
    d2, _ = nearest_points(src, dst, None if md < 0 else md)
    n, dev = int(d2.shape[0]), d2.device
    record = torch.empty(1 + MAX_THRESHOLDS, dtype=torch.int64, device=dev)
    work, nbytes = _scratch("gsr_distance_stats_scratch_bytes", dev, n)
    call("gsr_distance_stats", dev, d2 if n else None, n, md, (C.c_double * max(len(taus), 1))(*taus), len(taus), record, work, nbytes)
    host = record.cpu()                                   # the host read-back
    return host[:1].view(torch.float64).item(), [int(x) for x in host[1:1 + len(taus)].tolist()]


def surface_distance(pred, gt, spacing=None, voxel=None, max_dist=None, thresholds=()):
    """-> dict: pred and gt are each a mesh (sampled with sample_surface(., spacing); spacing is then required) or a float32 [N,3] point tensor;
    either side is thinned with voxel_downsample(., voxel) where voxel is given.  With d = sqrt(float64(d2)) of nearest_points in both directions,
    clamped to float32(max_dist) where that is given (a sample with no target inside the cap counts as max_dist, the DTU convention):
        accuracy      mean d from pred to gt            completeness   mean d from gt to pred            chamfer   the mean of the two
        precision[i]  share of pred samples with d < thresholds[i]         recall[i]   share of gt samples likewise
        fscore[i]     2 P R / (P + R), 0 where both are 0
        n_pred, n_gt  the sample counts;   thresholds  as floats
    The sums are float64 in a fixed order: two calls give the same bits.  An empty side gives NaN means (and NaN shares) and raises nothing.
    At most MAX_THRESHOLDS = 8 thresholds.  Host synchronisations: 1 per direction for all its statistics, +1 per sampled mesh, +1 per thinned
    side."""
    taus = [float(t) for t in thresholds]
    if len(taus) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds per call but found {len(taus)}")
    if any(math.isnan(t) for t in taus):
        raise ValueError("a threshold is NaN")
    md = _max_dist(max_dist)

    def side(x, name):
        if not isinstance(x, torch.Tensor):
            if spacing is None:
                raise ValueError(f"{name} is a mesh: spacing is required")
            x = sample_surface(x, spacing)
        x = _points(x, name)
        return voxel_downsample(x, voxel)[0] if voxel is not None else x

    p, g = side(pred, "pred"), side(gt, "gt")
    if p.device != g.device:
        raise RuntimeError("pred and gt must be on one device")
    n_p, n_g = int(p.shape[0]), int(g.shape[0])
    sum_p, below_p = _direction(p, g, md, taus)
    sum_g, below_g = _direction(g, p, md, taus)
    nan = float("nan")
    acc, comp = (sum_p / n_p if n_p else nan), (sum_g / n_g if n_g else nan)
    precision = [b / n_p if n_p else nan for b in below_p]
    recall = [b / n_g if n_g else nan for b in below_g]
    fscore = [(2.0 * P * R / (P + R) if P + R > 0.0 else (0.0 if P + R == 0.0 else nan)) for P, R in zip(precision, recall)]
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "thresholds": taus, "precision": precision, "recall": recall,
            "fscore": fscore, "n_pred": n_p, "n_gt": n_g}
