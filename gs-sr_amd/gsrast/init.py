"""The first anchors from the point cloud, on the device (include/gsrast.h "anchors from the point cloud", csrc/gsr_init.hip).

Replaces the pieces of `OctreeGaussian.create_from_data` (gssr/gaussian/octree_gaussian.py:152-182 set_level, octree_sample) and of
`ScaffoldGaussian.create_from_data` (scaffold_gaussian.py:257-298 voxelize_sample) that the reference runs as torch.quantile per camera (two sorts
of N values each), torch.unique(dim=0) per level and np.unique(axis=0) on the host:

    camera_dist_quantiles   per camera the two interpolated order statistics of the point distances, times the camera's scale ("all_dist")
    quantile, kthvalue      torch.quantile (linear) / torch.kthvalue of a float32 array of any size
    set_level               cam_infos, standard_dist, levels, init_level                      one host read, whatever the number of cameras
    octree_sample           the distinct cells of every level, rows in torch.unique's order    one host read, whatever the number of levels
    voxelize_sample         np.unique(np.round(data / voxel_size), axis=0) * voxel_size, without the reference's in-place shuffle of `data`

Ranks follow ATen: rank = float32(q) * (n - 1) evaluated in float32 (at n = 100003, q = 0.999 it is 99902 exactly, one element, where the float64 rank 99901.998 takes two),
floor, ceil, weight = rank - floor, then ATen's Lerp.h (w < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w)) operation by operation.  The order statistics
equal torch's bit for bit; the interpolation equals torch.quantile's on the CPU at ATen's DEFAULT dispatch level (its AVX2 / AVX512 kernels fuse the
product-sum and differ in the last bit now and then; tests/test_gpu_create_anchors.py).  The distances are correctly rounded roots; torch.sqrt on the
CPU is not correctly rounded in its vectorised path (about 6 values in 1000 are one ulp off), so a host torch.quantile(torch.sqrt(...)) may differ by that.
The model-level calls that use these are gsrast.anchors.octree_create_from_data_ and gsrast.anchors.create_from_data_."""
import ctypes as C
import math

import numpy as np
import torch

from . import call, lib, one_device, raise_status, scratch, status_text
from ._rows import _f32

ERR_NONFINITE, ERR_KEY_RANGE, ERR_RANK = 1, 2, 4
MAX_LEVELS = 32


STATUS = {
    ERR_NONFINITE: "a non-finite value (NaN or infinity) in the input",
    ERR_KEY_RANGE: "a voxel key outside int32: (point - init_pos) / cell exceeds 2^31",
    ERR_RANK: "a rank beyond the number of elements",
}


def status_message(what, status):
    """The text of the status word of a gsr_init.hip entry point."""
    return status_text(what, status, STATUS)


def _raise_on(what, status):
    raise_status(what, int(status), STATUS)


def ranks(q, n):
    """-> (k_lo, k_hi, w): torch.quantile's two 0-based ranks and its float32 weight for quantile q of n elements, with ATen's own arithmetic
    (aten/src/ATen/native/Sorting.cpp quantile_compute: q as a 0-dim tensor of the input's dtype, times n - 1, floor, ceil, rank - floor)."""
    if not 0.0 <= float(q) <= 1.0:
        raise RuntimeError(f"quantile() q must be in the range [0, 1] but got {q}")
    rank = torch.tensor(float(q), dtype=torch.float32) * (int(n) - 1)
    lo = torch.floor(rank)
    return int(lo), int(torch.ceil(rank)), float(rank - lo)


def _rank_args(targets):
    n = len(targets)
    return ((C.c_int64 * n)(*[t[0] for t in targets]), (C.c_int64 * n)(*[t[1] for t in targets]), (C.c_float * n)(*[t[2] for t in targets]))


def _cam_quantiles(points, cam_infos, dist_ratio):
    """-> (all_dist [2C], status [1] uint32-as-int32), nothing read."""
    pts = _f32(points, "points", (None, 3))
    cams = _f32(cam_infos, "cam_infos", (None, 4))
    one_device(("points", pts), ("cam_infos", cams))
    N, Cn = pts.shape[0], cams.shape[0]
    if N < 1 or Cn < 1:
        raise RuntimeError(f"camera_dist_quantiles: expected at least one point and one camera but found {N} and {Cn}")
    lo, hi, w = _rank_args([ranks(1 - dist_ratio, N), ranks(dist_ratio, N)])          # all_dist = [dist_min, dist_max] per camera
    L = lib()
    out = torch.empty(2 * Cn, dtype=torch.float32, device=pts.device)
    status = torch.empty(1, dtype=torch.int32, device=pts.device)
    nbytes = int(L.gsr_cam_dist_quantiles_scratch_bytes(N, Cn))
    work = scratch(nbytes, pts.device)
    call("gsr_cam_dist_quantiles", pts.device, pts, N, cams, Cn, lo, hi, w, out, work, nbytes, status)
    return out, status


def camera_dist_quantiles(points, cam_infos, dist_ratio):
    """-> all_dist float32 [2C] = [min_0, max_0, min_1, max_1, ...]: for every camera (cam_infos [C,4]: centre, scale) what the reference's set_level
    appends, torch.quantile(dist, 1 - dist_ratio) * scale and torch.quantile(dist, dist_ratio) * scale over dist = |points - centre| (float32).  The
    C x N distances are never stored.  One host read (the status word)."""
    out, status = _cam_quantiles(points, cam_infos, dist_ratio)
    _raise_on("camera_dist_quantiles", int(status.item()))
    return out


def _select(values, targets):
    """-> (out [len(targets)], status [1]) for targets = [(k_lo, k_hi, w)], one or two; nothing read."""
    v = _f32(values, "values").reshape(-1)
    n = v.shape[0]
    if n < 1:
        raise RuntimeError("select: expected a non-empty tensor")
    lo, hi, w = _rank_args(targets)
    L = lib()
    out = torch.empty(len(targets), dtype=torch.float32, device=v.device)
    status = torch.empty(1, dtype=torch.int32, device=v.device)
    nbytes = int(L.gsr_select_lerp_scratch_bytes(n))
    work = scratch(nbytes, v.device)
    call("gsr_select_lerp", v.device, v, n, None, len(targets), lo, hi, w, out, work, nbytes, status)
    return out, status


def quantile(values, q):
    """-> 0-dim float32 tensor (q a number) or [2] (q a pair): torch.quantile(values, q) with linear interpolation over the flattened float32
    tensor, of any size (torch.quantile refuses more than 16 M elements).  A NaN raises.  One host read (the status word)."""
    qs = list(q) if isinstance(q, (list, tuple)) else [q]
    if len(qs) not in (1, 2):
        raise RuntimeError("quantile: one or two q")
    n = values.numel()
    out, status = _select(values, [ranks(x, n) for x in qs])
    _raise_on("quantile", int(status.item()))
    return out if isinstance(q, (list, tuple)) else out[0]


def kthvalue(values, k):
    """-> 0-dim float32 tensor: torch.kthvalue(values, k).values over the flattened float32 tensor, k 1-based.  A NaN raises.  One host read."""
    n = values.numel()
    if not 1 <= int(k) <= n:
        raise RuntimeError(f"kthvalue(): selected number k out of range for dimension 0: k={k}, size {n}")
    out, status = _select(values, [(int(k) - 1, int(k) - 1, 0.0)])
    _raise_on("kthvalue", int(status.item()))
    return out[0]


def camera_infos(cameras_by_scale, device):
    """-> cam_infos float32 [C,4] (centre, scale) in the reference's order (scales as the mapping lists them, cameras in their list's order).  A value of
    the mapping is a list of cameras (objects with .camera_center) or a tensor / array [n,3] of centres.  Nothing is read from the device."""
    rows = []
    for scale, cams in cameras_by_scale.items():
        if isinstance(cams, (torch.Tensor, np.ndarray)):
            centres = torch.as_tensor(cams).to(device=device, dtype=torch.float32).reshape(-1, 3)
        else:
            centres = torch.stack([torch.as_tensor(c.camera_center).to(device=device, dtype=torch.float32).reshape(3) for c in cams]) if len(cams) else \
                torch.empty(0, 3, dtype=torch.float32, device=device)
        rows.append(torch.cat((centres, torch.full((centres.shape[0], 1), float(scale), dtype=torch.float32, device=device)), dim=1))
    if not rows:
        raise RuntimeError("set_level: no cameras")
    return torch.cat(rows).contiguous()


def _set_level(points, cameras_by_scale, dist_ratio, fork, extra=()):
    """The device part of set_level and its ONE host read.  -> (cam_infos, (dist_min, dist_max) device [2], host list
    [round(log2(dist_max / dist_min) / log2(fork)), dist_min, dist_max, *extra]); `extra`: 0-dim tensors that ride along in the same read."""
    pts = _f32(points, "points", (None, 3))
    cams = camera_infos(cameras_by_scale, pts.device)
    all_dist, s1 = _cam_quantiles(pts, cams, dist_ratio)
    mm, s2 = _select(all_dist, [ranks(1 - dist_ratio, all_dist.numel()), ranks(dist_ratio, all_dist.numel())])
    lv = torch.round(torch.log2(mm[1] / mm[0]) / math.log2(fork))
    host = torch.cat([s1.to(torch.float64), s2.to(torch.float64), lv.reshape(1).to(torch.float64), mm.to(torch.float64)] +
                     [e.detach().reshape(1).to(torch.float64) for e in extra]).tolist()          # the one host read
    _raise_on("set_level (per-camera quantiles)", int(host[0]))
    _raise_on("set_level (quantiles of all_dist)", int(host[1]))
    return cams, mm, host[2:]


def set_level(points, cameras_by_scale, dist_ratio, fork, levels=-1, init_level=-1):
    """OctreeGaussian.set_level -> (cam_infos [C,4] float32, standard_dist 0-dim float32 device tensor, levels int, init_level int).
    cameras_by_scale: {resolution scale: cameras} as camera_infos takes it.  standard_dist = quantile(all_dist, dist_ratio); levels = -1 becomes
    round(log2(dist_max / dist_min) / log2(fork)) + 1, init_level = -1 becomes int(levels / 2).  One host read, whatever the number of cameras; the
    peak scratch is 4 KiB per camera (no C x N array)."""
    cams, mm, host = _set_level(points, cameras_by_scale, dist_ratio, fork)
    if levels == -1:
        if not math.isfinite(host[0]):
            raise RuntimeError("set_level: dist_max / dist_min is not a positive finite number, levels cannot be derived")
        levels = int(host[0]) + 1
    if init_level == -1:
        init_level = int(levels / 2)
    return cams, mm[1], int(levels), int(init_level)


def _host_floats(x, n, name):
    """n Python floats from a number, a sequence or a tensor (a device tensor costs a host read)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().reshape(-1).tolist()
    elif isinstance(x, np.ndarray):
        x = x.reshape(-1).tolist()
    elif not isinstance(x, (list, tuple)):
        x = [x]
    if len(x) != n:
        raise RuntimeError(f"{name}: expected {n} number(s) but found {len(x)}")
    return [float(v) for v in x]


def _voxel_unique(pts, init_pos, cells, what):
    """pts float32 | float64 [N,3] on the device; init_pos 3 host floats; cells host floats -> (positions float32 [U,3], level int32 [U], counts)."""
    N, Ln = pts.shape[0], len(cells)
    if N < 1:
        raise RuntimeError(f"{what}: expected at least one point")
    if not 1 <= Ln <= MAX_LEVELS:
        raise RuntimeError(f"{what}: expected 1 to {MAX_LEVELS} levels but found {Ln}")
    mode = 0 if pts.dtype == torch.float32 else 1
    L = lib()
    ip, cl = (C.c_double * 3)(*init_pos), (C.c_double * Ln)(*cells)
    nbytes = int(L.gsr_voxel_unique_scratch_bytes(N, Ln))
    work = scratch(nbytes, pts.device)
    record = torch.empty(1 + Ln, dtype=torch.int32, device=pts.device)
    call("gsr_voxel_unique_count", pts.device, pts, N, Ln, ip, cl, mode, work, nbytes, record)
    host = record.tolist()                                                            # the one host read: status and every level's count
    _raise_on(what, host[0] & 0xFFFFFFFF)
    rec = (C.c_uint32 * (1 + Ln))(*[h & 0xFFFFFFFF for h in host])
    U = sum(host[1:])
    positions = torch.empty(U, 3, dtype=torch.float32, device=pts.device)
    level = torch.empty(U, dtype=torch.int32, device=pts.device)
    call("gsr_voxel_unique_emit", pts.device, pts, N, Ln, ip, cl, mode, work, nbytes, rec, positions, level)
    return positions, level, host[1:]


def level_cells(voxel_size, fork, levels):
    """The reference's per-level cell sizes, by its own scalar expression on a 0-dim float32 tensor: voxel_size / float(fork) ** l (so that
    fork = 3 rounds as it does there).  voxel_size: a number or a 0-dim tensor (a device tensor costs a host read)."""
    vs = voxel_size.detach().cpu().to(torch.float32).reshape(()) if isinstance(voxel_size, torch.Tensor) else torch.tensor(float(voxel_size), dtype=torch.float32)
    return [float(vs / (float(fork) ** l)) for l in range(int(levels))]


def octree_sample(points, init_pos, voxel_size, fork, levels):
    """OctreeGaussian.octree_sample -> (positions float32 [U,3], level int32 [U]): per level l = 0 .. levels - 1 the rows of
    torch.unique(torch.round((points - init_pos) / cell_l), dim=0) * cell_l + init_pos, cell_l = voxel_size / float(fork) ** l, levels concatenated;
    within a level rows ascend by x, then y, then z.  A zero coordinate is +0.0 (the reference's sign of zero depends on its sort).  One host read
    whatever `levels` is, when init_pos and voxel_size are host values (numbers, sequences, CPU tensors); each that lives on the device costs one
    more.  A point whose cell index leaves int32, or a non-finite point, raises.  `points` is left as it is."""
    pts = _f32(points, "points", (None, 3))
    return _voxel_unique(pts, _host_floats(init_pos, 3, "init_pos"), level_cells(voxel_size, fork, levels), "octree_sample")[:2]


def voxelize_sample(points, voxel_size, device="cuda"):
    """ScaffoldGaussian.voxelize_sample -> float32 [U,3] on the device: np.unique(np.round(data / voxel_size), axis=0) * voxel_size, cast to float32
    as create_from_data does.  `points`: a numpy array or tensor [N,3], float32 (fetchPly) or float64 (a COLMAP reader); the arithmetic runs in that
    precision, as numpy's does.  The reference shuffles `data` IN PLACE first (np.random.shuffle), which decides nothing but the sign of a zero; this
    function leaves the caller's array untouched and emits +0.0.  One host read."""
    t = torch.as_tensor(points)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"points: expected a float32 or float64 array of shape [N, 3] but found {t.dtype} {list(t.shape)}")
    if not t.is_cuda:
        t = t.to(device)
    vs = float(voxel_size)
    if t.dtype == torch.float32:
        vs = float(np.float32(vs))                        # numpy divides a float32 array by the float32 of a Python number
    return _voxel_unique(t.detach().contiguous(), [0.0, 0.0, 0.0], [vs], "voxelize_sample")[0]
