"""Plain torch / numpy restatement (CPU) of the reference's create_from_data pieces, written from their arithmetic and not from their code path:
OctreeGaussian.set_level / octree_sample / weed_out / create_from_data (gssr/gaussian/octree_gaussian.py:152-253) and ScaffoldGaussian.voxelize_sample
/ create_from_data (scaffold_gaussian.py:257-298).  tests/test_create_anchors_cpu.py holds it against the golden vectors the reference itself
produced (tests/golden/make_golden_create_anchors.py) with ==; tests/test_gpu_create_anchors.py holds the HIP ops against torch on the CPU.

What the restatement spells out (and gsr_init.hip implements):
  dist        sqrt(((dx*dx + dy*dy) + dz*dz)) in float32, every operation rounded on its own
  quantile    rank = float32(q) * (n - 1) IN FLOAT32, floor, ceil, w = rank - floor; lerp is ATen's Lerp.h, w < 0.5 ? a + w * (b - a) :
              b - (b - a) * (1 - w), every operation rounded on its own (what torch gives at ATen's DEFAULT CPU dispatch level, under which the
              golden vectors were produced; the AVX2 / AVX512 kernels fuse the product-sum and differ in the last bit now and then)
  cells       key = rint((p - init_pos) / cell) (half to even), rows sorted by x, then y, then z; position = key * cell + init_pos
  weed-out    per camera pred = log2(standard_dist / (dist * scale)) / log2(fork), floor | round | ceil, clamp, count of cameras with level <= it
"""
import math

import numpy as np
import torch

import glue_truth

F32 = np.float32
MODES = ("floor", "round", "ceil")


def lerp32(a, b, w):
    """ATen's Lerp.h in float32, every operation rounded on its own."""
    a, b, w = F32(a), F32(b), F32(w)
    d = F32(b - a)
    return F32(a + F32(w * d)) if abs(w) < 0.5 else F32(b - F32(d * F32(F32(1) - w)))


def ranks(q, n):
    """torch.quantile's ranks: float32(q) * (n - 1) in float32."""
    rank = F32(F32(q) * F32(n - 1))
    lo = F32(np.floor(rank))
    return int(lo), int(np.ceil(rank)), F32(rank - lo)


def quantile(values, q):
    s = np.sort(np.asarray(values, F32).reshape(-1))
    lo, hi, w = ranks(q, s.shape[0])
    return lerp32(s[lo], s[hi], w)


def distances(points, centre):
    p, c = np.asarray(points, F32), np.asarray(centre, F32)
    d = p - c[None, :]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def camera_dist_quantiles(points, cam_infos, dist_ratio):
    """all_dist [2C] = [min_0, max_0, ...]."""
    out = []
    for cam in np.asarray(cam_infos, F32):
        d = distances(points, cam[:3])
        out += [F32(quantile(d, 1 - dist_ratio) * cam[3]), F32(quantile(d, dist_ratio) * cam[3])]
    return np.array(out, F32)


def set_level(points, cam_infos, dist_ratio, fork, levels=-1, init_level=-1):
    """-> (all_dist, standard_dist float32, levels, init_level)"""
    all_dist = camera_dist_quantiles(points, cam_infos, dist_ratio)
    dist_max, dist_min = quantile(all_dist, dist_ratio), quantile(all_dist, 1 - dist_ratio)
    if levels == -1:
        levels = int(torch.round(torch.log2(torch.tensor(dist_max / dist_min)) / math.log2(fork)).int().item()) + 1
    if init_level == -1:
        init_level = int(levels / 2)
    return all_dist, dist_max, levels, init_level


def level_cells(voxel_size, fork, levels):
    return [F32(F32(voxel_size) / F32(float(fork) ** l)) for l in range(levels)]


def unique_cells(points, init_pos, cell):
    """Distinct rows of rint((p - init_pos) / cell), sorted by x, then y, then z, in the precision of `points`."""
    p = np.asarray(points)
    k = np.rint((p - np.asarray(init_pos, p.dtype)[None, :]) / p.dtype.type(cell))
    k = k[np.lexsort((k[:, 2], k[:, 1], k[:, 0]))]
    head = np.ones(k.shape[0], bool)
    head[1:] = (k[1:] != k[:-1]).any(axis=1)
    return k[head]


def octree_sample(points, init_pos, voxel_size, fork, levels):
    pos, lvl = [], []
    ip = np.asarray(init_pos, F32)
    for l, cell in enumerate(level_cells(voxel_size, fork, levels)):
        k = unique_cells(np.asarray(points, F32), ip, cell)
        pos.append((k * cell + ip[None, :]).astype(F32) + F32(0))          # + 0: a negative zero becomes +0
        lvl.append(np.full(k.shape[0], l, np.int32))
    return np.concatenate(pos), np.concatenate(lvl)


def weed_counts(positions, levels_of, cam_infos, standard_dist, fork, levels, mode):
    """visible_count int32 [U] (torch on the CPU: log2 is the platform's, the generator's margins keep the rounding decisions safe)."""
    pos, lv = torch.tensor(np.asarray(positions, F32)), torch.tensor(np.asarray(levels_of, np.int32))
    count = torch.zeros(pos.shape[0], dtype=torch.int32)
    fn = {"floor": torch.floor, "round": torch.round, "ceil": torch.ceil}[mode]
    for cam in torch.tensor(np.asarray(cam_infos, F32)):
        d = pos - cam[:3]
        dist = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * cam[3]
        pred = torch.log2(torch.tensor(F32(standard_dist)) / dist) / math.log2(fork)
        count += (lv <= torch.clamp(fn(pred).int(), min=0, max=levels - 1)).int()
    return count.numpy()


def octree_create(points, cam_infos, *, dist_ratio, fork, extend, levels, init_level, base_layer, visible_threshold, dist2level):
    """-> dict of everything OctreeGaussian.create_from_data leaves behind (arrays and scalars), with the positions before and after each weed-out."""
    p = np.asarray(points, F32)
    C = np.asarray(cam_infos).shape[0]
    all_dist, standard_dist, levels, init_level = set_level(p, cam_infos, dist_ratio, fork, levels, init_level)
    box_min, box_max = F32(p.min() * F32(extend)), F32(p.max() * F32(extend))
    box_d = F32(box_max - box_min)
    if base_layer < 0:
        base_layer = int(torch.round(torch.log2(torch.tensor(box_d) / 0.02)).int().item()) - (levels // 2) + 1
    voxel_size = F32(box_d / F32(float(fork) ** base_layer))
    init_pos = np.array([box_min] * 3, F32)
    pos0, lvl0 = octree_sample(p, init_pos, voxel_size, fork, levels)
    out = {"all_dist": all_dist, "standard_dist": standard_dist, "levels": levels, "init_level": init_level, "base_layer": base_layer,
           "voxel_size": voxel_size, "init_pos": init_pos, "positions0": pos0, "level0": lvl0}
    pos, lvl = pos0, lvl0
    if visible_threshold < 0:
        cnt = weed_counts(pos, lvl, cam_infos, standard_dist, fork, levels, dist2level)
        visible_threshold = float(F32(int(cnt.astype(np.int64).sum()) / (float(pos.shape[0]) * C)))
        keep = (cnt.astype(F32) / F32(C)) > F32(0.0)
        pos, lvl = pos[keep], lvl[keep]
        out["positions1"], out["level1"] = pos, lvl
    cnt = weed_counts(pos, lvl, cam_infos, standard_dist, fork, levels, dist2level)
    keep = (cnt.astype(F32) / F32(C)) > F32(visible_threshold)
    pos, lvl = pos[keep], lvl[keep]
    out.update(visible_threshold=visible_threshold, anchor=pos, level=lvl.reshape(-1, 1))
    return out


def scaling_of(dist2):
    """The reference's line: log(sqrt(clamp_min(dist2, 1e-7))) repeated six times (torch, float32)."""
    d = torch.clamp_min(torch.as_tensor(dist2).float(), 0.0000001)
    return torch.log(torch.sqrt(d))[..., None].repeat(1, 6)


def scaffold_create(points, voxel_size):
    """-> (voxel_size, anchor float32 [U,3]); points float32 or float64 [N,3], voxel_size <= 0: the median of distCUDA2 (kthvalue, k = int(N * 0.5))."""
    p = np.asarray(points)
    if voxel_size <= 0:
        d = np.sort(glue_truth.dist2_bruteforce(p.astype(F32)))
        voxel_size = float(d[int(d.shape[0] * 0.5) - 1])
    cell = p.dtype.type(voxel_size)
    k = unique_cells(p, np.zeros(3, p.dtype), cell)
    return voxel_size, ((k * cell).astype(F32) + F32(0))
