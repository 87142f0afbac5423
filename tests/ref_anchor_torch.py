"""Vectorised torch restatement of anchor growing + pruning (float32 arithmetic, int64 cell keys, sort + searchsorted instead of all-pairs).

Independent of gsrast.anchors and of the HIP unit: written from the semantics in include/gsrast.h.  tests/test_anchor_cpu.py holds it to the
fixtures the reference's own code produced, bit for bit; tests/test_gpu_anchor.py then uses it as the reference for randomised scenes.
Runs on whatever device its inputs live on (the tests use the CPU)."""
import math

import torch

BIAS = 1 << 20
NAMES = ("anchor", "offset", "anchor_feat", "opacity", "scaling", "rotation")


def _f32(x, like):
    return torch.tensor(x, dtype=torch.float32, device=like.device)


def cell_keys(points, origin, cell):
    """int64 key of rint((p - origin) / cell) per row (x major), and a flag per row: the cell fits 21 bits per axis."""
    q = torch.round((points - _f32(origin, points)) / _f32(cell, points))
    ok = (torch.isfinite(q) & (q >= -BIAS) & (q <= BIAS - 1)).all(1)
    c = torch.where(ok[:, None], q, torch.zeros_like(q)).to(torch.int64) + BIAS
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], ok


def key_points(keys, origin, cell):
    c = torch.stack(((keys >> 42) & 0x1FFFFF, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF), 1) - BIAS
    return c.to(torch.float32) * _f32(cell, c) + _f32(origin, c)


def grow_level(anchor, offset, scaling, anchor_feat, grads, offset_mask, *, cell, thr_lo, thr_hi=math.inf, rand=None, rand_thr=0.0, mask=None,
               origin=(0.0, 0.0, 0.0), n0=None):
    Na = anchor.shape[0]
    N0 = Na if n0 is None else n0
    k = offset.shape[1]
    grads = grads.reshape(-1)
    cand = (grads >= _f32(thr_lo, grads)) & offset_mask.reshape(-1).bool()
    if thr_hi != math.inf:                                           # thr_hi = +inf is no upper bound: a gradient of +inf is a candidate
        cand &= grads < _f32(thr_hi, grads)
    if rand is not None:
        cand &= rand.reshape(-1) > _f32(rand_thr, grads)
    occupied = torch.ones(Na, dtype=torch.bool, device=anchor.device)
    if mask is not None:
        cand &= mask.bool().repeat_interleave(k)
        occupied[:N0] = mask.bool()
    prod = offset * scaling[:, None, :3]
    pts = (anchor[:N0, None, :] + prod).reshape(-1, 3)[cand]
    owner = torch.arange(N0, device=anchor.device).repeat_interleave(k)[cand]
    ck, ok = cell_keys(pts, origin, cell)
    if not bool(ok.all()):
        raise RuntimeError("a candidate cell lies outside the packing range")
    ak, aok = cell_keys(anchor[occupied], origin, cell)
    taken = torch.unique(ak[aok])
    uniq, inv = torch.unique(ck, return_inverse=True)
    F = anchor_feat.shape[1]
    if uniq.numel() == 0:
        return anchor.new_zeros(0, 3), anchor.new_zeros(0, F)
    if taken.numel():
        at = torch.searchsorted(taken, uniq).clamp(max=taken.numel() - 1)
        free = taken[at] != uniq
    else:
        free = torch.ones_like(uniq, dtype=torch.bool)
    feat = torch.full((uniq.numel(), F), -math.inf, dtype=torch.float32, device=anchor.device)
    feat = feat.scatter_reduce(0, inv[:, None].expand(-1, F), anchor_feat[owner], "amax", include_self=True)
    return key_points(uniq[free], origin, cell), feat[free]


def anchor_growing(anchor, offset, scaling, anchor_feat, grads, offset_mask, threshold, *, voxel_size, n_offsets, update_depth=3, update_init_factor=16,
                   update_hierachy_factor=4, rand):
    N0 = anchor.shape[0]
    cur, rows, feats, counts = anchor, [], [], []
    for i in range(update_depth):
        if i > 0 and cur.shape[0] == N0:
            counts.append(0)
            continue
        size = voxel_size * (update_init_factor // update_hierachy_factor ** i)
        a, f = grow_level(cur, offset, scaling, anchor_feat, grads, offset_mask, cell=size, thr_lo=threshold * (update_hierachy_factor // 2) ** i,
                          rand=rand[i], rand_thr=0.5 ** (i + 1), n0=N0)
        counts.append(a.shape[0])
        if a.shape[0]:
            cur = torch.cat((cur, a))
            rows.append(torch.log(torch.ones(a.shape[0], 6) * _f32(size, a)))
            feats.append(f)
    U = cur.shape[0] - N0
    rot = torch.zeros(U, 4); rot[:, 0] = 1.0
    tenth = 0.1 * torch.ones(U, 1)
    d = {"anchor": cur[N0:], "scaling": torch.cat(rows) if rows else torch.zeros(0, 6), "rotation": rot,
         "anchor_feat": torch.cat(feats) if feats else torch.zeros(0, anchor_feat.shape[1]), "offset": torch.zeros(U, n_offsets, 3),
         "opacity": torch.log(tenth / (1 - tenth))}
    return d, counts


def adjust(fx, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005):
    """fx: a fixture's arrays as CPU tensors -> {"keep", "level_counts", "new_<param>", "out_<accumulator>"}."""
    k = int(fx["k"])
    depth = int(fx["update_depth"])
    accum, denom = fx["in_offset_gradient_accum"].clone(), fx["in_offset_denom"].clone()
    g = accum / denom
    g = torch.nan_to_num(g, nan=0.0, posinf=math.inf, neginf=-math.inf).abs().reshape(-1)
    seen = (denom > check_interval * success_threshold * 0.5).reshape(-1)
    d, counts = anchor_growing(fx["in_anchor"], fx["in_offset"], fx["scaling_act"], fx["in_anchor_feat"], g, seen, grad_threshold, voxel_size=float(fx["voxel_size"]),
                               n_offsets=k, update_depth=depth, update_init_factor=int(fx["update_init_factor"]),
                               update_hierachy_factor=int(fx["update_hierachy_factor"]), rand=[fx[f"rand_{i}"] for i in range(depth)])
    U = d["anchor"].shape[0]
    accum[seen] = 0.0; denom[seen] = 0.0
    demon, opac = fx["in_anchor_demon"].clone(), fx["in_opacity_accum"].clone()
    often = demon > check_interval * success_threshold
    keep = ~((opac < min_opacity * demon) & often).reshape(-1)
    opac[often] = 0.0; demon[often] = 0.0
    out = {"keep": keep, "level_counts": torch.tensor(counts)}
    out.update({"new_" + n: d[n] for n in NAMES})
    pad = lambda x, rows: torch.cat((x, torch.zeros(rows, *x.shape[1:])))
    out["out_opacity_accum"] = pad(opac[keep], U); out["out_anchor_demon"] = pad(demon[keep], U)
    out["out_offset_gradient_accum"] = pad(accum.reshape(-1, k)[keep], U).reshape(-1, 1)
    out["out_offset_denom"] = pad(denom.reshape(-1, k)[keep], U).reshape(-1, 1)
    return out
