"""Vectorised torch restatement of the Octree-GS anchor growing + pruning (float32 arithmetic, int64 cell keys, sort + searchsorted instead of
all-pairs, the cameras of the weed-out as one [U, C] block instead of a Python loop).

Independent of gsrast.anchors and of the HIP unit: written from the semantics in include/gsrast.h (gsr_octree_weed, gsr_anchor_level_find_weed)
and the docstring of gsrast.anchors.octree_adjust_anchor_.  tests/test_anchor_octree_cpu.py holds it to the fixtures the reference's own code
produced, bit for bit; tests/test_gpu_anchor_octree.py then uses it as the reference for randomised scenes.  Runs on the device of its inputs."""
import math

import torch

from ref_anchor_torch import NAMES, cell_keys, key_points

ACCS = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")


def pred_levels(positions, cam_infos, standard_dist, fork, dtype=torch.float32):
    """pred [U, C] = log2(standard_dist / (|p - c| * scale)) / log2(fork), every operation in `dtype`."""
    p, cam = positions.to(dtype), cam_infos.to(dtype)
    d = p[:, None, :] - cam[None, :, :3]
    dist = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * cam[None, :, 3]
    return torch.log2(torch.tensor(standard_dist, dtype=dtype, device=p.device) / dist) / torch.tensor(math.log2(fork), dtype=dtype, device=p.device)


def int_levels(pred, levels, dist2level):
    r = {"floor": torch.floor, "round": torch.round, "ceil": torch.ceil}[dist2level](pred)
    return r.clamp(0, levels - 1).to(torch.int32)


def weed_out(positions, levels_of, cam_infos, standard_dist, fork, levels, dist2level, visible_threshold, dtype=torch.float32):
    """-> (visible_count int32 [U], keep bool [U])."""
    il = int_levels(pred_levels(positions, cam_infos, standard_dist, fork, dtype), levels, dist2level)
    visible = (levels_of.reshape(-1, 1).to(torch.int32) <= il).sum(dim=1).to(torch.int32)
    keep = visible.to(torch.float32) / torch.tensor(float(cam_infos.shape[0]), dtype=torch.float32, device=positions.device) > \
        torch.tensor(visible_threshold, dtype=torch.float32, device=positions.device)
    return visible, keep


def grow_pass(anchor, occupied, offset, scaling, anchor_feat, grads, candidate, *, cell, origin):
    """New cells of one pass: anchor [Na,3] with the occupiers flagged by occupied [Na]; the first N0 = offset.shape[0] own the slots, of which
    candidate [N0*k] take part.  -> (positions [U,3], maximum feature [U,F]) in (x, y, z) cell order."""
    N0, k = offset.shape[0], offset.shape[1]
    pts = (anchor[:N0, None, :] + offset * scaling[:, None, :3]).reshape(-1, 3)[candidate]
    owner = torch.arange(N0, device=anchor.device).repeat_interleave(k)[candidate]
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


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adjust(fx, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, update_ratio=0.5, extra_ratio=4.0, extra_up=0.25, min_opacity=0.005):
    """fx: a fixture's arrays as tensors (all on one device) -> {"keep", "pass_found", "pass_kept", "new_<param>", "new_level", "out_level",
    "out_extra_level", "out_<accumulator>"}."""
    k, levels, fork = int(fx["k"]), int(fx["levels"]), int(fx["fork"])
    dist2level = str(fx["dist2level"]) if not torch.is_tensor(fx["dist2level"]) else ("floor", "round", "ceil")[int(fx["dist2level"])]
    anchor, offset, scaling, feat = fx["in_anchor"], fx["in_offset"], fx["scaling_act"], fx["in_anchor_feat"]
    dev = anchor.device
    N0, F = anchor.shape[0], feat.shape[1]
    vs, sd, thr = float(fx["voxel_size"]), float(fx["standard_dist"]), float(fx["visible_threshold"])
    origin = [float(v) for v in fx["init_pos"]]
    cams = fx["cam_infos"]
    accum, denom = fx["in_offset_gradient_accum"].clone(), fx["in_offset_denom"].clone()
    g = accum / denom
    g = torch.nan_to_num(g, nan=0.0, posinf=math.inf, neginf=-math.inf).abs().reshape(-1)
    seen = (denom > check_interval * success_threshold * 0.5).reshape(-1)
    g[~seen] = 0.0
    total = torch.zeros(N0, dtype=torch.float32, device=dev)
    for j in range(k):
        total = total + g.reshape(N0, k)[:, j]
    anchor_grads = total / (seen.reshape(N0, k).sum(dim=1) + 1e-6)
    level = fx["in_level"].reshape(-1).to(torch.int64)
    extra = fx["in_extra_level"].clone()
    grow_ds = (not bool(fx["progressive"])) or int(fx["iteration"]) > float(fx["coarse_intervals"][-1])
    uv = fork ** update_ratio
    found, kept = torch.zeros(levels, 2, dtype=torch.int64), torch.zeros(levels, 2, dtype=torch.int64)
    new_pos, new_feat, new_lv, new_size = [], [], [], []
    cur_level = level.clone()                                      # levels of [originals ; appended]
    for l in range(levels):
        if not bool((cur_level == l).any()):
            continue
        cur_size = f32(f32(vs) / f32(float(fork) ** l))
        ds_size = f32(cur_size / f32(fork))
        cur_thr = grad_threshold * uv ** l
        ds_thr = cur_thr * uv
        if grow_ds:
            extra = extra + extra_up * (anchor_grads >= cur_thr * extra_ratio).float()
        own = (level == l).repeat_interleave(k)
        allpos = torch.cat([anchor] + new_pos)
        a, fa = grow_pass(allpos, cur_level == l, offset, scaling, feat, g, (g >= cur_thr) & (g < ds_thr) & own, cell=cur_size, origin=origin)
        _, ka = weed_out(a, torch.full((a.shape[0],), l, device=dev), cams, sd, fork, levels, dist2level, thr)
        found[l, 0], kept[l, 0] = a.shape[0], int(ka.sum())
        a, fa = a[ka], fa[ka]
        b = anchor.new_zeros(0, 3)
        if grow_ds and l < levels - 1 and bool((cur_level == l + 1).any()):
            b, _ = grow_pass(allpos, cur_level == l + 1, offset, scaling, feat, g, (g >= ds_thr) & own, cell=ds_size, origin=origin)
            _, kb = weed_out(b, torch.full((b.shape[0],), l + 1, device=dev), cams, sd, fork, levels, dist2level, thr)
            found[l, 1], kept[l, 1] = b.shape[0], int(kb.sum())
            b = b[kb]
        for pos, ft, lv, size in ((a, fa, l, cur_size), (b, torch.zeros(b.shape[0], F, device=dev), l + 1, ds_size)):
            if pos.shape[0]:
                new_pos.append(pos); new_feat.append(ft); new_lv.append(torch.full((pos.shape[0],), lv, dtype=torch.int64, device=dev))
                new_size.append(torch.log(torch.ones(pos.shape[0], 6) * torch.tensor(size, dtype=torch.float32)).to(dev))
        cur_level = torch.cat([level] + new_lv)
    U = cur_level.shape[0] - N0
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    rot = z(U, 4); rot[:, 0] = 1.0
    tenth = 0.1 * torch.ones(U, 1)
    d = {"anchor": torch.cat(new_pos) if U else z(0, 3), "scaling": torch.cat(new_size) if U else z(0, 6), "rotation": rot,
         "anchor_feat": torch.cat(new_feat) if U else z(0, F), "offset": z(U, k, 3), "opacity": torch.log(tenth / (1 - tenth)).to(dev)}
    accum[seen] = 0.0; denom[seen] = 0.0
    demon, opac = fx["in_anchor_demon"].clone(), fx["in_opacity_accum"].clone()
    often = demon > check_interval * success_threshold
    keep = ~((opac < min_opacity * demon) & often).reshape(-1)
    opac[often] = 0.0; demon[often] = 0.0
    out = {"keep": keep, "pass_found": found, "pass_kept": kept}
    out.update({"new_" + n: d[n] for n in NAMES})
    out["new_level"] = cur_level[N0:].to(torch.float32).reshape(-1, 1)
    out["out_level"] = torch.cat((fx["in_level"][keep].to(torch.float32), out["new_level"])) if U else fx["in_level"][keep]
    out["out_extra_level"] = torch.cat((extra[keep], z(U)))
    pad = lambda x, rows: torch.cat((x, z(rows, *x.shape[1:])))
    out["out_opacity_accum"] = pad(opac[keep], U); out["out_anchor_demon"] = pad(demon[keep], U)
    out["out_offset_gradient_accum"] = pad(accum.reshape(-1, k)[keep], U).reshape(-1, 1)
    out["out_offset_denom"] = pad(denom.reshape(-1, k)[keep], U).reshape(-1, 1)
    return out
