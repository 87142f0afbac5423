"""Anchor growing and pruning of the Scaffold-GS and Octree-GS models on the device (include/gsrast.h gsr_anchor_level_*, gsr_octree_weed,
gsr_rows_compact_multi).

`adjust_anchor_(model)` replaces `ScaffoldGaussian.adjust_anchor` (gssr/gaussian/scaffold_gaussian.py:651-705) and the `anchor_growing` it calls
(:555-649): the consumer of the statistics `gsrast.decode.training_stats_` accumulates.  The reference compares every unique candidate cell with
every anchor (O(U N)), runs a `torch.unique(dim=0)` and a `torch_scatter.scatter_max` per level and then ~60 boolean-index / cat operations, each
with a `nonzero()` host synchronisation; here a level is one sort over packed cell keys and the prune + append of every parameter, Adam moment and
accumulator is one launch.  Results equal the reference's bit for bit (tests/test_gpu_anchor.py against fixtures its own code produced), with the
two deviations of DESIGN.md §7: cells must fit 21 bits per axis, and the division by the cell size is a true division.

`octree_adjust_anchor_(model, iteration)` does the same for `OctreeGaussian.adjust_anchor` (gssr/gaussian/octree_gaussian.py:536-588, with
anchor_growing :401-534, weed_out :203-214 and get_remove_duplicates :374-385): per level two sorts in the place of two torch.unique calls and two
all-pairs comparisons, and the weed-out of the new anchors -- in the reference a Python loop over every training camera, twice per level -- runs
inside the level's find pass, before its count is read.  Same two deviations; dist2level 'progressive' raises, as the reference's own weed_out
cannot run in that mode (:198 compares [N] with [U]).

There is no CPU fallback: host tensors raise."""
import ctypes as C
import math

import torch

from . import call, lib, one_device, ptr, scratch
from ._rows import Level, RowsTensor, _bytes, _f32, groups, install_, make_weed, moments

PARAM_ATTRS = {"anchor": "_anchor", "offset": "_offset", "anchor_feat": "_anchor_feat", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
_SKIP = ("mlp", "conv", "feat_base", "embedding")        # param groups the reference's optimizer surgery leaves alone


def grow_level(anchor, offset, scaling, anchor_feat, grads, offset_mask, *, cell, thr_lo, thr_hi=math.inf, rand=None, rand_thr=0.0, mask=None,
               origin=(0.0, 0.0, 0.0), n0=None, occupy=None, weed=None):
    """One growing level (gsr_anchor_level_find + gsr_anchor_level_emit) -> (new_anchor [U,3], new_feat [U,F]); see _grow_level."""
    return _grow_level(anchor, offset, scaling, anchor_feat, grads, offset_mask, cell=cell, thr_lo=thr_lo, thr_hi=thr_hi, rand=rand, rand_thr=rand_thr,
                       mask=mask, origin=origin, n0=n0, occupy=occupy, weed=weed)[:2]


def _grow_level(anchor, offset, scaling, anchor_feat, grads, offset_mask, *, cell, thr_lo, thr_hi=math.inf, rand=None, rand_thr=0.0, mask=None,
                origin=(0.0, 0.0, 0.0), n0=None, occupy=None, weed=None):
    """-> (new_anchor [U,3], new_feat [U,F], the number of new cells before the weed-out).

    anchor [Na,3]: the first n0 (default: all) own the candidate slots offset [n0,k,3] / grads [n0*k] / offset_mask [n0*k]; the others only occupy
    cells.  scaling [n0,>=3] is the ACTIVATED scaling, anchor_feat [n0,F].  Slot j is a candidate iff thr_lo <= grads[j] < thr_hi (thr_hi = inf: no
    upper bound, a gradient of +inf is a candidate), offset_mask[j], rand[j] > rand_thr (rand given) and mask[j // k] (mask [n0] given; a masked-out original anchor does not occupy its cell either).  The new
    anchors are the distinct cells rint((anchor + offset * scaling - origin) / cell) of the candidates that hold no admitted anchor, in (x, y, z)
    order, at cell * c + origin, with the element-wise maximum of the candidates' features.  One host synchronisation (the count).
    Octree-GS: occupy [n0] given, original anchor a occupies its cell iff occupy[a] and mask decides candidacy alone; weed (a gsr_octree_weed of
    _rows.make_weed) given, the new positions are weighed against its cameras on the device and only the kept ones are counted and written."""
    anchor = _f32(anchor, "anchor", (None, 3))
    Na = anchor.shape[0]
    N0 = Na if n0 is None else int(n0)
    if not 0 <= N0 <= Na:
        raise RuntimeError(f"n0: expected 0 <= n0 <= {Na} but found {N0}")
    offset = _f32(offset, "offset", (N0, None, 3))
    k = offset.shape[1]
    if k < 1:
        raise RuntimeError("offset: n_offsets must be >= 1")
    scaling = _f32(scaling, "scaling", (N0, None))
    if scaling.shape[1] < 3:
        raise RuntimeError(f"scaling: expected at least 3 columns but found {scaling.shape[1]}")
    anchor_feat = _f32(anchor_feat, "anchor_feat", (N0, None))
    F = anchor_feat.shape[1]
    grads = _f32(grads, "grads")
    if grads.numel() != N0 * k:
        raise RuntimeError(f"grads: expected {N0 * k} entries but found {grads.numel()}")
    offset_mask = _bytes(offset_mask, "offset_mask", N0 * k, anchor)
    if rand is not None:
        rand = _f32(rand, "rand")
        if rand.numel() != N0 * k:
            raise RuntimeError(f"rand: expected {N0 * k} entries but found {rand.numel()}")
    if mask is not None:
        mask = _bytes(mask, "mask", N0, anchor)
    if occupy is not None:
        occupy = _bytes(occupy, "occupy", N0, anchor)
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise RuntimeError(f"cell: expected a positive finite number but found {cell}")
    if len(origin) != 3:
        raise RuntimeError("origin: expected three numbers")
    dev = one_device(("anchor", anchor), ("offset", offset), ("scaling", scaling), ("anchor_feat", anchor_feat), ("grads", grads), ("rand", rand))
    if Na + N0 * k >= 1 << 31:
        raise RuntimeError(f"anchor: Na + n0 * k = {Na + N0 * k} entries exceed 2^31")
    L = lib()
    lv = Level(Na, N0, k, F, scaling.shape[1], thr_lo, thr_hi, rand_thr, cell, (C.c_float * 3)(*[float(o) for o in origin]),
               ptr(anchor).value, None if mask is None else ptr(mask).value, ptr(offset).value, ptr(scaling).value, ptr(anchor_feat).value, ptr(grads).value,
               ptr(offset_mask).value, None if rand is None else ptr(rand).value)
    nbytes = L.gsr_anchor_level_scratch_bytes(Na, N0, k)
    work = scratch(nbytes, dev)
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    if occupy is None and weed is None:
        call("gsr_anchor_level_find", dev, C.byref(lv), work, nbytes, status)
    else:
        call("gsr_anchor_level_find_weed", dev, C.byref(lv), occupy, None if weed is None else C.byref(weed), work, nbytes, status)
    count, overflow, found = status.tolist()              # the level's one host synchronisation
    if overflow:
        raise RuntimeError(f"gsrast anchor growing: a candidate cell lies outside the packing range of +-2^20 cells per axis "
                           f"(cell size {cell:g}: about +-{cell * (1 << 20):g} scene units around the origin)")
    new_anchor = torch.empty(count, 3, dtype=torch.float32, device=dev)
    new_feat = torch.empty(count, F, dtype=torch.float32, device=dev)
    if count:
        call("gsr_anchor_level_emit", dev, C.byref(lv), work, nbytes, count, new_anchor, new_feat)
    return new_anchor, new_feat, (found if (occupy is not None or weed is not None) else count)


def _host_log(x):
    """log of a float32 scalar as torch's CPU kernel computes it for a float32 tensor (the vector path: 16 lanes)."""
    return float(torch.log(torch.full((16,), x, dtype=torch.float32))[0])


def anchor_growing(anchor, offset, scaling, anchor_feat, grads, offset_mask, threshold, *, voxel_size, n_offsets, update_depth=3, update_init_factor=16,
                   update_hierachy_factor=4, rand=None, generator=None):
    """The reference's anchor_growing: every level's new anchors, concatenated in level order, as its dictionary `d`
    (anchor, scaling, rotation, anchor_feat, offset, opacity) -- handing the whole to cat_tensors_to_optimizer once equals the reference's call per level.
    `scaling` is the ACTIVATED get_scaling tensor as torch computed it; `rand`: one tensor of uniform draws [N*k] per level (None: drawn on the
    device from `generator`)."""
    anchor = _f32(anchor, "anchor", (None, 3))
    N0 = anchor.shape[0]
    k = int(n_offsets)
    offset = _f32(offset, "offset", (N0, k, 3))
    if update_depth < 0 or update_init_factor < 1 or update_hierachy_factor < 1:
        raise RuntimeError("update_depth / update_init_factor / update_hierachy_factor: expected update_depth >= 0 and factors >= 1")
    if not (float(voxel_size) > 0.0):
        raise RuntimeError(f"voxel_size: expected a positive number but found {voxel_size}")
    if rand is not None and len(rand) != update_depth:
        raise RuntimeError(f"rand: expected a list of update_depth = {update_depth} tensors but found {len(rand)}")
    dev = anchor.device
    added, feats, sizes = [], [], []
    for i in range(update_depth):
        cur_threshold = threshold * ((update_hierachy_factor // 2) ** i)
        r = rand[i] if rand is not None else torch.rand(N0 * k, dtype=torch.float32, device=dev, generator=generator)      # drawn at every level, as the reference does
        if i > 0 and not added:
            continue                                             # scaffold_gaussian.py:569-572: later levels wait for a first addition
        size_factor = update_init_factor // (update_hierachy_factor ** i)
        if size_factor < 1:
            raise RuntimeError(f"update_depth: level {i} has size factor {update_init_factor} // {update_hierachy_factor}**{i} = 0")
        cur_size = voxel_size * size_factor
        cur = torch.cat([anchor] + added) if added else anchor
        a, f = grow_level(cur, offset, scaling, anchor_feat, grads, offset_mask, cell=cur_size, thr_lo=cur_threshold, rand=r, rand_thr=0.5 ** (i + 1), n0=N0)
        if a.shape[0]:
            added.append(a); feats.append(f); sizes.append((a.shape[0], cur_size))
    U = sum(n for n, _ in sizes)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    new_scaling = z(U, 6)
    p = 0
    for n, cur_size in sizes:
        new_scaling[p:p + n] = _host_log(C.c_float(cur_size).value)
        p += n
    new_rotation = z(U, 4)
    new_rotation[:, 0] = 1.0
    x = C.c_float(0.1).value                                     # inverse_sigmoid(0.1 * ones) in float32
    xt = torch.full((16,), x, dtype=torch.float32)
    new_opacity = torch.full((U, 1), float(torch.log(xt / (1 - xt))[0]), dtype=torch.float32, device=dev)
    return {"anchor": torch.cat(added) if added else z(0, 3), "scaling": new_scaling, "rotation": new_rotation,
            "anchor_feat": torch.cat(feats) if feats else z(0, anchor_feat.shape[1]), "offset": z(U, k, 3), "opacity": new_opacity}


def rows_compact(keep, tensors, tails=None):
    """[torch.cat((x[keep], tail)) for x, tail in zip(tensors, tails)] in one launch (gsr_rows_compact_multi): `keep` a bool / uint8 mask over the
    rows (dim 0) of every tensor; a tail is a tensor with the same row shape, or an int = that many rows of zeros (None: 0).  One host
    synchronisation: the number of kept rows sizes the results."""
    if not tensors:
        return []
    N = tensors[0].shape[0]
    keep = _bytes(keep, "keep", N, tensors[0])
    tails = list(tails) if tails is not None else [0] * len(tensors)
    if len(tails) != len(tensors):
        raise RuntimeError("tails: expected one entry per tensor")
    srcs = []
    for i, x in enumerate(tensors):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != keep.device:
            raise RuntimeError(f"tensors[{i}] must be a CUDA tensor on the device of keep")
        if x.dim() < 1 or x.shape[0] != N:
            raise RuntimeError(f"tensors[{i}]: expected {N} rows but found {list(x.shape)}")
        x = x.detach().contiguous()
        rb = x.element_size() * (x.numel() // N if N else math.prod(x.shape[1:]))
        if rb <= 0 or rb % 4:
            raise RuntimeError(f"tensors[{i}]: a row must be a positive multiple of 4 bytes, found {rb}")
        t = tails[i]
        if isinstance(t, torch.Tensor):
            if t.dtype != x.dtype or t.device != x.device or t.shape[1:] != x.shape[1:]:
                raise RuntimeError(f"tails[{i}] must match tensors[{i}] in dtype, device and row shape")
            t = t.detach().contiguous()
        srcs.append((x, rb, t))
    L = lib()
    dev = keep.device
    n_keep = int(keep.count_nonzero()) if N else 0
    nbytes = L.gsr_rows_compact_scratch_bytes(N)
    work = scratch(nbytes, dev)
    table = (RowsTensor * len(srcs))()
    outs, n = [], 0
    for x, rb, t in srcs:
        nt = t.shape[0] if isinstance(t, torch.Tensor) else int(t or 0)
        out = torch.empty((n_keep + nt,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
        outs.append(out)
        if out.numel():                                      # nothing kept and no tail: nothing to write
            table[n] = RowsTensor(x.data_ptr() if N else None, out.data_ptr(), t.data_ptr() if isinstance(t, torch.Tensor) and nt else None, rb, nt)
            n += 1
    call("gsr_rows_compact_multi", dev, N, keep if N else None, n, table, work, nbytes)
    return outs


@torch.no_grad()
def adjust_anchor_(model, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005, rand=None):
    """ScaffoldGaussian.adjust_anchor on the device, for any object with the reference's attributes (_anchor, _offset, _anchor_feat, _opacity,
    _scaling, _rotation, get_scaling, optimizer, opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, n_offsets, voxel_size,
    update_depth, update_init_factor, update_hierachy_factor, max_radii2D).  Grows (every level), prunes, carries the Adam moments
    (gsrast.optim.Adam or torch.optim.Adam: same state keys, `step` untouched) and resets the statistics; returns the number of anchors."""
    for name in list(PARAM_ATTRS.values()) + ["get_scaling", "optimizer", "opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom", "n_offsets",
                                              "voxel_size", "update_depth", "update_init_factor", "update_hierachy_factor"]:
        if not hasattr(model, name):
            raise RuntimeError(f"model: attribute {name} is missing")
    k = int(model.n_offsets)
    anchor = _f32(model._anchor, "model._anchor", (None, 3))
    N0 = anchor.shape[0]
    dev = anchor.device
    shapes = {"_offset": (N0, k, 3), "_anchor_feat": (N0, None), "_opacity": (N0, 1), "_scaling": (N0, 6), "_rotation": (N0, 4),
              "opacity_accum": (N0, 1), "anchor_demon": (N0, 1), "offset_gradient_accum": (N0 * k, 1), "offset_denom": (N0 * k, 1)}
    for name, shp in shapes.items():
        _f32(getattr(model, name), "model." + name, shp)
    scaling = model.get_scaling() if callable(model.get_scaling) else model.get_scaling
    scaling = _f32(scaling, "model.get_scaling", (N0, None))
    grp = groups(model, PARAM_ATTRS, _SKIP)

    # 1. statistics -> per-slot gradient and the slots that were seen often enough
    grads = model.offset_gradient_accum / model.offset_denom
    grads = torch.where(grads.isnan(), torch.zeros_like(grads), grads).abs().reshape(-1)
    offset_mask = (model.offset_denom > check_interval * success_threshold * 0.5).reshape(-1)
    # 2. growing
    d = anchor_growing(anchor, model._offset, scaling, model._anchor_feat, grads, offset_mask, grad_threshold, voxel_size=model.voxel_size, n_offsets=k,
                       update_depth=model.update_depth, update_init_factor=model.update_init_factor, update_hierachy_factor=model.update_hierachy_factor,
                       rand=rand)
    U = d["anchor"].shape[0]
    # 3. - 5. reset the consumed statistics, prune mask
    om = offset_mask.reshape(-1, 1)
    model.offset_denom.masked_fill_(om, 0.0)
    model.offset_gradient_accum.masked_fill_(om, 0.0)
    anchors_mask = model.anchor_demon > check_interval * success_threshold
    prune = (model.opacity_accum < min_opacity * model.anchor_demon) & anchors_mask
    model.opacity_accum.masked_fill_(anchors_mask, 0.0)
    model.anchor_demon.masked_fill_(anchors_mask, 0.0)
    keep = ~prune.reshape(-1)
    # 6. one compaction + append pass: [old[keep] ; new]
    tensors, tails, carried = [], [], {}
    for n, g in grp.items():
        p = g["params"][0]
        carried[n] = moments(model.optimizer, p)
        tensors += [p] + list(carried[n] or ()); tails += [d[n]] + [U] * (2 if carried[n] else 0)
    accs = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")
    tensors += [getattr(model, n) for n in accs[:2]] + [getattr(model, n).reshape(N0, k) for n in accs[2:]]
    outs = iter(rows_compact(keep, tensors, tails + [U] * 4))
    # 7. fresh parameters, carried optimizer state
    for n, g in grp.items():
        data = next(outs)
        if n == "scaling":
            data[:, 3:].clamp_(max=0.05)                         # 8. scaffold_gaussian.py:527-531, on the raw parameter
        install_(model, g, PARAM_ATTRS[n], data, (next(outs), next(outs)) if carried[n] else None)
    for n in accs:
        setattr(model, n, next(outs).reshape(-1, 1))
    # 9.
    Na = model._anchor.shape[0]
    model.max_radii2D = torch.zeros(Na, dtype=torch.float32, device=dev)
    return Na


OCTREE_ATTRS = ("_level", "_extra_level", "levels", "fork", "voxel_size", "init_pos", "standard_dist", "cam_infos", "visible_threshold", "dist2level", "progressive",
                "coarse_intervals")


def _inverse_sigmoid_tenth():
    xt = torch.full((16,), C.c_float(0.1).value, dtype=torch.float32)                      # inverse_sigmoid(0.1 * ones) in float32
    return float(torch.log(xt / (1 - xt))[0])


@torch.no_grad()
def octree_adjust_anchor_(model, iteration, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, update_ratio=0.5, extra_ratio=4.0, extra_up=0.25,
                          min_opacity=0.005, trace=None):
    """OctreeGaussian.adjust_anchor on the device, for any object with the Scaffold attributes adjust_anchor_ checks (without the update_* factors and
    max_radii2D) and _level [N,1], _extra_level [N], levels, fork, voxel_size, init_pos, standard_dist, cam_infos [C,4], visible_threshold,
    dist2level, progressive, coarse_intervals.  Per level l that holds anchors: pass A (slots of level-l anchors with cur_thr <= g < ds_thr, cells of
    voxel_size / fork^l, occupied by every current level-l anchor, weeded with lv = l, feature = maximum) and, where the finer levels grow and level
    l+1 holds anchors, pass B (g >= ds_thr, cells of a fork-th of that, occupied by the level-(l+1) anchors, weeded with lv = l+1, feature zeros).
    Then one prune + append over parameters, Adam moments, accumulators, _level and _extra_level.  Host reads: the level histogram (with the
    model's scalars where they live on the device), one count per pass that runs, the number of kept rows.  `trace`: a list that receives
    (level, "A" | "B", cells found, cells kept) per pass.  Returns the number of anchors."""
    for name in list(PARAM_ATTRS.values()) + ["get_scaling", "optimizer", "opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom", "n_offsets"] + \
            list(OCTREE_ATTRS):
        if not hasattr(model, name):
            raise RuntimeError(f"model: attribute {name} is missing")
    if model.dist2level == "progressive":
        raise RuntimeError("octree_adjust_anchor_: dist2level 'progressive' is not supported: the reference's own weed_out cannot run in that mode")
    k = int(model.n_offsets)
    anchor = _f32(model._anchor, "model._anchor", (None, 3))
    N0 = anchor.shape[0]
    dev = anchor.device
    shapes = {"_offset": (N0, k, 3), "_anchor_feat": (N0, None), "_opacity": (N0, 1), "_scaling": (N0, 6), "_rotation": (N0, 4), "_extra_level": (N0,),
              "opacity_accum": (N0, 1), "anchor_demon": (N0, 1), "offset_gradient_accum": (N0 * k, 1), "offset_denom": (N0 * k, 1)}
    for name, shp in shapes.items():
        _f32(getattr(model, name), "model." + name, shp)
    level = model._level
    if not isinstance(level, torch.Tensor) or level.device != dev or tuple(level.shape) != (N0, 1) or level.dtype not in (torch.int32, torch.float32):
        raise RuntimeError(f"model._level: expected an int32 or float32 tensor of shape [{N0}, 1] on the device of model._anchor")
    scaling = model.get_scaling() if callable(model.get_scaling) else model.get_scaling
    scaling = _f32(scaling, "model.get_scaling", (N0, None))
    F = model._anchor_feat.shape[1]
    grp = groups(model, PARAM_ATTRS, _SKIP)
    levels, fork = int(model.levels), model.fork
    lvl = level.reshape(-1)

    # the one read before the loop: anchors per level, and the model's scalars where they are device tensors (as create_from_data leaves them)
    hist_dev = (lvl.reshape(-1, 1) == torch.arange(levels, device=dev, dtype=lvl.dtype)).sum(dim=0).to(torch.float64)
    sizes = {"voxel_size": 1, "standard_dist": 1, "visible_threshold": 1, "init_pos": 3}
    vals = {n: getattr(model, n) for n in sizes}
    for n, v in vals.items():
        if (v.numel() if isinstance(v, torch.Tensor) else len(v) if n == "init_pos" else 1) != sizes[n]:
            raise RuntimeError(f"model.{n}: expected {sizes[n]} number(s)")
    on_dev = [n for n in sizes if isinstance(vals[n], torch.Tensor) and vals[n].is_cuda]
    host = torch.cat([hist_dev] + [vals[n].detach().to(dev, torch.float64).reshape(-1) for n in on_dev]).tolist()
    hist, p = [int(c) for c in host[:levels]] + [0], levels
    for n in on_dev:
        vals[n] = host[p:p + sizes[n]]; p += sizes[n]
    flat = lambda v: [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v if isinstance(v, (list, tuple)) else [v])]
    vs, standard_dist, visible_threshold = (C.c_float(flat(vals[n])[0]).value for n in ("voxel_size", "standard_dist", "visible_threshold"))
    origin = flat(vals["init_pos"])
    f32 = lambda x: C.c_float(x).value

    # 1. statistics -> per-slot gradient, the slots seen often enough, per-anchor mean gradient (summed left to right)
    grads = model.offset_gradient_accum / model.offset_denom
    grads = torch.where(grads.isnan(), torch.zeros_like(grads), grads).abs().reshape(-1)
    offset_mask = (model.offset_denom > check_interval * success_threshold * 0.5).reshape(-1)
    grads = torch.where(offset_mask, grads, torch.zeros_like(grads))
    g2, m2 = grads.reshape(N0, k), offset_mask.reshape(N0, k)
    total = g2[:, 0].clone()
    for j in range(1, k):
        total += g2[:, j]
    anchor_grads = total / (m2.sum(dim=1) + 1e-6)

    # 2. the level loop
    grow_ds = (not model.progressive) or iteration > model.coarse_intervals[-1]
    update_value = fork ** update_ratio
    rows = []                                                     # (positions, features, level, cell size) of every pass that added anchors
    prev_b = None                                                 # the previous turn's pass-B anchors: the only appended ones of level l
    for l in range(levels):
        if hist[l] == 0:
            prev_b = None
            continue
        cur_size = f32(vs / f32(float(fork) ** l))
        ds_size = f32(cur_size / f32(fork))
        cur_thr = grad_threshold * (update_value ** l)
        ds_thr = cur_thr * update_value
        if grow_ds:
            model._extra_level[:N0] += extra_up * (anchor_grads >= cur_thr * extra_ratio).float()
        is_l = lvl == l
        cur = torch.cat((anchor, prev_b)) if prev_b is not None else anchor
        w, cams = make_weed(model.cam_infos, standard_dist, fork, levels, model.dist2level, visible_threshold, lv=l)
        one_device(("model._anchor", anchor), ("model.cam_infos", cams))
        a, f, found = _grow_level(cur, model._offset, scaling, model._anchor_feat, grads, offset_mask, cell=cur_size, thr_lo=cur_thr, thr_hi=ds_thr, mask=is_l,
                                  occupy=is_l, origin=origin, n0=N0, weed=w)
        if trace is not None:
            trace.append((l, "A", found, a.shape[0]))
        if a.shape[0]:
            rows.append((a, f, l, cur_size)); hist[l] += a.shape[0]
        prev_b = None
        if grow_ds and l < levels - 1 and hist[l + 1] > 0:
            w, cams = make_weed(model.cam_infos, standard_dist, fork, levels, model.dist2level, visible_threshold, lv=l + 1)
            b, _, found = _grow_level(anchor, model._offset, scaling, model._anchor_feat[:, :0], grads, offset_mask, cell=ds_size, thr_lo=ds_thr, mask=is_l,
                                      occupy=lvl == l + 1, origin=origin, weed=w)
            if trace is not None:
                trace.append((l, "B", found, b.shape[0]))
            if b.shape[0]:
                rows.append((b, torch.zeros(b.shape[0], F, dtype=torch.float32, device=dev), l + 1, ds_size)); hist[l + 1] += b.shape[0]
                prev_b = b
    U = sum(r[0].shape[0] for r in rows)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    new_scaling, new_level = z(U, 6), z(U, 1)
    p = 0
    for a, _, l, size in rows:
        new_scaling[p:p + a.shape[0]] = _host_log(size)
        new_level[p:p + a.shape[0]] = float(l)
        p += a.shape[0]
    new_rotation = z(U, 4)
    new_rotation[:, 0] = 1.0
    d = {"anchor": torch.cat([r[0] for r in rows]) if rows else z(0, 3), "scaling": new_scaling, "rotation": new_rotation,
         "anchor_feat": torch.cat([r[1] for r in rows]) if rows else z(0, F), "offset": z(U, k, 3),
         "opacity": torch.full((U, 1), _inverse_sigmoid_tenth(), dtype=torch.float32, device=dev)}

    # 3. reset the consumed statistics, prune mask
    om = offset_mask.reshape(-1, 1)
    model.offset_denom.masked_fill_(om, 0.0)
    model.offset_gradient_accum.masked_fill_(om, 0.0)
    anchors_mask = model.anchor_demon > check_interval * success_threshold
    prune = (model.opacity_accum < min_opacity * model.anchor_demon) & anchors_mask
    model.opacity_accum.masked_fill_(anchors_mask, 0.0)
    model.anchor_demon.masked_fill_(anchors_mask, 0.0)
    keep = ~prune.reshape(-1)
    # 4. one compaction + append pass: [old[keep] ; new]
    tensors, tails, carried = [], [], {}
    for n, g in grp.items():
        q = g["params"][0]
        carried[n] = moments(model.optimizer, q)
        tensors += [q] + list(carried[n] or ()); tails += [d[n]] + [U] * (2 if carried[n] else 0)
    accs = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")
    tensors += [getattr(model, n) for n in accs[:2]] + [getattr(model, n).reshape(N0, k) for n in accs[2:]]
    tails += [U] * 4
    tensors += [level.to(torch.float32) if U else level, model._extra_level]          # torch.cat's promotion: float32 once anything was added
    tails += [new_level if U else 0, U]
    outs = iter(rows_compact(keep, tensors, tails))
    for n, g in grp.items():
        data = next(outs)
        install_(model, g, PARAM_ATTRS[n], data, (next(outs), next(outs)) if carried[n] else None)
    for n in accs:
        setattr(model, n, next(outs).reshape(-1, 1))
    model._level = next(outs)
    model._extra_level = next(outs)
    return model._anchor.shape[0]


# ---------------------------------------------------------------------------------------------------------------- the first anchors
def _initial_parameters_(model, positions, device):
    """The O(U) fills both create_from_data end with (the reference's own torch lines): offsets, features, scaling from distCUDA2, unit quaternions, the
    constant opacity, as fresh Parameters on the model."""
    from simple_knn._C import distCUDA2
    from torch import nn
    U = positions.shape[0]
    offsets = torch.zeros((U, model.n_offsets, 3), dtype=torch.float32, device=device)
    anchors_feat = torch.zeros((U, model.feat_dim), dtype=torch.float32, device=device)
    dist2 = torch.clamp_min(distCUDA2(positions).float(), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 6)
    rots = torch.zeros((U, 4), device=device)
    rots[:, 0] = 1
    opacities = model.inverse_opacity_activation(0.1 * torch.ones((U, 1), dtype=torch.float, device=device))
    model._anchor = nn.Parameter(positions.requires_grad_(True))
    model._offset = nn.Parameter(offsets.requires_grad_(True))
    model._anchor_feat = nn.Parameter(anchors_feat.requires_grad_(True))
    model._scaling = nn.Parameter(scales.requires_grad_(True))
    model._rotation = nn.Parameter(rots.requires_grad_(False))
    model._opacity = nn.Parameter(opacities.requires_grad_(False))


def _sampling_ratio(model):
    cfg = getattr(model, "config", None)
    return int(getattr(cfg, "sampling_ratio", getattr(model, "sampling_ratio", 1)))


def octree_create_from_data_(model, pcd, cameras, spatial_lr_scale):
    """OctreeGaussian.create_from_data (octree_gaussian.py:216-253) on the device, for any object carrying the reference's attributes: dist_ratio, levels,
    init_level, fork, extend, base_layer, visible_threshold, dist2level, n_offsets, feat_dim, inverse_opacity_activation, config.sampling_ratio (and
    device, else "cuda").  pcd.points [N,3]; cameras {resolution scale: [camera with .camera_center]} (gsrast.init.camera_infos).  Steps: set_level
    (per-camera distance quantiles by radix select, no C x N array); the box, base_layer, voxel_size (left a 0-dim float32 device tensor, as the
    reference leaves it) and init_pos; octree_sample (sorted distinct cells per level); the two weed-out passes -- where visible_threshold is negative
    the first one runs at 0 and fixes it to the mean visible fraction, the integer sum of the counts divided by U * C in float64 and cast to float32
    (the reference's float32 torch.mean differs from it by that mean's rounding only); distCUDA2 and the parameter fills.  Leaves cam_infos,
    standard_dist, levels, init_level, base_layer, voxel_size, init_pos, positions, visible_threshold (a float), the six Parameters, _level [U,1]
    int32, _extra_level and _anchor_mask on the model.  Returns the number of anchors."""
    from . import init as ginit
    from .octree import weed_out
    with torch.no_grad():
        device = getattr(model, "device", "cuda")
        points = torch.as_tensor(pcd.points[::_sampling_ratio(model)]).float().to(device)
        fork = model.fork
        box = (torch.min(points) * model.extend, torch.max(points) * model.extend)
        cams, mm, host = ginit._set_level(points, cameras, model.dist_ratio, fork, extra=box)      # one host read: levels, the distances, the box
        model.cam_infos, model.standard_dist = cams, mm[1]
        if model.levels == -1:
            if not math.isfinite(host[0]):
                raise RuntimeError("octree_create_from_data_: dist_max / dist_min is not a positive finite number, levels cannot be derived")
            model.levels = int(host[0]) + 1
        if model.init_level == -1:
            model.init_level = int(model.levels / 2)
        model.spatial_lr_scale = spatial_lr_scale
        box_min, box_max = torch.tensor(host[3], dtype=torch.float32), torch.tensor(host[4], dtype=torch.float32)      # the device's float32 values, exactly
        box_d = box_max - box_min
        if model.base_layer < 0:
            default_voxel_size = 0.02
            model.base_layer = torch.round(torch.log2(box_d / default_voxel_size)).int().item() - (model.levels // 2) + 1
        voxel_size = box_d / (float(fork) ** model.base_layer)
        init_pos = torch.stack([box_min, box_min, box_min]).float()
        model.voxel_size, model.init_pos = voxel_size.to(device), init_pos.to(device)
        positions, level = ginit.octree_sample(points, init_pos, voxel_size, fork, model.levels)
        standard_dist = C.c_float(host[2]).value
        Cn = cams.shape[0]
        if model.visible_threshold < 0:
            count, keep = weed_out(positions, level, cams, standard_dist, fork, model.levels, model.dist2level, 0.0)
            total = int(count.sum(dtype=torch.int64).item())
            model.visible_threshold = C.c_float(total / (float(positions.shape[0]) * Cn)).value
            positions, level = positions[keep], level[keep]
        _, keep = weed_out(positions, level, cams, standard_dist, fork, model.levels, model.dist2level, float(model.visible_threshold))
        positions, level = positions[keep].contiguous(), level[keep].contiguous()
        model.positions = positions
        _initial_parameters_(model, positions, device)
        model._level = level.unsqueeze(dim=1)
        model._extra_level = torch.zeros(positions.shape[0], dtype=torch.float, device=device)
        model._anchor_mask = torch.ones(positions.shape[0], dtype=torch.bool, device=device)
        return positions.shape[0]


def create_from_data_(model, pcd, cameras, spatial_lr_scale):
    """ScaffoldGaussian.create_from_data (scaffold_gaussian.py:262-298) on the device, for any object carrying voxel_size, n_offsets, feat_dim,
    inverse_opacity_activation, config.sampling_ratio (and device, else "cuda").  Where voxel_size <= 0 it becomes the median of distCUDA2 over the
    cloud, torch.kthvalue(dist, int(N * 0.5)), by radix select (gsrast.init.kthvalue).  The distinct voxels come from gsrast.init.voxelize_sample: on
    the device, in the precision of pcd.points as numpy would compute them, without the round trip through the host.  The reference shuffles
    pcd.points IN PLACE (np.random.shuffle) before np.unique; this function does not touch the caller's array, and its rows are the same set in
    the same (sorted) order.  `cameras` is not read, as in the reference.  Returns the number of anchors."""
    from simple_knn._C import distCUDA2
    from . import init as ginit
    with torch.no_grad():
        device = getattr(model, "device", "cuda")
        model.spatial_lr_scale = spatial_lr_scale
        points = pcd.points[::_sampling_ratio(model)]
        if model.voxel_size <= 0:
            init_points = torch.as_tensor(points).float().to(device)
            init_dist = distCUDA2(init_points).float()
            model.voxel_size = ginit.kthvalue(init_dist, int(init_dist.shape[0] * 0.5)).item()
            del init_dist, init_points
        positions = ginit.voxelize_sample(points, model.voxel_size, device)
        _initial_parameters_(model, positions, device)
        model.max_radii2D = torch.zeros((positions.shape[0]), device=device)
        return positions.shape[0]
