"""Octree-GS level-of-detail mask fused with the visibility prefilter (include/gsrast.h gsr_octree_visible).

Replaces `OctreeGaussianModel.set_anchor_mask` (gssr/gaussian/octree_gaussian.py:255-267, incl. map_to_int_level :184-203) followed by
`OctreeScene.prefilter_voxel` (gssr/scene/octree_scene.py:136-172): no boolean-index gathers, no host synchronisation.

`weed_out` is `OctreeGaussianModel.weed_out` (:203-214) over the kernel the anchor growing weighs its new anchors with (gsr_octree_weed_out)."""
import ctypes as C

import torch

from . import EWA, LodCfg, call, dev_f32, make_cfg, one_device

MODES = {"floor": 0, "round": 1, "ceil": 2, "progressive": 3}


def octree_visible(raster_settings, anchor, level, scaling, rotation, voxel_size, fork, standard_dist, coarse_index, dist2level="round",
                   extra_level=None, resolution_scale=1.0):
    """-> dict(anchor_mask bool[Na], visible_mask bool[Na] (== prefilter_voxel's result), radii int32[Na],
               prog_ratio float[Na,1] | None, transition_mask bool[Na] | None)   (the last two only for dist2level='progressive').
    raster_settings: the GaussianRasterizationSettings prefilter_voxel builds; scaling = get_scaling (Na,6) or (Na,3); level int (Na,) | (Na,1);
    coarse_index = `coarse_index` of set_anchor_mask (levels in use: the reference passes coarse_index - 1 to map_to_int_level)."""
    if dist2level not in MODES:
        raise ValueError(f"Unknown dist2level: {dist2level}")
    with torch.no_grad():
        Na = int(anchor.shape[0])
        dev = anchor.device
        a = dev_f32(anchor, "anchor", allow_empty=Na == 0)                    # no anchors: empty outputs, nothing launched
        lv = level.reshape(-1).to(torch.int32).contiguous()
        sc = dev_f32(scaling, "scaling", allow_empty=Na == 0)
        ro = dev_f32(rotation, "rotation", allow_empty=Na == 0)
        ex = None if extra_level is None else dev_f32(extra_level.reshape(-1), "extra_level")
        amask = torch.empty(Na, dtype=torch.uint8, device=dev)
        radii = torch.empty(Na, dtype=torch.int32, device=dev)
        prog = torch.empty(Na, 1, dtype=torch.float32, device=dev) if dist2level == "progressive" else None
        trans = torch.empty(Na, dtype=torch.uint8, device=dev) if dist2level == "progressive" else None
        if Na:
            keep = []
            cfg = make_cfg(EWA, Na, raster_settings, 0, 0, False, keep)
            one_device(("anchor", a), *zip(("bg", "viewmatrix", "projmatrix", "campos"), keep))
            lod = LodCfg(float(voxel_size), float(fork), float(standard_dist), float(resolution_scale), int(coarse_index), MODES[dist2level])
            call("gsr_octree_visible", dev, C.byref(cfg), C.byref(lod), a, lv, ex, sc, int(sc.shape[1]), ro, amask, radii, prog, trans)
        return {"anchor_mask": amask.view(torch.bool), "visible_mask": radii > 0, "radii": radii, "prog_ratio": prog,
                "transition_mask": None if trans is None else trans.view(torch.bool)}


def weed_out(positions, levels_of, cam_infos, standard_dist, fork, levels, dist2level="round", visible_threshold=0.0):
    """-> (visible_count int32 [U], keep bool [U]): per position [U,3] of level levels_of [U] the number of cameras cam_infos [C,4] (centre, scale)
    whose distance level admits it, and visible_count / C > visible_threshold.  The reference loops over the cameras with eight launches each;
    this is one launch and no host synchronisation.  dist2level 'progressive' raises, as the reference's weed_out cannot run in it."""
    from ._rows import _f32, make_weed
    with torch.no_grad():
        pos = _f32(positions, "positions", (None, 3))
        U = pos.shape[0]
        if not isinstance(levels_of, torch.Tensor) or levels_of.device != pos.device or levels_of.numel() != U:
            raise RuntimeError(f"levels_of: expected a tensor of {U} entries on the device of positions")
        lv = levels_of.reshape(-1).to(torch.int32).contiguous()
        w, cams = make_weed(cam_infos, standard_dist, fork, levels, dist2level, visible_threshold)
        one_device(("positions", pos), ("cam_infos", cams))
        count = torch.empty(U, dtype=torch.int32, device=pos.device)
        keep = torch.empty(U, dtype=torch.uint8, device=pos.device)
        call("gsr_octree_weed_out", pos.device, pos, lv, U, C.byref(w), count, keep)
        return count, keep.view(torch.bool)
