"""The mesh of an unbounded scene on the device: GaussianExtractor.extract_mesh_unbounded (gssr/utils/mesh_utils.py:181-277) and the
marching_cubes_with_contraction it drives (gssr/utils/mcube_utils.py:17-95) -- the `--unbounded` branch of extract_mesh.py.

The reference materialises 134 M points per 512^3 crop, read-modify-writes them once per camera, copies the volume to the host for skimage, welds the crops
with trimesh and integrates every frame a second time at the vertices.  Here (include/gsrast.h, gsr_unbounded_*; csrc/gsr_unbounded.hip):
  lattice_tsdf            every frame over every lattice sample in one launch, state in registers, 4 B stored per sample
  lattice_marching_cubes  count / scan / emit over slabs of x-planes, vertices welded by edge identity, one host read per slab
  finish_vertices         un-contraction and clip
  texture_vertices        the second fusion pass, fused over the frames, 12 B stored per vertex
There is no CPU path, and marching-cubes parity with skimage / trimesh is unpinned: the mesh is defined by the contract in include/gsrast.h."""
import ctypes as C

import numpy as np
import torch

from . import call, dev_f32, lib, scratch
from .tsdf import TriangleMesh

DEFAULT_SLAB = 32       # x-planes per slab of extract_mesh_unbounded (33 are read): at 1023^2 points per plane 0.14 GB of samples and 0.14 GB of scratch


def lattice_axes(bounding_box_min, bounding_box_max, resolution, crop=512):
    """-> three HOST float32 arrays: the distinct sample planes per axis of the reference's crops (mcube_utils.py:28-52).  Per axis N = resolution / crop
    blocks; block b samples torch.linspace(lo_b, hi_b, crop) in float32 on the CPU, lo_b / hi_b out of np.linspace(min, max, N + 1).  Adjacent blocks
    share their boundary sample -- asserted bit-equal -- so an axis has N * (crop - 1) + 1 planes."""
    resolution, crop = int(resolution), int(crop)
    if crop < 2 or resolution % crop != 0 or resolution < crop:
        raise RuntimeError(f"lattice_axes: resolution {resolution} must be a positive multiple of crop {crop} >= 2")
    N = resolution // crop
    axes = []
    for a in range(3):
        edges = np.linspace(bounding_box_min[a], bounding_box_max[a], N + 1)
        blocks = [torch.linspace(edges[b], edges[b + 1], crop).numpy() for b in range(N)]
        for b in range(1, N):
            assert blocks[b - 1][-1].tobytes() == blocks[b][0].tobytes(), "adjacent crops do not share their boundary sample"
        ax = np.concatenate([blocks[0]] + [blk[1:] for blk in blocks[1:]]).astype(np.float32)
        assert ax.shape[0] == N * (crop - 1) + 1
        axes.append(ax)
    return tuple(axes)


def _axes(xs, ys, zs, device):
    out = []
    for a, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):
        t = torch.as_tensor(a, dtype=torch.float32).to(device).contiguous()
        if t.dim() != 1 or t.numel() < 2:
            raise RuntimeError(f"{n}: an axis is a 1-D array of at least 2 ascending samples")
        out.append(t)
    return out


def _center(center):
    """-> HOST float[3] for the C ABI; a converted centre passes through (a device tensor costs one host read: callers with a slab loop convert once)."""
    if isinstance(center, C.Array):
        return center
    c = torch.as_tensor(center, dtype=torch.float32).reshape(-1).cpu().tolist()
    if len(c) != 3:
        raise RuntimeError("center must have 3 components")
    return (C.c_float * 3)(*c)


def _f32(x):
    return float(np.float32(x))


def _frames(full_proj, depth, rgb=None):
    """-> [(full_proj [F,16], depth [F,H,W], rgb [F,3,H,W] or None)] per run of consecutive frames of one size, in frame order (the running average is
    order dependent).  depth / rgb: a tensor [F,1,H,W] / [F,3,H,W] or a list of per-frame maps."""
    P = dev_f32(torch.as_tensor(full_proj) if not isinstance(full_proj, (list, tuple)) else torch.stack(list(full_proj)), "full_proj", allow_empty=False)
    P = P.reshape(-1, 16)
    F = int(P.shape[0])
    if isinstance(depth, torch.Tensor):
        d = dev_f32(depth, "depth", allow_empty=False)
        H, W = int(d.shape[-2]), int(d.shape[-1])
        d = d.reshape(-1, H, W)
        c = None
        if rgb is not None:
            c = dev_f32(rgb if isinstance(rgb, torch.Tensor) else torch.stack(list(rgb)), "rgb", allow_empty=False).reshape(-1, 3, H, W)
        if int(d.shape[0]) != F or (c is not None and int(c.shape[0]) != F):
            raise RuntimeError("full_proj, depth and rgb must hold the same number of frames")
        return [(P, d, c)]
    maps = list(depth)
    if len(maps) != F or (rgb is not None and len(rgb) != F):
        raise RuntimeError("full_proj, depth and rgb must hold the same number of frames")
    groups, s = [], 0
    while s < F:
        e = s + 1
        while e < F and tuple(maps[e].shape[-2:]) == tuple(maps[s].shape[-2:]):
            e += 1
        H, W = int(maps[s].shape[-2]), int(maps[s].shape[-1])
        d = dev_f32(torch.stack([m.reshape(H, W) for m in maps[s:e]]), "depth", allow_empty=False)
        c = None if rgb is None else dev_f32(torch.stack([m.reshape(3, H, W) for m in rgb[s:e]]), "rgb", allow_empty=False)
        groups.append((P[s:e].contiguous(), d, c))
        s = e
    return groups


def lattice_points(xs, ys, zs, center, radius, voxel_size, device="cuda"):
    """-> (points [V,3] world, sdf_trunc [V]) of every lattice sample, V = nx * ny * nz, z fastest: what the per-frame op gsrast.tsdf.tsdf_integrate_
    takes -- the un-contraction and adaptive truncation of the contract, from the device function lattice_tsdf uses."""
    device = torch.device(device)
    xs, ys, zs = _axes(xs, ys, zs, device)
    V = xs.numel() * ys.numel() * zs.numel()
    pts = torch.empty((V, 3), dtype=torch.float32, device=device)
    tr = torch.empty((V,), dtype=torch.float32, device=device)
    call("gsr_unbounded_lattice_points", device, xs.numel(), ys.numel(), zs.numel(), xs, ys, zs, _center(center), _f32(radius), _f32(voxel_size), pts, tr)
    return pts, tr


def lattice_tsdf(xs, ys, zs, center, radius, voxel_size, full_proj, depth, state=None, device="cuda"):
    """-> tsdf [nx,ny,nz]: every frame fused over every sample (full_proj [F,4,4], depth [F,1,H,W] or a list of [1,H,W] maps of any sizes), bit for bit
    what lattice_points + one tsdf_integrate_ per frame leave.  Frames of one launch share W and H: a ragged list runs as one launch per run of
    equal-sized frames, with (tsdf, weight) carried between them -- the single-size path allocates no weight.  state: an optional (tsdf, weight) pair
    to continue from, updated in place; then (tsdf, weight) is returned."""
    device = torch.device(device)
    return _lattice_groups(_axes(xs, ys, zs, device), _center(center), radius, voxel_size, _frames(full_proj, depth), state, device)


def _lattice_groups(axes, c, radius, voxel_size, groups, state, device):
    """lattice_tsdf on device axes, a converted centre and the frame groups of _frames."""
    xs, ys, zs = axes
    shape = (xs.numel(), ys.numel(), zs.numel())
    if state is not None:
        tsdf, weight = state
        for t, n in ((tsdf, "tsdf"), (weight, "weight")):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
                raise RuntimeError(f"state {n} must be a contiguous float32 CUDA tensor of shape {shape}")
    else:
        tsdf = torch.empty(shape, dtype=torch.float32, device=device)
        weight = None
        if len(groups) > 1:
            tsdf.fill_(1.0)
            weight = torch.ones(shape, dtype=torch.float32, device=device)
    for P, d, _ in groups:
        call("gsr_unbounded_lattice_tsdf", device, shape[0], shape[1], shape[2], xs, ys, zs, c, _f32(radius), _f32(voxel_size), int(P.shape[0]), P,
             int(d.shape[-1]), int(d.shape[-2]), d, tsdf, weight)
    return tsdf if state is None else (tsdf, weight)


def slab_plan(nx, slab):
    """-> [(x0, own, planes)]: the slabs of an axis of nx planes.  A slab owns the points and cubes of planes [x0, x0 + own) and reads `planes` planes from
    x0 on.  slab None or >= nx: one slab owning everything.  Otherwise a slab owns slab - 1 planes, shares the next one with its successor and reads ONE
    more behind that -- slab + 1 planes in all: the cubes of its last layer name vertices of the shared plane, whose numbers depend on that plane's x
    edges.  The last slab ends the lattice and owns all it reads (at most slab planes)."""
    if slab is None or int(slab) >= nx:
        return [(0, nx, nx)]
    slab = int(slab)
    if slab < 2:
        raise RuntimeError("slab: at least 2 x-planes")
    out, x0 = [], 0
    while True:
        if x0 + slab >= nx:                     # the rest fits one slab
            out.append((x0, nx - x0, nx - x0))
            return out
        out.append((x0, slab - 1, slab + 1))
        x0 += slab - 1


def _mc_slab(f, xs, ys, zs, own, vbase, tbase):
    """One slab through count and emit: -> (vertices [v,3], triangles [t,3]); f [np,ny,nz], xs [np]."""
    L = lib()
    device = f.device
    np_, ny, nz = (int(v) for v in f.shape)
    nbytes = int(L.gsr_unbounded_mc_scratch_bytes(np_, ny, nz))
    work = scratch(nbytes, device)
    counts = (C.c_uint64 * 2)()
    call("gsr_unbounded_mc_count", device, np_, ny, nz, own, f, work, nbytes, vbase, tbase, counts)
    nv, nt = int(counts[0]), int(counts[1])
    verts = torch.empty((nv, 3), dtype=torch.float32, device=device)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=device)
    if nv or nt:
        call("gsr_unbounded_mc_emit", device, np_, ny, nz, own, f, xs, ys, zs, work, nbytes, vbase, nv, nt, verts, tris)
    return verts, tris


def _run(label, fn):
    return fn()


def _cubes_in_slabs(axes, slab, slab_tsdf, stage=_run):
    """THE slab loop: per slab of the plan, slab_tsdf(x0, planes, slab_axes) -> its samples, then count / emit, then append.  stage(label, fn) runs a
    piece (a hook for timing).  -> (vertices [V,3] contracted, triangles [T,3])."""
    xs, ys, zs = axes
    device = xs.device
    V, T, vs, ts = 0, 0, [], []
    for x0, own, np_ in slab_plan(xs.numel(), slab):
        sx = xs[x0:x0 + np_]
        f = stage("lattice", lambda: slab_tsdf(x0, np_, (sx, ys, zs)))
        v, t = stage("cubes", lambda: _mc_slab(f, sx, ys, zs, own, V, T))
        vs.append(v); ts.append(t); V += int(v.shape[0]); T += int(t.shape[0])
        del f

    def cat(parts, cols, dtype):
        parts = [p for p in parts if p.shape[0]]
        return parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.empty((0, cols), dtype=dtype, device=device)
    return stage("cubes", lambda: (cat(vs, 3, torch.float32), cat(ts, 3, torch.int32)))


def lattice_marching_cubes(tsdf, xs, ys, zs, slab=None):
    """-> (vertices [V,3] float32 in CONTRACTED coordinates, triangles [T,3] int32): marching cubes at level 0 over the dense lattice tsdf [nx,ny,nz] with
    axes xs, ys, zs, in the canonical order of the contract (vertices by (gx, gy, gz, axis), triangles by cube, then table order).  Worked in slabs
    (slab_plan: slab - 1 x-planes owned, slab + 1 read; None: one slab); scratch is bounded by the slab and the result does not depend on it.  One host
    read per slab.  An empty result is an empty mesh."""
    f = dev_f32(tsdf, "tsdf", allow_empty=False)
    axes = _axes(xs, ys, zs, f.device)
    if tuple(f.shape) != tuple(a.numel() for a in axes):
        raise RuntimeError("tsdf must be [nx,ny,nz] for the given axes")
    return _cubes_in_slabs(axes, slab, lambda x0, np_, _: f[x0:x0 + np_])


def finish_vertices(vertices, center, radius, max_range=32.0):
    """Contracted vertices -> world, IN PLACE: the un-contraction of the contract, then the clip to +-max_range in world coordinates
    (mcube_utils.py:91-93)."""
    v = vertices
    if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.dim() == 2 and v.shape[1] == 3):
        raise RuntimeError("vertices must be a contiguous float32 CUDA tensor [V,3]")
    call("gsr_unbounded_finish", v.device, int(v.shape[0]), _center(center), _f32(radius), _f32(max_range), v)
    return v


def texture_vertices(vertices, voxel_size, full_proj, depth, rgb):
    """-> colors [V,3]: the reference's second compute_unbounded_tsdf call (inv_contraction=None, scalar truncation 5 * voxel_size, return_rgb=True) at
    world-space vertices, fused over the frames (rgb [F,3,H,W] or a list of [3,H,W] maps); bit for bit what one tsdf_integrate_ per frame leaves in rgbs.
    Frames must share one size."""
    v = dev_f32(vertices, "vertices", allow_empty=True)
    groups = _frames(full_proj, depth, rgb)
    if len(groups) != 1:
        raise RuntimeError("texture_vertices: frames of one call share W and H")
    P, d, c = groups[0]
    V = 0 if v is None else int(v.shape[0])
    out = torch.empty((V, 3), dtype=torch.float32, device=P.device)
    if V:
        call("gsr_unbounded_texture", P.device, V, v, _f32(voxel_size), int(P.shape[0]), P, int(d.shape[-1]), int(d.shape[-2]), d, c, out)
    return out


def contraction_bound(xyz, center, radius):
    """-> float: the reference's R = min(np.quantile(|contract((xyz - center) / radius)|, 0.95) + 0.01, 1.9) (mesh_utils.py:258-260), on the device with one
    host read: two order statistics and numpy's linear interpolation between them (torch.quantile refuses large inputs)."""
    x = dev_f32(xyz, "xyz", allow_empty=False).reshape(-1, 3)
    c = torch.as_tensor(center, dtype=torch.float32).reshape(1, 3).to(x.device)
    y = (x - c) / _f32(radius)
    mag = torch.linalg.norm(y, ord=2, dim=-1)[..., None]
    y = torch.where(mag < 1, y, (2 - (1 / mag)) * (y / mag))
    r = y.norm(dim=-1)
    n = int(r.shape[0])
    pos = 0.95 * (n - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    a = torch.stack([torch.kthvalue(r, lo + 1).values, torch.kthvalue(r, hi + 1).values]).cpu().numpy()      # the one host read
    frac = pos - lo
    q = float(a[0]) + (float(a[1]) - float(a[0])) * frac
    return float(min(q + 0.01, 1.9))


def marching_cubes_with_contraction(full_proj, depthmaps, center, radius, voxel_size, resolution=512, bounding_box_min=(-1.0, -1.0, -1.0),
                                    bounding_box_max=(1.0, 1.0, 1.0), level=0, max_range=32.0, crop=512, slab=DEFAULT_SLAB, device="cuda", stage=_run):
    """-> (vertices [V,3] world, triangles [T,3]): the reference's function of that name with its sdf callable (compute_unbounded_tsdf over the frames)
    and its inv_contraction folded in.  Slab by slab (slab_plan): lattice -> cubes -> append; then un-contraction and clip.  level is 0 (the reference
    overrides it, mcube_utils.py:32).  stage(label, fn): an optional hook that runs each piece ("lattice", "cubes", "finish"), for timing."""
    if level != 0:
        raise RuntimeError("marching_cubes_with_contraction: level is 0")
    device = torch.device(device)
    axes = _axes(*lattice_axes(bounding_box_min, bounding_box_max, resolution, crop), device)
    groups = _frames(full_proj, depthmaps)
    c = _center(center)                          # once: a device tensor costs a host read
    verts, tris = _cubes_in_slabs(axes, slab, lambda x0, np_, sa: _lattice_groups([a.contiguous() for a in sa], c, radius, voxel_size, groups, None, device),
                                  stage)
    return stage("finish", lambda: finish_vertices(verts, c, radius, max_range)), tris


def extract_mesh_unbounded(full_proj, depthmaps, rgbmaps, xyz, center, radius, resolution=1024, crop=512, slab=DEFAULT_SLAB, max_range=32.0, stage=_run):
    """-> gsrast.tsdf.TriangleMesh: GaussianExtractor.extract_mesh_unbounded(resolution) (mesh_utils.py:181-277).  full_proj [F,4,4]: the cameras'
    full_proj_transform; depthmaps [F,1,H,W], rgbmaps [F,3,H,W] (or per-frame lists); xyz: the Gaussians' positions (the bound of the lattice is the
    0.95 quantile of their contracted norm); center, radius: the extractor's.  The result feeds post_process_mesh and write_triangle_mesh unchanged.
    stage(label, fn): an optional hook that runs each piece ("bound", "lattice", "cubes", "finish", "texture"), for timing."""
    P = dev_f32(torch.as_tensor(full_proj) if not isinstance(full_proj, (list, tuple)) else torch.stack(list(full_proj)), "full_proj", allow_empty=False)
    voxel_size = np.float32(radius * 2 / int(resolution))
    c = _center(center)
    R = stage("bound", lambda: contraction_bound(xyz, torch.tensor(list(c)), radius))
    verts, tris = marching_cubes_with_contraction(P, depthmaps, c, radius, voxel_size, resolution=resolution, bounding_box_min=(-R, -R, -R),
                                                  bounding_box_max=(R, R, R), level=0, max_range=max_range, crop=crop, slab=slab, device=P.device, stage=stage)
    colors = stage("texture", lambda: texture_vertices(verts, voxel_size, P, depthmaps, rgbmaps))
    return TriangleMesh(verts, colors, tris)
