"""Floaters filtered from an extracted mesh on the device: `post_process_mesh` of the reference (gssr/utils/mesh_utils.py:28-48, called by
extract_mesh.py:130-134 and extract_mesh_split.py:122-127 on what `extract_triangle_mesh()` returned) and the Open3D call it starts with,
`cluster_connected_triangles`.  Open3D is not part of the reference tree: PARITY UNPINNED (semantics restated from Open3D 0.18's published
sources in include/gsrast.h, gsr_mesh_*; kernels in csrc/gsr_mesh_post.hip).  Every integer result is exact and a pure function of the index
buffer; the cluster areas are added up with double atomics and are the one result that is not bit-reproducible.

`simplify_vertex_clustering` is the step after it: the mesh made smaller by vertex clustering (csrc/gsr_mesh_simplify.hip), the role
of Open3D's call of that name with semantics of this project's own -- no float atomics, every output bit-reproducible.

`vertex_adjacency`, `filter_smooth_simple` / `_laplacian` / `_taubin` and `compute_triangle_normals` / `compute_vertex_normals` take the voxel-scale
ripple off such a mesh and give it normals (csrc/gsr_mesh_smooth.hip), again with semantics of this project's own: every sum in a
stated order, float64 state, no float atomics.

`rasterize_mesh`, `triangle_view_counts` and `cull_unseen_triangles` look at the mesh from the cameras it was fused from (csrc/gsr_mesh_raster.hip;
DESIGN.md 4.16): depth, triangle id and barycentrics per pixel, and the triangles no camera saw taken out -- semantics of this project's own, float64
and integer, bit-reproducible.

There is no CPU path: a mesh that is not on a HIP device raises, like ScalableTSDFVolume."""
import ctypes as C
import math

import numpy as np
import torch

from . import call, lib, scratch
from ._abi import gsr_mesh_filter as Filter, gsr_rows_tensor as RowsTensor

DROP_UNREFERENCED, DROP_DEGENERATE = 1, 2             # include/gsrast.h GSR_MESH_DROP_*
ERR_INDEX, ERR_INTERNAL, ERR_KEEP = 1, 2, 4           # GSR_MESH_ERR_*
ERR_RANGE, ERR_NONFINITE = 8, 16                      # GSR_MESH_ERR_* of the simplification
SIMPLIFY_AVERAGE, SIMPLIFY_QUADRIC = 0, 1             # GSR_SIMPLIFY_*
CONTRACTIONS = {"average": SIMPLIFY_AVERAGE, "quadric": SIMPLIFY_QUADRIC}
CELL_LIMIT = 1 << 21                                  # simplify_vertex_clustering: cells per axis at most
FLOOR = 50                                            # mesh_utils.py:41 "filter meshes smaller than 50"


def _arrays(mesh):
    """(vertices, vertex_colors, triangles) of a TriangleMesh, checked: contiguous float32 [V,3] x 2 and int32 [T,3] on one HIP device."""
    v, c, t = mesh.vertices, mesh.vertex_colors, mesh.triangles
    for x, name, dt in ((v, "vertices", torch.float32), (c, "vertex_colors", torch.float32), (t, "triangles", torch.int32)):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"mesh.{name} must be a tensor")
        if not x.is_cuda:
            raise RuntimeError(f"mesh.{name} must be a CUDA tensor: the mesh filter has no CPU path")
        if x.dtype != dt or x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError(f"mesh.{name}: expected a {dt} tensor of shape [n, 3] but found {x.dtype} {list(x.shape)}")
    if v.device != t.device or c.device != t.device:
        raise RuntimeError("mesh: vertices, vertex_colors and triangles must be on one device")
    if c.shape[0] != v.shape[0]:
        raise RuntimeError(f"mesh.vertex_colors: expected {v.shape[0]} rows but found {c.shape[0]}")
    return v.contiguous(), c.contiguous(), t.contiguous()


def _scratch(T, V, dev):
    n = int(lib().gsr_mesh_post_scratch_bytes(T, V))
    if n == 0:
        raise RuntimeError(f"mesh: {T} triangles / {V} vertices: 3T must stay below 2^31 (the half-edges are indexed with 32 bits); filter the mesh in parts")
    return scratch(n, dev), n


def _raise_status(status):
    if status & ERR_INDEX:
        raise RuntimeError("mesh: a triangle index lies outside [0, number of vertices)")
    if status & ERR_INTERNAL:
        raise RuntimeError("mesh: internal error, a bounded loop of the clustering ran out")


def cluster_connected_triangles(mesh, with_area=True):
    """-> (triangle_clusters int32 [T], cluster_n_triangles int32 [C], cluster_area float64 [C] or None), device tensors: Open3D's
    `TriangleMesh.cluster_connected_triangles()`.  Two triangles are connected iff they share an undirected edge; clusters are numbered in
    ascending order of their smallest triangle.  The integer results are exact; the areas are sums of double atomics, equal to the float64 sum
    up to the order of the additions (not bit-reproducible).  One host read-back (the number of clusters)."""
    v, _, t = _arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    clusters = torch.empty(T, dtype=torch.int32, device=dev)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    area = torch.empty(T, dtype=torch.float64, device=dev) if with_area else None
    work, nbytes = _scratch(T, 0, dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    call("gsr_mesh_cluster_triangles", dev, t, T, V, v if with_area else None, clusters, counts, area, work, nbytes, status)
    st, n = status.tolist()
    _raise_status(st)
    return clusters, counts[:n].clone(), (area[:n].clone() if with_area else None)


def _filter(mesh, remove_mask=None, cluster_to_keep=0, flags=0):
    """One count call, the one host read-back, one emit call -> (vertices, vertex_colors, triangles, record); the mesh is only read.  Without
    DROP_UNREFERENCED the vertex tensors are the mesh's own."""
    v, c, t = _arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    f = Filter(t.data_ptr() if T else None, None if remove_mask is None else remove_mask.data_ptr(), T, V, int(cluster_to_keep), FLOOR, int(flags), 0)
    work, nbytes = _scratch(T, V, dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    L = lib()
    call("gsr_mesh_filter_count", dev, C.byref(f), work, nbytes, record)
    rec = [x & 0xFFFFFFFF for x in record.tolist()]                       # the host read-back
    if rec[0] & ERR_KEEP and not rec[0] & (ERR_INDEX | ERR_INTERNAL):
        raise IndexError(f"index -{cluster_to_keep} is out of bounds for axis 0 with size {rec[1]}")      # numpy's words for n[-cluster_to_keep]
    _raise_status(rec[0])
    n_v, n_t = rec[3], rec[4]
    tris = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
    rows, n_rows = None, 0
    if flags & DROP_UNREFERENCED:
        nv, nc = torch.empty((n_v, 3), dtype=torch.float32, device=dev), torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        rows, n_rows = (RowsTensor * 2)(RowsTensor(v.data_ptr(), nv.data_ptr(), None, 12, 0), RowsTensor(c.data_ptr(), nc.data_ptr(), None, 12, 0)), 2
    else:
        nv, nc = v, c
    call("gsr_mesh_filter_emit", dev, C.byref(f), work, nbytes, (C.c_uint32 * 8)(*rec), n_rows, rows, tris if n_t else None)
    return nv, nc, tris, rec


def post_process_mesh(mesh, cluster_to_keep=1000):
    """The reference's post_process_mesh (gssr/utils/mesh_utils.py:28-48) on the device -> a new TriangleMesh on the mesh's device; the input is
    left untouched (the reference deep-copies it).
      1. n = sort(cluster_n_triangles); threshold = max(n[-cluster_to_keep], 50)
      2. triangles whose cluster has fewer triangles than the threshold go (strictly fewer: ties stay); the others keep their order
      3. vertices no surviving triangle references go; order kept, colours move with their vertices bit for bit, triangle indices renumbered
      4. triangles with two equal indices go, after step 3: a vertex only such a triangle references stays, as in the reference
    cluster_to_keep larger than the number of clusters (an empty mesh included) raises IndexError, as numpy does in the reference;
    cluster_to_keep < 1 raises ValueError -- a departure: there a negative index quietly selects from the other end, which means nothing.
    Exactly ONE host read-back per call: the five-word record {status, clusters, threshold, vertices kept, triangles kept} between the
    counting and the emitting pass.  Parity with Open3D unpinned (module docstring)."""
    from .tsdf import TriangleMesh
    if int(cluster_to_keep) != cluster_to_keep or cluster_to_keep < 1:
        raise ValueError(f"cluster_to_keep must be a positive integer but found {cluster_to_keep}")
    if cluster_to_keep > 0x7FFFFFFF:
        _arrays(mesh)
        raise IndexError(f"index -{cluster_to_keep} is out of bounds for axis 0")
    v, c, t, _ = _filter(mesh, cluster_to_keep=int(cluster_to_keep), flags=DROP_UNREFERENCED | DROP_DEGENERATE)
    return TriangleMesh(v, c, t)


def _simplify(mesh, voxel_size, contraction, want_map):
    """One count call, the one host read-back, one emit call -> (vertices, vertex_colors, triangles, vertex_map or None, record)."""
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)} but found {contraction!r}")
    vs = float(voxel_size)
    if not (vs > 0.0) or math.isinf(vs):
        raise ValueError(f"voxel_size must be a positive finite number but found {voxel_size}")
    v, c, t = _arrays(mesh)
    T, V, dev, mode = int(t.shape[0]), int(v.shape[0]), t.device, CONTRACTIONS[contraction]
    if V == 0 and T == 0:                                                 # nothing to launch
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev),
                torch.empty((0, 3), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev) if want_map else None, [0, 0, 0, 0])
    nbytes = int(lib().gsr_mesh_simplify_scratch_bytes(T, V, mode))
    if nbytes == 0:
        raise RuntimeError(f"mesh: {T} triangles / {V} vertices: V and 3T must stay below 2^31; simplify the mesh in parts")
    work = scratch(nbytes, dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    call("gsr_mesh_simplify_count", dev, v if V else None, V, t if T else None, T, vs, mode, work, nbytes, record)
    rec = [x & 0xFFFFFFFF for x in record.tolist()]                       # the host read-back
    if rec[0] & ERR_NONFINITE:
        raise RuntimeError("mesh: a vertex has a non-finite component (NaN or inf)")
    if rec[0] & ERR_RANGE:
        extent = (v.max(0).values.double() - v.min(0).values.double()).tolist()      # the error path reads back once more, to name the figures
        raise RuntimeError(f"mesh: extent {extent} at voxel_size {vs} spans {max(extent) / vs:.4g} cells along an axis, the limit is 2^21 = {CELL_LIMIT}: "
                           f"use a larger voxel_size or simplify the mesh in parts")
    _raise_status(rec[0])
    n_v, n_t = rec[1], rec[2]
    nv, nc = torch.empty((n_v, 3), dtype=torch.float32, device=dev), torch.empty((n_v, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev) if want_map else None
    call("gsr_mesh_simplify_emit", dev, v if V else None, c if V else None, V, T, vs, mode, work, nbytes, (C.c_uint32 * 8)(*rec), nv if n_v else None,
         nc if n_v else None, tris if n_t else None, vmap if want_map and V else None)
    return nv, nc, tris, vmap, rec[:4]


def simplify_vertex_clustering(mesh, voxel_size, contraction="average", return_map=False):
    """The mesh made smaller by vertex clustering -> a new TriangleMesh on the mesh's device (and, with return_map, vertex_map int32 [V]: the new
    index of every old vertex); the input is only read.  The role of Open3D's `simplify_vertex_clustering`; the semantics are this project's own
    (include/gsrast.h, "mesh simplification") and every result is deterministic, bit for bit from run to run:
      1. origin = float64(per-axis minimum over all vertices) - voxel_size / 2; the cell of a vertex is floor((float64(v) - origin) / voxel_size)
      2. one new vertex per occupied cell, numbered by the cell's lowest member; unreferenced vertices are clustered like any other
      3. position and colour: the float64 mean of the members, added in ascending vertex index, rounded to float32
      4. contraction="quadric": the minimiser of the cell's summed triangle-plane quadrics instead, where it exists and lies inside the cell's
         closed box; flat and edge-like cells fall back to the mean by themselves.  Colours are always the mean.
      5. triangles are re-indexed; those with two equal indices go; each is rotated to start with its smallest index, and of equal triples the
         first stays (a mirrored triple is another triple); survivors keep their order.
    Raises RuntimeError for a mesh that spans 2^21 cells or more along an axis, for a non-finite vertex and for a triangle index outside [0, V);
    ValueError for a voxel_size that is not a positive finite number or an unknown contraction.  An empty mesh gives an empty mesh.
    Exactly ONE host read-back per call: the record {status, vertices, triangles, quadric cells} between the counting and the emitting pass."""
    from .tsdf import TriangleMesh
    nv, nc, tris, vmap, _ = _simplify(mesh, voxel_size, contraction, return_map)
    out = TriangleMesh(nv, nc, tris)
    return (out, vmap) if return_map else out


SMOOTH_SIMPLE, SMOOTH_LAPLACIAN, SMOOTH_TAUBIN = 0, 1, 2    # GSR_SMOOTH_*
SCOPES = {"all": 0, "vertex": 1}                           # GSR_SMOOTH_SCOPE_*


def _limits(T, V, rule="V must stay below 2^31 and 6T within 2^32 - 4096"):
    return RuntimeError(f"mesh: {T} triangles / {V} vertices: {rule}; process the mesh in parts")


def _raise_smooth_status(status):
    if status & ERR_NONFINITE:
        raise RuntimeError("mesh: a vertex has a non-finite component (NaN or inf)")
    _raise_status(status)


def vertex_adjacency(mesh):
    """-> (start int32 [V + 1], neighbours int32 [E]) as device tensors: the vertex -> vertex adjacency of the index buffer as a CSR.
    N(i) = neighbours[start[i] : start[i + 1]] is the set of j != i that share at least one triangle with i, distinct and ascending; a triangle with
    two equal indices adds no self-loop and still connects its two distinct vertices (include/gsrast.h, "mesh smoothing and normals").
    Raises RuntimeError for a triangle index outside [0, V).  Exactly ONE host read-back per call: the record {status, E} between the counting and
    the emitting pass."""
    v, _, t = _arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    nbytes = int(lib().gsr_mesh_adjacency_scratch_bytes(T, V))
    if nbytes == 0:
        raise _limits(T, V)
    work = scratch(nbytes, dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    call("gsr_mesh_adjacency_count", dev, t if T else None, T, V, work, nbytes, record)
    rec = [x & 0xFFFFFFFF for x in record.tolist()]                       # the host read-back
    _raise_status(rec[0])
    start = torch.empty(V + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(rec[1], dtype=torch.int32, device=dev)
    call("gsr_mesh_adjacency_emit", dev, T, V, work, nbytes, (C.c_uint32 * 8)(*rec), start, neighbours if rec[1] else None)
    return start, neighbours


def _normals(mesh, normalized, want_triangle, want_vertex):
    """One call, one read-back (the status word) -> (triangle_normals or None, vertex_normals or None)."""
    v, _, t = _arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    nbytes = int(lib().gsr_mesh_normals_scratch_bytes(T, V))
    if nbytes == 0:
        raise _limits(T, V)
    work = scratch(nbytes if want_vertex else 1, dev)
    tn = torch.empty((T, 3), dtype=torch.float32, device=dev) if want_triangle else None
    vn = torch.empty((V, 3), dtype=torch.float32, device=dev) if want_vertex else None
    status = torch.empty(2, dtype=torch.int32, device=dev)
    call("gsr_mesh_normals", dev, v if V else None, V, t if T else None, T, 1 if normalized else 0, tn, vn, work, nbytes if want_vertex else 0, status)
    _raise_status(status.tolist()[0] & 0xFFFFFFFF)                        # the host read-back
    return tn, vn


def compute_triangle_normals(mesh, normalized=True):
    """-> triangle_normals float32 [T,3] on the mesh's device: n = (v1 - v0) x (v2 - v0) in float64 from the float32 vertices, divided by its length
    when `normalized` -- (0, 0, 1) where that length is 0 or not finite -- and rounded to float32 once.  The role of Open3D's
    `compute_triangle_normals`; the semantics are this project's own (include/gsrast.h), parity with Open3D unpinned.
    Exactly ONE host read-back per call: the status word."""
    return _normals(mesh, normalized, True, False)[0]


def compute_vertex_normals(mesh, normalized=True):
    """-> vertex_normals float32 [V,3] on the mesh's device: per vertex the float64 sum of the UNNORMALISED normals of the triangles that reference
    it (area weighting), added in ascending corner index 3 t + k, then normalised like a triangle normal (or left as the sum) and rounded to float32
    once.  A vertex no triangle references gets (0, 0, 1) when normalised and (0, 0, 0) when not.  No float atomics: two runs give the same bits.
    The role of Open3D's `compute_vertex_normals`, parity unpinned.  Exactly ONE host read-back per call: the status word."""
    return _normals(mesh, normalized, False, True)[1]


def _smooth(mesh, kind, number_of_iterations, lam, mu, filter_scope):
    """The argument checks, one call, one read-back (the status word) -> a new TriangleMesh."""
    from .tsdf import TriangleMesh
    n = number_of_iterations
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n > 0x3FFFFFFF:
        raise ValueError(f"number_of_iterations must be a non-negative integer but found {n!r}")
    if filter_scope not in SCOPES:
        raise ValueError(f"filter_scope must be one of {sorted(SCOPES)} but found {filter_scope!r}")
    for name, x in (("lambda_filter", lam), ("mu", mu)):
        if not math.isfinite(float(x)):
            raise ValueError(f"{name} must be a finite number but found {x}")
    v, c, t = _arrays(mesh)
    T, V, dev = int(t.shape[0]), int(v.shape[0]), t.device
    nbytes = int(lib().gsr_mesh_smooth_scratch_bytes(T, V, SCOPES[filter_scope]))
    if nbytes == 0:
        raise _limits(T, V)
    work = scratch(nbytes, dev)
    nv, nc = torch.empty((V, 3), dtype=torch.float32, device=dev), torch.empty((V, 3), dtype=torch.float32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    call("gsr_mesh_smooth", dev, v if V else None, c if V else None, V, t if T else None, T, kind, int(n), float(lam), float(mu), SCOPES[filter_scope],
         nv if V else None, nc if V else None, work, nbytes, status)
    tris = t.clone()
    _raise_smooth_status(status.tolist()[0] & 0xFFFFFFFF)                 # the host read-back
    return TriangleMesh(nv, nc, tris)


def filter_smooth_simple(mesh, number_of_iterations=1, filter_scope="all"):
    """-> a NEW mesh: per iteration every vertex becomes the mean of itself and its neighbours, q_i = (p_i + sum p_j) / (|N(i)| + 1).  See
    filter_smooth_taubin for what all three filters share."""
    return _smooth(mesh, SMOOTH_SIMPLE, number_of_iterations, 0.0, 0.0, filter_scope)


def filter_smooth_laplacian(mesh, number_of_iterations=1, lambda_filter=0.5, filter_scope="all"):
    """-> a NEW mesh: per iteration q_i = p_i + lambda * (sum w_ij p_j / sum w_ij - p_i) with w_ij = 1 / (|p_i - p_j| + 1e-12) on the positions of
    the iteration's input.  It shrinks the mesh; filter_smooth_taubin does not.  See there for what all three filters share."""
    return _smooth(mesh, SMOOTH_LAPLACIAN, number_of_iterations, lambda_filter, 0.0, filter_scope)


def filter_smooth_taubin(mesh, number_of_iterations=1, lambda_filter=0.5, mu=-0.53, filter_scope="all"):
    """-> a NEW mesh: per iteration a Laplacian step with lambda_filter, then one with mu (negative: it undoes the shrinkage of the first).
    The role of Open3D's `filter_smooth_taubin` / `_laplacian` / `_simple`; the semantics are this project's own (include/gsrast.h, "mesh smoothing
    and normals"), parity with Open3D unpinned.  What the three filters share:
      * N(i), the vertices that share a triangle with i, is walked in ascending order and every sum is added one term after another in float64;
        the state stays float64 from the first iteration to the last and is rounded to float32 once.  No float atomics: two runs give the same bits.
      * filter_scope="all" filters positions and colours (the colours with the positions' weights; they are the only further channel that is
        filtered), "vertex" positions only: the colours are copied bit for bit.
      * a vertex without neighbours stays where it is -- a departure from the model, which divides 0 by 0 there.
      * number_of_iterations=0 returns a copy, bit for bit.  The new mesh has a copy of the input's triangles and NO normals: compute_vertex_normals
        is one call.
    Raises ValueError before any launch for a negative or non-integer number_of_iterations, a non-finite lambda_filter / mu or an unknown
    filter_scope; RuntimeError for a triangle index outside [0, V), a non-finite vertex, a host mesh or a mesh past V < 2^31, 6T <= 2^32 - 4096.
    Exactly ONE host read-back per call, whatever the number of iterations: the status word, behind all the steps."""
    return _smooth(mesh, SMOOTH_TAUBIN, number_of_iterations, lambda_filter, mu, filter_scope)


LARGE_FROM = 64                                           # candidate pixels above which a triangle is swept by a wave (the sweep)


class MeshRaster:
    """What rasterize_mesh returns, all device tensors: depth float32 [V,H,W] (0 where no triangle covers the pixel), triangle_id int32 [V,H,W]
    (-1 there), barycentric float32 [V,H,W,2] or None (the perspective-correct weights of the winner's vertices 1 and 2 in the index buffer's order;
    vertex 0 has 1 minus their sum), dropped int32 [V,3]: the triangles each view dropped as {near, guard, zero_area}."""

    def __init__(self, depth, triangle_id, barycentric, dropped):
        self.depth, self.triangle_id, self.barycentric, self.dropped = depth, triangle_id, barycentric, dropped

    def interpolate(self, triangles, attr):
        """A per-vertex attribute [n_vertices, C] at every pixel -> [V,H,W,C] of attr's dtype, 0 at empty pixels: a plain torch gather, with the
        weights rounded to float32 (not the hot path, not bit-defined)."""
        if self.barycentric is None:
            raise RuntimeError("interpolate: the maps were made with want_barycentric=False")
        if attr.dim() != 2:
            raise RuntimeError(f"attr: expected shape [n_vertices, C] but found {list(attr.shape)}")
        hit = self.triangle_id >= 0
        corners = triangles.long()[self.triangle_id.clamp(min=0).long()]                     # [V,H,W,3]
        b1, b2 = self.barycentric[..., 0:1].to(attr.dtype), self.barycentric[..., 1:2].to(attr.dtype)
        out = (1 - b1 - b2) * attr[corners[..., 0]] + b1 * attr[corners[..., 1]] + b2 * attr[corners[..., 2]]
        return out * hit[..., None].to(attr.dtype)

    def __repr__(self):
        return f"MeshRaster({int(self.depth.shape[0])} views, {int(self.depth.shape[2])} x {int(self.depth.shape[1])}, {self.depth.device})"


def _raster_args(mesh, full_proj_transform, width, height, near, cull_sign, depth_tolerance=None, min_views=1):
    """Every check of the three functions below, before the library is touched -> (vertices, triangles, matrices [n,4,4], W, H)."""
    for name, x in (("width", width), ("height", height), ("min_views", min_views)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError(f"{name} must be a positive integer but found {x!r}")
    if not (float(near) > 0.0) or math.isinf(float(near)):
        raise ValueError(f"near must be a positive finite number but found {near}")
    if isinstance(cull_sign, bool) or cull_sign not in (-1, 0, 1):
        raise ValueError(f"cull_sign must be one of -1, 0, 1 but found {cull_sign!r}")
    if depth_tolerance is not None and not (float(depth_tolerance) >= 0.0):
        raise ValueError(f"depth_tolerance must be None or a non-negative number but found {depth_tolerance}")
    if width > 16384 or height > 16384:
        raise ValueError(f"width and height must stay within 16384 but found {width} x {height}")
    v, _, t = _arrays(mesh)
    m = full_proj_transform
    if not isinstance(m, torch.Tensor):
        raise RuntimeError("full_proj_transform must be a tensor")
    if not m.is_cuda:
        raise RuntimeError("full_proj_transform must be a CUDA tensor: the mesh rasterizer has no CPU path")
    if m.dtype != torch.float32 or m.dim() not in (2, 3) or tuple(m.shape[-2:]) != (4, 4):
        raise RuntimeError(f"full_proj_transform: expected a torch.float32 tensor of shape [4, 4] or [n, 4, 4] but found {m.dtype} {list(m.shape)}")
    if m.device != t.device:
        raise RuntimeError("full_proj_transform must be on the device of the mesh")
    return v, t, m.detach().reshape(-1, 4, 4).contiguous(), int(width), int(height)


def _rasterize(v, t, m, W, H, near, cull_sign, depth_tolerance, large_from, want_maps, want_barycentric, want_counts):
    """One call, the one host read-back (the status word) -> (depth, triangle_id, barycentric, counts, dropped), None for what was not asked for."""
    T, V, n, dev = int(t.shape[0]), int(v.shape[0]), int(m.shape[0]), t.device
    nbytes = int(lib().gsr_mesh_raster_scratch_bytes(T, V, n, W, H))
    if nbytes == 0:
        raise _limits(T, V, "3V and 3T must stay below 2^31")
    work = scratch(nbytes, dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_maps else None
    tid = torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_maps else None
    bary = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev) if want_maps and want_barycentric else None
    counts = torch.empty(T, dtype=torch.int32, device=dev) if want_counts else None
    dropped = torch.empty((n, 3), dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    call("gsr_mesh_rasterize", dev, v if V else None, V, t if T else None, T, m if n else None, n, W, H, float(near), int(cull_sign),
         -1.0 if depth_tolerance is None else float(depth_tolerance), int(large_from), depth, tid, bary, counts if T else None, dropped if n else None,
         work, nbytes, status)
    _raise_smooth_status(status.tolist()[0] & 0xFFFFFFFF)                 # the host read-back
    return depth, tid, bary, counts, dropped


def rasterize_mesh(mesh, full_proj_transform, width, height, near=0.01, cull_sign=0, want_barycentric=True, _large_from=LARGE_FROM):
    """The mesh as the cameras see it -> MeshRaster(depth [V,H,W], triangle_id [V,H,W], barycentric [V,H,W,2] or None, dropped [V,3]) on the
    mesh's device; the mesh is only read.  full_proj_transform: float32 [4,4] (one view) or [V,4,4], the reference's `Camera.full_proj_transform`
    (row-vector convention: clip = [x y z 1] @ M); width, height: the image size of the Gaussian renderer, whose pixel grid the maps share.
    The semantics are this project's own (include/gsrast.h, "mesh rasterization and visibility"; tests/raster_truth.py): float64
    arithmetic, coordinates snapped to 1/256 pixel, a watertight top-left rule, per pixel the nearest covering triangle and of equally near ones the
    one with the lowest index; no float atomics, two runs give the same bits.
      * a triangle with a vertex at w <= near is dropped in that view, NOT clipped -- a stated departure, conservative for culling; one whose
        snapped coordinates leave +-2^24 / 256 pixels, or whose snapped area is zero, is dropped too; dropped[v] counts the three.
      * cull_sign=+1 / -1 keeps only the triangles whose snapped signed area2 has that sign.  -1 is the OUTSIDE of this repository's marching-cubes
        meshes (extract_triangle_mesh: the TSDF is positive outside, the triangles counter-clockwise seen from there, signed volume > 0) under the
        reference's camera convention (getWorld2View2 + getProjectionMatrix: +z forward, y down in the image): found on the CPU on the sphere of
        tests/ref_mesh_numpy.py, where every triangle that owns a pixel has area2 < 0 (tests/test_raster_cpu.py).  0 rasterizes both sides.
    Raises ValueError for width / height < 1, near <= 0 or a cull_sign outside {-1, 0, 1}; RuntimeError for host tensors, wrong dtypes or shapes,
    a non-finite vertex and a triangle index outside [0, V).  Exactly ONE host read-back per call, whatever the number of views: the status word."""
    v, t, m, W, H = _raster_args(mesh, full_proj_transform, width, height, near, cull_sign)
    depth, tid, bary, _, dropped = _rasterize(v, t, m, W, H, near, cull_sign, None, _large_from, True, want_barycentric, False)
    return MeshRaster(depth, tid, bary, dropped)


def triangle_view_counts(mesh, full_proj_transform, width, height, near=0.01, cull_sign=0, depth_tolerance=None, _large_from=LARGE_FROM):
    """-> counts int32 [T] on the mesh's device: in how many of the views each triangle is SEEN.  A triangle is seen in a view iff it was neither
    dropped nor culled there (rasterize_mesh) and it owns at least one pixel of the view's triangle_id map, or -- with depth_tolerance, in the
    units of the depth -- one of its vertices lies in the image and is no farther than the depth map at its nearest pixel plus the tolerance (or
    that pixel is empty): a fused mesh has many triangles smaller than a pixel, which own no pixel centre and are plainly visible.  No maps are
    kept beyond the views in flight.  Exactly ONE host read-back per call: the status word."""
    v, t, m, W, H = _raster_args(mesh, full_proj_transform, width, height, near, cull_sign, depth_tolerance)
    return _rasterize(v, t, m, W, H, near, cull_sign, depth_tolerance, _large_from, False, False, True)[3]


def cull_unseen_triangles(mesh, full_proj_transform, width, height, min_views=1, depth_tolerance=None, near=0.01, cull_sign=0, return_counts=False):
    """-> a NEW TriangleMesh without the triangles that fewer than min_views of the views see (triangle_view_counts): the back walls, interior
    sheets and skirts of a fused TSDF that no training camera looked at and that post_process_mesh keeps because they hang on the surface.  The
    surviving triangles keep their order, vertices no survivor references go (colours move with them); the input is left untouched and the
    result has no normals.  With return_counts also the counts int32 [T] of the INPUT's triangles.  Two host read-backs: the status word and the
    record of the compaction."""
    from .tsdf import TriangleMesh
    v, t, m, W, H = _raster_args(mesh, full_proj_transform, width, height, near, cull_sign, depth_tolerance, min_views)
    counts = _rasterize(v, t, m, W, H, near, cull_sign, depth_tolerance, LARGE_FROM, False, False, True)[3]
    nv, nc, tris, _ = _filter(mesh, remove_mask=(counts < int(min_views)).view(torch.uint8), flags=DROP_UNREFERENCED)
    out = TriangleMesh(nv, nc, tris)
    return (out, counts) if return_counts else out


def as_remove_mask(mask, n, device):
    """A numpy or torch bool (or uint8) mask of n triangles as bytes on `device`."""
    if isinstance(mask, torch.Tensor):
        m = mask
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
    if m.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"mask: expected a bool mask but found {m.dtype}")
    if m.numel() != n:
        raise RuntimeError(f"mask: expected {n} entries, one per triangle, but found {m.numel()}")
    m = m.reshape(-1).to(device).contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m
