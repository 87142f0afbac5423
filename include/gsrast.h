/*
 * gsrast.h -- C ABI of libgsrast_hip.so: MI355X-native (gfx950) differentiable Gaussian-splat rasterizer.
 *
 * Drop-in boundary for the four CUDA extensions GS-SR imports.  Every entry point names the reference
 * interface it replaces (paths relative to /root/reference/submodules):
 *
 *   gsr_forward_stage1/2   <- _C.rasterize_gaussians            diff-gaussian-rasterization/rasterize_points.cu:35-115
 *                                                               diff-surfel-rasterization/rasterize_points.cu:39-135
 *                                                               diff-plane-rasterization/rasterize_points.cu:35-125
 *                             (CudaRasterizer::Rasterizer::forward, <ext>/cuda_rasterizer/rasterizer_impl.cu:198-352)
 *   gsr_backward           <- _C.rasterize_gaussians_backward   <ext>/rasterize_points.cu:117-234
 *                             (CudaRasterizer::Rasterizer::backward, <ext>/cuda_rasterizer/rasterizer_impl.cu:338-448)
 *   gsr_mark_visible       <- _C.mark_visible                   diff-gaussian-rasterization/rasterize_points.cu:198-217
 *   gsr_visible_filter     <- _C.rasterize_gaussians_filter     scaffold-filter/rasterize_points.cu:219-283
 *   gsr_dist2              <- simple_knn._C.distCUDA2           simple-knn/ext.cpp:15-17, simple_knn.cu:186-222
 *   gsr_tsdf_integrate     <- the per-frame TSDF update of gssr/utils/mesh_utils.py:195-246 (compute_sdf_perframe +
 *                             the integration step of compute_unbounded_tsdf)
 *   gsr_*_bytes            <- required<GeometryState/ImageState/BinningState>(), <ext>/cuda_rasterizer/rasterizer_impl.h:21-73
 *
 * Conventions
 *   - All array pointers are DEVICE pointers (HIP) unless marked HOST; plain C types only, no torch types.
 *   - NULL for an optional input == "not provided" (the reference passes an empty tensor -> nullptr).
 *   - The caller owns every buffer.  The three scratch arenas (geom, binning, img) must stay alive and unmodified
 *     between forward and backward of the same call (the reference saves them in the autograd ctx); their internal
 *     layout is private to the library.
 *   - Every function returns 0 on success, non-zero on error; gsr_last_error() gives a thread-local message.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  The reference launches on the legacy
 *     default stream; pass torch.cuda.current_stream().cuda_stream from PyTorch.
 *   - Matrices follow the reference's row-vector convention: p_view = [x y z 1] * viewmatrix (16 floats, row-major).
 *   - Layouts: images are CHW float32; radii/out_observe are int32; quaternions are (w,x,y,z).
 *   - Threading: every entry point may be called concurrently from several host threads and on several streams of one device.
 *     All per-call state lives in caller-owned buffers.  The library's only process-wide state is (i) one pinned mailbox per
 *     device for the num_rendered read-back, whose slots are handed out with an atomic ticket + per-slot busy flag (a forward owns
 *     its slot until it has read the word), (ii) the optional stage profiler (gsr_profile_*), a mutex-guarded event list, and
 *     (iii) read-once environment switches.  tests/test_gpu_stress.py runs forwards from two threads on two streams.
 */
#ifndef GSRAST_H
#define GSRAST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ABI_VERSION 8

enum gsr_variant {
    GSR_EWA = 0,     /* diff_gaussian_rasterization : 3DGS EWA splats, RGB only                          */
    GSR_SURFEL = 1,  /* diff_surfel_rasterization   : 2DGS surfels, 11 auxiliary channels                */
    GSR_PLANE = 2    /* diff_plane_rasterization    : PGSR planes, all_map[5], plane_depth, out_observe  */
};

/* Per-call camera/state: the GaussianRasterizationSettings NamedTuple
 * (diff_gaussian_rasterization/__init__.py:157-169; diff_plane_rasterization/__init__.py:173-186 adds render_geo). */
typedef struct gsr_cfg {
    int32_t variant;          /* enum gsr_variant */
    int32_t P;                /* number of gaussians (means3D.size(0)) */
    int32_t D;                /* sh_degree (active) */
    int32_t M;                /* SH coefficients per gaussian = sh.size(1); 0 when colors are precomputed */
    int32_t W, H;             /* image_width, image_height */
    float tanfovx, tanfovy;
    float scale_modifier;
    int32_t prefiltered;
    int32_t debug;            /* synchronise + check after every stage (CHECK_CUDA, auxiliary.h:166-173) */
    int32_t render_geo;       /* PLANE only */
    const float* bg;          /* [3]  */
    const float* viewmatrix;  /* [16] */
    const float* projmatrix;  /* [16] */
    const float* campos;      /* [3]  */
} gsr_cfg;

typedef struct gsr_inputs {
    const float* means3D;        /* [P,3] */
    const float* shs;            /* [P,M,3] or NULL */
    const float* colors_precomp; /* [P,3]  or NULL */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3] (SURFEL [P,2]) or NULL */
    const float* rotations;      /* [P,4] or NULL */
    const float* cov3D_precomp;  /* [P,6] (SURFEL: transMat_precomp [P,9]) or NULL */
    const float* all_map;        /* PLANE [P,5] or NULL */
} gsr_inputs;

typedef struct gsr_outputs {
    float* out_color;        /* [3,H,W] */
    float* out_others;       /* SURFEL [11,H,W]: 0 depth*alpha,1 alpha,2-4 normal,5 median depth,6 distortion,7 median idx,8-10 median normal */
    int32_t* out_observe;    /* PLANE [P]; must be zero-filled by the caller (torch::full(0)) */
    float* out_all_map;      /* PLANE [5,H,W] */
    float* out_plane_depth;  /* PLANE [1,H,W] */
} gsr_outputs;

typedef struct gsr_out_grads {       /* dL/d(outputs); NULL == zeros */
    const float* dL_dcolor;          /* [3,H,W]  */
    const float* dL_dothers;         /* SURFEL [11,H,W] */
    const float* dL_dout_all_map;    /* PLANE [5,H,W] */
    const float* dL_dplane_depth;    /* PLANE [1,H,W] */
    const float* all_map_pixels;     /* PLANE [5,H,W]: the forward's out_all_map (saved by the caller) */
} gsr_out_grads;

typedef struct gsr_in_grads {        /* all written in full by the library (no zero-init required) */
    float* dL_dmeans3D;     /* [P,3] */
    float* dL_dmeans2D;     /* [P,3] (z component is always 0) */
    float* dL_dmeans2D_abs; /* PLANE [P,3] or NULL */
    float* dL_dcolors;      /* [P,3] */
    float* dL_dopacity;     /* [P]   */
    float* dL_dcov3D;       /* [P,6] (SURFEL: dL_dtransMat [P,9]), or NULL = not wanted (no cov3D_precomp to hand it to): the store is skipped */
    float* dL_dsh;          /* [P,M,3] or NULL when M == 0 */
    float* dL_dscales;      /* [P,3] (SURFEL [P,2]) */
    float* dL_drotations;   /* [P,4] */
    float* dL_dall_map;     /* PLANE [P,5] or NULL */
} gsr_in_grads;

/* ---- scratch sizing (bytes).  binning is sized for a capacity of R tile-instances. */
size_t gsr_geom_bytes(int32_t variant, int32_t P);
size_t gsr_img_bytes(int32_t variant, int32_t W, int32_t H);
size_t gsr_binning_bytes(int32_t variant, uint32_t R, int32_t W, int32_t H);
/* scratch needed by gsr_backward (gradient accumulators, zeroed by the library) */
size_t gsr_backward_scratch_bytes(int32_t variant, int32_t P);

/* ---- forward.  stage1 = preprocess + depth ordering + prefix sum; it writes radii and returns the number of
 * tile instances R in *num_rendered_host (HOST pointer) after synchronising `stream` once -- the same single
 * host<->device sync the reference performs (rasterizer_impl.cu:281).  The caller then sizes `binning` for R and
 * calls stage2 = duplicate-with-keys + stable tile sort + tile ranges + per-tile alpha blend. */
int gsr_forward_stage1(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                       int32_t* radii /*[P]*/, uint32_t* num_rendered_host, void* stream);
int gsr_forward_stage2(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                       void* binning, size_t binning_bytes, void* img, size_t img_bytes,
                       uint32_t num_rendered, const gsr_outputs* out, void* stream);
/* ABI 7.  The same pair with the forward's depth order made explicit: stage 1 decides it (and records it in the geom arena), *depth_order_host receives an
 * opaque non-zero word that the caller hands back to stage 2 -- which is then a pure enqueue.  gsr_forward_stage2 (= depth_order 0) reads the record back from
 * the arena instead: one more host<->device round trip per forward (it also serves the redo after an overflowed gsr_forward). */
int gsr_forward_stage1_ex(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                          int32_t* radii /*[P]*/, uint32_t* num_rendered_host, uint32_t* depth_order_host, void* stream);
int gsr_forward_stage2_ex(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                          void* binning, size_t binning_bytes, void* img, size_t img_bytes,
                          uint32_t num_rendered, uint32_t depth_order, const gsr_outputs* out, void* stream);

/* ---- single-call forward without the GPU idle gap at the sync.  `binning` is an arena of ANY capacity
 * (gsr_binning_capacity(bytes) instances, e.g. sized from the previous iteration's num_rendered with head-room):
 * stage 2 is enqueued right behind stage 1 and reads the exact instance count on the device; the host waits only on an
 * event recorded after stage 1 and returns num_rendered.  *overflow_host = 1 iff num_rendered > capacity: outputs are
 * then incomplete and the caller re-runs gsr_forward_stage2 with a large-enough arena (geom stays valid; PLANE callers
 * re-zero out_observe first).  Results are identical to stage1 + stage2. */
uint32_t gsr_binning_capacity(int32_t variant, size_t binning_bytes, int32_t W, int32_t H);
int gsr_forward(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                void* binning, size_t binning_bytes, void* img, size_t img_bytes, int32_t* radii /*[P]*/,
                const gsr_outputs* out, uint32_t* num_rendered_host, int32_t* overflow_host, void* stream);

/* ---- backward of the same call.  radii is the forward's radii output. */
int gsr_backward(const gsr_cfg* cfg, const gsr_inputs* in, const int32_t* radii,
                 const void* geom, size_t geom_bytes, const void* binning, size_t binning_bytes,
                 const void* img, size_t img_bytes, uint32_t num_rendered,
                 void* scratch, size_t scratch_bytes,
                 const gsr_out_grads* og, const gsr_in_grads* ig, void* stream);

/* gsr_backward with flags (round 3).  The gradient accumulators in `scratch` are what the blend backward adds into and the preprocess backward
 * reads exactly once:
 *   GSR_BWD_SCRATCH_IS_ZERO  the caller guarantees scratch holds only zeros (e.g. left so by the previous call): the 24 MB memset
 *                            (+ its launch gap) in front of the blend backward is skipped;
 *   GSR_BWD_LEAVE_ZERO       the preprocess backward writes zeros back over every accumulator row after reading it, so the SAME scratch can be
 *                            passed with GSR_BWD_SCRATCH_IS_ZERO next time (a training loop keeps one scratch per model: ~11 us per iteration).
 * flags = 0 is gsr_backward. */
enum { GSR_BWD_SCRATCH_IS_ZERO = 1, GSR_BWD_LEAVE_ZERO = 2 };
int gsr_backward_ex(const gsr_cfg* cfg, const gsr_inputs* in, const int32_t* radii,
                    const void* geom, size_t geom_bytes, const void* binning, size_t binning_bytes,
                    const void* img, size_t img_bytes, uint32_t num_rendered,
                    void* scratch, size_t scratch_bytes,
                    const gsr_out_grads* og, const gsr_in_grads* ig, uint32_t flags, void* stream);

/* ---- forward with NO host synchronisation at all (round 3): the form that can be recorded into a HIP graph (hipStreamBeginCapture /
 * torch.cuda.graph) and replayed.  Like gsr_forward it runs against a binning arena of fixed capacity and the kernels read the instance
 * count on the device; unlike gsr_forward the host never learns it: status_dev[0] <- num_rendered, status_dev[1] <- 1 if it exceeded the
 * capacity (outputs then incomplete; status_dev[1] is sticky: the library only ever sets it, the caller clears it), status_dev[2] <- 1 (sticky)
 * if cfg->prefiltered is set and a gaussian failed the frustum test (the reference traps the device, auxiliary.h:156-160; the synchronous forwards
 * fail the call) -- three DEVICE words the caller reads whenever it synchronises anyway.  gsr_backward[_ex] of such a call takes num_rendered =
 * the capacity. */
int gsr_forward_async(const gsr_cfg* cfg, const gsr_inputs* in, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* img, size_t img_bytes, int32_t* radii /*[P]*/,
                      const gsr_outputs* out, uint32_t* status_dev /*[3]*/, void* stream);

/* ---- helpers of the same extensions */
int gsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present /*[P] bool*/, void* stream);
int gsr_visible_filter(const gsr_cfg* cfg, const float* means3D, const float* scales /*[P,3]*/,
                       const float* rotations, const float* cov3D_precomp, int32_t* radii /*[P]*/, void* stream);

/* ---- adjacent kernels */
int gsr_tsdf_integrate(int64_t V, const float* points /*[V,3]*/, const float* full_proj /*[16]*/,
                       int32_t W, int32_t H, const float* depth /*[H,W]*/, const float* rgb /*[3,H,W]*/,
                       float sdf_trunc, const float* sdf_trunc_per_point /*[V] or NULL*/,
                       float* tsdf /*[V]*/, float* weight /*[V]*/, float* rgb_acc /*[V,3]*/,
                       void* rgbd_scratch /*[H*W*16 bytes], 16-B aligned, or NULL (slower dword gathers)*/, void* stream);
/* Dense-grid, Open3D-style integration (the bounded path of gssr/utils/mesh_utils.py:138-179 calls
 * o3d.pipelines.integration.ScalableTSDFVolume.integrate, Open3D 0.18.0 -- NOT vendored in the reference, so the voxel
 * update is restated from Open3D's published UniformTSDFVolume algorithm and its parity is UNPINNED):
 * voxel centre p = origin + voxel_length*(idx+0.5); p_cam = extrinsic*p (row-major 4x4 world->camera); skip z<=0;
 * (u,v) = (int)(fx*x/z + cx + 0.5, fy*y/z + cy + 0.5) nearest pixel; d = depth[v,u], skip d<=0 or d>depth_trunc;
 * sdf = (d - z) * sqrt(((u-cx)/fx)^2 + ((v-cy)/fy)^2 + 1); if sdf > -sdf_trunc: t = min(1, sdf/sdf_trunc);
 * tsdf = (tsdf*w + t)/(w+1); color = (color*w + rgb[:,v,u])/(w+1); w += 1.  Arrays are [nx,ny,nz] x-major, initial 0. */
int gsr_tsdf_integrate_dense(int32_t nx, int32_t ny, int32_t nz, const float* origin /*[3] HOST*/, float voxel_length,
                             float sdf_trunc, float depth_trunc, int32_t W, int32_t H, const float* depth /*[H,W]*/,
                             const float* rgb /*[3,H,W]*/, float fx, float fy, float cx, float cy,
                             const float* extrinsic /*[16] HOST, row-major world->camera*/,
                             float* tsdf, float* weight, float* color /*[nx,ny,nz,3]*/, void* stream);
/* Block-sparse TSDF volume = the role of o3d.pipelines.integration.ScalableTSDFVolume in the reference's mesh extraction
 * (gssr/utils/mesh_utils.py:154-178, extract_mesh.py:125-128: voxel_length = depth_trunc / 1024, sdf_trunc = 5 * voxel_length;
 * extract_mesh_split.py:91-119 fuses the frames of every tile into one such volume).  Open3D 0.18 is NOT part of /root/reference:
 * the algorithm is restated from its published sources (ScalableTSDFVolume::Integrate, UniformTSDFVolume::
 * IntegrateWithDepthToCameraDistanceMultiplier) and its PARITY IS UNPINNED.  Units of 16^3 voxels in a hash map keyed by the unit
 * coordinate floor(p / (16 * voxel_length)); a frame opens every unit overlapping [p - sdf_trunc, p + sdf_trunc] for every
 * `stride`-th valid depth pixel's world point p and applies the gsr_tsdf_integrate_dense voxel rule to each opened unit once.
 * All buffers are caller-owned device memory: keys [2^cap_hash_log2] int64 filled with -1, slot [2^cap_hash_log2] int32,
 * coord [cap_blocks,3] int32, stamp/list [cap_blocks], counters [4] int32 zero-filled; counters[0] = units allocated so far.
 * ABI 8, the voxel storage:
 * (1) unit RECORDS of 5 x 4096 float32 (planes tsdf, weight, r, g, b: every plane is read and written in coalesced 16-byte groups) in up to
 *     GSR_TSDF_MAX_CHUNKS chunks of doubling size: chunk[0] holds units [0, 2^chunk0_log2), chunk[c >= 1] the units [2^(chunk0_log2+c-1), 2^(chunk0_log2+c));
 *     cap_blocks = 2^(chunk0_log2 + n_chunks - 1).  Growing a volume = one more chunk + larger small arrays + gsr_tsdf_sparse_rehash: no voxel is copied.
 * (2) NOTHING is initialised: a unit whose stamp is 0 has never been written, and mask [cap_blocks,16] uint64 (uninitialised as well) says per unit which of its
 *     1024 16-byte groups (four consecutive z) have ever been written.  A clear bit means (tsdf 0, weight 0, colour 0) whatever the record holds there: the
 *     kernels never read such a group and a unit's first frame writes only the 128-byte lines it observed.  A reader of the raw records calls
 *     gsr_tsdf_sparse_materialize first.  (ABI <= 6 zero-filled 80 KB per unit of capacity, ABI 7 wrote a unit's first frame in full.)
 * (3) A plane is stored in bricks, not x-major: voxel (x,y,z) of a unit lives at float index 4*g + (z & 3) of its plane with
 *       g = (x>>2)<<8 | (y>>2)<<6 | (z>>2)<<4 | ((x>>1)&1)<<3 | ((y>>1)&1)<<2 | (x&1)<<1 | (y&1)
 *     (4x4x4 bricks of 256 B, 128-byte lines of 2x4x4 voxels, 64-byte sectors of 2x2x4: the surface shell a frame updates cuts compact lines less often than
 *     the 1x1x16 columns of an x-major plane). */
#define GSR_TSDF_MAX_CHUNKS 24
typedef struct gsr_tsdf_sparse {
    void* keys; int32_t* slot; int32_t* coord; uint32_t* stamp; int32_t* list; int32_t* counters;
    void* mask;
    float* chunk[GSR_TSDF_MAX_CHUNKS];
    uint32_t chunk0_log2, n_chunks;
    uint32_t cap_hash_log2, cap_blocks;
    float voxel_length, sdf_trunc;
} gsr_tsdf_sparse;
/* One frame (ABI 7; the round-2 entry point gsr_tsdf_sparse_integrate with its host read in front of the voxel pass is gone since ABI 8).
 * extrinsic = world->camera, pose = camera->world (both [12] HOST, row-major 3x4); `frame` must be a fresh non-zero number per call.
 * rgb [3,H,W] as rendered; quant 0 = store as given, 1 = clamp to [0,1] and scale to
 * 0..255, 2 = additionally truncate to an integer (the uint8 conversion of mesh_utils.py:170) -- done on the device while the planes are interleaved into
 * `texels` [H*W*4] floats (caller-owned scratch; quant 2 uses half of it: 8-byte texels (depth, rgb bytes)); the voxel pass reads the length of its work
 * list on the device, so nothing waits for the host in front of it.
 * status_host [4] (may be NULL without GSR_TSDF_NO_SYNC) receives {units allocated, units integrated by this frame, capacity exhausted, sample out of range}.
 * Default: synchronises once at the end and reports the two error conditions (in either case NOTHING of the frame has been
 * integrated: grow the volume and run it again with a new frame number).  GSR_TSDF_NO_SYNC: returns after enqueuing; status_host must be pinned and stay
 * alive; the caller waits for an event of its own and passes the words to gsr_tsdf_sparse_status. */
#define GSR_TSDF_NO_SYNC 1u
int gsr_tsdf_sparse_integrate2(const gsr_tsdf_sparse* vol, int32_t W, int32_t H, const float* depth /*[H,W]*/, const float* rgb /*[3,H,W]*/, int32_t quant,
                               float fx, float fy, float cx, float cy, const float* extrinsic, const float* pose, float depth_trunc, int32_t stride,
                               uint32_t frame, float* texels, int32_t* status_host, uint32_t flags, void* stream);
int gsr_tsdf_sparse_status(const gsr_tsdf_sparse* vol, const int32_t* status_host, void* stream);
/* After the caller re-allocated a volume's arrays (growth: a further chunk, larger coord / stamp / list / mask with units [0, n_units) copied, keys all -1), counters[0] = n_units --
 * gives every unit its key back with the slot it had.  No voxel is touched. */
int gsr_tsdf_sparse_rehash(const gsr_tsdf_sparse* vol, int32_t n_units, void* stream);
/* vol <- weighted merge with n_units units given as plain arrays in LOGICAL voxel order (coords [n,3] int32, tsdf/weight [n,16,16,16] x-major,
 * color [n,16,16,16,3]; weight 0 = no data): the fusion step of extract_mesh_split.py when every GPU integrated its own tile's frames (running averages are
 * associative in (sum w*tsdf, sum w)); the lists other ranks send.  A coordinate outside [-2^20 + 1, 2^20 - 2] has no key of its own: the call is refused
 * ("outside the addressable volume", like a frame with such a sample) before any voxel is merged. */
int gsr_tsdf_sparse_merge(const gsr_tsdf_sparse* vol, int32_t n_units, const int32_t* coords, const float* tsdf, const float* weight,
                          const float* color, void* stream);
/* ABI 8.  vol <- weighted merge with units [0, n_units) of another volume on the same device, read where they lie (storage order, written-group words):
 * the per-tile volumes of one GPU.  Synchronises once (capacity check). */
int gsr_tsdf_sparse_merge_volume(const gsr_tsdf_sparse* vol, const gsr_tsdf_sparse* other, int32_t n_units, void* stream);
/* ABI 8.  Zero-fills the never-written groups of units [0, n_units) and marks them written: afterwards the pools are plain arrays (still in brick order). */
int gsr_tsdf_sparse_materialize(const gsr_tsdf_sparse* vol, int32_t n_units, void* stream);
/* The triangle mesh of the volume (the role of `volume.extract_triangle_mesh()`, gssr/utils/mesh_utils.py:178; extends ABI 8), read from the pools where
 * they lie: the volume is not materialised and not written.  The mesh, defined:
 *  - a voxel COUNTS iff its weight > min_weight (0: Open3D's `w != 0`); a clear written-group bit, a unit with stamp 0 and a unit that is not in the table
 *    read as weight 0.  Voxel (x,y,z) of the unit at `coord` has the global index G = 16*coord + (x,y,z) and the centre voxel_length*(G + 0.5).
 *  - the cube with origin G has corner i at G + (i&1, (i>>1)&1, (i>>2)&1); it is VALID iff its 8 corners count; its case has bit i set iff tsdf_i < 0
 *    (a tsdf of exactly 0 is outside); the triangles of a case are those of csrc/gsr_mc_table.h (tools/gen_mc_table.py), cases 0 and 255 have none.
 *  - the edge from G to G + e_a carries one vertex iff the signs of its ends differ and at least one of its four cubes is valid: no vertex is unreferenced,
 *    none appears twice (also across units).  With f0 the tsdf at G, t = f0 / (f0 - f1): the position's component a is voxel_length*((float)G_a + 0.5f + t),
 *    the other two voxel_length*((float)G + 0.5f) (float32, no FMA contraction); the colour (c0 + t*(c1 - c0)) / 255.  Triangles that are degenerate
 *    because t is 0 or 1 are kept.
 *  - order: units as `order` lists them (a permutation of [0, n_units): for a mesh that does not depend on the pool layout, ascending (coord.x, coord.y,
 *    coord.z)); inside a unit voxels x-major with z fastest; inside a voxel vertices by axis 0, 1, 2 and triangles in table order.  The mesh is a pure
 *    function of the volume's content and `order`.
 * gsr_tsdf_sparse_mesh_count writes the per-unit state of the mesh into `scratch` (gsr_tsdf_sparse_mesh_scratch_bytes(n_units) bytes of device memory,
 * 16-byte aligned, about 2 KB per unit) and returns the number of vertices and of triangles in counts_host[0 / 1] (HOST; it synchronises once); more
 * than 2^31 - 1 of either is refused.  gsr_tsdf_sparse_mesh_emit, called with the same arguments and the scratch as count left it, writes
 * vertices [V,3] float32, colors [V,3] float32 in [0,1] and triangles [T,3] int32 (device). */
size_t gsr_tsdf_sparse_mesh_scratch_bytes(int32_t n_units);
int gsr_tsdf_sparse_mesh_count(const gsr_tsdf_sparse* vol, int32_t n_units, const int32_t* order /*[n_units] device*/, float min_weight, void* scratch,
                               size_t scratch_bytes, uint64_t* counts_host /*[2]*/, void* stream);
int gsr_tsdf_sparse_mesh_emit(const gsr_tsdf_sparse* vol, int32_t n_units, const int32_t* order, float min_weight, void* scratch, size_t scratch_bytes,
                              float* vertices, float* colors, int32_t* triangles, void* stream);
/* Fused image-side loss right behind the rasterizer (the L1 term of gssr/scene/vanilla_scene.py:63-69
 * plus a linear functional of the auxiliary maps): loss = mean|color - gt| + sum(aux * waux); one streaming pass
 * writes dL/dcolor = sign(color-gt)/n and accumulates the scalar into *loss_out (device, caller zero-fills).
 * dL/daux is waux itself, so nothing is written for it. */
int gsr_loss_l1_linear(int64_t n_color, const float* color, const float* gt, float* dL_dcolor,
                       int64_t n_aux, const float* aux, const float* waux, float* loss_out, void* stream);
/* Fused Adam step over one parameter tensor -- the optimizer every Gaussian model of the reference steps once per iteration
 * (`torch.optim.Adam(l, lr=0.0, eps=1e-15)`, gssr/gaussian/vanilla_gaussian.py:120-139; gssr/engine/trainer.py:127), with the arithmetic of torch's
 * single-tensor implementation (no amsgrad, no weight decay):
 *   exp_avg += (grad - exp_avg)(1 - beta1);  exp_avg_sq = exp_avg_sq beta2 + grad^2 (1 - beta2);
 *   param  -= step_size * exp_avg / (sqrt(exp_avg_sq) / bias_correction2_sqrt + eps)
 * step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t), both formed by the caller in double; the betas are doubles
 * because the weights 1 - beta are rounded to float after the subtraction, as torch does.  lr_scale (or NULL): one
 * multiplier of step_size per element.  All pointers device float32 of n elements; one streaming pass, no host synchronisation. */
int gsr_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float step_size, double beta1, double beta2,
                  float bias_correction2_sqrt, float eps, const float* lr_scale, void* stream);
/* The same update for `count` parameter tensors in one launch per 24 tensors (a model has 6-20 parameter tensors, most of them tiny).
 * `t` is a HOST array; every entry carries its own hyper-parameters (the reference gives every tensor its own param group / learning rate). */
typedef struct gsr_adam_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    const float* lr_scale;            /* optional per-element multiplier of step_size, or NULL */
    int64_t n;
    double beta1, beta2;
    float step_size;                  /* lr / (1 - beta1^t) */
    float bias_correction2_sqrt;      /* sqrt(1 - beta2^t) */
    float eps, pad_;
    const float* grad2;               /* optional second gradient of the same tensor, or NULL: the update uses grad + grad2 (one fp32 add per element,
                                       * what autograd's accumulation would have produced).  For parameters that feed two render passes through two
                                       * sets of leaves over the same storage (gsrast.optim.shadow_parameters): no add kernel per tensor, no summed copy. */
} gsr_adam_tensor;
int gsr_adam_step_multi(int32_t count, const gsr_adam_tensor* t, void* stream);
/* The same with the two per-step scalars of every tensor read from DEVICE memory at run time -- hyper_dev[2 * i] = step_size,
 * hyper_dev[2 * i + 1] = bias_correction2_sqrt of entry i (the fields of t[i] are ignored) -- so that the launch can sit in a HIP graph: the caller
 * refreshes the small buffer (learning-rate schedule, bias correction of the current step) before every replay. */
int gsr_adam_step_multi_dev(int32_t count, const gsr_adam_tensor* t, const float* hyper_dev /*[count,2]*/, void* stream);
/* Octree-GS level-of-detail mask fused with the prefilter (OctreeGaussianModel.set_anchor_mask / map_to_int_level,
 * gssr/gaussian/octree_gaussian.py:184-203,255-267; OctreeScene.prefilter_voxel, gssr/scene/octree_scene.py:136-172):
 *   dist = |anchor + (voxel_size/2)/fork^level - campos| * resolution_scale;  pred = log2(standard_dist/dist)/log2(fork) + extra_level
 *   int_level = clamp(floor|round|ceil(pred), 0, coarse_index-1)   ('progressive': floor(clamp(pred+1, .9999, coarse_index-1+.9999)),
 *                                                                  prog_ratio = frac(.), transition_mask = (level == int_level))
 *   anchor_mask = level <= int_level;  radii = anchor_mask ? visible_filter radius : 0     (visible_mask == radii > 0)
 * cfg: camera/settings as for gsr_visible_filter with P = number of anchors.  scales: first three of every `scale_stride` floats
 * (6 for get_scaling).  prog_ratio / transition_mask may be NULL.  No host synchronisation. */
typedef struct gsr_lod_cfg {
    float voxel_size, fork, standard_dist, resolution_scale;
    int32_t coarse_index;     /* levels in use (the reference passes coarse_index - 1 as cur_level) */
    int32_t mode;             /* dist2level: 0 floor, 1 round, 2 ceil, 3 progressive */
} gsr_lod_cfg;
int gsr_octree_visible(const gsr_cfg* cfg, const gsr_lod_cfg* lod, const float* anchor /*[Na,3]*/, const int32_t* level /*[Na]*/,
                       const float* extra_level /*[Na] or NULL*/, const float* scales, int32_t scale_stride, const float* rotations /*[Na,4]*/,
                       uint8_t* anchor_mask /*[Na]*/, int32_t* radii /*[Na]*/, float* prog_ratio /*[Na] or NULL*/,
                       uint8_t* transition_mask /*[Na] or NULL*/, void* stream);
/* Fused photometric loss (gssr/scene/vanilla_scene.py:29-69, used by every method's get_loss_dict):
 *   loss = (1-lambda)*mean|img-gt| + lambda*(1 - SSIM(img,gt)), SSIM with the 11x11 sigma-1.5 window, zero padding, C1=0.01^2, C2=0.03^2.
 * loss_out (device, 3 floats, overwritten): {mean|img-gt|, mean SSIM, loss}.  dL_dimg [C,H,W] = d loss / d img.
 * scratch >= gsr_loss_l1_ssim_scratch_bytes (three derivative maps). */
size_t gsr_loss_l1_ssim_scratch_bytes(int32_t C, int32_t H, int32_t W);
int gsr_loss_l1_ssim(int32_t C, int32_t H, int32_t W, const float* img /*[C,H,W]*/, const float* gt, float lambda_dssim,
                     float* loss_out /*[3]*/, float* dL_dimg, void* scratch, size_t scratch_bytes, void* stream);
/* 2DGS geometric regularisers fused with the render() post-processing (gssr/scene/twodgs_scene.py:25-35,88-115;
 * gssr/utils/point_utils.py:9-37 depths_to_points / depth_to_normal):
 *   depth = nan_to_num(allmap[0]/allmap[1])*(1-depth_ratio) + depth_ratio*nan_to_num(allmap[5]);  P = depth * ([x y 1] * ray_mat)
 *   surf_normal = normalize(cross(P(y+1,x)-P(y-1,x), P(y,x+1)-P(y,x-1))) * allmap[1] (alpha detached), 0 on the image border
 *   normal = allmap[2:5] * normal_rot;  loss = lambda_normal*mean(1 - <normal, surf_normal>) + lambda_dist*mean(allmap[6])
 * ray_mat, normal_rot: DEVICE [9] row-major, row-vector convention (gsrast.losses.camera_ray_matrices builds them as the reference does).
 * loss_out (device [3]): {mean normal error, mean distortion, loss}; dL_dallmap [11,H,W] overwritten (0 where the reference's autograd
 * yields NaN: channels 0/1 at pixels with allmap[1] == 0).  out_* may be NULL ('depth' [H,W], 'normal' [3,H,W], 'surf_normal' [3,H,W]). */
size_t gsr_loss_surfel_geo_scratch_bytes(int32_t H, int32_t W);
int gsr_loss_surfel_geo(int32_t H, int32_t W, const float* allmap, const float* ray_mat, const float* normal_rot, float depth_ratio,
                        float lambda_normal, float lambda_dist, float* loss_out, float* dL_dallmap, float* out_surf_depth,
                        float* out_normal_world, float* out_surf_normal, void* scratch, size_t scratch_bytes, void* stream);
/* PGSR single-view normal regulariser (gssr/scene/pgsr_scene.py:105-112,320; normal_from_depth_image, gssr/utils/graphics_utils.py:80-146):
 *   P = plane_depth * ([x y 1] * ray_mat), ray_mat = inverse(K^T) (DEVICE [9]);  depth_normal = normalize(cross(P(y,x+1)-P(y,x-1),
 *   P(y-1,x)-P(y+1,x))) * alpha (alpha detached), 0 on the border;  loss = lambda * mean(weight * sum_c |depth_normal_c - normal_c|).
 * weight [H,W] or NULL (= 1): the detached image-gradient weight.  loss_out (device [3]) = {mean weighted L1, 0, loss};
 * dL_ddepth [H,W], dL_dnormal [3,H,W] overwritten; out_depth_normal [3,H,W] or NULL.  scratch as for gsr_loss_surfel_geo. */
int gsr_loss_plane_geo(int32_t H, int32_t W, const float* plane_depth, const float* alpha, const float* normal, const float* weight,
                       const float* ray_mat, float lambda_normal, float* loss_out, float* dL_ddepth, float* dL_dnormal,
                       float* out_depth_normal, void* scratch, size_t scratch_bytes, void* stream);
/* Scaling regulariser of the scaffold / octree scenes (gssr/scene/scaffold_scene.py:184, scaffold_2dgs_scene.py:25, scaffold_pgsr_scene.py:20,
 * octree_2dgs_scene.py:25, octree_pgsr_scene.py:23): loss = lambda_scaling * mean_i prod_{c < cols} scaling[i*stride + c], value and gradient in one
 * pass.  cols 1..3, stride >= cols floats per row (the first `cols` columns of a wider tensor without a copy; the other columns get gradient 0).
 * With count_dev (device int32; static-shape iterations) only the first *count_dev rows are live: the mean divides by that count and the rows behind
 * it contribute nothing and get zero gradient; NULL: all P rows.
 * loss_out (device float) must be ZERO on entry (one atomic per block adds into it); dL_dscaling [P, stride] is overwritten. */
int gsr_loss_scaling_prod(int64_t P, int32_t cols, int32_t stride, const float* scaling, const int32_t* count_dev, float lambda_scaling,
                          float* loss_out, float* dL_dscaling, void* stream);

/* Per-iteration densification statistics of the explicit-Gaussian methods (gssr/gaussian/vanilla_gaussian.py:467-472 densify + :428-430
 * add_densification_stats; gssr/gaussian/pgsr_gaussian.py:164-172 + :157-161).  For every p with visibility_filter[p] != 0:
 *   max_radii2D[p] = max(max_radii2D[p], radii[p])          (PGSR: only where out_observe[p] > 0; pass NULL for 3DGS / 2DGS)
 *   xyz_gradient_accum[p] += |viewspace_grad[p,0:2]|; denom[p] += 1;  and the same for the *_abs pair when viewspace_grad_abs != NULL (PGSR).
 * All accumulators float [P], updated in place; viewspace_grad [P, grad_stride].  One launch, no host synchronisation. */
int gsr_densify_stats(int32_t P, const uint8_t* visibility_filter, const int32_t* radii, const int32_t* out_observe, const float* viewspace_grad,
                      int32_t grad_stride, const float* viewspace_grad_abs, float* max_radii2D, float* xyz_gradient_accum, float* denom,
                      float* xyz_gradient_accum_abs, float* denom_abs, void* stream);

/* ---- activations of the explicit-Gaussian models (round 4): replaces the three torch ops + ~8 autograd kernels of
 * /root/reference/gssr/gaussian/vanilla_gaussian.py:86-90,250-269 (get_scaling = exp, get_rotation = F.normalize(dim=1, eps=1e-12),
 * get_opacity = sigmoid) in front of every rasterizer call of vanilla-3dgs / 2dgs / pgsr.  scaling (P, scale_dim <= 3), rotation (P, 4), opacity (P, 1);
 * backward: upstream gradients may be NULL (that output was unused). */
int gsr_gauss_activations(int32_t P, int32_t scale_dim, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                          float* scaling, float* rotation, float* opacity, void* stream);
int gsr_gauss_activations_backward(int32_t P, int32_t scale_dim, const float* scaling, const float* rotation_raw, const float* rotation,
                                   const float* opacity, const float* dL_dscaling, const float* dL_drotation, const float* dL_dopacity,
                                   float* dL_dscaling_raw, float* dL_drotation_raw, float* dL_dopacity_raw, void* stream);

/* Per-Gaussian `all_map` input of the plane rasterizer, as PGSRScene.render() builds it (gssr/scene/pgsr_scene.py:241-257
 * get_rotation_matrix / get_smallest_axis / get_normal and :297-304):  all_map[i] = {local_normal (3), 1, local_distance} with
 *   n = quaternion_to_matrix(rotations[i])[:, argmin(scales[i])] (pytorch3d convention: real part first, normalised by 2/(q.q); first
 *   minimum on ties), flipped where n . (campos - means3D[i]) < 0;  local_normal = n Wv[:3,:3];
 *   local_distance = |local_normal . (means3D[i] Wv[:3,:3] + Wv[3,:3])|.
 * viewmatrix [16] / campos [3]: DEVICE pointers, the reference's world_view_transform / camera_center (as in gsr_cfg).
 * scales [P, scale_stride] (scale_stride >= 3: get_scaling may be wider).  rotations / dL_drotations 16-byte aligned.
 * Backward: dL_dall_map [P,5] (the rasterizer's gsr_in_grads.dL_dall_map) -> dL_dmeans3D [P,3] (through the camera-space centre only),
 * dL_drotations [P,4] (through R, including the 2/(q.q) term); both overwritten.  scales get no gradient (argmin). */
int gsr_plane_allmap(int32_t P, const float* means3D, const float* rotations, const float* scales, int32_t scale_stride,
                     const float* viewmatrix, const float* campos, float* all_map, void* stream);
int gsr_plane_allmap_backward(int32_t P, const float* means3D, const float* rotations, const float* scales, int32_t scale_stride,
                              const float* viewmatrix, const float* campos, const float* dL_dall_map, float* dL_dmeans3D,
                              float* dL_drotations, void* stream);

/* Uniform sample WITHOUT replacement of at most `num` set bytes of mask [n] (pgsr_scene.py:147-151: the reference draws it with
 * np.random.choice on the host).  Keys = 24-bit hash of (seed, index); the `num` smallest are taken (two histogram levels find the exact
 * threshold; no sort).  idx_out [min(num, n)] (DEVICE): the selected indices ascending, then the threshold ties that fill up, then -1.
 * All set entries are returned when there are at most `num` of them.  Deterministic in (mask, num, seed). */
size_t gsr_sample_mask_scratch_bytes(int64_t n);
int gsr_sample_mask(int64_t n, const uint8_t* mask, int32_t num, uint64_t seed, int32_t* idx_out, void* scratch, size_t scratch_bytes, void* stream);

/* PGSR multi-view regularisers (gssr/scene/pgsr_scene.py:113-204 -- the "multi-view loss" branch of get_loss_dict; lncc :60-95;
 * get_points_from_depth / get_points_depth_in_depth_map gssr/utils/point_utils.py:38-75; patch_offsets / patch_warp
 * gssr/utils/graphics_utils.py:185-198; get_rays / get_k / get_inv_k gssr/cameras/__init__.py:96-121).
 * Cameras are row-vector (X_cam = X_world R + T, world_view_transform[:3,:3] = R, [3,:3] = T); the two rigid maps are handed in composed:
 *   v2n = {A row-major [9], b [3]} with X_near = X_view A + b  (A = Rv^T Rn, b = Tn - Tv A);  n2v = its inverse.
 * (fx,fy,cx,cy) / (nfx,..) are Camera.Fx.. of the view / the neighbour; (W,H) the view's maps, (Wn,Hn) the neighbour's plane depth,
 * (Wg,Hg) both gray images (the reference assumes they agree); patch = config.patch_size (half width), noise_th = pixel_noise_threshold. */
typedef struct gsr_mv_cfg {
    int32_t W, H, Wn, Hn, Wg, Hg;
    float fx, fy, cx, cy, nfx, nfy, ncx, ncy;
    float v2n[12], n2v[12];
    float ncc_scale, noise_th;
    int32_t patch;
} gsr_mv_cfg;
/* scratch for either call below (block partials) */
size_t gsr_loss_plane_mv_scratch_bytes(int32_t W, int32_t H, int32_t n_samples);
/* Geometric consistency (pgsr_scene.py:117-143): per pixel, reproject through plane_depth into the neighbour, sample its plane depth
 * (bilinear, border clamp), reproject back; pixel_noise = reprojection error, d_mask = in-frustum & noise < noise_th,
 * weight = exp(-noise) (detached; 0 outside d_mask).  Outputs (all DEVICE): noise/d_mask/weight [H*W]; stats[3] = {sum_{d_mask} weight*noise,
 * |d_mask|, their ratio (0 if empty)};  g_depth [H*W], g_near [Hn*Wn] (overwritten) = d stats[0] / d plane_depth, d near_plane_depth.
 * geo_loss = lambda_geo * stats[2]; its gradients are lambda_geo / stats[1] times the g_* maps (the caller scales: no host sync). */
int gsr_loss_plane_mv_geo(const gsr_mv_cfg* cfg, const float* plane_depth, const float* near_plane_depth, float* noise, uint8_t* d_mask,
                          float* weight, float* stats, float* g_depth, float* g_near, void* scratch, size_t scratch_bytes, void* stream);
/* Patch NCC (pgsr_scene.py:145-199): idx [n_samples] = sampled pixel indices y*W+x, each at most once, -1 = unused slot.
 * Per sample: plane-induced homography from normal [3,H,W] / distance [H,W], (2*patch+1)^2 bilinear taps (zeros padding) in both gray
 * images, lncc; ncc [n] / mask [n] may be NULL.  stats[3] = {sum_{mask} ncc*weight, |mask|, ratio};  g_normal [3,H,W], g_distance [H,W]
 * (overwritten, zero where unsampled) = d stats[0] / d normal, d distance.  ncc_loss = lambda_ncc * stats[2]. */
int gsr_loss_plane_mv_ncc(const gsr_mv_cfg* cfg, int32_t n_samples, const int32_t* idx, const float* weight, const float* normal,
                          const float* distance, const float* gray, const float* near_gray, float* ncc, uint8_t* mask, float* stats,
                          float* g_normal, float* g_distance, void* scratch, size_t scratch_bytes, void* stream);
/* The two loss values and the scaled gradient maps from the six stats words of the two calls above (stats[0..2] geo, stats[3..5] ncc), on the device:
 * out2 = {lambda_geo * stats[2], lambda_ncc * stats[5]};  o_depth / o_near = g_depth / g_near * up_geo * lambda_geo / max(stats[1], 1),
 * o_am = g_am * up_ncc * lambda_ncc / max(stats[4], 1) (g_am: the n_am floats of the normal / distance gradient maps, contiguous); up_geo / up_ncc:
 * DEVICE scalars (upstream gradients of the two loss values), NULL = 1.  have_add != 0: o_depth += add_depth * up_add, o_am += add_am * up_add (maps
 * of another loss over the same pixels -- gsr_loss_plane_geo's -- and its upstream scalar, NULL = 1; either map may be NULL; g_depth / g_am may then
 * be NULL as well = that loss sent no gradient).  Replaces the framework's scalar-op chain of pgsr_scene.py:141-143,197-199. */
int gsr_loss_plane_mv_values(const float* stats, float lambda_geo, float lambda_ncc, float* out2, void* stream);
int gsr_loss_plane_mv_scale(size_t n_depth, size_t n_near, size_t n_am, const float* g_depth, const float* g_near, const float* g_am,
                            const float* stats, float lambda_geo, float lambda_ncc, const float* up_geo, const float* up_ncc,
                            const float* add_depth, const float* add_am, const float* up_add, int32_t have_add,
                            float* o_depth, float* o_near, float* o_am, void* stream);
/* ---- densification geometry of the anchor models (no ABI bump: additions only).
 * One growing level of ScaffoldGaussian.anchor_growing (gssr/gaussian/scaffold_gaussian.py:555-649), general enough for the loop body of
 * OctreeGaussian.anchor_growing (octree_gaussian.py:401-534).  anchor [Na,3]: the first N0 are the original anchors and own the N0*k candidate
 * slots; the rest were added at earlier levels and only occupy cells.  mask [N0] bytes or NULL: the slots of anchor a may be candidates, and its
 * cell counts as occupied, only where mask[a] != 0 (anchors >= N0 always occupy).  Slot j of anchor a = j / k is a candidate iff
 *   thr_lo <= grads[j] < thr_hi  and  offset_mask[j]  and  (rand == NULL or rand[j] > rand_thr)  and  the mask admits a
 * (thr_hi = +inf is no upper bound: grads[j] = +inf is then a candidate; a NaN gradient never is);
 * its point is p = anchor[a] + offset[j] * scaling[a,:3] (a multiply, then an add) and its cell c = rint((p - origin) / cell) (round-half-even,
 * IEEE division), all in float32 with every operation rounded on its own.  Result: the distinct candidate cells that hold no admitted anchor,
 * in lexicographic signed (x, y, z) order (torch.unique(dim=0)); new_anchor = float(c) * cell + origin; new_feat [.,F] = the element-wise maximum
 * of anchor_feat[a] over the candidate slots of the cell (torch_scatter.scatter_max).  Bitwise deterministic.
 * Cells are packed 21 bits per axis: a candidate cell outside [-2^20, 2^20) sets the sticky word status_dev[1] (the library only ever sets it);
 * it never wraps.  gsr_anchor_level_find leaves the count in status_dev[0] and its state in `scratch` (>= gsr_anchor_level_scratch_bytes, caller-owned,
 * unmodified until the emit); the caller reads the two words (its one host synchronisation per level), sizes new_anchor [count,3] / new_feat
 * [count,F] and calls gsr_anchor_level_emit with the same level. */
typedef struct gsr_anchor_level {
    int32_t Na, N0, k, F;
    int32_t scaling_stride;           /* floats per row of scaling, >= 3 (6 for get_scaling) */
    float thr_lo, thr_hi;             /* thr_hi = +inf for Scaffold-GS */
    float rand_thr, cell;
    float origin[3];                  /* 0 for Scaffold-GS, init_pos for Octree-GS */
    const float* anchor;              /* [Na,3] */
    const uint8_t* mask;              /* [N0] or NULL */
    const float* offset;              /* [N0,k,3] */
    const float* scaling;             /* [N0,scaling_stride], activated */
    const float* anchor_feat;         /* [N0,F] */
    const float* grads;               /* [N0*k] */
    const uint8_t* offset_mask;       /* [N0*k] */
    const float* rand;                /* [N0*k] uniform draws, or NULL */
} gsr_anchor_level;
size_t gsr_anchor_level_scratch_bytes(int32_t Na, int32_t N0, int32_t k);
int gsr_anchor_level_find(const gsr_anchor_level* lv, void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[2]*/, void* stream);
int gsr_anchor_level_emit(const gsr_anchor_level* lv, const void* scratch, size_t scratch_bytes, uint32_t count, float* new_anchor /*[count,3]*/,
                          float* new_feat /*[count,F]*/, void* stream);
/* Octree-GS (OctreeGaussian.anchor_growing / weed_out, octree_gaussian.py:401-534, :203-214; additions, no ABI bump).
 * gsr_octree_weed: the cameras a new anchor is weighed against.  For a position p and a level lv, per camera (centre c, scale s), in float32
 * with every operation rounded on its own:
 *   d = sqrt(((p.x-c.x)^2 + (p.y-c.y)^2) + (p.z-c.z)^2) * s;  pred = log2(standard_dist / d) / (float)log2(fork)   (IEEE divisions)
 *   il = clamp(floor | rint (half to even) | ceil (pred), 0, levels - 1), clamped in float before the conversion
 *   visible = #cameras with lv <= il;  keep iff (float)visible / (float)C > visible_threshold.       d == 0 is outside the contract.
 * mode: 0 floor, 1 round, 2 ceil; 3 ('progressive') is an error, as the reference's own weed_out cannot run in it (:198).
 * gsr_anchor_level_find_weed is gsr_anchor_level_find with two additions; scratch, emit and the order of the result are the same.
 *   occupy [N0] bytes or NULL: where given, original anchor a occupies its cell iff occupy[a] while its slots are candidates iff mask[a]
 *     (pass B of an Octree level: candidates from level l, occupiers of level l+1); NULL: the mask decides both.  Anchors >= N0 always occupy.
 *   weed or NULL: where given, every new position is weighed with lv = weed->lv before the count is published; gsr_anchor_level_emit then
 *     writes the kept rows only.  status_dev has THREE words: {count, sticky overflow, count before the weed-out}.
 * gsr_octree_weed_out: the same function over rows (positions [U,3], levels [U]; weed->lv is not read) -> visible_count [U], keep [U]. */
#define GSR_OCTREE_WEED_CHUNK 256     /* cameras staged in LDS at a time */
typedef struct gsr_octree_weed {
    const float* cam_infos;           /* [C,4]: centre, scale */
    int32_t C, levels;
    int32_t mode;                     /* dist2level: 0 floor, 1 round, 2 ceil */
    int32_t lv;                       /* the level of every new anchor of the pass */
    float standard_dist, fork, visible_threshold;
} gsr_octree_weed;
int gsr_anchor_level_find_weed(const gsr_anchor_level* lv, const uint8_t* occupy /*[N0] or NULL*/, const gsr_octree_weed* weed /*or NULL*/, void* scratch,
                               size_t scratch_bytes, uint32_t* status_dev /*[3]*/, void* stream);
int gsr_octree_weed_out(const float* positions /*[U,3]*/, const int32_t* levels /*[U]*/, int64_t U, const gsr_octree_weed* weed,
                        int32_t* visible_count /*[U]*/, uint8_t* keep /*[U]*/, void* stream);
/* Row compaction + append for `count` tensors that share one keep mask over N rows, in one copy launch per 24 tensors (in the manner of
 * gsr_adam_step_multi): dst = [src[keep] ; tail], tail == NULL meaning n_tail rows of zeros.  Replaces the reference's per-tensor x[mask] + cat
 * (_prune_anchor_optimizer / cat_tensors_to_optimizer, scaffold_gaussian.py:460-541) over parameters, Adam moments and accumulators; the
 * keep -> position scan runs once.  `t` is a HOST array; row_bytes a multiple of 4 (16- / 8-byte copies where sizes and pointers allow);
 * dst holds (number kept + n_tail) rows and must not overlap src. */
typedef struct gsr_rows_tensor {
    const void* src; void* dst; const void* tail;
    int64_t row_bytes, n_tail;
} gsr_rows_tensor;
size_t gsr_rows_compact_scratch_bytes(int64_t N);
int gsr_rows_compact_multi(int64_t N, const uint8_t* keep /*[N]*/, int32_t count, const gsr_rows_tensor* t, void* scratch, size_t scratch_bytes,
                           void* stream);
/* ---- densify / clone / split / prune of the explicit Gaussians (3DGS, 2DGS, PGSR; no ABI bump: additions only).
 * VanillaGaussian.densify_and_prune (gssr/gaussian/vanilla_gaussian.py:295-426), TwoDGaussian.densify_and_split (twod_gaussian.py:22-46) and
 * PGSRGaussian.densify_and_prune (pgsr_gaussian.py:43-155) as one classification pass and one copy pass.  Per original Gaussian i of P:
 *   g = accum[i] / denom[i] (IEEE division, NaN -> 0);  ms = max_c scaling[i,c] over the ACTIVATED scaling [P,scaling_cols], scaling_cols 2 or 3;
 *   clone  = |g| >= clone_thr and ms <= dense_thr      (GSR_DEN_CLONE_CAP: (that ? g : 0) >  clone_cap instead);
 *   split  =  g  >= split_thr and ms >  dense_thr      (GSR_DEN_SPLIT_CAP: (that ? g : 0) >  split_cap instead, and no abs rule);
 *   abs rule (accum_abs != NULL): v = (not split and ms > dense_thr and max_radii2D[i] > abs_radii_thr) ? accum_abs[i] / denom_abs[i] : 0;
 *            split |= v >= abs_thr                     (GSR_DEN_ABS_CAP: v > abs_cap instead);
 *   pruned = opacity[i] < min_opacity or (GSR_DEN_SIZE_PRUNE and ms > world_thr); a child is pruned with ms / child_div in the place of ms.
 * The radius term of the reference's final prune compares the zeros its densification_postfix has just allocated and never fires: it is not
 * evaluated.  Output rows: [originals neither split nor pruned][clones of unpruned originals][children, repetition 0][repetition 1]...[N - 1],
 * each part in index order.  gsr_densify_plan leaves in status_dev (the caller's one host synchronisation):
 *   [0] clones selected C  [1] splits selected S  [2] originals kept  [3] clones kept  [4] split parents whose children are kept
 *   [5] splits selected by the gradient rule;   output rows = [2] + [3] + N * [4].
 * masked_out [3,P] or NULL receives the three masked values the caps take their quantile of (clone, split, abs).  `scratch`
 * (>= gsr_densify_plan_scratch_bytes, caller-owned) holds the output-row -> source-row map and must stay unmodified until the emit. */
enum { GSR_DEN_SIZE_PRUNE = 1, GSR_DEN_CLONE_CAP = 2, GSR_DEN_SPLIT_CAP = 4, GSR_DEN_ABS_CAP = 8 };
typedef struct gsr_densify_args {
    int32_t P, scaling_cols, N, flags;
    float clone_thr, split_thr, abs_thr, dense_thr, min_opacity, world_thr, abs_radii_thr, child_div;   /* child_div = 0.8 * N */
    float clone_cap, split_cap, abs_cap;
    const float *accum, *denom;       /* [P] */
    const float *accum_abs, *denom_abs; /* [P] or NULL: no abs rule */
    const float* scaling;             /* [P,scaling_cols], activated */
    const float* opacity;             /* [P], activated */
    const float* max_radii2D;         /* [P]; read by the abs rule only */
    float* masked_out;                /* [3,P] or NULL */
} gsr_densify_args;
size_t gsr_densify_plan_scratch_bytes(int32_t P, int32_t N);
int gsr_densify_plan(const gsr_densify_args* a, void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[8]*/, void* stream);
/* The copy pass, destination-driven, one launch per 24 tensors: dst row j = src row map[j]; zero_new != 0 (an Adam moment): clone and child
 * rows are zeros and nothing is read for them.  `t` is a HOST array; row_bytes any positive multiple of 4 (16- / 8-byte units where sizes and
 * pointers allow); dst holds counts[2] + counts[3] + N * counts[4] rows and must not overlap src.  counts: the HOST copy of status_dev.
 * A second launch writes the computed columns when `c` is given: a child of parent i in repetition r gets
 *   xyz = R(rotation[i] / |rotation[i]|) . (z * s) + xyz[i],  z = noise_split[r * S + (rank of i among the splits)],  s = scaling[i] (third 0 for 2 columns)
 *   scaling = log(scaling[i] / child_div)
 * and, where noise_clone is given (PGSR), a clone gets the same xyz from noise_clone[rank of i among the clones].  Float32, every operation
 * rounded on its own. */
typedef struct gsr_densify_tensor {
    const void* src; void* dst;
    int64_t row_bytes;
    int32_t zero_new, pad_;
} gsr_densify_tensor;
typedef struct gsr_densify_compute {
    const float* xyz;                 /* [P,3] source */
    const float* rotation;            /* [P,4] source, not normalised */
    float* xyz_dst;                   /* [rows,3] */
    float* scaling_dst;               /* [rows,scaling_cols] */
    const float* noise_split;         /* [N*S,3] */
    const float* noise_clone;         /* [C,3] or NULL */
} gsr_densify_compute;
int gsr_densify_emit(const gsr_densify_args* a, const void* scratch, size_t scratch_bytes, const uint32_t* counts /*[8] host*/, int32_t count,
                     const gsr_densify_tensor* t, const gsr_densify_compute* c, void* stream);
/* ---- floaters filtered from a triangle mesh (no ABI bump: additions only).
 * The four Open3D calls of the reference's post_process_mesh (gssr/utils/mesh_utils.py:28-48): cluster_connected_triangles,
 * remove_triangles_by_mask, remove_unreferenced_vertices, remove_degenerate_triangles.  Open3D is not part of the reference tree: the semantics
 * below are restated from Open3D 0.18's published sources and their PARITY IS UNPINNED.  triangles: int32 [T,3], indices into V vertices.
 *   adjacency: two triangles are adjacent iff they share an undirected edge (min(a,b), max(a,b)); a shared vertex alone does not connect, an edge
 *     of three or more triangles connects all of them, a triangle equal to another is adjacent to it, and the (a,a) edge of an index-degenerate
 *     triangle is an edge like any other.
 *   clusters: the connected components, numbered 0..C-1 in ascending order of their smallest triangle index (Open3D's BFS order).
 * gsr_mesh_cluster_triangles: triangle_clusters [T], cluster_n_triangles [T] of which the first C are written (the rest is zero), cluster_area
 *   [T] doubles or NULL likewise: sum of 0.5 * |(v1 - v0) x (v2 - v0)| in double from the float32 vertices, added up with double atomics -- the
 *   one output that is NOT bit-reproducible (the order of the additions varies from run to run); every integer output is exact.  vertices may be
 *   NULL when cluster_area is: no vertex memory is touched then, whatever V says.  status_dev [2]: {status, C}.  scratch:
 *   gsr_mesh_post_scratch_bytes(T, 0).
 * status bits: GSR_MESH_ERR_INDEX an index outside [0, V) (such a triangle is never dereferenced; the results are to be discarded),
 *   GSR_MESH_ERR_KEEP cluster_to_keep > C, GSR_MESH_ERR_INTERNAL a bounded loop ran out (cannot happen).  3T >= 2^31 is refused by every call.
 * gsr_mesh_filter_count / _emit: the filter as one count call, one read of the record by the caller (its one host synchronisation) and one emit call.
 *   1. keep rule -- remove_mask [T] bytes: triangle t goes iff remove_mask[t] != 0;  else cluster_to_keep = k > 0: with n the sorted cluster sizes and
 *      thr = max(n[C - k], floor), triangle t goes iff the size of its cluster < thr (strictly: ties stay);  else every triangle stays.
 *   2. GSR_MESH_DROP_UNREFERENCED: the vertices no triangle that survived step 1 references go, the others keep their order; the triangle indices are
 *      renumbered and the rows of every tensor in `rows` (vertices, colours, ...; src / dst / row_bytes, bit for bit) move with them.
 *   3. GSR_MESH_DROP_DEGENERATE: triangles with two equal indices go, AFTER step 2 (a vertex only such a triangle references stays).
 *   Surviving triangles keep their order.  record_dev [8 words, 5 used]: {status, C, thr, V', T'} (C and thr 0 without the cluster rule).  The emit
 *   takes the HOST copy of the record, refuses a non-zero status, and writes triangles_out [T',3] and the rows' dst [V', .]; `scratch`
 *   (>= gsr_mesh_post_scratch_bytes(T, V), caller-owned) must stay unmodified between the two calls.  Inputs are only read. */
enum { GSR_MESH_DROP_UNREFERENCED = 1, GSR_MESH_DROP_DEGENERATE = 2 };
enum { GSR_MESH_ERR_INDEX = 1, GSR_MESH_ERR_INTERNAL = 2, GSR_MESH_ERR_KEEP = 4 };
typedef struct gsr_mesh_filter {
    const int32_t* triangles;         /* [T,3] */
    const uint8_t* remove_mask;       /* [T] or NULL */
    int64_t n_triangles, n_vertices;
    int32_t cluster_to_keep;          /* 0: no cluster rule */
    int32_t floor;                    /* 50 in the reference */
    int32_t flags, pad_;
} gsr_mesh_filter;
size_t gsr_mesh_post_scratch_bytes(int64_t n_triangles, int64_t n_vertices);
int gsr_mesh_cluster_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const float* vertices /*[V,3] or NULL*/,
                               int32_t* triangle_clusters /*[T]*/, int32_t* cluster_n_triangles /*[T]*/, double* cluster_area /*[T] or NULL*/,
                               void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[2]*/, void* stream);
int gsr_mesh_filter_count(const gsr_mesh_filter* f, void* scratch, size_t scratch_bytes, uint32_t* record_dev /*[8]*/, void* stream);
int gsr_mesh_filter_emit(const gsr_mesh_filter* f, const void* scratch, size_t scratch_bytes, const uint32_t* record /*[8] host*/, int32_t n_rows,
                         const gsr_rows_tensor* rows, int32_t* triangles_out /*[T',3]*/, void* stream);
/* ---- mesh simplification by vertex clustering (no ABI bump: additions only).
 * The role of Open3D's simplify_vertex_clustering after post_process_mesh.  Open3D is not part of the reference tree and nothing here is held
 * against it: the semantics below are this project's own, stated so that every result is deterministic (no float atomics: two runs give the same
 * bits), and restated operation by operation in tests/simplify_truth.py.  Edge-collapse decimation is sequential by definition and is not offered.
 * Inputs: vertices [V,3] float32, vertex_colors [V,3] float32, triangles [T,3] int32, voxel_size > 0 (double), contraction GSR_SIMPLIFY_*.
 *   1. bound: lo = the per-axis minimum over ALL V vertices, referenced or not (a float32 minimum is exact in any order);
 *      origin = (double)lo - 0.5 * voxel_size.
 *   2. cell of a vertex: c = floor(((double)v - origin) / voxel_size) per axis: a float64 subtraction, an IEEE division, a floor.  Every component
 *      must lie in [0, 2^21) or GSR_MESH_ERR_RANGE is set; a non-finite vertex component sets GSR_MESH_ERR_NONFINITE; a triangle index outside
 *      [0, V) sets GSR_MESH_ERR_INDEX (such a triangle is never dereferenced).  With a status the results are to be discarded.
 *   3. new vertices: one per occupied cell, numbered in ascending order of the cell's lowest member vertex index; vertex_map[v] (int32 [V]) is the
 *      new index of old vertex v.  Unreferenced vertices are clustered like any other.
 *   4. average position and colour: the float64 sum of the members' (double) values, added one after another in ascending vertex index, divided by
 *      the count as a double, rounded to float32.  A vertex alone in its cell comes back bit for bit.  Colours are always the average.
 *   5. GSR_SIMPLIFY_QUADRIC: for triangle t with corners a, b, c (in range), every operation in float64, rounded on its own, left to right:
 *        a' = (double)a - origin, likewise b', c';  e1 = b' - a', e2 = c' - a';
 *        N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);  L = sqrt((Nx Nx + Ny Ny) + Nz Nz); L == 0 or non-finite: no contribution;
 *        n = N / L per component, d = -((nx a'x + ny a'y) + nz a'z), p = (nx, ny, nz, d), w = L * 0.5, q_ij = w * (p_i * p_j) for the ten i <= j.
 *      Each of the three corners adds q to the cell of that corner (two corners in one cell: twice); a cell's Q is the sum of its contributions in
 *      ascending (triangle, corner) order, starting from 0.  With a_ij = Q_ij (i, j < 3) and r_i = -Q_i3:
 *        c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11, c11 = a00 a22 - a02 a02, c12 = a01 a02 - a00 a12,
 *        c22 = a00 a11 - a01 a01;  det = (a00 c00 + a01 c01) + a02 c02;
 *        x0 = ((c00 r0 + c01 r1) + c02 r2) / det, x1 = ((c01 r0 + c11 r1) + c12 r2) / det, x2 = ((c02 r0 + c12 r1) + c22 r2) / det.
 *      The cell's position is (float)(origin + x) iff det is finite and > 0, every x_i is finite and (double)c_i * voxel_size <= x_i <=
 *      ((double)c_i + 1.0) * voxel_size on every axis; otherwise the average of step 4.  The box test is the whole guard: no determinant threshold.
 *   6. triangles: the three indices go through vertex_map; a triangle with two equal new indices goes; the rest are rotated so that the smallest
 *      index comes first (orientation kept); of every distinct rotated triple only the occurrence with the lowest original triangle index stays (a
 *      mirrored triple is another triple); survivors keep their original order and are emitted rotated.
 *   7. limits: V < 2^31 and 3T < 2^31; gsr_mesh_simplify_scratch_bytes returns 0 beyond them (and for an unknown contraction).
 * gsr_mesh_simplify_count: everything up to the counts; record_dev [8 words, 4 used] = {status, new vertices V', new triangles T', occupied cells
 *   that took the quadric position}.  The caller reads the record (its one host synchronisation), allocates, and calls gsr_mesh_simplify_emit with
 *   the HOST copy of the record and the UNMODIFIED scratch (>= gsr_mesh_simplify_scratch_bytes(T, V, contraction), caller-owned): it refuses a
 *   non-zero status and writes vertices_out [V',3], vertex_colors_out [V',3], triangles_out [T',3] and, unless NULL, vertex_map_out [V].  Inputs
 *   are only read; voxel_size and contraction are the same in both calls. */
enum { GSR_SIMPLIFY_AVERAGE = 0, GSR_SIMPLIFY_QUADRIC = 1 };
enum { GSR_MESH_ERR_RANGE = 8, GSR_MESH_ERR_NONFINITE = 16 };
size_t gsr_mesh_simplify_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t contraction);
int gsr_mesh_simplify_count(const float* vertices /*[V,3]*/, int64_t n_vertices, const int32_t* triangles /*[T,3]*/, int64_t n_triangles, double voxel_size,
                            int32_t contraction, void* scratch, size_t scratch_bytes, uint32_t* record_dev /*[8]*/, void* stream);
int gsr_mesh_simplify_emit(const float* vertices, const float* vertex_colors /*[V,3]*/, int64_t n_vertices, int64_t n_triangles, double voxel_size,
                           int32_t contraction, const void* scratch, size_t scratch_bytes, const uint32_t* record /*[8] host*/, float* vertices_out,
                           float* vertex_colors_out, int32_t* triangles_out, int32_t* vertex_map_out /*[V] or NULL*/, void* stream);
/* ---- mesh smoothing and normals (no ABI bump: additions only).
 * The role of Open3D's filter_smooth_simple / filter_smooth_laplacian / filter_smooth_taubin, compute_triangle_normals and compute_vertex_normals
 * on the mesh post_process_mesh and the simplification leave.  Open3D 0.18's published sources are the model (area-weighted vertex normals,
 * inverse-distance Laplacian weights, the (0, 0, 1) fallback) but Open3D is not part of the reference tree and PARITY IS UNPINNED: the semantics
 * below are this project's own, stated so that every result is deterministic (no float atomics: two runs give the same bits), and restated operation
 * by operation in tests/smooth_truth.py.  Mesh: vertices [V,3] float32, vertex_colors [V,3] float32, triangles [T,3] int32; V < 2^31 and 6T <= 2^32 - 4096
 * (the 6T vertex pairs are counted, with the rounding of their grids, in 32 bits), every *_scratch_bytes function below returns 0 beyond that (and for an
 * unknown scope).
 *   1. adjacency: N(i) = the set of j != i that share at least one triangle with i, distinct and ascending.  A triangle with two equal indices
 *      adds no self-loop and still connects its two distinct vertices.  A triangle index outside [0, V) sets GSR_MESH_ERR_INDEX; nothing is
 *      dereferenced through it and its triangle connects nothing.  The result is a CSR: start int32 [V + 1], neighbours int32 [E],
 *      N(i) = neighbours[start[i] .. start[i + 1]).
 *   2. triangle normal: n_t = (v1 - v0) x (v2 - v0), the float32 inputs widened to float64 and every operation in float64, rounded on its own:
 *      e1 = v1 - v0, e2 = v2 - v0, n_t = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x).  normalized: n_t / L per component with
 *      L = sqrt((nx nx + ny ny) + nz nz); where L is 0 or not finite the normal is (0, 0, 1).  Rounded to float32 once.
 *   3. vertex normal: the float64 sum, starting from 0, of the UNNORMALISED n_t over the corners that reference the vertex, added in ascending
 *      corner index 3 t + k (area weighting; a triangle that names a vertex twice adds twice); then normalised by the rule of 2, or left as the
 *      sum with normalized = 0; rounded to float32 once.  An unreferenced vertex gets (0, 0, 1) when normalised and (0, 0, 0) when not.
 *   4. smoothing: the state p (positions; with GSR_SMOOTH_SCOPE_ALL also the colours -- the only further channel that is filtered, normals are
 *      not) is held in float64 from the first step to the last and rounded to float32 once at the end.  Every sum runs over N(i) in ascending
 *      order, one addition after another.  One step, from p to q:
 *        GSR_SMOOTH_SIMPLE     q_i = (p_i + sum_j p_j) / (double)(|N(i)| + 1), the sum starting from p_i.
 *        GSR_SMOOTH_LAPLACIAN  d = p_i - p_j on the positions of the step's input, w_ij = 1.0 / (sqrt((dx dx + dy dy) + dz dz) + 1e-12);
 *                              W = sum w_ij and s = sum w_ij * p_j per channel, both starting from 0; q_i = p_i + lambda * (s / W - p_i).  The colours
 *                              use the same w.  N(i) empty: q_i = p_i -- a DEPARTURE from the model, which divides 0 by 0 there.
 *        GSR_SMOOTH_TAUBIN     one iteration = a Laplacian step with lambda, then one with mu (the model's defaults: 0.5 and -0.53).
 *      iterations = 0 copies vertices and colours bit for bit and looks at nothing.  GSR_SMOOTH_SCOPE_VERTEX copies the colours bit for bit.  A
 *      non-finite vertex component sets GSR_MESH_ERR_NONFINITE, an index out of range GSR_MESH_ERR_INDEX; with a status the results are to be
 *      discarded.  The triangles are not touched: the smoothed mesh has the input's.
 * gsr_mesh_adjacency_count: everything up to the count; record_dev [8 words, 2 used] = {status, E}.  The caller reads the record (its one host
 *   synchronisation), allocates, and calls gsr_mesh_adjacency_emit with the HOST copy of the record and the UNMODIFIED scratch
 *   (>= gsr_mesh_adjacency_scratch_bytes(T, V), caller-owned): it refuses a non-zero status and an E beyond 2^31 - 1 and writes start_out [V + 1] and
 *   neighbours_out [E].
 * gsr_mesh_normals: either output may be NULL; scratch (>= gsr_mesh_normals_scratch_bytes(T, V)) is needed for the vertex normals only;
 *   status_dev [1].
 * gsr_mesh_smooth: builds the adjacency in scratch (>= gsr_mesh_smooth_scratch_bytes(T, V, scope)) and enqueues every step behind it; the number
 *   of launches is a constant plus a constant times `iterations`, and nothing synchronises.  status_dev [2] = {status, E}.  lambda is ignored by
 *   GSR_SMOOTH_SIMPLE, mu by everything but GSR_SMOOTH_TAUBIN.  The outputs must not alias the inputs.
 * Inputs are only read.  Keeping the state in float32 between the steps would halve the gathered bytes and is not offered. */
enum { GSR_SMOOTH_SIMPLE = 0, GSR_SMOOTH_LAPLACIAN = 1, GSR_SMOOTH_TAUBIN = 2 };
enum { GSR_SMOOTH_SCOPE_ALL = 0, GSR_SMOOTH_SCOPE_VERTEX = 1 };
size_t gsr_mesh_adjacency_scratch_bytes(int64_t n_triangles, int64_t n_vertices);
int gsr_mesh_adjacency_count(const int32_t* triangles /*[T,3]*/, int64_t n_triangles, int64_t n_vertices, void* scratch, size_t scratch_bytes,
                             uint32_t* record_dev /*[8]*/, void* stream);
int gsr_mesh_adjacency_emit(int64_t n_triangles, int64_t n_vertices, const void* scratch, size_t scratch_bytes, const uint32_t* record /*[8] host*/,
                            int32_t* start_out /*[V+1]*/, int32_t* neighbours_out /*[E]*/, void* stream);
size_t gsr_mesh_normals_scratch_bytes(int64_t n_triangles, int64_t n_vertices);
int gsr_mesh_normals(const float* vertices /*[V,3]*/, int64_t n_vertices, const int32_t* triangles /*[T,3]*/, int64_t n_triangles, int32_t normalized,
                     float* triangle_normals_out /*[T,3] or NULL*/, float* vertex_normals_out /*[V,3] or NULL*/, void* scratch, size_t scratch_bytes,
                     uint32_t* status_dev /*[1]*/, void* stream);
size_t gsr_mesh_smooth_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t scope);
int gsr_mesh_smooth(const float* vertices, const float* vertex_colors /*[V,3]*/, int64_t n_vertices, const int32_t* triangles /*[T,3]*/, int64_t n_triangles,
                    int32_t filter, int32_t iterations, double lambda, double mu, int32_t scope, float* vertices_out, float* vertex_colors_out /*[V,3]*/,
                    void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[2]*/, void* stream);
/* ---- mesh rasterization and visibility (no ABI bump: additions only).
 * A mesh looked at from the cameras it was fused from: per view a depth map, a triangle-id map and perspective-correct barycentrics at the pixel grid
 * of the Gaussian rasterizers, and per triangle the number of views that see it (what the upstream evaluation scripts cull a fused mesh with before
 * they measure it).  The semantics are this project's own, restated operation by operation in tests/raster_truth.py.  Everything is float64 arithmetic
 * on widened float32 inputs, each expression evaluated operation by operation in the order written, no FMA contraction; integers are exact; every
 * output is a pure function of the inputs (no float atomics: two runs give the same bits).
 * Inputs: vertices [V,3] float32, triangles [T,3] int32, full_proj [n_views,4,4] float32 row-major (the reference's full_proj_transform), width W,
 * height H, near > 0 (double), cull_sign in {0, +1, -1}.
 *   1. view: row-vector convention (compute_sdf_perframe, gssr/utils/mesh_utils.py:199-201): c_k = ((x M[0,k] + y M[1,k]) + z M[2,k]) + M[3,k];
 *      the depth of a vertex is w = c_3.
 *   2. pixel coordinates: ndc_x = c_0 / w, px = ((ndc_x + 1) W - 1) 0.5, likewise py with c_1 and H: the rasterizers' ndc2Pix, pixel centres at
 *      integer coordinates.  Snapping: X = rint(px 256), Y = rint(py 256), ties to even, held as integers (1/256 pixel).
 *   3. a triangle is DROPPED in a view and counted in dropped[view] = {near, guard, zero_area}:
 *        near       some vertex has !(w > near).  There is NO CLIPPING -- a stated departure, conservative for culling.
 *        guard      otherwise, some coordinate has !(|X| <= 2^24) (NaN falls here): every edge function below is then an integer below 2^52.
 *        zero_area  otherwise, area2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) == 0.
 *      cull_sign != 0 keeps only the triangles whose area2 has that sign; the others are culled, not counted as dropped.
 *   4. coverage: where area2 < 0, vertices 1 and 2 are exchanged; u0, u1, u2 below are the vertices in that order, "the order of the coverage
 *      test".  For k = 0, 1, 2 with i = (k + 1) % 3, j = (k + 2) % 3: dx = Xj - Xi, dy = Yj - Yi, E_k(P) = dx (Py - Yi) - dy (Px - Xi) at the pixel
 *      centre P = (256 col, 256 row).  The pixel is covered iff for every k: E_k > 0, or E_k == 0 and (dy < 0 or (dy == 0 and dx > 0)) -- a
 *      top-left rule: a centre on a shared edge belongs to exactly one of the two triangles, whatever their winding.  Candidate pixels:
 *      ceil(Xmin / 256) .. floor(Xmax / 256) and the same in y, clamped to the image.
 *   5. depth at a covered pixel: l_k = E_k / |area2|; iw = (l0 (1/w0) + l1 (1/w1)) + l2 (1/w2) with w_k the depth of u_k; z64 = 1 / iw;
 *      z = (float)z64.  The winner of a pixel is the lexicographic minimum of (z as float32, triangle index) over the covering triangles.
 *   6. outputs per view: depth [H,W] float32, the winner's z, 0 where no triangle covers (the TSDF's "no depth"); triangle_id [H,W] int32, -1 there;
 *      barycentric [H,W,2] float32: the perspective-correct weights of the triangle's vertices 1 and 2 IN THE INDEX BUFFER'S ORDER,
 *      (float)((l_k (1/w_k)) z64) of the u_k that is that vertex; 0 where empty.
 *   7. visibility: a triangle is SEEN in a view iff it was neither dropped nor culled there and (a) it owns at least one pixel, or (b)
 *      depth_tolerance >= 0 and one of its vertices passes the vertex test: fx = rint(px), fy = rint(py) lie in [0, W - 1] x [0, H - 1], compared
 *      in float64, and that pixel is empty or w <= (double)depth[fy, fx] + depth_tolerance.  (b) is there for the triangles smaller than a pixel,
 *      which own no centre and are plainly visible.  counts [T] int32: the number of views that see the triangle.
 *   8. errors: a non-finite component of ANY vertex sets GSR_MESH_ERR_NONFINITE, a triangle index outside [0, V) GSR_MESH_ERR_INDEX (such a
 *      triangle is never dereferenced), whatever the number of views; with a status the results are to be discarded.
 *   9. limits: 3V < 2^31, 3T < 2^31, 1 <= W, H <= 16384; gsr_mesh_raster_scratch_bytes returns 0 beyond them.
 * gsr_mesh_rasterize: every output may be NULL: depth_out [n_views,H,W], triangle_id_out [n_views,H,W], barycentric_out [n_views,H,W,2],
 *   counts_out [T], dropped_out [n_views,3]; status_dev [1].  depth_tolerance < 0: no vertex test.  large_from >= 0: a triangle whose candidate box
 *   holds more than large_from pixels is rasterized by a wave with lanes as pixels, a smaller one by one thread; the outputs do not depend on it.
 *   Views are processed in chunks whose per-view scratch (8 H W + 5 T bytes per view) stays within 256 MiB (a chunk holds at least one view and at
 *   most 1024); the chunks follow each other on the stream, nothing synchronises, the number of launches is a constant per chunk.  scratch:
 *   >= gsr_mesh_raster_scratch_bytes(T, V, n_views, W, H), caller-owned.  Inputs are only read. */
size_t gsr_mesh_raster_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t n_views, int32_t width, int32_t height);
int gsr_mesh_rasterize(const float* vertices /*[V,3]*/, int64_t n_vertices, const int32_t* triangles /*[T,3]*/, int64_t n_triangles,
                       const float* full_proj /*[n_views,16]*/, int32_t n_views, int32_t width, int32_t height, double near_plane, int32_t cull_sign,
                       double depth_tolerance, int32_t large_from, float* depth_out, int32_t* triangle_id_out, float* barycentric_out,
                       int32_t* counts_out, uint32_t* dropped_out, void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[1]*/, void* stream);
/* ---- the mesh of an unbounded scene (no ABI bump: additions only).
 * GaussianExtractor.extract_mesh_unbounded (gssr/utils/mesh_utils.py:181-277) over marching_cubes_with_contraction (gssr/utils/mcube_utils.py:17-95).
 * THE LATTICE.  Samples live in contracted coordinates on a dense lattice with ascending float32 axes xs[nx], ys[ny], zs[nz] (device arrays), flat
 *   index (ix * ny + iy) * nz + iz.  The reference's sample set: per axis N = resolution / crop blocks, block b samples
 *   torch.linspace(lo_b, hi_b, crop) in float32 on the CPU with lo_b, hi_b out of np.linspace(min, max, N + 1); adjacent blocks share their boundary
 *   sample bit for bit (a linspace starts with `start` and ends with `end`), so the lattice has N * (crop - 1) + 1 distinct planes per axis
 *   (gsrast.unbounded.lattice_axes).  Every entry point takes arbitrary ascending axes.
 * UN-CONTRACTION of a sample c = (x, y, z), every float32 operation rounded on its own, left to right:
 *     mag = sqrtf(x*x + y*y + z*z);   p = mag < 1 ? c : (1 / (2 - mag)) * (c / mag) per component;   world = p * radius + center
 *     truncation t = 5f * voxel_size, and for mag > 1:  t *= 1 / (2 - fminf(mag, 1.9f))
 *   voxel_size = radius * 2 / resolution is the caller's (float32).  mag >= 2 gives inf or negative scales as in the reference: such a sample fails
 *   every comparison of the update rule and stays at 1.  center: HOST float[3].
 * gsr_unbounded_lattice_points: points [V,3] and sdf_trunc [V] of every sample, V = nx * ny * nz: what the per-frame op gsr_tsdf_integrate takes.
 * gsr_unbounded_lattice_tsdf: ALL F frames (full_proj [F,16] row-major device array, depth [F,H,W]) over every sample in one launch: the sample is
 *   un-contracted once, (tsdf, weight) start at (1, 1) and run through the frames IN ORDER in registers under the per-point rule of
 *   gsr_tsdf_integrate (depth only: the reference's sdf callable discards the colours), tsdf [nx,ny,nz] is stored once.  weight == NULL: nothing else is
 *   read or written.  weight != NULL (a further size group of a ragged frame set): tsdf and weight are read first and both written.  tsdf / weight
 *   16-byte aligned.  Bit for bit what gsr_unbounded_lattice_points + F calls of gsr_tsdf_integrate leave in tsdf.
 * MARCHING CUBES over a slab f [np,ny,nz] of consecutive x-planes with their axes xs[np], ys, zs; the rules of gsr_tsdf_sparse_mesh_* with every
 *   sample counting:
 *     case bit i = (f_i < 0) (level 0; f == 0 and NaN are outside), corners G + (i & 1, (i >> 1) & 1, (i >> 2) & 1), the same table and winding;
 *     the lattice edge from point G along axis a carries ONE vertex iff the signs of its ends differ; its position is G's coordinates with component
 *     a replaced by ax[g] + t * (ax[g + 1] - ax[g]), t = f0 / (f0 - f1), float32 without contraction, CONTRACTED coordinates;
 *     vertices in order of (gx, gy, gz, axis), z fastest; triangles in order of their cube (gx, gy, gz), then table order.
 *   A slab OWNS its first `own` planes: the vertices on edges that start there and the cubes with their origin there.  own == np: the slab ends the
 *   lattice (its last plane has no x edges and no cubes).  Otherwise own + 2 <= np: the cubes of plane own - 1 name vertices of plane `own`, whose
 *   numbers depend on that plane's x edges, i.e. on plane own + 1.  The next slab starts at plane `own`.  Concatenated slabs give the mesh of the whole
 *   lattice whatever the slab size: shared planes carry identical samples, hence identical vertices, welded by edge identity -- vertices that are merely
 *   close are never fused.  At most (2^31 - 1) / 5 numbered points ((own + 1) * ny * nz) per slab.
 *   gsr_unbounded_mc_count: count and scan; counts_host {vertices, triangles} of the slab -- the one host synchronisation; refuses
 *     vertex_base + vertices or triangle_base + triangles above 2^31 - 1.  scratch >= gsr_unbounded_mc_scratch_bytes(np, ny, nz), 16-byte aligned,
 *     unmodified until the emit (4 B per numbered point + 8 B per 256 of them).
 *   gsr_unbounded_mc_emit: vertices [n_vertices,3] (the slab's own array), triangles [n_triangles,3] holding vertex_base + the slab-local number.
 * gsr_unbounded_finish: vertices [V,3] contracted -> world IN PLACE by the un-contraction above (no truncation), then clipped to +-max_range
 *   componentwise in WORLD coordinates as the reference does.
 * gsr_unbounded_texture: the reference's second fusion pass (inv_contraction=None, scalar truncation 5f * voxel_size, return_rgb=True) fused over the
 *   frames: per vertex (tsdf, weight, rgb) = (1, 1, 0) run through the F frames in registers under the rule of gsr_tsdf_integrate (depth [F,H,W], rgb
 *   [F,3,H,W]), colors [V,3] stored once.  Any V.  Bit for bit what F calls of gsr_tsdf_integrate leave in rgb_acc.
 * Marching-cubes parity with skimage's Lewiner triangulation and trimesh's rounding weld is UNPINNED: the mesh is defined by the table and the rules above. */
int gsr_unbounded_lattice_points(int32_t nx, int32_t ny, int32_t nz, const float* xs, const float* ys, const float* zs, const float* center /*host [3]*/,
                                 float radius, float voxel_size, float* points /*[V,3]*/, float* sdf_trunc /*[V]*/, void* stream);
int gsr_unbounded_lattice_tsdf(int32_t nx, int32_t ny, int32_t nz, const float* xs, const float* ys, const float* zs, const float* center /*host [3]*/,
                               float radius, float voxel_size, int32_t F, const float* full_proj /*[F,16]*/, int32_t W, int32_t H,
                               const float* depth /*[F,H,W]*/, float* tsdf /*[nx,ny,nz]*/, float* weight /*[nx,ny,nz] in/out or NULL*/, void* stream);
size_t gsr_unbounded_mc_scratch_bytes(int32_t np, int32_t ny, int32_t nz);
int gsr_unbounded_mc_count(int32_t np, int32_t ny, int32_t nz, int32_t own, const float* tsdf /*[np,ny,nz]*/, void* scratch, size_t scratch_bytes,
                           int64_t vertex_base, int64_t triangle_base, uint64_t* counts_host /*[2]*/, void* stream);
int gsr_unbounded_mc_emit(int32_t np, int32_t ny, int32_t nz, int32_t own, const float* tsdf, const float* xs /*[np]*/, const float* ys, const float* zs,
                          const void* scratch, size_t scratch_bytes, int64_t vertex_base, int64_t n_vertices, int64_t n_triangles,
                          float* vertices /*[n_vertices,3]*/, int32_t* triangles /*[n_triangles,3]*/, void* stream);
int gsr_unbounded_finish(int64_t V, const float* center /*host [3]*/, float radius, float max_range, float* vertices /*[V,3] in place*/, void* stream);
int gsr_unbounded_texture(int64_t V, const float* vertices /*[V,3] world*/, float voxel_size, int32_t F, const float* full_proj /*[F,16]*/, int32_t W,
                          int32_t H, const float* depth /*[F,H,W]*/, const float* rgb /*[F,3,H,W]*/, float* colors /*[V,3]*/, void* stream);
size_t gsr_dist2_scratch_bytes(int32_t P);
int gsr_dist2(int32_t P, const float* points /*[P,3]*/, float* out /*[P]*/, void* scratch, size_t scratch_bytes,
              void* stream);

/* ---- anchors from the point cloud (OctreeGaussian.create_from_data: set_level, octree_sample, octree_gaussian.py:152-182; ScaffoldGaussian.
 * create_from_data: voxelize_sample, scaffold_gaussian.py:257-298; additions, no ABI bump).  N, n < 2^31.  status words are cleared by the call
 * and carry GSR_INIT_ERR_* bits afterwards; the host wrapper reads them with its results and raises.
 * gsr_cam_dist_quantiles: per camera c (cam_infos row: centre, scale), over dist_i = sqrt(((dx*dx + dy*dy) + dz*dz)) in float32 with every
 *   operation rounded on its own, the two interpolated order statistics torch.quantile gives:
 *     all_dist[2c + t] = lerp(sorted[k_lo[t]], sorted[k_hi[t]], w[t]) * scale,   t = 0 ("min", q = 1 - dist_ratio), 1 ("max", q = dist_ratio)
 *   k_lo, k_hi (0-based, k_lo <= k_hi <= k_lo + 1 < N) and w are HOST arrays of two; the caller derives them as ATen does (rank = float32(q) *
 *   (N - 1) in float32, floor, ceil, weight = rank - floor).  lerp is ATen's Lerp.h: w < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w), every
 *   operation rounded on its own.  The C x N distances are never stored: radix select over the bits of the squared distance, recomputed in each of four passes;
 *   scratch is O(C).  A point or camera that makes a distance non-finite sets GSR_INIT_ERR_NONFINITE.
 * gsr_select_lerp: the same select and lerp over a float array (any sign; NaN sets GSR_INIT_ERR_NONFINITE): out[t] for n_targets = 1 or 2 targets.
 *   n_dev (or NULL): the device-side element count, n is then the most it can be; a rank at or beyond it sets GSR_INIT_ERR_RANK.
 * gsr_voxel_unique_*: for each of L <= 32 cell sizes the distinct rows of key = rint((p - init_pos) / cell_l) per axis (subtract, IEEE divide,
 *   half to even, in the precision of the points: mode GSR_VOXEL_F32 float points, GSR_VOXEL_F64 double points; init_pos and cell are HOST
 *   doubles converted to that precision).  Keys are any int32; a quotient beyond sets GSR_INIT_ERR_KEY_RANGE, a non-finite coordinate
 *   GSR_INIT_ERR_NONFINITE.  count: record_dev [1 + L] = {status, rows of level 0, 1, ...}; the run heads stay in scratch.  emit (record: the
 *   HOST copy of those words, status 0): positions [sum, 3] = (float)(key * cell_l + init_pos) (multiply, then add; a zero key gives +0) and
 *   level [sum] = l, levels in ascending order, within a level rows ascending by x, then y, then z (torch.unique(dim=0) / np.unique(axis=0)). */
#define GSR_INIT_ERR_NONFINITE 1u
#define GSR_INIT_ERR_KEY_RANGE 2u
#define GSR_INIT_ERR_RANK 4u
#define GSR_VOXEL_F32 0
#define GSR_VOXEL_F64 1
size_t gsr_cam_dist_quantiles_scratch_bytes(int64_t N, int32_t C);
int gsr_cam_dist_quantiles(const float* points /*[N,3]*/, int64_t N, const float* cam_infos /*[C,4]*/, int32_t C, const int64_t* k_lo /*host [2]*/,
                           const int64_t* k_hi /*host [2]*/, const float* w /*host [2]*/, float* all_dist /*[2C]*/, void* scratch, size_t scratch_bytes,
                           uint32_t* status_dev /*[1]*/, void* stream);
size_t gsr_select_lerp_scratch_bytes(int64_t n);
int gsr_select_lerp(const float* values /*[n]*/, int64_t n, const uint32_t* n_dev /*or NULL*/, int32_t n_targets, const int64_t* k_lo /*host*/,
                    const int64_t* k_hi /*host*/, const float* w /*host*/, float* out /*[n_targets]*/, void* scratch, size_t scratch_bytes,
                    uint32_t* status_dev /*[1]*/, void* stream);
size_t gsr_voxel_unique_scratch_bytes(int64_t N, int32_t L);
int gsr_voxel_unique_count(const void* points /*[N,3]*/, int64_t N, int32_t L, const double* init_pos /*host [3]*/, const double* cell /*host [L]*/,
                           int32_t mode, void* scratch, size_t scratch_bytes, uint32_t* record_dev /*[1 + L]*/, void* stream);
int gsr_voxel_unique_emit(const void* points, int64_t N, int32_t L, const double* init_pos, const double* cell, int32_t mode, const void* scratch,
                          size_t scratch_bytes, const uint32_t* record /*host [1 + L]*/, float* positions /*[sum,3]*/, int32_t* level /*[sum]*/,
                          void* stream);

/* ---- neighbour views (PGSR's view_selection / calc_score, gssr/utils/mvsnet_utils.py:306-343; additions, no ABI bump).
 * For C <= GSR_VIEWS_MAX_IMAGES images (an LDS row of C doubles per workgroup), M < 2^31 observations and Np < 2^31 points, everything in float64:
 *   S[i,j] = S[j,i] = sum over the entries pid of image i's observations (i < j; in their multiplicity in image i), pid != -1 and observed by j, of
 *       exp(-(theta - theta0)^2 / (2 s^2)),  theta = (180 / pi) acos(dot(ci - p, cj - p) / |ci - p| / |cj - p|),  s = theta <= theta0 ? sigma1 : sigma2
 *   and S[i,i] = 0; near_ids / near_scores [C,k]: per image the k <= C best columns of its row, by descending score, among EQUAL scores the higher
 *   index first (a stable ascending sort, reversed); the image's own index competes with its 0.  scores [C,C] is written where it is not NULL.
 * obs_ids [M] are the images' point ids one image after the other, image a in [obs_offsets[a], obs_offsets[a + 1]); point_ids [Np] ascends strictly
 * and point_xyz [Np,3] goes with it.  id_bits = 32 promises that no id other than -1 has a bit above 2^32 set (the sort then skips the high word;
 * a broken promise sets GSR_VIEWS_ERR_ID_RANGE), 64 promises nothing.  The sums run over the shared points in ascending id: the order is a function
 * of the input alone, two calls give the same bits and S is symmetric bit for bit; no floating-point atomics.
 * *status_dev is cleared by the call and carries GSR_VIEWS_ERR_* bits afterwards (the outputs then mean nothing); the host wrapper reads it and raises:
 *   NONFINITE  a centre or a term of a score is NaN or infinite (the reference leaves a NaN score in place)
 *   ABSENT     an id that two or more distinct images observe has no row in point_ids (the reference's KeyError; seen by one image it is no error)
 *   TABLE      point_ids does not ascend strictly          OFFSETS  obs_offsets does not ascend from 0 to M
 *   ID_RANGE   id_bits = 32, but an id other than -1 is negative or 2^32 or more */
#define GSR_VIEWS_MAX_IMAGES 16384
#define GSR_VIEWS_ERR_NONFINITE 1u
#define GSR_VIEWS_ERR_ABSENT 2u
#define GSR_VIEWS_ERR_TABLE 4u
#define GSR_VIEWS_ERR_OFFSETS 8u
#define GSR_VIEWS_ERR_ID_RANGE 16u
size_t gsr_view_select_scratch_bytes(int64_t M, int32_t C);
int gsr_view_select(const double* centres /*[C,3]*/, int32_t C, const int64_t* obs_offsets /*[C + 1]*/, const int64_t* obs_ids /*[M]*/, int64_t M,
                    const int64_t* point_ids /*[Np]*/, const double* point_xyz /*[Np,3]*/, int64_t Np, double theta0, double sigma1, double sigma2,
                    int32_t k, int32_t id_bits, int32_t* near_ids /*[C,k]*/, double* near_scores /*[C,k]*/, double* scores /*[C,C] or NULL*/,
                    void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[1]*/, void* stream);

/* ---- scene partition (VastGaussian tiles: split_scene.py:39-53, gssr/utils/vastgaussian_utils.py:150-286; additions, no ABI bump).
 * T <= GSR_PART_MAX_TILES tiles (their boxes and counters are held in LDS); a tile mask is W = ceil(T / 32) words per row, bit t & 31 of word t >> 5.
 * N, M, Np < 2^31.  Everything is float64 unless said otherwise.  *status_dev carries GSR_PART_ERR_* bits afterwards; the host wrapper reads it and raises.
 * gsr_partition_boxes: mask [N,W] and counts [T] of the rows (x, y = the first two of `stride` doubles) inside boxes [T,4] = (mx, Mx, my, My), bounds
 *   included, compared in float64.  One pass over the rows whatever T.  A NaN coordinate is in no box; a NaN bound sets NONFINITE.  Clears status and counts.
 * gsr_partition_zrange: for ONE tile, count = the rows of xyz [N,3] whose bit is set (the caller knows it from counts; n_max >= count sizes the scratch):
 *   their float32 xyz compacted, gsr_dist2 on that subset, mean and population std of the distances in float64 in a fixed order (stats [T,2], row
 *   `tile`), and zrange [T,2] row `tile` = min and max of float32 z over mean - 3 std < dist < mean + 3 std (strict).  count < 4, or no distance inside,
 *   sets FEW; a coordinate that is not finite as float32, or a non-finite threshold, NONFINITE; count != the bits of the mask, COUNT.  *status_dev is
 *   NOT cleared: the caller clears it once and calls per tile.
 * gsr_partition_visibility: md [T] = 1.2 x the mean over tile t's member images (member [C,W]) of the largest Euclidean distance from the centre to
 *   the eight corners of (box t, zrange t); then per (t, c), row-major [T,C]: the corners through w2c [C,12] (rows of [R | t]) and K = (fx, fy, width / 2,
 *   height / 2) from intr [C,4] = (fx, fy, width, height), no test of the sign of z; ratio = area(hull of the eight projections, clipped to
 *   [0, width] x [0, height]) / (width height); dist = the mean over the corners of |dx| + |dy| + |dz| to centres [C,3]; add = ratio > threshold and
 *   dist < md[t] and c is no member of t.  A hull of zero area gives ratio 0.  A corner with camera-space z == 0 sets ZERO_Z, a non-finite term NONFINITE.
 * gsr_partition_coverage_mask: point_mask [Np,W] = OR over the observations (image a in [obs_offsets[a], obs_offsets[a + 1]), id != -1) of
 *   image_mask [C,W] row a into the row of point_ids [Np] (ascending strictly) that holds the id; counts [T] = rows per tile.  An id absent from
 *   point_ids that an image of at least one tile observes sets ABSENT.  TABLE / OFFSETS as for the neighbour views.  Clears status, counts, point_mask.
 * gsr_partition_coverage_rows: rows [tile_offsets[T]] = per tile t, at tile_offsets[t] (HOST, the exclusive prefix of counts), the rows of point_mask
 *   with bit t, ascending: one compaction per tile. */
#define GSR_PART_MAX_TILES 1024
#define GSR_PART_BLOCK 256
#define GSR_PART_ERR_FEW 1u
#define GSR_PART_ERR_NONFINITE 2u
#define GSR_PART_ERR_ZERO_Z 4u
#define GSR_PART_ERR_ABSENT 8u
#define GSR_PART_ERR_TABLE 16u
#define GSR_PART_ERR_OFFSETS 32u
#define GSR_PART_ERR_COUNT 64u
int gsr_partition_boxes(const double* xyz /*[N,stride]*/, int64_t N, int32_t stride, const double* boxes /*[T,4]*/, int32_t T, uint32_t* mask /*[N,W]*/,
                        uint32_t* counts /*[T]*/, uint32_t* status_dev /*[1]*/, void* stream);
size_t gsr_partition_zrange_scratch_bytes(int64_t N, int64_t n_max);
int gsr_partition_zrange(const double* xyz /*[N,3]*/, int64_t N, const uint32_t* mask /*[N,W]*/, int32_t T, int32_t tile, int64_t count, int64_t n_max,
                         float* zrange /*[T,2]*/, double* stats /*[T,2]*/, void* scratch, size_t scratch_bytes, uint32_t* status_dev /*[1]*/, void* stream);
int gsr_partition_visibility(const double* boxes /*[T,4]*/, const float* zrange /*[T,2]*/, int32_t T, const double* w2c /*[C,12]*/, const double* centres /*[C,3]*/,
                             const double* intr /*[C,4]*/, int32_t C, const uint32_t* member /*[C,W]*/, double threshold, double* ratio /*[T,C]*/,
                             double* dist /*[T,C]*/, double* md /*[T]*/, uint8_t* add /*[T,C]*/, uint32_t* status_dev /*[1]*/, void* stream);
int gsr_partition_coverage_mask(const int64_t* obs_offsets /*[C + 1]*/, const int64_t* obs_ids /*[M]*/, int64_t M, const uint32_t* image_mask /*[C,W]*/, int32_t C,
                                const int64_t* point_ids /*[Np]*/, int64_t Np, int32_t T, uint32_t* point_mask /*[Np,W]*/, uint32_t* counts /*[T]*/,
                                uint32_t* status_dev /*[1]*/, void* stream);
size_t gsr_partition_coverage_rows_scratch_bytes(int64_t Np);
int gsr_partition_coverage_rows(const uint32_t* point_mask /*[Np,W]*/, int64_t Np, int32_t T, const int64_t* tile_offsets /*host [T + 1]*/, int64_t* rows,
                                void* scratch, size_t scratch_bytes, void* stream);

/* ---- surface distance: an extracted mesh against a ground-truth cloud (accuracy / completeness / Chamfer / F-score, the DTU and Tanks-and-Temples
 * shape of evaluation; additions, no ABI bump).  The reference tree has no evaluation: nothing here has a counterpart there.  Counts < 2^31.  Point
 * arrays are packed float32 [n,3] with no alignment beyond 4 bytes.  Scratch is caller-owned, 16-byte aligned, *_scratch_bytes() bytes.
 * gsr_nearest_points: for every query q the nearest target t under
 *     d2 = (dx*dx + dy*dy) + dz*dz,  dx = t.x - q.x, ...  float32, every operation rounded on its own;
 *   among equal d2 the lowest target index; max_dist >= 0: a target counts only if d2 <= max_dist * max_dist (float32 product; equality stays in),
 *   max_dist < 0: no cap.  A target with a non-finite coordinate never counts; a query with one, or with no counting target (n_target == 0
 *   included), gets d2 = +inf and index = -1.  Bit for bit the all-pairs search, found through a uniform grid over the targets whose pruning is
 *   conservative (csrc/gsr_chamfer.hip).  No status word and no host synchronisation.
 * gsr_sample_surface_*: per triangle (a, b, c) of triangles [T,3] over vertices [V,3]: L2 = the largest of its three squared edge lengths (the
 *   formula above), n = max(1, ceil(sqrt((double)L2) / spacing)), and n * n samples, the centroids of its n * n congruent sub-triangles: row
 *   i = 0..n-1 holds the n - i "up" ones at u = (i + 1/3) / n, v = (j + 1/3) / n, j = 0..n-i-1, then the n - i - 1 "down" ones at
 *   u = (i + 2/3) / n, v = (j + 2/3) / n;  p = (a + u * (b - a)) + v * (c - a) in double (1/3 and 2/3 the double quotients), every operation
 *   rounded on its own, rounded to float32 once.  Triangle-major, then row, then that order.  count: record_dev [4 words] = {status, 0, total as
 *   64 bits}; status GSR_CHAMFER_ERR_INDEX an index outside [0, V), GSR_CHAMFER_ERR_CAP an n above GSR_SAMPLE_MAX_N.  The caller reads the record
 *   (its one host synchronisation), refuses a status or a total of 2^31 or more, and calls emit with the scratch as count left it: points [total,3].
 * gsr_voxel_downsample_*: the cell of a point is floor((double)p / cell) per axis, inside [-2^20, 2^20) or GSR_CHAMFER_ERR_RANGE is set; per
 *   occupied cell the point with the lowest index stays, points with a non-finite coordinate go.  count: record_dev [2] = {status, kept}; emit
 *   (n_kept: the caller's copy of that count): points_out [n_kept,3] and index_out [n_kept] in ascending input index.
 * gsr_distance_stats: over d = sqrt((double)d2[i]), clamped to max_dist where max_dist >= 0 (an infinite d2 then counts as max_dist): record_dev
 *   [1 + GSR_CHAMFER_MAX_THRESHOLDS 64-bit words] = {the sum of d as a double, per threshold (HOST doubles) the number of d < threshold as
 *   uint64}.  The sum runs in a fixed order that depends on n alone: bit-reproducible.  n == 0: all zero. */
#define GSR_CHAMFER_ERR_INDEX 1u
#define GSR_CHAMFER_ERR_CAP 2u
#define GSR_CHAMFER_ERR_RANGE 4u
#define GSR_SAMPLE_MAX_N 1024
#define GSR_CHAMFER_MAX_THRESHOLDS 8
size_t gsr_nearest_points_scratch_bytes(int64_t n_query, int64_t n_target);
int gsr_nearest_points(const float* query /*[Q,3]*/, int64_t n_query, const float* target /*[T,3]*/, int64_t n_target, float max_dist, float* d2 /*[Q]*/,
                       int32_t* index /*[Q]*/, void* scratch, size_t scratch_bytes, void* stream);
size_t gsr_sample_surface_scratch_bytes(int64_t n_triangles);
int gsr_sample_surface_count(const float* vertices /*[V,3]*/, int64_t n_vertices, const int32_t* triangles /*[T,3]*/, int64_t n_triangles, double spacing,
                             void* scratch, size_t scratch_bytes, uint32_t* record_dev /*[4]*/, void* stream);
int gsr_sample_surface_emit(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double spacing, const void* scratch,
                            size_t scratch_bytes, int64_t total, float* points /*[total,3]*/, void* stream);
size_t gsr_voxel_downsample_scratch_bytes(int64_t n_points);
int gsr_voxel_downsample_count(const float* points /*[N,3]*/, int64_t n_points, double cell, void* scratch, size_t scratch_bytes, uint32_t* record_dev /*[2]*/,
                               void* stream);
int gsr_voxel_downsample_emit(const float* points, int64_t n_points, const void* scratch, size_t scratch_bytes, int64_t n_kept, float* points_out /*[n_kept,3]*/,
                              int32_t* index_out /*[n_kept]*/, void* stream);
size_t gsr_distance_stats_scratch_bytes(int64_t n);
int gsr_distance_stats(const float* d2 /*[n]*/, int64_t n, double max_dist, const double* thresholds /*host [n_thresholds]*/, int32_t n_thresholds,
                       void* record_dev /*[9 x 8 bytes]*/, void* scratch, size_t scratch_bytes, void* stream);

/* ---- registration: a reconstruction brought into the frame of its ground-truth scan before gsr_nearest_points / gsr_distance_stats score it -- the
 * similarity fit of corresponding points, point-to-point ICP, the crop to a polygon volume (the Tanks-and-Temples shape of evaluation; additions, no
 * ABI bump).  Open3D 0.18's registration_icp, TransformationEstimationPointToPoint and SelectionPolygonVolume are the model, parity with them is not
 * pinned: every result is defined here.  Counts < 2^31, point arrays packed float32 [n,3], scratch caller-owned and 16-byte aligned, as above.
 * A transformation is 16 doubles, row-major, in the COLUMN-vector convention: p' = M[0..2][0..2] p + M[0..2][3], bottom row (0,0,0,1) -- not the
 * row-vector convention of gsr_cfg.projmatrix.
 * gsr_nearest_grid_*: gsr_nearest_points in its two halves.  build: the grid over the targets into scratch (gsr_nearest_grid_scratch_bytes, the figure of
 *   gsr_nearest_points_scratch_bytes); query: any number of times against a built scratch, with the n_target and the max_dist of the build (the cell
 *   size depends on the cap).  gsr_nearest_points is build + query: the same launches, the same bits.  skip_dev (nullable): one device word; while it is
 *   non-zero every workgroup of the query returns at once and d2 / index stay as they are.
 * gsr_transform_points: out = (float)(((m00 * x + m01 * y) + m02 * z) + m03), likewise y' and z', in double on the widened input, every operation
 *   rounded on its own; non-finite coordinates come out as the arithmetic gives them.  transformation: HOST [16], finite.
 * gsr_correspondence_sums: over the pairs (p, q) = (source[i], target[index[i]]) with index[i] >= 0, in double: record_dev [GSR_REG_RECORD_WORDS 64-bit
 *   words, indices GSR_REG_R_*] = {status (uint64), n (uint64), sum p [3], sum q [3], pm = sum p / n [3], qm = sum q / n [3] (0 where n == 0),
 *   H[a][b] = sum (p - pm)_a * (q - qm)_b [9, row-major], Spp = sum ((dx*dx + dy*dy) + dz*dz) of p - pm, Sqq likewise of q - qm, M = the identity
 *   [16], the words of gsr_icp zero}.  Two passes: the means first, the centred sums with them.  The order of the additions depends on n_source alone
 *   (csrc/gsr_register.hip) and there are no float atomics: bit-reproducible.  index[i] == -1: no pair; any other index outside [0, n_target) sets
 *   GSR_REG_ERR_INDEX and counts as no pair.
 * gsr_solve_transform: from the record's n, H, Spp, Sqq, pm, qm the least-squares M with q ~ s R p + t, written to the record's M.  n < 3, Spp == 0 or
 *   Sqq == 0: GSR_REG_ERR_DEGENERATE is set and M stays as it is.  Else, everything in double and every operation rounded on its own (Horn 1987):
 *     A (symmetric 4x4): A00 = (H00 + H11) + H22, A11 = (H00 - H11) - H22, A22 = (H11 - H00) - H22, A33 = (H22 - H00) - H11,
 *       A01 = H12 - H21, A02 = H20 - H02, A03 = H01 - H10, A12 = H01 + H10, A13 = H20 + H02, A23 = H12 + H21;  V = I.
 *     Sweeps of the pairs (p,q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), until a sweep begins with all six off-diagonal elements exactly 0 or
 *       GSR_REG_SWEEPS sweeps are done.  A pair with Apq == 0 is passed over; else
 *         theta = (Aqq - App) / (2 * Apq);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta * theta + 1));  c = 1 / sqrt(t * t + 1);  s = t * c;
 *         App -= t * Apq;  Aqq += t * Apq;  Apq = Aqp = 0;
 *         for r = 0..3:  r != p, q:  (Arp, Arq) = (c * Arp - s * Arq, s * Arp + c * Arq), mirrored to Apr, Aqr;
 *                        every r:    (Vrp, Vrq) = (c * Vrp - s * Vrq, s * Vrp + c * Vrq).
 *     e = column j of V, j the index of the largest Ajj (the lowest among equal ones);  e /= sqrt(((e0*e0 + e1*e1) + e2*e2) + e3*e3);  e = -e where its
 *       first non-zero component is negative;  (w, x, y, z) = e;
 *     R00 = ((ww + xx) - yy) - zz, R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = ((ww - xx) + yy) - zz, R12 = 2 (yz - wx),
 *       R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = ((ww - xx) - yy) + zz   (ww = w * w, ...): a proper rotation whatever H, no determinant fix-up.
 *     with_scaling: s = (sum over a, then b, of Rab * Hba, added in that order from 0) / Spp and M = [s * R | qm - s * ((Ra0 pm0 + Ra1 pm1) + Ra2 pm2)];
 *       else M = [R | qm - ((Ra0 pm0 + Ra1 pm1) + Ra2 pm2)].
 *   Collinear pairs are NOT flagged: the rotation about their line is whatever the fixed order gives.
 * gsr_icp: M_0 = init (HOST [16], finite); the grid over the targets built ONCE with max_dist (>= 0, finite).  Iteration k = 0, 1, ...:
 *     P = gsr_transform_points(source, M_k) -- always of the ORIGINAL source;  (d2, index) = the query of P;  n_k = the number of index >= 0;
 *     fitness_k = (double)n_k / n_source;  rmse_k = sqrt(sum (double)d2 / n_k) over them (0 where n_k == 0; the sum in the fixed order above);
 *     k > 0 and |fitness_k - fitness_(k-1)| < relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse: converged, stop;
 *     k == max_iteration: stop;
 *     gsr_correspondence_sums(source, target, index) and gsr_solve_transform: degenerate: stop with the status, else M_(k+1) and one more iteration.
 *   Everything is enqueued at once, 9 launches per iteration after the build; the evaluation that stops raises the record's stop word and every
 *   later launch returns on it.  record_dev as above plus {fitness, inlier_rmse (doubles), n_inliers, iterations = solves done, converged, stop
 *   (uint64), sum d2 (double)} of the M at the stop, which is the record's M.  The caller reads the record: its one host synchronisation.
 * gsr_crop_polygon_volume: keep[i] = 1 iff point i is finite, axis_min <= w <= axis_max and the crossing number is odd; axis 0 / 1 / 2 = X / Y / Z is
 *   the coordinate w, (u, v) are the other two in ascending order; polygon: HOST [n_polygon,2] doubles (u, v), finite, 3 <= n_polygon <=
 *   GSR_REG_MAX_POLYGON.  In double, for every edge a -> b (vertex k - 1 to vertex k, cyclically) the edge is crossed iff
 *     (a.v > v) != (b.v > v)  and  u < ((b.u - a.u) * (v - a.v)) / (b.v - a.v) + a.u
 *   -- half-open in v, so that a vertex shared by two edges counts once.  scratch: gsr_crop_polygon_scratch_bytes(). */
#define GSR_REG_ERR_INDEX 1u
#define GSR_REG_ERR_DEGENERATE 2u
#define GSR_REG_SWEEPS 32
#define GSR_REG_MAX_POLYGON 1024
#define GSR_REG_MAX_ITERATION 4096
#define GSR_REG_RECORD_WORDS 48
#define GSR_REG_R_STATUS 0
#define GSR_REG_R_N 1
#define GSR_REG_R_SUM_P 2
#define GSR_REG_R_SUM_Q 5
#define GSR_REG_R_MEAN_P 8
#define GSR_REG_R_MEAN_Q 11
#define GSR_REG_R_H 14
#define GSR_REG_R_SPP 23
#define GSR_REG_R_SQQ 24
#define GSR_REG_R_M 25
#define GSR_REG_R_FITNESS 41
#define GSR_REG_R_RMSE 42
#define GSR_REG_R_INLIERS 43
#define GSR_REG_R_ITERATIONS 44
#define GSR_REG_R_CONVERGED 45
#define GSR_REG_R_STOP 46
#define GSR_REG_R_SUM_D2 47
size_t gsr_nearest_grid_scratch_bytes(int64_t n_target);
int gsr_nearest_grid_build(const float* target /*[T,3]*/, int64_t n_target, float max_dist, void* scratch, size_t scratch_bytes, void* stream);
int gsr_nearest_grid_query(const float* query /*[Q,3]*/, int64_t n_query, int64_t n_target, float max_dist, const void* scratch, size_t scratch_bytes,
                           float* d2 /*[Q]*/, int32_t* index /*[Q]*/, const uint32_t* skip_dev /*[1] or NULL*/, void* stream);
int gsr_transform_points(const float* points /*[N,3]*/, int64_t n_points, const double* transformation /*host [16]*/, float* out /*[N,3]*/, void* stream);
size_t gsr_correspondence_sums_scratch_bytes(int64_t n_source);
int gsr_correspondence_sums(const float* source /*[N,3]*/, int64_t n_source, const float* target /*[T,3]*/, int64_t n_target, const int32_t* index /*[N]*/,
                            void* record_dev /*[48 x 8 bytes]*/, void* scratch, size_t scratch_bytes, void* stream);
int gsr_solve_transform(void* record_dev, int32_t with_scaling, void* stream);
size_t gsr_icp_scratch_bytes(int64_t n_source, int64_t n_target);
int gsr_icp(const float* source /*[N,3]*/, int64_t n_source, const float* target /*[T,3]*/, int64_t n_target, float max_dist, const double* init /*host [16]*/,
            int32_t max_iteration, double relative_fitness, double relative_rmse, int32_t with_scaling, void* record_dev /*[48 x 8 bytes]*/, void* scratch,
            size_t scratch_bytes, void* stream);
size_t gsr_crop_polygon_scratch_bytes(void);
int gsr_crop_polygon_volume(const float* points /*[N,3]*/, int64_t n_points, const double* polygon /*host [K,2]*/, int32_t n_polygon, int32_t axis, double axis_min,
                            double axis_max, uint8_t* keep /*[N]*/, void* scratch, size_t scratch_bytes, void* stream);

/* ---- image preparation: a training photograph brought to its training size and into the tensors a camera holds (PILtoTorch,
 * gssr/utils/general_utils.py:21-27; Camera.__init__, gssr/cameras/__init__.py:59-77; additions, no ABI bump).  Pillow's 8-bit resampler is an integer
 * algorithm over a float64 coefficient table: the result is DEFINED as the bytes of PIL.Image.resize((W, H)) with its defaults (bicubic, no box, no
 * reducing_gap) and held to a restatement of the following, operation by operation (tests/images_truth.py).
 * image: uint8 [h, w, C], interleaved, row r at image + r * row_stride bytes, row_stride >= w * C; C = 1 (mode L), 3 (RGB) or 4 (RGBA).  Rows of C = 1 and 3
 *   start at any byte; for C = 4 a pixel is one dword: image and row_stride are multiples of 4.  Limits: 1 <= w, h, W, H, h * w * C < 2^31 and
 *   H * W * C < 2^31.
 * An axis of input size `in` and output size `out`, everything in double and every operation rounded on its own:
 *     scale = in / out,  fs = max(scale, 1),  support = 2 * fs,  ss = 1 / fs;
 *     output index xx:  center = (xx + 0.5) * scale,  xmin = max((int)(center - support + 0.5), 0),  xmax = min((int)(center + support + 0.5), in),
 *       n = xmax - xmin,  w_x = f(((x + xmin) - center + 0.5) * ss) for x < n;
 *     f(t), t = |t|:  ((1.5 * t - 2.5) * t * t + 1 for t < 1,  (((t - 5) * t + 8) * t - 4) * -0.5 for t < 2,  else 0;
 *     ww = the sum of the w_x in ascending x from 0;  where ww != 0:  w_x = w_x / ww;
 *     k_x = (int)(w_x * 2^22 + 0.5) for w_x >= 0, else (int)(w_x * 2^22 - 0.5): both truncate toward zero.
 *   A pass: out = clip8(((1 << 21) + sum of k_x * pixel[xmin + x]) >> 22), a signed 32-bit sum, an arithmetic shift, clip8 clamps to [0, 255].
 *   The horizontal pass (only where W != w) is rounded to uint8, the vertical pass (only where H != h) runs on its result.  An axis that does not run
 *   is evaluated here as the one tap k = 2^22 at xmin = xx, which gives the same bytes.
 * C = 4, unless (W, H) == (w, h): colours are premultiplied first, t = c * a + 128, c' = ((t >> 8) + t) >> 8, alpha is resampled as it is, and colours
 *   are un-premultiplied last: as they are where the resampled alpha is 0 or 255, else min((255 * c) / a, 255) with integer division.
 *   (W, H) == (w, h): the result is a copy.
 * Outputs, each of them nullable, from the resampled bytes v of a pixel, q_c = (float)v_c / 255.0f, the correctly rounded float32 quotient (what
 *   torch.from_numpy(u8) / 255.0 gives on the host; a product with the float32 reciprocal differs in 126 of the 256 values):
 *     out_u8     uint8 [H, W, C], interleaved and packed: v;
 *     out_planes float [n_planes, H, W], n_planes <= C: plane c = q_c -- times q_3 for c < 3 where out_mask is given;
 *     out_gray   float [H, W], C >= 3: (0.2989f * q_0 + 0.587f * q_1) + 0.114f * q_2, three products and two sums, each rounded (torchvision's
 *                Grayscale on the clamped image, taken BEFORE the mask is applied, as Camera.__init__ line 64 does);
 *     out_mask   float [H, W], C == 4 and n_planes <= 3: q_3.
 * Three launches (the two coefficient tables, the horizontal pass, the vertical pass with the outputs), no host synchronisation, no atomics.  The
 * tables and the intermediate image live in the scratch: caller-owned, 16-byte aligned, gsr_image_resample_scratch_bytes() bytes (0: sizes out of range).
 * GSR_IMG_HSTRIP / GSR_IMG_VSTRIP: output columns per workgroup of the horizontal / vertical pass (csrc/gsr_image.hip). */
#define GSR_IMG_HSTRIP 256
#define GSR_IMG_VSTRIP 256
size_t gsr_image_resample_scratch_bytes(int32_t w, int32_t h, int32_t C, int32_t W, int32_t H);
int gsr_image_resample(const uint8_t* image /*[h,w,C]*/, int32_t w, int32_t h, int32_t C, int64_t row_stride, int32_t W, int32_t H, uint8_t* out_u8 /*[H,W,C] or NULL*/,
                       float* out_planes /*[n_planes,H,W] or NULL*/, int32_t n_planes, float* out_gray /*[H,W] or NULL*/, float* out_mask /*[H,W] or NULL*/,
                       void* scratch, size_t scratch_bytes, void* stream);

/* ---- introspection for parity tests (copies a private stage result into a caller DEVICE buffer) */
enum gsr_debug_field {
    GSR_DBG_TILES_TOUCHED = 0, /* uint32 [P]                                      (from geom)    */
    GSR_DBG_POINT_LIST = 1,    /* uint32 [R] gaussian ids sorted by (tile, depth) (from binning) */
    GSR_DBG_RANGES = 2,        /* uint32 [T,2]                                    (from img)     */
    GSR_DBG_FINAL_T = 3,       /* float  [N] (SURFEL [3,N])                       (from img)     */
    GSR_DBG_N_CONTRIB = 4,     /* uint32 [N] (SURFEL [2,N])                       (from img)     */
    GSR_DBG_TILE_KEYS = 5,     /* uint32 [R] tile id per sorted instance          (from binning) */
    GSR_DBG_REC = 6            /* float  [P,4S] packed blend records, S = 3 EWA / 4 PLANE / 5 SURFEL float4 (from geom) */
};
int gsr_debug_read(const gsr_cfg* cfg, int32_t field, const void* geom, const void* binning, size_t binning_bytes,
                   const void* img, uint32_t num_rendered, void* dst, void* stream);

/* ---- optional stage profiler: HIP events recorded on the launch stream around every stage.
 * gsr_profile_enable(1) resets and starts every stage, gsr_profile_enable(mask << 8) only the stages whose bit is set in mask (an event pair
 * costs ~10 us of stream idle time per stage boundary), 0 stops; gsr_profile_read returns total milliseconds and launch counts per label. */
enum gsr_prof_label {
    GSR_PROF_PREPROCESS = 0, GSR_PROF_DEPTH_ORDER = 1, GSR_PROF_BINNING = 2, GSR_PROF_BLEND_FWD = 3,
    GSR_PROF_BWD_MEMSET = 4, GSR_PROF_BLEND_BWD = 5, GSR_PROF_PREPROCESS_BWD = 6, GSR_PROF_LABELS = 8
};
int gsr_profile_enable(int32_t enable);
int gsr_profile_read(double* ms_total /*[GSR_PROF_LABELS]*/, uint64_t* counts /*[GSR_PROF_LABELS]*/);

const char* gsr_last_error(void);
int32_t gsr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H */
