// gsr_mesh_raster.hip -- a triangle mesh rasterized into the cameras it was fused from: depth, triangle id and perspective-correct barycentrics per
// pixel, and per triangle the number of views that see it.  The semantics are this project's own, DEFINED in include/gsrast.h ("mesh rasterization
// and visibility") and restated operation by operation in tests/raster_truth.py: float64 arithmetic on widened float32 inputs,
// coordinates snapped to 1/256 pixel and held as integers, int64 edge functions under a top-left rule, and per pixel the lexicographic minimum of
// (float32 depth, triangle index).  Every output is a pure function of the inputs: no float atomics, two runs give the same bits.
//
//   key buffer   [views of the chunk][H W] 64-bit words, float32 bits of z << 32 | triangle, cleared to all ones.  z > 0, so the bits order like the
//                depths and an unsigned 64-bit atomicMin leaves the winner whatever the order of arrival.
//   k_rs_small   one thread per (triangle, view of the chunk): set-up, the drop counts, and the triangle rasterized inline where its candidate box
//                has at most large_from pixels.  A plain load of the key in front of the atomic skips it where the key is already smaller: the
//                minimum only ever falls, so a stale value can only cost an atomic, never lose one.  A larger box goes to the view's list
//                (wave-aggregated append; at most one entry per triangle and view, capacity T).
//   k_rs_large   a fixed grid; a wave takes the entries of a view's list in turn and sweeps the box with lanes as pixels, 8x8 per step.
//   k_rs_resolve one thread per pixel: the key unpacked into the maps, the winner's barycentrics from its own set-up, its triangle marked as owner.
//   k_rs_counts  one thread per triangle: over the views of the chunk, owner or -- with a tolerance -- the vertex test against the keys; one plain add.
// The set-up is ONE function (rs_setup) evaluated again wherever it is needed; with FMA contraction off (PRE_FLAGS) every evaluation gives the same bits.
// Views go through in chunks that keep the per-view scratch within RS_BUDGET bytes; chunks follow each other on the stream, nothing synchronises.
// Termination: every loop runs over a clamped box, a list of known length or the views of a chunk; no kernel waits for another workgroup.
#include "gsr_common.h"
#include <algorithm>

#define RS_BLOCK 256
#define RS_BUDGET ((size_t)256 << 20)         // per-view scratch of one chunk (a single view may exceed it)
#define RS_CHUNK_MAX 1024                     // views per chunk at most (grid.y)
#define RS_LARGE_BLOCKS 1024                  // workgroups per view of the sweep over the large triangles
#define RS_DIM_MAX 16384                      // width, height
#define RS_EMPTY 0xFFFFFFFFFFFFFFFFull

enum { RS_OK = 0, RS_NEAR = 1, RS_GUARD = 2, RS_ZERO = 3, RS_CULLED = 4, RS_BAD = 5 };

struct RsArgs {
    const float* verts; const int32_t* tris; const float* mats;       // mats: the first view of the chunk
    uint32_t T, V; int32_t W, H;
    double near_; int32_t cull_sign;
};
struct RsSetup {
    long long X[3], Y[3], area2;              // in the order of the coverage test: vertices 1 and 2 exchanged where swapped
    double rw[3];                             // 1 / w
    double px[3], py[3], w[3];                // unsnapped pixel coordinates and depths, index buffer's order
    bool swapped;
};

__device__ __forceinline__ bool rs_finite(float x) { return x - x == 0.f; }

// The set-up of triangle t in the view with matrix M (row-vector convention: c_k = ((x M[0,k] + y M[1,k]) + z M[2,k]) + M[3,k])
__device__ __forceinline__ int rs_setup(const RsArgs& a, const float* __restrict__ M, uint32_t t, RsSetup& s)
{
    const uint32_t ix[3] = { (uint32_t)a.tris[3 * (size_t)t], (uint32_t)a.tris[3 * (size_t)t + 1], (uint32_t)a.tris[3 * (size_t)t + 2] };
    if (ix[0] >= a.V || ix[1] >= a.V || ix[2] >= a.V) return RS_BAD;
    double Xd[3], Yd[3];
    bool nearhit = false, guard = false;
    const double Wd = (double)a.W, Hd = (double)a.H;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = (double)a.verts[3 * (size_t)ix[k]], y = (double)a.verts[3 * (size_t)ix[k] + 1], z = (double)a.verts[3 * (size_t)ix[k] + 2];
        const double c0 = ((x * (double)M[0] + y * (double)M[4]) + z * (double)M[8]) + (double)M[12];
        const double c1 = ((x * (double)M[1] + y * (double)M[5]) + z * (double)M[9]) + (double)M[13];
        const double w = ((x * (double)M[3] + y * (double)M[7]) + z * (double)M[11]) + (double)M[15];
        nearhit |= !(w > a.near_);
        const double nx = c0 / w, ny = c1 / w;
        s.px[k] = ((nx + 1.0) * Wd - 1.0) * 0.5;
        s.py[k] = ((ny + 1.0) * Hd - 1.0) * 0.5;
        s.w[k] = w;
        Xd[k] = rint(s.px[k] * 256.0);
        Yd[k] = rint(s.py[k] * 256.0);
        guard |= !(fabs(Xd[k]) <= 16777216.0) || !(fabs(Yd[k]) <= 16777216.0);
    }
    if (nearhit) return RS_NEAR;
    if (guard) return RS_GUARD;
#pragma unroll
    for (int k = 0; k < 3; k++) { s.X[k] = (long long)Xd[k]; s.Y[k] = (long long)Yd[k]; s.rw[k] = 1.0 / s.w[k]; }
    const long long area2 = (s.X[1] - s.X[0]) * (s.Y[2] - s.Y[0]) - (s.Y[1] - s.Y[0]) * (s.X[2] - s.X[0]);
    if (area2 == 0) return RS_ZERO;
    if (a.cull_sign != 0 && (area2 > 0) != (a.cull_sign > 0)) return RS_CULLED;
    s.swapped = area2 < 0;
    if (s.swapped) {
        long long q = s.X[1]; s.X[1] = s.X[2]; s.X[2] = q;
        q = s.Y[1]; s.Y[1] = s.Y[2]; s.Y[2] = q;
        const double r = s.rw[1]; s.rw[1] = s.rw[2]; s.rw[2] = r;
    }
    s.area2 = s.swapped ? -area2 : area2;                 // |area2|
    return RS_OK;
}

// The candidate pixels: ceil(min / 256) .. floor(max / 256) per axis, clamped to the image; false where there is none
__device__ __forceinline__ bool rs_box(const RsSetup& s, int32_t W, int32_t H, int32_t& c0, int32_t& c1, int32_t& r0, int32_t& r1)
{
    const long long xmin = min(s.X[0], min(s.X[1], s.X[2])), xmax = max(s.X[0], max(s.X[1], s.X[2]));
    const long long ymin = min(s.Y[0], min(s.Y[1], s.Y[2])), ymax = max(s.Y[0], max(s.Y[1], s.Y[2]));
    const long long a0 = max((xmin + 255) >> 8, 0ll), a1 = min(xmax >> 8, (long long)W - 1);
    const long long b0 = max((ymin + 255) >> 8, 0ll), b1 = min(ymax >> 8, (long long)H - 1);
    if (a0 > a1 || b0 > b1) return false;
    c0 = (int32_t)a0; c1 = (int32_t)a1; r0 = (int32_t)b0; r1 = (int32_t)b1;
    return true;
}

// E_k at the centre of pixel (col, row) and the top-left rule: true where the pixel is covered
__device__ __forceinline__ bool rs_cover(const RsSetup& s, int32_t col, int32_t row, long long (&E)[3])
{
    const long long Px = 256ll * col, Py = 256ll * row;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const long long dx = s.X[j] - s.X[i], dy = s.Y[j] - s.Y[i];
        E[k] = dx * (Py - s.Y[i]) - dy * (Px - s.X[i]);
        in &= E[k] > 0 || (E[k] == 0 && (dy < 0 || (dy == 0 && dx > 0)));
    }
    return in;
}

// z64 = 1 / ((l0 rw0 + l1 rw1) + l2 rw2) with l_k = E_k / |area2|, all in the order of the coverage test
__device__ __forceinline__ double rs_depth(const RsSetup& s, const long long (&E)[3], double (&l)[3])
{
    const double A = (double)s.area2;
#pragma unroll
    for (int k = 0; k < 3; k++) l[k] = (double)E[k] / A;
    const double iw = (l[0] * s.rw[0] + l[1] * s.rw[1]) + l[2] * s.rw[2];
    return 1.0 / iw;
}

__device__ __forceinline__ void rs_pixel(const RsSetup& s, uint32_t t, int32_t col, int32_t row, int32_t W, unsigned long long* __restrict__ keys)
{
    long long E[3];
    if (!rs_cover(s, col, row, E)) return;
    double l[3];
    const float z = (float)rs_depth(s, E, l);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | t;
    unsigned long long* p = keys + (size_t)row * W + col;
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// The two input errors, whatever the views: a non-finite component of ANY vertex, an index outside [0, V)
__global__ void __launch_bounds__(RS_BLOCK) k_rs_check(const float* __restrict__ verts, uint32_t n_comp, const int32_t* __restrict__ tris, uint32_t n_idx, uint32_t V,
                                                       uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i < n_comp && !rs_finite(verts[i])) atomicOr(status, (uint32_t)GSR_MESH_ERR_NONFINITE);
    if (i < n_idx && (uint32_t)tris[i] >= V) atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX);
}

// One atomic per wave and word: the lanes with `f` add up to *p
__device__ __forceinline__ void rs_wave_count(bool f, uint32_t* p)
{
    const unsigned long long m = __ballot(f);
    if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(p, (uint32_t)__popcll(m));
}

// grid (ceil(T / RS_BLOCK), views of the chunk).  dropped: [views][3] or NULL; list: [views][T]; n_list: [views]
__global__ void __launch_bounds__(RS_BLOCK) k_rs_small(RsArgs a, size_t HW, long long large_from, unsigned long long* __restrict__ keys, uint32_t* __restrict__ list,
                                                       uint32_t* __restrict__ n_list, uint32_t* __restrict__ dropped)
{
    const uint32_t t = blockIdx.x * RS_BLOCK + threadIdx.x, v = blockIdx.y;
    RsSetup s;
    const int st = t < a.T ? rs_setup(a, a.mats + 16 * (size_t)v, t, s) : RS_CULLED;
    if (dropped) {
        rs_wave_count(st == RS_NEAR, dropped + 3 * (size_t)v);
        rs_wave_count(st == RS_GUARD, dropped + 3 * (size_t)v + 1);
        rs_wave_count(st == RS_ZERO, dropped + 3 * (size_t)v + 2);
    }
    int32_t c0 = 0, c1 = -1, r0 = 0, r1 = -1;
    const bool box = st == RS_OK && rs_box(s, a.W, a.H, c0, c1, r0, r1);
    const bool large = box && (long long)(c1 - c0 + 1) * (long long)(r1 - r0 + 1) > large_from;
    const unsigned long long m = __ballot(large);
    if (m) {                                              // wave-uniform
        const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)(__ffsll((long long)m) - 1);
        uint32_t base = 0u;
        if (lane == leader) base = atomicAdd(n_list + v, (uint32_t)__popcll(m));
        base = __shfl(base, (int)leader);
        const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (large && pos < a.T) list[(size_t)v * a.T + pos] = t;
    }
    if (!box || large) return;
    unsigned long long* kv = keys + (size_t)v * HW;
    for (int32_t row = r0; row <= r1; row++)
        for (int32_t col = c0; col <= c1; col++) rs_pixel(s, t, col, row, a.W, kv);
}

// grid (RS_LARGE_BLOCKS, views of the chunk): wave g of a view takes entries g, g + waves, ... of its list
__global__ void __launch_bounds__(RS_BLOCK) k_rs_large(RsArgs a, size_t HW, unsigned long long* __restrict__ keys, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ n_list)
{
    const uint32_t v = blockIdx.y, lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (RS_BLOCK / 64) + (threadIdx.x >> 6), waves = gridDim.x * (RS_BLOCK / 64);
    const uint32_t n = min(n_list[v], a.T);
    unsigned long long* kv = keys + (size_t)v * HW;
    for (uint32_t e = wave; e < n; e += waves) {
        const uint32_t t = list[(size_t)v * a.T + e];
        if (t >= a.T) continue;
        RsSetup s;
        int32_t c0, c1, r0, r1;
        if (rs_setup(a, a.mats + 16 * (size_t)v, t, s) != RS_OK || !rs_box(s, a.W, a.H, c0, c1, r0, r1)) continue;
        for (int32_t by = r0; by <= r1; by += 8)
            for (int32_t bx = c0; bx <= c1; bx += 8) {
                const int32_t col = bx + (int32_t)(lane & 7u), row = by + (int32_t)(lane >> 3);
                if (col <= c1 && row <= r1) rs_pixel(s, t, col, row, a.W, kv);
            }
    }
}

// grid (ceil(HW / RS_BLOCK), views of the chunk); the maps start at the chunk's first view; every output may be NULL.  owner: [views][T] bytes
__global__ void __launch_bounds__(RS_BLOCK) k_rs_resolve(RsArgs a, size_t HW, const unsigned long long* __restrict__ keys, float* __restrict__ depth,
                                                         int32_t* __restrict__ tri_id, float* __restrict__ bary, uint8_t* __restrict__ owner)
{
    const size_t p = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    const uint32_t v = blockIdx.y;
    if (p >= HW) return;
    const unsigned long long key = keys[(size_t)v * HW + p];
    const size_t o = (size_t)v * HW + p;
    const uint32_t t = (uint32_t)key;
    const bool hit = key != RS_EMPTY && t < a.T;
    if (depth) depth[o] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    if (tri_id) tri_id[o] = hit ? (int32_t)t : -1;
    if (hit && owner) owner[(size_t)v * a.T + t] = 1;     // the same byte from every pixel of the triangle
    if (!bary) return;
    float b1 = 0.f, b2 = 0.f;
    RsSetup s;
    if (hit && rs_setup(a, a.mats + 16 * (size_t)v, t, s) == RS_OK) {
        long long E[3];
        double l[3];
        rs_cover(s, (int32_t)(p % (size_t)a.W), (int32_t)(p / (size_t)a.W), E);
        const double z64 = rs_depth(s, E, l);
        const float q1 = (float)((l[1] * s.rw[1]) * z64), q2 = (float)((l[2] * s.rw[2]) * z64);
        b1 = s.swapped ? q2 : q1; b2 = s.swapped ? q1 : q2;
    }
    bary[2 * o] = b1; bary[2 * o + 1] = b2;
}

// One thread per triangle: counts[t] += the views of the chunk that see it.  Seen: not dropped or culled, and an owner or -- with a tolerance --
// a vertex whose nearest pixel (ix, iy) = (rint(px), rint(py)) lies in the image and is empty or has w <= depth + tolerance.
__global__ void __launch_bounds__(RS_BLOCK) k_rs_counts(RsArgs a, size_t HW, uint32_t n_views, const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ owner,
                                                        int32_t has_tol, double tol, int32_t* __restrict__ counts)
{
    const uint32_t t = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (t >= a.T) return;
    int32_t n = 0;
    for (uint32_t v = 0; v < n_views; v++) {
        if (owner[(size_t)v * a.T + t]) { n++; continue; }
        if (!has_tol) continue;
        RsSetup s;
        if (rs_setup(a, a.mats + 16 * (size_t)v, t, s) != RS_OK) continue;
        bool seen = false;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double fx = rint(s.px[k]), fy = rint(s.py[k]);
            if (!(fx >= 0.0 && fx <= (double)(a.W - 1) && fy >= 0.0 && fy <= (double)(a.H - 1))) continue;
            const unsigned long long key = keys[(size_t)v * HW + (size_t)fy * (size_t)a.W + (size_t)fx];
            seen |= key == RS_EMPTY || s.w[k] <= (double)__uint_as_float((uint32_t)(key >> 32)) + tol;
        }
        n += seen ? 1 : 0;
    }
    if (n) counts[t] += n;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
struct RsScratch {
    uint32_t* n_list;                             // [chunk]
    unsigned long long* keys;                     // [chunk][H W]
    uint32_t* list;                               // [chunk][T]
    uint8_t* owner;                               // [chunk][T]
    uint32_t chunk; size_t bytes;
};
// 3V as well as 3T: k_rs_check takes one thread per vertex component and index, and its grid rounds 3 max(V, T) up in 32 bits
static bool rs_sizes_ok(int64_t T, int64_t V, int64_t n_views, int64_t W, int64_t H)
{
    return T >= 0 && V >= 0 && V <= 0x7FFFFFFFll && 3 * (unsigned long long)V < (1ull << 31) && T <= 0x7FFFFFFFll && 3 * (unsigned long long)T < (1ull << 31) &&
           n_views >= 0 && n_views <= 0x7FFFFFFFll && W >= 1 && H >= 1 && W <= RS_DIM_MAX && H <= RS_DIM_MAX;
}
static RsScratch rs_carve(uint64_t T, uint64_t n_views, uint64_t HW, const void* base)
{
    RsScratch m; GsrCarve c(base);
    const size_t t = T > 0 ? T : 1;
    const size_t per_view = gsr_align(HW * 8) + gsr_align(t * 4) + gsr_align(t);
    size_t chunk = RS_BUDGET / per_view;
    chunk = std::min<size_t>(std::max<size_t>(chunk, 1), RS_CHUNK_MAX);
    chunk = std::min<size_t>(chunk, n_views > 0 ? n_views : 1);
    m.chunk = (uint32_t)chunk;
    m.n_list = c.take<uint32_t>(chunk);
    m.keys = c.take<unsigned long long>(chunk * HW);
    m.list = c.take<uint32_t>(chunk * t);
    m.owner = c.take<uint8_t>(gsr_align(chunk * t, 4));
    m.bytes = c.bytes();
    return m;
}

extern "C" size_t gsr_mesh_raster_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t n_views, int32_t width, int32_t height)
{
    if (!rs_sizes_ok(n_triangles, n_vertices, n_views, width, height)) return 0;
    return rs_carve((uint64_t)n_triangles, (uint64_t)n_views, (uint64_t)width * (uint64_t)height, nullptr).bytes;
}

extern "C" int gsr_mesh_rasterize(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float* full_proj, int32_t n_views,
                                  int32_t width, int32_t height, double near_plane, int32_t cull_sign, double depth_tolerance, int32_t large_from,
                                  float* depth_out, int32_t* triangle_id_out, float* barycentric_out, int32_t* counts_out, uint32_t* dropped_out, void* scratch,
                                  size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "mesh_rasterize";
    if (!rs_sizes_ok(n_triangles, n_vertices, n_views, width, height)) {
        gsr_set_error("%s: %lld triangles / %lld vertices / %d views at %d x %d out of range: 3V and 3T must stay below 2^31, width and height within [1, %d]", who,
                      (long long)n_triangles, (long long)n_vertices, n_views, width, height, RS_DIM_MAX);
        return 1;
    }
    if (!(near_plane > 0.0)) { gsr_set_error("%s: near must be positive", who); return 1; }
    if (cull_sign < -1 || cull_sign > 1) { gsr_set_error("%s: cull_sign %d", who, cull_sign); return 1; }
    if (large_from < 0) { gsr_set_error("%s: large_from %d", who, large_from); return 1; }
    if (!status_dev || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles) || (n_views > 0 && !full_proj)) { gsr_set_error("%s: null pointer", who); return 1; }
    const uint32_t T = (uint32_t)n_triangles, V = (uint32_t)n_vertices;
    const size_t HW = (size_t)width * (size_t)height;
    const RsScratch m = rs_carve(T, (uint64_t)n_views, HW, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (counts_out && T > 0u && gsr_memset_async(counts_out, 0, (size_t)T * 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (dropped_out && n_views > 0 && gsr_memset_async(dropped_out, 0, (size_t)n_views * 12, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (V > 0u || T > 0u)
        hipLaunchKernelGGL(k_rs_check, dim3(gsr_div_up(3u * std::max(V, T), RS_BLOCK)), dim3(RS_BLOCK), 0, s, vertices, 3u * V, triangles, 3u * T, V, status_dev);
    const bool maps = depth_out || triangle_id_out || barycentric_out;
    for (int64_t v0 = 0; v0 < n_views; v0 += m.chunk) {
        const uint32_t nv = (uint32_t)std::min<int64_t>(m.chunk, n_views - v0);
        const RsArgs a = { vertices, triangles, full_proj + 16 * (size_t)v0, T, V, width, height, near_plane, cull_sign };
        if (gsr_memset_async(m.keys, 0xFF, (size_t)nv * HW * 8, s) || gsr_memset_async(m.n_list, 0, gsr_align((size_t)nv * 4, 4), s)) { gsr_set_error("%s: clear", who); return 1; }
        if (counts_out && T > 0u && gsr_memset_async(m.owner, 0, gsr_align((size_t)nv * T, 4), s)) { gsr_set_error("%s: clear", who); return 1; }
        if (T > 0u) {
            hipLaunchKernelGGL(k_rs_small, dim3(gsr_div_up(T, RS_BLOCK), nv), dim3(RS_BLOCK), 0, s, a, HW, (long long)large_from, m.keys, m.list, m.n_list,
                               dropped_out ? dropped_out + 3 * (size_t)v0 : (uint32_t*)nullptr);
            hipLaunchKernelGGL(k_rs_large, dim3(RS_LARGE_BLOCKS, nv), dim3(RS_BLOCK), 0, s, a, HW, m.keys, (const uint32_t*)m.list, (const uint32_t*)m.n_list);
        }
        if (maps || (counts_out && T > 0u))
            hipLaunchKernelGGL(k_rs_resolve, dim3((uint32_t)((HW + RS_BLOCK - 1) / RS_BLOCK), nv), dim3(RS_BLOCK), 0, s, a, HW, (const unsigned long long*)m.keys,
                               depth_out ? depth_out + (size_t)v0 * HW : (float*)nullptr, triangle_id_out ? triangle_id_out + (size_t)v0 * HW : (int32_t*)nullptr,
                               barycentric_out ? barycentric_out + 2 * (size_t)v0 * HW : (float*)nullptr, counts_out && T > 0u ? m.owner : (uint8_t*)nullptr);
        if (counts_out && T > 0u)
            hipLaunchKernelGGL(k_rs_counts, dim3(gsr_div_up(T, RS_BLOCK)), dim3(RS_BLOCK), 0, s, a, HW, nv, (const unsigned long long*)m.keys, (const uint8_t*)m.owner,
                               depth_tolerance >= 0.0 ? 1 : 0, depth_tolerance, counts_out);
    }
    return gsr_check_launch(who, s, false);
}
