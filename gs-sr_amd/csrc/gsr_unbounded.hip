// gsr_unbounded.hip -- the mesh of an unbounded scene: GaussianExtractor.extract_mesh_unbounded (gssr/utils/mesh_utils.py:181-277) over
// marching_cubes_with_contraction (gssr/utils/mcube_utils.py:17-95), on the device.  The contract is in include/gsrast.h (gsr_unbounded_*):
//   lattice:  a dense lattice in CONTRACTED coordinates with arbitrary ascending axes.  k_ub_lattice_tsdf un-contracts a sample once, runs every frame of
//             the call over it with (tsdf, weight) in registers -- the rule is tsdf_point_rule of gsr_tsdf_point.h, the one gsr_tsdf_integrate applies
//             frame by frame -- and stores 4 B per sample once, 16 bytes per thread.  No points, truncations, weights or colours in memory.
//   cubes:    count / scan / emit over a slab of x-planes.  One packed word per lattice point (which of its three edges carry a vertex, and the
//             workgroup-local prefixes of vertices and triangles) and one pair of sums per workgroup; the emit pass adds the two.  Vertices are welded by
//             edge identity: the edge from point G along axis a has one vertex whoever names it.
//   finish:   un-contraction and clip of the vertices; texture: the second fusion pass (scalar truncation, colours) fused over the frames.
// Built without FMA contraction (PRE_FLAGS): sign decisions and positions follow the float32 formulas of the contract operation for operation.
#include "gsr_common.h"
#include "gsr_scan.h"
#include "gsr_tsdf_point.h"
#include <algorithm>
#include "gsr_mc.h"

struct UbFrame {
    float cx, cy, cz, radius, voxel;
};

// contracted (x, y, z) -> world position and, where asked for, the adaptive truncation (mesh_utils.py:191-193, 213-217, 248-250)
__device__ __forceinline__ void ub_uncontract(const UbFrame& c, float x, float y, float z, float* w, float* trunc)
{
    const float mag = sqrtf(x * x + y * y + z * z);
    float px = x, py = y, pz = z;
    if (!(mag < 1.f)) {
        const float s = 1.f / (2.f - mag);
        px = s * (x / mag); py = s * (y / mag); pz = s * (z / mag);
    }
    w[0] = px * c.radius + c.cx; w[1] = py * c.radius + c.cy; w[2] = pz * c.radius + c.cz;
    if (trunc) {
        float t = 5.f * c.voxel;
        if (mag > 1.f) t *= 1.f / (2.f - fminf(mag, 1.9f));
        *trunc = t;
    }
}

struct UbAxes {
    const float *xs, *ys, *zs;
    int nx, ny, nz;
};

// ------------------------------------------------------------------------------------------------ lattice
__global__ void __launch_bounds__(256) k_ub_lattice_points(UbAxes a, UbFrame c, int64_t V, float* __restrict__ points, float* __restrict__ trunc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int iz = (int)(i % a.nz);
    const int64_t r = i / a.nz;
    const int iy = (int)(r % a.ny), ix = (int)(r / a.ny);
    float w[3], t;
    ub_uncontract(c, a.xs[ix], a.ys[iy], a.zs[iz], w, &t);
    points[3 * i] = w[0]; points[3 * i + 1] = w[1]; points[3 * i + 2] = w[2];
    trunc[i] = t;
}

// Thread i owns the samples 4 i .. 4 i + 3 of the flat [nx, ny, nz] array (z fastest; a group may run over the end of a z row).  carry: tsdf / weight
// are read first and both written (a further size group of a ragged frame set); else both start at 1 and only tsdf is written.
__global__ void __launch_bounds__(256) k_ub_lattice_tsdf(UbAxes a, UbFrame c, int64_t V, int F, const float* __restrict__ proj, int W, int H,
                                                         const float* __restrict__ depth, float* __restrict__ tsdf, float* __restrict__ weight)
{
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= V) return;
    const int n = (int)std::min<int64_t>(4, V - i0);
    int iz = (int)(i0 % a.nz);
    const int64_t r = i0 / a.nz;
    int iy = (int)(r % a.ny), ix = (int)(r / a.ny);
    float wx[4], wy[4], wz[4], tr[4], t[4] = { 1.f, 1.f, 1.f, 1.f }, wt[4] = { 1.f, 1.f, 1.f, 1.f };
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float w[3] = { 0.f, 0.f, 0.f };
        tr[k] = 1.f;
        if (k < n) ub_uncontract(c, a.xs[ix], a.ys[iy], a.zs[iz], w, &tr[k]);
        wx[k] = w[0]; wy[k] = w[1]; wz[k] = w[2];
        if (++iz == a.nz) { iz = 0; if (++iy == a.ny) { iy = 0; ix = std::min(ix + 1, a.nx - 1); } }
    }
    if (weight) {
        if (n == 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(tsdf + i0), w4 = *reinterpret_cast<const float4*>(weight + i0);
            t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w; wt[0] = w4.x; wt[1] = w4.y; wt[2] = w4.z; wt[3] = w4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < n) { t[k] = tsdf[i0 + k]; wt[k] = weight[i0 + k]; }
        }
    }
    const size_t HW = (size_t)W * H;
    for (int f = 0; f < F; f++) {
        float P[16];
#pragma unroll
        for (int k = 0; k < 16; k++) P[k] = proj[16 * f + k];      // wave-uniform: scalar loads
        const float* d = depth + (size_t)f * HW;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) tsdf_point_depth(P, wx[k], wy[k], wz[k], W, H, d, tr[k], t[k], wt[k]);
    }
    if (n == 4) {
        *reinterpret_cast<float4*>(tsdf + i0) = make_float4(t[0], t[1], t[2], t[3]);
        if (weight) *reinterpret_cast<float4*>(weight + i0) = make_float4(wt[0], wt[1], wt[2], wt[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (k < n) { tsdf[i0 + k] = t[k]; if (weight) weight[i0 + k] = wt[k]; }
    }
}

// ------------------------------------------------------------------------------------------------ cubes
// Word of lattice point i of the slab: bits [0, 11) triangles of the workgroup's cubes in front of its cube, [11, 21) vertices of the workgroup's points in
// front of it, [21, 24) its edges along x / y / z carry a vertex.  256 points per workgroup: at most 1280 triangles and 768 vertices.
#define UB_T_BITS 11
#define UB_V_BITS 10
#define UB_BLOCK 256

struct UbMc {
    const float* f;             // [np, ny, nz]
    uint32_t* word;             // [M]
    uint32_t* vsum;             // [nb] vertices per workgroup; after the scan their exclusive prefix
    uint32_t* tsum;             // [nb]
    unsigned long long* totals; // {vertices of the owned planes, triangles}
    int64_t M;                  // points numbered: the owned planes and, where there is one, the plane behind them
    int64_t P0;                 // points owned: own * ny * nz
    int np, ny, nz, own;
    uint32_t nb;
};

// the edges of point i (plane p, row gy, place gz) that carry a vertex
__device__ __forceinline__ uint32_t ub_edges(const UbMc& m, int64_t i, int p, int gy, int gz)
{
    const bool in0 = m.f[i] < 0.f;
    uint32_t e = 0;
    if (p + 1 < m.np && ((m.f[i + (int64_t)m.ny * m.nz] < 0.f) != in0)) e |= 1u;
    if (gy + 1 < m.ny && ((m.f[i + m.nz] < 0.f) != in0)) e |= 2u;
    if (gz + 1 < m.nz && ((m.f[i + 1] < 0.f) != in0)) e |= 4u;
    return e;
}
// the case of the cube with origin i, or -1 where the slab has no such cube
__device__ __forceinline__ int ub_case(const UbMc& m, int64_t i, int p, int gy, int gz)
{
    if (p >= m.own || p + 1 >= m.np || gy + 1 >= m.ny || gz + 1 >= m.nz) return -1;
    const int64_t sx = (int64_t)m.ny * m.nz;
    return mc_case([&](int k) { return m.f[i + (k & 1) * sx + ((k >> 1) & 1) * (int64_t)m.nz + ((k >> 2) & 1)]; });
}
__device__ __forceinline__ void ub_place(const UbMc& m, int64_t i, int& p, int& gy, int& gz)
{
    gz = (int)(i % m.nz);
    const int64_t r = i / m.nz;
    gy = (int)(r % m.ny); p = (int)(r / m.ny);
}

__global__ void __launch_bounds__(UB_BLOCK) k_ub_mc_count(UbMc m)
{
    __shared__ uint32_t scan[17];
    const int64_t i = (int64_t)blockIdx.x * UB_BLOCK + threadIdx.x;
    uint32_t e = 0, nt = 0;
    if (i < m.M) {
        int p, gy, gz;
        ub_place(m, i, p, gy, gz);
        e = ub_edges(m, i, p, gy, gz);
        const int c = ub_case(m, i, p, gy, gz);
        if (c >= 0) nt = mc_tris_const(c);
    }
    uint32_t totv = 0, tott = 0;
    const uint32_t pv = block_excl_scan((uint32_t)__popc(e), scan, &totv);
    const uint32_t pt = block_excl_scan(nt, scan, &tott);
    if (i < m.M) m.word[i] = pt | (pv << UB_T_BITS) | (e << (UB_T_BITS + UB_V_BITS));
    if (threadIdx.x == 0) { m.vsum[blockIdx.x] = totv; m.tsum[blockIdx.x] = tott; }
}

// vsum / tsum -> their exclusive prefixes (one workgroup), totals[0] the vertices in front of point P0, totals[1] the triangles
__global__ void __launch_bounds__(1024) k_ub_mc_scan(UbMc m)
{
    __shared__ uint32_t lds[17];
    uint32_t* const d[2] = { m.vsum, m.tsum };
    unsigned long long total[2] = { 0ull, 0ull };
    block_scan_arrays<1024, 2>(d, m.nb, lds, total);      // the prefixes fit: the host refuses slabs of more than (2^31 - 1) / 5 points
    // the vertices in front of P0, the first point that is not owned: its workgroup's prefix, read by the thread that stored it, + its own place in the workgroup
    const uint32_t b0 = (uint32_t)(m.P0 / UB_BLOCK);
    if (m.P0 < m.M && threadIdx.x == b0 % 1024u) m.totals[0] = (unsigned long long)m.vsum[b0] + ((m.word[m.P0] >> UB_T_BITS) & ((1u << UB_V_BITS) - 1u));
    if (threadIdx.x == 0) {
        if (m.P0 >= m.M) m.totals[0] = total[0];
        m.totals[1] = total[1];
    }
}

__device__ __forceinline__ uint32_t ub_vertex(const UbMc& m, int64_t j, int axis)
{
    const uint32_t w = m.word[j], e = w >> (UB_T_BITS + UB_V_BITS);
    return m.vsum[j / UB_BLOCK] + ((w >> UB_T_BITS) & ((1u << UB_V_BITS) - 1u)) + (uint32_t)__popc(e & ((1u << axis) - 1u));
}

// vertices: local to the slab's arrays; triangle indices: vbase + local
__global__ void __launch_bounds__(UB_BLOCK) k_ub_mc_emit(UbMc m, UbAxes a, int64_t vbase, int64_t nv, int64_t nt, float* __restrict__ verts,
                                                         int32_t* __restrict__ tris)
{
    __shared__ uint32_t tab[256][4];
    mc_stage_table(tab);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * UB_BLOCK + threadIdx.x;
    if (i >= m.P0 || i >= m.M) return;
    int p, gy, gz;
    ub_place(m, i, p, gy, gz);
    const uint32_t w = m.word[i], e = w >> (UB_T_BITS + UB_V_BITS);
    if (e) {
        int64_t vi = (int64_t)m.vsum[blockIdx.x] + ((w >> UB_T_BITS) & ((1u << UB_V_BITS) - 1u));
        const float f0 = m.f[i];
        const float q[3] = { a.xs[p], a.ys[gy], a.zs[gz] };
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            if (!((e >> ax) & 1u)) continue;
            const float f1 = m.f[i + (ax == 0 ? (int64_t)m.ny * m.nz : ax == 1 ? (int64_t)m.nz : 1)];
            const float t = mc_cross(f0, f1);
            const float lo = q[ax], hi = ax == 0 ? a.xs[p + 1] : ax == 1 ? a.ys[gy + 1] : a.zs[gz + 1];
            float o[3] = { q[0], q[1], q[2] };
            o[ax] = lo + t * (hi - lo);
            if (vi < nv) { verts[3 * vi] = o[0]; verts[3 * vi + 1] = o[1]; verts[3 * vi + 2] = o[2]; }
            vi++;
        }
    }
    const int c = ub_case(m, i, p, gy, gz);
    if (c < 0) return;
    const int64_t sx = (int64_t)m.ny * m.nz;
    mc_triangles(tab, c, (int64_t)m.tsum[blockIdx.x] + (w & ((1u << UB_T_BITS) - 1u)), nt, tris, [&](int cn, int axis) {
        return vbase + ub_vertex(m, i + (cn & 1) * sx + ((cn >> 1) & 1) * (int64_t)m.nz + ((cn >> 2) & 1), axis);
    });
}

// ------------------------------------------------------------------------------------------------ finish / texture
__global__ void __launch_bounds__(256) k_ub_finish(int64_t V, UbFrame c, float max_range, float* __restrict__ verts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    float w[3];
    ub_uncontract(c, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], w, nullptr);
#pragma unroll
    for (int k = 0; k < 3; k++) verts[3 * i + k] = w[k] < -max_range ? -max_range : (w[k] > max_range ? max_range : w[k]);      // np.clip: a NaN stays
}

__global__ void __launch_bounds__(256) k_ub_texture(int64_t V, const float* __restrict__ verts, float trunc, int F, const float* __restrict__ proj, int W,
                                                    int H, const float* __restrict__ depth, const float* __restrict__ rgb, float* __restrict__ colors)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    float t = 1.f, w = 1.f, col[3] = { 0.f, 0.f, 0.f };
    const size_t HW = (size_t)W * H;
    for (int f = 0; f < F; f++) {
        float P[16];
#pragma unroll
        for (int k = 0; k < 16; k++) P[k] = proj[16 * f + k];
        tsdf_point(P, x, y, z, W, H, depth + (size_t)f * HW, rgb + (size_t)f * 3 * HW, nullptr, trunc, t, w, col);
    }
    colors[3 * i] = col[0]; colors[3 * i + 1] = col[1]; colors[3 * i + 2] = col[2];
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
#define UB_MAX_POINTS (0x7FFFFFFFll / 5)      // per slab: 5 triangles per cube and 3 vertices per point stay below 2^31

static int ub_axes(const char* who, int32_t nx, int32_t ny, int32_t nz, const float* xs, const float* ys, const float* zs, UbAxes& a)
{
    if (nx < 2 || ny < 2 || nz < 2) { gsr_set_error("%s: a lattice needs at least 2 planes per axis, got %d x %d x %d", who, nx, ny, nz); return 1; }
    if (!xs || !ys || !zs) { gsr_set_error("%s: null pointer (axes)", who); return 1; }
    a.xs = xs; a.ys = ys; a.zs = zs; a.nx = nx; a.ny = ny; a.nz = nz;
    return 0;
}
static int ub_frame(const char* who, const float* center, float radius, float voxel_size, UbFrame& c)
{
    if (!center) { gsr_set_error("%s: null pointer (center)", who); return 1; }
    if (!(radius > 0.f) || !(voxel_size > 0.f)) { gsr_set_error("%s: radius and voxel_size must be positive", who); return 1; }
    c.cx = center[0]; c.cy = center[1]; c.cz = center[2]; c.radius = radius; c.voxel = voxel_size;
    return 0;
}
static int ub_frames(const char* who, int32_t F, const float* full_proj, int32_t W, int32_t H, const float* depth)
{
    if (F <= 0 || W <= 0 || H <= 0) { gsr_set_error("%s: bad sizes: %d frames of %d x %d", who, F, W, H); return 1; }
    if (!full_proj || !depth) { gsr_set_error("%s: null pointer (full_proj / depth)", who); return 1; }
    return 0;
}
static int ub_grid(const char* who, int64_t n, uint32_t& blocks)
{
    const int64_t b = (n + 255) / 256;
    if (b > 0xFFFFFFFFll / 256) {      // a launch holds fewer than 2^32 threads per dimension
        gsr_set_error("%s: %lld elements are more than one launch covers", who, (long long)n);
        return 1;
    }
    blocks = (uint32_t)b;
    return 0;
}

extern "C" int gsr_unbounded_lattice_points(int32_t nx, int32_t ny, int32_t nz, const float* xs, const float* ys, const float* zs, const float* center,
                                            float radius, float voxel_size, float* points, float* sdf_trunc, void* stream)
{
    const char* who = "unbounded_lattice_points";
    UbAxes a; UbFrame c; uint32_t blocks;
    if (ub_axes(who, nx, ny, nz, xs, ys, zs, a) || ub_frame(who, center, radius, voxel_size, c)) return 1;
    if (!points || !sdf_trunc) { gsr_set_error("%s: null pointer (outputs)", who); return 1; }
    const int64_t V = (int64_t)nx * ny * nz;
    if (ub_grid(who, V, blocks)) return 1;
    hipLaunchKernelGGL(k_ub_lattice_points, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, c, V, points, sdf_trunc);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}

extern "C" int gsr_unbounded_lattice_tsdf(int32_t nx, int32_t ny, int32_t nz, const float* xs, const float* ys, const float* zs, const float* center,
                                          float radius, float voxel_size, int32_t F, const float* full_proj, int32_t W, int32_t H, const float* depth,
                                          float* tsdf, float* weight, void* stream)
{
    const char* who = "unbounded_lattice_tsdf";
    UbAxes a; UbFrame c; uint32_t blocks;
    if (ub_axes(who, nx, ny, nz, xs, ys, zs, a) || ub_frame(who, center, radius, voxel_size, c) || ub_frames(who, F, full_proj, W, H, depth)) return 1;
    if (!tsdf) { gsr_set_error("%s: null pointer (tsdf)", who); return 1; }
    if (((uintptr_t)tsdf | (uintptr_t)weight) & 15) { gsr_set_error("%s: tsdf / weight must be 16-byte aligned", who); return 1; }
    const int64_t V = (int64_t)nx * ny * nz;
    if (ub_grid(who, (V + 3) / 4, blocks)) return 1;
    hipLaunchKernelGGL(k_ub_lattice_tsdf, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, c, V, F, full_proj, W, H, depth, tsdf, weight);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}

static int64_t ub_numbered(int32_t np, int32_t ny, int32_t nz, int32_t own) { return (int64_t)std::min(own + 1, np) * ny * nz; }
// fills the scratch pointers of `m` for M numbered points; returns the bytes
static size_t ub_carve(UbMc& m, int64_t M, const void* base)
{
    GsrCarve c(base);
    const size_t nb = (size_t)((M + UB_BLOCK - 1) / UB_BLOCK);      // workgroups
    m.word = c.take<uint32_t>((size_t)M); m.vsum = c.take<uint32_t>(nb); m.tsum = c.take<uint32_t>(nb); m.totals = c.take<unsigned long long>(2);
    return c.bytes();
}
extern "C" size_t gsr_unbounded_mc_scratch_bytes(int32_t np, int32_t ny, int32_t nz)
{
    UbMc m;
    return ub_carve(m, (np < 1 || ny < 1 || nz < 1) ? 0 : (int64_t)np * ny * nz, nullptr);
}
static int ub_mc(const char* who, int32_t np, int32_t ny, int32_t nz, int32_t own, const float* f, const void* scratch, size_t scratch_bytes, UbMc& m)
{
    if (np < 2 || ny < 2 || nz < 2) { gsr_set_error("%s: a slab needs at least 2 planes per axis, got %d x %d x %d", who, np, ny, nz); return 1; }
    if (own < 1 || !(own == np || own + 2 <= np)) {
        gsr_set_error("%s: a slab of %d planes owns all of them (the lattice's last) or at most %d, with two planes behind; got %d", who, np, np - 2, own); return 1;
    }
    if (!f || !scratch) { gsr_set_error("%s: null pointer (tsdf / scratch)", who); return 1; }
    const int64_t M = ub_numbered(np, ny, nz, own);
    if (M > UB_MAX_POINTS) { gsr_set_error("%s: %lld points in one slab, at most %lld: use a smaller slab", who, (long long)M, (long long)UB_MAX_POINTS); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, gsr_unbounded_mc_scratch_bytes(np, ny, nz))) return 1;      // a slab's size, whatever it owns
    ub_carve(m, M, scratch);
    m.f = f; m.M = M; m.P0 = (int64_t)own * ny * nz; m.np = np; m.ny = ny; m.nz = nz; m.own = own; m.nb = (uint32_t)((M + UB_BLOCK - 1) / UB_BLOCK);
    return 0;
}

extern "C" int gsr_unbounded_mc_count(int32_t np, int32_t ny, int32_t nz, int32_t own, const float* tsdf, void* scratch, size_t scratch_bytes,
                                      int64_t vertex_base, int64_t triangle_base, uint64_t* counts_host, void* stream)
{
    const char* who = "unbounded_mc_count";
    UbMc m;
    if (ub_mc(who, np, ny, nz, own, tsdf, scratch, scratch_bytes, m)) return 1;
    if (!counts_host) { gsr_set_error("%s: null pointer (counts)", who); return 1; }
    if (vertex_base < 0 || triangle_base < 0) { gsr_set_error("%s: negative base", who); return 1; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ub_mc_count, dim3(m.nb), dim3(UB_BLOCK), 0, st, m);
    hipLaunchKernelGGL(k_ub_mc_scan, dim3(1), dim3(1024), 0, st, m);
    unsigned long long tot[2] = { 0ull, 0ull };
    GSR_CHECK(hipMemcpyAsync(tot, m.totals, sizeof(tot), hipMemcpyDeviceToHost, st), "unbounded_mc_count: read totals");
    GSR_CHECK(hipStreamSynchronize(st), "unbounded_mc_count: sync");
    counts_host[0] = tot[0]; counts_host[1] = tot[1];
    if ((unsigned long long)vertex_base + tot[0] > 0x7FFFFFFFull || (unsigned long long)triangle_base + tot[1] > 0x7FFFFFFFull) {
        gsr_set_error("%s: %llu vertices / %llu triangles exceed the 2^31 - 1 an int32 index addresses", who, (unsigned long long)vertex_base + tot[0],
                      (unsigned long long)triangle_base + tot[1]);
        return 1;
    }
    return gsr_check_launch(who, st, false);
}

extern "C" int gsr_unbounded_mc_emit(int32_t np, int32_t ny, int32_t nz, int32_t own, const float* tsdf, const float* xs, const float* ys, const float* zs,
                                     const void* scratch, size_t scratch_bytes, int64_t vertex_base, int64_t n_vertices, int64_t n_triangles, float* vertices,
                                     int32_t* triangles, void* stream)
{
    const char* who = "unbounded_mc_emit";
    UbMc m; UbAxes a;
    if (ub_mc(who, np, ny, nz, own, tsdf, scratch, scratch_bytes, m) || ub_axes(who, np, ny, nz, xs, ys, zs, a)) return 1;
    if (n_vertices < 0 || n_triangles < 0 || vertex_base < 0 || vertex_base + n_vertices > 0x7FFFFFFFll || n_triangles > 0x7FFFFFFFll) {
        gsr_set_error("%s: bad counts", who); return 1;
    }
    if (n_vertices == 0 && n_triangles == 0) return 0;
    if ((n_vertices && !vertices) || (n_triangles && !triangles)) { gsr_set_error("%s: null pointer (outputs)", who); return 1; }
    const int64_t owned = std::min(m.P0, m.M);
    hipLaunchKernelGGL(k_ub_mc_emit, dim3((uint32_t)((owned + UB_BLOCK - 1) / UB_BLOCK)), dim3(UB_BLOCK), 0, (hipStream_t)stream, m, a, vertex_base, n_vertices,
                       n_triangles, vertices, triangles);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}

extern "C" int gsr_unbounded_finish(int64_t V, const float* center, float radius, float max_range, float* vertices, void* stream)
{
    const char* who = "unbounded_finish";
    UbFrame c; uint32_t blocks;
    if (V < 0) { gsr_set_error("%s: bad sizes", who); return 1; }
    if (ub_frame(who, center, radius, 1.f, c)) return 1;
    if (!(max_range >= 0.f)) { gsr_set_error("%s: max_range must not be negative", who); return 1; }
    if (V == 0) return 0;
    if (!vertices) { gsr_set_error("%s: null pointer (vertices)", who); return 1; }
    if (ub_grid(who, V, blocks)) return 1;
    hipLaunchKernelGGL(k_ub_finish, dim3(blocks), dim3(256), 0, (hipStream_t)stream, V, c, max_range, vertices);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}

extern "C" int gsr_unbounded_texture(int64_t V, const float* vertices, float voxel_size, int32_t F, const float* full_proj, int32_t W, int32_t H,
                                     const float* depth, const float* rgb, float* colors, void* stream)
{
    const char* who = "unbounded_texture";
    uint32_t blocks;
    if (V < 0) { gsr_set_error("%s: bad sizes", who); return 1; }
    if (ub_frames(who, F, full_proj, W, H, depth)) return 1;
    if (!(voxel_size > 0.f)) { gsr_set_error("%s: voxel_size must be positive", who); return 1; }
    if (V == 0) return 0;
    if (!vertices || !rgb || !colors) { gsr_set_error("%s: null pointer (vertices / rgb / colors)", who); return 1; }
    if (ub_grid(who, V, blocks)) return 1;
    hipLaunchKernelGGL(k_ub_texture, dim3(blocks), dim3(256), 0, (hipStream_t)stream, V, vertices, 5.f * voxel_size, F, full_proj, W, H, depth, rgb, colors);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}
