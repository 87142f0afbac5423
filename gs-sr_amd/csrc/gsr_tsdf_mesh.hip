// gsr_tsdf_mesh.hip -- the triangle mesh of a block-sparse TSDF volume, extracted from the pools where they lie: the role of Open3D's
// ScalableTSDFVolume::ExtractTriangleMesh in the reference's mesh extraction (gssr/utils/mesh_utils.py:154-178 `volume.extract_triangle_mesh()`).
// Nothing is materialised, exported or re-ordered: the volume is only read.  The output contract (include/gsrast.h, gsr_tsdf_sparse_mesh_*):
//   * a voxel counts iff its weight > min_weight (a clear written-group bit, a unit with stamp 0 and a unit that is not in the table read as weight 0);
//   * the cube with origin voxel G (corners G + (i & 1, (i >> 1) & 1, (i >> 2) & 1)) is valid iff its 8 corners count; case bit i = (tsdf_i < 0);
//   * the edge from G along axis a carries ONE vertex iff the signs of its ends differ and one of its four cubes is valid; it belongs to the unit of G;
//   * units in the caller's order, inside a unit voxels x-major (z fastest), inside a voxel vertices by axis and triangles in table order.
// Two passes of one workgroup per unit with the same staging: the unit's tsdf with a one-voxel halo (18^3 floats; what does not count reads 0 = outside)
// and the validity of the 17^3 cubes with an origin in [-1, 15]^3 in LDS.  Thread t owns the row (x, y) = (t >> 4, t & 15) of 16 voxels, so a block scan
// over the threads numbers vertices and triangles in x-major order.
//   count: per row a 64-bit word -- bits [0, 48): edge (z, a) carries a vertex (bit 3 z + a), bits [48, 64): vertices of the unit in front of the row --
//          and per unit the two counts.  A cube on a unit's upper faces names vertices that belong to up to 7 other units: their index is
//          base[unit] + row prefix + popcount(row bits below the edge), which is what the row words are kept for (2 KB per unit instead of a 48 KB index table).
//   scan:  exclusive prefix of the counts over the units in output order (one workgroup; the totals are 64-bit).
//   emit:  vertices, colours and triangles at their final places.
// Built without FMA contraction (PRE_FLAGS): positions follow the float32 formula of the contract operation for operation.
#include "gsr_common.h"
#include "gsr_tsdf_view.h"
#include "gsr_scan.h"
#include <algorithm>
#include "gsr_mc.h"

#define TM_H 18                          // staged edge: the unit and one voxel on either side
#define TM_HV (TM_H * TM_H * TM_H)
#define TM_C 17                          // cubes with origin -1 .. 15 per axis
#define TM_CV (TM_C * TM_C * TM_C)
#define TM_GRID 4096
#define TM_ROWS 256                      // row words per unit

struct alignas(16) TmShared {
    float f[TM_HV];                      // tsdf where the voxel counts, else 0
    unsigned long long row[TM_ROWS];
    uint32_t tab[256][4];                // the case table, a row = 16 bytes
    uint32_t scan[17];
    int nb[27];                          // pool index of the unit at offset (dx, dy, dz) in {-1, 0, 1}^3: [dx + 1 + 3 (dy + 1) + 9 (dz + 1)], -1 = reads as empty
    uint32_t nbase[8];                   // first vertex of the unit at offset {0, 1}^3: [dx + 2 dy + 4 dz]
    uint8_t ok[TM_HV];                   // the voxel counts
    uint8_t cv[TM_CV];                   // the cube is valid
};
__device__ __forceinline__ int tm_h(int x, int y, int z) { return ((x + 1) * TM_H + (y + 1)) * TM_H + (z + 1); }      // x, y, z in [-1, 16]
__device__ __forceinline__ int tm_c(int x, int y, int z) { return ((x + 1) * TM_C + (y + 1)) * TM_C + (z + 1); }      // x, y, z in [-1, 15]
__device__ __forceinline__ int tm_nb(int dx, int dy, int dz) { return dx + 1 + 3 * (dy + 1) + 9 * (dz + 1); }

struct TmArgs {
    const int32_t* order;                // [n] pool index of the k-th unit of the output
    unsigned long long* rows;            // [n][256] row words, by pool index
    int32_t* inv;                        // [n] pool index -> place in `order`
    uint32_t* base;                      // [2 n]: vertex counts, then triangle counts, by place; after the scan their exclusive prefixes
    unsigned long long* totals;          // [2]
    int n;
    float min_weight, vl;
};

// one float of plane p of voxel (x, y, z) of unit nb as the contract reads it: 0 where the written-group bit is clear
__device__ __forceinline__ bool tm_written(const SparseTsdf& v, int nb, int g) { return (v.mask[(size_t)nb * 16 + (g >> 6)] >> (g & 63)) & 1ull; }

// fills f / ok / cv / nb / tab for unit b at coordinate c.  Ends with a barrier.
__device__ __forceinline__ void tm_stage(const SparseTsdf& v, TmShared& S, int b, int n, float min_weight)
{
    const int tid = (int)threadIdx.x;
    if (tid < 27) {
        const int dx = tid % 3 - 1, dy = (tid / 3) % 3 - 1, dz = tid / 9 - 1;
        int nb = b;
        if (tid != 13) {
            const int x = v.coord[3 * b] + dx, y = v.coord[3 * b + 1] + dy, z = v.coord[3 * b + 2] + dz;
            const int lim = 1 << 20;
            nb = (x < -lim || x >= lim || y < -lim || y >= lim || z < -lim || z >= lim) ? -1 : ts_find(v, x, y, z);
            if ((uint32_t)nb >= (uint32_t)n || v.stamp[nb] == 0u) nb = -1;      // not in the table, beyond the units the caller listed, or never written
        }
        S.nb[tid] = nb;
    }
    mc_stage_table(S.tab);
    // the unit itself: its weight and tsdf planes in brick order, 16 bytes per lane (the lanes of a wave read 1 KB per plane); a clear bit loads nothing
    {
        const TsLane L = ts_lane(tid);
        const int lane = tid & 63, wv = tid >> 6;
        const float* rec = ts_unit(v, b);
        const float4* S4 = reinterpret_cast<const float4*>(rec);
        const float4* W4 = reinterpret_cast<const float4*>(rec + TS_VOX);
        const unsigned long long* M = v.mask + (size_t)b * 16;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned long long had = ts_uniform64(M[wv + 4 * r]);
            float w[4] = { 0.f, 0.f, 0.f, 0.f }, s[4] = { 0.f, 0.f, 0.f, 0.f };
            if ((had >> lane) & 1ull) { ts_unpack4(W4[tid + 256 * r], w); ts_unpack4(S4[tid + 256 * r], s); }
            const int h0 = tm_h(L.lx + 4 * r, L.iy, L.iz0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool k = w[j] > min_weight;
                S.f[h0 + j] = k ? s[j] : 0.f;
                S.ok[h0 + j] = k ? 1 : 0;
            }
        }
    }
    __syncthreads();
    // the halo: 18^3 - 16^3 = 1736 voxels of up to 26 other units
    for (int i = tid; i < TM_HV; i += 256) {
        const int hx = i / (TM_H * TM_H) - 1, hy = (i / TM_H) % TM_H - 1, hz = i % TM_H - 1;
        if (((hx | hy | hz) & ~15) == 0) continue;      // inside the unit
        const int nb = S.nb[tm_nb(hx >> 4, hy >> 4, hz >> 4)];      // -1 >> 4 = -1, 16 >> 4 = 1
        float w = 0.f, s = 0.f;
        if (nb >= 0) {
            const int x = hx & 15, y = hy & 15, z = hz & 15, g = ts_group(x, y, z);
            if (tm_written(v, nb, g)) {
                const float* rec = ts_unit(v, nb) + 4 * g + (z & 3);
                w = rec[TS_VOX];
                if (w > min_weight) s = rec[0];
            }
        }
        const bool k = w > min_weight;
        S.f[i] = k ? s : 0.f;
        S.ok[i] = k ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < TM_CV; i += 256) {
        const int cx = i / (TM_C * TM_C) - 1, cy = (i / TM_C) % TM_C - 1, cz = i % TM_C - 1;
        const int h = tm_h(cx, cy, cz);
        S.cv[i] = S.ok[h] & S.ok[h + 1] & S.ok[h + TM_H] & S.ok[h + TM_H + 1] & S.ok[h + TM_H * TM_H] & S.ok[h + TM_H * TM_H + 1] &
                  S.ok[h + TM_H * TM_H + TM_H] & S.ok[h + TM_H * TM_H + TM_H + 1];
    }
    __syncthreads();
}

// the case of the cube with origin (x, y, z) of the unit
__device__ __forceinline__ int tm_case(const TmShared& S, int x, int y, int z)
{
    const int h = tm_h(x, y, z);
    return mc_case([&](int i) { return S.f[h + (i & 1) * TM_H * TM_H + ((i >> 1) & 1) * TM_H + ((i >> 2) & 1)]; });
}
__device__ __forceinline__ uint32_t tm_tris(const TmShared& S, int c) { return mc_tris(S.tab, c); }

// row (x, y): which of its 48 edges carry a vertex, and how many triangles its 16 cubes emit
__device__ __forceinline__ unsigned long long tm_row(const TmShared& S, int x, int y, uint32_t* ntri)
{
    unsigned long long bits = 0ull;
    uint32_t nt = 0;
    for (int z = 0; z < 16; z++) {
        const int h = tm_h(x, y, z);
        const bool in0 = S.f[h] < 0.f;
        const int c = tm_c(x, y, z);
        const uint32_t v000 = S.cv[c], v100 = S.cv[c - TM_C * TM_C], v010 = S.cv[c - TM_C], v001 = S.cv[c - 1];      // cubes with origin G, G - ex, G - ey, G - ez
        const uint32_t v110 = S.cv[c - TM_C * TM_C - TM_C], v101 = S.cv[c - TM_C * TM_C - 1], v011 = S.cv[c - TM_C - 1];
        // the four cubes around the edge along axis a have their origin at G minus any subset of the other two axes
        if ((in0 != (S.f[h + TM_H * TM_H] < 0.f)) && (v000 | v010 | v001 | v011)) bits |= 1ull << (3 * z);
        if ((in0 != (S.f[h + TM_H] < 0.f)) && (v000 | v100 | v001 | v101)) bits |= 1ull << (3 * z + 1);
        if ((in0 != (S.f[h + 1] < 0.f)) && (v000 | v100 | v010 | v110)) bits |= 1ull << (3 * z + 2);
        if (v000) nt += tm_tris(S, tm_case(S, x, y, z));
    }
    *ntri = nt;
    return bits;
}

__global__ void __launch_bounds__(256) k_tm_count(SparseTsdf v, TmArgs a)
{
    __shared__ TmShared S;
    const int tid = (int)threadIdx.x;
    for (int k = blockIdx.x; k < a.n; k += gridDim.x) {
        const int b = a.order[k];
        const bool live = (uint32_t)b < (uint32_t)a.n && v.stamp[b] != 0u;      // workgroup-uniform
        if ((uint32_t)b < (uint32_t)a.n && tid == 0) a.inv[b] = k;
        if (!live) {
            if (tid == 0) { a.base[k] = 0u; a.base[a.n + k] = 0u; }
            continue;
        }
        tm_stage(v, S, b, a.n, a.min_weight);
        uint32_t nt = 0, totv = 0, tott = 0;
        const unsigned long long bits = tm_row(S, tid >> 4, tid & 15, &nt);
        const uint32_t nv = (uint32_t)__popcll(bits);
        const uint32_t pv = block_excl_scan(nv, S.scan, &totv);
        (void)block_excl_scan(nt, S.scan, &tott);
        a.rows[(size_t)b * TM_ROWS + tid] = bits | ((unsigned long long)pv << 48);      // pv <= 3 * 4096 < 2^16
        if (tid == 0) { a.base[k] = totv; a.base[a.n + k] = tott; }
    }
}

// base[0, n) and base[n, 2 n) -> their exclusive prefixes, totals[0 / 1] the sums.  One workgroup of 1024: n is the number of units, not of voxels.
__global__ void __launch_bounds__(1024) k_tm_scan(TmArgs a)
{
    __shared__ uint32_t lds[17];
    uint32_t* const d[2] = { a.base, a.base + a.n };
    unsigned long long total[2] = { 0ull, 0ull };
    block_scan_arrays<1024, 2>(d, (uint32_t)a.n, lds, total);      // an entry wraps only if the total does not fit either: the host refuses such a mesh
    if (threadIdx.x == 0) { a.totals[0] = total[0]; a.totals[1] = total[1]; }
}

// the colour of voxel (lx, ly, lz) in [0, 16]^3 of the staged unit (16 = the next unit)
__device__ __forceinline__ void tm_color(const SparseTsdf& v, const TmShared& S, int lx, int ly, int lz, float* c)
{
    c[0] = c[1] = c[2] = 0.f;
    const int nb = S.nb[tm_nb(lx >> 4, ly >> 4, lz >> 4)];
    if (nb < 0) return;
    const int x = lx & 15, y = ly & 15, z = lz & 15, g = ts_group(x, y, z);
    if (!tm_written(v, nb, g)) return;
    const float* rec = ts_unit(v, nb) + 2 * TS_VOX + 4 * g + (z & 3);
    c[0] = rec[0]; c[1] = rec[TS_VOX]; c[2] = rec[2 * TS_VOX];
}
// the index of the vertex on the edge from voxel (lx, ly, lz) in [0, 16]^3 along `axis`
__device__ __forceinline__ uint32_t tm_vertex(const TmArgs& a, const TmShared& S, int lx, int ly, int lz, int axis)
{
    const int dx = lx >> 4, dy = ly >> 4, dz = lz >> 4, row = ((lx & 15) << 4) | (ly & 15);
    unsigned long long w;
    if ((dx | dy | dz) == 0) w = S.row[row];
    else {
        const int nb = S.nb[tm_nb(dx, dy, dz)];
        if (nb < 0) return 0u;      // cannot happen: a valid cube's corners belong to written units
        w = a.rows[(size_t)nb * TM_ROWS + row];
    }
    const int bit = 3 * (lz & 15) + axis;
    return S.nbase[dx + 2 * dy + 4 * dz] + (uint32_t)(w >> 48) + (uint32_t)__popcll(w & ((1ull << bit) - 1ull));
}

__global__ void __launch_bounds__(256) k_tm_emit(SparseTsdf v, TmArgs a, float* __restrict__ verts, float* __restrict__ cols, int32_t* __restrict__ tris)
{
    __shared__ TmShared S;
    const int tid = (int)threadIdx.x;
    const unsigned long long totv = a.totals[0], tott = a.totals[1];
    for (int k = blockIdx.x; k < a.n; k += gridDim.x) {
        const int b = a.order[k];
        if ((uint32_t)b >= (uint32_t)a.n || v.stamp[b] == 0u) continue;
        const uint32_t v0 = a.base[k], t0 = a.base[a.n + k];
        const unsigned long long v1 = k + 1 < a.n ? a.base[k + 1] : totv, t1 = k + 1 < a.n ? a.base[a.n + k + 1] : tott;
        if (v1 == v0 && t1 == t0) continue;      // nothing of the surface in this unit: most units of a truncation band's free-space side
        tm_stage(v, S, b, a.n, a.min_weight);
        const unsigned long long word = a.rows[(size_t)b * TM_ROWS + tid];
        S.row[tid] = word;
        if (tid < 8) {
            const int nb = S.nb[tm_nb(tid & 1, (tid >> 1) & 1, tid >> 2)];
            S.nbase[tid] = nb >= 0 ? a.base[a.inv[nb]] : 0u;
        }
        const int x = tid >> 4, y = tid & 15;
        uint32_t nt = 0, tt = 0;
        for (int z = 0; z < 16; z++)
            if (S.cv[tm_c(x, y, z)]) nt += tm_tris(S, tm_case(S, x, y, z));
        unsigned long long ti = (unsigned long long)t0 + block_excl_scan(nt, S.scan, &tt);      // the scan's barriers also publish row / nbase
        unsigned long long vi = (unsigned long long)v0 + (uint32_t)(word >> 48);
        const int gx = v.coord[3 * b] * TS_RES + x, gy = v.coord[3 * b + 1] * TS_RES + y, gz0 = v.coord[3 * b + 2] * TS_RES;
        for (int z = 0; z < 16; z++) {
            const uint32_t eb = (uint32_t)(word >> (3 * z)) & 7u;
            if (eb) {
                const int h = tm_h(x, y, z);
                const float f0 = S.f[h];
                const float p[3] = { a.vl * ((float)gx + 0.5f), a.vl * ((float)gy + 0.5f), a.vl * ((float)(gz0 + z) + 0.5f) };
                float c0[3];
                tm_color(v, S, x, y, z, c0);
#pragma unroll
                for (int ax = 0; ax < 3; ax++) {
                    if (!((eb >> ax) & 1u)) continue;
                    const float f1 = S.f[h + (ax == 0 ? TM_H * TM_H : ax == 1 ? TM_H : 1)];
                    const float t = mc_cross(f0, f1);
                    float c1[3];
                    tm_color(v, S, x + (ax == 0), y + (ax == 1), z + (ax == 2), c1);
                    const int g = ax == 0 ? gx : ax == 1 ? gy : gz0 + z;
                    float q[3] = { p[0], p[1], p[2] };
                    q[ax] = a.vl * ((float)g + 0.5f + t);
                    if (vi < totv) {
                        verts[3 * vi] = q[0]; verts[3 * vi + 1] = q[1]; verts[3 * vi + 2] = q[2];
                        cols[3 * vi] = (c0[0] + t * (c1[0] - c0[0])) / 255.0f;
                        cols[3 * vi + 1] = (c0[1] + t * (c1[1] - c0[1])) / 255.0f;
                        cols[3 * vi + 2] = (c0[2] + t * (c1[2] - c0[2])) / 255.0f;
                    }
                    vi++;
                }
            }
            if (!S.cv[tm_c(x, y, z)]) continue;
            ti = mc_triangles(S.tab, tm_case(S, x, y, z), ti, tott, tris,
                              [&](int cn, int axis) { return tm_vertex(a, S, x + (cn & 1), y + ((cn >> 1) & 1), z + ((cn >> 2) & 1), axis); });
        }
        __syncthreads();      // the next unit's staging overwrites what slower threads still read
    }
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
// fills the scratch pointers of `a` for n units; returns the bytes
static size_t tm_carve(TmArgs& a, size_t n, const void* base)
{
    GsrCarve c(base);
    a.rows = c.take<unsigned long long>(n * TM_ROWS); a.inv = c.take<int32_t>(n); a.base = c.take<uint32_t>(2 * n); a.totals = c.take<unsigned long long>(2);
    return c.bytes();
}
extern "C" size_t gsr_tsdf_sparse_mesh_scratch_bytes(int32_t n_units)
{
    TmArgs a;
    return tm_carve(a, n_units > 0 ? (size_t)n_units : 0, nullptr);
}
static int tm_args(const char* who, const gsr_tsdf_sparse* s, int32_t n_units, const int32_t* order, float min_weight, void* scratch, size_t scratch_bytes, TmArgs& a)
{
    if (check_vol(s)) return 1;
    if (n_units <= 0 || (uint32_t)n_units > s->cap_blocks) { gsr_set_error("%s: %d units do not fit the volume", who, n_units); return 1; }
    if (!order || !scratch) { gsr_set_error("%s: null unit order / scratch", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, tm_carve(a, (size_t)n_units, scratch))) return 1;
    if (!(min_weight == min_weight)) { gsr_set_error("%s: min_weight is not a number", who); return 1; }
    a.order = order; a.n = n_units; a.min_weight = min_weight; a.vl = s->voxel_length;
    return 0;
}
extern "C" int gsr_tsdf_sparse_mesh_count(const gsr_tsdf_sparse* s, int32_t n_units, const int32_t* order, float min_weight, void* scratch, size_t scratch_bytes,
                                          uint64_t* counts_host, void* stream)
{
    TmArgs a;
    if (tm_args("tsdf_sparse_mesh_count", s, n_units, order, min_weight, scratch, scratch_bytes, a)) return 1;
    if (!counts_host) { gsr_set_error("tsdf_sparse_mesh_count: null counts"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    if (gsr_memset_async(a.inv, 0, gsr_align((size_t)n_units * sizeof(int32_t)), st)) { gsr_set_error("tsdf_sparse_mesh_count: clear"); return 1; }      // an `order` that is no permutation stays in bounds
    hipLaunchKernelGGL(k_tm_count, dim3((uint32_t)std::min(n_units, TM_GRID)), dim3(256), 0, st, make_view(s), a);
    hipLaunchKernelGGL(k_tm_scan, dim3(1), dim3(1024), 0, st, a);
    unsigned long long tot[2] = { 0ull, 0ull };
    GSR_CHECK(hipMemcpyAsync(tot, a.totals, sizeof(tot), hipMemcpyDeviceToHost, st), "tsdf_sparse_mesh_count: read totals");
    GSR_CHECK(hipStreamSynchronize(st), "tsdf_sparse_mesh_count: sync");
    counts_host[0] = tot[0]; counts_host[1] = tot[1];
    if (tot[0] > 0x7FFFFFFFull || tot[1] > 0x7FFFFFFFull) {
        gsr_set_error("tsdf_sparse_mesh_count: %llu vertices / %llu triangles exceed the 2^31 - 1 an int32 index addresses; extract the volume in parts", tot[0], tot[1]);
        return 1;
    }
    return gsr_check_launch("tsdf_sparse_mesh_count", st, false);
}
extern "C" int gsr_tsdf_sparse_mesh_emit(const gsr_tsdf_sparse* s, int32_t n_units, const int32_t* order, float min_weight, void* scratch, size_t scratch_bytes,
                                         float* vertices, float* colors, int32_t* triangles, void* stream)
{
    TmArgs a;
    if (tm_args("tsdf_sparse_mesh_emit", s, n_units, order, min_weight, scratch, scratch_bytes, a)) return 1;
    if (!vertices || !colors || !triangles) { gsr_set_error("tsdf_sparse_mesh_emit: null output arrays"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tm_emit, dim3((uint32_t)std::min(n_units, TM_GRID)), dim3(256), 0, st, make_view(s), a, vertices, colors, triangles);
    return gsr_check_launch("tsdf_sparse_mesh_emit", st, false);
}
