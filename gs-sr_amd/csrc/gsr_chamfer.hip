// gsr_chamfer.hip -- an extracted mesh held against a ground-truth cloud on the device: exact cross-set nearest neighbours, deterministic surface
// samples, voxel thinning and the float64 statistics behind accuracy / completeness / Chamfer / F-score (include/gsrast.h, "surface distance";
// DESIGN.md 4.13).  The reference tree ships no evaluation; the DTU / Tanks-and-Temples scripts this stands in for are host KD-tree code.
//
//   grid        uniform grid over the FINITE targets.  k_np_bbox: box and count (integer atomics on order-preserving bit patterns);
//               k_np_grid (one thread): the cell size h from extent and count, clamped from below by max_dist and by extent / 2^20, cells per
//               axis, and whether the dense table applies -- all on the device, the host never learns them.  A coordinate's cell is
//               clamp(floor((double(x) - min) * (1 / h)), 0, n - 1): evaluated in double, monotone in x, the same function for targets and queries.
//   sort        key = ix | iy << 21 | iz << 42 (non-finite targets: all ones, they end up behind the Tf finite ones); the project's stable LSD
//               sort on the low word, then on the high word (gsr_sort.h); run heads by gsr_compact -> ukey[r], ustart[r].
//   table       run of a cell: dense[cell] = r + 1 while nx ny nz <= the table's capacity (4 T words, at least 4096), else a binary search of ukey.
//   query       one thread per query, its cell clamped into the grid (a query outside the box starts at the nearest boundary cell), shells of
//               cells of Chebyshev radius k = 0, 1, ...  A cell / a shell is skipped / the search ends when
//                   min(best, max_dist^2) < gap^2 (1 - 1e-6) - 1e-36,      gap = the axis-aligned distance from the query to the cell planes minus
//               a slack of 1e-12 of the magnitudes involved: every target beyond has a float32 d2 STRICTLY above the best (the float32 evaluation
//               loses less than 3e-7 of the true square; a tie with a lower index can only sit at equal d2), so pruning is conservative.
//               After shells 0..CF_RINGS (dense table) or 0..CF_RINGS_SPARSE without an end the query falls back to the box scan: the sorted
//               targets in chunks of 256 with their bounding boxes (k_np_gather), every box tested under the same strict rule, by the whole
//               wave for one such query at a time (nearest box first, then whatever its best does not rule out) -- the bounded cost of a query
//               far from everything.
//   halves      grid, sort and table are the BUILD (gsr_np_build), into caller-owned scratch that then holds all a QUERY (gsr_np_query) reads, a sorted copy
//               of the targets included: an ICP against a fixed scan builds once and queries per iteration (gsr_register.hip).  gsr_nearest_points is the
//               two in a row.  A query takes a nullable device word, skip: non-zero and every workgroup returns at once, the outputs stay as they are.
//   samples     per triangle n = max(1, ceil(sqrt(double(L2)) / spacing)), n^2 centroids; count (block scan + 64-bit total), one read-back, emit
//               (a thread per sample: two binary searches find its triangle, an integer square root its row).
//   thinning    key of floor(double(p) / cell), the same sort, the first of each run keeps (stable: the lowest index), keep scan in input order.
//   statistics  d = sqrt(double(d2)) clamped to max_dist; per-block sums in a fixed order (wave butterfly, waves in order), one block adds the
//               partials and the per-block counts in order: no atomics.  Bit-reproducible.
// Built without FMA contraction (PRE_FLAGS).  Every launch is on the caller's stream; nothing synchronises; no kernel waits for another workgroup.
#include "gsr_common.h"
#include "gsr_scan.h"
#include "gsr_compact.h"
#include "gsr_reduce.h"
#include <algorithm>

#define CF_BLOCK 256
#define CF_AXIS_BITS 21
#define CF_AXIS_MAX (1 << CF_AXIS_BITS)       // cells per axis at most
#define CF_BAD 0xFFFFFFFFu                    // both words of the key of a point that has no cell
#define CF_RINGS 6                            // dense table: shells 0..6 (13^3 cells at most, one independent 4-byte read each), then the box scan
#define CF_RINGS_SPARSE 2                     // binary search per cell, ~20 dependent reads each: shells 0..2 (5^3 cells), then the box scan
#define CF_CHUNK 256                          // sorted targets per bounding box of the box scan
#define CF_DENSE_MIN 4096u
#define CF_STAT_BLOCKS 1024u

struct CfGrid {                               // written by k_np_grid, read by everything after it
    double mn[3], h, inv_h;
    int32_t n[3];
    uint32_t dense, Tf, pad_;
};
struct CfView {
    const CfGrid* grid;
    const uint32_t* nruns;                    // device count of the occupied cells
    const unsigned long long* ukey;           // [nruns] ascending
    const uint32_t* ustart;                   // [nruns] first sorted target of the run
    const uint32_t* dense;                    // [dense_cap] run + 1, 0 = empty
    const uint4* sorted;                      // [T] {x, y, z bits, target index} in key order
    const float* box;                         // [chunks][6] min xyz, max xyz
};

__device__ __forceinline__ uint32_t cf_fold(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }      // float bits -> unsigned order
__device__ __forceinline__ uint32_t cf_unfold(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
__device__ __forceinline__ bool cf_finite3(float x, float y, float z) { return x - x == 0.f && y - y == 0.f && z - z == 0.f; }
__device__ __forceinline__ float cf_d2(float tx, float ty, float tz, float qx, float qy, float qz)
{
    const float dx = tx - qx, dy = ty - qy, dz = tz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ uint32_t cf_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------ the grid
// bb[0..2] = max of ~fold(x) (the complement of the minimum), bb[3..5] = max of fold(x), bb[6] = finite targets; zero on entry
__global__ void __launch_bounds__(CF_BLOCK) k_np_bbox(const float* __restrict__ pts, uint32_t T, uint32_t* __restrict__ bb)
{
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u}, cnt = 0u;
    for (uint32_t i = blockIdx.x * CF_BLOCK + threadIdx.x; i < T; i += gridDim.x * CF_BLOCK) {
        const float p[3] = { pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2] };
        if (!cf_finite3(p[0], p[1], p[2])) continue;
        cnt++;
#pragma unroll
        for (int a = 0; a < 3; a++) { const uint32_t f = cf_fold(__float_as_uint(p[a] + 0.f)); lo[a] = max(lo[a], ~f); hi[a] = max(hi[a], f); }      // + 0.f: -0 counts as +0
    }
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = cf_wave_max(lo[a]); hi[a] = cf_wave_max(hi[a]); }
    cnt = wave_sum(cnt);
    __shared__ uint32_t red[4][7];                        // one set of atomics per workgroup: they all meet at seven words
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
        red[threadIdx.x >> 6][6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 7u) {
        const uint32_t t = threadIdx.x;
        if (t < 6u) { const uint32_t m = max(max(red[0][t], red[1][t]), max(red[2][t], red[3][t])); if (m) atomicMax(bb + t, m); }
        else { const uint32_t c = (red[0][6] + red[1][6]) + (red[2][6] + red[3][6]); if (c) atomicAdd(bb + 6, c); }
    }
}

// the cell-size rule, float64: a surface sampled evenly in a box of extents e has about one sample per cell of
// h = sqrt((ex ey + ey ez + ez ex) / Tf); a line, emax / Tf; a point, 1
__global__ void __launch_bounds__(64) k_np_grid(const uint32_t* __restrict__ bb, float max_dist, uint32_t dense_cap, CfGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    const uint32_t Tf = bb[6];
    g->Tf = Tf; g->dense = 0u; g->pad_ = 0u;
    if (Tf == 0u) { for (int a = 0; a < 3; a++) { g->mn[a] = 0.0; g->n[a] = 0; } g->h = 1.0; g->inv_h = 1.0; return; }
    double e[3], emax = 0.0;
    for (int a = 0; a < 3; a++) {
        const double mn = (double)__uint_as_float(cf_unfold(~bb[a])), mx = (double)__uint_as_float(cf_unfold(bb[3 + a]));
        g->mn[a] = mn; e[a] = mx - mn; emax = fmax(emax, e[a]);
    }
    const double A = (e[0] * e[1] + e[1] * e[2]) + e[2] * e[0];
    double h = A > 0.0 ? sqrt(A / (double)Tf) : (emax > 0.0 ? emax / (double)Tf : 1.0);
    if (max_dist >= 0.f && h < (double)max_dist) h = (double)max_dist;
    if (h < emax / 1048576.0) h = emax / 1048576.0;
    if (!(h > 0.0) || !(h < 1.0e300)) h = 1.0;
    double inv_h = 1.0 / h;
    if (!(inv_h < 1.0e300)) { h = 1.0; inv_h = 1.0; }      // a subnormal extent: one cell
    g->h = h; g->inv_h = inv_h;
    unsigned long long cells = 1ull;
    for (int a = 0; a < 3; a++) {
        const double c = fmin(floor(e[a] * inv_h) + 1.0, (double)CF_AXIS_MAX);
        g->n[a] = (int32_t)c;
        cells *= (unsigned long long)g->n[a];               // <= 2^63
    }
    g->dense = cells <= (unsigned long long)dense_cap ? 1u : 0u;
}

// the cell of coordinate x on axis a: monotone in x, defined for every finite x (n[a] >= 1)
__device__ __forceinline__ int32_t cf_cell(const CfGrid& g, int a, double x)
{
    const double v = floor((x - g.mn[a]) * g.inv_h);
    return (int32_t)fmin(fmax(v, 0.0), (double)(g.n[a] - 1));
}
// A lower bound (>= 0) of |x_t - q| along axis a for every target whose cell index on that axis is >= j (j > cq) or <= j (j < cq); 0 for j == cq.
// cell(x) >= j means (x - mn) * inv_h >= j up to two roundings of 2^-53, cell(x) <= j means it is < j + 1: the plane mn + j h (or mn + (j + 1) h)
// lies between, the slack covers the roundings of plane and difference a thousandfold.
__device__ __forceinline__ double cf_gap(const CfGrid& g, int a, int32_t j, int32_t cq, double q)
{
    if (j == cq) return 0.0;
    const double off = (double)(j > cq ? j : j + 1) * g.h, plane = g.mn[a] + off;
    const double d = j > cq ? plane - q : q - plane;
    return fmax(d - 1.0e-12 * ((fabs(g.mn[a]) + fabs(off)) + fabs(q)), 0.0);
}
// nothing at a squared distance of lb2 or more can replace or tie the limit
__device__ __forceinline__ bool cf_beyond(float lim, double lb2) { return (double)lim < lb2 * (1.0 - 1.0e-6) - 1.0e-36; }

__global__ void __launch_bounds__(CF_BLOCK) k_np_keys(const float* __restrict__ pts, uint32_t T, const CfGrid* __restrict__ gp, uint32_t* __restrict__ key_lo,
                                                      uint32_t* __restrict__ key_hi, uint32_t* __restrict__ sort_lo)
{
    const uint32_t i = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= T) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    uint32_t lo = CF_BAD, hi = CF_BAD;
    if (cf_finite3(x, y, z) && gp->Tf > 0u) {
        const CfGrid& g = *gp;
        const unsigned long long k = (unsigned long long)cf_cell(g, 0, (double)x) | ((unsigned long long)cf_cell(g, 1, (double)y) << CF_AXIS_BITS) |
                                     ((unsigned long long)cf_cell(g, 2, (double)z) << (2 * CF_AXIS_BITS));
        lo = (uint32_t)k; hi = (uint32_t)(k >> 32);
    }
    key_lo[i] = lo; key_hi[i] = hi; sort_lo[i] = lo;
}

// the heads of the runs of equal keys among the first Tf places: ustart[r] = the place, ukey[r] = the key
struct CfRunOp {
    const CfGrid* grid; const uint32_t *khi, *order, *key_lo; uint32_t* ustart; unsigned long long* ukey;
    __device__ unsigned long long key(uint32_t i) const { return gsr_sort_key64(khi, order, key_lo, i); }
    __device__ bool keep(uint32_t i) const { return i < grid->Tf && (i == 0u || key(i) != key(i - 1u)); }
    __device__ void place(uint32_t i, uint32_t p) const { ustart[p] = i; ukey[p] = key(i); }
};

__global__ void __launch_bounds__(CF_BLOCK) k_np_dense(CfView v, uint32_t T, uint32_t dense_cap, uint32_t* __restrict__ dense)
{
    const uint32_t r = blockIdx.x * CF_BLOCK + threadIdx.x;
    const CfGrid& g = *v.grid;
    if (!g.dense || r >= min(*v.nruns, T)) return;
    const unsigned long long k = v.ukey[r];
    const unsigned long long ix = k & (CF_AXIS_MAX - 1), iy = (k >> CF_AXIS_BITS) & (CF_AXIS_MAX - 1), iz = k >> (2 * CF_AXIS_BITS);
    const unsigned long long c = (iz * (unsigned long long)g.n[1] + iy) * (unsigned long long)g.n[0] + ix;
    if (c < dense_cap) dense[c] = r + 1u;
}

// sorted[i] and the bounding box of every chunk of CF_CHUNK places over the finite targets
__global__ void __launch_bounds__(CF_CHUNK) k_np_gather(const float* __restrict__ pts, uint32_t T, const CfGrid* __restrict__ gp, const uint32_t* __restrict__ order,
                                                        uint4* __restrict__ sorted, float* __restrict__ box)
{
    __shared__ uint32_t red[4][6];
    const uint32_t i = blockIdx.x * CF_CHUNK + threadIdx.x;
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    if (i < T) {
        const uint32_t src = min(order[i], T - 1u);
        const float p[3] = { pts[3 * (size_t)src], pts[3 * (size_t)src + 1], pts[3 * (size_t)src + 2] };
        sorted[i] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), src);
        if (i < gp->Tf) {
#pragma unroll
            for (int a = 0; a < 3; a++) { const uint32_t f = cf_fold(__float_as_uint(p[a])); lo[a] = ~f; hi[a] = f; }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = cf_wave_max(lo[a]); hi[a] = cf_wave_max(hi[a]); }
    if ((threadIdx.x & 63u) == 0u) for (int a = 0; a < 3; a++) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6u) {
        const uint32_t m = max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x]));
        box[6 * (size_t)blockIdx.x + threadIdx.x] = __uint_as_float(cf_unfold(threadIdx.x < 3u ? ~m : m));
    }
}

// ------------------------------------------------------------------------------------------------ the query
struct CfBest { float d2; int32_t idx; };
__device__ __forceinline__ void cf_try(CfBest& b, float md2, float d2, uint32_t idx)
{
    if (d2 <= md2 && (d2 < b.d2 || (d2 == b.d2 && idx < (uint32_t)b.idx))) { b.d2 = d2; b.idx = (int32_t)idx; }
}
__device__ __forceinline__ void cf_scan(const CfView& v, uint32_t b, uint32_t e, float qx, float qy, float qz, float md2, CfBest& best)
{
    for (uint32_t i = b; i < e; i++) {
        const uint4 t = v.sorted[i];
        cf_try(best, md2, cf_d2(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), qx, qy, qz), t.w);
    }
}
// the places [*b, *e) of cell (ix, iy, iz); false = empty
__device__ __forceinline__ bool cf_cell_range(const CfView& v, const CfGrid& g, uint32_t nruns, int32_t ix, int32_t iy, int32_t iz, uint32_t* b, uint32_t* e)
{
    uint32_t r;
    if (g.dense) {
        r = v.dense[((size_t)iz * (size_t)g.n[1] + (size_t)iy) * (size_t)g.n[0] + (size_t)ix];
        if (r == 0u || r > nruns) return false;
        r -= 1u;
    } else {
        const unsigned long long key = (unsigned long long)ix | ((unsigned long long)iy << CF_AXIS_BITS) | ((unsigned long long)iz << (2 * CF_AXIS_BITS));
        uint32_t lo = 0u, hi = nruns;                     // the first run whose key is >= key
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (v.ukey[mid] < key) lo = mid + 1u; else hi = mid; }
        if (lo >= nruns || v.ukey[lo] != key) return false;
        r = lo;
    }
    *b = v.ustart[r];
    *e = r + 1u < nruns ? v.ustart[r + 1u] : g.Tf;
    return true;
}

// ---- the box scan, by a whole wave for one query at a time.  (d2, index) travels as one 64-bit key, d2's bit pattern above the index: d2 >= +0 orders
// as an unsigned integer and index -1 is the largest, so the smaller key is the better candidate under cf_try's rule and "none" is the largest key.
__device__ __forceinline__ unsigned long long cf_key(float d2, uint32_t idx) { return ((unsigned long long)__float_as_uint(d2) << 32) | idx; }
__device__ __forceinline__ float cf_key_d2(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ unsigned long long cf_wave_min64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
// squared distance from q to the bounding box of chunk ch, a lower bound for every target in it
__device__ __forceinline__ double cf_box_lb2(const float* __restrict__ box, uint32_t ch, const double (&q)[3])
{
    const float* bx = box + 6 * (size_t)ch;
    double lb2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) { const double d = fmax(fmax((double)bx[a] - q[a], q[a] - (double)bx[3 + a]), 0.0); lb2 += d * d; }
    return lb2;
}
// every lane of the wave takes every 64th target of chunk ch; the wave's best key comes back in every lane
__device__ __forceinline__ unsigned long long cf_chunk_scan(const CfView& v, uint32_t ch, uint32_t Tf, uint32_t lane, float qx, float qy, float qz, float md2, unsigned long long key)
{
    const uint32_t end = min(Tf, (ch + 1u) * CF_CHUNK);
    for (uint32_t i = ch * CF_CHUNK + lane; i < end; i += 64u) {
        const uint4 t = v.sorted[i];
        const float d2 = cf_d2(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), qx, qy, qz);
        if (d2 <= md2) { const unsigned long long c = cf_key(d2, t.w); key = c < key ? c : key; }
    }
    return cf_wave_min64(key);
}
// Called by all 64 lanes.  Pass 1 finds the chunk whose box is nearest and scans it: its best is about the true distance.  Pass 2 scans the chunks
// whose boxes that best does not rule out (the strict rule of cf_beyond, re-tested against the best as it tightens).  2 Tf / 256 / 64 box tests per lane.
__device__ __forceinline__ unsigned long long cf_box_scan(const CfView& v, uint32_t Tf, uint32_t lane, float qx, float qy, float qz, float md2, unsigned long long key)
{
    const uint32_t chunks = gsr_div_up(Tf, CF_CHUNK);
    const double q[3] = { (double)qx, (double)qy, (double)qz };
    double mlb = 1.0e308;
    uint32_t mch = 0xFFFFFFFFu;
    for (uint32_t ch = lane; ch < chunks; ch += 64u) { const double lb2 = cf_box_lb2(v.box, ch, q); if (lb2 < mlb) { mlb = lb2; mch = ch; } }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                   // (lb2, chunk) is a total order: every lane ends with the same pair
        const double olb = __shfl_xor(mlb, d, 64); const uint32_t och = (uint32_t)__shfl_xor((int)mch, d, 64);
        if (olb < mlb || (olb == mlb && och < mch)) { mlb = olb; mch = och; }
    }
    if (mch >= chunks) return key;                        // no chunk at all (Tf == 0)
    key = cf_chunk_scan(v, mch, Tf, lane, qx, qy, qz, md2, key);
    for (uint32_t base = 0; base < chunks; base += 64u) {
        const uint32_t ch = base + lane;
        const bool hit = ch < chunks && ch != mch && !cf_beyond(fminf(cf_key_d2(key), md2), cf_box_lb2(v.box, ch, q));
        unsigned long long hits = __ballot(hit);
        while (hits) {                                    // wave-uniform
            const uint32_t c = base + (uint32_t)(__ffsll((long long)hits) - 1);
            hits &= hits - 1ull;
            if (cf_beyond(fminf(cf_key_d2(key), md2), cf_box_lb2(v.box, c, q))) continue;
            key = cf_chunk_scan(v, c, Tf, lane, qx, qy, qz, md2, key);
        }
    }
    return key;
}

// No lane leaves early: the box scan at the end is the whole wave's work.
// skip (nullable): a device word; non-zero = every workgroup returns at once and leaves its outputs alone (the launches an ICP enqueued past its stop).
__global__ void __launch_bounds__(CF_BLOCK) k_np_query(const float* __restrict__ query, uint32_t Q, CfView v, float md2, float* __restrict__ d2_out, int32_t* __restrict__ idx_out,
                                                       const uint32_t* __restrict__ skip)
{
    if (skip && *skip) return;                            // uniform over the launch
    const uint32_t qi = blockIdx.x * CF_BLOCK + threadIdx.x;
    const bool valid = qi < Q;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) { qx = query[3 * (size_t)qi]; qy = query[3 * (size_t)qi + 1]; qz = query[3 * (size_t)qi + 2]; }
    CfBest best = { __uint_as_float(0x7F800000u), -1 };
    const CfGrid& g = *v.grid;
    bool fallback = false;
    if (valid && cf_finite3(qx, qy, qz) && g.Tf > 0u) {
        const uint32_t nruns = min(*v.nruns, g.Tf);
        const double q[3] = { (double)qx, (double)qy, (double)qz };
        const int32_t c[3] = { cf_cell(g, 0, q[0]), cf_cell(g, 1, q[1]), cf_cell(g, 2, q[2]) };
        bool done = false;
        const int32_t rings = g.dense ? CF_RINGS : CF_RINGS_SPARSE;
        for (int32_t k = 0; k <= rings && !done; k++) {
            const int32_t z0 = max(c[2] - k, 0), z1 = min(c[2] + k, g.n[2] - 1), y0 = max(c[1] - k, 0), y1 = min(c[1] + k, g.n[1] - 1);
            for (int32_t iz = z0; iz <= z1; iz++) {
                const double gz = cf_gap(g, 2, iz, c[2], q[2]);
                for (int32_t iy = y0; iy <= y1; iy++) {
                    const double gy = cf_gap(g, 1, iy, c[1], q[1]), gyz = gz * gz + gy * gy;
                    if (cf_beyond(fminf(best.d2, md2), gyz)) continue;
                    const bool shell = abs(iz - c[2]) == k || abs(iy - c[1]) == k;      // the whole row belongs to shell k, else only its two ends
                    const int32_t step = shell ? 1 : 2 * k;
                    for (int32_t ix = c[0] - k; ix <= c[0] + k; ix += step) {
                        if (ix < 0 || ix >= g.n[0]) continue;
                        const double gx = cf_gap(g, 0, ix, c[0], q[0]);
                        if (cf_beyond(fminf(best.d2, md2), gyz + gx * gx)) continue;
                        uint32_t b, e;
                        if (cf_cell_range(v, g, nruns, ix, iy, iz, &b, &e)) cf_scan(v, b, e, qx, qy, qz, md2, best);
                    }
                }
            }
            // what lies beyond shell k: per axis and side the cells from c + k + 1 up / c - k - 1 down, if the grid has any
            double r = 1.0e300;
            bool more = false;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (c[a] + k + 1 <= g.n[a] - 1) { more = true; r = fmin(r, cf_gap(g, a, c[a] + k + 1, c[a], q[a])); }
                if (c[a] - k - 1 >= 0) { more = true; r = fmin(r, cf_gap(g, a, c[a] - k - 1, c[a], q[a])); }
            }
            done = !more || cf_beyond(fminf(best.d2, md2), r * r);
        }
        fallback = !done;
    }
    unsigned long long need = __ballot(fallback);         // every lane of the wave is here
    const uint32_t lane = lane_id();
    while (need) {                                        // wave-uniform: one query of the wave at a time
        const int src = __ffsll((long long)need) - 1;
        need &= need - 1ull;
        const float sx = __shfl(qx, src, 64), sy = __shfl(qy, src, 64), sz = __shfl(qz, src, 64);
        const unsigned long long k0 = cf_key(__shfl(best.d2, src, 64), (uint32_t)__shfl(best.idx, src, 64));
        const unsigned long long k1 = cf_box_scan(v, g.Tf, lane, sx, sy, sz, md2, k0);
        if ((int)lane == src) { best.d2 = cf_key_d2(k1); best.idx = (int32_t)(uint32_t)k1; }
    }
    if (valid) { d2_out[qi] = best.d2; idx_out[qi] = best.idx; }
}

__global__ void __launch_bounds__(CF_BLOCK) k_np_none(uint32_t Q, float* __restrict__ d2_out, int32_t* __restrict__ idx_out, const uint32_t* __restrict__ skip)
{
    if (skip && *skip) return;
    const uint32_t qi = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (qi >= Q) return;
    d2_out[qi] = __uint_as_float(0x7F800000u);
    idx_out[qi] = -1;
}

struct NpScratch {
    GsrSortBuf so; uint32_t *key_lo, *key_hi, *bb, *nruns, *sums, *ustart, *dense; CfGrid* grid; unsigned long long* ukey; uint4* sorted; float* box;
    uint32_t dense_cap; size_t bytes;
};
static uint32_t np_dense_cap(uint64_t T) { const uint64_t c = 4 * T; return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c, CF_DENSE_MIN), 1ull << 30); }
static NpScratch np_carve(uint64_t T, const void* base)
{
    NpScratch m; GsrCarve c(base);
    const size_t n = T > 0 ? T : 1;
    m.bb = c.take<uint32_t>(64);                          // bb[0..6], nruns at word 8: one clear
    m.nruns = m.bb + 8;
    m.grid = c.take<CfGrid>(1);
    m.so = gsr_sort_carve(c, n); m.key_lo = c.take<uint32_t>(n); m.key_hi = c.take<uint32_t>(n);
    m.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    m.ustart = c.take<uint32_t>(n); m.ukey = c.take<unsigned long long>(n);
    m.sorted = c.take<uint4>(n); m.box = c.take<float>(6 * ((n + CF_CHUNK - 1) / CF_CHUNK));
    m.dense_cap = np_dense_cap(T);
    m.dense = c.take<uint32_t>(m.dense_cap);
    m.bytes = c.bytes();
    return m;
}
static bool cf_count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }

static CfView np_view(const NpScratch& m) { return CfView{ m.grid, m.nruns, m.ukey, m.ustart, m.dense, m.sorted, m.box }; }

// ---- build and query (declared in gsr_common.h: gsr_register.hip builds the grid over a scan once and queries it per ICP iteration).  The scratch of
// a build holds everything a query reads -- grid, runs, dense table, the sorted copy of the targets and their boxes -- so the target array itself is
// not needed again.  T == 0 builds nothing and every query answers (+inf, -1).
size_t gsr_np_scratch_bytes(uint64_t T) { return np_carve(T, nullptr).bytes; }

int gsr_np_build(const char* who, const float* target, uint32_t T, float max_dist, void* scratch, hipStream_t s)
{
    if (T == 0) return 0;
    const NpScratch m = np_carve((uint64_t)T, scratch);
    const uint32_t gt = gsr_div_up(T, CF_BLOCK);
    if (gsr_memset_async(m.bb, 0, 256, s) || gsr_memset_async(m.dense, 0, (size_t)m.dense_cap * 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    hipLaunchKernelGGL(k_np_bbox, dim3(std::min(gsr_div_up(T, CF_BLOCK * 16u), 512u)), dim3(CF_BLOCK), 0, s, target, T, m.bb);
    hipLaunchKernelGGL(k_np_grid, dim3(1), dim3(64), 0, s, m.bb, max_dist, m.dense_cap, m.grid);
    hipLaunchKernelGGL(k_np_keys, dim3(gt), dim3(CF_BLOCK), 0, s, target, T, m.grid, m.key_lo, m.key_hi, m.so.ka);
    GsrSort st(m.so);                                     // the low word, then the high word
    if (st.sort(T, nullptr, 32, true, s) || gsr_sort_next_word(st, T, nullptr, GsrWordFromArray{m.key_hi}, s)) return 1;
    const CfView v = np_view(m);
    gsr_compact(CfRunOp{m.grid, st.keys, st.order, m.key_lo, m.ustart, m.ukey}, T, m.sums, m.nruns, s);
    hipLaunchKernelGGL(k_np_dense, dim3(gt), dim3(CF_BLOCK), 0, s, v, T, m.dense_cap, m.dense);
    hipLaunchKernelGGL(k_np_gather, dim3(gsr_div_up(T, CF_CHUNK)), dim3(CF_CHUNK), 0, s, target, T, m.grid, st.order, m.sorted, m.box);
    return 0;
}

// the cap is the cap of the build: the cell size was chosen with it
void gsr_np_query(const float* query, uint32_t Q, uint32_t T, float max_dist, const void* scratch, float* d2, int32_t* index, const uint32_t* skip, hipStream_t s)
{
    if (Q == 0) return;
    const uint32_t gq = gsr_div_up(Q, CF_BLOCK);
    if (T == 0) { hipLaunchKernelGGL(k_np_none, dim3(gq), dim3(CF_BLOCK), 0, s, Q, d2, index, skip); return; }
    const NpScratch m = np_carve((uint64_t)T, scratch);
    const float md2 = max_dist >= 0.f ? max_dist * max_dist : __builtin_inff();
    hipLaunchKernelGGL(k_np_query, dim3(gq), dim3(CF_BLOCK), 0, s, query, Q, np_view(m), md2, d2, index, skip);
}

extern "C" size_t gsr_nearest_points_scratch_bytes(int64_t n_query, int64_t n_target)
{
    if (!cf_count_ok(n_query) || !cf_count_ok(n_target)) return 0;
    return np_carve((uint64_t)n_target, nullptr).bytes;
}

extern "C" int gsr_nearest_points(const float* query, int64_t n_query, const float* target, int64_t n_target, float max_dist, float* d2, int32_t* index, void* scratch,
                                  size_t scratch_bytes, void* stream)
{
    const char* who = "nearest_points";
    if (!cf_count_ok(n_query) || !cf_count_ok(n_target)) { gsr_set_error("%s: %lld queries / %lld targets out of range [0, 2^31)", who, (long long)n_query, (long long)n_target); return 1; }
    if (max_dist != max_dist) { gsr_set_error("%s: max_dist is NaN (a negative value means none)", who); return 1; }
    if ((n_query > 0 && (!query || !d2 || !index)) || (n_target > 0 && !target)) { gsr_set_error("%s: null pointer", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, np_carve((uint64_t)n_target, nullptr).bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n_query == 0) return 0;                           // nobody asks: nothing is built
    if (gsr_np_build(who, target, (uint32_t)n_target, max_dist, scratch, s)) return 1;
    gsr_np_query(query, (uint32_t)n_query, (uint32_t)n_target, max_dist, scratch, d2, index, nullptr, s);
    return gsr_check_launch(who, s, false);
}

extern "C" size_t gsr_nearest_grid_scratch_bytes(int64_t n_target)
{
    if (!cf_count_ok(n_target)) return 0;
    return np_carve((uint64_t)n_target, nullptr).bytes;
}

extern "C" int gsr_nearest_grid_build(const float* target, int64_t n_target, float max_dist, void* scratch, size_t scratch_bytes, void* stream)
{
    const char* who = "nearest_grid_build";
    if (!cf_count_ok(n_target)) { gsr_set_error("%s: %lld targets out of range [0, 2^31)", who, (long long)n_target); return 1; }
    if (max_dist != max_dist) { gsr_set_error("%s: max_dist is NaN (a negative value means none)", who); return 1; }
    if (n_target > 0 && !target) { gsr_set_error("%s: null pointer", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, np_carve((uint64_t)n_target, nullptr).bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_np_build(who, target, (uint32_t)n_target, max_dist, scratch, s)) return 1;
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_nearest_grid_query(const float* query, int64_t n_query, int64_t n_target, float max_dist, const void* scratch, size_t scratch_bytes, float* d2,
                                      int32_t* index, const uint32_t* skip_dev, void* stream)
{
    const char* who = "nearest_grid_query";
    if (!cf_count_ok(n_query) || !cf_count_ok(n_target)) { gsr_set_error("%s: %lld queries / %lld targets out of range [0, 2^31)", who, (long long)n_query, (long long)n_target); return 1; }
    if (max_dist != max_dist) { gsr_set_error("%s: max_dist is NaN (a negative value means none)", who); return 1; }
    if (n_query > 0 && (!query || !d2 || !index)) { gsr_set_error("%s: null pointer", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, np_carve((uint64_t)n_target, nullptr).bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    gsr_np_query(query, (uint32_t)n_query, (uint32_t)n_target, max_dist, scratch, d2, index, skip_dev, s);
    return gsr_check_launch(who, s, false);
}

// ------------------------------------------------------------------------------------------------ surface samples
#define SS_BLOCK 1024
#define SS_R_STATUS 0
#define SS_R_TOTAL 2                          // 64 bits: words 2, 3

struct SsArgs { const float* verts; const int32_t* tris; uint32_t V, T; double spacing; };

// n of triangle t; 0 with *err set where it has none
__device__ __forceinline__ uint32_t ss_n(const SsArgs& a, uint32_t t, int32_t* i, uint32_t* err)
{
    i[0] = a.tris[3 * (size_t)t]; i[1] = a.tris[3 * (size_t)t + 1]; i[2] = a.tris[3 * (size_t)t + 2];
    if ((uint32_t)i[0] >= a.V || (uint32_t)i[1] >= a.V || (uint32_t)i[2] >= a.V) { *err |= GSR_CHAMFER_ERR_INDEX; return 0u; }
    const float* p0 = a.verts + 3 * (size_t)i[0]; const float* p1 = a.verts + 3 * (size_t)i[1]; const float* p2 = a.verts + 3 * (size_t)i[2];
    const float L2 = fmaxf(fmaxf(cf_d2(p1[0], p1[1], p1[2], p0[0], p0[1], p0[2]), cf_d2(p2[0], p2[1], p2[2], p1[0], p1[1], p1[2])),
                           cf_d2(p0[0], p0[1], p0[2], p2[0], p2[1], p2[2]));
    const double n = ceil(sqrt((double)L2) / a.spacing);
    if (n > (double)GSR_SAMPLE_MAX_N) { *err |= GSR_CHAMFER_ERR_CAP; return 0u; }
    return n >= 1.0 ? (uint32_t)n : 1u;
}

// offs[t] = samples of the triangles in front of t inside its block of SS_BLOCK, sums[block] = the block's samples (<= 2^30), record: status, total
__global__ void __launch_bounds__(SS_BLOCK) k_ss_count(SsArgs a, uint32_t* __restrict__ offs, uint32_t* __restrict__ sums, uint32_t* __restrict__ record)
{
    __shared__ uint32_t lds[17];
    const uint32_t t = blockIdx.x * SS_BLOCK + threadIdx.x;
    uint32_t cnt = 0u, err = 0u;
    if (t < a.T) { int32_t i[3]; const uint32_t n = ss_n(a, t, i, &err); cnt = n * n; }
    uint32_t tot;
    const uint32_t ex = block_excl_scan(cnt, lds, &tot);
    if (t < a.T) offs[t] = ex;
    if (err) atomicOr(record + SS_R_STATUS, err);
    if (threadIdx.x == 0) { sums[blockIdx.x] = tot; atomicAdd((unsigned long long*)(record + SS_R_TOTAL), (unsigned long long)tot); }
}

__global__ void __launch_bounds__(CF_BLOCK) k_ss_emit(SsArgs a, uint32_t total, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ sums, uint32_t nblk,
                                                      float* __restrict__ out)
{
    const uint32_t j = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (j >= total) return;
    uint32_t lo = 0u, hi = nblk;                          // the last block whose exclusive prefix is <= j
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (sums[mid] <= j) lo = mid; else hi = mid; }
    const uint32_t jb = j - sums[lo];
    uint32_t t0 = lo * SS_BLOCK, t1 = min(a.T, t0 + SS_BLOCK);      // the last triangle of the block whose prefix is <= jb (every triangle has a sample)
    while (t1 - t0 > 1u) { const uint32_t mid = t0 + ((t1 - t0) >> 1); if (offs[mid] <= jb) t0 = mid; else t1 = mid; }
    int32_t i[3]; uint32_t err = 0u;
    const uint32_t n = ss_n(a, t0, i, &err), m = jb - offs[t0];
    if (n == 0u || m >= n * n) return;                    // the count refused this mesh: nothing to write
    const uint32_t rem = n * n - m;                       // row r starts at r (2n - r) = n^2 - (n - r)^2: n - r = the smallest k with k^2 >= rem
    uint32_t k = (uint32_t)ceil(sqrt((double)rem));
    while (k * k < rem) k++;
    while (k > 1u && (k - 1u) * (k - 1u) >= rem) k--;
    const uint32_t r = n - k, pos = m - r * (2u * n - r);
    const bool up = pos < k;
    const double third = up ? 1.0 / 3.0 : 2.0 / 3.0, dn = (double)n;
    const double u = ((double)r + third) / dn, w = ((double)(up ? pos : pos - k) + third) / dn;
    const float* pa = a.verts + 3 * (size_t)i[0]; const float* pb = a.verts + 3 * (size_t)i[1]; const float* pc = a.verts + 3 * (size_t)i[2];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const double A = (double)pa[ax], B = (double)pb[ax], Cc = (double)pc[ax];
        out[3 * (size_t)j + ax] = (float)((A + u * (B - A)) + w * (Cc - A));
    }
}

struct SsScratch { uint32_t *offs, *sums, *word; size_t bytes; };
static SsScratch ss_carve(uint64_t T, const void* base)
{
    SsScratch m; GsrCarve c(base);
    const size_t n = T > 0 ? T : 1;
    m.offs = c.take<uint32_t>(n); m.sums = c.take<uint32_t>((n + SS_BLOCK - 1) / SS_BLOCK + 1); m.word = c.take<uint32_t>(16);
    m.bytes = c.bytes();
    return m;
}
static int ss_args(const char* who, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, double spacing)
{
    if (!cf_count_ok(T) || V < 0 || V > 0x7FFFFFFFll) { gsr_set_error("%s: %lld triangles / %lld vertices out of range", who, (long long)T, (long long)V); return 1; }
    if (!(spacing > 0.0) || !(spacing < 1.0e300)) { gsr_set_error("%s: spacing must be a positive finite number", who); return 1; }
    if (T > 0 && (!triangles || (V > 0 && !vertices))) { gsr_set_error("%s: null pointer", who); return 1; }
    return 0;
}
extern "C" size_t gsr_sample_surface_scratch_bytes(int64_t n_triangles)
{
    if (!cf_count_ok(n_triangles)) return 0;
    return ss_carve((uint64_t)n_triangles, nullptr).bytes;
}
extern "C" int gsr_sample_surface_count(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double spacing, void* scratch,
                                        size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "sample_surface_count";
    if (ss_args(who, vertices, n_vertices, triangles, n_triangles, spacing)) return 1;
    if (!record_dev) { gsr_set_error("%s: null record", who); return 1; }
    const SsScratch m = ss_carve((uint64_t)n_triangles, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(record_dev, 0, 16, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (n_triangles == 0) return gsr_check_launch(who, s, false);
    const SsArgs a = { vertices, triangles, (uint32_t)n_vertices, (uint32_t)n_triangles, spacing };
    const uint32_t nblk = gsr_div_up(a.T, SS_BLOCK);
    hipLaunchKernelGGL(k_ss_count, dim3(nblk), dim3(SS_BLOCK), 0, s, a, m.offs, m.sums, record_dev);
    gsr_scan_small(m.sums, nblk, 1, 0, m.word, nullptr, s);
    return gsr_check_launch(who, s, false);
}
extern "C" int gsr_sample_surface_emit(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double spacing, const void* scratch,
                                       size_t scratch_bytes, int64_t total, float* points, void* stream)
{
    const char* who = "sample_surface_emit";
    if (ss_args(who, vertices, n_vertices, triangles, n_triangles, spacing)) return 1;
    if (!cf_count_ok(total)) { gsr_set_error("%s: %lld samples out of range [0, 2^31)", who, (long long)total); return 1; }
    const SsScratch m = ss_carve((uint64_t)n_triangles, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    if (total == 0) return 0;
    if (n_triangles == 0 || !points) { gsr_set_error("%s: samples without triangles, or a null output", who); return 1; }
    const SsArgs a = { vertices, triangles, (uint32_t)n_vertices, (uint32_t)n_triangles, spacing };
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ss_emit, dim3(gsr_div_up((uint32_t)total, CF_BLOCK)), dim3(CF_BLOCK), 0, s, a, (uint32_t)total, m.offs, m.sums, gsr_div_up(a.T, SS_BLOCK), points);
    return gsr_check_launch(who, s, false);
}

// ------------------------------------------------------------------------------------------------ voxel thinning
#define VD_HALF 1048576.0                     // cells per axis: [-2^20, 2^20)

__global__ void __launch_bounds__(CF_BLOCK) k_vd_keys(const float* __restrict__ pts, uint32_t N, double cell, uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi,
                                                      uint32_t* __restrict__ sort_lo, uint32_t* __restrict__ record)
{
    const uint32_t i = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float p[3] = { pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2] };
    uint32_t lo = CF_BAD, hi = CF_BAD;
    if (cf_finite3(p[0], p[1], p[2])) {
        unsigned long long k = 0ull;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double c = floor((double)p[a] / cell);
            if (!(c >= -VD_HALF && c < VD_HALF)) { ok = false; continue; }
            k |= (unsigned long long)(uint32_t)(int32_t)(c + VD_HALF) << (a * CF_AXIS_BITS);
        }
        if (ok) { lo = (uint32_t)k; hi = (uint32_t)(k >> 32); }
        else atomicOr(record, (uint32_t)GSR_CHAMFER_ERR_RANGE);
    }
    key_lo[i] = lo; key_hi[i] = hi; sort_lo[i] = lo;
}

// keep[point] = it leads the run of its cell in the sorted order (stable: it has the lowest index of the cell) and has a cell
__global__ void __launch_bounds__(CF_BLOCK) k_vd_flag(uint32_t N, const uint32_t* __restrict__ khi, const uint32_t* __restrict__ order, const uint32_t* __restrict__ key_lo,
                                                      uint8_t* __restrict__ keep)
{
    const uint32_t i = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= N) return;
    const uint32_t src = order[i];
    if (src >= N) return;
    const uint32_t hi = khi[i], lo = key_lo[src];
    bool head = !(hi == CF_BAD && lo == CF_BAD);
    if (head && i > 0u) { const uint32_t prev = order[i - 1u]; head = khi[i - 1u] != hi || (prev < N ? key_lo[prev] : CF_BAD) != lo; }
    keep[src] = head ? 1 : 0;
}

__global__ void __launch_bounds__(CF_BLOCK) k_vd_emit(const float* __restrict__ pts, uint32_t N, uint32_t n_kept, const uint32_t* __restrict__ map, float* __restrict__ out,
                                                      int32_t* __restrict__ index)
{
    const uint32_t j = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (j >= n_kept) return;
    const uint32_t src = map[j];
    if (src >= N) return;
    index[j] = (int32_t)src;
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * (size_t)j + a] = pts[3 * (size_t)src + a];
}

struct VdScratch { GsrSortBuf so; uint32_t *key_lo, *key_hi, *sums, *map; uint8_t* keep; size_t bytes; };
static VdScratch vd_carve(uint64_t N, const void* base)
{
    VdScratch m; GsrCarve c(base);
    const size_t n = N > 0 ? N : 1;
    m.so = gsr_sort_carve(c, n); m.key_lo = c.take<uint32_t>(n); m.key_hi = c.take<uint32_t>(n);
    m.sums = c.take<uint32_t>(gsr_compact_sums_words(n)); m.map = c.take<uint32_t>(n); m.keep = c.take<uint8_t>(n);
    m.bytes = c.bytes();
    return m;
}
extern "C" size_t gsr_voxel_downsample_scratch_bytes(int64_t n_points)
{
    if (!cf_count_ok(n_points)) return 0;
    return vd_carve((uint64_t)n_points, nullptr).bytes;
}
extern "C" int gsr_voxel_downsample_count(const float* points, int64_t n_points, double cell, void* scratch, size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "voxel_downsample_count";
    if (!cf_count_ok(n_points)) { gsr_set_error("%s: %lld points out of range [0, 2^31)", who, (long long)n_points); return 1; }
    if (!(cell > 0.0) || !(cell < 1.0e300)) { gsr_set_error("%s: the cell size must be a positive finite number", who); return 1; }
    if (!record_dev || (n_points > 0 && !points)) { gsr_set_error("%s: null pointer", who); return 1; }
    const VdScratch m = vd_carve((uint64_t)n_points, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(record_dev, 0, 8, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (n_points == 0) return gsr_check_launch(who, s, false);
    const uint32_t N = (uint32_t)n_points, g = gsr_div_up(N, CF_BLOCK);
    hipLaunchKernelGGL(k_vd_keys, dim3(g), dim3(CF_BLOCK), 0, s, points, N, cell, m.key_lo, m.key_hi, m.so.ka, record_dev);
    GsrSort st(m.so);
    if (st.sort(N, nullptr, 32, true, s) || gsr_sort_next_word(st, N, nullptr, GsrWordFromArray{m.key_hi}, s)) return 1;
    hipLaunchKernelGGL(k_vd_flag, dim3(g), dim3(CF_BLOCK), 0, s, N, st.keys, st.order, m.key_lo, m.keep);
    gsr_rows_keep_scan(m.keep, N, m.sums, m.map, nullptr, record_dev + 1, s);
    return gsr_check_launch(who, s, false);
}
extern "C" int gsr_voxel_downsample_emit(const float* points, int64_t n_points, const void* scratch, size_t scratch_bytes, int64_t n_kept, float* points_out,
                                         int32_t* index_out, void* stream)
{
    const char* who = "voxel_downsample_emit";
    if (!cf_count_ok(n_points) || n_kept < 0 || n_kept > n_points) { gsr_set_error("%s: %lld of %lld points out of range", who, (long long)n_kept, (long long)n_points); return 1; }
    const VdScratch m = vd_carve((uint64_t)n_points, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    if (n_kept == 0) return 0;
    if (!points || !points_out || !index_out) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vd_emit, dim3(gsr_div_up((uint32_t)n_kept, CF_BLOCK)), dim3(CF_BLOCK), 0, s, points, (uint32_t)n_points, (uint32_t)n_kept, m.map, points_out, index_out);
    return gsr_check_launch(who, s, false);
}

// ------------------------------------------------------------------------------------------------ statistics
struct StTau { double tau[GSR_CHAMFER_MAX_THRESHOLDS]; int32_t K; };

// thread t of block b adds elements (b * 256 + t) + i * blocks * 256 in ascending i; the block's sum is the butterfly per wave, then (w0 + w1) + (w2 + w3).
// partial[b] = the block's sum, below[k * CF_STAT_BLOCKS + b] = its elements under threshold k: no atomics, k_st_finish adds them up.
__global__ void __launch_bounds__(CF_BLOCK) k_st_partial(const float* __restrict__ d2, uint32_t Q, double max_dist, StTau tau, double* __restrict__ partial,
                                                         uint32_t* __restrict__ below_out)
{
    __shared__ double red[4];
    __shared__ uint32_t redc[4][GSR_CHAMFER_MAX_THRESHOLDS];
    double sum = 0.0;
    uint32_t below[GSR_CHAMFER_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < GSR_CHAMFER_MAX_THRESHOLDS; k++) below[k] = 0u;
    for (uint32_t i = blockIdx.x * CF_BLOCK + threadIdx.x; i < Q; i += gridDim.x * CF_BLOCK) {
        double d = sqrt((double)d2[i]);
        if (max_dist >= 0.0) d = fmin(d, max_dist);
        sum += d;
#pragma unroll
        for (int k = 0; k < GSR_CHAMFER_MAX_THRESHOLDS; k++) if (k < tau.K && d < tau.tau[k]) below[k]++;
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = sum;
#pragma unroll
    for (int k = 0; k < GSR_CHAMFER_MAX_THRESHOLDS; k++) {
        const uint32_t c = wave_sum(below[k]);
        if ((threadIdx.x & 63u) == 0u) redc[threadIdx.x >> 6][k] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (threadIdx.x < (uint32_t)tau.K) below_out[threadIdx.x * CF_STAT_BLOCKS + blockIdx.x] = (redc[0][threadIdx.x] + redc[1][threadIdx.x]) + (redc[2][threadIdx.x] + redc[3][threadIdx.x]);
}
// one block: thread t adds partials t, t + 256, ... in order, then as above; the counts likewise (integers: any order)
__global__ void __launch_bounds__(CF_BLOCK) k_st_finish(const double* __restrict__ partial, const uint32_t* __restrict__ below, uint32_t n, int32_t K, double* __restrict__ out,
                                                        unsigned long long* __restrict__ counts)
{
    __shared__ double red[4];
    __shared__ uint32_t redc[4][GSR_CHAMFER_MAX_THRESHOLDS];
    double sum = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += CF_BLOCK) sum += partial[i];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = sum;
    for (int32_t k = 0; k < K; k++) {                     // every count is at most n < 2^31
        uint32_t c = 0u;
        for (uint32_t i = threadIdx.x; i < n; i += CF_BLOCK) c += below[(uint32_t)k * CF_STAT_BLOCKS + i];
        c = wave_sum(c);
        if ((threadIdx.x & 63u) == 0u) redc[threadIdx.x >> 6][k] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
    if (threadIdx.x < (uint32_t)K) counts[threadIdx.x] = (unsigned long long)((redc[0][threadIdx.x] + redc[1][threadIdx.x]) + (redc[2][threadIdx.x] + redc[3][threadIdx.x]));
}
#define ST_SCRATCH_BYTES (gsr_align((size_t)CF_STAT_BLOCKS * 8) + gsr_align((size_t)CF_STAT_BLOCKS * 4 * GSR_CHAMFER_MAX_THRESHOLDS))
static uint32_t st_blocks(uint64_t Q) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((Q + CF_BLOCK * 8ull - 1) / (CF_BLOCK * 8ull), 1), CF_STAT_BLOCKS); }
extern "C" size_t gsr_distance_stats_scratch_bytes(int64_t n)
{
    if (!cf_count_ok(n)) return 0;
    return ST_SCRATCH_BYTES;
}
extern "C" int gsr_distance_stats(const float* d2, int64_t n, double max_dist, const double* thresholds, int32_t n_thresholds, void* record_dev, void* scratch,
                                  size_t scratch_bytes, void* stream)
{
    const char* who = "distance_stats";
    if (!cf_count_ok(n)) { gsr_set_error("%s: %lld distances out of range [0, 2^31)", who, (long long)n); return 1; }
    if (n_thresholds < 0 || n_thresholds > GSR_CHAMFER_MAX_THRESHOLDS || (n_thresholds > 0 && !thresholds)) {
        gsr_set_error("%s: %d thresholds, at most %d", who, n_thresholds, GSR_CHAMFER_MAX_THRESHOLDS); return 1;
    }
    if (max_dist != max_dist) { gsr_set_error("%s: max_dist is NaN (a negative value means none)", who); return 1; }
    if (!record_dev || (n > 0 && !d2)) { gsr_set_error("%s: null pointer", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, ST_SCRATCH_BYTES)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(record_dev, 0, 8 * (1 + GSR_CHAMFER_MAX_THRESHOLDS), s)) { gsr_set_error("%s: clear", who); return 1; }
    if (n == 0) return gsr_check_launch(who, s, false);
    StTau tau; tau.K = n_thresholds;
    for (int k = 0; k < GSR_CHAMFER_MAX_THRESHOLDS; k++) tau.tau[k] = k < n_thresholds ? thresholds[k] : 0.0;
    const uint32_t nb = st_blocks((uint64_t)n);
    double* partial = (double*)scratch;
    uint32_t* below = (uint32_t*)((char*)scratch + gsr_align((size_t)CF_STAT_BLOCKS * 8));
    hipLaunchKernelGGL(k_st_partial, dim3(nb), dim3(CF_BLOCK), 0, s, d2, (uint32_t)n, max_dist, tau, partial, below);
    hipLaunchKernelGGL(k_st_finish, dim3(1), dim3(CF_BLOCK), 0, s, (const double*)partial, (const uint32_t*)below, nb, n_thresholds, (double*)record_dev,
                       (unsigned long long*)record_dev + 1);
    return gsr_check_launch(who, s, false);
}
