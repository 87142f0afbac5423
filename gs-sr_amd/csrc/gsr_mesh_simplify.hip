// gsr_mesh_simplify.hip -- a welded triangle mesh made smaller on the device by vertex clustering: the role of Open3D's simplify_vertex_clustering
// after post_process_mesh.  Open3D is not part of the reference tree and nothing is held against it: the result is DEFINED in include/gsrast.h
// ("mesh simplification") and restated operation by operation in tests/simplify_truth.py.  Every output is a pure function of the
// arrays: no float atomics, two runs give the same bits.
//
//   bound       per-axis minimum of all V vertices by integer atomicMax on the complemented order-preserving bit pattern (as gsr_chamfer.hip);
//               origin = (double)lo - 0.5 voxel.
//   cells       c = floor(((double)v - origin) / voxel) per axis, inside [0, 2^21) or GSR_MESH_ERR_RANGE; key = cx | cy << 21 | cz << 42, sorted with the
//               vertex index as value by the stable sort on the low word, then on the high word (gsr_sort.h): the members of a cell stand in a run in
//               ascending vertex index, its head is the lowest member.
//   numbering   head flags in VERTEX order -> keep scan (gsr_rows_keep_scan): rank of a head = its new index, first[p] = the head of new vertex p.  The
//               heads in SORTED order -> gsr_compact: ustart[r].  One thread per run writes vertex_map of its members.  No second sort.
//   quadric     key of corner h = 3 t + corner: the new index of its vertex, sorted with h as value (stable: ascending (triangle, corner) inside a
//               cell); run heads by gsr_compact; one thread per cell adds the ten entries of its corners' triangle quadrics in that order and solves.
//   triangles   indices mapped, rotated smallest first (k_ms_rotate), equal triples found through an open-addressing table whose slot holds a triangle
//               of the triple -- the key of a slot is the triple of its owner, atomicCAS claims an empty slot, an integer atomicMin lowers the owner
//               within the triple (k_ms_insert); a kernel later a triangle stays iff it owns its slot (k_ms_tkeep).  Keep scan in original order.
//   emit        one thread per cell: float64 sums of positions and colours over the run, in ascending vertex index, divided by the count, rounded to
//               float32; the quadric position instead where the count pass accepted one.
// Termination: probe loops are capped at the table size; the per-cell loops run over a run of the sort; no kernel waits for another workgroup.
// Everything runs on the caller's stream; nothing synchronises.  Built without FMA contraction (PRE_FLAGS).
#include "gsr_common.h"
#include "gsr_scan.h"
#include "gsr_compact.h"
#include <algorithm>

#define MS_BLOCK 256
#define MS_AXIS_BITS 21
#define MS_AXIS_CELLS 2097152.0               // 2^21 cells per axis at most
#define MS_BAD 0xFFFFFFFFu                    // both key words of a vertex that has no cell; an empty table slot
// record words (include/gsrast.h)
#define MS_R_STATUS 0
#define MS_R_V 1
#define MS_R_T 2
#define MS_R_Q 3

__device__ __forceinline__ uint32_t ms_fold(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }      // float bits -> unsigned order
__device__ __forceinline__ uint32_t ms_unfold(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
__device__ __forceinline__ bool ms_finite(float x) { return x - x == 0.f; }
__device__ __forceinline__ bool ms_finite(double x) { return x - x == 0.0; }
__device__ __forceinline__ uint32_t ms_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
// origin = (double)lo - 0.5 voxel, lo read back from the complemented maxima
__device__ __forceinline__ void ms_origin(const uint32_t* __restrict__ bb, double voxel, double (&o)[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) o[a] = (double)__uint_as_float(ms_unfold(~bb[a])) - 0.5 * voxel;
}

// ------------------------------------------------------------------------------------------------ cells of the vertices
// bb[a] = max of ~fold(x) over the finite components of axis a (the complement of the minimum); zero on entry
__global__ void __launch_bounds__(MS_BLOCK) k_ms_bound(const float* __restrict__ verts, uint32_t V, uint32_t* __restrict__ bb, uint32_t* __restrict__ status)
{
    uint32_t lo[3] = {0u, 0u, 0u};
    bool bad = false;
    for (uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x; i < V; i += gridDim.x * MS_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float x = verts[3 * (size_t)i + a];
            if (ms_finite(x)) lo[a] = max(lo[a], ~ms_fold(__float_as_uint(x)));
            else bad = true;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = ms_wave_max(lo[a]);
        if (lane_id() == 0 && lo[a]) atomicMax(bb + a, lo[a]);
    }
    if (bad) atomicOr(status, (uint32_t)GSR_MESH_ERR_NONFINITE);
}

__global__ void __launch_bounds__(MS_BLOCK) k_ms_keys(const float* __restrict__ verts, uint32_t V, const uint32_t* __restrict__ bb, double voxel,
                                                      uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi, uint32_t* __restrict__ sort_lo,
                                                      uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= V) return;
    const float p[3] = { verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2] };
    uint32_t lo = MS_BAD, hi = MS_BAD;
    if (ms_finite(p[0]) && ms_finite(p[1]) && ms_finite(p[2])) {      // a non-finite component: k_ms_bound has said so
        double o[3];
        ms_origin(bb, voxel, o);
        unsigned long long k = 0ull;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double c = floor(((double)p[a] - o[a]) / voxel);
            if (!(c >= 0.0 && c < MS_AXIS_CELLS)) { ok = false; continue; }
            k |= (unsigned long long)(uint32_t)c << (a * MS_AXIS_BITS);
        }
        if (ok) { lo = (uint32_t)k; hi = (uint32_t)(k >> 32); }
        else atomicOr(status, (uint32_t)GSR_MESH_ERR_RANGE);
    }
    key_lo[i] = lo; key_hi[i] = hi; sort_lo[i] = lo;
}

// What the sort left, as every later kernel reads it: place i holds vertex order[i] with key (khi[i], key_lo[order[i]]) -- gsr_sort_key64, compared word by word with a bound on order[i]
struct MsRuns {
    const uint32_t *khi, *order, *key_lo; uint32_t V;
    __device__ bool head(uint32_t i) const
    {
        if (i == 0u) return true;
        const uint32_t a = order[i], b = order[i - 1u];
        return khi[i] != khi[i - 1u] || (a < V ? key_lo[a] : MS_BAD) != (b < V ? key_lo[b] : MS_BAD);
    }
};
// flag[vertex] = it leads the run of its cell (stable sort: it is the cell's lowest member);
// sorted[i] = the vertex at place i, where the emit call finds it whichever buffer the sort ended in
__global__ void __launch_bounds__(MS_BLOCK) k_ms_heads(MsRuns ru, uint8_t* __restrict__ flag, uint32_t* __restrict__ sorted)
{
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= ru.V) return;
    const uint32_t src = ru.order[i];
    sorted[i] = src;
    if (src < ru.V) flag[src] = ru.head(i) ? 1 : 0;
}
// the run heads in sorted order: ustart[r] = the place where run r begins
struct MsRunOp {
    MsRuns ru; uint32_t* ustart;
    __device__ bool keep(uint32_t i) const { return ru.head(i); }
    __device__ void place(uint32_t i, uint32_t p) const { ustart[p] = i; }
};
// one thread per cell: vertex_map of its members = the rank of its head
__global__ void __launch_bounds__(MS_BLOCK) k_ms_vmap(const uint32_t* __restrict__ order, uint32_t V, const uint32_t* __restrict__ n_cells, const uint32_t* __restrict__ ustart,
                                                      const uint32_t* __restrict__ rank, uint32_t* __restrict__ vmap)
{
    const uint32_t r = blockIdx.x * MS_BLOCK + threadIdx.x, nc = min(*n_cells, V);
    if (r >= nc) return;
    const uint32_t b = ustart[r], e = r + 1u < nc ? ustart[r + 1u] : V;
    if (b >= V) return;
    const uint32_t head = order[b];
    if (head >= V) return;
    const uint32_t p = rank[head];
    for (uint32_t i = b; i < e && i < V; i++) { const uint32_t v = order[i]; if (v < V) vmap[v] = p; }
}

// ------------------------------------------------------------------------------------------------ quadrics
__global__ void __launch_bounds__(MS_BLOCK) k_ms_corner_keys(const int32_t* __restrict__ tris, uint32_t H, uint32_t V, const uint32_t* __restrict__ vmap, uint32_t* __restrict__ keys)
{
    const uint32_t h = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (h >= H) return;
    const uint32_t i = (uint32_t)tris[h];
    keys[h] = i < V ? vmap[i] : 0u;               // an index out of range: k_ms_rotate reports it, its triangle contributes nothing
}
struct MsCornerRunOp {
    const uint32_t* keys; uint32_t* qstart;
    __device__ bool keep(uint32_t i) const { return i == 0u || keys[i] != keys[i - 1u]; }
    __device__ void place(uint32_t i, uint32_t p) const { qstart[p] = i; }
};

struct MsMesh { const float* verts; const int32_t* tris; uint32_t V, T; double voxel; };

// One thread per cell that has corners: Q = the sum of (L / 2) p p^T over its corners in ascending (triangle, corner), then A x = r by the adjugate
// over the determinant (include/gsrast.h writes the order of the operations down).  qflag is zero on entry.
__global__ void __launch_bounds__(MS_BLOCK) k_ms_quadric(MsMesh m, const uint32_t* __restrict__ bb, const uint32_t* __restrict__ n_runs, const uint32_t* __restrict__ qstart,
                                                         const uint32_t* __restrict__ ckey, const uint32_t* __restrict__ corder, const uint32_t* __restrict__ first,
                                                         const uint32_t* __restrict__ key_lo, const uint32_t* __restrict__ key_hi, float* __restrict__ qpos,
                                                         uint8_t* __restrict__ qflag, uint32_t* __restrict__ record)
{
    const uint32_t r = blockIdx.x * MS_BLOCK + threadIdx.x, H = 3u * m.T, nr = min(*n_runs, H), nv = min(record[MS_R_V], m.V);
    bool take = false;
    if (r < nr) {
        const uint32_t b = qstart[r], e = r + 1u < nr ? qstart[r + 1u] : H;
        const uint32_t p = b < H ? ckey[b] : MS_BAD;
        const uint32_t v0 = p < nv ? first[p] : MS_BAD;
        if (v0 < m.V) {
            double o[3];
            ms_origin(bb, m.voxel, o);
            double Q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint32_t i = b; i < e && i < H; i++) {
                const uint32_t h = corder[i];
                if (h >= H) continue;
                const uint32_t t = h / 3u;
                const int32_t ix[3] = { m.tris[3 * (size_t)t], m.tris[3 * (size_t)t + 1], m.tris[3 * (size_t)t + 2] };
                if ((uint32_t)ix[0] >= m.V || (uint32_t)ix[1] >= m.V || (uint32_t)ix[2] >= m.V) continue;
                double A[3], e1[3], e2[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    A[a] = (double)m.verts[3 * (size_t)ix[0] + a] - o[a];
                    e1[a] = ((double)m.verts[3 * (size_t)ix[1] + a] - o[a]) - A[a];
                    e2[a] = ((double)m.verts[3 * (size_t)ix[2] + a] - o[a]) - A[a];
                }
                const double N[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
                const double L = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
                if (!(L > 0.0) || !ms_finite(L)) continue;
                double pl[4] = { N[0] / L, N[1] / L, N[2] / L, 0.0 };
                pl[3] = -((pl[0] * A[0] + pl[1] * A[1]) + pl[2] * A[2]);
                const double w = L * 0.5;
                int k = 0;
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int c = a; c < 4; c++) Q[k++] += w * (pl[a] * pl[c]);      // 00 01 02 03 11 12 13 22 23 33
            }
            const double a00 = Q[0], a01 = Q[1], a02 = Q[2], a11 = Q[4], a12 = Q[5], a22 = Q[7];
            const double r0 = -Q[3], r1 = -Q[6], r2 = -Q[8];
            const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
            const double det = (a00 * c00 + a01 * c01) + a02 * c02;
            if (ms_finite(det) && det > 0.0) {
                const double x[3] = { ((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det };
                const unsigned long long key = ((unsigned long long)key_hi[v0] << 32) | key_lo[v0];
                take = true;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double c = (double)(uint32_t)((key >> (a * MS_AXIS_BITS)) & ((1u << MS_AXIS_BITS) - 1u));
                    if (!ms_finite(x[a]) || !(x[a] >= c * m.voxel && x[a] <= (c + 1.0) * m.voxel)) take = false;
                }
                if (take) {
#pragma unroll
                    for (int a = 0; a < 3; a++) qpos[3 * (size_t)p + a] = (float)(o[a] + x[a]);
                    qflag[p] = 1;
                }
            }
        }
    }
    const unsigned long long took = __ballot(take);       // one integer atomic per wave
    if (take && (int)lane_id() == __ffsll((long long)took) - 1) atomicAdd(record + MS_R_Q, (uint32_t)__popcll(took));
}

// ------------------------------------------------------------------------------------------------ triangles
__device__ __forceinline__ unsigned long long ms_mix(unsigned long long x)      // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ unsigned long long ms_hash3(const uint32_t* t) { return ms_mix(ms_mix(((unsigned long long)t[0] << 32) | t[1]) ^ t[2]); }

// rt[t] = the triple of new indices, the smallest first; live[t] = it has three distinct ones
__global__ void __launch_bounds__(MS_BLOCK) k_ms_rotate(const int32_t* __restrict__ tris, uint32_t T, uint32_t V, const uint32_t* __restrict__ vmap, uint32_t* __restrict__ rt,
                                                        uint8_t* __restrict__ live, uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t i[3] = { (uint32_t)tris[3 * (size_t)t], (uint32_t)tris[3 * (size_t)t + 1], (uint32_t)tris[3 * (size_t)t + 2] };
    uint32_t a = 0u, b = 0u, c = 0u;
    bool ok = false;
    if (i[0] >= V || i[1] >= V || i[2] >= V) atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX);
    else {
        a = vmap[i[0]]; b = vmap[i[1]]; c = vmap[i[2]];
        ok = a != b && b != c && c != a;
        if (b < a && b < c) { const uint32_t x = a; a = b; b = c; c = x; }
        else if (c < a && c < b) { const uint32_t x = c; c = b; b = a; a = x; }
    }
    rt[3 * (size_t)t] = a; rt[3 * (size_t)t + 1] = b; rt[3 * (size_t)t + 2] = c;
    live[t] = ok ? 1 : 0;
}

struct MsTable { uint32_t* owner; uint32_t mask; };       // mask = slots - 1; a slot holds one triangle of its triple, or MS_BAD
__device__ __forceinline__ bool ms_same(const uint32_t* __restrict__ rt, uint32_t t, const uint32_t* mine)
{
    return rt[3 * (size_t)t] == mine[0] && rt[3 * (size_t)t + 1] == mine[1] && rt[3 * (size_t)t + 2] == mine[2];
}
// at most `slots` probes.  The triple of a slot never changes once it is claimed: the owner is only ever lowered to a triangle of the same triple.
__global__ void __launch_bounds__(MS_BLOCK) k_ms_insert(const uint32_t* __restrict__ rt, const uint8_t* __restrict__ live, uint32_t T, MsTable tb, uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= T || !live[t]) return;
    const uint32_t mine[3] = { rt[3 * (size_t)t], rt[3 * (size_t)t + 1], rt[3 * (size_t)t + 2] };
    uint32_t h = (uint32_t)ms_hash3(mine) & tb.mask;
    for (uint32_t n = 0; n <= tb.mask; n++, h = (h + 1u) & tb.mask) {
        uint32_t cur = __hip_atomic_load(tb.owner + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MS_BAD) { cur = atomicCAS(tb.owner + h, MS_BAD, t); if (cur == MS_BAD) return; }
        if (cur < T && ms_same(rt, cur, mine)) { atomicMin(tb.owner + h, t); return; }
    }
    atomicOr(status, (uint32_t)GSR_MESH_ERR_INTERNAL);    // the table is full: cannot happen with slots >= 2 T
}
// keep[t] = t is the lowest triangle of its triple
__global__ void __launch_bounds__(MS_BLOCK) k_ms_tkeep(const uint32_t* __restrict__ rt, const uint8_t* __restrict__ live, uint32_t T, MsTable tb, uint8_t* __restrict__ keep,
                                                       uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= T) return;
    bool k = false;
    if (live[t]) {
        const uint32_t mine[3] = { rt[3 * (size_t)t], rt[3 * (size_t)t + 1], rt[3 * (size_t)t + 2] };
        uint32_t h = (uint32_t)ms_hash3(mine) & tb.mask;
        bool found = false;
        for (uint32_t n = 0; n <= tb.mask && !found; n++, h = (h + 1u) & tb.mask) {
            const uint32_t cur = tb.owner[h];
            if (cur == MS_BAD) break;
            if (cur < T && ms_same(rt, cur, mine)) { found = true; k = cur == t; }
        }
        if (!found) atomicOr(status, (uint32_t)GSR_MESH_ERR_INTERNAL);
    }
    keep[t] = k ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ emit
// one thread per cell: the float64 sums over its members in ascending vertex index
__global__ void __launch_bounds__(MS_BLOCK) k_ms_average(const float* __restrict__ verts, const float* __restrict__ cols, uint32_t V, uint32_t n_cells,
                                                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ vmap,
                                                         const float* __restrict__ qpos, const uint8_t* __restrict__ qflag, float* __restrict__ verts_out,
                                                         float* __restrict__ cols_out)
{
    const uint32_t r = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (r >= n_cells) return;
    const uint32_t b = ustart[r], e = r + 1u < n_cells ? ustart[r + 1u] : V;
    if (b >= V || e > V || e <= b) return;
    const uint32_t head = order[b];
    if (head >= V) return;
    const uint32_t p = vmap[head];
    if (p >= n_cells) return;
    double sv[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = b; i < e; i++) {
        const uint32_t v = order[i];
        if (v >= V) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) { sv[a] += (double)verts[3 * (size_t)v + a]; sc[a] += (double)cols[3 * (size_t)v + a]; }
    }
    const double n = (double)(e - b);
    const bool q = qflag && qflag[p];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        verts_out[3 * (size_t)p + a] = q ? qpos[3 * (size_t)p + a] : (float)(sv[a] / n);
        cols_out[3 * (size_t)p + a] = (float)(sc[a] / n);
    }
}
__global__ void __launch_bounds__(MS_BLOCK) k_ms_emit_tris(const uint32_t* __restrict__ rt, uint32_t T, uint32_t n_out, const uint32_t* __restrict__ tmap, int32_t* __restrict__ out)
{
    const uint32_t j = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (j >= n_out) return;
    const uint32_t t = tmap[j];
    if (t >= T) return;
#pragma unroll
    for (int q = 0; q < 3; q++) out[3 * (size_t)j + q] = (int32_t)rt[3 * (size_t)t + q];
}
__global__ void __launch_bounds__(MS_BLOCK) k_ms_emit_map(const uint32_t* __restrict__ vmap, uint32_t V, int32_t* __restrict__ out)
{
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v < V) out[v] = (int32_t)vmap[v];
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
struct MsScratch {
    uint32_t *bb, *n_qruns;                       // bb[0..2], the corner runs at word 8: one clear
    GsrSortBuf so; uint32_t *key_lo, *key_hi;     // the vertices' sort and the two words of their keys
    uint32_t *sums, *order, *ustart, *rank, *first, *vmap;      // order .. vmap stay until the emit
    uint8_t *vflag, *qflag, *live, *tkeep;
    float* qpos;
    GsrSortBuf cso; uint32_t* qstart;             // the corners' sort (quadric only)
    uint32_t *rt, *tmap;
    MsTable tb;
    size_t bytes;
};
static MsScratch ms_carve(uint64_t T, uint64_t V, bool quadric, const void* base)
{
    MsScratch m; GsrCarve c(base);
    const size_t v = V > 0 ? V : 1, t = T > 0 ? T : 1, h = 3 * t, n = std::max(v, quadric ? h : t);
    m.bb = c.take<uint32_t>(64); m.n_qruns = m.bb + 8;
    m.so = gsr_sort_carve(c, v); m.key_lo = c.take<uint32_t>(v); m.key_hi = c.take<uint32_t>(v);
    m.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    m.order = c.take<uint32_t>(v); m.ustart = c.take<uint32_t>(v); m.rank = c.take<uint32_t>(v); m.first = c.take<uint32_t>(v); m.vmap = c.take<uint32_t>(v);
    m.vflag = c.take<uint8_t>(v); m.qflag = c.take<uint8_t>(v); m.live = c.take<uint8_t>(t); m.tkeep = c.take<uint8_t>(t);
    m.qpos = c.take<float>(quadric ? 3 * v : 1);
    const size_t hq = quadric ? h : 1;
    m.cso = gsr_sort_carve(c, hq); m.qstart = c.take<uint32_t>(hq);
    m.rt = c.take<uint32_t>(3 * t); m.tmap = c.take<uint32_t>(t);
    uint32_t slots = 64;
    while (slots < 2 * t) slots <<= 1;            // 2 t < 2^31: at most 2^31 slots
    m.tb.mask = slots - 1u; m.tb.owner = c.take<uint32_t>(slots);
    m.bytes = c.bytes();
    return m;
}
static bool ms_sizes_ok(int64_t T, int64_t V) { return T >= 0 && V >= 0 && V <= 0x7FFFFFFFll && 3 * (unsigned long long)T < (1ull << 31); }
static int ms_args(const char* who, int64_t T, int64_t V, double voxel, int32_t contraction)
{
    if (!ms_sizes_ok(T, V)) { gsr_set_error("%s: %lld triangles / %lld vertices out of range: V and 3T must stay below 2^31", who, (long long)T, (long long)V); return 1; }
    if (!(voxel > 0.0) || !(voxel < 1.0e300)) { gsr_set_error("%s: voxel_size must be a positive finite number", who); return 1; }
    if (contraction != GSR_SIMPLIFY_AVERAGE && contraction != GSR_SIMPLIFY_QUADRIC) { gsr_set_error("%s: unknown contraction %d", who, contraction); return 1; }
    return 0;
}
static uint32_t ms_grid(uint32_t n) { return gsr_div_up(n > 0 ? n : 1u, MS_BLOCK); }

extern "C" size_t gsr_mesh_simplify_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t contraction)
{
    if (!ms_sizes_ok(n_triangles, n_vertices) || (contraction != GSR_SIMPLIFY_AVERAGE && contraction != GSR_SIMPLIFY_QUADRIC)) return 0;
    return ms_carve((uint64_t)n_triangles, (uint64_t)n_vertices, contraction == GSR_SIMPLIFY_QUADRIC, nullptr).bytes;
}

extern "C" int gsr_mesh_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double voxel_size, int32_t contraction,
                                       void* scratch, size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "mesh_simplify_count";
    if (ms_args(who, n_triangles, n_vertices, voxel_size, contraction)) return 1;
    if (!record_dev || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) { gsr_set_error("%s: null pointer", who); return 1; }
    const bool quadric = contraction == GSR_SIMPLIFY_QUADRIC;
    const MsScratch m = ms_carve((uint64_t)n_triangles, (uint64_t)n_vertices, quadric, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t V = (uint32_t)n_vertices, T = (uint32_t)n_triangles, H = 3u * T;
    if (gsr_memset_async(record_dev, 0, 32, s) || gsr_memset_async(m.bb, 0, 256, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (V > 0) {
        hipLaunchKernelGGL(k_ms_bound, dim3(std::min(gsr_div_up(V, MS_BLOCK * 16u), 512u)), dim3(MS_BLOCK), 0, s, vertices, V, m.bb, record_dev + MS_R_STATUS);
        hipLaunchKernelGGL(k_ms_keys, dim3(ms_grid(V)), dim3(MS_BLOCK), 0, s, vertices, V, m.bb, voxel_size, m.key_lo, m.key_hi, m.so.ka, record_dev + MS_R_STATUS);
        GsrSort st(m.so);
        if (st.sort(V, nullptr, 32, true, s) || gsr_sort_next_word(st, V, nullptr, GsrWordFromArray{m.key_hi}, s)) return 1;
        const MsRuns ru = { st.keys, st.order, m.key_lo, V };
        hipLaunchKernelGGL(k_ms_heads, dim3(ms_grid(V)), dim3(MS_BLOCK), 0, s, ru, m.vflag, m.order);
        gsr_rows_keep_scan(m.vflag, V, m.sums, m.first, m.rank, record_dev + MS_R_V, s);
        gsr_compact(MsRunOp{ru, m.ustart}, V, m.sums, m.n_qruns + 1, s);      // the same count once more, into a spare word
        hipLaunchKernelGGL(k_ms_vmap, dim3(ms_grid(V)), dim3(MS_BLOCK), 0, s, m.order, V, record_dev + MS_R_V, m.ustart, m.rank, m.vmap);
    }
    if (quadric && V > 0 && T > 0) {
        int bits = 1;
        while (bits < 32 && (1ull << bits) < (unsigned long long)V) bits++;
        if (gsr_memset_async(m.qflag, 0, V, s)) { gsr_set_error("%s: clear", who); return 1; }
        hipLaunchKernelGGL(k_ms_corner_keys, dim3(ms_grid(H)), dim3(MS_BLOCK), 0, s, triangles, H, V, m.vmap, m.cso.ka);
        GsrSort cst(m.cso);
        if (cst.sort(H, nullptr, bits, true, s)) return 1;
        gsr_compact(MsCornerRunOp{cst.keys, m.qstart}, H, m.sums, m.n_qruns, s);
        const MsMesh mesh = { vertices, triangles, V, T, voxel_size };
        hipLaunchKernelGGL(k_ms_quadric, dim3(ms_grid(std::min(H, V))), dim3(MS_BLOCK), 0, s, mesh, m.bb, m.n_qruns, m.qstart, cst.keys, cst.order, m.first, m.key_lo, m.key_hi, m.qpos,
                           m.qflag, record_dev);
    }
    if (T > 0) {
        if (gsr_memset_async(m.tb.owner, 0xFF, ((size_t)m.tb.mask + 1) * 4, s)) { gsr_set_error("%s: clear", who); return 1; }
        hipLaunchKernelGGL(k_ms_rotate, dim3(ms_grid(T)), dim3(MS_BLOCK), 0, s, triangles, T, V, m.vmap, m.rt, m.live, record_dev + MS_R_STATUS);
        hipLaunchKernelGGL(k_ms_insert, dim3(ms_grid(T)), dim3(MS_BLOCK), 0, s, m.rt, m.live, T, m.tb, record_dev + MS_R_STATUS);
        hipLaunchKernelGGL(k_ms_tkeep, dim3(ms_grid(T)), dim3(MS_BLOCK), 0, s, m.rt, m.live, T, m.tb, m.tkeep, record_dev + MS_R_STATUS);
        gsr_rows_keep_scan(m.tkeep, T, m.sums, m.tmap, nullptr, record_dev + MS_R_T, s);
    }
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_mesh_simplify_emit(const float* vertices, const float* vertex_colors, int64_t n_vertices, int64_t n_triangles, double voxel_size, int32_t contraction,
                                      const void* scratch, size_t scratch_bytes, const uint32_t* record, float* vertices_out, float* vertex_colors_out,
                                      int32_t* triangles_out, int32_t* vertex_map_out, void* stream)
{
    const char* who = "mesh_simplify_emit";
    if (ms_args(who, n_triangles, n_vertices, voxel_size, contraction)) return 1;
    if (!record) { gsr_set_error("%s: null record", who); return 1; }
    if (record[MS_R_STATUS]) { gsr_set_error("%s: the count reported status %u, nothing to emit", who, record[MS_R_STATUS]); return 1; }
    const bool quadric = contraction == GSR_SIMPLIFY_QUADRIC;
    const MsScratch m = ms_carve((uint64_t)n_triangles, (uint64_t)n_vertices, quadric, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    const uint32_t V = (uint32_t)n_vertices, T = (uint32_t)n_triangles, n_v = record[MS_R_V], n_t = record[MS_R_T];
    if (n_v > V || n_t > T || (V > 0 && n_v == 0) || record[MS_R_Q] > n_v || (!quadric && record[MS_R_Q])) { gsr_set_error("%s: the record does not belong to this mesh", who); return 1; }
    if ((n_v > 0 && (!vertices || !vertex_colors || !vertices_out || !vertex_colors_out)) || (n_t > 0 && !triangles_out)) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (n_v > 0) {
        hipLaunchKernelGGL(k_ms_average, dim3(ms_grid(n_v)), dim3(MS_BLOCK), 0, s, vertices, vertex_colors, V, n_v, m.order, m.ustart, m.vmap, m.qpos,
                           (quadric && T > 0) ? m.qflag : nullptr, vertices_out, vertex_colors_out);
    }
    if (n_t > 0) hipLaunchKernelGGL(k_ms_emit_tris, dim3(ms_grid(n_t)), dim3(MS_BLOCK), 0, s, m.rt, T, n_t, m.tmap, triangles_out);
    if (vertex_map_out && V > 0) hipLaunchKernelGGL(k_ms_emit_map, dim3(ms_grid(V)), dim3(MS_BLOCK), 0, s, m.vmap, V, vertex_map_out);
    return gsr_check_launch(who, s, false);
}
