// gsr_mesh_smooth.hip -- the vertex -> vertex adjacency of an index buffer, the smoothing filters that gather over it and the normals of a mesh, on
// the device: the role of Open3D's filter_smooth_simple / _laplacian / _taubin, compute_triangle_normals and compute_vertex_normals after
// post_process_mesh and simplify_vertex_clustering.  Open3D is not part of the reference tree and nothing is held against it: the result is DEFINED
// in include/gsrast.h ("mesh smoothing and normals") and restated operation by operation in tests/smooth_truth.py.  Every output is
// a pure function of the arrays: no float atomics, every sum in a stated order, two runs give the same bits.
//
//   adjacency   the 6 T directed pairs (src, dst) of the triangles, element e = 6 t + q: src = corner q / 2, dst = one of the other two.  A pair with
//               src == dst, or of a triangle with an index out of range, gets the key (V, V) and stands behind every real one.  Stable sort on dst,
//               then on src (gsr_sort.h: a key of two words, least significant first, ceil(log2(V + 1)) bits each): the pairs of a vertex stand in a
//               run in ascending dst.  Run heads (a pair that differs from the one in front of it) by gsr_compact: neighbours[p] = dst, and src[p]
//               beside it; start[v] = the first p with src[p] >= v, by bisection (k_sm_starts).  The cost does not depend on the degrees.
//   corners     key of corner h = 3 t + k: its vertex (V where out of range), sorted stably with h as value: the corners of a vertex stand in a run
//               in ascending h; cstart[v] by the same bisection.  One thread per vertex adds the float64 normals of its corners' triangles.
//   step        one thread per vertex walks neighbours[start[i] .. start[i + 1]) IN ORDER, four rows of the previous float64 state in flight, and
//               writes its row of the next state (ping-pong); the order of the sum is part of the definition, so a long list is walked by one thread.
// Termination: every loop runs over a run of a sort or bisects an array; no kernel waits for another workgroup.  Everything runs on the caller's
// stream; nothing synchronises.  Built without FMA contraction (PRE_FLAGS).
#include "gsr_common.h"
#include "gsr_scan.h"
#include "gsr_compact.h"
#include <algorithm>

#define SM_BLOCK 256
#define SM_R_STATUS 0
#define SM_R_E 1

__device__ __forceinline__ bool sm_finite(float x) { return x - x == 0.f; }
__device__ __forceinline__ bool sm_finite(double x) { return x - x == 0.0; }

// ------------------------------------------------------------------------------------------------ adjacency
// The directed pair of element e = 6 t + q: false where it is a self-loop or its triangle has an index out of range
struct SmPairs {
    const int32_t* tris; uint32_t T, V;
    __device__ bool ends(uint32_t e, uint32_t& src, uint32_t& dst) const
    {
        const uint32_t t = e / 6u, q = e - 6u * t, a = q >> 1, b = (a + 1u + (q & 1u)) % 3u;
        if (t >= T) return false;
        const uint32_t ix[3] = { (uint32_t)tris[3 * (size_t)t], (uint32_t)tris[3 * (size_t)t + 1], (uint32_t)tris[3 * (size_t)t + 2] };
        if (ix[0] >= V || ix[1] >= V || ix[2] >= V) return false;
        src = ix[a]; dst = ix[b];
        return src != dst;
    }
};
__global__ void __launch_bounds__(SM_BLOCK) k_sm_pair_dst(SmPairs pr, uint32_t n, uint32_t* __restrict__ keys, uint32_t* __restrict__ status)
{
    const uint32_t e = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (e >= n) return;
    uint32_t src = 0u, dst = 0u;
    const bool ok = pr.ends(e, src, dst);
    keys[e] = ok ? dst : pr.V;
    if (!ok && e % 6u == 0u) {                            // once per triangle: a self-loop is data, an index out of range an error
        const uint32_t t = e / 6u;
        if ((uint32_t)pr.tris[3 * (size_t)t] >= pr.V || (uint32_t)pr.tris[3 * (size_t)t + 1] >= pr.V || (uint32_t)pr.tris[3 * (size_t)t + 2] >= pr.V)
            atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX);
    }
}
struct SmSrcWord {
    SmPairs pr;
    __device__ uint32_t operator()(uint32_t e) const { uint32_t src = 0u, dst = 0u; return pr.ends(e, src, dst) ? src : pr.V; }
};
// sdst[i] = the dst of the pair at place i (V behind the real ones)
__global__ void __launch_bounds__(SM_BLOCK) k_sm_sorted_dst(SmPairs pr, uint32_t n, const uint32_t* __restrict__ order, uint32_t* __restrict__ sdst)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t src = 0u, dst = 0u;
    const uint32_t e = order[i];
    sdst[i] = (e < n && pr.ends(e, src, dst)) ? dst : pr.V;
}
// the run heads in sorted order: pair p of the adjacency is (usrc[p], udst[p])
struct SmEdgeOp {
    const uint32_t *ssrc, *sdst; uint32_t V; uint32_t *usrc, *udst;
    __device__ bool keep(uint32_t i) const
    {
        const uint32_t s = ssrc[i], d = sdst[i];
        if (s >= V || d >= V) return false;
        return i == 0u || ssrc[i - 1u] != s || sdst[i - 1u] != d;
    }
    __device__ void place(uint32_t i, uint32_t p) const { usrc[p] = ssrc[i]; udst[p] = sdst[i]; }
};
// out[v] = the first place of keys[0 .. n) that holds a key >= v, for v in [0, V]; n = min(n_max, *n_dev) where n_dev is given
__global__ void __launch_bounds__(SM_BLOCK) k_sm_starts(const uint32_t* __restrict__ keys, uint32_t n_max, const uint32_t* __restrict__ n_dev, uint32_t V, uint32_t* __restrict__ out)
{
    const uint32_t v = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (v > V) return;
    uint32_t lo = 0u, hi = n_dev ? min(*n_dev, n_max) : n_max;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1u; else hi = mid;
    }
    out[v] = lo;
}

// ------------------------------------------------------------------------------------------------ normals
// n = (v1 - v0) x (v2 - v0), float32 inputs widened, every operation in float64
__device__ __forceinline__ void sm_cross(const float* __restrict__ verts, const uint32_t* ix, double (&n)[3])
{
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) p[k][a] = (double)verts[3 * (size_t)ix[k] + a];
    const double e1[3] = { p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2] };
    const double e2[3] = { p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2] };
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}
// n / |n|, or (0, 0, 1) where the length is 0 or not finite
__device__ __forceinline__ void sm_unit(double (&n)[3])
{
    const double L = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(L > 0.0) || !sm_finite(L)) { n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; return; }
    n[0] = n[0] / L; n[1] = n[1] / L; n[2] = n[2] / L;
}
__global__ void __launch_bounds__(SM_BLOCK) k_sm_tri_normals(const float* __restrict__ verts, const int32_t* __restrict__ tris, uint32_t T, uint32_t V, int normalized,
                                                             float* __restrict__ out, uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t ix[3] = { (uint32_t)tris[3 * (size_t)t], (uint32_t)tris[3 * (size_t)t + 1], (uint32_t)tris[3 * (size_t)t + 2] };
    double n[3] = {0.0, 0.0, 0.0};
    if (ix[0] >= V || ix[1] >= V || ix[2] >= V) atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX);
    else sm_cross(verts, ix, n);
    if (normalized) sm_unit(n);
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * (size_t)t + a] = (float)n[a];
}
__global__ void __launch_bounds__(SM_BLOCK) k_sm_corner_keys(const int32_t* __restrict__ tris, uint32_t H, uint32_t V, uint32_t* __restrict__ keys, uint32_t* __restrict__ status)
{
    const uint32_t h = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (h >= H) return;
    const uint32_t i = (uint32_t)tris[h];
    keys[h] = i < V ? i : V;
    if (i >= V) atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX);
}
// one thread per vertex: the float64 sum of its corners' triangle normals in ascending corner index
__global__ void __launch_bounds__(SM_BLOCK) k_sm_vert_normals(const float* __restrict__ verts, const int32_t* __restrict__ tris, uint32_t T, uint32_t V, int normalized,
                                                              const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ corder, float* __restrict__ out)
{
    const uint32_t v = blockIdx.x * SM_BLOCK + threadIdx.x, H = 3u * T;
    if (v >= V) return;
    const uint32_t e = min(cstart[v + 1u], H), b = min(cstart[v], e);
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = b; i < e; i++) {
        const uint32_t h = corder[i];
        if (h >= H) continue;
        const uint32_t t = h / 3u;
        const uint32_t ix[3] = { (uint32_t)tris[3 * (size_t)t], (uint32_t)tris[3 * (size_t)t + 1], (uint32_t)tris[3 * (size_t)t + 2] };
        if (ix[0] >= V || ix[1] >= V || ix[2] >= V) continue;         // k_sm_corner_keys has said so
        double n[3];
        sm_cross(verts, ix, n);
        s[0] += n[0]; s[1] += n[1]; s[2] += n[2];
    }
    if (normalized) sm_unit(s);
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * (size_t)v + a] = (float)s[a];
}

// ------------------------------------------------------------------------------------------------ the filters
// The state: one row of C doubles per vertex, C = 3 (position) or 6 (position, colour).  A row of six starts on a 16-byte boundary.
template <int C> __device__ __forceinline__ void sm_load(const double* __restrict__ state, uint32_t j, double (&r)[C]);
template <> __device__ __forceinline__ void sm_load<3>(const double* __restrict__ state, uint32_t j, double (&r)[3])
{
    const double* p = state + 3 * (size_t)j;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
}
template <> __device__ __forceinline__ void sm_load<6>(const double* __restrict__ state, uint32_t j, double (&r)[6])
{
    const double2* p = reinterpret_cast<const double2*>(state + 6 * (size_t)j);
    const double2 a = p[0], b = p[1], c = p[2];
    r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y; r[4] = c.x; r[5] = c.y;
}
template <int C> __device__ __forceinline__ void sm_store(double* __restrict__ state, uint32_t j, const double (&r)[C])
{
    if constexpr (C == 6) {
        double2* p = reinterpret_cast<double2*>(state + 6 * (size_t)j);
        p[0] = make_double2(r[0], r[1]); p[1] = make_double2(r[2], r[3]); p[2] = make_double2(r[4], r[5]);
    } else {
        double* p = state + 3 * (size_t)j;
        p[0] = r[0]; p[1] = r[1]; p[2] = r[2];
    }
}
template <int C>
__global__ void __launch_bounds__(SM_BLOCK) k_sm_widen(const float* __restrict__ verts, const float* __restrict__ cols, uint32_t V, double* __restrict__ state, uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= V) return;
    double r[C];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float x = verts[3 * (size_t)i + a];
        bad |= !sm_finite(x);
        r[a] = (double)x;
        if constexpr (C == 6) r[3 + a] = (double)cols[3 * (size_t)i + a];
    }
    sm_store<C>(state, i, r);
    if (bad) atomicOr(status, (uint32_t)GSR_MESH_ERR_NONFINITE);
}
template <int C>
__global__ void __launch_bounds__(SM_BLOCK) k_sm_narrow(const double* __restrict__ state, uint32_t V, float* __restrict__ verts_out, float* __restrict__ cols_out)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= V) return;
    double r[C];
    sm_load<C>(state, i, r);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        verts_out[3 * (size_t)i + a] = (float)r[a];
        if constexpr (C == 6) cols_out[3 * (size_t)i + a] = (float)r[3 + a];
    }
}

// What one neighbour adds.  SIMPLE: s += r.  Otherwise w = 1 / (|p - r| + 1e-12) on the positions, W += w, s += w * r.
template <int C, bool SIMPLE> struct SmAcc {
    double s[C], W;
    __device__ __forceinline__ void add(const double (&p)[C], const double (&r)[C])
    {
        if constexpr (SIMPLE) {
#pragma unroll
            for (int c = 0; c < C; c++) s[c] += r[c];
        } else {
            const double dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
            const double w = 1.0 / (sqrt((dx * dx + dy * dy) + dz * dz) + 1e-12);
            W += w;
#pragma unroll
            for (int c = 0; c < C; c++) s[c] += w * r[c];
        }
    }
};
// One step: SIMPLE q = (p + sum r) / (n + 1), the sum starting from p; otherwise q = p + lambda * (s / W - p), and q = p where there is no neighbour.
// The neighbours are added in the order of the list; four rows are in flight.
template <int C, bool SIMPLE>
__global__ void __launch_bounds__(SM_BLOCK) k_sm_step(const double* __restrict__ in, double* __restrict__ out, const uint32_t* __restrict__ start, const uint32_t* __restrict__ nb,
                                                      uint32_t V, uint32_t e_max, double lambda)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= V) return;
    const uint32_t e = min(start[i + 1u], e_max), b = min(start[i], e);
    double p[C];
    sm_load<C>(in, i, p);
    SmAcc<C, SIMPLE> acc;
    acc.W = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) acc.s[c] = SIMPLE ? p[c] : 0.0;
    uint32_t k = b;
    for (; k + 4u <= e; k += 4u) {
        uint32_t j[4];
        double r[4][C];
#pragma unroll
        for (int u = 0; u < 4; u++) j[u] = min(nb[k + u], V - 1u);        // a list holds indices below V; the bound costs nothing
#pragma unroll
        for (int u = 0; u < 4; u++) sm_load<C>(in, j[u], r[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) acc.add(p, r[u]);
    }
    for (; k < e; k++) {
        double r[C];
        sm_load<C>(in, min(nb[k], V - 1u), r);
        acc.add(p, r);
    }
    double q[C];
    if constexpr (SIMPLE) {
        const double n = (double)(e - b + 1u);
#pragma unroll
        for (int c = 0; c < C; c++) q[c] = acc.s[c] / n;
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) q[c] = e > b ? p[c] + lambda * (acc.s[c] / acc.W - p[c]) : p[c];
    }
    sm_store<C>(out, i, q);
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
struct SmScratch {
    uint32_t* words;                              // word 0: the pairs kept, where the caller has no record
    GsrSortBuf so; uint32_t* sums;                // the sort of the 6 T pairs (or the 3 T corners) and the compaction's block sums
    uint32_t* start;                              // [V + 1], smoothing and normals only
    double *sa, *sb;                              // the two states, smoothing only
    size_t bytes;
};
static int sm_bits(uint64_t V) { int b = 1; while (b < 32 && (1ull << b) <= V) b++; return b; }        // the keys are 0 .. V
// The 6T pairs go through kernels, the sort and the compaction, whose grids and block counts round their number up in 32 bits, by up to
// SM_SIZE_SLACK (the sort's largest block, GSR_SORT_THREADS * 16): 6T + SM_SIZE_SLACK <= 2^32, a few hundred triangles short of 3T < 2^31.
#define SM_SIZE_SLACK 4096ull
static bool sm_sizes_ok(int64_t T, int64_t V)
{
    return T >= 0 && V >= 0 && V <= 0x7FFFFFFFll && T <= 0x7FFFFFFFll && 6 * (unsigned long long)T + SM_SIZE_SLACK <= (1ull << 32);
}
static uint32_t sm_grid(uint32_t n) { return gsr_div_up(n > 0 ? n : 1u, SM_BLOCK); }
// per_tri: the elements of the sort per triangle (6 pairs or 3 corners); starts: the V + 1 words; channels: doubles per state row (0: no state)
static SmScratch sm_carve(uint64_t T, uint64_t V, int per_tri, bool starts, int channels, const void* base)
{
    SmScratch m; GsrCarve c(base);
    const size_t n = per_tri * (T > 0 ? T : 1), v = V > 0 ? V : 1;
    m.words = c.take<uint32_t>(64);
    m.so = gsr_sort_carve(c, n);
    m.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    m.start = c.take<uint32_t>(starts ? v + 1 : 1);
    m.sa = c.take<double>(channels ? channels * v : 1);
    m.sb = c.take<double>(channels ? channels * v : 1);
    m.bytes = c.bytes();
    return m;
}
// Where the sort of the pairs leaves them: two sorts of `bits` bits each
struct SmAdj { uint32_t *ssrc, *sdst, *usrc, *udst; };
static SmAdj sm_adj(const SmScratch& m, int bits)
{
    GsrSort st(m.so);
    st.advance(bits); st.advance(bits);
    return SmAdj{ st.keys, st.free_keys, st.order, st.free_order };
}
// Everything up to the unique pairs: *n_edges = E, pair p = (usrc[p], udst[p]) in ascending (src, dst).  *status and *n_edges are zero on entry.
static int sm_build(const char* who, const int32_t* tris, uint32_t T, uint32_t V, const SmScratch& m, uint32_t* status, uint32_t* n_edges, hipStream_t s)
{
    if (T == 0u) return 0;
    const uint32_t n = 6u * T;
    const int bits = sm_bits(V);
    const SmPairs pr = { tris, T, V };
    hipLaunchKernelGGL(k_sm_pair_dst, dim3(sm_grid(n)), dim3(SM_BLOCK), 0, s, pr, n, m.so.ka, status);
    GsrSort st(m.so);
    if (st.sort(n, nullptr, bits, true, s)) return 1;
    hipLaunchKernelGGL(k_sort_word<SmSrcWord>, dim3(gsr_div_up(n, GSR_SORT_WORD_BLOCK)), dim3(GSR_SORT_WORD_BLOCK), 0, s, SmSrcWord{pr}, n, (const uint32_t*)nullptr,
                       (const uint32_t*)st.order, st.keys);
    if (st.sort(n, nullptr, bits, false, s)) return 1;
    const SmAdj a = sm_adj(m, bits);
    if (a.ssrc != st.keys || a.usrc != st.order) { gsr_set_error("%s: internal: the sort's buffers", who); return 1; }
    hipLaunchKernelGGL(k_sm_sorted_dst, dim3(sm_grid(n)), dim3(SM_BLOCK), 0, s, pr, n, (const uint32_t*)st.order, a.sdst);
    gsr_compact(SmEdgeOp{a.ssrc, a.sdst, V, a.usrc, a.udst}, n, m.sums, n_edges, s);      // usrc overwrites the order: k_sm_sorted_dst was its last reader
    return 0;
}

extern "C" size_t gsr_mesh_adjacency_scratch_bytes(int64_t n_triangles, int64_t n_vertices)
{
    if (!sm_sizes_ok(n_triangles, n_vertices)) return 0;
    return sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 6, false, 0, nullptr).bytes;
}
extern "C" size_t gsr_mesh_normals_scratch_bytes(int64_t n_triangles, int64_t n_vertices)
{
    if (!sm_sizes_ok(n_triangles, n_vertices)) return 0;
    return sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 3, true, 0, nullptr).bytes;
}
static bool sm_scope_ok(int32_t scope) { return scope == GSR_SMOOTH_SCOPE_ALL || scope == GSR_SMOOTH_SCOPE_VERTEX; }
extern "C" size_t gsr_mesh_smooth_scratch_bytes(int64_t n_triangles, int64_t n_vertices, int32_t scope)
{
    if (!sm_sizes_ok(n_triangles, n_vertices) || !sm_scope_ok(scope)) return 0;
    return sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 6, true, scope == GSR_SMOOTH_SCOPE_ALL ? 6 : 3, nullptr).bytes;
}
static int sm_sizes(const char* who, int64_t T, int64_t V)
{
    if (sm_sizes_ok(T, V)) return 0;
    gsr_set_error("%s: %lld triangles / %lld vertices out of range: V must stay below 2^31 and 6T within 2^32 - 4096", who, (long long)T, (long long)V);
    return 1;
}

extern "C" int gsr_mesh_adjacency_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* scratch, size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "mesh_adjacency_count";
    if (sm_sizes(who, n_triangles, n_vertices)) return 1;
    if (!record_dev || (n_triangles > 0 && !triangles)) { gsr_set_error("%s: null pointer", who); return 1; }
    const SmScratch m = sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 6, false, 0, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(record_dev, 0, 32, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (sm_build(who, triangles, (uint32_t)n_triangles, (uint32_t)n_vertices, m, record_dev + SM_R_STATUS, record_dev + SM_R_E, s)) return 1;
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_mesh_adjacency_emit(int64_t n_triangles, int64_t n_vertices, const void* scratch, size_t scratch_bytes, const uint32_t* record, int32_t* start_out,
                                       int32_t* neighbours_out, void* stream)
{
    const char* who = "mesh_adjacency_emit";
    if (sm_sizes(who, n_triangles, n_vertices)) return 1;
    if (!record || !start_out) { gsr_set_error("%s: null pointer", who); return 1; }
    if (record[SM_R_STATUS]) { gsr_set_error("%s: the count reported status %u, nothing to emit", who, record[SM_R_STATUS]); return 1; }
    const SmScratch m = sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 6, false, 0, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    const uint32_t T = (uint32_t)n_triangles, V = (uint32_t)n_vertices, E = record[SM_R_E];
    if ((unsigned long long)E > 6ull * T) { gsr_set_error("%s: the record does not belong to this mesh", who); return 1; }
    if (E > 0x7FFFFFFFu) { gsr_set_error("%s: %u directed edges do not fit the int32 offsets of start", who, E); return 1; }
    if (E > 0u && !neighbours_out) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const SmAdj a = sm_adj(m, sm_bits(V));
    hipLaunchKernelGGL(k_sm_starts, dim3(sm_grid(V + 1u)), dim3(SM_BLOCK), 0, s, (const uint32_t*)a.usrc, E, (const uint32_t*)nullptr, V, (uint32_t*)start_out);
    if (E > 0u) GSR_CHECK(hipMemcpyAsync(neighbours_out, a.udst, (size_t)E * 4, hipMemcpyDeviceToDevice, s), who);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_mesh_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t normalized, float* triangle_normals_out,
                                float* vertex_normals_out, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "mesh_normals";
    if (sm_sizes(who, n_triangles, n_vertices)) return 1;
    if (!status_dev || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t T = (uint32_t)n_triangles, V = (uint32_t)n_vertices, H = 3u * T;
    if (gsr_memset_async(status_dev, 0, 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (triangle_normals_out && T > 0u)
        hipLaunchKernelGGL(k_sm_tri_normals, dim3(sm_grid(T)), dim3(SM_BLOCK), 0, s, vertices, triangles, T, V, (int)normalized, triangle_normals_out, status_dev);
    if (vertex_normals_out) {
        const SmScratch m = sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 3, true, 0, scratch);
        if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
        GsrSort st(m.so);
        if (T > 0u) {
            hipLaunchKernelGGL(k_sm_corner_keys, dim3(sm_grid(H)), dim3(SM_BLOCK), 0, s, triangles, H, V, m.so.ka, status_dev);
            if (st.sort(H, nullptr, sm_bits(V), true, s)) return 1;
        }
        hipLaunchKernelGGL(k_sm_starts, dim3(sm_grid(V + 1u)), dim3(SM_BLOCK), 0, s, (const uint32_t*)st.keys, H, (const uint32_t*)nullptr, V, m.start);
        if (V > 0u)
            hipLaunchKernelGGL(k_sm_vert_normals, dim3(sm_grid(V)), dim3(SM_BLOCK), 0, s, vertices, triangles, T, V, (int)normalized, (const uint32_t*)m.start,
                               (const uint32_t*)st.order, vertex_normals_out);
    }
    return gsr_check_launch(who, s, false);
}

template <int C>
static void sm_steps(const SmScratch& m, const uint32_t* nb, uint32_t V, uint32_t e_max, int32_t filter, int32_t iterations, double lambda, double mu, const float* vertices,
                     const float* colors, float* vertices_out, float* colors_out, uint32_t* status, hipStream_t s)
{
    const dim3 g(sm_grid(V)), blk(SM_BLOCK);
    double *cur = m.sa, *nxt = m.sb;
    hipLaunchKernelGGL(k_sm_widen<C>, g, blk, 0, s, vertices, colors, V, cur, status);
    for (int32_t it = 0; it < iterations; it++) {
        if (filter == GSR_SMOOTH_SIMPLE) {
            hipLaunchKernelGGL((k_sm_step<C, true>), g, blk, 0, s, (const double*)cur, nxt, (const uint32_t*)m.start, nb, V, e_max, 0.0);
            std::swap(cur, nxt);
        } else {
            hipLaunchKernelGGL((k_sm_step<C, false>), g, blk, 0, s, (const double*)cur, nxt, (const uint32_t*)m.start, nb, V, e_max, lambda);
            std::swap(cur, nxt);
            if (filter == GSR_SMOOTH_TAUBIN) {
                hipLaunchKernelGGL((k_sm_step<C, false>), g, blk, 0, s, (const double*)cur, nxt, (const uint32_t*)m.start, nb, V, e_max, mu);
                std::swap(cur, nxt);
            }
        }
    }
    hipLaunchKernelGGL(k_sm_narrow<C>, g, blk, 0, s, (const double*)cur, V, vertices_out, colors_out);
}

extern "C" int gsr_mesh_smooth(const float* vertices, const float* vertex_colors, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t filter,
                               int32_t iterations, double lambda, double mu, int32_t scope, float* vertices_out, float* vertex_colors_out, void* scratch, size_t scratch_bytes,
                               uint32_t* status_dev, void* stream)
{
    const char* who = "mesh_smooth";
    if (sm_sizes(who, n_triangles, n_vertices)) return 1;
    if (filter != GSR_SMOOTH_SIMPLE && filter != GSR_SMOOTH_LAPLACIAN && filter != GSR_SMOOTH_TAUBIN) { gsr_set_error("%s: unknown filter %d", who, filter); return 1; }
    if (!sm_scope_ok(scope)) { gsr_set_error("%s: unknown scope %d", who, scope); return 1; }
    if (iterations < 0) { gsr_set_error("%s: %d iterations", who, iterations); return 1; }
    if (filter != GSR_SMOOTH_SIMPLE && (!(lambda - lambda == 0.0) || (filter == GSR_SMOOTH_TAUBIN && !(mu - mu == 0.0)))) { gsr_set_error("%s: lambda and mu must be finite", who); return 1; }
    if (!status_dev || (n_vertices > 0 && (!vertices || !vertex_colors || !vertices_out || !vertex_colors_out)) || (n_triangles > 0 && !triangles)) {
        gsr_set_error("%s: null pointer", who); return 1;
    }
    const bool all = scope == GSR_SMOOTH_SCOPE_ALL;
    const SmScratch m = sm_carve((uint64_t)n_triangles, (uint64_t)n_vertices, 6, true, all ? 6 : 3, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t T = (uint32_t)n_triangles, V = (uint32_t)n_vertices;
    if (gsr_memset_async(status_dev, 0, 8, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (V == 0u) return gsr_check_launch(who, s, false);
    const size_t row = (size_t)V * 12;
    if (iterations == 0) {                                // a copy, bit for bit; nothing is looked at
        GSR_CHECK(hipMemcpyAsync(vertices_out, vertices, row, hipMemcpyDeviceToDevice, s), who);
        GSR_CHECK(hipMemcpyAsync(vertex_colors_out, vertex_colors, row, hipMemcpyDeviceToDevice, s), who);
        return gsr_check_launch(who, s, false);
    }
    if (sm_build(who, triangles, T, V, m, status_dev + SM_R_STATUS, status_dev + SM_R_E, s)) return 1;
    const SmAdj a = sm_adj(m, sm_bits(V));
    hipLaunchKernelGGL(k_sm_starts, dim3(sm_grid(V + 1u)), dim3(SM_BLOCK), 0, s, (const uint32_t*)a.usrc, 6u * T, (const uint32_t*)(status_dev + SM_R_E), V, m.start);
    if (all) sm_steps<6>(m, a.udst, V, 6u * T, filter, iterations, lambda, mu, vertices, vertex_colors, vertices_out, vertex_colors_out, status_dev + SM_R_STATUS, s);
    else {
        sm_steps<3>(m, a.udst, V, 6u * T, filter, iterations, lambda, mu, vertices, vertex_colors, vertices_out, vertex_colors_out, status_dev + SM_R_STATUS, s);
        GSR_CHECK(hipMemcpyAsync(vertex_colors_out, vertex_colors, row, hipMemcpyDeviceToDevice, s), who);
    }
    return gsr_check_launch(who, s, false);
}
