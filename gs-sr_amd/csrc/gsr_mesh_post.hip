// gsr_mesh_post.hip -- floaters filtered from a welded triangle mesh on the device: the role of the four Open3D calls behind the reference's
// post_process_mesh (gssr/utils/mesh_utils.py:28-48: cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices,
// remove_degenerate_triangles).  Open3D is not part of the reference tree: the semantics are restated from Open3D 0.18's published sources and
// their parity is UNPINNED (include/gsrast.h, gsr_mesh_*).  Every integer output is a pure function of the index buffer.
//
//   edge table   open addressing, a power of two of slots >= 2 * 3T, a slot = 64-bit key (min << 32 | max) + the smallest triangle that carries the
//                edge.  k_mp_insert: atomicCAS on the key, atomicMin on the triangle.  k_mp_union, a kernel later: every half-edge looks its slot
//                up and unites its triangle with that smallest one -- nobody reads an owner before the last writer has left.
//   union-find   parent[T], the larger root is hooked under the smaller with atomicCAS, so parent[x] <= x always holds: a find walks strictly
//                downwards (at most T steps), the root of a component is its smallest triangle, and a failed hook lowers the larger of the two
//                roots it retries with (at most T rounds).  k_mp_flatten reads the roots off.
//   numbering    root flags -> exclusive ranks (the keep scan the row compaction uses, gsr_rows_keep_scan) = cluster ids in ascending order of the
//                smallest triangle; counts by integer atomics, areas by double atomics (wave-aggregated where neighbours share a cluster).
//   threshold    k-th largest of the C counts: the radix select of gsr_init.hip (gsr_select, gsr_common.h) over the complemented counts, rank
//                k - 1, with C read on the device; k_mp_finish applies the floor.
//   filter       triangle keep flags and vertex-referenced flags (plain byte stores), one keep scan each, then the triangles remapped at their final
//                places (k_mp_emit) and the vertex rows through the row mover (gsr_rows_move).
// Termination: probe loops are capped at the table size, find and hook loops by the invariant above; no kernel waits for another workgroup; the
// multi-block scans are count / scan / place passes.  Everything runs on the caller's stream; nothing synchronises.
// Built without FMA contraction (PRE_FLAGS): the areas are evaluated in double operation by operation.
#include "gsr_common.h"
#include "gsr_scan.h"
#include <algorithm>
#include <vector>

#define MP_BLOCK 256
#define MP_EMPTY 0xFFFFFFFFFFFFFFFFull      // no edge has this key: a vertex index is at most 2^31 - 2
// record words (include/gsrast.h)
#define MP_R_STATUS 0
#define MP_R_C 1
#define MP_R_THR 2
#define MP_R_V 3
#define MP_R_T 4

struct MpTable { unsigned long long* keys; uint32_t* owner; unsigned long long mask; };      // mask = slots - 1

__device__ __forceinline__ unsigned long long mp_hash(unsigned long long x)      // splitmix64's finaliser: all 64 bits of the key decide the slot
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ unsigned long long mp_key(int32_t a, int32_t b)
{
    const uint32_t lo = (uint32_t)min(a, b), hi = (uint32_t)max(a, b);
    return ((unsigned long long)lo << 32) | hi;
}
__device__ __forceinline__ bool mp_in_range(const int32_t* i, uint32_t V) { return (uint32_t)i[0] < V && (uint32_t)i[1] < V && (uint32_t)i[2] < V; }
__device__ __forceinline__ uint32_t mp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// at most `slots` probes; false = the table is full (cannot happen with slots >= 2 * 3T)
__device__ __forceinline__ bool mp_insert(const MpTable& tb, unsigned long long key, uint32_t t)
{
    unsigned long long h = mp_hash(key) & tb.mask;
    for (unsigned long long n = 0; n <= tb.mask; n++, h = (h + 1) & tb.mask) {
        unsigned long long k = __hip_atomic_load(tb.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // a key never changes once it is set
        if (k == MP_EMPTY) k = atomicCAS(tb.keys + h, MP_EMPTY, key);
        if (k == MP_EMPTY || k == key) { atomicMin(tb.owner + h, t); return true; }
    }
    return false;
}
// the smallest triangle on the edge, 0xFFFFFFFF = not in the table (cannot happen after k_mp_insert)
__device__ __forceinline__ uint32_t mp_owner(const MpTable& tb, unsigned long long key)
{
    unsigned long long h = mp_hash(key) & tb.mask;
    for (unsigned long long n = 0; n <= tb.mask; n++, h = (h + 1) & tb.mask) {
        const unsigned long long k = tb.keys[h];
        if (k == key) return tb.owner[h];
        if (k == MP_EMPTY) break;
    }
    return 0xFFFFFFFFu;
}

// x strictly decreases: at most x + 1 rounds.  Path halving: parent[x] <- its grandparent, an ancestor of x for good (only roots are ever hooked).
__device__ __forceinline__ uint32_t mp_find(uint32_t* parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = mp_load(parent + x);
        if (p >= x) return x;                     // p == x: a root (p > x never holds; read as a root, it ends the walk all the same)
        const uint32_t g = mp_load(parent + p);
        if (g < p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
    }
}
// false = the invariant parent[x] <= x was found broken (cannot happen)
__device__ __forceinline__ bool mp_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    for (;;) {                                    // a failed hook replaces the larger root by a smaller index: max(a, b) strictly decreases
        a = mp_find(parent, a); b = mp_find(parent, b);
        if (a == b) return true;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return true;
        if (old > a) return false;
        a = old;
    }
}

__global__ void __launch_bounds__(MP_BLOCK) k_mp_insert(const int32_t* __restrict__ tris, uint32_t T, uint32_t V, MpTable tb, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * MP_BLOCK + threadIdx.x;
    if (t >= T) return;
    parent[t] = t;
    const int32_t i[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    if (!mp_in_range(i, V)) { atomicOr(status, (uint32_t)GSR_MESH_ERR_INDEX); return; }      // stays a cluster of its own; the host raises
    bool ok = mp_insert(tb, mp_key(i[0], i[1]), t);
    ok = mp_insert(tb, mp_key(i[1], i[2]), t) && ok;
    ok = mp_insert(tb, mp_key(i[2], i[0]), t) && ok;
    if (!ok) atomicOr(status, (uint32_t)GSR_MESH_ERR_INTERNAL);
}

__global__ void __launch_bounds__(MP_BLOCK) k_mp_union(const int32_t* __restrict__ tris, uint32_t T, uint32_t V, MpTable tb, uint32_t* parent, uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * MP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int32_t i[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    if (!mp_in_range(i, V)) return;
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t m = mp_owner(tb, mp_key(i[e], i[e == 2 ? 0 : e + 1]));
        if (m >= T) { ok = false; continue; }
        if (m != t) ok = mp_unite(parent, t, m) && ok;
    }
    if (!ok) atomicOr(status, (uint32_t)GSR_MESH_ERR_INTERNAL);
}

// parent is read only here: root[t] and the byte flag "t is a root"
__global__ void __launch_bounds__(MP_BLOCK) k_mp_flatten(const uint32_t* __restrict__ parent, uint32_t T, uint32_t* __restrict__ root, uint8_t* __restrict__ is_root)
{
    const uint32_t t = blockIdx.x * MP_BLOCK + threadIdx.x;
    if (t >= T) return;
    uint32_t x = t;
    for (;;) { const uint32_t p = parent[x]; if (p >= x) break; x = p; }
    root[t] = x;
    is_root[t] = x == t ? 1 : 0;
}

__device__ __forceinline__ double mp_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// clusters[t] = rank of t's root; counts and areas by atomics.  Neighbours in the index buffer mostly share a cluster: up to four groups of a wave
// are summed across the lanes first (one atomic per group), what is left adds alone.  counts / area are zero on entry.
__global__ void __launch_bounds__(MP_BLOCK) k_mp_label(const int32_t* __restrict__ tris, uint32_t T, uint32_t V, const float* __restrict__ verts,
                                                       const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank, int32_t* __restrict__ clusters,
                                                       uint32_t* __restrict__ counts, double* __restrict__ area)
{
    const uint32_t t = blockIdx.x * MP_BLOCK + threadIdx.x;
    bool live = t < T;
    uint32_t c = 0;
    double a = 0.0;
    if (live) {
        c = rank[root[t]];                        // < C <= T
        clusters[t] = (int32_t)c;
        if (area) {
            const int32_t i[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
            if (mp_in_range(i, V)) {
                const float* p0 = verts + 3 * (size_t)i[0]; const float* p1 = verts + 3 * (size_t)i[1]; const float* p2 = verts + 3 * (size_t)i[2];
                const double x1 = (double)p1[0] - (double)p0[0], y1 = (double)p1[1] - (double)p0[1], z1 = (double)p1[2] - (double)p0[2];
                const double x2 = (double)p2[0] - (double)p0[0], y2 = (double)p2[1] - (double)p0[1], z2 = (double)p2[2] - (double)p0[2];
                const double cx = y1 * z2 - z1 * y2, cy = z1 * x2 - x1 * z2, cz = x1 * y2 - y1 * x2;
                a = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
            }
        }
    }
    const uint32_t lane = lane_id();
    unsigned long long todo = __ballot(live);
    for (int it = 0; it < 4 && todo; it++) {      // wave-uniform
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)c, lead, 64);
        const bool mine = live && c == c0;
        const unsigned long long m = __ballot(mine);
        if (area) {
            const double s = mp_wave_sum(mine ? a : 0.0);
            if ((int)lane == lead) atomicAdd(area + c0, s);
        }
        if ((int)lane == lead) atomicAdd(counts + c0, (uint32_t)__popcll(m));
        if (mine) live = false;
        todo &= ~m;
    }
    if (live) {
        atomicAdd(counts + c, 1u);
        if (area) atomicAdd(area + c, a);
    }
}

// the fixed words of the record: the threshold (cluster rule) and the counts a scan does not write
__global__ void __launch_bounds__(64) k_mp_finish(uint32_t* __restrict__ record, const uint32_t* __restrict__ sel_state, int cluster_rule, uint32_t k, uint32_t floor_,
                                                  uint32_t V)
{
    if (threadIdx.x != 0) return;
    uint32_t thr = 0u;
    if (cluster_rule) {
        const uint32_t C = record[MP_R_C];
        if (k < 1u || k > C) { atomicOr(record + MP_R_STATUS, (uint32_t)GSR_MESH_ERR_KEEP); thr = 0xFFFFFFFFu; }      // the select did not run, or ran beyond the keys
        else thr = max(~sel_state[0], floor_);        // the key of rank k - 1 is the complement of the k-th largest count
    } else record[MP_R_C] = 0u;
    record[MP_R_THR] = thr;
    record[MP_R_V] = V;                           // overwritten by the vertex scan where unreferenced vertices are dropped
}

// step 2 (the keep rule), the vertices step 3 keeps, and step 4 folded into the triangle flag
__global__ void __launch_bounds__(MP_BLOCK) k_mp_keep(const int32_t* __restrict__ tris, uint32_t T, uint32_t V, const uint8_t* __restrict__ remove,
                                                      const int32_t* __restrict__ clusters, const uint32_t* __restrict__ counts, uint32_t* __restrict__ record,
                                                      int flags, uint8_t* __restrict__ tflag, uint8_t* __restrict__ vflag)
{
    const uint32_t t = blockIdx.x * MP_BLOCK + threadIdx.x;
    if (t >= T) return;
    bool keep = true;
    if (remove) keep = remove[t] == 0;
    else if (clusters) keep = counts[clusters[t]] >= record[MP_R_THR];
    const int32_t i[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    if (!mp_in_range(i, V)) { atomicOr(record + MP_R_STATUS, (uint32_t)GSR_MESH_ERR_INDEX); keep = false; }
    if (keep && (flags & GSR_MESH_DROP_UNREFERENCED)) { vflag[i[0]] = 1; vflag[i[1]] = 1; vflag[i[2]] = 1; }      // racing stores of the same byte
    if ((flags & GSR_MESH_DROP_DEGENERATE) && (i[0] == i[1] || i[1] == i[2] || i[2] == i[0])) keep = false;
    tflag[t] = keep ? 1 : 0;
}

// output triangle j = source triangle tmap[j], its indices renumbered by vrank where vertices were dropped
__global__ void __launch_bounds__(MP_BLOCK) k_mp_emit(const int32_t* __restrict__ tris, uint32_t n_out, uint32_t T, uint32_t V, const uint32_t* __restrict__ tmap,
                                                      const uint32_t* __restrict__ vrank, int32_t* __restrict__ out)
{
    const uint32_t j = blockIdx.x * MP_BLOCK + threadIdx.x;
    if (j >= n_out) return;
    const uint32_t t = tmap[j];
    if (t >= T) return;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int32_t i = tris[3 * (size_t)t + q];
        out[3 * (size_t)j + q] = (vrank && (uint32_t)i < V) ? (int32_t)vrank[i] : i;
    }
}

// ------------------------------------------------------------------------------------------------ C ABI (include/gsrast.h)
struct MpScratch {
    MpTable tb;
    uint32_t *parent, *root, *rank, *counts, *sums, *tmap, *sel, *sel_status, *vrank, *vmap;
    int32_t* clusters;
    uint8_t *tflag, *vflag;
    size_t table_bytes, bytes;
};
static MpScratch mp_carve(uint64_t T, uint64_t V, const void* base)
{
    MpScratch m; GsrCarve c(base);
    const uint64_t t = T > 0 ? T : 1, n = t > V ? t : V;
    unsigned long long slots = 64;
    while (slots < 2 * 3 * t) slots <<= 1;
    m.tb.mask = slots - 1;
    m.tb.keys = c.take<unsigned long long>(slots); m.tb.owner = c.take<uint32_t>(slots);
    m.table_bytes = c.bytes();                      // keys and owners are contiguous: one fill with 0xFF
    m.parent = c.take<uint32_t>(t); m.root = c.take<uint32_t>(t); m.rank = c.take<uint32_t>(t); m.counts = c.take<uint32_t>(t);
    m.clusters = c.take<int32_t>(t); m.tmap = c.take<uint32_t>(t); m.tflag = c.take<uint8_t>(t);
    m.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    m.sel_status = c.take<uint32_t>(64); m.sel = c.take<uint32_t>(GSR_SELECT_STATE_BYTES / 4);      // contiguous: one clear; the select's rank-beyond-keys flag stays out of the record
    m.vflag = c.take<uint8_t>(V); m.vrank = c.take<uint32_t>(V); m.vmap = c.take<uint32_t>(V);
    m.bytes = c.bytes();
    return m;
}
static bool mp_sizes_ok(const char* who, int64_t T, int64_t V)
{
    if (T < 0 || V < 0 || V > 0x7FFFFFFFll) { gsr_set_error("%s: %lld triangles / %lld vertices out of range", who, (long long)T, (long long)V); return false; }
    if (3 * (unsigned long long)T >= (1ull << 31)) {
        gsr_set_error("%s: %lld triangles: 3T reaches 2^31, the half-edges no longer fit a 32-bit index; filter the mesh in parts", who, (long long)T); return false;
    }
    return true;
}
extern "C" size_t gsr_mesh_post_scratch_bytes(int64_t n_triangles, int64_t n_vertices)
{
    if (n_triangles < 0 || n_vertices < 0 || n_vertices > 0x7FFFFFFFll || 3 * (unsigned long long)n_triangles >= (1ull << 31)) return 0;
    return mp_carve((uint64_t)n_triangles, (uint64_t)n_vertices, nullptr).bytes;
}
static uint32_t mp_grid(uint32_t n) { return gsr_div_up(n > 0 ? n : 1u, MP_BLOCK); }

// components -> clusters / counts (/ area); *status_dev |= errors, *c_dev = C.  counts and area hold T entries.
static int mp_cluster(const char* who, const int32_t* tris, uint32_t T, uint32_t V, const float* verts, const MpScratch& m, int32_t* clusters, uint32_t* counts, double* area,
                      uint32_t* status_dev, uint32_t* c_dev, hipStream_t s)
{
    if (gsr_memset_async(m.tb.keys, 0xFF, m.table_bytes, s) || gsr_memset_async(counts, 0, (size_t)T * 4, s) ||
        (area && T > 0 && gsr_memset_async(area, 0, (size_t)T * 8, s))) { gsr_set_error("%s: clear", who); return 1; }
    const uint32_t g = mp_grid(T);
    hipLaunchKernelGGL(k_mp_insert, dim3(g), dim3(MP_BLOCK), 0, s, tris, T, V, m.tb, m.parent, status_dev);
    hipLaunchKernelGGL(k_mp_union, dim3(g), dim3(MP_BLOCK), 0, s, tris, T, V, m.tb, m.parent, status_dev);
    hipLaunchKernelGGL(k_mp_flatten, dim3(g), dim3(MP_BLOCK), 0, s, m.parent, T, m.root, m.tflag);
    gsr_rows_keep_scan(m.tflag, T, m.sums, nullptr, m.rank, c_dev, s);
    hipLaunchKernelGGL(k_mp_label, dim3(g), dim3(MP_BLOCK), 0, s, tris, T, V, verts, m.root, m.rank, clusters, counts, area);
    return 0;
}

extern "C" int gsr_mesh_cluster_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const float* vertices, int32_t* triangle_clusters,
                                          int32_t* cluster_n_triangles, double* cluster_area, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "mesh_cluster_triangles";
    if (!mp_sizes_ok(who, n_triangles, n_vertices)) return 1;
    if (!status_dev || !scratch || (n_triangles > 0 && (!triangles || !triangle_clusters || !cluster_n_triangles))) { gsr_set_error("%s: null pointer", who); return 1; }
    if (cluster_area && !vertices) { gsr_set_error("%s: the areas need the vertices", who); return 1; }
    const MpScratch m = mp_carve((uint64_t)n_triangles, 0, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 8, s)) { gsr_set_error("%s: status", who); return 1; }
    if (n_triangles == 0) return gsr_check_launch(who, s, false);
    if (mp_cluster(who, triangles, (uint32_t)n_triangles, (uint32_t)n_vertices, cluster_area ? vertices : nullptr, m, triangle_clusters, (uint32_t*)cluster_n_triangles,
                   cluster_area, status_dev, status_dev + 1, s)) return 1;
    return gsr_check_launch(who, s, false);
}

static int mp_filter_args(const char* who, const gsr_mesh_filter* f, const void* scratch, size_t scratch_bytes, MpScratch& m)
{
    if (!f) { gsr_set_error("%s: null filter", who); return 1; }
    if (!mp_sizes_ok(who, f->n_triangles, f->n_vertices)) return 1;
    if (!scratch || (f->n_triangles > 0 && !f->triangles)) { gsr_set_error("%s: null pointer", who); return 1; }
    if (f->flags & ~(GSR_MESH_DROP_UNREFERENCED | GSR_MESH_DROP_DEGENERATE)) { gsr_set_error("%s: unknown flags %d", who, f->flags); return 1; }
    if (f->remove_mask && f->cluster_to_keep != 0) { gsr_set_error("%s: a remove mask and cluster_to_keep exclude each other", who); return 1; }
    if (f->cluster_to_keep < 0 || f->floor < 0) { gsr_set_error("%s: cluster_to_keep and floor must not be negative", who); return 1; }
    m = mp_carve((uint64_t)f->n_triangles, (uint64_t)f->n_vertices, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    return 0;
}

extern "C" int gsr_mesh_filter_count(const gsr_mesh_filter* f, void* scratch, size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "mesh_filter_count";
    MpScratch m;
    if (mp_filter_args(who, f, scratch, scratch_bytes, m)) return 1;
    if (!record_dev) { gsr_set_error("%s: null record", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t T = (uint32_t)f->n_triangles, V = (uint32_t)f->n_vertices, g = mp_grid(T);
    const bool rule = f->cluster_to_keep > 0, unref = (f->flags & GSR_MESH_DROP_UNREFERENCED) != 0;
    if (gsr_memset_async(record_dev, 0, 32, s) ||
        (unref && V > 0 && gsr_memset_async(m.vflag, 0, gsr_align(V, 4), s))) { gsr_set_error("%s: clear", who); return 1; }
    if (rule) {
        if (T > 0 && mp_cluster(who, f->triangles, T, V, nullptr, m, m.clusters, m.counts, nullptr, record_dev + MP_R_STATUS, record_dev + MP_R_C, s)) return 1;
        // a cluster_to_keep beyond the clusters is the device's to report (GSR_MESH_ERR_KEEP): beyond T it cannot be a rank, and the select is left out
        const uint32_t rank[4] = { (uint32_t)f->cluster_to_keep - 1u, (uint32_t)f->cluster_to_keep - 1u, (uint32_t)f->cluster_to_keep - 1u, (uint32_t)f->cluster_to_keep - 1u };
        if ((uint32_t)f->cluster_to_keep <= T && gsr_memset_async(m.sel_status, 0, 256 + GSR_SELECT_STATE_BYTES, s)) { gsr_set_error("%s: clear", who); return 1; }
        if ((uint32_t)f->cluster_to_keep <= T) gsr_select(GSR_SELECT_U32_DESC, m.counts, T, record_dev + MP_R_C, rank, m.sel, m.sel_status, s);
    }
    hipLaunchKernelGGL(k_mp_finish, dim3(1), dim3(64), 0, s, record_dev, m.sel, rule ? 1 : 0, (uint32_t)f->cluster_to_keep, (uint32_t)f->floor, V);
    hipLaunchKernelGGL(k_mp_keep, dim3(g), dim3(MP_BLOCK), 0, s, f->triangles, T, V, f->remove_mask, rule ? m.clusters : nullptr, m.counts, record_dev, f->flags, m.tflag,
                       m.vflag);
    gsr_rows_keep_scan(m.tflag, T, m.sums, m.tmap, nullptr, record_dev + MP_R_T, s);
    if (unref) gsr_rows_keep_scan(m.vflag, V, m.sums, m.vmap, m.vrank, record_dev + MP_R_V, s);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_mesh_filter_emit(const gsr_mesh_filter* f, const void* scratch, size_t scratch_bytes, const uint32_t* record, int32_t n_rows, const gsr_rows_tensor* rows,
                                    int32_t* triangles_out, void* stream)
{
    const char* who = "mesh_filter_emit";
    MpScratch m;
    if (mp_filter_args(who, f, scratch, scratch_bytes, m)) return 1;
    if (!record) { gsr_set_error("%s: null record", who); return 1; }
    if (record[MP_R_STATUS]) { gsr_set_error("%s: the count reported status %u, nothing to emit", who, record[MP_R_STATUS]); return 1; }
    const uint32_t T = (uint32_t)f->n_triangles, V = (uint32_t)f->n_vertices, n_t = record[MP_R_T], n_v = record[MP_R_V];
    const bool unref = (f->flags & GSR_MESH_DROP_UNREFERENCED) != 0;
    if (n_t > T || n_v > V || (!unref && n_v != V)) { gsr_set_error("%s: the record does not belong to this mesh", who); return 1; }
    if (n_t > 0 && !triangles_out) { gsr_set_error("%s: null triangle output", who); return 1; }
    if (n_rows < 0 || (n_rows > 0 && (!rows || !unref))) { gsr_set_error("%s: vertex rows move only where unreferenced vertices are dropped", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<gsr_rows_item> items;
    for (int32_t i = 0; i < n_rows; i++) items.push_back({rows[i].src, rows[i].dst, nullptr, rows[i].row_bytes, 0, false});
    const gsr_rows_map map = {m.vmap, nullptr, n_v, 0u, V};
    if (n_rows > 0 && n_v > 0 && gsr_rows_move(who, map, n_rows, items.data(), true, s)) return 1;      // no vertex left: nothing to move, and dst may be NULL
    if (n_t > 0) hipLaunchKernelGGL(k_mp_emit, dim3(mp_grid(n_t)), dim3(MP_BLOCK), 0, s, f->triangles, n_t, T, V, m.tmap, unref ? m.vrank : nullptr, triangles_out);
    return gsr_check_launch(who, s, false);
}
