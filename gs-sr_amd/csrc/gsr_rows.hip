// gsr_rows.hip -- the row mover (gsr_common.h gsr_rows_move): one destination-driven copy kernel behind gsr_rows_compact_multi (below),
// gsr_densify_emit (gsr_densify.hip) and gsr_mesh_filter_emit (gsr_mesh_post.hip); and the keep scan that drives it (gsr_rows_keep_scan).  Output row r of every tensor of a table is src row map[r], zeros, or a row of the tensor's tail.
//
// Destination-driven because densify needs it (a split parent has several output rows: a scatter cannot serve) and because it writes whole
// lines: a lane owns one unit of consecutive output bytes, reads are contiguous over every run of surviving rows.
#include "gsr_compact.h"
#include <vector>

#define ROWS_MAX_T 24               // tensors per launch: the table travels in the kernel arguments
#define ROWS_CHUNK 2048             // copy units per block of 256 threads
#define ROWS_ZERO 0xFFFFFFFFu       // a lane's source: zeros / the tail; anything else is a row of src (< 2^31)
#define ROWS_TAIL 0xFFFFFFFEu
struct MoveEntry { const char* src; char* dst; const char* tail; uint64_t n_tail; uint32_t upr, ulog, first_block, zero_new; };     // upr: units per row
struct MoveTable { int32_t count; uint32_t n_map, n_carried, src_rows; MoveEntry e[ROWS_MAX_T]; };

template <typename T>
__device__ __forceinline__ void rows_copy(const MoveEntry& E, uint64_t base, const uint32_t* __restrict__ map, uint32_t n_map, uint32_t n_carried, uint32_t src_rows)
{
    const T* src = reinterpret_cast<const T*>(E.src);
    const T* tail = reinterpret_cast<const T*>(E.tail);
    T* dst = reinterpret_cast<T*>(E.dst);
    const uint64_t tail0 = (uint64_t)n_map * E.upr;
    const uint64_t end = min(tail0 + E.n_tail * E.upr, base + ROWS_CHUNK);
    if (base >= end) return;                                     // the grid is sized for the largest n_map: blocks beyond the real end leave
    const uint64_t row0 = base / E.upr;
    const uint32_t rem = (uint32_t)(base - row0 * E.upr);
    T zero;
    memset(&zero, 0, sizeof(T));
    constexpr int IT = ROWS_CHUNK / 256;
    // three passes over the lane's IT units, so that the IT map reads, then the IT row reads, are in flight together
    uint32_t srow[IT], col[IT];
    T v[IT];
#pragma unroll
    for (int j = 0; j < IT; j++) {
        const uint32_t k = threadIdx.x + j * 256, o = rem + k, dr = o / E.upr;
        const uint64_t row = row0 + dr;
        col[j] = o - dr * E.upr;
        srow[j] = ROWS_ZERO;
        if (base + k < end) {
            if (row >= n_map) srow[j] = tail ? ROWS_TAIL : ROWS_ZERO;
            else if (!(E.zero_new && row >= n_carried)) srow[j] = map[row];
        }
    }
#pragma unroll
    for (int j = 0; j < IT; j++) {
        v[j] = zero;
        if (srow[j] < src_rows) v[j] = src[(uint64_t)srow[j] * E.upr + col[j]];
        else if (srow[j] == ROWS_TAIL) v[j] = tail[base + threadIdx.x + j * 256 - tail0];
    }
#pragma unroll
    for (int j = 0; j < IT; j++) {
        const uint32_t k = threadIdx.x + j * 256;
        if (base + k < end) dst[base + k] = v[j];
    }
}

__global__ void __launch_bounds__(256) k_rows_move(MoveTable T, const uint32_t* __restrict__ map, const uint32_t* __restrict__ n_map_dev)
{
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < T.count; i++) k = (blockIdx.x >= T.e[i].first_block) ? i : k;
    const MoveEntry& E = T.e[k];
    const uint64_t base = (uint64_t)(blockIdx.x - E.first_block) * ROWS_CHUNK;
    const uint32_t n_map = n_map_dev ? *n_map_dev : T.n_map;
    if (E.ulog == 4) rows_copy<uint4>(E, base, map, n_map, T.n_carried, T.src_rows);
    else if (E.ulog == 3) rows_copy<uint2>(E, base, map, n_map, T.n_carried, T.src_rows);
    else rows_copy<uint32_t>(E, base, map, n_map, T.n_carried, T.src_rows);
}

// the widest of 16, 8 and 4 bytes that divides the row and every pointer
static uint32_t rows_ulog(const gsr_rows_item& a)
{
    const uintptr_t al = (uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.tail | (uintptr_t)a.row_bytes;
    return (al & 15) == 0 ? 4u : ((al & 7) == 0 ? 3u : 2u);
}

int gsr_rows_move(const char* who, const gsr_rows_map& m, int32_t count, const gsr_rows_item* t, bool launch, hipStream_t s)
{
    if (count < 0 || (count > 0 && !t)) { gsr_set_error("%s: bad table", who); return 1; }
    for (int32_t i = 0; i < count; i++) {
        const gsr_rows_item& a = t[i];
        if (a.row_bytes <= 0 || (a.row_bytes & 3) || a.n_tail < 0) { gsr_set_error("%s: tensor %d: row_bytes must be a positive multiple of 4, n_tail >= 0", who, i); return 1; }
        if (!a.dst || (m.src_rows > 0 && !a.src)) { gsr_set_error("%s: tensor %d: null pointer", who, i); return 1; }
        if (((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.tail) & 3) { gsr_set_error("%s: tensor %d: pointers must be 4-byte aligned", who, i); return 1; }
        if (((uint64_t)a.row_bytes >> rows_ulog(a)) * ROWS_CHUNK >= (1ull << 31)) { gsr_set_error("%s: tensor %d: row_bytes too large", who, i); return 1; }
    }
    int32_t i = 0;
    while (launch && i < count) {
        MoveTable T; T.count = 0; T.n_map = m.n_map; T.n_carried = m.n_carried; T.src_rows = m.src_rows;
        uint64_t blocks = 0;
        for (; i < count && T.count < ROWS_MAX_T; i++) {
            const gsr_rows_item& a = t[i];
            MoveEntry& E = T.e[T.count];
            E.src = (const char*)a.src; E.dst = (char*)a.dst; E.tail = (const char*)a.tail; E.n_tail = (uint64_t)a.n_tail;
            E.ulog = rows_ulog(a); E.upr = (uint32_t)(a.row_bytes >> E.ulog); E.zero_new = a.zero_new ? 1u : 0u;
            const uint64_t units = ((uint64_t)m.n_map + E.n_tail) * E.upr;
            if (units == 0) continue;
            E.first_block = (uint32_t)blocks;
            blocks += (units + ROWS_CHUNK - 1) / ROWS_CHUNK;
            if (blocks >= (1ull << 31)) { gsr_set_error("%s: tensor %d: too many bytes for one launch", who, i); return 1; }
            T.count++;
        }
        if (blocks) hipLaunchKernelGGL(k_rows_move, dim3((uint32_t)blocks), dim3(256), 0, s, T, m.map, m.n_map_dev);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- rows: compact + append
// dst = [src[keep] ; tail] for many tensors that share one keep mask over N rows (the reference's per-tensor x[mask] + cat over six parameters,
// twelve Adam moments and four accumulators: ~60 launches and a nonzero() synchronisation each).  The keep -> position scan runs once and leaves
// map[position] = row for every kept row; the row mover does the rest, with the number kept read on the device.
struct RowsKeepOp {
    const uint8_t* mask; uint32_t *map, *rank;
    __device__ bool keep(uint32_t i) const { return mask[i] != 0; }
    __device__ void place(uint32_t i, uint32_t p) const { if (map) map[p] = i; if (rank) rank[i] = p; }      // p <= i < N
};
void gsr_rows_keep_scan(const uint8_t* keep, uint32_t N, uint32_t* sums, uint32_t* map, uint32_t* rank, uint32_t* count_dev, hipStream_t s)
{
    gsr_compact(RowsKeepOp{keep, map, rank}, N, sums, count_dev, s);
}

struct RowsScratch { uint32_t *sums, *map, *count; size_t bytes; };
static RowsScratch rows_carve(uint32_t N, const void* base)
{
    RowsScratch r; GsrCarve c(base);
    const size_t n = N > 0 ? N : 1;
    r.sums = c.take<uint32_t>(gsr_compact_sums_words(n)); r.map = c.take<uint32_t>(n); r.count = c.take<uint32_t>(16);
    r.bytes = c.bytes();
    return r;
}
extern "C" size_t gsr_rows_compact_scratch_bytes(int64_t N)
{
    if (N < 0 || N >= (1ll << 31)) return 0;
    return rows_carve((uint32_t)N, nullptr).bytes;
}

extern "C" int gsr_rows_compact_multi(int64_t N, const uint8_t* keep, int32_t count, const gsr_rows_tensor* t, void* scratch, size_t scratch_bytes,
                                      void* stream)
{
    const char* who = "rows_compact_multi";
    if (N < 0 || N >= (1ll << 31)) { gsr_set_error("%s: N=%lld out of range", who, (long long)N); return 1; }
    if (N > 0 && !keep) { gsr_set_error("%s: keep is NULL", who); return 1; }
    const RowsScratch r = rows_carve((uint32_t)N, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, r.bytes, false)) return 1;
    std::vector<gsr_rows_item> items;
    for (int32_t i = 0; t && i < count; i++) items.push_back({t[i].src, t[i].dst, t[i].tail, t[i].row_bytes, t[i].n_tail, false});
    const gsr_rows_map m = {r.map, r.count, (uint32_t)N, 0u, (uint32_t)N};
    hipStream_t s = (hipStream_t)stream;
    if (gsr_rows_move(who, m, count, t ? items.data() : nullptr, false, s)) return 1;                      // the checks, before anything is launched
    gsr_rows_keep_scan(keep, (uint32_t)N, r.sums, r.map, nullptr, r.count, s);
    if (gsr_rows_move(who, m, count, t ? items.data() : nullptr, true, s)) return 1;
    return gsr_check_launch(who, s, false);
}
