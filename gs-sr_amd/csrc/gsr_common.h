// gsr_common.h -- private declarations shared by the HIP translation units of libgsrast_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/gsrast.h"

#define GSR_TILE 16            // tile edge in pixels (BLOCK_X/BLOCK_Y of the reference, config.h:16-17)
#define GSR_WAVE 64
#define GSR_SUB 8              // one wavefront owns an 8x8 sub-tile: 4 waves per 16x16 tile

// record stride (in float4) per variant, see DESIGN.md "data layout in HBM"
#define GSR_REC_EWA 3
#define GSR_REC_PLANE 4
#define GSR_REC_SURFEL 5
// backward accumulator: floats per gaussian row (STRIDE) and the part the kernels write (USED: EWA 9, PLANE 16, SURFEL 18 components, rounded up to
// float4s).  The rows are packed.  Round 4 measured power-of-two strides (EWA 16, SURFEL 32 floats), with which the 16-lane float atomic of the blend
// backward's flush stays inside one 64-byte line instead of straddling two for 50-84 % of the instructions (TCC_ATOMIC 1.85 M / 1.64 M line operations
// for 1.25 M / 0.89 M instructions): blend_bwd 0.4007 vs 0.4014 ms (SURFEL), 0.2793 vs 0.2791 (EWA), iterations 1.5 % / 0.4 % SLOWER (the preprocess
// backward reads and clears wider rows) -- the atomics are not what the kernel waits for.  -DGSR_ACC_SURFEL=32 -DGSR_ACC_EWA=16 rebuilds that variant.
#ifndef GSR_ACC_EWA
#define GSR_ACC_EWA 12
#endif
#define GSR_ACC_PLANE 16
#ifndef GSR_ACC_SURFEL
#define GSR_ACC_SURFEL 20
#endif
#define GSR_ACC_USED_EWA 12
#define GSR_ACC_USED_PLANE 16
#define GSR_ACC_USED_SURFEL 20

// radix sort geometry
#define GSR_SORT_THREADS 256
#define GSR_SORT_ITEMS 4
#define GSR_SORT_BLOCK (GSR_SORT_THREADS * GSR_SORT_ITEMS)
#define GSR_SCAN_BLOCK 1024

static inline __host__ __device__ int gsr_rec_stride(int variant)
{
    return variant == GSR_EWA ? GSR_REC_EWA : (variant == GSR_PLANE ? GSR_REC_PLANE : GSR_REC_SURFEL);
}
static inline __host__ __device__ int gsr_acc_stride(int variant)
{
    return variant == GSR_EWA ? GSR_ACC_EWA : (variant == GSR_PLANE ? GSR_ACC_PLANE : GSR_ACC_SURFEL);
}

static inline __host__ __device__ size_t gsr_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
static inline __host__ __device__ uint32_t gsr_div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Scratch carving: consecutive arrays, each starting on a 256-byte boundary of the caller's block.  With a NULL base only bytes() means
// anything (the *_scratch_bytes functions).
struct GsrCarve {
    char* base; size_t cur;
    explicit GsrCarve(const void* b) : base((char*)const_cast<void*>(b)), cur(0) {}
    template <typename T> T* take(size_t count) { T* r = reinterpret_cast<T*>(base + cur); cur += gsr_align(count * sizeof(T)); return r; }
    size_t bytes() const { return cur; }
};

// ---- arena views -------------------------------------------------------------------------------------------
struct GeomView {
    uint32_t* depth_key;      // [P]  bit pattern of view-space depth; 0xFFFFFFFF for culled gaussians
    uint32_t* tiles_touched;  // [P]
    ushort4* rect;            // [P]  tile rect {x0,y0,x1,y1}
    float4* cull;             // [2P] region of alpha >= 1/255.  EWA/PLANE {x,y,A,B},{C,2tau,-,-}; SURFEL {cx,cy,A,B},{C,r2,pix,piy}: ellipse form <= 1 or disc
    float4* rec;              // [P * stride] packed blend record
    uint32_t* clamped;        // [P]  3 bits: SH colour clamped to 0 per channel
    uint32_t* sorted_idx;     // [P]  gaussian ids in (depth, id) order
    uint32_t* offsets;        // [P]  BLOCK-LOCAL inclusive prefix of tiles_touched in depth order (k_offsets_local); the global prefix is offsets[i] + scan_tmp[i / GSR_SCAN_BLOCK]
    uint32_t* keys_b;         // [P]  sort ping-pong
    uint32_t* vals_a;         // [P]
    uint32_t* vals_b;         // [P]
    uint32_t* hist;           // [256 * nblk(P)]
    uint32_t* scan_tmp;       // [>= nblk]
    uint32_t* counters;       // [64] misc device scalars; [0] = num_rendered
    float* tw_z;              // [P]  SURFEL only (else nullptr): Tw.z = transMat[8], the float of rec[2].x once more, packed -- the one record word the preprocess
                              //      backward needs (its densification proxy); read out of the 80-byte records it cost a line fetch of the whole record array
    size_t bytes;
};
struct BinView {
    uint32_t* point_list;     // [R] final: gaussian id per instance, sorted by (tile, depth, id)
    uint32_t* tile_keys;      // [R] final: tile id per instance
    uint32_t* keys_b;         // [R]
    uint32_t* vals_b;         // [R]
    uint32_t* hist;           // [128 * nblk(R)]
    uint32_t* scan_tmp;
    uint32_t* tile_tab;       // [(rows + 1) * Tp] one-pass bucket sort on the tile id (gsr_binning.hip): instances per (16384-key chunk, tile), then the tiles' totals
    uint32_t cap;             // the R this view was carved for
    // per (tile, 64-entry batch of its list, 8x8 quadrant): the forward's sub-tile cull ballot, reused by the splat-parallel backward instead of
    // re-testing every entry against the four quadrants.  Word index ((range.x >> 6) + tile + batch) * 4 + quadrant (unique per tile and batch).
    unsigned long long* qmask;
    size_t bytes;
};
struct ImgView {
    float* final_T;           // [N] (SURFEL [3N]: T, M1, M2)
    uint32_t* n_contrib;      // [N] (SURFEL [2N]: last, median)
    uint2* ranges;            // [T]
    uint32_t* tile_order;     // [T + 1] launch order of the blend kernels: tiles by descending list length (gsr_binning.hip k_tile_order); word T: 1 = the
                              // order of THIS forward is in place (k_tile_order ran), 0 = blockIdx -> tile directly
    size_t bytes;
};

GeomView gsr_carve_geom(int variant, int P, void* base);
BinView gsr_carve_bin(int variant, uint32_t R, int W, int H, void* base);
ImgView gsr_carve_img(int variant, int W, int H, void* base);

// ---- error plumbing ----------------------------------------------------------------------------------------
void gsr_set_error(const char* fmt, ...);
int gsr_check_launch(const char* what, hipStream_t s, bool debug);
// the scratch block holds `need` bytes and, where the entry point's contract says so (`aligned`), starts on a 16-byte boundary; else the error is set and 1 returned
static inline int gsr_scratch_check(const char* who, const void* scratch, size_t given, size_t need, bool aligned = true)
{
    if (scratch && given >= need && !(aligned && ((uintptr_t)scratch & 15))) return 0;
    gsr_set_error("%s: scratch too small: scratch of %zu bytes%s needed, %zu given", who, need, aligned ? " (16-byte aligned)" : "", given);
    return 1;
}
#define GSR_CHECK(call, what)                                                                \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) { gsr_set_error("%s: %s", what, hipGetErrorString(e_)); return 1; } \
    } while (0)

// ---- stage launchers (each in its own .hip) ------------------------------------------------------------------
// How ONE forward runs: filled once by its entry point (gsr_api.hip, the only reader of the GSR_* switches and of the long-list feedback) and handed to
// every stage launcher, which derives nothing of its own.  The backward has no plan: it reads the lists the forward left.
struct FwdPlan {
    bool global_order;        // depth order: global stable sort of the gaussians by depth, or every tile's list sorted in the blend forward's prologue.  It fixes
                              // the layout of offsets / scan_tmp / sorted_idx in the geom arena, so the preprocess kernel records it IN the arena
                              // (GeomView::counters[GSR_CNT_MODE]); a later call on that arena (gsr_forward_stage2, also the redo after an overflowed
                              // gsr_forward) reads the record back and refuses an arena that carries none
    bool tile_cull;           // tile instances culled at emission (gsr_tile_cull.h): the preprocess kernel counts what k_duplicate emits, instance for instance
    bool tile_order;          // k_tile_order runs: the blend workgroups take the tiles longest list first
    uint32_t bucket_chunk;    // instances per chunk of the one-pass bucket sort on the tile id, 0: the two-pass radix sort.  Filled once the binning arena's
                              // capacity is known (stage 2); the preprocess and the depth order do not look at it
};
#define GSR_CNT_MODE 1
// counters[GSR_CNT_CULL_MISMATCH]: set by k_duplicate when a wave emitted a different number of instances than its gaussians counted in the preprocess kernel
// (both run gsr_tile_cull.h's test on the same words; a disagreement would shift every later instance of the list).  Cleared by the preprocess kernel, looked
// at by the forward when cfg->debug is set (it synchronises after every stage then; gsr_debug_read does not expose the word).
#define GSR_CNT_CULL_MISMATCH 2
#define GSR_MODE_TILE 0x47530001u
#define GSR_MODE_GLOBAL 0x47530002u
int gsr_launch_preprocess(const gsr_cfg* cfg, const gsr_inputs* in, GeomView g, int32_t* radii, hipStream_t s, const FwdPlan& plan, uint32_t* prefiltered_err = nullptr);
// global order: sorted_idx, offsets, the scanned block sums and counters[0]; per-tile order: nothing unless `need_total` (two-stage forward: the host
// sizes the binning arena from num_rendered) -- otherwise k_duplicate adds up the raw block sums and publishes the total itself
int gsr_launch_depth_order(const gsr_cfg* cfg, GeomView g, uint32_t* host_word_dev, hipStream_t s, const FwdPlan& plan, bool need_total);
int gsr_launch_binning(const gsr_cfg* cfg, GeomView g, BinView b, ImgView im, uint32_t R, const uint32_t* n_dev, hipStream_t s,
                       const FwdPlan& plan, uint32_t* host_word_dev = nullptr);
int gsr_launch_blend_fwd(const gsr_cfg* cfg, const gsr_inputs* in, GeomView g, BinView b, ImgView im,
                         const gsr_outputs* out, hipStream_t s, const FwdPlan& plan, uint32_t* status_dev = nullptr, uint32_t status_cap = 0u);
int gsr_launch_blend_bwd(const gsr_cfg* cfg, const gsr_inputs* in, GeomView g, BinView b, ImgView im,
                         const gsr_out_grads* og, float* acc, hipStream_t s);
void gsr_blend_bwd_attach_events(hipEvent_t start, hipEvent_t stop);     // the next gsr_launch_blend_bwd of this thread carries them on its dispatch (gsr_blend_sp.hip)
bool gsr_depth_order_static_rule(int P, int T, int variant);            // GSR_DEPTH_ORDER=auto: global above ~192 gaussians per tile (gsr_binning.hip)
// One-pass bucket sort on the tile id (per-tile depth order only: it leaves a tile's list in no particular order, which the sort by (depth, id) that
// follows does not mind).  Chunks of 4096 / 8192 / 16384 instances (the smallest that keeps the arena's capacity within GSR_TB_ROWS_MAX chunks: more
// workgroups for the scattered stores), a table of per-(chunk, tile) counts; applies up to GSR_TB_TILES_MAX tiles (the 16-bit counters of two tiles
// share an LDS word) and GSR_TB_ROWS_MAX chunks of 16384, else the two-pass radix sort (FwdPlan::bucket_chunk, gsr_api.hip).  GSR_TILE_BUCKET=0: never.
#define GSR_TB_ROWS_MAX 256u
#define GSR_TB_TILES_MAX 16384
static inline size_t gsr_tile_bucket_words(uint32_t cap, size_t T)
{
    if (T > (size_t)GSR_TB_TILES_MAX) return 0;
    const size_t Tp = (T + 1) & ~(size_t)1, rows = ((size_t)cap + 4095) / 4096;      // upper envelope over the three chunk sizes, monotone in cap:
    return ((rows < GSR_TB_ROWS_MAX ? rows : (size_t)GSR_TB_ROWS_MAX) + 1) * Tp;      // gsr_binning_capacity inverts gsr_binning_bytes by bisection
}
#define GSR_TB_GROUPS_MAX (GSR_TB_TILES_MAX / 64)       // behind the table (BinView::tile_tab + gsr_tile_bucket_words(cap, T)): per chunk, the exclusive prefix of its
                                                        // instances over the groups of 64 tiles, [GSR_TB_ROWS_MAX][GSR_TB_GROUPS_MAX]
const uint32_t* gsr_static_tile_map(int gx, int gy, hipStream_t s);     // device [gx*gy] blockIdx -> tile, block-cyclic over the XCDs; cached per device and grid; nullptr if unavailable (gsr_api.hip)
uint32_t* gsr_long_list_word();       // device pointer of the per-device feedback word the blend forward reports long lists into, or nullptr (gsr_api.hip)
// hipMemsetAsync that is safe to record into a HIP graph: on ROCm 7.2 a memset NODE replays with a corrupted fill value from the second replay
// on (measured round 3: vis_idx filled with 0x5A5A5A5A instead of 0xFF...), so while `s` is being captured the fill is a kernel; eagerly it is
// the runtime's memset.  nbytes must be a multiple of 4.
int gsr_memset_async(void* p, int byte_value, size_t nbytes, hipStream_t s);
int gsr_launch_preprocess_bwd(const gsr_cfg* cfg, const gsr_inputs* in, const int32_t* radii, GeomView g,
                              float* acc, const gsr_in_grads* ig, bool leave_zero, hipStream_t s);

// generic device-wide primitives, each with the unit that holds it.  What a caller of the radix sort (gsr_binning.hip) needs is in gsr_sort.h.
#include "gsr_sort.h"
// In-place exclusive scan of `rows` rows of n words (row r at data + r * stride), one block per row, n small (block sums): k_scan_small.  Row r's
// total goes to totals[r] and, where given, to totals2[r] as well.
void gsr_scan_small(uint32_t* data, uint32_t n, uint32_t rows, uint32_t stride, uint32_t* totals, uint32_t* totals2, hipStream_t s);

// The row mover (gsr_rows.hip): for every tensor of a host table, one launch per 24 tensors,
//   dst row r = src row map[r]            r < n_map         (zeros instead where zero_new and r >= n_carried; nothing is read for those)
//             = tail row r - n_map        n_map <= r < n_map + n_tail   (zeros where tail is NULL)
// n_map is read from *n_map_dev where that is given; n_map is then the most it can be and sizes the grid.  src has src_rows rows.
struct gsr_rows_item { const void* src; void* dst; const void* tail; int64_t row_bytes, n_tail; bool zero_new; };
struct gsr_rows_map { const uint32_t* map; const uint32_t* n_map_dev; uint32_t n_map, n_carried, src_rows; };
// Checks the table (errors are prefixed with `who`), then launches unless !launch: an entry point with kernels of its own in front validates first.
int gsr_rows_move(const char* who, const gsr_rows_map& m, int32_t count, const gsr_rows_item* t, bool launch, hipStream_t s);
// The count / scan / place compaction (gsr_compact.h): workgroups of GSR_COMPACT_BLOCK elements, one word of `sums` each and one for the total.
#define GSR_COMPACT_BLOCK 1024
static inline size_t gsr_compact_sums_words(size_t n) { return (n > 0 ? (n + GSR_COMPACT_BLOCK - 1) / GSR_COMPACT_BLOCK : 1) + 1; }
// The keep scan of the row compaction on its own (gsr_rows.hip): for every i < N with keep[i], p = the number of kept rows in front of it;
// map[p] = i and rank[i] = p (either may be NULL), *count_dev = the number kept.  sums: gsr_compact_sums_words(N) words.
void gsr_rows_keep_scan(const uint8_t* keep, uint32_t N, uint32_t* sums, uint32_t* map, uint32_t* rank, uint32_t* count_dev, hipStream_t s);

// The radix select (gsr_init.hip): up to four order statistics of one array, MSB first, 8 bits per pass: four times a histogram kernel and
// a one-workgroup advance.  rank[t] is 0-based in ascending key order; the keys are the first min(n, *n_dev) values (n alone where n_dev is
// NULL).  GSR_SELECT_FLOAT: float32 values (a NaN sets GSR_INIT_ERR_NONFINITE in *status); GSR_SELECT_U32_DESC: uint32 values in
// DESCENDING order, so that rank k - 1 is the k-th largest.  Afterwards word t of `state` holds the KEY of rank t: the float's bit pattern
// folded to unsigned order, or the complement of the uint32 value.  A rank beyond the keys sets GSR_INIT_ERR_RANK in *status.  The caller
// clears the GSR_SELECT_STATE_BYTES of `state` and *status on the stream beforehand.
#define GSR_SELECT_FLOAT 0
#define GSR_SELECT_U32_DESC 1
#define GSR_SELECT_STATE_BYTES (2 * 256 + 4 * 256 * 4)
void gsr_select(int kind, const void* values, uint32_t n, const uint32_t* n_dev, const uint32_t rank[4], uint32_t* state, uint32_t* status, hipStream_t s);

// The exact nearest-neighbour search (gsr_chamfer.hip) in its two halves: the grid over T targets built into gsr_np_scratch_bytes(T) bytes of
// caller-owned scratch, and any number of queries against it.  max_dist is the same number for both (the cell size depends on it; < 0: none).
// skip (nullable): a device word; while it is non-zero a query's workgroups return at once and write nothing.  Arguments are the caller's to check.
size_t gsr_np_scratch_bytes(uint64_t T);
int gsr_np_build(const char* who, const float* target, uint32_t T, float max_dist, void* scratch, hipStream_t s);
void gsr_np_query(const float* query, uint32_t Q, uint32_t T, float max_dist, const void* scratch, float* d2, int32_t* index, const uint32_t* skip, hipStream_t s);
