// gsr_anchor.hip -- Scaffold-GS / Octree-GS densification geometry on the device (include/gsrast.h gsr_anchor_*).
//
// One growing level (ScaffoldGaussian.anchor_growing, gssr/gaussian/scaffold_gaussian.py:555-649; the loop body of OctreeGaussian.anchor_growing,
// octree_gaussian.py:401-534): the reference compares every unique candidate cell against every anchor (O(U N), chunks of 4096), after a
// torch.unique(dim=0) and before a scatter_max.  Here the cells of the admitted anchors and of the candidate slots are packed into 64-bit keys
// (21 bits per axis + a tag bit that puts an occupied entry in front of the candidates of its cell) and sorted together by the radix sort
// (gsr_sort.h: low word, then stable by the high word); a run of equal cells that STARTS with a candidate is a new anchor.  Run heads come out in key
// order = lexicographic signed (x, y, z), the order of torch.unique(dim=0).  Everything is integer compares and maxima: bitwise deterministic.
//
// This unit is built with -ffp-contract=off: the cell of a point is an integer output and must not depend on FMA contraction.
#include "gsr_common.h"
#include "gsr_compact.h"
#include <cmath>

#define ANC_BIAS 1048576            // 2^20: cells in [-2^20, 2^20 - 1] per axis
#define ANC_CNT_ENTRIES 0           // counters: entries in the sort
#define ANC_CNT_HEADS 1             //           new anchors
#define ANC_CNT_FOUND 2             //           new anchors before the weed-out (gsr_anchor_level_find_weed)
#define WEED_BLOCK 256
#define WEED_CHUNK GSR_OCTREE_WEED_CHUNK      // cameras staged in LDS at a time (16 bytes each)

// ---------------------------------------------------------------------------------------------------------------- entries of a level
// c = rint((p - origin) / cell): round-half-even, IEEE division (no reciprocal), every operation rounded on its own
__device__ __forceinline__ bool anc_cell_key(float px, float py, float pz, const gsr_anchor_level& L, uint64_t* key63)
{
    const float rx = rintf(__fdiv_rn(px - L.origin[0], L.cell)), ry = rintf(__fdiv_rn(py - L.origin[1], L.cell)),
                rz = rintf(__fdiv_rn(pz - L.origin[2], L.cell));
    const float lo = -(float)ANC_BIAS, hi = (float)(ANC_BIAS - 1);
    if (!(rx >= lo && rx <= hi && ry >= lo && ry <= hi && rz >= lo && rz <= hi)) return false;       // NaN and infinities fail too
    const uint64_t ux = (uint64_t)((int)rx + ANC_BIAS), uy = (uint64_t)((int)ry + ANC_BIAS), uz = (uint64_t)((int)rz + ANC_BIAS);
    *key63 = (ux << 42) | (uy << 21) | uz;
    return true;
}

// Entry i of the level: i < Na the cell of anchor i (tag 0), otherwise candidate slot i - Na (tag 1).  Returns whether the entry takes part.
// occupy [N0] (Octree-GS: occupancy apart from candidacy) or NULL: an original anchor occupies its cell iff occupy[i], where NULL iff the mask admits it.
__device__ __forceinline__ bool anc_entry(uint32_t i, const gsr_anchor_level& L, const uint8_t* __restrict__ occupy, uint64_t* key, uint32_t* status)
{
    const uint32_t Na = (uint32_t)L.Na, N0 = (uint32_t)L.N0;
    uint64_t k63;
    if (i < Na) {
        if (i < N0 && (occupy ? !occupy[i] : (L.mask && !L.mask[i]))) return false;
        // an anchor outside the packing range cannot share a cell with a candidate inside it: it is left out, not an error
        if (!anc_cell_key(L.anchor[3 * (size_t)i], L.anchor[3 * (size_t)i + 1], L.anchor[3 * (size_t)i + 2], L, &k63)) return false;
        *key = k63 << 1;
        return true;
    }
    const uint32_t j = i - Na, a = j / (uint32_t)L.k;
    const float g = L.grads[j];
    // an infinite thr_hi is no upper bound (Scaffold-GS, Octree pass B: `grads >= threshold` alone): a gradient of +inf is a candidate; NaN never is
    if (!(g >= L.thr_lo && (g < L.thr_hi || L.thr_hi == INFINITY)) || !L.offset_mask[j]) return false;
    if (L.rand && !(L.rand[j] > L.rand_thr)) return false;
    if (L.mask && !L.mask[a]) return false;
    const float* sc = L.scaling + (size_t)a * L.scaling_stride;
    const float mx = L.offset[3 * (size_t)j] * sc[0], my = L.offset[3 * (size_t)j + 1] * sc[1], mz = L.offset[3 * (size_t)j + 2] * sc[2];
    const float px = L.anchor[3 * (size_t)a] + mx, py = L.anchor[3 * (size_t)a + 1] + my, pz = L.anchor[3 * (size_t)a + 2] + mz;
    if (!anc_cell_key(px, py, pz, L, &k63)) { atomicOr(status + 1, 1u); return false; }      // sticky: the cell does not fit 21 bits per axis
    *key = (k63 << 1) | 1u;
    return true;
}

// the compaction (gsr_compact.h) of the entries that take part: anc_entry runs in both passes (its sticky atomicOr is idempotent)
struct AncEntryOp {
    gsr_anchor_level L; const uint8_t* occupy; uint32_t *status, *key_lo, *key_hi, *sort_keys, *src;
    uint64_t key;
    __device__ bool keep(uint32_t i) { return anc_entry(i, L, occupy, &key, status); }
    // pos < capacity: at most one position per entry
    __device__ void place(uint32_t i, uint32_t pos) const { key_lo[pos] = (uint32_t)key; sort_keys[pos] = (uint32_t)key; key_hi[pos] = (uint32_t)(key >> 32); src[pos] = i; }
};

// sorted position p starts a new anchor iff it holds a candidate and the entry before it lies in another cell (occupied entries lead their run)
__device__ __forceinline__ bool anc_is_head(uint32_t p, uint32_t n, const uint32_t* __restrict__ hi, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_lo)
{
    if (p >= n) return false;
    const uint64_t k = gsr_sort_key64(hi, perm, key_lo, p);
    if (!(k & 1u)) return false;
    if (p == 0) return true;
    const uint64_t q = gsr_sort_key64(hi, perm, key_lo, p - 1);
    return (q >> 1) != (k >> 1);
}

struct AncHeadOp {
    const uint32_t *n_dev, *hi, *perm, *key_lo; uint32_t* head_pos;
    __device__ bool keep(uint32_t p) const { return anc_is_head(p, *n_dev, hi, perm, key_lo); }
    __device__ void place(uint32_t p, uint32_t q) const { head_pos[q] = p; }      // q <= p < capacity
};

__global__ void __launch_bounds__(64) k_anc_publish(const uint32_t* __restrict__ counters, uint32_t* __restrict__ status)
{
    if (threadIdx.x == 0) status[0] = counters[ANC_CNT_HEADS];
}

// ---------------------------------------------------------------------------------------------------------------- Octree-GS weed-out
// OctreeGaussian.weed_out (octree_gaussian.py:203-214): the number of cameras that would show a new anchor of level lv at p.  Per camera
//   d = sqrt(((dx^2 + dy^2) + dz^2)) * scale;  pred = log2(standard_dist / d) / log2(fork);  il = clamp(floor | rint | ceil (pred), 0, levels - 1)
// in float32, every operation rounded on its own (this unit is built without FMA contraction), the clamp applied before the conversion.
// The whole block calls this: cameras are staged through LDS in chunks of WEED_CHUNK and every lane reads the same address (a broadcast).
struct WeedArgs { const float* cam; int32_t C, levels, mode; float standard_dist, log2_fork, visible_threshold; };

__device__ __forceinline__ uint32_t weed_visible(bool active, float px, float py, float pz, int32_t lv, const WeedArgs& W, float4* cams)
{
    uint32_t visible = 0;
    const float top = (float)(W.levels - 1);
    for (int32_t c0 = 0; c0 < W.C; c0 += WEED_CHUNK) {
        const int32_t nc = min(WEED_CHUNK, W.C - c0);
        for (int32_t c = threadIdx.x; c < nc; c += blockDim.x) {
            const float* q = W.cam + 4 * (size_t)(c0 + c);
            cams[c] = make_float4(q[0], q[1], q[2], q[3]);
        }
        __syncthreads();
        if (active) {
            for (int32_t c = 0; c < nc; c++) {
                const float4 cam = cams[c];
                const float dx = px - cam.x, dy = py - cam.y, dz = pz - cam.z;
                const float d = __fsqrt_rn((dx * dx + dy * dy) + dz * dz) * cam.w;
                const float pred = __fdiv_rn(log2f(__fdiv_rn(W.standard_dist, d)), W.log2_fork);
                float r = W.mode == 0 ? floorf(pred) : (W.mode == 1 ? rintf(pred) : ceilf(pred));
                r = fminf(fmaxf(r, 0.0f), top);                     // the clamp, before the conversion
                visible += (lv <= (int32_t)r) ? 1u : 0u;
            }
        }
        __syncthreads();
    }
    return visible;
}
__device__ __forceinline__ bool weed_keep(uint32_t visible, const WeedArgs& W)
{
    return __fdiv_rn((float)visible, (float)W.C) > W.visible_threshold;
}

__global__ void __launch_bounds__(WEED_BLOCK) k_weed_rows(WeedArgs W, uint32_t U, const float* __restrict__ pos, const int32_t* __restrict__ level,
                                                          int32_t* __restrict__ visible_count, uint8_t* __restrict__ keep)
{
    __shared__ float4 cams[WEED_CHUNK];
    const uint32_t i = blockIdx.x * WEED_BLOCK + threadIdx.x;
    const bool active = i < U;
    float px = 0.f, py = 0.f, pz = 0.f; int32_t lv = 0;
    if (active) { px = pos[3 * (size_t)i]; py = pos[3 * (size_t)i + 1]; pz = pos[3 * (size_t)i + 2]; lv = level[i]; }
    const uint32_t v = weed_visible(active, px, py, pz, lv, W, cams);
    if (active) { visible_count[i] = (int32_t)v; keep[i] = weed_keep(v, W) ? 1 : 0; }
}

// One thread per numbered head: flag[q] = the cell's position survives the weed-out; head_pos is copied to `heads` so that the compaction can
// write it back in place.  The head count is read on the device; the grid covers the worst case and surplus blocks leave.
__global__ void __launch_bounds__(WEED_BLOCK) k_anc_weed_flag(gsr_anchor_level L, WeedArgs W, int32_t lv, const uint32_t* __restrict__ counters,
                                                              const uint32_t* __restrict__ hi, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_lo,
                                                              const uint32_t* __restrict__ head_pos, uint32_t* __restrict__ heads, uint32_t* __restrict__ flag)
{
    __shared__ float4 cams[WEED_CHUNK];
    const uint32_t n_heads = counters[ANC_CNT_HEADS];
    if (blockIdx.x * WEED_BLOCK >= n_heads) return;                 // the whole block
    const uint32_t q = blockIdx.x * WEED_BLOCK + threadIdx.x;
    const bool active = q < n_heads;
    float px = 0.f, py = 0.f, pz = 0.f;
    uint32_t p = 0;
    if (active) {
        p = head_pos[q];
        const uint64_t cellkey = gsr_sort_key64(hi, perm, key_lo, p) >> 1;
        const int cx = (int)((cellkey >> 42) & 0x1FFFFFu) - ANC_BIAS, cy = (int)((cellkey >> 21) & 0x1FFFFFu) - ANC_BIAS, cz = (int)(cellkey & 0x1FFFFFu) - ANC_BIAS;
        const float ax = (float)cx * L.cell, ay = (float)cy * L.cell, az = (float)cz * L.cell;       // as k_anc_emit writes it
        px = ax + L.origin[0]; py = ay + L.origin[1]; pz = az + L.origin[2];
    }
    const uint32_t v = weed_visible(active, px, py, pz, lv, W, cams);
    if (active) { heads[q] = p; flag[q] = weed_keep(v, W) ? 1u : 0u; }
}

// the heads whose flag is set, back into head_pos
struct AncWeedOp {
    const uint32_t *counters, *flag, *heads; uint32_t* head_pos;
    __device__ bool keep(uint32_t q) const { return q < counters[ANC_CNT_HEADS] && flag[q]; }
    __device__ void place(uint32_t q, uint32_t w) const { head_pos[w] = heads[q]; }      // w <= q < capacity
};

// the weeded count takes the place of the head count (gsr_anchor_level_emit reads it); status = {final, overflow (sticky), found before the weed-out}
__global__ void __launch_bounds__(64) k_anc_publish_weed(uint32_t* __restrict__ counters, uint32_t* __restrict__ status, int weeded)
{
    if (threadIdx.x == 0) {
        const uint32_t found = counters[ANC_CNT_HEADS];
        if (weeded) counters[ANC_CNT_HEADS] = counters[ANC_CNT_FOUND];
        status[0] = counters[ANC_CNT_HEADS];
        status[2] = found;
    }
}

// new_anchor = float(c) * cell + origin (a multiply, then an add); new_feat = element-wise maximum of anchor_feat over the run's candidates
__global__ void __launch_bounds__(256) k_anc_emit(gsr_anchor_level L, uint32_t count, const uint32_t* __restrict__ counters, const uint32_t* __restrict__ hi,
                                                  const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_lo, const uint32_t* __restrict__ src,
                                                  const uint32_t* __restrict__ head_pos, float* __restrict__ new_anchor, float* __restrict__ new_feat)
{
    const uint32_t F = (uint32_t)L.F, per = F > 0 ? F : 1u;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t q = (uint32_t)(t / per), f = (uint32_t)(t % per);
    if (q >= count || q >= counters[ANC_CNT_HEADS]) return;
    const uint32_t n = counters[ANC_CNT_ENTRIES];
    uint32_t p = head_pos[q];
    const uint64_t cellkey = gsr_sort_key64(hi, perm, key_lo, p) >> 1;
    if (f == 0) {
        const int cx = (int)((cellkey >> 42) & 0x1FFFFFu) - ANC_BIAS, cy = (int)((cellkey >> 21) & 0x1FFFFFu) - ANC_BIAS, cz = (int)(cellkey & 0x1FFFFFu) - ANC_BIAS;
        const float ax = (float)cx * L.cell, ay = (float)cy * L.cell, az = (float)cz * L.cell;
        new_anchor[3 * (size_t)q] = ax + L.origin[0]; new_anchor[3 * (size_t)q + 1] = ay + L.origin[1]; new_anchor[3 * (size_t)q + 2] = az + L.origin[2];
    }
    if (F == 0) return;
    float m = 0.f;
    bool first = true;
    for (; p < n; p++) {                                         // every entry of the run is a candidate: an occupied entry would have led it
        const uint32_t e = perm[p];
        if (!first && ((((uint64_t)hi[p] << 32) | key_lo[e]) >> 1) != cellkey) break;
        const uint32_t a = (src[e] - (uint32_t)L.Na) / (uint32_t)L.k;
        const float v = L.anchor_feat[(size_t)a * F + f];
        m = (first || v > m) ? v : m;
        first = false;
    }
    new_feat[(size_t)q * F + f] = m;
}

struct AncScratch { uint32_t *sums, *key_lo, *key_hi, *src, *counters; GsrSortBuf so; size_t bytes; };
static AncScratch anc_carve(uint32_t cap, const void* base)
{
    AncScratch a; GsrCarve c(base);
    const size_t n = cap > 0 ? cap : 1;
    a.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    a.key_lo = c.take<uint32_t>(n); a.key_hi = c.take<uint32_t>(n); a.src = c.take<uint32_t>(n);
    a.so = gsr_sort_carve(c, n);
    a.counters = c.take<uint32_t>(16);
    a.bytes = c.bytes();
    return a;
}
// What the two 32-bit sorts of anc_find leave where, for anc_find and for gsr_anchor_level_emit, which carves the same block again in a later call:
// the high words and the order, and the free pair, which takes the run heads and (weed-out) their flags.
struct AncSorted { uint32_t *hi, *perm, *head_pos, *flag; };
static AncSorted anc_sorted(const AncScratch& a)
{
    GsrSort st(a.so);
    st.advance(32); st.advance(32);
    return { st.keys, st.order, st.free_keys, st.free_order };
}

static int anc_check(const gsr_anchor_level* lv, const char* who, uint32_t* cap)
{
    if (!lv) { gsr_set_error("%s: level is NULL", who); return 1; }
    if (lv->N0 < 0 || lv->Na < lv->N0) { gsr_set_error("%s: bad sizes Na=%d N0=%d", who, lv->Na, lv->N0); return 1; }
    if (lv->k < 1) { gsr_set_error("%s: n_offsets k=%d must be >= 1", who, lv->k); return 1; }
    if (lv->F < 0) { gsr_set_error("%s: feat_dim F=%d must be >= 0", who, lv->F); return 1; }
    if (lv->scaling_stride < 3) { gsr_set_error("%s: scaling_stride=%d must be >= 3", who, lv->scaling_stride); return 1; }
    if (!(lv->cell > 0.0f) || !(lv->cell < 3.0e38f)) { gsr_set_error("%s: cell must be a positive finite number", who); return 1; }
    const uint64_t c = (uint64_t)lv->Na + (uint64_t)lv->N0 * (uint64_t)lv->k;
    if (c >= (1ull << 31)) { gsr_set_error("%s: Na + N0 * k = %llu entries exceed 2^31", who, (unsigned long long)c); return 1; }
    if (lv->Na && !lv->anchor) { gsr_set_error("%s: anchor is NULL", who); return 1; }
    if (lv->N0 && (!lv->offset || !lv->scaling || !lv->grads || !lv->offset_mask || (lv->F && !lv->anchor_feat))) {
        gsr_set_error("%s: offset / scaling / anchor_feat / grads / offset_mask must be provided", who); return 1;
    }
    *cap = (uint32_t)c;
    return 0;
}

extern "C" size_t gsr_anchor_level_scratch_bytes(int32_t Na, int32_t N0, int32_t k)
{
    if (Na < 0 || N0 < 0 || k < 1) return 0;
    const uint64_t c = (uint64_t)Na + (uint64_t)N0 * (uint64_t)k;
    if (c >= (1ull << 31)) return 0;
    return anc_carve((uint32_t)c, nullptr).bytes;
}

static int weed_check(const gsr_octree_weed* w, const char* who, WeedArgs* W)
{
    if (!w) { gsr_set_error("%s: weed is NULL", who); return 1; }
    if (w->C < 1 || !w->cam_infos) { gsr_set_error("%s: cam_infos must hold at least one camera", who); return 1; }
    if (w->levels < 1) { gsr_set_error("%s: levels=%d must be >= 1", who, w->levels); return 1; }
    if (w->mode == 3) { gsr_set_error("%s: dist2level 'progressive' is not supported by the weed-out", who); return 1; }
    if (w->mode < 0 || w->mode > 2) { gsr_set_error("%s: Unknown dist2level: %d", who, w->mode); return 1; }
    if (!(w->fork > 1.0f) || !(w->standard_dist > 0.0f)) { gsr_set_error("%s: fork must exceed 1 and standard_dist must be positive", who); return 1; }
    *W = {w->cam_infos, w->C, w->levels, w->mode, w->standard_dist, (float)log2((double)w->fork), w->visible_threshold};
    return 0;
}

// three_words: the caller's status_dev holds the third word (found before the weed-out); gsr_anchor_level_find's holds two
static int anc_find(const char* who, const gsr_anchor_level* lv, const uint8_t* occupy, const gsr_octree_weed* weed, bool three_words, void* scratch,
                    size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    uint32_t cap;
    WeedArgs W = {};
    if (anc_check(lv, who, &cap)) return 1;
    if (weed && weed_check(weed, who, &W)) return 1;
    if (!status_dev) { gsr_set_error("%s: status_dev is NULL", who); return 1; }
    const AncScratch a = anc_carve(cap, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, a.bytes, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(a.counters, 0, 64, s)) { gsr_set_error("%s: counters", who); return 1; }
    if (cap) {
        gsr_compact(AncEntryOp{*lv, occupy, status_dev, a.key_lo, a.key_hi, a.so.ka, a.src, 0}, cap, a.sums, a.counters + ANC_CNT_ENTRIES, s);
        const uint32_t* n_dev = a.counters + ANC_CNT_ENTRIES;
        GsrSort st(a.so);
        if (st.sort(cap, n_dev, 32, true, s) || gsr_sort_next_word(st, cap, n_dev, GsrWordFromArray{a.key_hi}, s)) return 1;
        const AncSorted so = anc_sorted(a);
        gsr_compact(AncHeadOp{n_dev, so.hi, so.perm, a.key_lo, so.head_pos}, cap, a.sums, a.counters + ANC_CNT_HEADS, s);
        if (weed) {
            // heads <= candidate slots; key_hi (consumed by the second sort) keeps the unweeded heads, the free order the flags
            const uint32_t worst = (uint32_t)lv->N0 * (uint32_t)lv->k;
            if (worst) {
                hipLaunchKernelGGL(k_anc_weed_flag, dim3(gsr_div_up(worst, WEED_BLOCK)), dim3(WEED_BLOCK), 0, s, *lv, W, weed->lv, a.counters, so.hi, so.perm, a.key_lo,
                                   so.head_pos, a.key_hi, so.flag);
                gsr_compact(AncWeedOp{a.counters, so.flag, a.key_hi, so.head_pos}, cap, a.sums, a.counters + ANC_CNT_FOUND, s);
            }
        }
    }
    if (three_words) hipLaunchKernelGGL(k_anc_publish_weed, dim3(1), dim3(64), 0, s, a.counters, status_dev, (weed && cap && lv->N0) ? 1 : 0);
    else hipLaunchKernelGGL(k_anc_publish, dim3(1), dim3(64), 0, s, a.counters, status_dev);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_anchor_level_find(const gsr_anchor_level* lv, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    return anc_find("anchor_level_find", lv, nullptr, nullptr, false, scratch, scratch_bytes, status_dev, stream);
}

extern "C" int gsr_anchor_level_find_weed(const gsr_anchor_level* lv, const uint8_t* occupy, const gsr_octree_weed* weed, void* scratch, size_t scratch_bytes,
                                          uint32_t* status_dev, void* stream)
{
    return anc_find("anchor_level_find_weed", lv, occupy, weed, true, scratch, scratch_bytes, status_dev, stream);
}

extern "C" int gsr_octree_weed_out(const float* positions, const int32_t* levels, int64_t U, const gsr_octree_weed* weed, int32_t* visible_count, uint8_t* keep,
                                   void* stream)
{
    const char* who = "octree_weed_out";
    WeedArgs W;
    if (weed_check(weed, who, &W)) return 1;
    if (U < 0 || U >= (1ll << 31)) { gsr_set_error("%s: U=%lld out of range", who, (long long)U); return 1; }
    if (U == 0) return 0;
    if (!positions || !levels || !visible_count || !keep) { gsr_set_error("%s: positions / levels / visible_count / keep is NULL", who); return 1; }
    hipLaunchKernelGGL(k_weed_rows, dim3(gsr_div_up((uint32_t)U, WEED_BLOCK)), dim3(WEED_BLOCK), 0, (hipStream_t)stream, W, (uint32_t)U, positions, levels,
                       visible_count, keep);
    return gsr_check_launch(who, (hipStream_t)stream, false);
}

extern "C" int gsr_anchor_level_emit(const gsr_anchor_level* lv, const void* scratch, size_t scratch_bytes, uint32_t count, float* new_anchor, float* new_feat,
                                     void* stream)
{
    uint32_t cap;
    if (anc_check(lv, "anchor_level_emit", &cap)) return 1;
    const AncScratch a = anc_carve(cap, scratch);
    if (gsr_scratch_check("anchor_level_emit", scratch, scratch_bytes, a.bytes, false)) return 1;
    if (count == 0) return 0;
    if (count > (uint32_t)lv->N0 * (uint32_t)lv->k) { gsr_set_error("anchor_level_emit: count %u exceeds the N0 * k candidate slots", count); return 1; }
    if (!new_anchor || (lv->F && !new_feat)) { gsr_set_error("anchor_level_emit: new_anchor / new_feat is NULL"); return 1; }
    const size_t threads = (size_t)count * (size_t)(lv->F > 0 ? lv->F : 1);
    if ((threads + 255) / 256 >= (1ull << 31)) { gsr_set_error("anchor_level_emit: count * F too large"); return 1; }
    const AncSorted so = anc_sorted(a);
    hipLaunchKernelGGL(k_anc_emit, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *lv, count, a.counters, so.hi, so.perm, a.key_lo, a.src,
                       so.head_pos, new_anchor, new_feat);
    return gsr_check_launch("anchor_level_emit", (hipStream_t)stream, false);
}
