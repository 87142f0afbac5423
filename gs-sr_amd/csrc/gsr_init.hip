// gsr_init.hip -- the first anchors from the point cloud, on the device: what OctreeGaussian.create_from_data (set_level, octree_sample;
// gssr/gaussian/octree_gaussian.py:152-182) and ScaffoldGaussian.create_from_data (voxelize_sample; scaffold_gaussian.py:257-298) compute with
// torch.quantile per camera, torch.unique(dim=0) per level and np.unique(axis=0) on the host (include/gsrast.h, "anchors from the point cloud").
//
//   select      order statistics by MSB-first radix select, 8 bits per pass, four passes.  A problem (a camera, or an array) carries up to four
//               ranks; per rank the state is {prefix, rank among the keys that share the prefix}.  A pass = one histogram kernel (keys whose high
//               bits equal a rank's prefix are counted by their next 8 bits) + k_sel_advance (one wave per rank: scan of 256 bins, new prefix, the
//               histogram cleared for the next pass).  Ranks whose prefixes are equal share ONE histogram (the first of them counts, the others
//               read it): in pass 0 that is all four, and the lo / hi ranks of a quantile stay together to the end unless a bin boundary parts them.
//   cameras     k_cq_hist: the key is the bit pattern of the squared distance ((dx*dx + dy*dy) + dz*dz, float32, no contraction; >= 0, so the
//               pattern orders as an unsigned integer), recomputed in every pass -- C x N distances are never stored.  A block holds CQ_PPT points
//               per thread in registers and walks a batch of CQ_CB cameras whose histograms live in LDS: a point is fetched once per camera batch.
//               Pass 0 meets few bins (the top 8 bits are sign + 7 exponent bits): the histograms are private to a wave there, and lanes that
//               share the wave's leading bin add once (CQ_AGG rounds), the rest by LDS atomics.  The root is taken of the selected values only
//               (a correctly rounded sqrt is monotone), then ATen's lerp and the camera's scale.
//   arrays      k_sel_hist: the same select over an array (gsr_select, gsr_common.h): floats with their sign-magnitude patterns folded to unsigned
//               order, or uint32 complemented for a descending order (the mesh filter's k-th largest cluster, gsr_mesh_post.hip).
//   voxels      per cell size: key = rint((p - init_pos) / cell) per axis (IEEE divide, half to even), three stable LSD sorts (z, y, x) of the
//               sign-biased int32 keys, each word regenerated through the order (gsr_sort.h), run heads by the keep scan; the heads' point indices stay in scratch for the emit.
// lerp: ATen's Lerp.h, w < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w), every operation rounded on its own (PRE_FLAGS: no contraction).  That is what
// torch.quantile gives on the CPU at ATen's DEFAULT dispatch level; its AVX2 / AVX512 kernels fuse the product-sum and differ in the last bit in about
// one case in a hundred (measured).
// Every launch is on the caller's stream; nothing synchronises; no kernel waits for another workgroup.
#include "gsr_common.h"
#include "gsr_scan.h"
#include <algorithm>

#define SEL_RANKS 4
#define SEL_BLOCK 256
#define CQ_CB 8               // cameras per batch: CQ_CB * SEL_RANKS * 256 words = 32 KiB of LDS, two workgroups per CU keep 8 waves in flight
#define CQ_PPT 8              // points per thread and chunk
#define CQ_CHUNK (SEL_BLOCK * CQ_PPT)
#define CQ_AGG 2              // pass 0: rounds of wave aggregation before the LDS atomic
#define CQ_BLOCKS 4096u       // workgroups aimed at: the point chunks are dealt to CQ_BLOCKS / batches of them per camera batch, each looping over its share
#define CQ_LDS_WORDS (CQ_CB * SEL_RANKS * 256)
#define SEL_NOMATCH 1u        // a prefix no key can have from pass 1 on (its low 8 bits are clear in every masked key)
#define VU_BLOCK 256
#define VU_MAX_LEVELS 32

struct SelRanks { uint32_t k[SEL_RANKS]; };      // 0-based ranks, ascending order
struct SelState { uint32_t* prefix; uint32_t* krem; uint32_t* hist; };      // [P][4], [P][4], [P][4][256]

// prefixes of problem p as the histogram kernels use them: a rank that shares its prefix with an earlier one does not count (SEL_NOMATCH)
__device__ __forceinline__ uint32_t sel_count_prefix(const uint32_t* prefix, int pass, uint32_t p, int t)
{
    if (pass == 0) return t == 0 ? 0u : SEL_NOMATCH;
    const uint32_t v = prefix[p * SEL_RANKS + t];
    for (int u = 0; u < t; u++) if (prefix[p * SEL_RANKS + u] == v) return SEL_NOMATCH;
    return v;
}

// one workgroup per problem, wave t = rank t.  hist is left cleared.
__global__ void __launch_bounds__(SEL_BLOCK) k_sel_advance(SelState st, SelRanks ranks, int pass, uint32_t* __restrict__ status)
{
    const uint32_t p = blockIdx.x, t = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t pre = pass ? st.prefix[p * SEL_RANKS + t] : 0u;
    const uint32_t r = pass ? st.krem[p * SEL_RANKS + t] : ranks.k[t] + 1u;      // 1-based among the keys that share the prefix
    uint32_t src = t;
    if (pass == 0) src = 0;
    else for (int u = (int)t - 1; u >= 0; u--) if (st.prefix[p * SEL_RANKS + u] == pre) src = (uint32_t)u;
    __syncthreads();                                      // every wave has read the old prefixes
    const uint32_t* h = st.hist + ((size_t)p * SEL_RANKS + src) * 256;
    const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const uint32_t sum = c0 + c1 + c2 + c3;
    const uint32_t before = wave_incl_scan(sum) - sum;
    const bool mine = r != 0u && before < r && r <= before + sum;
    if (mine) {
        uint32_t b = 0, cum = before;
        if (cum + c0 >= r) b = 0;
        else if ((cum += c0) + c1 >= r) b = 1;
        else if ((cum += c1) + c2 >= r) b = 2;
        else { cum += c2; b = 3; }
        st.prefix[p * SEL_RANKS + t] = pre | ((4 * lane + b) << (24 - 8 * pass));
        st.krem[p * SEL_RANKS + t] = r - cum;
    }
    if (__ballot(mine) == 0ull && lane == 0) {            // the rank lies beyond the keys (or a histogram lost a key: non-finite input)
        atomicOr(status, (uint32_t)GSR_INIT_ERR_RANK);
        st.krem[p * SEL_RANKS + t] = 0u;                  // stays without a bin in the later passes
    }
    __syncthreads();                                      // every wave has read its histogram
    uint32_t* hz = st.hist + (size_t)p * SEL_RANKS * 256;
    for (uint32_t i = threadIdx.x; i < SEL_RANKS * 256; i += SEL_BLOCK) hz[i] = 0u;
}

// ATen's Lerp.h, operation by operation
__device__ __forceinline__ float sel_lerp(float a, float b, float w)
{
    const float d = b - a;
    return fabsf(w) < 0.5f ? a + w * d : b - d * (1.0f - w);
}

// ------------------------------------------------------------------------------------------------ per-camera distance order statistics
__device__ __forceinline__ uint32_t cq_key(float px, float py, float pz, float cx, float cy, float cz)
{
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return __float_as_uint((dx * dx + dy * dy) + dz * dz);
}

template <bool PASS0>
__global__ void __launch_bounds__(SEL_BLOCK) k_cq_hist(const float* __restrict__ points, uint32_t N, const float* __restrict__ cams, uint32_t C, SelState st, int pass,
                                                       uint32_t* __restrict__ status)
{
    __shared__ uint32_t h[CQ_LDS_WORDS];                  // pass 0: [wave][camera][256]; later: [camera][rank][256]
    __shared__ float cam[CQ_CB][4];
    __shared__ uint32_t pfx[CQ_CB][SEL_RANKS];
    const uint32_t c0 = blockIdx.y * CQ_CB, nc = min((uint32_t)CQ_CB, C - c0), tid = threadIdx.x;
    for (uint32_t i = tid; i < CQ_LDS_WORDS; i += SEL_BLOCK) h[i] = 0u;
    if (tid < nc * 4) cam[tid >> 2][tid & 3] = cams[(size_t)(c0 + (tid >> 2)) * 4 + (tid & 3)];
    if (!PASS0 && tid < nc * SEL_RANKS) pfx[tid >> 2][tid & 3] = sel_count_prefix(st.prefix, pass, c0 + (tid >> 2), (int)(tid & 3));
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = PASS0 ? 0u : ~0u << (32 - 8 * pass);
    const uint32_t nchunks = gsr_div_up(N, CQ_CHUNK), lane = tid & 63u;
    uint32_t* hw = h + (tid >> 6) * (CQ_CB * 256);        // pass 0: this wave's histograms
    bool bad = false;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        float px[CQ_PPT], py[CQ_PPT], pz[CQ_PPT];
        const uint32_t base = chunk * CQ_CHUNK + tid;
#pragma unroll
        for (int j = 0; j < CQ_PPT; j++) {
            const uint32_t i = base + j * SEL_BLOCK;
            const bool in = i < N;
            px[j] = in ? points[3 * (size_t)i] : 0.f; py[j] = in ? points[3 * (size_t)i + 1] : 0.f; pz[j] = in ? points[3 * (size_t)i + 2] : 0.f;
        }
        for (uint32_t cb = 0; cb < nc; cb++) {
            const float cx = cam[cb][0], cy = cam[cb][1], cz = cam[cb][2];
#pragma unroll
            for (int j = 0; j < CQ_PPT; j++) {
                const bool in = base + j * SEL_BLOCK < N;
                const uint32_t key = cq_key(px[j], py[j], pz[j], cx, cy, cz);
                if (PASS0) {
                    if (in && key >= 0x7F800000u) bad = true;             // inf, NaN (a squared distance carries no sign)
                    const uint32_t bin = key >> 24;                        // < 256
                    bool live = in;
                    unsigned long long todo = __ballot(live);
#pragma unroll
                    for (int it = 0; it < CQ_AGG; it++) {
                        if (!todo) break;                                  // wave-uniform
                        const int lead = __ffsll((long long)todo) - 1;
                        const uint32_t b0 = (uint32_t)__shfl((int)bin, lead, 64);
                        const bool mine = live && bin == b0;
                        const unsigned long long m = __ballot(mine);
                        if ((int)lane == lead) atomicAdd(&hw[cb * 256 + b0], (uint32_t)__popcll(m));      // one lane, one add for the group
                        if (mine) live = false;
                        todo &= ~m;
                    }
                    if (live) atomicAdd(&hw[cb * 256 + bin], 1u);
                } else if (in) {
                    const uint32_t hb = key & himask, bin = (key >> shift) & 255u;
#pragma unroll
                    for (int t = 0; t < SEL_RANKS; t++)
                        if (hb == pfx[cb][t]) atomicAdd(&h[(cb * SEL_RANKS + t) * 256 + bin], 1u);
                }
            }
        }
    }
    __syncthreads();
    if (PASS0) {
        for (uint32_t i = tid; i < nc * 256; i += SEL_BLOCK) {
            const uint32_t v = h[i] + h[CQ_CB * 256 + i] + h[2 * CQ_CB * 256 + i] + h[3 * CQ_CB * 256 + i];
            if (v) atomicAdd(st.hist + ((size_t)(c0 + (i >> 8)) * SEL_RANKS) * 256 + (i & 255u), v);
        }
        if (bad) atomicOr(status, (uint32_t)GSR_INIT_ERR_NONFINITE);
    } else {
        for (uint32_t i = tid; i < nc * SEL_RANKS * 256; i += SEL_BLOCK) {
            const uint32_t v = h[i];
            if (v) atomicAdd(st.hist + (size_t)c0 * SEL_RANKS * 256 + i, v);
        }
    }
}

__global__ void __launch_bounds__(SEL_BLOCK) k_cq_finish(const float* __restrict__ cams, uint32_t C, SelState st, float w0, float w1, float* __restrict__ all_dist)
{
    const uint32_t c = blockIdx.x * SEL_BLOCK + threadIdx.x;
    if (c >= C) return;
    const uint32_t* p = st.prefix + (size_t)c * SEL_RANKS;
    const float s = cams[(size_t)c * 4 + 3];
    all_dist[2 * (size_t)c] = sel_lerp(sqrtf(__uint_as_float(p[0])), sqrtf(__uint_as_float(p[1])), w0) * s;
    all_dist[2 * (size_t)c + 1] = sel_lerp(sqrtf(__uint_as_float(p[2])), sqrtf(__uint_as_float(p[3])), w1) * s;
}

// ------------------------------------------------------------------------------------------------ order statistics of an array
__device__ __forceinline__ uint32_t sel_fold(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t sel_unfold(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// the key of element i in ascending unsigned order; *bad where the element has none
struct SelKeyFloat {
    const float* v;
    __device__ uint32_t operator()(uint32_t i, bool* bad) const
    {
        const uint32_t bits = __float_as_uint(v[i]);
        if ((bits & 0x7FFFFFFFu) > 0x7F800000u) *bad = true;              // NaN
        return sel_fold(bits);
    }
};
struct SelKeyU32Desc { const uint32_t* v; __device__ uint32_t operator()(uint32_t i, bool*) const { return ~v[i]; } };      // descending: no value is bad

template <typename Key>
__global__ void __launch_bounds__(SEL_BLOCK) k_sel_hist(Key key_of, uint32_t n, const uint32_t* __restrict__ n_dev, SelState st, int pass, uint32_t* __restrict__ status)
{
    __shared__ uint32_t h[SEL_RANKS * 256];
    __shared__ uint32_t pfx[SEL_RANKS];
    if (n_dev) n = min(n, *n_dev);
    for (uint32_t i = threadIdx.x; i < SEL_RANKS * 256; i += SEL_BLOCK) h[i] = 0u;
    if (threadIdx.x < SEL_RANKS) pfx[threadIdx.x] = sel_count_prefix(st.prefix, pass, 0u, (int)threadIdx.x);
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass ? ~0u << (32 - 8 * pass) : 0u;
    bool bad = false;
    for (uint32_t i = blockIdx.x * SEL_BLOCK + threadIdx.x; i < n; i += gridDim.x * SEL_BLOCK) {
        const uint32_t key = key_of(i, &bad), hb = key & himask, bin = (key >> shift) & 255u;
#pragma unroll
        for (int t = 0; t < SEL_RANKS; t++)
            if (hb == pfx[t] && (pass || t == 0)) atomicAdd(&h[t * 256 + bin], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SEL_RANKS * 256; i += SEL_BLOCK) if (h[i]) atomicAdd(st.hist + i, h[i]);
    if (bad && pass == 0) atomicOr(status, (uint32_t)GSR_INIT_ERR_NONFINITE);
}

__global__ void __launch_bounds__(64) k_sel_finish(SelState st, int n_targets, float w0, float w1, float* __restrict__ out)
{
    const int t = (int)threadIdx.x;
    if (t >= n_targets) return;
    const float a = __uint_as_float(sel_unfold(st.prefix[2 * t])), b = __uint_as_float(sel_unfold(st.prefix[2 * t + 1]));
    out[t] = sel_lerp(a, b, t ? w1 : w0);
}

static SelState sel_carve(uint32_t problems, const void* base, size_t* bytes)
{
    SelState st; GsrCarve c(base);
    const size_t P = problems > 0 ? problems : 1;
    st.prefix = c.take<uint32_t>(P * SEL_RANKS); st.krem = c.take<uint32_t>(P * SEL_RANKS); st.hist = c.take<uint32_t>(P * SEL_RANKS * 256);
    *bytes = c.bytes();
    return st;
}

void gsr_select(int kind, const void* values, uint32_t n, const uint32_t* n_dev, const uint32_t rank[4], uint32_t* state, uint32_t* status, hipStream_t s)
{
    size_t bytes;
    const SelState st = sel_carve(1, state, &bytes);      // the prefixes lead: word t of the state ends as the key of rank t
    static_assert(GSR_SELECT_STATE_BYTES == 2 * 256 + SEL_RANKS * 256 * 4, "one problem's state");
    const SelRanks r = {{rank[0], rank[1], rank[2], rank[3]}};
    const uint32_t grid = std::min(gsr_div_up(n, SEL_BLOCK * 8u), 1024u);
    for (int pass = 0; pass < 4; pass++) {
        if (kind == GSR_SELECT_FLOAT) hipLaunchKernelGGL(k_sel_hist<SelKeyFloat>, dim3(grid), dim3(SEL_BLOCK), 0, s, SelKeyFloat{(const float*)values}, n, n_dev, st, pass, status);
        else hipLaunchKernelGGL(k_sel_hist<SelKeyU32Desc>, dim3(grid), dim3(SEL_BLOCK), 0, s, SelKeyU32Desc{(const uint32_t*)values}, n, n_dev, st, pass, status);
        hipLaunchKernelGGL(k_sel_advance, dim3(1), dim3(SEL_BLOCK), 0, s, st, r, pass, status);
    }
}

// ranks {lo0, hi0, lo1, hi1} of up to two targets; false with the error set where one lies outside [0, n)
static bool sel_ranks(const char* who, int n_targets, const int64_t* k_lo, const int64_t* k_hi, int64_t n, SelRanks* r)
{
    for (int t = 0; t < 2; t++) {
        const int u = t < n_targets ? t : 0;
        if (k_lo[u] < 0 || k_hi[u] < k_lo[u] || k_hi[u] > k_lo[u] + 1 || k_hi[u] >= n) {
            gsr_set_error("%s: ranks k_lo=%lld k_hi=%lld of target %d do not lie in [0, %lld) one apart at most", who, (long long)k_lo[u], (long long)k_hi[u], u, (long long)n);
            return false;
        }
        r->k[2 * t] = (uint32_t)k_lo[u]; r->k[2 * t + 1] = (uint32_t)k_hi[u];
    }
    return true;
}

extern "C" size_t gsr_cam_dist_quantiles_scratch_bytes(int64_t N, int32_t C)
{
    if (N < 1 || N >= (1ll << 31) || C < 1) return 0;
    size_t b; sel_carve((uint32_t)C, nullptr, &b);
    return b;
}

extern "C" int gsr_cam_dist_quantiles(const float* points, int64_t N, const float* cam_infos, int32_t C, const int64_t* k_lo, const int64_t* k_hi, const float* w,
                                      float* all_dist, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "cam_dist_quantiles";
    if (N < 1 || N >= (1ll << 31)) { gsr_set_error("%s: N=%lld points out of range [1, 2^31)", who, (long long)N); return 1; }
    if (C < 1) { gsr_set_error("%s: at least one camera is needed, C=%d", who, C); return 1; }
    if (!points || !cam_infos || !k_lo || !k_hi || !w || !all_dist || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    SelRanks r;
    if (!sel_ranks(who, 2, k_lo, k_hi, N, &r)) return 1;
    size_t need;
    const SelState st = sel_carve((uint32_t)C, scratch, &need);
    if (gsr_scratch_check(who, scratch, scratch_bytes, need, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s) || gsr_memset_async(st.hist, 0, (size_t)C * SEL_RANKS * 256 * 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    const uint32_t batches = gsr_div_up((uint32_t)C, CQ_CB);
    if (batches > 65535u) { gsr_set_error("%s: C=%d cameras exceed %d", who, C, 65535 * CQ_CB); return 1; }
    const dim3 grid(std::min(gsr_div_up((uint32_t)N, CQ_CHUNK), std::max(1u, CQ_BLOCKS / batches)), batches);
    for (int pass = 0; pass < 4; pass++) {
        if (pass == 0) hipLaunchKernelGGL((k_cq_hist<true>), grid, dim3(SEL_BLOCK), 0, s, points, (uint32_t)N, cam_infos, (uint32_t)C, st, pass, status_dev);
        else hipLaunchKernelGGL((k_cq_hist<false>), grid, dim3(SEL_BLOCK), 0, s, points, (uint32_t)N, cam_infos, (uint32_t)C, st, pass, status_dev);
        hipLaunchKernelGGL(k_sel_advance, dim3((uint32_t)C), dim3(SEL_BLOCK), 0, s, st, r, pass, status_dev);
    }
    hipLaunchKernelGGL(k_cq_finish, dim3(gsr_div_up((uint32_t)C, SEL_BLOCK)), dim3(SEL_BLOCK), 0, s, cam_infos, (uint32_t)C, st, w[0], w[1], all_dist);
    return gsr_check_launch(who, s, false);
}

extern "C" size_t gsr_select_lerp_scratch_bytes(int64_t n)
{
    if (n < 1 || n >= (1ll << 31)) return 0;
    size_t b; sel_carve(1, nullptr, &b);
    return b;
}

extern "C" int gsr_select_lerp(const float* values, int64_t n, const uint32_t* n_dev, int32_t n_targets, const int64_t* k_lo, const int64_t* k_hi, const float* w,
                               float* out, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "select_lerp";
    if (n < 1 || n >= (1ll << 31)) { gsr_set_error("%s: n=%lld values out of range [1, 2^31)", who, (long long)n); return 1; }
    if (n_targets < 1 || n_targets > 2) { gsr_set_error("%s: one or two targets, not %d", who, n_targets); return 1; }
    if (!values || !k_lo || !k_hi || !w || !out || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    SelRanks r;
    if (!sel_ranks(who, n_targets, k_lo, k_hi, n, &r)) return 1;
    size_t need;
    const SelState st = sel_carve(1, scratch, &need);
    if (gsr_scratch_check(who, scratch, scratch_bytes, need, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s) || gsr_memset_async(scratch, 0, GSR_SELECT_STATE_BYTES, s)) { gsr_set_error("%s: clear", who); return 1; }
    gsr_select(GSR_SELECT_FLOAT, values, (uint32_t)n, n_dev, r.k, (uint32_t*)scratch, status_dev, s);
    hipLaunchKernelGGL(k_sel_finish, dim3(1), dim3(64), 0, s, st, n_targets, w[0], w[n_targets > 1 ? 1 : 0], out);
    return gsr_check_launch(who, s, false);
}

// ------------------------------------------------------------------------------------------------ unique voxel rows
template <typename T> struct VuArgs { const T* points; uint32_t N; T init[3]; T cell; };

// the key of one coordinate; *err |= the status bits of a coordinate that has none (the key is then 0)
template <typename T> __device__ __forceinline__ int32_t vu_key(T p, T init, T cell, uint32_t* err)
{
    const T q = rint((p - init) / cell);
    if (!(fabs(q) < (T)2147483648.0)) { *err |= (p - p == (T)0) ? GSR_INIT_ERR_KEY_RANGE : GSR_INIT_ERR_NONFINITE; return 0; }
    return (int32_t)q;
}
__device__ __forceinline__ uint32_t vu_bias(int32_t k) { return (uint32_t)k ^ 0x80000000u; }

// the biased key of axis `axis` of point src < N, one word of the sort's key (gsr_sort_next_word); its error bits go to *status
template <typename T> struct VuAxisOp {
    VuArgs<T> a; int axis; uint32_t* status;
    __device__ uint32_t operator()(uint32_t src) const
    {
        uint32_t err = 0;
        const int32_t k = vu_key<T>(a.points[3 * (size_t)src + axis], a.init[axis], a.cell, &err);
        if (err) atomicOr(status, err);
        return vu_bias(k);
    }
};
// the first word, in point order: keys[i] = op(i)
template <typename T>
__global__ void __launch_bounds__(VU_BLOCK) k_vu_keys(VuAxisOp<T> op, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * VU_BLOCK + threadIdx.x;
    if (i < op.a.N) keys[i] = op(i);
}

template <typename T> __device__ __forceinline__ void vu_key3(const VuArgs<T>& a, uint32_t src, int32_t* k)
{
    uint32_t err = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) k[ax] = src < a.N ? vu_key<T>(a.points[3 * (size_t)src + ax], a.init[ax], a.cell, &err) : 0;
}

// flag[i] = row i of the sorted order starts a run of equal keys
template <typename T>
__global__ void __launch_bounds__(VU_BLOCK) k_vu_flag(VuArgs<T> a, const uint32_t* __restrict__ order, uint8_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * VU_BLOCK + threadIdx.x;
    if (i >= a.N) return;
    bool head = i == 0;
    if (!head) {
        int32_t k0[3], k1[3];
        vu_key3<T>(a, order[i - 1], k0); vu_key3<T>(a, order[i], k1);
        head = k0[0] != k1[0] || k0[1] != k1[1] || k0[2] != k1[2];
    }
    flag[i] = head ? 1 : 0;
}

// heads[p] = the point that leads run p
__global__ void __launch_bounds__(VU_BLOCK) k_vu_heads(const uint32_t* __restrict__ count_dev, uint32_t N, const uint32_t* __restrict__ map, const uint32_t* __restrict__ order,
                                                       uint32_t* __restrict__ heads)
{
    const uint32_t p = blockIdx.x * VU_BLOCK + threadIdx.x;
    if (p >= min(*count_dev, N)) return;
    const uint32_t i = map[p];
    heads[p] = i < N ? order[i] : 0u;
}

struct VuLevels { uint32_t end[VU_MAX_LEVELS]; double cell[VU_MAX_LEVELS]; int32_t L; };      // end[l] = rows of the levels up to and including l

template <typename T>
__global__ void __launch_bounds__(VU_BLOCK) k_vu_emit(VuArgs<T> a, VuLevels lv, uint32_t total, const uint32_t* __restrict__ heads, float* __restrict__ positions,
                                                      int32_t* __restrict__ level)
{
    const uint32_t j = blockIdx.x * VU_BLOCK + threadIdx.x;
    if (j >= total) return;
    int l = 0;
    while (l < lv.L - 1 && j >= lv.end[l]) l++;
    const uint32_t p = j - (l ? lv.end[l - 1] : 0u);      // < the count of level l <= N
    a.cell = (T)lv.cell[l];
    int32_t k[3];
    vu_key3<T>(a, heads[(size_t)l * a.N + p], k);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) positions[3 * (size_t)j + ax] = (float)((T)k[ax] * a.cell + a.init[ax]);      // multiply, then add; a zero key gives +0
    level[j] = l;
}

struct VuScratch { GsrSortBuf so; uint32_t *sums, *map, *heads; uint8_t* flag; size_t bytes; };
static VuScratch vu_carve(uint32_t N, int32_t L, const void* base)
{
    VuScratch v; GsrCarve c(base);
    const size_t n = N > 0 ? N : 1;
    v.so = gsr_sort_carve(c, n);
    v.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    v.map = c.take<uint32_t>(n); v.flag = c.take<uint8_t>(n);
    v.heads = c.take<uint32_t>(n * (size_t)(L > 0 ? L : 1));
    v.bytes = c.bytes();
    return v;
}

static int vu_args(const char* who, const void* points, int64_t N, int32_t L, const double* init_pos, const double* cell, int32_t mode)
{
    if (N < 1 || N >= (1ll << 31)) { gsr_set_error("%s: N=%lld points out of range [1, 2^31)", who, (long long)N); return 1; }
    if (L < 1 || L > VU_MAX_LEVELS) { gsr_set_error("%s: L=%d cell sizes out of range [1, %d]", who, L, VU_MAX_LEVELS); return 1; }
    if (mode != GSR_VOXEL_F32 && mode != GSR_VOXEL_F64) { gsr_set_error("%s: unknown mode %d", who, mode); return 1; }
    if (!points || !init_pos || !cell) { gsr_set_error("%s: null pointer", who); return 1; }
    for (int l = 0; l < L; l++) {
        const double c = mode == GSR_VOXEL_F32 ? (double)(float)cell[l] : cell[l];
        if (!(c > 0.0) || !(c < 3.0e38)) { gsr_set_error("%s: cell size %d must be a positive finite number", who, l); return 1; }
    }
    for (int ax = 0; ax < 3; ax++) if (!(init_pos[ax] - init_pos[ax] == 0.0)) { gsr_set_error("%s: init_pos must be finite", who); return 1; }
    return 0;
}

extern "C" size_t gsr_voxel_unique_scratch_bytes(int64_t N, int32_t L)
{
    if (N < 1 || N >= (1ll << 31) || L < 1 || L > VU_MAX_LEVELS) return 0;
    return vu_carve((uint32_t)N, L, nullptr).bytes;
}

template <typename T>
static int vu_count(const char* who, const void* points, uint32_t N, int32_t L, const double* init_pos, const double* cell, const VuScratch& v, uint32_t* record_dev,
                    hipStream_t s)
{
    VuArgs<T> a;
    a.points = (const T*)points; a.N = N;
    for (int ax = 0; ax < 3; ax++) a.init[ax] = (T)init_pos[ax];
    const uint32_t g = gsr_div_up(N, VU_BLOCK);
    for (int l = 0; l < L; l++) {
        a.cell = (T)cell[l];
        GsrSort st(v.so);                                 // stable LSD: z, then y, then x -> rows ascend by x, then y, then z
        hipLaunchKernelGGL((k_vu_keys<T>), dim3(g), dim3(VU_BLOCK), 0, s, VuAxisOp<T>{a, 2, record_dev}, st.keys);
        if (st.sort(N, nullptr, 32, true, s)) return 1;
        for (int axis = 1; axis >= 0; axis--)
            if (gsr_sort_next_word(st, N, nullptr, VuAxisOp<T>{a, axis, record_dev}, s)) return 1;
        hipLaunchKernelGGL((k_vu_flag<T>), dim3(g), dim3(VU_BLOCK), 0, s, a, st.order, v.flag);
        gsr_rows_keep_scan(v.flag, N, v.sums, v.map, nullptr, record_dev + 1 + l, s);
        hipLaunchKernelGGL(k_vu_heads, dim3(g), dim3(VU_BLOCK), 0, s, record_dev + 1 + l, N, v.map, st.order, v.heads + (size_t)l * N);
    }
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_voxel_unique_count(const void* points, int64_t N, int32_t L, const double* init_pos, const double* cell, int32_t mode, void* scratch,
                                      size_t scratch_bytes, uint32_t* record_dev, void* stream)
{
    const char* who = "voxel_unique_count";
    if (vu_args(who, points, N, L, init_pos, cell, mode)) return 1;
    if (!record_dev) { gsr_set_error("%s: null record", who); return 1; }
    const VuScratch v = vu_carve((uint32_t)N, L, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, v.bytes, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(record_dev, 0, (size_t)(1 + L) * 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    return mode == GSR_VOXEL_F32 ? vu_count<float>(who, points, (uint32_t)N, L, init_pos, cell, v, record_dev, s)
                                 : vu_count<double>(who, points, (uint32_t)N, L, init_pos, cell, v, record_dev, s);
}

template <typename T>
static void vu_emit(const void* points, uint32_t N, const double* init_pos, const VuLevels& lv, uint32_t total, const VuScratch& v, float* positions, int32_t* level,
                    hipStream_t s)
{
    VuArgs<T> a;
    a.points = (const T*)points; a.N = N; a.cell = (T)1;
    for (int ax = 0; ax < 3; ax++) a.init[ax] = (T)init_pos[ax];
    hipLaunchKernelGGL((k_vu_emit<T>), dim3(gsr_div_up(total, VU_BLOCK)), dim3(VU_BLOCK), 0, s, a, lv, total, v.heads, positions, level);
}

extern "C" int gsr_voxel_unique_emit(const void* points, int64_t N, int32_t L, const double* init_pos, const double* cell, int32_t mode, const void* scratch,
                                     size_t scratch_bytes, const uint32_t* record, float* positions, int32_t* level, void* stream)
{
    const char* who = "voxel_unique_emit";
    if (vu_args(who, points, N, L, init_pos, cell, mode)) return 1;
    if (!record) { gsr_set_error("%s: null record", who); return 1; }
    if (record[0]) { gsr_set_error("%s: the count reported status %u, nothing to emit", who, record[0]); return 1; }
    const VuScratch v = vu_carve((uint32_t)N, L, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, v.bytes, false)) return 1;
    VuLevels lv;
    lv.L = L;
    uint64_t total = 0;
    for (int l = 0; l < L; l++) {
        if (record[1 + l] < 1 || record[1 + l] > (uint64_t)N) { gsr_set_error("%s: the record does not belong to this cloud", who); return 1; }
        total += record[1 + l];
        if (total >= (1ull << 31)) { gsr_set_error("%s: %llu rows exceed 2^31", who, (unsigned long long)total); return 1; }
        lv.end[l] = (uint32_t)total; lv.cell[l] = cell[l];
    }
    if (!positions || !level) { gsr_set_error("%s: null output", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (mode == GSR_VOXEL_F32) vu_emit<float>(points, (uint32_t)N, init_pos, lv, (uint32_t)total, v, positions, level, s);
    else vu_emit<double>(points, (uint32_t)N, init_pos, lv, (uint32_t)total, v, positions, level, s);
    return gsr_check_launch(who, s, false);
}
