// gsr_views.hip -- the PGSR neighbour views, on the device: what view_selection / calc_score (gssr/utils/mvsnet_utils.py:306-343) compute on the host
// with one list search per pair of images (include/gsrast.h, "neighbour views").
//
// The score of a pair of images is a sum over the 3-D points both observe, so it is accumulated per point TRACK (the images that observe one point)
// and not per pair: sum_p t_p^2 / 2 evaluations of one acos and one exp instead of C^2 / 2 intersections of id lists.
//
//   flatten     the observations are image-major ([offsets[a], offsets[a + 1]) belongs to image a); the entries != -1 are compacted in that order
//               (gsr_compact.h) with their image and the low word of their id
//   sort        stable LSD radix sort by id (gsr_sort.h): the low word, then -- only where the caller says ids need it (id_bits = 64) -- the
//               sign-biased high word.  The input is image-major and the sort stable, so a run of equal ids is a track with its images ascending and
//               the repeats of one image adjacent
//   entries     heads of the runs of equal (id, image): entry e = one image of one track, multiplicity = the length of its run; tracks = heads of
//               the runs of equal id among the entries.  Both by the same compaction.  Tracks of two or more entries find their row of the point
//               table by binary search (the table ascends strictly; checked on the device)
//   by image    a second stable sort of the entries by image: image a's entries, still in ascending id order
//   score       one workgroup of ONE wave per image a: it walks a's entries in ascending id order, lanes take the track's other images b and add
//               m * g into row[b] of an LDS row of C doubles, g evaluated with the lower-indexed image's operands first and m that image's
//               multiplicity, as the reference counts.  The terms of as many consecutive tracks as fill the wave are evaluated side by side (their loads
//               in flight together: the walk is bound by latency, not arithmetic); the ADDITIONS are made by one wave, one track after the other: the
//               order of every sum is ascending id, whatever the machine does, S[a,b] and S[b,a] are the same operations on the same operands (no
//               contraction: PRE_FLAGS) and so the same bits, and there is no floating-point atomic.  The same wave then takes the k best of the finished row by repeated arg-max: descending score,
//               among equal scores the HIGHER index first (a stable ascending sort, reversed); the image's own index competes with its score 0.
// Failures go to one status word (GSR_VIEWS_ERR_*).  Every launch is on the caller's stream; nothing synchronises; no kernel waits for another workgroup.
#include "gsr_common.h"
#include "gsr_compact.h"
#include "gsr_scan.h"
#include <algorithm>

#define VW_BLOCK 256
#define VW_WAVE 64            // the score workgroup: one wave
#define VW_MAX_C GSR_VIEWS_MAX_IMAGES
#define VW_NONE 0xFFFFFFFFu
#define VW_CNT_OBS 0          // counters: observations != -1, entries, tracks
#define VW_CNT_ENTRIES 1
#define VW_CNT_TRACKS 2

struct VwScratch {
    uint32_t *cnt, *sums, *map, *cimg, *simg, *emap, *eimg, *tmap, *etrack, *tpi, *ioff;
    GsrSortBuf so;            // both sorts: the observations by id, then the entries by image
    int64_t* sid;
    size_t bytes;
};
static VwScratch vw_carve(uint32_t n, uint32_t C, const void* base)
{
    VwScratch v; GsrCarve c(base);
    v.cnt = c.take<uint32_t>(16);
    v.sums = c.take<uint32_t>(gsr_compact_sums_words(n));
    v.map = c.take<uint32_t>(n); v.cimg = c.take<uint32_t>(n);
    v.so = gsr_sort_carve(c, n);
    v.sid = c.take<int64_t>(n); v.simg = c.take<uint32_t>(n);
    v.emap = c.take<uint32_t>(n); v.eimg = c.take<uint32_t>(n); v.tmap = c.take<uint32_t>(n); v.etrack = c.take<uint32_t>(n); v.tpi = c.take<uint32_t>(n);
    v.ioff = c.take<uint32_t>((size_t)C + 1);
    v.bytes = c.bytes();
    return v;
}

// ------------------------------------------------------------------------------------------------ input checks
__global__ void __launch_bounds__(VW_BLOCK) k_vw_check(const double* __restrict__ centres, uint32_t C, const int64_t* __restrict__ offsets, int64_t M,
                                                       const int64_t* __restrict__ point_ids, uint32_t Np, uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * VW_BLOCK + threadIdx.x;
    uint32_t err = 0;
    if (i < 3 * C) { const double v = centres[i]; if (!(v - v == 0.0)) err |= GSR_VIEWS_ERR_NONFINITE; }
    if (i < C && offsets[i] > offsets[i + 1]) err |= GSR_VIEWS_ERR_OFFSETS;
    if (i == 0 && (offsets[0] != 0 || offsets[C] != M)) err |= GSR_VIEWS_ERR_OFFSETS;
    if (i + 1 < Np && point_ids[i] >= point_ids[i + 1]) err |= GSR_VIEWS_ERR_TABLE;
    if (err) atomicOr(status, err);
}

// the image of observation slot i: the last a in [0, C) with offsets[a] <= i (offsets that do not ascend give some image of the range, and the status bit)
__device__ __forceinline__ uint32_t vw_image_of(const int64_t* __restrict__ offsets, uint32_t C, int64_t i)
{
    uint32_t lo = 0, hi = C;                              // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ the three compactions
struct VwValidOp {
    const int64_t *ids, *offsets; uint32_t M, C; int32_t id_bits; uint32_t *map, *cimg, *key, *status;
    __device__ bool keep(uint32_t i) const { return i < M && ids[i] != -1; }
    __device__ void place(uint32_t i, uint32_t p) const
    {
        const uint64_t id = (uint64_t)ids[i];
        map[p] = i; cimg[p] = vw_image_of(offsets, C, (int64_t)i); key[p] = (uint32_t)id;
        if (id_bits == 32 && (id >> 32)) atomicOr(status, (uint32_t)GSR_VIEWS_ERR_ID_RANGE);
    }
};
struct VwEntryOp {
    const int64_t* sid; const uint32_t *simg, *cnt; uint32_t n; uint32_t *emap, *eimg, *key;
    __device__ bool keep(uint32_t i) const
    {
        if (i >= min(n, cnt[VW_CNT_OBS])) return false;
        return i == 0 || sid[i] != sid[i - 1] || simg[i] != simg[i - 1];
    }
    __device__ void place(uint32_t i, uint32_t e) const { emap[e] = i; eimg[e] = simg[i]; key[e] = simg[i]; }
};
struct VwTrackOp {
    const int64_t* sid; const uint32_t *emap, *cnt; uint32_t n; uint32_t* tmap;
    __device__ bool keep(uint32_t e) const
    {
        if (e >= min(n, cnt[VW_CNT_ENTRIES])) return false;
        return e == 0 || sid[emap[e]] != sid[emap[e - 1]];
    }
    __device__ void place(uint32_t e, uint32_t t) const { tmap[t] = e; }
};

// the sign-biased high word of the id of compacted observation p (gsr_sort_next_word): ascending as int64 after the second sort
struct VwHighOp {
    const int64_t* ids; const uint32_t* map;
    __device__ uint32_t operator()(uint32_t p) const { return (uint32_t)((uint64_t)ids[map[p]] >> 32) ^ 0x80000000u; }
};

__global__ void __launch_bounds__(VW_BLOCK) k_vw_sorted(const int64_t* __restrict__ ids, const uint32_t* __restrict__ map, const uint32_t* __restrict__ cimg,
                                                        const uint32_t* __restrict__ order, uint32_t n, const uint32_t* __restrict__ cnt, int64_t* __restrict__ sid,
                                                        uint32_t* __restrict__ simg)
{
    const uint32_t i = blockIdx.x * VW_BLOCK + threadIdx.x;
    if (i >= min(n, cnt[VW_CNT_OBS])) return;
    const uint32_t p = min(order[i], n - 1u);
    sid[i] = ids[map[p]]; simg[i] = cimg[p];
}

// one thread per track (neighbouring tracks own neighbouring entries): etrack of its entries, and for a track of two or more images its row of the point table
__global__ void __launch_bounds__(VW_BLOCK) k_vw_tracks(const int64_t* __restrict__ sid, const uint32_t* __restrict__ emap, const uint32_t* __restrict__ tmap, uint32_t n,
                                                        const uint32_t* __restrict__ cnt, const int64_t* __restrict__ point_ids, uint32_t Np, uint32_t* __restrict__ etrack,
                                                        uint32_t* __restrict__ tpi, uint32_t* __restrict__ status)
{
    const uint32_t t = blockIdx.x * VW_BLOCK + threadIdx.x;
    const uint32_t E = min(n, cnt[VW_CNT_ENTRIES]), T = min(n, cnt[VW_CNT_TRACKS]);
    if (t >= T) return;
    const uint32_t e0 = tmap[t], e1 = min(t + 1 < T ? tmap[t + 1] : E, E);
    for (uint32_t e = e0; e < e1; e++) etrack[e] = t;
    uint32_t row = VW_NONE;
    if (e1 > e0 && e1 - e0 >= 2u) {
        const int64_t id = sid[emap[e0]];
        uint32_t lo = 0, hi = Np;                         // the first row with point_ids[row] >= id
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (point_ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo < Np && point_ids[lo] == id) row = lo;
        else atomicOr(status, (uint32_t)GSR_VIEWS_ERR_ABSENT);
    }
    tpi[t] = row;
}

// ioff[a] = the first entry of image a in the image-major order, a in [0, C]
__global__ void __launch_bounds__(VW_BLOCK) k_vw_image_offsets(const uint32_t* __restrict__ img_sorted, uint32_t n, const uint32_t* __restrict__ cnt, uint32_t C,
                                                               uint32_t* __restrict__ ioff)
{
    const uint32_t a = blockIdx.x * VW_BLOCK + threadIdx.x;
    if (a > C) return;
    uint32_t lo = 0, hi = min(n, cnt[VW_CNT_ENTRIES]);
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (img_sorted[mid] < a) lo = mid + 1; else hi = mid;
    }
    ioff[a] = lo;
}

// ------------------------------------------------------------------------------------------------ scores and selection
struct VwParams { double theta0, sigma1, sigma2; };

// the reference's term, operation by operation, for centres ci (the lower-indexed image) and cj
__device__ __forceinline__ double vw_term(const double* ci, const double* cj, const double* p, const VwParams& q)
{
    const double ax = ci[0] - p[0], ay = ci[1] - p[1], az = ci[2] - p[2];
    const double bx = cj[0] - p[0], by = cj[1] - p[1], bz = cj[2] - p[2];
    const double dot = (ax * bx + ay * by) + az * bz;
    const double na = sqrt((ax * ax + ay * ay) + az * az), nb = sqrt((bx * bx + by * by) + bz * bz);
    const double theta = (180.0 / 3.141592653589793) * acos(dot / na / nb);
    const double d = theta - q.theta0, s = theta <= q.theta0 ? q.sigma1 : q.sigma2;
    return exp(-(d * d) / (2.0 * (s * s)));
}

__global__ void __launch_bounds__(VW_WAVE) k_vw_score(const double* __restrict__ centres, uint32_t C, const double* __restrict__ xyz, uint32_t n,
                                                      const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ ioff, const uint32_t* __restrict__ by_image,
                                                      const uint32_t* __restrict__ etrack, const uint32_t* __restrict__ tmap, const uint32_t* __restrict__ tpi,
                                                      const uint32_t* __restrict__ emap, const uint32_t* __restrict__ eimg, VwParams q, uint32_t k,
                                                      int32_t* __restrict__ near_ids, double* __restrict__ near_scores, double* __restrict__ scores,
                                                      uint32_t* __restrict__ status)
{
    extern __shared__ double vw_row[];                    // [C]
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t Mv = min(n, cnt[VW_CNT_OBS]), E = min(n, cnt[VW_CNT_ENTRIES]), T = min(n, cnt[VW_CNT_TRACKS]);
    for (uint32_t b = lane; b < C; b += VW_WAVE) vw_row[b] = 0.0;
    const double ca[3] = { centres[3 * (size_t)a], centres[3 * (size_t)a + 1], centres[3 * (size_t)a + 2] };
    const uint32_t beg = min(ioff[a], E), end = min(ioff[a + 1], E);
    bool bad = false;
    __syncthreads();
    // what entry f of a track (row `row` of the point table) adds to column *b of image a's row, a's entry being e with multiplicity ma; *b = VW_NONE: nothing
    auto term_of = [&](uint32_t f, uint32_t e, uint32_t ma, uint32_t row, uint32_t* b) -> double {
        *b = VW_NONE;
        if (f == e) return 0.0;
        const uint32_t o = eimg[f];
        if (o >= C || o == a) return 0.0;
        const double p[3] = { xyz[3 * (size_t)row], xyz[3 * (size_t)row + 1], xyz[3 * (size_t)row + 2] };
        const double cb[3] = { centres[3 * (size_t)o], centres[3 * (size_t)o + 1], centres[3 * (size_t)o + 2] };
        double g; uint32_t m;
        if (a < o) { g = vw_term(ca, cb, p, q); m = ma; }
        else { g = vw_term(cb, ca, p, q); m = (f + 1 < E ? emap[f + 1] : Mv) - emap[f]; }
        if (!(g - g == 0.0)) bad = true;
        *b = o;
        return (double)m * g;
    };
    for (uint32_t base = beg; base < end; base += VW_WAVE) {
        // 64 of the image's entries at a time: lane l fetches what the walk needs of entry base + l.  len: the entries of its track, 0 where the track adds nothing
        uint32_t e = 0, f0 = 0, len = 0, ma = 0, row = VW_NONE;
        if (base + lane < end) {
            e = min(by_image[base + lane], E - 1u);
            const uint32_t t = min(etrack[e], T - 1u);
            f0 = tmap[t];
            const uint32_t f1 = t + 1 < T ? tmap[t + 1] : E;
            ma = (e + 1 < E ? emap[e + 1] : Mv) - emap[e];
            row = tpi[t];
            if (f1 <= E && f1 > f0 && f1 - f0 >= 2u && row != VW_NONE) len = f1 - f0;
        }
        const uint32_t incl = wave_incl_scan(len);
        const unsigned long long live = __ballot(len != 0u);
        const uint32_t here = min((uint32_t)VW_WAVE, end - base);
        uint32_t s0 = 0;
        while (s0 < here) {                               // wave-uniform: the tracks of this batch in ascending id order, as many at a time as fill the wave
            const uint32_t len0 = (uint32_t)__shfl((int)len, (int)s0, 64), start = (uint32_t)__shfl((int)incl, (int)s0, 64) - len0;
            if (len0 > VW_WAVE) {                         // a long track on its own, 64 of its entries per round; an image occurs once in a track: no two lanes meet in a column
                const uint32_t e0 = (uint32_t)__shfl((int)e, (int)s0, 64), f00 = (uint32_t)__shfl((int)f0, (int)s0, 64);
                const uint32_t ma0 = (uint32_t)__shfl((int)ma, (int)s0, 64), row0 = (uint32_t)__shfl((int)row, (int)s0, 64);
                for (uint32_t f = f00 + lane; f < f00 + len0; f += VW_WAVE) {
                    uint32_t b;
                    const double v = term_of(f, e0, ma0, row0, &b);
                    if (b != VW_NONE) vw_row[b] += v;
                }
                __syncthreads();                          // the next track may meet this one's columns from other lanes
                s0++;
                continue;
            }
            // tracks s0 .. s1 - 1 hold 64 entries or fewer together (incl ascends, so the tracks that fit are consecutive): lane l takes the l-th of these
            // entries.  The terms -- the loads and the arithmetic -- of all of them are evaluated side by side; only the additions keep the tracks' order.
            const uint32_t s1 = s0 + (uint32_t)__popcll(__ballot(lane >= s0 && lane < here && incl - start <= VW_WAVE));
            const uint32_t total = (uint32_t)__shfl((int)incl, (int)(s1 - 1u), 64) - start;
            uint32_t lo = s0, hi = s1 - 1u;               // the first track whose entries end behind this lane's
#pragma unroll
            for (int it = 0; it < 6; it++) {
                const uint32_t mid = (lo + hi) >> 1;
                const uint32_t v = (uint32_t)__shfl((int)incl, (int)mid, 64) - start;
                if (lo < hi) { if (v > lane) hi = mid; else lo = mid + 1u; }
            }
            const uint32_t es = (uint32_t)__shfl((int)e, (int)lo, 64), f0s = (uint32_t)__shfl((int)f0, (int)lo, 64), mas = (uint32_t)__shfl((int)ma, (int)lo, 64);
            const uint32_t rows = (uint32_t)__shfl((int)row, (int)lo, 64), lens = (uint32_t)__shfl((int)len, (int)lo, 64);
            const uint32_t at = lane - ((uint32_t)__shfl((int)incl, (int)lo, 64) - lens - start);      // this lane's place in its track
            uint32_t b = VW_NONE;
            double v = 0.0;
            if (lane < total && at < lens && rows != VW_NONE) v = term_of(f0s + at, es, mas, rows, &b);
            unsigned long long todo = live & (s1 < 64u ? (1ull << s1) - 1ull : ~0ull) & ~((1ull << s0) - 1ull);
            while (todo) {                                // wave-uniform
                const uint32_t s = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1ull;
                if (b != VW_NONE && lo == s) vw_row[b] += v;
                __syncthreads();                          // the next track may meet this one's columns from other lanes
            }
            s0 = s1;
        }
    }
    if (bad) atomicOr(status, (uint32_t)GSR_VIEWS_ERR_NONFINITE);
    if (scores) for (uint32_t b = lane; b < C; b += VW_WAVE) scores[(size_t)a * C + b] = vw_row[b];
    // the k best: descending score, the higher index first among equal scores.  Scores are >= 0; a column already taken holds -1.
    for (uint32_t r = 0; r < k; r++) {
        double best = -2.0; uint32_t at = VW_NONE;
        for (uint32_t b = lane; b < C; b += VW_WAVE) {
            const double s = vw_row[b];
            if (s > best || (s == best && at != VW_NONE && b > at)) { best = s; at = b; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double os = __shfl_xor(best, d, 64);
            const uint32_t oa = (uint32_t)__shfl_xor((int)at, d, 64);
            if (oa != VW_NONE && (at == VW_NONE || os > best || (os == best && oa > at))) { best = os; at = oa; }
        }
        __syncthreads();                                  // every lane has read the row
        if (lane == 0) {
            const bool ok = at < C;                       // not so only where the row holds NaN: the status word says so
            near_ids[(size_t)a * k + r] = ok ? (int32_t)at : 0;
            near_scores[(size_t)a * k + r] = ok ? best : 0.0;
            if (ok) vw_row[at] = -1.0;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static int vw_sizes(const char* who, int64_t M, int32_t C, int64_t Np)
{
    if (C < 1 || C > VW_MAX_C) { gsr_set_error("%s: C=%d images out of range [1, %d] (a row of scores is held in LDS: %d doubles)", who, C, VW_MAX_C, VW_MAX_C); return 1; }
    if (M < 0 || M >= (1ll << 31)) { gsr_set_error("%s: M=%lld observations out of range [0, 2^31)", who, (long long)M); return 1; }
    if (Np < 0 || Np >= (1ll << 31)) { gsr_set_error("%s: Np=%lld points out of range [0, 2^31)", who, (long long)Np); return 1; }
    return 0;
}

extern "C" size_t gsr_view_select_scratch_bytes(int64_t M, int32_t C)
{
    if (vw_sizes("view_select", M, C, 0)) return 0;
    return vw_carve((uint32_t)std::max<int64_t>(M, 1), (uint32_t)C, nullptr).bytes;
}

extern "C" int gsr_view_select(const double* centres, int32_t C, const int64_t* obs_offsets, const int64_t* obs_ids, int64_t M, const int64_t* point_ids,
                               const double* point_xyz, int64_t Np, double theta0, double sigma1, double sigma2, int32_t k, int32_t id_bits, int32_t* near_ids,
                               double* near_scores, double* scores, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "view_select";
    if (vw_sizes(who, M, C, Np)) return 1;
    if (k < 1 || k > C) { gsr_set_error("%s: k=%d views out of range [1, C=%d]", who, k, C); return 1; }
    if (id_bits != 32 && id_bits != 64) { gsr_set_error("%s: id_bits is 32 or 64, not %d", who, id_bits); return 1; }
    if (!(theta0 - theta0 == 0.0) || !(sigma1 > 0.0) || !(sigma2 > 0.0) || !(sigma1 - sigma1 == 0.0) || !(sigma2 - sigma2 == 0.0)) {
        gsr_set_error("%s: theta0 must be finite and sigma1, sigma2 positive finite numbers", who); return 1;
    }
    if (!centres || !obs_offsets || (M > 0 && !obs_ids) || (Np > 0 && (!point_ids || !point_xyz)) || !near_ids || !near_scores || !status_dev) {
        gsr_set_error("%s: null pointer", who); return 1;
    }
    const uint32_t n = (uint32_t)std::max<int64_t>(M, 1), Cu = (uint32_t)C;
    const VwScratch v = vw_carve(n, Cu, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, v.bytes, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s) || gsr_memset_async(v.cnt, 0, 64, s)) { gsr_set_error("%s: clear", who); return 1; }
    const uint32_t g = gsr_div_up(n, VW_BLOCK);

    hipLaunchKernelGGL(k_vw_check, dim3(gsr_div_up(std::max(3u * Cu, (uint32_t)Np), VW_BLOCK)), dim3(VW_BLOCK), 0, s, centres, Cu, obs_offsets, M, point_ids, (uint32_t)Np,
                       status_dev);
    gsr_compact(VwValidOp{obs_ids, obs_offsets, (uint32_t)M, Cu, id_bits, v.map, v.cimg, v.so.ka, status_dev}, n, v.sums, v.cnt + VW_CNT_OBS, s);
    GsrSort by_id(v.so);
    if (by_id.sort(n, v.cnt + VW_CNT_OBS, 32, true, s)) return 1;
    if (id_bits == 64 && gsr_sort_next_word(by_id, n, v.cnt + VW_CNT_OBS, VwHighOp{obs_ids, v.map}, s)) return 1;
    hipLaunchKernelGGL(k_vw_sorted, dim3(g), dim3(VW_BLOCK), 0, s, obs_ids, v.map, v.cimg, by_id.order, n, v.cnt, v.sid, v.simg);
    // the sort buffers are free again: the entries' image keys go to ka
    gsr_compact(VwEntryOp{v.sid, v.simg, v.cnt, n, v.emap, v.eimg, v.so.ka}, n, v.sums, v.cnt + VW_CNT_ENTRIES, s);
    gsr_compact(VwTrackOp{v.sid, v.emap, v.cnt, n, v.tmap}, n, v.sums, v.cnt + VW_CNT_TRACKS, s);
    hipLaunchKernelGGL(k_vw_tracks, dim3(g), dim3(VW_BLOCK), 0, s, v.sid, v.emap, v.tmap, n, v.cnt, point_ids, (uint32_t)Np, v.etrack, v.tpi,
                       status_dev);
    int img_bits = 1;
    while (img_bits < 31 && (1u << img_bits) < Cu) img_bits++;
    GsrSort by_img(v.so);
    if (by_img.sort(n, v.cnt + VW_CNT_ENTRIES, img_bits, true, s)) return 1;
    hipLaunchKernelGGL(k_vw_image_offsets, dim3(gsr_div_up(Cu + 1u, VW_BLOCK)), dim3(VW_BLOCK), 0, s, by_img.keys, n, v.cnt, Cu, v.ioff);
    const size_t lds = (size_t)Cu * sizeof(double);
    if (lds > 65536) GSR_CHECK(hipFuncSetAttribute((const void*)k_vw_score, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "view_select: LDS row");
    const VwParams q = {theta0, sigma1, sigma2};
    hipLaunchKernelGGL(k_vw_score, dim3(Cu), dim3(VW_WAVE), lds, s, centres, Cu, point_xyz, n, v.cnt, v.ioff, by_img.order, v.etrack, v.tmap, v.tpi, v.emap, v.eimg, q, (uint32_t)k,
                       near_ids, near_scores, scores, status_dev);
    return gsr_check_launch(who, s, false);
}
