// gsr_partition.hip -- the VastGaussian scene split on the device: what split_scene.py:39-53 computes through gssr/utils/vastgaussian_utils.py with one
// Python loop over every point, image and id per tile (include/gsrast.h, "scene partition").  Step 1 (which cameras found a tile) stays on the host.
//
//   boxes       one pass over the points whatever T: the T boxes sit in LDS, a thread tests its point against them 32 at a time and stores one mask
//               word per 32 tiles; the per-tile counts are wave ballots added into LDS words and from there into the T global words (integer adds:
//               the result does not depend on their order).  The same kernel takes the camera centres
//   z-range     per tile: the in-box points' float32 xyz compacted (gsr_compact.h), gsr_dist2 on the subset, then ONE workgroup reduces mean and
//               population std in float64 -- a thread adds its strided elements in ascending order, the 1024 partial sums meet in a fixed tree -- and the
//               min / max of float32 z over mean - 3 std < dist < mean + 3 std
//   visibility  md[t] by one workgroup per tile (the same fixed tree), then one thread per (tile, image): eight projections, monotone-chain hull,
//               Sutherland-Hodgman clip against the image rectangle, shoelace area, the L1 mean distance and the decision.  float64, no contraction
//   coverage    one pass over the observations: image by binary search in the offsets, row by binary search in the ascending id table, the image's
//               tile words ORed into the point's (integer atomics); then per-tile counts, and -- once the host knows them -- one compaction per tile
//               into the CSR rows, ascending row = ascending id
// Failures go to one status word per op (GSR_PART_ERR_*).  Every launch is on the caller's stream; nothing synchronises; no kernel waits for another workgroup.
#include "gsr_common.h"
#include "gsr_compact.h"
#include "gsr_scan.h"
#include <algorithm>

#define PT_BLOCK GSR_PART_BLOCK
#define PT_RED 1024           // the one workgroup of the z-range reduction
#define PT_MAX_T GSR_PART_MAX_TILES

__device__ __forceinline__ bool pt_finite(double v) { return v - v == 0.0; }

// adds, per tile of word w (tiles 32 w ..), the number of lanes whose bit is set into the LDS counters
__device__ __forceinline__ void pt_count_word(uint32_t word, uint32_t w, uint32_t T, uint32_t* cnt)
{
    const uint32_t nb = min(32u, T - 32u * w);
    for (uint32_t b = 0; b < nb; b++) {
        const unsigned long long bal = __ballot((word >> b) & 1u);
        if (bal && lane_id() == 0) atomicAdd(&cnt[32u * w + b], (uint32_t)__popcll(bal));
    }
}

// ------------------------------------------------------------------------------------------------ box membership
__global__ void __launch_bounds__(PT_BLOCK) k_pt_boxes(const double* __restrict__ xyz, uint32_t N, uint32_t stride, const double* __restrict__ boxes, uint32_t T, uint32_t W,
                                                       uint32_t* __restrict__ mask, uint32_t* __restrict__ counts, uint32_t* __restrict__ status)
{
    extern __shared__ double pt_box[];                    // [4 T] boxes, then T counters
    uint32_t* cnt = (uint32_t*)(pt_box + 4 * (size_t)T);
    bool bad = false;
    for (uint32_t j = threadIdx.x; j < 4 * T; j += PT_BLOCK) { const double v = boxes[j]; pt_box[j] = v; bad |= v != v; }
    for (uint32_t j = threadIdx.x; j < T; j += PT_BLOCK) cnt[j] = 0;
    if (bad && blockIdx.x == 0) atomicOr(status, (uint32_t)GSR_PART_ERR_NONFINITE);
    __syncthreads();
    const uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x;
    const bool in = i < N;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double x = in ? xyz[(size_t)i * stride] : nan, y = in ? xyz[(size_t)i * stride + 1] : nan;      // NaN is inside no box
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t nb = min(32u, T - 32u * w);
        uint32_t word = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const double* bx = pt_box + 4 * (size_t)(32u * w + b);
            if (x >= bx[0] && x <= bx[1] && y >= bx[2] && y <= bx[3]) word |= 1u << b;
        }
        if (in) mask[(size_t)i * W + w] = word;
        pt_count_word(word, w, T, cnt);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < T; j += PT_BLOCK) if (cnt[j]) atomicAdd(&counts[j], cnt[j]);
}

// per-tile counts of a mask [n, W]
__global__ void __launch_bounds__(PT_BLOCK) k_pt_count(const uint32_t* __restrict__ mask, uint32_t n, uint32_t T, uint32_t W, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t cnt[PT_MAX_T];
    for (uint32_t j = threadIdx.x; j < T; j += PT_BLOCK) cnt[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x;
    for (uint32_t w = 0; w < W; w++) pt_count_word(i < n ? mask[(size_t)i * W + w] : 0u, w, T, cnt);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < T; j += PT_BLOCK) if (cnt[j]) atomicAdd(&counts[j], cnt[j]);
}

// ------------------------------------------------------------------------------------------------ tile z-range
struct PtSubOp {
    const double* xyz; const uint32_t* mask; uint32_t n, W, t, cap; float* sub; uint32_t* status;
    __device__ bool keep(uint32_t i) const { return i < n && ((mask[(size_t)i * W + (t >> 5)] >> (t & 31u)) & 1u); }
    __device__ void place(uint32_t i, uint32_t p) const
    {
        if (p >= cap) return;                             // more bits than the caller's count: k_pt_zrange reports it
        const float x = (float)xyz[3 * (size_t)i], y = (float)xyz[3 * (size_t)i + 1], z = (float)xyz[3 * (size_t)i + 2];
        sub[3 * (size_t)p] = x; sub[3 * (size_t)p + 1] = y; sub[3 * (size_t)p + 2] = z;
        if (!(x - x == 0.f) || !(y - y == 0.f) || !(z - z == 0.f)) atomicOr(status, (uint32_t)GSR_PART_ERR_NONFINITE);
    }
};

// the sum of the workgroup's 1024 values in a fixed tree; every thread gets it
__device__ __forceinline__ double pt_block_sum(double v, double* lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = PT_RED / 2; d >= 1; d >>= 1) {
        if (threadIdx.x < d) lds[threadIdx.x] += lds[threadIdx.x + d];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(PT_RED) k_pt_zrange(const float* __restrict__ sub, const float* __restrict__ dist, uint32_t n, const uint32_t* __restrict__ n_dev, uint32_t t,
                                                      float* __restrict__ zrange, double* __restrict__ stats, uint32_t* __restrict__ status)
{
    __shared__ double lds[PT_RED];
    __shared__ float fmin_[PT_RED], fmax_[PT_RED];
    __shared__ uint32_t kept_[PT_RED];
    const uint32_t tid = threadIdx.x;
    uint32_t err = 0;
    if (*n_dev != n) err = GSR_PART_ERR_COUNT;
    else if (n < 4u) err = GSR_PART_ERR_FEW;
    if (err) {                                            // uniform over the workgroup
        if (tid == 0) { atomicOr(status, err); zrange[2 * t] = 0.f; zrange[2 * t + 1] = 0.f; stats[2 * t] = 0.0; stats[2 * t + 1] = 0.0; }
        return;
    }
    double s = 0.0;
    for (uint32_t i = tid; i < n; i += PT_RED) s += (double)dist[i];
    const double mean = pt_block_sum(s, lds) / (double)n;
    s = 0.0;
    for (uint32_t i = tid; i < n; i += PT_RED) { const double d = (double)dist[i] - mean; s += d * d; }
    const double sd = sqrt(pt_block_sum(s, lds) / (double)n);
    const double lo = mean - 3.0 * sd, hi = mean + 3.0 * sd;
    float zmin = 3.402823466e+38f, zmax = -3.402823466e+38f;
    uint32_t kept = 0;
    for (uint32_t i = tid; i < n; i += PT_RED) {
        const double d = (double)dist[i];
        if (d > lo && d < hi) { const float z = sub[3 * (size_t)i + 2]; zmin = fminf(zmin, z); zmax = fmaxf(zmax, z); kept++; }
    }
    fmin_[tid] = zmin; fmax_[tid] = zmax; kept_[tid] = kept;
    __syncthreads();
    for (uint32_t d = PT_RED / 2; d >= 1; d >>= 1) {
        if (tid < d) { fmin_[tid] = fminf(fmin_[tid], fmin_[tid + d]); fmax_[tid] = fmaxf(fmax_[tid], fmax_[tid + d]); kept_[tid] += kept_[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (!pt_finite(lo) || !pt_finite(hi)) err |= GSR_PART_ERR_NONFINITE;
        else if (kept_[0] == 0u) err |= GSR_PART_ERR_FEW;   // every distance equal: the strict inequalities keep nothing
        if (err) atomicOr(status, err);
        zrange[2 * t] = err ? 0.f : fmin_[0]; zrange[2 * t + 1] = err ? 0.f : fmax_[0];
        stats[2 * t] = mean; stats[2 * t + 1] = sd;
    }
}

// ------------------------------------------------------------------------------------------------ visibility
// corner k of tile t's box, in the reference's order: x = k & 4 ? Mx : mx, y = k & 2 ? My : my, z = k & 1 ? Mz : mz
__device__ __forceinline__ void pt_corner(const double* bx, double mz, double Mz, int k, double* X, double* Y, double* Z)
{
    *X = (k & 4) ? bx[1] : bx[0]; *Y = (k & 2) ? bx[3] : bx[2]; *Z = (k & 1) ? Mz : mz;
}

__global__ void __launch_bounds__(PT_BLOCK) k_pt_md(const double* __restrict__ boxes, const float* __restrict__ zrange, const double* __restrict__ centres, uint32_t C,
                                                    const uint32_t* __restrict__ member, uint32_t W, double* __restrict__ md)
{
    __shared__ double sum_[PT_BLOCK];
    __shared__ uint32_t num_[PT_BLOCK];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const double* bx = boxes + 4 * (size_t)t;
    const double mz = (double)zrange[2 * t], Mz = (double)zrange[2 * t + 1];
    double s = 0.0;
    uint32_t k = 0;
    for (uint32_t c = tid; c < C; c += PT_BLOCK) {
        if (!((member[(size_t)c * W + (t >> 5)] >> (t & 31u)) & 1u)) continue;
        const double c0 = centres[3 * (size_t)c], c1 = centres[3 * (size_t)c + 1], c2 = centres[3 * (size_t)c + 2];
        double far = 0.0;
        for (int q = 0; q < 8; q++) {
            double X, Y, Z;
            pt_corner(bx, mz, Mz, q, &X, &Y, &Z);
            const double dx = c0 - X, dy = c1 - Y, dz = c2 - Z;
            far = fmax(far, sqrt((dx * dx + dy * dy) + dz * dz));
        }
        s += far; k++;
    }
    sum_[tid] = s; num_[tid] = k;
    __syncthreads();
    for (uint32_t d = PT_BLOCK / 2; d >= 1; d >>= 1) {
        if (tid < d) { sum_[tid] += sum_[tid + d]; num_[tid] += num_[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) md[t] = sum_[0] / (double)num_[0] * 1.2;      // no member: NaN, and d < md holds for no image (the reference's empty mean)
}

#define PT_POLY 16            // 8 hull vertices, and a clip edge adds at most one to a convex polygon

// keeps the part of the convex polygon with coordinate `axis` >= bound (ge) or <= bound; -> the number of vertices
__device__ int pt_clip(const double* ix, const double* iy, int n, double* ox, double* oy, int axis, double bound, bool ge)
{
    int m = 0;
    for (int i = 0; i < n; i++) {
        const int j = i == 0 ? n - 1 : i - 1;
        const double cx = ix[i], cy = iy[i], px = ix[j], py = iy[j];
        const double cv = axis ? cy : cx, pv = axis ? py : px;
        const bool cin = ge ? cv >= bound : cv <= bound, pin = ge ? pv >= bound : pv <= bound;
        if (cin != pin && m < PT_POLY) {
            const double f = (bound - pv) / (cv - pv);
            ox[m] = axis ? px + f * (cx - px) : bound;
            oy[m] = axis ? bound : py + f * (cy - py);
            m++;
        }
        if (cin && m < PT_POLY) { ox[m] = cx; oy[m] = cy; m++; }
    }
    return m;
}

__global__ void __launch_bounds__(PT_BLOCK) k_pt_visibility(const double* __restrict__ boxes, const float* __restrict__ zrange, uint32_t T, const double* __restrict__ w2c,
                                                            const double* __restrict__ centres, const double* __restrict__ intr, uint32_t C,
                                                            const uint32_t* __restrict__ member, uint32_t W, double threshold, const double* __restrict__ md,
                                                            double* __restrict__ ratio, double* __restrict__ dist, uint8_t* __restrict__ add, uint32_t* __restrict__ status)
{
    const uint32_t idx = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (idx >= T * C) return;
    const uint32_t t = idx / C, c = idx - t * C;
    const double* bx = boxes + 4 * (size_t)t;
    const double mz = (double)zrange[2 * t], Mz = (double)zrange[2 * t + 1];
    const double* E = w2c + 12 * (size_t)c;               // rows of [R | t]
    const double fx = intr[4 * (size_t)c], fy = intr[4 * (size_t)c + 1], wd = intr[4 * (size_t)c + 2], ht = intr[4 * (size_t)c + 3];
    const double hw = wd / 2.0, hh = ht / 2.0;
    const double c0 = centres[3 * (size_t)c], c1 = centres[3 * (size_t)c + 1], c2 = centres[3 * (size_t)c + 2];
    double u[8], v[8], l1[8];
    bool bad = false, zero = false;
    for (int q = 0; q < 8; q++) {
        double X, Y, Z;
        pt_corner(bx, mz, Mz, q, &X, &Y, &Z);
        const double xc = ((E[0] * X + E[1] * Y) + E[2] * Z) + E[3];
        const double yc = ((E[4] * X + E[5] * Y) + E[6] * Z) + E[7];
        const double zc = ((E[8] * X + E[9] * Y) + E[10] * Z) + E[11];
        if (zc == 0.0) zero = true;
        u[q] = (fx * xc + hw * zc) / zc;                  // K's principal point is the image's middle; a corner behind the camera is mirrored, as in the reference
        v[q] = (fy * yc + hh * zc) / zc;
        l1[q] = (fabs(X - c0) + fabs(Y - c1)) + fabs(Z - c2);
        if (!pt_finite(u[q]) || !pt_finite(v[q]) || !pt_finite(l1[q])) bad = true;
    }
    const double d = (((l1[0] + l1[1]) + (l1[2] + l1[3])) + ((l1[4] + l1[5]) + (l1[6] + l1[7]))) / 8.0;
    if (zero || bad || !pt_finite(wd * ht)) {
        atomicOr(status, zero ? (uint32_t)GSR_PART_ERR_ZERO_Z : (uint32_t)GSR_PART_ERR_NONFINITE);
        ratio[idx] = 0.0; dist[idx] = d; add[idx] = 0;
        return;
    }
    // the eight points in ascending (u, v), then Andrew's monotone chain: counter-clockwise, collinear points dropped
    int ord[8];
    for (int q = 0; q < 8; q++) {
        int p = q;
        while (p > 0 && (u[ord[p - 1]] > u[q] || (u[ord[p - 1]] == u[q] && v[ord[p - 1]] > v[q]))) { ord[p] = ord[p - 1]; p--; }
        ord[p] = q;
    }
    double ax[PT_POLY], ay[PT_POLY], bxp[PT_POLY], byp[PT_POLY];
    int n = 0, least = 2;                                 // least: a chain pops only down to its own first edge
    for (int s = 0; s < 15; s++) {                        // the lower chain left to right (s < 8), then the upper chain back over ord[6] .. ord[0]
        if (s == 8) least = n + 1;
        const int q = s < 8 ? ord[s] : ord[14 - s];
        while (n >= least && (ax[n - 1] - ax[n - 2]) * (v[q] - ay[n - 2]) - (ay[n - 1] - ay[n - 2]) * (u[q] - ax[n - 2]) <= 0.0) n--;
        if (n < PT_POLY) { ax[n] = u[q]; ay[n] = v[q]; n++; }      // at most 15 vertices are ever held
    }
    n--;                                                  // the first vertex came round again
    double area = 0.0;
    if (n >= 3) {
        int m = pt_clip(ax, ay, n, bxp, byp, 0, 0.0, true);
        m = pt_clip(bxp, byp, m, ax, ay, 0, wd, false);
        m = pt_clip(ax, ay, m, bxp, byp, 1, 0.0, true);
        m = pt_clip(bxp, byp, m, ax, ay, 1, ht, false);
        double s2 = 0.0;
        for (int i = 0; i < m; i++) { const int j = i + 1 == m ? 0 : i + 1; s2 += ax[i] * ay[j] - ax[j] * ay[i]; }
        area = 0.5 * fabs(s2);
    }
    const double r = area / (wd * ht);
    const bool is_member = (member[(size_t)c * W + (t >> 5)] >> (t & 31u)) & 1u;
    if (!pt_finite(r)) atomicOr(status, (uint32_t)GSR_PART_ERR_NONFINITE);
    ratio[idx] = r; dist[idx] = d;
    add[idx] = (!is_member && r > threshold && d < md[t]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ coverage
__global__ void __launch_bounds__(PT_BLOCK) k_pt_cover_check(const int64_t* __restrict__ offsets, uint32_t C, int64_t M, const int64_t* __restrict__ point_ids, uint32_t Np,
                                                             uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x;
    uint32_t err = 0;
    if (i < C && offsets[i] > offsets[i + 1]) err |= GSR_PART_ERR_OFFSETS;
    if (i == 0 && (offsets[0] != 0 || offsets[C] != M)) err |= GSR_PART_ERR_OFFSETS;
    if (i + 1 < Np && point_ids[i] >= point_ids[i + 1]) err |= GSR_PART_ERR_TABLE;
    if (err) atomicOr(status, err);
}

__global__ void __launch_bounds__(PT_BLOCK) k_pt_cover(const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, uint32_t M, uint32_t C,
                                                       const uint32_t* __restrict__ image_mask, uint32_t W, const int64_t* __restrict__ point_ids, uint32_t Np,
                                                       uint32_t* __restrict__ point_mask, uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= M) return;
    const int64_t id = ids[i];
    if (id == -1) return;
    uint32_t lo = 0, hi = C;                              // the image of slot i: the last a with offsets[a] <= i
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= (int64_t)i) lo = mid; else hi = mid;
    }
    const uint32_t* im = image_mask + (size_t)lo * W;
    uint32_t any = 0;
    for (uint32_t w = 0; w < W; w++) any |= im[w];
    if (!any) return;                                     // an image of no tile: its ids are never looked up
    uint32_t a = 0, b = Np;                               // the first row with point_ids[row] >= id
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (point_ids[mid] < id) a = mid + 1; else b = mid;
    }
    if (a >= Np || point_ids[a] != id) { atomicOr(status, (uint32_t)GSR_PART_ERR_ABSENT); return; }
    uint32_t* pm = point_mask + (size_t)a * W;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t m = im[w];
        if (m && (__atomic_load_n(pm + w, __ATOMIC_RELAXED) & m) != m) atomicOr(pm + w, m);      // a stale read only repeats an OR
    }
}

struct PtRowsOp {
    const uint32_t* mask; uint32_t n, W, t, cap; int64_t* rows;
    __device__ bool keep(uint32_t i) const { return i < n && ((mask[(size_t)i * W + (t >> 5)] >> (t & 31u)) & 1u); }
    __device__ void place(uint32_t i, uint32_t p) const { if (p < cap) rows[p] = (int64_t)i; }
};

// ------------------------------------------------------------------------------------------------ entry points
static int pt_sizes(const char* who, int64_t n, const char* what, int32_t T)
{
    if (T < 1 || T > PT_MAX_T) { gsr_set_error("%s: T=%d tiles out of range [1, %d] (the boxes and their counters are held in LDS)", who, T, PT_MAX_T); return 1; }
    if (n < 0 || n >= (1ll << 31)) { gsr_set_error("%s: %s=%lld out of range [0, 2^31)", who, what, (long long)n); return 1; }
    return 0;
}

extern "C" int gsr_partition_boxes(const double* xyz, int64_t N, int32_t stride, const double* boxes, int32_t T, uint32_t* mask, uint32_t* counts, uint32_t* status_dev,
                                   void* stream)
{
    const char* who = "partition_boxes";
    if (pt_sizes(who, N, "N", T)) return 1;
    if (stride < 2) { gsr_set_error("%s: stride=%d: a row holds x and y at least", who, stride); return 1; }
    if ((N > 0 && (!xyz || !mask)) || !boxes || !counts || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s) || gsr_memset_async(counts, 0, 4 * (size_t)T, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (N > 0) {
        const uint32_t W = gsr_div_up((uint32_t)T, 32);
        hipLaunchKernelGGL(k_pt_boxes, dim3(gsr_div_up((uint32_t)N, PT_BLOCK)), dim3(PT_BLOCK), (size_t)T * 36, s, xyz, (uint32_t)N, (uint32_t)stride, boxes, (uint32_t)T, W,
                           mask, counts, status_dev);
    }
    return gsr_check_launch(who, s, false);
}

struct PtZScratch { uint32_t *cnt, *sums; float *sub, *dist; void* knn; size_t knn_bytes, bytes; };
static PtZScratch pt_zcarve(uint32_t N, uint32_t n_max, const void* base)
{
    PtZScratch z; GsrCarve c(base);
    z.cnt = c.take<uint32_t>(16);
    z.sums = c.take<uint32_t>(gsr_compact_sums_words(N));
    z.sub = c.take<float>(3 * (size_t)std::max(n_max, 1u));
    z.dist = c.take<float>(std::max(n_max, 1u));
    z.knn_bytes = gsr_dist2_scratch_bytes((int32_t)n_max);
    z.knn = c.take<char>(z.knn_bytes);
    z.bytes = c.bytes();
    return z;
}

extern "C" size_t gsr_partition_zrange_scratch_bytes(int64_t N, int64_t n_max)
{
    if (N < 0 || N >= (1ll << 31) || n_max < 0 || n_max > N) return 0;
    return pt_zcarve((uint32_t)N, (uint32_t)n_max, nullptr).bytes;
}

extern "C" int gsr_partition_zrange(const double* xyz, int64_t N, const uint32_t* mask, int32_t T, int32_t tile, int64_t count, int64_t n_max, float* zrange, double* stats,
                                    void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    const char* who = "partition_zrange";
    if (pt_sizes(who, N, "N", T)) return 1;
    if (tile < 0 || tile >= T) { gsr_set_error("%s: tile=%d out of range [0, T=%d)", who, tile, T); return 1; }
    if (count < 0 || count > n_max || n_max > N) { gsr_set_error("%s: count=%lld, n_max=%lld, N=%lld: expected 0 <= count <= n_max <= N", who, (long long)count, (long long)n_max, (long long)N); return 1; }
    if ((N > 0 && (!xyz || !mask)) || !zrange || !stats || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    const PtZScratch z = pt_zcarve((uint32_t)N, (uint32_t)n_max, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, z.bytes, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t W = gsr_div_up((uint32_t)T, 32), n = (uint32_t)count;
    if (gsr_memset_async(z.cnt, 0, 64, s)) { gsr_set_error("%s: clear", who); return 1; }
    if (N > 0) gsr_compact(PtSubOp{xyz, mask, (uint32_t)N, W, (uint32_t)tile, n, z.sub, status_dev}, (uint32_t)N, z.sums, z.cnt, s);
    if (n >= 4u && gsr_dist2((int32_t)n, z.sub, z.dist, z.knn, z.knn_bytes, stream)) return 1;
    hipLaunchKernelGGL(k_pt_zrange, dim3(1), dim3(PT_RED), 0, s, z.sub, z.dist, n, z.cnt, (uint32_t)tile, zrange, stats, status_dev);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_partition_visibility(const double* boxes, const float* zrange, int32_t T, const double* w2c, const double* centres, const double* intr, int32_t C,
                                        const uint32_t* member, double threshold, double* ratio, double* dist, double* md, uint8_t* add, uint32_t* status_dev, void* stream)
{
    const char* who = "partition_visibility";
    if (pt_sizes(who, C, "C", T)) return 1;
    if (C < 1 || (int64_t)T * C >= (1ll << 31)) { gsr_set_error("%s: C=%d images with T=%d tiles: expected C >= 1 and T C < 2^31", who, C, T); return 1; }
    if (!(threshold - threshold == 0.0)) { gsr_set_error("%s: threshold must be finite", who); return 1; }
    if (!boxes || !zrange || !w2c || !centres || !intr || !member || !ratio || !dist || !md || !add || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 4, s)) { gsr_set_error("%s: clear", who); return 1; }
    const uint32_t W = gsr_div_up((uint32_t)T, 32);
    hipLaunchKernelGGL(k_pt_md, dim3((uint32_t)T), dim3(PT_BLOCK), 0, s, boxes, zrange, centres, (uint32_t)C, member, W, md);
    hipLaunchKernelGGL(k_pt_visibility, dim3(gsr_div_up((uint32_t)T * (uint32_t)C, PT_BLOCK)), dim3(PT_BLOCK), 0, s, boxes, zrange, (uint32_t)T, w2c, centres, intr, (uint32_t)C,
                       member, W, threshold, md, ratio, dist, add, status_dev);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_partition_coverage_mask(const int64_t* obs_offsets, const int64_t* obs_ids, int64_t M, const uint32_t* image_mask, int32_t C, const int64_t* point_ids,
                                           int64_t Np, int32_t T, uint32_t* point_mask, uint32_t* counts, uint32_t* status_dev, void* stream)
{
    const char* who = "partition_coverage_mask";
    if (pt_sizes(who, M, "M", T) || pt_sizes(who, Np, "Np", T)) return 1;
    if (C < 1) { gsr_set_error("%s: C=%d: expected at least one image", who, C); return 1; }
    if (!obs_offsets || (M > 0 && !obs_ids) || !image_mask || (Np > 0 && (!point_ids || !point_mask)) || !counts || !status_dev) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t W = gsr_div_up((uint32_t)T, 32);
    if (gsr_memset_async(status_dev, 0, 4, s) || gsr_memset_async(counts, 0, 4 * (size_t)T, s) ||
        (Np > 0 && gsr_memset_async(point_mask, 0, 4 * (size_t)Np * W, s))) { gsr_set_error("%s: clear", who); return 1; }
    hipLaunchKernelGGL(k_pt_cover_check, dim3(gsr_div_up(std::max((uint32_t)C, (uint32_t)Np), PT_BLOCK)), dim3(PT_BLOCK), 0, s, obs_offsets, (uint32_t)C, M, point_ids, (uint32_t)Np,
                       status_dev);
    if (M > 0) hipLaunchKernelGGL(k_pt_cover, dim3(gsr_div_up((uint32_t)M, PT_BLOCK)), dim3(PT_BLOCK), 0, s, obs_offsets, obs_ids, (uint32_t)M, (uint32_t)C, image_mask, W, point_ids,
                                  (uint32_t)Np, point_mask, status_dev);
    if (Np > 0) hipLaunchKernelGGL(k_pt_count, dim3(gsr_div_up((uint32_t)Np, PT_BLOCK)), dim3(PT_BLOCK), 0, s, point_mask, (uint32_t)Np, (uint32_t)T, W, counts);
    return gsr_check_launch(who, s, false);
}

extern "C" size_t gsr_partition_coverage_rows_scratch_bytes(int64_t Np)
{
    if (Np < 0 || Np >= (1ll << 31)) return 0;
    GsrCarve c(nullptr);
    c.take<uint32_t>(16); c.take<uint32_t>(gsr_compact_sums_words((size_t)Np));
    return c.bytes();
}

extern "C" int gsr_partition_coverage_rows(const uint32_t* point_mask, int64_t Np, int32_t T, const int64_t* tile_offsets, int64_t* rows, void* scratch, size_t scratch_bytes,
                                           void* stream)
{
    const char* who = "partition_coverage_rows";
    if (pt_sizes(who, Np, "Np", T)) return 1;
    if (!tile_offsets || tile_offsets[0] != 0) { gsr_set_error("%s: tile_offsets must start at 0", who); return 1; }
    for (int32_t t = 0; t < T; t++)
        if (tile_offsets[t + 1] < tile_offsets[t] || tile_offsets[t + 1] - tile_offsets[t] > Np) { gsr_set_error("%s: tile_offsets[%d..%d] does not ascend by at most Np", who, t, t + 1); return 1; }
    if (tile_offsets[T] > 0 && (!point_mask || !rows)) { gsr_set_error("%s: null pointer", who); return 1; }
    GsrCarve c(scratch);
    uint32_t* cnt = c.take<uint32_t>(16);
    uint32_t* sums = c.take<uint32_t>(gsr_compact_sums_words((size_t)Np));
    if (gsr_scratch_check(who, scratch, scratch_bytes, c.bytes(), false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t W = gsr_div_up((uint32_t)T, 32);
    for (int32_t t = 0; t < T; t++) {
        const uint32_t cap = (uint32_t)(tile_offsets[t + 1] - tile_offsets[t]);
        if (cap) gsr_compact(PtRowsOp{point_mask, (uint32_t)Np, W, (uint32_t)t, cap, rows + tile_offsets[t]}, (uint32_t)Np, sums, cnt, s);
    }
    return gsr_check_launch(who, s, false);
}
