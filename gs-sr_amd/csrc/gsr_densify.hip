// gsr_densify.hip -- densify / clone / split / prune of the explicit Gaussians on the device (include/gsrast.h gsr_densify_*).
//
// The reference (VanillaGaussian.densify_and_prune, gssr/gaussian/vanilla_gaussian.py:295-426; twod_gaussian.py:22-46; pgsr_gaussian.py:43-155)
// rebuilds all 6 parameters and 12 Adam moments four times (cat for the clones, cat for the children, a boolean gather for the split parents, a
// boolean gather for the final prune).  Here one pass classifies every original (k_den_count / k_den_place: flags, six prefix sums, the
// output-row -> source-row map) and one launch of the row mover (gsr_rows.hip) writes every output row once; k_den_compute then overwrites the
// few computed columns (children's xyz and scaling, PGSR clones' xyz).
//
// This unit is built with -ffp-contract=off: the selections are comparisons of float32 quotients and must not depend on FMA contraction.
#include "gsr_common.h"
#include <vector>

#define DEN_BLOCK 1024
#define DEN_NQ 6                    // scanned flags, in status order: clone, split, original kept, clone kept, children kept, split by the gradient rule
#define DEN_F_CLONE 1u
#define DEN_F_SPLIT 2u
#define DEN_F_KEEP_O 4u
#define DEN_F_KEEP_C 8u
#define DEN_F_KEEP_S 16u
#define DEN_F_SPLIT_G 32u
#define DEN_CNT 16                  // words of device counters

// classification of original i (see include/gsrast.h)
__device__ __forceinline__ uint32_t den_classify(const gsr_densify_args& A, uint32_t i)
{
    float g = __fdiv_rn(A.accum[i], A.denom[i]);
    if (g != g) g = 0.0f;
    const float* s = A.scaling + (size_t)i * A.scaling_cols;
    float ms = fmaxf(s[0], s[1]);
    if (A.scaling_cols == 3) ms = fmaxf(ms, s[2]);
    const bool big = ms > A.dense_thr;
    const bool c0 = fabsf(g) >= A.clone_thr && ms <= A.dense_thr;
    const bool s0 = g >= A.split_thr && big;
    const float vc = c0 ? g : 0.0f, vs = s0 ? g : 0.0f;
    const bool clone = (A.flags & GSR_DEN_CLONE_CAP) ? (vc > A.clone_cap) : c0;
    bool sg, sa = false;
    float va = 0.0f;
    if (A.accum_abs) {
        float ga = __fdiv_rn(A.accum_abs[i], A.denom_abs[i]);
        if (ga != ga) ga = 0.0f;
        va = (!s0 && big && A.max_radii2D[i] > A.abs_radii_thr) ? ga : 0.0f;
    }
    if (A.flags & GSR_DEN_SPLIT_CAP) sg = vs > A.split_cap;
    else {
        sg = s0;
        if (A.accum_abs) sa = (A.flags & GSR_DEN_ABS_CAP) ? (va > A.abs_cap) : (va >= A.abs_thr);
    }
    if (A.masked_out) { A.masked_out[i] = vc; A.masked_out[(size_t)A.P + i] = vs; A.masked_out[2 * (size_t)A.P + i] = va; }
    const bool split = (sg || sa) && !clone;                  // a clone is never split (its padded gradient is 0)
    const bool low = A.opacity[i] < A.min_opacity, size = (A.flags & GSR_DEN_SIZE_PRUNE) != 0;
    const bool prune_self = low || (size && ms > A.world_thr);
    const bool prune_child = low || (size && __fdiv_rn(ms, A.child_div) > A.world_thr);
    uint32_t f = 0;
    if (clone) f |= DEN_F_CLONE;
    if (split) f |= DEN_F_SPLIT;
    if (split && sg) f |= DEN_F_SPLIT_G;
    if (!split && !prune_self) f |= DEN_F_KEEP_O;
    if (clone && !prune_self) f |= DEN_F_KEEP_C;
    if (split && !prune_child) f |= DEN_F_KEEP_S;
    return f;
}

// exclusive ranks of the DEN_NQ flag bits of f inside the block (wave ballot + popcount, wave totals through LDS), and the block totals
__device__ __forceinline__ void den_block_ranks(uint32_t f, uint32_t (*wsum)[DEN_NQ], uint32_t* rank, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < DEN_NQ; q++) {
        const uint64_t b = __ballot((f >> q) & 1u);
        rank[q] = (uint32_t)__popcll(b & below);
        if (lane == 0) wsum[wave][q] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < DEN_NQ; q++) {
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < DEN_BLOCK / 64; w++) { const uint32_t v = wsum[w][q]; all += v; before += (w < wave) ? v : 0u; }
        rank[q] += before;
        total[q] = all;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(DEN_BLOCK) k_den_count(gsr_densify_args A, uint8_t* __restrict__ flags, uint32_t* __restrict__ sums, uint32_t stride)
{
    __shared__ uint32_t wsum[DEN_BLOCK / 64][DEN_NQ];
    const uint32_t i = blockIdx.x * DEN_BLOCK + threadIdx.x;
    uint32_t f = 0;
    if (i < (uint32_t)A.P) { f = den_classify(A, i); flags[i] = (uint8_t)f; }
    uint32_t rank[DEN_NQ], total[DEN_NQ];
    den_block_ranks(f, wsum, rank, total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < DEN_NQ; q++) sums[(size_t)q * stride + blockIdx.x] = total[q];
    }
}

// rank[i]: position of i among the clones (a clone) or among the splits (a split parent); map: output row -> source row.
// map has P * max(2, N) words: an original yields itself and a clone, or N children, never more.
__global__ void __launch_bounds__(DEN_BLOCK) k_den_place(uint32_t P, uint32_t N, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums, uint32_t stride,
                                                         const uint32_t* __restrict__ counters, uint32_t* __restrict__ rank_out, uint32_t* __restrict__ map)
{
    __shared__ uint32_t wsum[DEN_BLOCK / 64][DEN_NQ];
    const uint32_t i = blockIdx.x * DEN_BLOCK + threadIdx.x;
    const uint32_t f = i < P ? flags[i] : 0u;
    uint32_t rank[DEN_NQ], total[DEN_NQ];
    den_block_ranks(f, wsum, rank, total);
    if (i >= P) return;
#pragma unroll
    for (int q = 0; q < DEN_NQ; q++) rank[q] += sums[(size_t)q * stride + blockIdx.x];
    const uint32_t nO = counters[2], nC = counters[3], nS = counters[4];
    rank_out[i] = (f & DEN_F_CLONE) ? rank[0] : rank[1];
    if (f & DEN_F_KEEP_O) map[rank[2]] = i;
    if (f & DEN_F_KEEP_C) map[(size_t)nO + rank[3]] = i;
    if (f & DEN_F_KEEP_S)
        for (uint32_t r = 0; r < N; r++) map[(size_t)nO + nC + (size_t)r * nS + rank[4]] = i;
}

// ---------------------------------------------------------------------------------------------------------------- computed columns
// build_rotation (gssr/utils/general_utils.py:78-99) of the raw quaternion, times (z * s), plus the parent's position
__device__ __forceinline__ void den_sample(const float* __restrict__ q4, const float* __restrict__ s, int cols, const float* __restrict__ z, const float* __restrict__ p,
                                           float* __restrict__ out)
{
    const float a = q4[0], b = q4[1], c = q4[2], d = q4[3];
    const float norm = sqrtf(a * a + b * b + c * c + d * d);
    const float r = __fdiv_rn(a, norm), x = __fdiv_rn(b, norm), y = __fdiv_rn(c, norm), w = __fdiv_rn(d, norm);
    const float v0 = z[0] * s[0], v1 = z[1] * s[1], v2 = cols == 3 ? z[2] * s[2] : 0.0f;
    const float R00 = 1.0f - 2.0f * (y * y + w * w), R01 = 2.0f * (x * y - r * w), R02 = 2.0f * (x * w + r * y);
    const float R10 = 2.0f * (x * y + r * w), R11 = 1.0f - 2.0f * (x * x + w * w), R12 = 2.0f * (y * w - r * x);
    const float R20 = 2.0f * (x * w - r * y), R21 = 2.0f * (y * w + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
    out[0] = (R00 * v0 + R01 * v1 + R02 * v2) + p[0];
    out[1] = (R10 * v0 + R11 * v1 + R12 * v2) + p[1];
    out[2] = (R20 * v0 + R21 * v1 + R22 * v2) + p[2];
}

__global__ void __launch_bounds__(256) k_den_compute(gsr_densify_args A, gsr_densify_compute Cc, const uint32_t* __restrict__ map, const uint32_t* __restrict__ rank,
                                                     uint32_t S, uint32_t nO, uint32_t nC, uint32_t nS, uint32_t n_clone_rows, uint32_t total)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const bool child = t >= n_clone_rows;
    const uint32_t u = t - (child ? n_clone_rows : 0u);
    const size_t row = child ? (size_t)nO + nC + u : (size_t)nO + u;
    const uint32_t i = map[row];
    if (i >= (uint32_t)A.P) return;
    const float* s = A.scaling + (size_t)i * A.scaling_cols;
    const float* z = child ? Cc.noise_split + 3 * ((size_t)(u / nS) * S + rank[i]) : Cc.noise_clone + 3 * (size_t)rank[i];
    den_sample(Cc.rotation + 4 * (size_t)i, s, A.scaling_cols, z, Cc.xyz + 3 * (size_t)i, Cc.xyz_dst + 3 * row);
    if (child)
        for (int c = 0; c < A.scaling_cols; c++) Cc.scaling_dst[row * A.scaling_cols + c] = logf(__fdiv_rn(s[c], A.child_div));
}

// ---------------------------------------------------------------------------------------------------------------- host
struct DenScratch { uint8_t* flags; uint32_t *rank, *sums, *counters, *map; uint32_t nblk, stride; size_t bytes; };
static DenScratch den_carve(uint32_t P, uint32_t N, const void* base)
{
    DenScratch d; GsrCarve c(base);
    const size_t n = P > 0 ? P : 1;
    d.nblk = gsr_div_up((uint32_t)n, DEN_BLOCK); d.stride = d.nblk + 1;
    d.flags = c.take<uint8_t>(n); d.rank = c.take<uint32_t>(n);
    d.sums = c.take<uint32_t>((size_t)DEN_NQ * d.stride); d.counters = c.take<uint32_t>(DEN_CNT);
    d.map = c.take<uint32_t>(n * (N > 2 ? N : 2));
    d.bytes = c.bytes();
    return d;
}

static int den_check(const gsr_densify_args* a, const char* who)
{
    if (!a) { gsr_set_error("%s: args is NULL", who); return 1; }
    if (a->P < 0) { gsr_set_error("%s: P=%d must be >= 0", who, a->P); return 1; }
    if (a->N < 1) { gsr_set_error("%s: N=%d must be >= 1", who, a->N); return 1; }
    if (a->scaling_cols != 2 && a->scaling_cols != 3) { gsr_set_error("%s: scaling_cols=%d must be 2 or 3", who, a->scaling_cols); return 1; }
    const uint64_t rows = (uint64_t)a->P * (uint64_t)(a->N > 2 ? a->N : 2);
    if (rows >= (1ull << 31)) { gsr_set_error("%s: P + clones + N * splits can reach %llu rows, which exceed 2^31", who, (unsigned long long)rows); return 1; }
    if (!(a->child_div > 0.0f)) { gsr_set_error("%s: child_div must be positive", who); return 1; }
    if (a->P && (!a->accum || !a->denom || !a->scaling || !a->opacity)) { gsr_set_error("%s: accum / denom / scaling / opacity: null pointer", who); return 1; }
    if ((a->accum_abs == nullptr) != (a->denom_abs == nullptr)) { gsr_set_error("%s: accum_abs and denom_abs go together", who); return 1; }
    if (a->P && a->accum_abs && !a->max_radii2D) { gsr_set_error("%s: the abs rule needs max_radii2D", who); return 1; }
    return 0;
}

extern "C" size_t gsr_densify_plan_scratch_bytes(int32_t P, int32_t N)
{
    if (P < 0 || N < 1 || (uint64_t)P * (uint64_t)(N > 2 ? N : 2) >= (1ull << 31)) return 0;
    return den_carve((uint32_t)P, (uint32_t)N, nullptr).bytes;
}

extern "C" int gsr_densify_plan(const gsr_densify_args* a, void* scratch, size_t scratch_bytes, uint32_t* status_dev, void* stream)
{
    if (den_check(a, "densify_plan")) return 1;
    if (!status_dev) { gsr_set_error("densify_plan: status_dev is NULL"); return 1; }
    const DenScratch d = den_carve((uint32_t)a->P, (uint32_t)a->N, scratch);
    if (gsr_scratch_check("densify_plan", scratch, scratch_bytes, d.bytes, false)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (gsr_memset_async(status_dev, 0, 8 * 4, s) || gsr_memset_async(d.counters, 0, DEN_CNT * 4, s)) { gsr_set_error("densify_plan: counters"); return 1; }
    if (a->P) {
        hipLaunchKernelGGL(k_den_count, dim3(d.nblk), dim3(DEN_BLOCK), 0, s, *a, d.flags, d.sums, d.stride);
        gsr_scan_small(d.sums, d.nblk, DEN_NQ, d.stride, d.counters, status_dev, s);      // flag q's total to counters[q] and status[q]
        hipLaunchKernelGGL(k_den_place, dim3(d.nblk), dim3(DEN_BLOCK), 0, s, (uint32_t)a->P, (uint32_t)a->N, d.flags, d.sums, d.stride, d.counters, d.rank, d.map);
    }
    return gsr_check_launch("densify_plan", s, false);
}

extern "C" int gsr_densify_emit(const gsr_densify_args* a, const void* scratch, size_t scratch_bytes, const uint32_t* counts, int32_t count,
                                const gsr_densify_tensor* t, const gsr_densify_compute* c, void* stream)
{
    if (den_check(a, "densify_emit")) return 1;
    if (!counts) { gsr_set_error("densify_emit: counts is NULL"); return 1; }
    const DenScratch d = den_carve((uint32_t)a->P, (uint32_t)a->N, scratch);
    if (gsr_scratch_check("densify_emit", scratch, scratch_bytes, d.bytes, false)) return 1;
    const uint32_t P = (uint32_t)a->P, N = (uint32_t)a->N;
    const uint32_t C = counts[0], S = counts[1], nO = counts[2], nC = counts[3], nS = counts[4];
    if (C > P || S > P - C || nO > P - S || nC > C || nS > S) { gsr_set_error("densify_emit: counts are not those of a plan over P=%u rows", P); return 1; }
    const uint64_t rows = (uint64_t)nO + nC + (uint64_t)N * nS;              // <= P * max(2, N) < 2^31: inside the map
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    std::vector<gsr_rows_item> items;
    for (int32_t i = 0; t && i < count; i++) items.push_back({t[i].src, t[i].dst, nullptr, t[i].row_bytes, 0, t[i].zero_new != 0});
    const gsr_rows_map m = {d.map, nullptr, (uint32_t)rows, nO, P};                          // no tails: every output row comes through the map
    if (gsr_rows_move("densify_emit", m, count, t ? items.data() : nullptr, true, s)) return 1;
    if (c) {
        const uint32_t n_clone_rows = c->noise_clone ? nC : 0u;
        const uint64_t total = (uint64_t)n_clone_rows + (uint64_t)N * nS;
        if (total) {
            if (!c->xyz || !c->rotation || !c->xyz_dst || (nS && (!c->scaling_dst || !c->noise_split))) { gsr_set_error("densify_emit: compute: null pointer"); return 1; }
            hipLaunchKernelGGL(k_den_compute, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, *a, *c, d.map, d.rank, S, nO, nC, nS, n_clone_rows, (uint32_t)total);
        }
    }
    return gsr_check_launch("densify_emit", s, false);
}
