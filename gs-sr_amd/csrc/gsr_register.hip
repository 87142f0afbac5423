// gsr_register.hip -- a reconstruction registered to its ground-truth scan on the device: the similarity fit of corresponding points (Horn's
// closed form), point-to-point ICP around the exact nearest-neighbour search of gsr_chamfer.hip, and the crop to a scene's polygon volume
// (include/gsrast.h, "registration").  The reference tree ships no evaluation; the Tanks-and-Temples scripts this stands in for are
// host code over Open3D.
//
//   transform   x' = ((m00 x + m01 y) + m02 z) + m03 in double on the widened float32 input, rounded to float32 once; the matrix travels as a kernel
//               argument (public entry point) or is read from the record on the device (ICP).
//   sums        over the pairs (source[i], target[index[i]]), index[i] >= 0, two passes: n, sum p, sum q, the means by one division each; then with
//               those means H[a][b] = sum (p - pm)_a (q - qm)_b, sum |p - pm|^2, sum |q - qm|^2.  Thread t of block b adds its elements
//               (b * 256 + t) + i * blocks * 256 in ascending i, the block's sum is the wave butterfly (gsr_reduce.h) then (w0 + w1) + (w2 + w3), and one
//               block adds the per-block partials the same way: k_st_partial / k_st_finish of gsr_chamfer.hip over 7 + 11 quantities.  No atomics on
//               floats: two runs give the same bits.
//   solve       one lane: Horn's symmetric 4x4 matrix of H, cyclic Jacobi in the pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) until every off-diagonal
//               element is exactly 0 or GSR_REG_SWEEPS sweeps have passed, the eigenvector of the largest eigenvalue as a unit quaternion, R from it
//               (always a proper rotation), Umeyama's scale, t = qm - s R pm.  Every formula is written out in the header.
//   icp         the whole loop enqueued at once: per iteration transform, query, evaluation (2 launches), sums (4), solve (1), and after the last one
//               transform, query and evaluation again.  The evaluation decides the stop and raises a flag in the record; every later launch
//               reads the flag first and returns.  The host reads the record once.
//   crop        the polygon reaches the device as kernel arguments (128 vertices a launch: no host copy to wait for), each block keeps it in LDS,
//               one thread per point, even-odd crossing number in double.
// Built without FMA contraction (PRE_FLAGS).  Every launch is on the caller's stream; nothing synchronises; no kernel waits for another workgroup.
#include "gsr_common.h"
#include "gsr_reduce.h"
#include <algorithm>

#define RG_BLOCK 256
#define RG_BLOCKS 1024u                       // the most partials a pass leaves: the grid of blocks stops growing at RG_BLOCKS * RG_PER_BLOCK elements
#define RG_PER_BLOCK 1024u                    // elements per block while the grid still grows: 4 per thread
#define RG_Q1 6                               // float64 quantities of pass 1 (the count is an integer beside them)
#define RG_Q2 11                              // of pass 2
#define RG_CROP_CHUNK 128                     // polygon vertices per upload launch (2 KiB of kernel arguments)

// the record, 64-bit words (include/gsrast.h GSR_REG_R_*)
#define R_STATUS GSR_REG_R_STATUS
#define R_N GSR_REG_R_N
#define R_SUM_P GSR_REG_R_SUM_P
#define R_SUM_Q GSR_REG_R_SUM_Q
#define R_MEAN_P GSR_REG_R_MEAN_P
#define R_MEAN_Q GSR_REG_R_MEAN_Q
#define R_H GSR_REG_R_H
#define R_SPP GSR_REG_R_SPP
#define R_SQQ GSR_REG_R_SQQ
#define R_M GSR_REG_R_M
#define R_FITNESS GSR_REG_R_FITNESS
#define R_RMSE GSR_REG_R_RMSE
#define R_INLIERS GSR_REG_R_INLIERS
#define R_ITERATIONS GSR_REG_R_ITERATIONS
#define R_CONVERGED GSR_REG_R_CONVERGED
#define R_STOP GSR_REG_R_STOP
#define R_SUM_D2 GSR_REG_R_SUM_D2

struct RgMat { double m[16]; };

static bool rg_count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }
static uint32_t rg_blocks(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + RG_PER_BLOCK - 1) / RG_PER_BLOCK, 1), RG_BLOCKS); }
__device__ __forceinline__ bool rg_skip(const uint32_t* skip) { return skip && *skip; }

// ------------------------------------------------------------------------------------------------ the record and the transform
// every word zero, M = the caller's matrix
__global__ void __launch_bounds__(64) k_rg_init(unsigned long long* __restrict__ rec, RgMat M)
{
    const uint32_t t = threadIdx.x;
    if (t >= GSR_REG_RECORD_WORDS) return;
    rec[t] = (t >= R_M && t < R_M + 16) ? (unsigned long long)__double_as_longlong(M.m[t - R_M]) : 0ull;
}

// M_dev (nullable) wins over M: the ICP's matrix lives in its record
__global__ void __launch_bounds__(RG_BLOCK) k_rg_transform(const float* __restrict__ pts, uint32_t N, RgMat M, const double* __restrict__ M_dev, float* __restrict__ out,
                                                           const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    const uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= N) return;
    double m[12];
#pragma unroll
    for (int j = 0; j < 12; j++) m[j] = M_dev ? M_dev[j] : M.m[j];
    const double x = (double)pts[3 * (size_t)i], y = (double)pts[3 * (size_t)i + 1], z = (double)pts[3 * (size_t)i + 2];
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * (size_t)i + a] = (float)(((m[4 * a] * x + m[4 * a + 1] * y) + m[4 * a + 2] * z) + m[4 * a + 3]);
}

// ------------------------------------------------------------------------------------------------ fixed-order sums
// NQ per-thread values -> partial[q * RG_BLOCKS + block]; count -> cnt[block].  Every thread of the block calls.
template <int NQ>
__device__ __forceinline__ void rg_block_out(double (&v)[NQ], uint32_t count, double* __restrict__ partial, uint32_t* __restrict__ cnt)
{
    __shared__ double red[NQ][4];
    __shared__ uint32_t redc[4];
#pragma unroll
    for (int q = 0; q < NQ; q++) v[q] = wave_sum(v[q]);
    count = wave_sum(count);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int q = 0; q < NQ; q++) red[q][threadIdx.x >> 6] = v[q];
        redc[threadIdx.x >> 6] = count;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)NQ) partial[threadIdx.x * RG_BLOCKS + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
    if (threadIdx.x == 0 && cnt) cnt[blockIdx.x] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
}
// One block: thread t adds partials t, t + 256, ... in order, then as above; tot[q] and *count are valid in thread 0 after the call.
template <int NQ>
__device__ __forceinline__ void rg_block_total(const double* __restrict__ partial, const uint32_t* __restrict__ cnt, uint32_t nb, double (&tot)[NQ], uint32_t* count)
{
    __shared__ double red[NQ][4];
    __shared__ uint32_t redc[4];
    uint32_t c = 0u;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        double s = 0.0;
        for (uint32_t i = threadIdx.x; i < nb; i += RG_BLOCK) s += partial[(uint32_t)q * RG_BLOCKS + i];
        tot[q] = wave_sum(s);
    }
    if (cnt) for (uint32_t i = threadIdx.x; i < nb; i += RG_BLOCK) c += cnt[i];
    c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int q = 0; q < NQ; q++) red[q][threadIdx.x >> 6] = tot[q];
        redc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) tot[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    *count = (redc[0] + redc[1]) + (redc[2] + redc[3]);
}

// the pair of element i: false where it has none (index -1) or where the index is out of range (*err set)
__device__ __forceinline__ bool rg_pair(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ index, uint32_t T, uint32_t i, double (&p)[3],
                                        double (&q)[3], uint32_t* err)
{
    const int32_t j = index[i];
    if (j == -1) return false;
    if (j < -1 || (uint32_t)j >= T) { *err |= GSR_REG_ERR_INDEX; return false; }
#pragma unroll
    for (int a = 0; a < 3; a++) { p[a] = (double)src[3 * (size_t)i + a]; q[a] = (double)tgt[3 * (size_t)j + a]; }
    return true;
}

__global__ void __launch_bounds__(RG_BLOCK) k_rg_sum1(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ index, uint32_t N, uint32_t T,
                                                      double* __restrict__ partial, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ rec, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    double v[RG_Q1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t n = 0u, err = 0u;
    for (uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x; i < N; i += gridDim.x * RG_BLOCK) {
        double p[3], q[3];
        if (!rg_pair(src, tgt, index, T, i, p, q, &err)) continue;
        n++;
#pragma unroll
        for (int a = 0; a < 3; a++) { v[a] += p[a]; v[3 + a] += q[a]; }
    }
    if (err) atomicOr((uint32_t*)(rec + R_STATUS), err);  // an integer flag: the order does not matter
    rg_block_out<RG_Q1>(v, n, partial, cnt);
}
__global__ void __launch_bounds__(RG_BLOCK) k_rg_fin1(const double* __restrict__ partial, const uint32_t* __restrict__ cnt, uint32_t nb, unsigned long long* __restrict__ rec,
                                                      const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    double tot[RG_Q1]; uint32_t n;
    rg_block_total<RG_Q1>(partial, cnt, nb, tot, &n);
    if (threadIdx.x != 0) return;
    double* r = (double*)rec;
    rec[R_N] = (unsigned long long)n;
    for (int a = 0; a < 3; a++) {
        r[R_SUM_P + a] = tot[a]; r[R_SUM_Q + a] = tot[3 + a];
        r[R_MEAN_P + a] = n ? tot[a] / (double)n : 0.0; r[R_MEAN_Q + a] = n ? tot[3 + a] / (double)n : 0.0;
    }
}
__global__ void __launch_bounds__(RG_BLOCK) k_rg_sum2(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ index, uint32_t N, uint32_t T,
                                                      const unsigned long long* __restrict__ rec, double* __restrict__ partial, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    const double* r = (const double*)rec;
    const double pm[3] = { r[R_MEAN_P], r[R_MEAN_P + 1], r[R_MEAN_P + 2] }, qm[3] = { r[R_MEAN_Q], r[R_MEAN_Q + 1], r[R_MEAN_Q + 2] };
    double v[RG_Q2];
#pragma unroll
    for (int q = 0; q < RG_Q2; q++) v[q] = 0.0;
    uint32_t err = 0u;
    for (uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x; i < N; i += gridDim.x * RG_BLOCK) {
        double p[3], q[3];
        if (!rg_pair(src, tgt, index, T, i, p, q, &err)) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) { p[a] -= pm[a]; q[a] -= qm[a]; }
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) v[3 * a + b] += p[a] * q[b];
        v[9] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        v[10] += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    }
    rg_block_out<RG_Q2>(v, 0u, partial, nullptr);
}
__global__ void __launch_bounds__(RG_BLOCK) k_rg_fin2(const double* __restrict__ partial, uint32_t nb, unsigned long long* __restrict__ rec, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    double tot[RG_Q2]; uint32_t n;
    rg_block_total<RG_Q2>(partial, nullptr, nb, tot, &n);
    if (threadIdx.x != 0) return;
    double* r = (double*)rec;
    for (int q = 0; q < 9; q++) r[R_H + q] = tot[q];
    r[R_SPP] = tot[9]; r[R_SQQ] = tot[10];
}

static void rg_sums(const float* src, const float* tgt, const int32_t* index, uint32_t N, uint32_t T, unsigned long long* rec, double* partial, uint32_t* cnt, const uint32_t* skip,
                    hipStream_t s)
{
    const uint32_t nb = rg_blocks(N);
    hipLaunchKernelGGL(k_rg_sum1, dim3(nb), dim3(RG_BLOCK), 0, s, src, tgt, index, N, T, partial, cnt, rec, skip);
    hipLaunchKernelGGL(k_rg_fin1, dim3(1), dim3(RG_BLOCK), 0, s, (const double*)partial, (const uint32_t*)cnt, nb, rec, skip);
    hipLaunchKernelGGL(k_rg_sum2, dim3(nb), dim3(RG_BLOCK), 0, s, src, tgt, index, N, T, (const unsigned long long*)rec, partial, skip);
    hipLaunchKernelGGL(k_rg_fin2, dim3(1), dim3(RG_BLOCK), 0, s, (const double*)partial, nb, rec, skip);
}

// ------------------------------------------------------------------------------------------------ the solve (include/gsrast.h has the formulas)
// One rotation of the cyclic Jacobi method on the symmetric A with the eigenvector columns in V.
__device__ __forceinline__ void rg_rotate(double (&A)[4][4], double (&V)[4][4], int p, int q)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p][p] = A[p][p] - t * apq;
    A[q][q] = A[q][q] + t * apq;
    A[p][q] = 0.0; A[q][p] = 0.0;
    for (int r = 0; r < 4; r++) {
        if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
            A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
        }
        const double vrp = V[r][p], vrq = V[r][q];
        V[r][p] = c * vrp - s * vrq;
        V[r][q] = s * vrp + c * vrq;
    }
}

// icp: a degenerate record also raises the stop flag, a solved one counts an iteration
__global__ void __launch_bounds__(64) k_rg_solve(unsigned long long* __restrict__ rec, int32_t with_scaling, int32_t icp, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    if (threadIdx.x != 0) return;
    double* r = (double*)rec;
    const unsigned long long n = rec[R_N];
    const double spp = r[R_SPP], sqq = r[R_SQQ];
    if (n < 3ull || spp == 0.0 || sqq == 0.0) {
        rec[R_STATUS] |= (unsigned long long)GSR_REG_ERR_DEGENERATE;
        if (icp) rec[R_STOP] = 1ull;
        return;
    }
    double H[3][3];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) H[a][b] = r[R_H + 3 * a + b];
    double A[4][4], V[4][4];
    A[0][0] = (H[0][0] + H[1][1]) + H[2][2];
    A[1][1] = (H[0][0] - H[1][1]) - H[2][2];
    A[2][2] = (H[1][1] - H[0][0]) - H[2][2];
    A[3][3] = (H[2][2] - H[0][0]) - H[1][1];
    A[0][1] = A[1][0] = H[1][2] - H[2][1];
    A[0][2] = A[2][0] = H[2][0] - H[0][2];
    A[0][3] = A[3][0] = H[0][1] - H[1][0];
    A[1][2] = A[2][1] = H[0][1] + H[1][0];
    A[1][3] = A[3][1] = H[2][0] + H[0][2];
    A[2][3] = A[3][2] = H[1][2] + H[2][1];
    for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < GSR_REG_SWEEPS; sweep++) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[0][3] == 0.0 && A[1][2] == 0.0 && A[1][3] == 0.0 && A[2][3] == 0.0) break;
        rg_rotate(A, V, 0, 1); rg_rotate(A, V, 0, 2); rg_rotate(A, V, 0, 3);
        rg_rotate(A, V, 1, 2); rg_rotate(A, V, 1, 3); rg_rotate(A, V, 2, 3);
    }
    int best = 0;
    for (int a = 1; a < 4; a++) if (A[a][a] > A[best][best]) best = a;
    double e[4] = { V[0][best], V[1][best], V[2][best], V[3][best] };
    const double norm = sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);
    for (int a = 0; a < 4; a++) e[a] = e[a] / norm;
    for (int a = 0; a < 4; a++) {
        if (e[a] == 0.0) continue;
        if (e[a] < 0.0) for (int b = 0; b < 4; b++) e[b] = -e[b];
        break;
    }
    const double w = e[0], x = e[1], y = e[2], z = e[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    double R[3][3];
    R[0][0] = ((ww + xx) - yy) - zz; R[0][1] = 2.0 * (xy - wz);       R[0][2] = 2.0 * (xz + wy);
    R[1][0] = 2.0 * (xy + wz);       R[1][1] = ((ww - xx) + yy) - zz; R[1][2] = 2.0 * (yz - wx);
    R[2][0] = 2.0 * (xz - wy);       R[2][1] = 2.0 * (yz + wx);       R[2][2] = ((ww - xx) - yy) + zz;
    double scale = 1.0;
    if (with_scaling) {
        double acc = 0.0;
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) acc += R[a][b] * H[b][a];
        scale = acc / spp;
    }
    for (int a = 0; a < 3; a++) {
        const double rp = (R[a][0] * r[R_MEAN_P] + R[a][1] * r[R_MEAN_P + 1]) + R[a][2] * r[R_MEAN_P + 2];
        for (int b = 0; b < 3; b++) r[R_M + 4 * a + b] = with_scaling ? scale * R[a][b] : R[a][b];
        r[R_M + 4 * a + 3] = r[R_MEAN_Q + a] - (with_scaling ? scale * rp : rp);
    }
    r[R_M + 12] = 0.0; r[R_M + 13] = 0.0; r[R_M + 14] = 0.0; r[R_M + 15] = 1.0;
    if (icp) rec[R_ITERATIONS] += 1ull;
}

// ------------------------------------------------------------------------------------------------ the evaluation of an ICP iteration
__global__ void __launch_bounds__(RG_BLOCK) k_rg_eval(const float* __restrict__ d2, const int32_t* __restrict__ index, uint32_t N, double* __restrict__ partial,
                                                      uint32_t* __restrict__ cnt, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    double v[1] = {0.0};
    uint32_t n = 0u;
    for (uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x; i < N; i += gridDim.x * RG_BLOCK)
        if (index[i] >= 0) { n++; v[0] += (double)d2[i]; }
    rg_block_out<1>(v, n, partial, cnt);
}
// fitness and rmse of iteration k, the stop rule, the flag
__global__ void __launch_bounds__(RG_BLOCK) k_rg_eval_fin(const double* __restrict__ partial, const uint32_t* __restrict__ cnt, uint32_t nb, uint32_t N, int32_t k, int32_t max_iteration,
                                                          double rel_fitness, double rel_rmse, unsigned long long* __restrict__ rec, const uint32_t* __restrict__ skip)
{
    if (rg_skip(skip)) return;
    double tot[1]; uint32_t n;
    rg_block_total<1>(partial, cnt, nb, tot, &n);
    if (threadIdx.x != 0) return;
    double* r = (double*)rec;
    const double fitness = (double)n / (double)N, rmse = n ? sqrt(tot[0] / (double)n) : 0.0;
    const bool converged = k > 0 && fabs(fitness - r[R_FITNESS]) < rel_fitness && fabs(rmse - r[R_RMSE]) < rel_rmse;
    r[R_FITNESS] = fitness; r[R_RMSE] = rmse; r[R_SUM_D2] = tot[0];
    rec[R_INLIERS] = (unsigned long long)n;
    if (converged) rec[R_CONVERGED] = 1ull;
    if (converged || k == max_iteration) rec[R_STOP] = 1ull;
}

// ------------------------------------------------------------------------------------------------ the crop
struct RgPolyChunk { double u[RG_CROP_CHUNK], v[RG_CROP_CHUNK]; };
__global__ void __launch_bounds__(RG_CROP_CHUNK) k_rg_poly_put(RgPolyChunk c, uint32_t first, uint32_t K, double2* __restrict__ poly)
{
    const uint32_t i = first + threadIdx.x;
    if (i < K) poly[i] = make_double2(c.u[threadIdx.x], c.v[threadIdx.x]);
}
__global__ void __launch_bounds__(RG_BLOCK) k_rg_crop(const float* __restrict__ pts, uint32_t N, const double2* __restrict__ poly, uint32_t K, int32_t axis, double axis_min,
                                                      double axis_max, uint8_t* __restrict__ keep)
{
    __shared__ double2 lds[GSR_REG_MAX_POLYGON];
    for (uint32_t i = threadIdx.x; i < K; i += RG_BLOCK) lds[i] = poly[i];
    __syncthreads();
    const uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float p[3] = { pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2] };
    const int iu = axis == 0 ? 1 : 0, iv = axis == 2 ? 1 : 2;
    const double w = (double)p[axis], u = (double)p[iu], v = (double)p[iv];
    bool in = p[0] - p[0] == 0.f && p[1] - p[1] == 0.f && p[2] - p[2] == 0.f && axis_min <= w && w <= axis_max;
    if (in) {
        bool odd = false;
        double2 a = lds[K - 1u];
        for (uint32_t k = 0; k < K; k++) {                // the edge from vertex k - 1 (cyclically) to vertex k
            const double2 b = lds[k];
            if ((a.y > v) != (b.y > v) && u < ((b.x - a.x) * (v - a.y)) / (b.y - a.y) + a.x) odd = !odd;
            a = b;
        }
        in = odd;
    }
    keep[i] = in ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ entry points
static int rg_matrix(const char* who, const double* M, RgMat* out)
{
    if (!M) { gsr_set_error("%s: null transformation", who); return 1; }
    for (int i = 0; i < 16; i++) {
        if (!(M[i] - M[i] == 0.0)) { gsr_set_error("%s: the transformation has a non-finite element", who); return 1; }
        out->m[i] = M[i];
    }
    return 0;
}

extern "C" int gsr_transform_points(const float* points, int64_t n_points, const double* transformation, float* out, void* stream)
{
    const char* who = "transform_points";
    if (!rg_count_ok(n_points)) { gsr_set_error("%s: %lld points out of range [0, 2^31)", who, (long long)n_points); return 1; }
    RgMat M;
    if (rg_matrix(who, transformation, &M)) return 1;
    if (n_points == 0) return 0;
    if (!points || !out) { gsr_set_error("%s: null pointer", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rg_transform, dim3(gsr_div_up((uint32_t)n_points, RG_BLOCK)), dim3(RG_BLOCK), 0, s, points, (uint32_t)n_points, M, (const double*)nullptr, out,
                       (const uint32_t*)nullptr);
    return gsr_check_launch(who, s, false);
}

struct SumScratch { double* partial; uint32_t* cnt; size_t bytes; };
static SumScratch rg_sum_carve(GsrCarve& c)
{
    SumScratch m;
    m.partial = c.take<double>((size_t)RG_Q2 * RG_BLOCKS); m.cnt = c.take<uint32_t>(RG_BLOCKS);
    m.bytes = c.bytes();
    return m;
}
extern "C" size_t gsr_correspondence_sums_scratch_bytes(int64_t n_source)
{
    if (!rg_count_ok(n_source)) return 0;
    GsrCarve c(nullptr);
    return rg_sum_carve(c).bytes;
}
extern "C" int gsr_correspondence_sums(const float* source, int64_t n_source, const float* target, int64_t n_target, const int32_t* index, void* record_dev, void* scratch,
                                       size_t scratch_bytes, void* stream)
{
    const char* who = "correspondence_sums";
    if (!rg_count_ok(n_source) || !rg_count_ok(n_target)) { gsr_set_error("%s: %lld sources / %lld targets out of range [0, 2^31)", who, (long long)n_source, (long long)n_target); return 1; }
    if (!record_dev || (n_source > 0 && (!source || !index)) || (n_target > 0 && !target)) { gsr_set_error("%s: null pointer", who); return 1; }
    GsrCarve c(scratch);
    const SumScratch m = rg_sum_carve(c);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    RgMat I;
    for (int i = 0; i < 16; i++) I.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
    unsigned long long* rec = (unsigned long long*)record_dev;
    hipLaunchKernelGGL(k_rg_init, dim3(1), dim3(64), 0, s, rec, I);
    if (n_source > 0) rg_sums(source, target, index, (uint32_t)n_source, (uint32_t)n_target, rec, m.partial, m.cnt, nullptr, s);
    return gsr_check_launch(who, s, false);
}

extern "C" int gsr_solve_transform(void* record_dev, int32_t with_scaling, void* stream)
{
    const char* who = "solve_transform";
    if (!record_dev) { gsr_set_error("%s: null record", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rg_solve, dim3(1), dim3(64), 0, s, (unsigned long long*)record_dev, with_scaling ? 1 : 0, 0, (const uint32_t*)nullptr);
    return gsr_check_launch(who, s, false);
}

struct IcpScratch { void* grid; float *moved, *d2; int32_t* index; SumScratch sum; size_t bytes; };
static IcpScratch rg_icp_carve(uint64_t N, uint64_t T, const void* base)
{
    IcpScratch m; GsrCarve c(base);
    const size_t n = N > 0 ? N : 1;
    m.grid = c.take<char>(gsr_np_scratch_bytes(T));
    m.moved = c.take<float>(3 * n); m.d2 = c.take<float>(n); m.index = c.take<int32_t>(n);
    m.sum = rg_sum_carve(c);
    m.bytes = c.bytes();
    return m;
}
extern "C" size_t gsr_icp_scratch_bytes(int64_t n_source, int64_t n_target)
{
    if (!rg_count_ok(n_source) || !rg_count_ok(n_target)) return 0;
    return rg_icp_carve((uint64_t)n_source, (uint64_t)n_target, nullptr).bytes;
}
extern "C" int gsr_icp(const float* source, int64_t n_source, const float* target, int64_t n_target, float max_dist, const double* init, int32_t max_iteration,
                       double relative_fitness, double relative_rmse, int32_t with_scaling, void* record_dev, void* scratch, size_t scratch_bytes, void* stream)
{
    const char* who = "icp";
    if (!rg_count_ok(n_source) || !rg_count_ok(n_target) || n_source == 0) {
        gsr_set_error("%s: %lld sources / %lld targets out of range: [1, 2^31) and [0, 2^31)", who, (long long)n_source, (long long)n_target); return 1;
    }
    if (!(max_dist >= 0.f) || !(max_dist - max_dist == 0.f)) { gsr_set_error("%s: max_dist is NaN, negative or infinite", who); return 1; }
    if (!(relative_fitness >= 0.0) || !(relative_rmse >= 0.0) || !(relative_fitness - relative_fitness == 0.0) || !(relative_rmse - relative_rmse == 0.0)) {
        gsr_set_error("%s: a threshold is NaN, negative or infinite", who); return 1;
    }
    if (max_iteration < 0 || max_iteration > GSR_REG_MAX_ITERATION) { gsr_set_error("%s: max_iteration %d outside [0, %d]", who, max_iteration, GSR_REG_MAX_ITERATION); return 1; }
    RgMat M;
    if (rg_matrix(who, init, &M)) return 1;
    if (!record_dev || !source || (n_target > 0 && !target)) { gsr_set_error("%s: null pointer", who); return 1; }
    const IcpScratch m = rg_icp_carve((uint64_t)n_source, (uint64_t)n_target, scratch);
    if (gsr_scratch_check(who, scratch, scratch_bytes, m.bytes)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = (uint32_t)n_source, T = (uint32_t)n_target, nb = rg_blocks(N);
    unsigned long long* rec = (unsigned long long*)record_dev;
    const uint32_t* stop = (const uint32_t*)(rec + R_STOP);
    const double* M_dev = (const double*)(rec + R_M);
    hipLaunchKernelGGL(k_rg_init, dim3(1), dim3(64), 0, s, rec, M);
    if (gsr_np_build(who, target, T, max_dist, m.grid, s)) return 1;          // once
    for (int32_t k = 0; k <= max_iteration; k++) {
        hipLaunchKernelGGL(k_rg_transform, dim3(gsr_div_up(N, RG_BLOCK)), dim3(RG_BLOCK), 0, s, source, N, M, M_dev, m.moved, stop);      // always from the original source
        gsr_np_query(m.moved, N, T, max_dist, m.grid, m.d2, m.index, stop, s);
        hipLaunchKernelGGL(k_rg_eval, dim3(nb), dim3(RG_BLOCK), 0, s, (const float*)m.d2, (const int32_t*)m.index, N, m.sum.partial, m.sum.cnt, stop);
        hipLaunchKernelGGL(k_rg_eval_fin, dim3(1), dim3(RG_BLOCK), 0, s, (const double*)m.sum.partial, (const uint32_t*)m.sum.cnt, nb, N, k, max_iteration, relative_fitness,
                           relative_rmse, rec, stop);
        if (k == max_iteration) break;
        rg_sums(source, target, m.index, N, T, rec, m.sum.partial, m.sum.cnt, stop, s);
        hipLaunchKernelGGL(k_rg_solve, dim3(1), dim3(64), 0, s, rec, with_scaling ? 1 : 0, 1, stop);
    }
    return gsr_check_launch(who, s, false);
}

extern "C" size_t gsr_crop_polygon_scratch_bytes(void) { return gsr_align((size_t)GSR_REG_MAX_POLYGON * sizeof(double2)); }
extern "C" int gsr_crop_polygon_volume(const float* points, int64_t n_points, const double* polygon, int32_t n_polygon, int32_t axis, double axis_min, double axis_max,
                                       uint8_t* keep, void* scratch, size_t scratch_bytes, void* stream)
{
    const char* who = "crop_polygon_volume";
    if (!rg_count_ok(n_points)) { gsr_set_error("%s: %lld points out of range [0, 2^31)", who, (long long)n_points); return 1; }
    if (n_polygon < 3 || n_polygon > GSR_REG_MAX_POLYGON) { gsr_set_error("%s: a polygon of %d vertices, 3 to %d are possible", who, n_polygon, GSR_REG_MAX_POLYGON); return 1; }
    if (axis < 0 || axis > 2) { gsr_set_error("%s: axis %d is not 0, 1 or 2", who, axis); return 1; }
    if (axis_min != axis_min || axis_max != axis_max) { gsr_set_error("%s: axis_min or axis_max is NaN", who); return 1; }
    if (!polygon || (n_points > 0 && (!points || !keep))) { gsr_set_error("%s: null pointer", who); return 1; }
    for (int32_t i = 0; i < 2 * n_polygon; i++) if (!(polygon[i] - polygon[i] == 0.0)) { gsr_set_error("%s: the polygon has a non-finite coordinate", who); return 1; }
    if (gsr_scratch_check(who, scratch, scratch_bytes, gsr_crop_polygon_scratch_bytes())) return 1;
    if (n_points == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t K = (uint32_t)n_polygon;
    double2* poly = (double2*)scratch;
    for (uint32_t first = 0; first < K; first += RG_CROP_CHUNK) {
        RgPolyChunk c;
        for (uint32_t j = 0; j < RG_CROP_CHUNK; j++) {
            const uint32_t i = std::min(first + j, K - 1u);
            c.u[j] = polygon[2 * i]; c.v[j] = polygon[2 * i + 1];
        }
        hipLaunchKernelGGL(k_rg_poly_put, dim3(1), dim3(RG_CROP_CHUNK), 0, s, c, first, K, poly);
    }
    hipLaunchKernelGGL(k_rg_crop, dim3(gsr_div_up((uint32_t)n_points, RG_BLOCK)), dim3(RG_BLOCK), 0, s, points, (uint32_t)n_points, (const double2*)poly, K, axis, axis_min, axis_max,
                       keep);
    return gsr_check_launch(who, s, false);
}
