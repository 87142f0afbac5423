// gsr_reduce.h -- sums with a pinned order of additions, shared by the loss units and the decode: a wave butterfly, the 256-thread block sums and
// the one-block finish kernel over per-block float2 partials.  Every result is reproducible bit for bit from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// xor butterfly 32, 16, ..., 1 across a 64-lane wave: every lane gets the sum (float, uint32_t)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// sum over a 256-thread block, (w0 + w1) + (w2 + w3), in every thread.  Two calls on the same `red` need a __syncthreads() between them.
__device__ __forceinline__ float block_sum256(float v, float* red /*4*/)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the same for two values behind one barrier
__device__ __forceinline__ float2 block_sum256(float a, float b, float* red /*8*/)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[4 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    return make_float2((red[0] + red[1]) + (red[2] + red[3]), (red[4] + red[5]) + (red[6] + red[7]));
}

// One block of 1024 threads: epi(sum of partial[].x, sum of partial[].y), called by thread 0.  Thread t adds elements t, t + 1024, ... in that order
// (eight loads in flight; an index past n adds +0.0f, which leaves the accumulator as it is), then the butterfly, then the 16 wave values in order.
// One partial per block and this kernel instead of same-address atomics from thousands of blocks, which serialise (measured 0.5 ms).
template <typename Epilogue>
__global__ void __launch_bounds__(1024) k_finish2(const float2* __restrict__ partial, int n, Epilogue epi)
{
    __shared__ float r1[16], r2[16];
    float a = 0.f, b = 0.f;
    for (int i0 = 0; i0 < n; i0 += 8 * 1024) {
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int i = i0 + u * 1024 + threadIdx.x; v[u] = partial[i < n ? i : 0]; if (i >= n) v[u] = make_float2(0.f, 0.f); }
#pragma unroll
        for (int u = 0; u < 8; u++) { a += v[u].x; b += v[u].y; }
    }
    a = wave_sum(a); b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = a; r2[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sa = 0.f, sb = 0.f;
        for (int w = 0; w < 16; w++) { sa += r1[w]; sb += r2[w]; }
        epi(sa, sb);
    }
}

// photometric loss: {mean L1, mean SSIM, (1 - lambda) L1 + lambda (1 - SSIM)}
struct FinishSsim {
    float* loss; float inv_n, lambda;
    __device__ void operator()(float sa, float sb) const
    {
        const float l1 = sa * inv_n, ss = sb * inv_n;
        loss[0] = l1; loss[1] = ss; loss[2] = (1.0f - lambda) * l1 + lambda * (1.0f - ss);
    }
};
// geometric regularisers: {a / n, b / n, ln a / n + ld b / n}
struct FinishGeo {
    float* loss; float inv_n, ln, ld;
    __device__ void operator()(float sa, float sb) const { loss[0] = sa * inv_n; loss[1] = sb * inv_n; loss[2] = ln * loss[0] + ld * loss[1]; }
};
// multi-view losses: {sum, count, sum / count (0 if count == 0)}
struct FinishMean {
    float* stats;
    __device__ void operator()(float sa, float sb) const { stats[0] = sa; stats[1] = sb; stats[2] = sb > 0.f ? sa / sb : 0.f; }
};

template <typename Epilogue>
static void gsr_finish2(const float2* partial, int n, Epilogue epi, hipStream_t s)
{
    hipLaunchKernelGGL(k_finish2<Epilogue>, dim3(1), dim3(1024), 0, s, partial, n, epi);
}
