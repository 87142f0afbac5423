// gsr_scan.h -- wave and block prefix sums shared by the integer units: binning (k_scan_small, k_scan_rows), the compaction of
// gsr_compact.h (anchors, rows and through them mesh filter and first anchors), densify, the first anchors' select, and the unit / workgroup
// scans of the two mesh extractions.  The blend forward's prologue keeps its own 256-thread forms in gsr_tile_sort.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// inclusive scan across a 64-lane wave
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if ((int)lane_id() >= d) v += t;
    }
    return v;
}

// block-wide inclusive scan for up to 1024 threads; returns inclusive value, *total = block sum
__device__ __forceinline__ uint32_t block_incl_scan(uint32_t v, uint32_t* lds /*>=17 words*/, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    uint32_t s = wave_incl_scan(v);
    if (lane == 63) lds[wave] = s;
    __syncthreads();
    if (wave == 0) {
        uint32_t w = (lane < nw) ? lds[lane] : 0;
        uint32_t ws = wave_incl_scan(w);
        if (lane < nw) lds[lane] = ws - w;        // exclusive prefix per wave
        if (lane == nw - 1) lds[16] = ws;
    }
    __syncthreads();
    s += lds[wave];
    *total = lds[16];
    __syncthreads();
    return s;
}

// the same, exclusive
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* lds /*>=17 words*/, uint32_t* total)
{
    return block_incl_scan(v, lds, total) - v;
}

// In-place exclusive scan of K arrays d[k][0, n) by ONE workgroup of W threads, W entries of each at a time (their loads in flight together)
// with 64-bit carries between the chunks; the sums are ADDED to total[k].  An entry wraps modulo 2^32 only where its total does not fit either.  The
// stores are not published to the other threads on return.
template <int W, int K>
__device__ __forceinline__ void block_scan_arrays(uint32_t* const (&d)[K], uint32_t n, uint32_t* lds /*>=17 words*/, unsigned long long (&total)[K])
{
    for (uint32_t i0 = 0; i0 < n; i0 += W) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t c[K];
#pragma unroll
        for (int k = 0; k < K; k++) c[k] = i < n ? d[k][i] : 0u;
#pragma unroll
        for (int k = 0; k < K; k++) {
            uint32_t tot;
            const uint32_t ex = block_excl_scan(c[k], lds, &tot);
            if (i < n) d[k][i] = (uint32_t)(total[k] + ex);
            total[k] += tot;
        }
    }
}
