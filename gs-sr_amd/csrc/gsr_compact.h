// gsr_compact.h -- count / scan / place stream compaction, once: the level entries, run heads and weed-out survivors of gsr_anchor.hip and the
// keep scan of gsr_rows.hip (and through it the mesh filter and the first anchors).  Element i < n is kept iff op.keep(i); the kept elements
// are numbered in ascending i and op.place(i, pos) stores the one with pos kept elements in front of it (pos <= i).  An operation is passed by value
// and lives in the thread's registers: keep() may leave in it what place() needs, and may read a device-side count itself.  Three launches:
// per-workgroup counts, gsr_scan_small over them (the total goes to *total_dev), placement.  No workgroup waits for another.
#pragma once
#include "gsr_common.h"
#include "gsr_scan.h"

template <typename Op>
__global__ void __launch_bounds__(GSR_COMPACT_BLOCK) k_compact_count(Op op, uint32_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t lds[17];
    const uint32_t i = blockIdx.x * GSR_COMPACT_BLOCK + threadIdx.x;
    uint32_t tot;
    block_excl_scan((i < n && op.keep(i)) ? 1u : 0u, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

template <typename Op>
__global__ void __launch_bounds__(GSR_COMPACT_BLOCK) k_compact_place(Op op, uint32_t n, const uint32_t* __restrict__ sums)
{
    __shared__ uint32_t lds[17];
    const uint32_t i = blockIdx.x * GSR_COMPACT_BLOCK + threadIdx.x;
    const bool f = i < n && op.keep(i);
    uint32_t tot;
    const uint32_t pos = sums[blockIdx.x] + block_excl_scan(f ? 1u : 0u, lds, &tot);
    if (f) op.place(i, pos);
}

// n: the most elements there can be (it sizes the grid); sums: gsr_compact_sums_words(n) words
template <typename Op>
static void gsr_compact(const Op& op, uint32_t n, uint32_t* sums, uint32_t* total_dev, hipStream_t s)
{
    const uint32_t nblk = gsr_div_up(n > 0 ? n : 1u, GSR_COMPACT_BLOCK);
    hipLaunchKernelGGL(k_compact_count<Op>, dim3(nblk), dim3(GSR_COMPACT_BLOCK), 0, s, op, n, sums);
    gsr_scan_small(sums, nblk, 1, 0, total_dev, nullptr, s);
    hipLaunchKernelGGL(k_compact_place<Op>, dim3(nblk), dim3(GSR_COMPACT_BLOCK), 0, s, op, n, sums);
}
