// gsr_sort.h -- what a caller of the device-wide radix sort needs: the sizes of its scratch, the buffers, which of them hold the result, and the
// step that extends a sort to a key of several 32-bit words.  The sort itself (gsr_radix_sort_pairs and its kernels) is in gsr_binning.hip; the
// rasteriser's forward calls it directly (arena-owned buffers, big_blocks, group0_zeroed), everything else goes through GsrSort.  gsr_common.h
// includes this header, so every unit has it.
//
// A key of several words is sorted least significant word first (stable LSD): the first word with identity values, then per further word
// gsr_sort_next_word -- one kernel writes that word of the element at every place, one stable 32-bit sort moves the order along.  Afterwards
// order[i] = the element at place i and keys[i] = the LAST word sorted of that element; an earlier word is read through the order (gsr_sort_key64).
#pragma once
#include "gsr_common.h"
#include <utility>

// Histogram scratch of the sort: [2 group-histogram buffers of NB * groups words][block histograms NB * nblk], groups = ceil(nblk / 16).
// `group0_zeroed`: the caller's preceding kernel already zeroed the first NB * groups words (gsr_sort_group_words) -- otherwise a memset does.
#define GSR_SORT_GROUP 16
#ifndef GSR_SORT_MAX_GROUPS
#define GSR_SORT_MAX_GROUPS 96        // re-measured with 1024-key blocks (tools/ab_sort_groups.sh): binning 0.0678 / 0.0688 / 0.071 ms at 96 / 48 / 160 groups
#endif
static inline uint32_t gsr_sort_blocks(uint32_t n, bool big_blocks) { return gsr_div_up(n, GSR_SORT_THREADS * (big_blocks ? 16u : (uint32_t)GSR_SORT_ITEMS)); }
static inline uint32_t gsr_sort_group_words(uint32_t n, bool big_blocks, uint32_t NB) { return NB * gsr_div_up(gsr_sort_blocks(n, big_blocks), GSR_SORT_GROUP); }
static inline size_t gsr_sort_hist_words(uint32_t nblk_1024, uint32_t NB) { return (size_t)NB * nblk_1024 + 2 * (size_t)NB * (nblk_1024 / GSR_SORT_GROUP + 1); }
int gsr_radix_sort_pairs(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n, const uint32_t* n_dev,
                         int begin_bit, int end_bit, int bits_per_pass, bool identity_vals, uint32_t* hist,
                         bool* result_in_b, hipStream_t s, bool big_blocks = false, bool group0_zeroed = false);

// The arrays of one sort of up to n pairs.  The caller writes the first word of its keys to ka.
struct GsrSortBuf { uint32_t *ka, *kb, *va, *vb, *hist; };
static inline GsrSortBuf gsr_sort_carve(GsrCarve& c, size_t n)
{
    GsrSortBuf b;
    b.ka = c.take<uint32_t>(n); b.kb = c.take<uint32_t>(n); b.va = c.take<uint32_t>(n); b.vb = c.take<uint32_t>(n);
    b.hist = c.take<uint32_t>(gsr_sort_hist_words(gsr_div_up((uint32_t)n, GSR_SORT_BLOCK), 256));
    return b;
}

// Which pair of a GsrSortBuf is current (keys / order) and which is free to be overwritten.  A sort of `bits` bits takes ceil(bits / 8) passes
// (gsr_radix_sort_pairs with 8 bits per pass) and every pass goes from one pair to the other: where the result stands depends on `bits` alone, so a
// later call on the same scratch block finds it with advance() and launches nothing.
struct GsrSort {
    uint32_t *keys, *order, *free_keys, *free_order, *hist;
    explicit GsrSort(const GsrSortBuf& b) : keys(b.ka), order(b.va), free_keys(b.kb), free_order(b.vb), hist(b.hist) {}
    void advance(int bits) { if (((bits + 7) / 8) & 1) { std::swap(keys, free_keys); std::swap(order, free_order); } }
    // stable sort of the first min(n, *n_dev) pairs (n alone where n_dev is NULL) by the low `bits` bits of keys; identity_vals: order starts as 0, 1, 2, ...
    int sort(uint32_t n, const uint32_t* n_dev, int bits, bool identity_vals, hipStream_t s)
    {
        if (gsr_radix_sort_pairs(keys, order, free_keys, free_order, n, n_dev, 0, bits, 8, identity_vals, hist, nullptr, s)) return 1;
        advance(bits);
        return 0;
    }
};

// keys[i] = op(order[i]) for every place i that holds an element.  An order[i] outside [0, n) is not handed to op: there is none in a place that
// holds an element, and the word written for it does not matter.
#define GSR_SORT_WORD_BLOCK 256
template <class WordOp>
static __global__ void __launch_bounds__(GSR_SORT_WORD_BLOCK) k_sort_word(WordOp op, uint32_t n, const uint32_t* __restrict__ n_dev, const uint32_t* __restrict__ order,
                                                                          uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * GSR_SORT_WORD_BLOCK + threadIdx.x;
    if (i >= n || (n_dev && i >= *n_dev)) return;
    const uint32_t src = order[i];
    keys[i] = src < n ? op(src) : 0xFFFFFFFFu;
}
// The next more significant word of the key: op(e) = that word of element e (a struct with one __device__ call operator, passed by value).
template <class WordOp>
static int gsr_sort_next_word(GsrSort& st, uint32_t n, const uint32_t* n_dev, WordOp op, hipStream_t s)
{
    hipLaunchKernelGGL(k_sort_word<WordOp>, dim3(gsr_div_up(n, GSR_SORT_WORD_BLOCK)), dim3(GSR_SORT_WORD_BLOCK), 0, s, op, n, n_dev, st.order, st.keys);
    return st.sort(n, n_dev, 32, false, s);
}
struct GsrWordFromArray { const uint32_t* word; __device__ uint32_t operator()(uint32_t e) const { return word[e]; } };

// The 64-bit key at place i after a first pass on key_lo and gsr_sort_next_word on the high word: keys[i] holds the high word, the low one is the element's.
__device__ __forceinline__ uint64_t gsr_sort_key64(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order, const uint32_t* __restrict__ key_lo, uint32_t i)
{
    return ((uint64_t)keys[i] << 32) | key_lo[order[i]];
}
