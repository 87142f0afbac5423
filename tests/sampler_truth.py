"""gsr_sample_mask restated on the host (numpy): the 24-bit hashed key of (seed, index) and the selection rule, for an exact, slot-for-slot
comparison with the device (tests/test_gpu_mvloss_edges.py).

Rule.  Among the set entries of the mask take the `num` smallest keys: with T the (num+1)-th smallest key, first every entry whose key is below T
in ascending index, then the entries whose key equals T in ascending index until `num` slots are full (T untied: none of them), -1 in the slots
that stay empty.  With at most `num` set entries all of them are taken, ascending.  gsrast.losses.sample_valid_pixels answers a mask of at
most `num` entries without the kernel: every set entry at its own position, -1 elsewhere."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def key24(p, seed):
    """sm_key24 of csrc/gsr_mvloss.hip on uint32 indices p; seed is the 64-bit seed (s0 = low word, s1 = high word)"""
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    x = (np.asarray(p, np.uint64) * np.uint64(0x9E3779B1) + s0) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13); x = (x + s1) & M32; x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(8)).astype(np.uint32)


def threshold(mask, num, seed):
    """-> (T, number of keys below T, number equal to T) or None when every set entry is taken"""
    idx = np.nonzero(np.asarray(mask).reshape(-1))[0]
    if idx.size <= num:
        return None
    k = key24(idx, seed)
    T = np.partition(k, num)[num]
    return int(T), int((k < T).sum()), int((k == T).sum())


def select(mask, num, seed):
    """-> int32 [min(n, num)]: what sample_valid_pixels(mask, num, seed=seed) returns"""
    m = np.asarray(mask).reshape(-1).astype(bool)
    n = m.size
    if n <= num:
        return np.where(m, np.arange(n), -1).astype(np.int32)
    idx = np.nonzero(m)[0]
    out = np.full(num, -1, np.int32)
    if idx.size <= num:
        out[:idx.size] = idx
        return out
    k = key24(idx, seed)
    T = np.partition(k, num)[num]
    out[:] = np.concatenate([idx[k < T], idx[k == T]])[:num]
    return out


def tie_mask():
    """the 20 011-entry mask (not a multiple of 256, four full blocks of 4096 and a partial one) of the tied-threshold cases"""
    return np.random.default_rng(77).random(20011) < 0.6


TIE_NUM = 3000
TIE_SEEDS = (866, 918, 16045690981097406655)      # find_tied_seeds(2), and the first tied seed of the form 0xDEADBEEF << 32 | k (k = 191: high word set)


def fills_from_ties(mask, num, seed):
    """the threshold key is shared and at least one slot is filled from the ties: k_sm_write's second branch writes for certain"""
    t = threshold(mask, num, seed)
    return t is not None and t[2] >= 2 and num - t[1] >= 1


def find_tied_seeds(count=2, start=0, limit=200000):
    """host search that produced TIE_SEEDS: the first `count` seeds from `start` whose threshold is tied on tie_mask() with TIE_NUM slots"""
    m, out = tie_mask(), []
    for seed in range(start, limit):
        if fills_from_ties(m, TIE_NUM, seed):
            out.append(seed)
            if len(out) == count:
                break
    return out
