"""GPU: the device-wide radix sort (gsr_radix_sort_pairs / GsrSort, csrc/gsr_binning.hip, gsr_sort.h) held bit for bit to numpy's stable sorts on both
sides of every element count at which its code changes path -- through public calls whose OUTPUT shows the order, so a misplaced element, a lost one
or an unstable pass fails a test (tests/test_sort_cases_cpu.py proves that of the checkers on the CPU).  Sizes come from sort_cases.limits(), which
reads the sources; every case first asserts, through sort_cases.path / passes / forward_sorts, that it does take the path it is here for.

Which case covers which path flag (sizes for the current sources):
  one block                              A  voxelize_sample N = 1, 1023, 1024; F P = 1, 63 (test_gpu_stress.py)
  more than one block in one group       A  N = 1025, 16384;  E  select_views, > 2 blocks (test_gpu_view_selection.py)
  more than one group                    A, B  N = 16385, 262144;  C  vertex_adjacency, 18000 pairs
  more than one row chunk                A, B  N = 262145, 1572864;  D  anchor_growing capacity 1572857
  digit-major, 1024-key blocks           A, B  N = 1572865;  D  capacity 1572868;  F  test_sort_block_and_group_boundaries[1572865] (the depth sort; test_gpu_stress.py)
  4096-key blocks                        F  test_gpu_stress.py::test_tile_sort_with_4096_key_blocks[big_blocks]
  digit-major, 4096-key blocks           F  test_gpu_stress.py::test_tile_sort_with_4096_key_blocks[big_blocks_digit_major]
  n_dev below the capacity               D  (entries of a level);  E  (entries below the observations)
  even number of passes                  A, B, D  (4 per word);  C  V = 65535 (16 bits: 8, 8);  E  C = 257 (9 bits: 5, 4);  F  > 256 tiles (9 bits)
  odd number of passes                   C  V = 65536, 65537 (17 bits: 6, 6, 5);  E  C = 256 (8 bits);  F  one tile (1 bit)
  identity_vals false                    C  (the second sort carries the first one's order);  A, B, D  every word after the first

A and B sort three- and two-word keys with k_sort_word between the words: 12 and 8 passes of 8-bit digits per call."""
import numpy as np
import pytest
import torch

import smooth_truth
import sort_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = sc.limits()
BLOCK, GROUP, CHUNK, SWITCH = L["block"], L["group"], L["row_chunk"], L["digit_major"]


def _flags(n):
    p = sc.path(n)
    return {"one_block": p.blocks == 1, "blocks_in_a_group": p.blocks > 1 and p.groups == 1, "groups": p.groups > 1 and p.row_chunks == 1,
            "row_chunks": p.row_chunks > 1, "digit_major": p.digit_major}


def _takes(n, flag):
    f = _flags(n)
    assert f[flag] and sum(f.values()) == 1, (n, flag, f)


# the side of every limit a count is on, by name: (count, the one path flag it must show)
SIDES = [(1, "one_block"), (BLOCK - 1, "one_block"), (sc.around(BLOCK)[0], "one_block"), (sc.around(BLOCK)[1], "blocks_in_a_group"),
         (sc.around(GROUP)[0], "blocks_in_a_group"), (sc.around(GROUP)[1], "groups"), (sc.around(CHUNK)[0], "groups"), (sc.around(CHUNK)[1], "row_chunks"),
         (sc.around(SWITCH)[0], "row_chunks"), (sc.around(SWITCH)[1], "digit_major")]
PATTERNS = ["ascending", "descending", "all_equal", "two_values"]


def _pattern_rows(pattern, n, row, flip):
    if pattern == "ascending":
        return sc.ascending(n, words=3)
    if pattern == "descending":
        return sc.descending(n, words=3)
    if pattern == "all_equal":
        return sc.all_equal(n, row)
    return sc.two_values(n, n, row, flip)


# ---------------------------------------------------------------------------------------------------------------- A: three words, the order is the output
def _voxelize(keys, dtype):
    from gsrast import init
    data = keys.astype(dtype)
    assert np.array_equal(data.astype(np.int64), keys), "the keys are exact in this precision"
    got = init.voxelize_sample(data, 1.0, DEV)
    assert got.dtype == torch.float32
    sc.check_unique_rows(got.cpu().numpy(), keys)


@pytest.mark.parametrize("n,flag", SIDES, ids=[f"{n}-{f}" for n, f in SIDES])
def test_voxelize_sample_float64_keys_over_the_whole_int32_range(n, flag):
    """np.unique(keys, axis=0).astype(float32), row for row: keys of both signs, every byte of the three words random, every key about three times."""
    _takes(n, flag)
    keys = sc.pool(n, seed=n % 1009, words=3)
    assert n < 8 or ((keys < -(1 << 30)).any() and (keys > (1 << 30)).any())
    _voxelize(keys, np.float64)


F32_SIDES = [s for s in SIDES if s[0] in sc.around(GROUP) + sc.around(SWITCH)]


@pytest.mark.parametrize("n,flag", F32_SIDES, ids=[f"{n}-{f}" for n, f in F32_SIDES])
def test_voxelize_sample_float32_mode(n, flag):
    _takes(n, flag)
    _voxelize(sc.pool(n, seed=7 + n % 1009, words=3, lo=-(1 << 24) + 1, hi=1 << 24), np.float32)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_voxelize_sample_ordered_and_degenerate_keys(pattern):
    """Already sorted, reversed, one key, and two keys whose biased first word differs in its top bit only (every pass but the last sees one digit)."""
    n = sc.around(GROUP)[1]
    _takes(n, "groups")
    _voxelize(_pattern_rows(pattern, n, (-5, 3, -(1 << 31) + 1), 1 << 31), np.float64)


# ---------------------------------------------------------------------------------------------------------------- B: two words, stability is the output
def _downsample(cells, seed):
    """cells int64 [n,3] in [-2^20, 2^20): points at the cells' centres (exact in float32), one row in a hundred non-finite."""
    from gsrast import chamfer
    r = np.random.default_rng(seed)
    pts = (cells.astype(np.float64) + 0.5).astype(np.float32)
    assert np.array_equal(np.floor(pts.astype(np.float64)).astype(np.int64), cells)
    n = len(pts)
    bad = r.choice(n, n // 100, replace=False)
    pts[bad, r.integers(0, 3, len(bad))] = np.asarray([np.nan, np.inf, -np.inf], np.float32)[r.integers(0, 3, len(bad))]
    keys, valid = sc.voxel_keys(pts, 1.0)
    assert int((~valid).sum()) == n // 100
    kept, index = chamfer.voxel_downsample(torch.from_numpy(pts).to(DEV), 1.0)
    assert index.dtype == torch.int32 and kept.dtype == torch.float32
    index = index.cpu().numpy()
    sc.check_first_of_run(index, keys, valid)
    assert np.array_equal(kept.cpu().numpy(), pts[index])
    return index


B_SIDES = [s for s in SIDES if s[0] in sc.around(GROUP) + sc.around(CHUNK) + sc.around(SWITCH)]


@pytest.mark.parametrize("n,flag", B_SIDES, ids=[f"{n}-{f}" for n, f in B_SIDES])
def test_voxel_downsample_keeps_the_lowest_index_of_every_cell(n, flag):
    """A misplaced element makes a false run head, an unstable pass returns a head that is not the cell's lowest index; the non-finite rows carry the
    largest key and must not come out."""
    _takes(n, flag)
    index = _downsample(sc.pool(n, seed=3 + n % 1009, words=3, lo=-(1 << 19), hi=1 << 19), n)
    assert n // 4 < len(index) <= n // 3


@pytest.mark.parametrize("pattern", ["all_equal", "two_values"])
def test_voxel_downsample_one_cell_and_two_cells(pattern):
    """two_values: the z cell is the key's most significant axis, -5 and -5 + 2^20 differ in the top bit of its biased 21 bits only."""
    n = sc.around(GROUP)[1]
    _takes(n, "groups")
    rows = _pattern_rows(pattern, n, (-5, 3, 2), 1 << 20)[:, ::-1]
    index = _downsample(np.ascontiguousarray(rows), n)
    assert len(index) == (1 if pattern == "all_equal" else 2)


# ---------------------------------------------------------------------------------------------------------------- C: pass parity, a sort that carries values
@pytest.mark.parametrize("V", [65535, 65536, 65537])
def test_vertex_adjacency_around_16_bit_vertex_counts(V):
    """Two sorts of sm_bits(V) bits over the 6 T directed pairs, the second with the first one's order as its values (identity_vals = false); the
    result is found with GsrSort::advance twice.  V = 65535: 16 bits, two passes; 65536 and 65537: 17 bits, three balanced passes (6, 6, 5)."""
    import gsrast
    from gsrast.tsdf import TriangleMesh
    T = 3000
    bits = V.bit_length()                                                        # sm_bits: the smallest b with 2^b > V
    assert sc.passes(bits) == ([8, 8] if V == 65535 else [6, 6, 5]) and sc.result_swapped(bits) == (V != 65535)
    _takes(6 * T, "groups")
    r = np.random.default_rng(V)
    t = r.integers(0, V, (T, 3)).astype(np.int32)
    t[0] = (0, V - 1, V - 2)
    t[7] = t[1500]                                                               # a repeated triangle
    t[11, 2] = t[11, 0]                                                          # two equal indices: no self-loop, its two vertices still connected
    assert len(np.unique(t[:, 0] >> 8)) > 200 and t.max() == V - 1
    v = torch.from_numpy(r.normal(0, 1, (V, 3)).astype(np.float32)).to(DEV)
    start, nb = gsrast.vertex_adjacency(TriangleMesh(v, v.clone(), torch.from_numpy(t).to(DEV)))
    want_start, want_nb = smooth_truth.adjacency(t, V)
    assert start.dtype == nb.dtype == torch.int32
    assert np.array_equal(start.cpu().numpy(), want_start) and np.array_equal(nb.cpu().numpy(), want_nb)


# ---------------------------------------------------------------------------------------------------------------- D: the count on the device, across the switch
@pytest.mark.parametrize("N,k,F,digit_major", [(142987, 10, 5, False), (142988, 10, 5, True)])
def test_anchor_growing_on_both_sides_of_the_digit_major_switch(N, k, F, digit_major):
    """The first level sorts a CAPACITY of N (1 + k) entries -- 1 572 857 and 1 572 868, the two sides of the switch -- while the entries themselves
    (the anchors and the candidates that pass the thresholds) are counted on the device and stay a fraction of it; the later levels, which have
    more anchors, are beyond the switch in both cases."""
    import test_gpu_anchor as harness
    cap = N * (1 + k)
    assert sc.path(cap).digit_major == digit_major and abs(cap - SWITCH) < 2 * (1 + k)
    _takes(cap, "digit_major" if digit_major else "row_chunks")
    s, counts = harness.growing_equals_restatement(N, k, F)
    entries = N + int(((s["grads"] >= np.float32(0.0002)) & s["seen"] & (s["rand"][0] > 0.5)).sum())
    assert GROUP < entries < cap // 2 and counts[0] > 0
