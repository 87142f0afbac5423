"""CPU: tests/sort_cases.py -- the radix sort's limits as read from the sources, the restated path decisions, and the proof that the exact checkers
of the GPU tests report a subtly wrong sort.

The proof needs no wrong library: a numpy model of the sort (stable LSD passes over the digits of passes(32), least significant word first) runs with
ONE defect planted in its last pass, the outputs are derived from the order it leaves the way the kernels derive them (a row of the result per run of
equal keys; the element at the head of every run kept), and each checker must raise on each defect."""
import numpy as np
import pytest

import chamfer_cases
import chamfer_truth
import sort_cases as sc


# ---------------------------------------------------------------------------------------------------------------- constants and model
def test_every_constant_is_found_in_the_sources():
    c = sc.constants()
    assert set(c) == set(sc.PATTERNS)
    for name in ("GSR_SORT_THREADS", "GSR_SORT_ITEMS", "GSR_SORT_GROUP", "GSR_SORT_MAX_GROUPS", "GB", "big_from0", "GSR_TB_TILES_MAX", "GSR_TB_ROWS_MAX", "BIG_ITEMS"):
        assert isinstance(c[name], int) and c[name] > 0, name
    assert len(c["STATIC_RULE"]) == 3 and all(isinstance(v, int) and v > 0 for v in c["STATIC_RULE"])


def test_a_constant_that_is_not_found_raises(monkeypatch):
    monkeypatch.setitem(sc.PATTERNS, "GB", ("gsr_binning.hip", r"constexpr int GB = (\d+) rows;"))
    sc.constants.cache_clear()
    try:
        with pytest.raises(LookupError, match="GB"):
            sc.constants()
    finally:
        monkeypatch.undo()
        sc.constants.cache_clear()
    assert sc.constants()["GB"] > 0


def test_limits_are_the_products_written_out():
    """Meant to fail when someone moves a limit: the sizes of the GPU tests follow limits() by themselves, this is where the move is seen."""
    L = sc.limits()
    assert (L["block"], L["group"], L["row_chunk"], L["digit_major"], L["digit_major_big"]) == (1024, 16384, 262144, 1572864, 6291456)
    assert (L["big_block"], L["big_from0"], L["big_from0_device_count"]) == (4096, 1700000, 2125000)
    assert sc.constants()["STATIC_RULE"] == (155, 176, 192) and sc.constants()["GSR_TB_TILES_MAX"] == 16384
    assert sc.around(L["group"]) == (16384, 16385)


def test_path_changes_exactly_between_the_two_sides_of_every_limit():
    L = sc.limits()
    lo, hi = sc.around(L["block"])
    assert sc.path(1).blocks == sc.path(lo).blocks == 1 and sc.path(hi).blocks == 2 and sc.path(hi).groups == 1
    lo, hi = sc.around(L["group"])
    assert sc.path(lo).groups == 1 and sc.path(hi).groups == 2 and sc.path(hi).row_chunks == 1
    lo, hi = sc.around(L["row_chunk"])
    assert sc.path(lo).row_chunks == 1 and sc.path(hi).row_chunks == 2 and not sc.path(hi).digit_major
    lo, hi = sc.around(L["digit_major"])
    assert sc.path(lo) == (1536, 96, 6, False) and sc.path(hi) == (1537, 97, 0, True)
    assert not sc.path(hi, big_blocks=True).digit_major
    lo, hi = sc.around(L["digit_major_big"])
    assert not sc.path(lo, True).digit_major and sc.path(hi, True).digit_major and sc.path(hi, True).blocks == 1537
    assert not sc.tile_sort_big_blocks(L["big_from0"] - 1) and sc.tile_sort_big_blocks(L["big_from0"])
    assert not sc.tile_sort_big_blocks(L["big_from0_device_count"] - 1, True) and sc.tile_sort_big_blocks(L["big_from0_device_count"], True)


def test_passes_are_balanced_and_their_parity_places_the_result():
    assert sc.passes(30) == [8, 8, 7, 7]
    assert sc.passes(32) == [8, 8, 8, 8] and sc.passes(17) == [6, 6, 5] and sc.passes(16) == [8, 8] and sc.passes(9) == [5, 4] and sc.passes(8) == [8]
    assert sc.passes(1) == [1] and sc.passes(5) == [5]
    for bits in range(1, 33):
        w = sc.passes(bits)
        assert sum(w) == bits and len(w) == (bits + 7) // 8 and max(w) - min(w) <= 1 and w == sorted(w, reverse=True)
        assert sc.result_swapped(bits) == bool(((bits + 7) // 8) & 1)


def test_forward_sorts_restates_the_static_rule_and_the_bucket_sort():
    assert sc.forward_sorts("ewa", 155, 1) == () and sc.forward_sorts("ewa", 156, 1) == ("depth", "tile")
    assert sc.forward_sorts("plane", 176 * 24, 24) == () and sc.forward_sorts("plane", 176 * 24 + 1, 24) == ("depth", "tile")
    assert sc.forward_sorts("surfel", 192 * 400, 400) == () and sc.forward_sorts("surfel", 192 * 400 + 1, 400) == ("depth", "tile")
    assert sc.forward_sorts("ewa", 1, 1, depth_order="global") == ("depth", "tile") and sc.forward_sorts("ewa", 10 ** 6, 1, depth_order="tile") == ()
    assert sc.forward_sorts("ewa", 1000, 16384) == () and sc.forward_sorts("ewa", 1000, 16385) == ("tile",)
    assert sc.forward_sorts("ewa", 1000, 24, bucket=False) == ("tile",)
    assert sc.forward_sorts("ewa", 1000, 24, cap=256 * 16384) == () and sc.forward_sorts("ewa", 1000, 24, cap=256 * 16384 + 1) == ("tile",)
    assert sc.tile_bits(1) == 1 and sc.tile_bits(256) == 8 and sc.tile_bits(257) == 9 and sc.tile_bits(24) == 5


# ---------------------------------------------------------------------------------------------------------------- generators
def test_generators():
    k = sc.pool(3000, 1, words=3)
    assert k.shape == (3000, 3) and k.dtype == np.int64 and k.min() > -(1 << 31) and k.max() < (1 << 31) and (k < 0).any() and (k > 0).any()
    distinct = np.unique(k, axis=0)
    assert 600 < len(distinct) <= 1000, "every key repeats about three times"
    for w in range(3):
        for byte in range(4):
            assert len(np.unique((k[:, w] >> (8 * byte)) & 255)) > 200, "every byte of every word varies"
    assert np.array_equal(sc.pool(3000, 1, words=3), k) and not np.array_equal(sc.pool(3000, 2, words=3), k)
    assert sc.pool(1, 0, words=3).shape == (1, 3) and sc.pool(2, 0).shape == (2, 1)
    small = sc.pool(5000, 3, words=3, lo=-(1 << 19), hi=1 << 19)
    assert small.min() >= -(1 << 19) and small.max() < (1 << 19)
    assert len(np.unique(sc.all_equal(50, (7, -8, 9)), axis=0)) == 1
    t = sc.two_values(999, 4, (-5, 3, 2), 1 << 31)
    u = np.unique(t, axis=0)
    assert u.tolist() == [[-5, 3, 2], [(1 << 31) - 5, 3, 2]] and ((u[0, 0] + (1 << 31)) ^ (u[1, 0] + (1 << 31))) == 1 << 31, "the biased words differ in the top bit only"
    a = sc.ascending(16385, words=3)
    key = (a[:, 0] * 32 + (a[:, 1] + 16)) * 32 + (a[:, 2] + 16)
    assert (np.diff(key) == 1).all() and (a[:, 0] < 0).any() and (a[:, 0] > 0).any() and np.array_equal(sc.descending(16385, 3), a[::-1])
    assert np.array_equal(sc.unique_rows(k), np.unique(k, axis=0)) and np.array_equal(sc.unique_rows(a), a)


# ---------------------------------------------------------------------------------------------------------------- the checkers trip
N = 3 * 1024 + 17              # three full blocks and a partial one
BLOCK_END = 1023               # the last element of the first block


def radix_model(words, defect=None):
    """The order a stable LSD sort leaves: words least significant first, uint32 each, digits of passes(32).  `defect(order, digit, full)` changes the
    order the LAST pass leaves (digit: that pass's digit at every place; full: the whole key at every place, most significant word first)."""
    n = len(words[0])
    order = np.arange(n)
    widths = sc.passes(32)
    for wi, w in enumerate(words):
        shift = 0
        for pi, bits in enumerate(widths):
            d = (w[order] >> shift) & ((1 << bits) - 1)
            by_digit = np.argsort(d, kind="stable")
            order = order[by_digit]
            if defect is not None and wi == len(words) - 1 and pi == len(widths) - 1:
                order = defect(order.copy(), d[by_digit], np.stack([x[order] for x in words[::-1]], axis=1))
            shift += bits
    return order


def _swap(order, i, j):
    order[i], order[j] = order[j], order[i]
    return order


def swap_unequal(order, digit, full):
    """Two neighbouring unequal keys swapped (both in runs of two or more, so that the heads of the runs move)."""
    same = (full[1:] == full[:-1]).all(axis=1)
    i = next(i for i in range(len(order) // 2, len(order) - 2) if not same[i] and same[i - 1] and same[i + 1])
    return _swap(order, i, i + 1)


def swap_equal_digit(order, digit, full):
    """Stability of a pass: two neighbours with the same digit in this pass, whose order the earlier passes decided, swapped."""
    i = next(i for i in range(len(order) // 3, len(order) - 1) if digit[i] == digit[i + 1] and not (full[i] == full[i + 1]).all())
    return _swap(order, i, i + 1)


def swap_equal_keys(order, digit, full):
    """Stability proper: the first two elements of a run of equal keys swapped."""
    same = (full[1:] == full[:-1]).all(axis=1)
    i = next(i for i in range(len(order) // 3, len(order) - 1) if same[i] and (i == 0 or not same[i - 1]))
    return _swap(order, i, i + 1)


def lost_and_doubled(order, digit, full):
    """One element lost and another doubled: a place holds its neighbour run's element a second time."""
    same = (full[1:] == full[:-1]).all(axis=1)
    i = next(i for i in range(len(order) // 2, len(order) - 1) if not same[i] and (i + 2 == len(order) or not same[i + 1]) and not same[i - 1])
    order[i] = order[i + 1]        # the only element of its key is gone, the next key's head stands twice
    return order


def split_run(order, digit, full):
    """A run of equal keys split by a foreign key."""
    same = (full[1:] == full[:-1]).all(axis=1)
    i = next(i for i in range(10, len(order) // 2) if same[i])                   # places i, i + 1 hold equal keys
    j = next(j for j in range(len(order) - 1, i + 2, -1) if not (full[j] == full[i]).all())
    return np.concatenate([order[:i + 1], order[j:j + 1], order[i + 1:j], order[j + 1:]])


def block_end_left_in_place(order, digit, full):
    """The last element of a block left in place: place 1023 still holds element 1023, which went nowhere else."""
    p = int(np.flatnonzero(order == BLOCK_END)[0])
    assert p != BLOCK_END
    return _swap(order, p, BLOCK_END)


def _biased_words(keys):
    """int64 [n, w], word 0 the most significant -> the sort's words, least significant first, sign-biased uint32."""
    return [((keys[:, w] + (1 << 31)) & 0xFFFFFFFF).astype(np.int64) for w in range(keys.shape[1] - 1, -1, -1)]


def rows_from_order(keys, order):
    """What gsr_voxel_unique_* makes of the order: one row per run of equal keys, float32."""
    s = keys[order]
    head = np.ones(len(s), bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    return s[head].astype(np.float32)


def kept_from_order(keys, valid, order):
    """What gsr_voxel_downsample_* makes of the order: the element at the head of every run of equal keys is kept (a key without a cell never), and
    the kept come out in index order."""
    s = np.where(valid, keys, np.iinfo(np.int64).max)[order]
    head = np.ones(len(s), bool)
    head[1:] = s[1:] != s[:-1]
    keep = np.zeros(len(keys), bool)
    keep[order[head & valid[order]]] = True
    return np.flatnonzero(keep).astype(np.int32)


def _rows_case():
    return sc.pool(N, 11, words=3, lo=-(1 << 24) + 1, hi=1 << 24)             # float32 holds every key: no two distinct rows round together


def _kept_case():
    cells = sc.pool(N, 12, words=3, lo=-(1 << 19), hi=1 << 19)
    valid = np.ones(N, bool)
    valid[::97] = False
    b = cells + (1 << 20)
    keys = (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]
    words = [np.where(valid, keys & 0xFFFFFFFF, 0xFFFFFFFF), np.where(valid, keys >> 32, 0xFFFFFFFF)]
    return keys, valid, words


def test_the_model_without_a_defect_passes_both_checkers():
    keys = _rows_case()
    order = radix_model(_biased_words(keys))
    assert np.array_equal(keys[order], keys[np.lexsort(keys.T[::-1])]) and np.array_equal(np.sort(order), np.arange(N))
    sc.check_unique_rows(rows_from_order(keys, order), keys)
    k, valid, words = _kept_case()
    order = radix_model(words)
    assert np.array_equal(order, np.argsort(np.where(valid, k, np.iinfo(np.int64).max), kind="stable"))
    sc.check_first_of_run(kept_from_order(k, valid, order), k, valid)
    with pytest.raises(AssertionError, match="first of run"):                             # a kept element without a cell is reported too
        sc.check_first_of_run(np.sort(np.append(kept_from_order(k, valid, order), 0)), k, valid)


ROW_DEFECTS = [swap_unequal, swap_equal_digit, lost_and_doubled, split_run, block_end_left_in_place]
KEPT_DEFECTS = [swap_unequal, swap_equal_keys, lost_and_doubled, split_run, block_end_left_in_place]


@pytest.mark.parametrize("defect", ROW_DEFECTS, ids=[d.__name__ for d in ROW_DEFECTS])
def test_check_unique_rows_reports(defect):
    """Two rows with the same key swapped leave the same rows behind, so the stability defect of this checker is the one a multi-pass sort can show:
    equal digits in the pass, unequal keys."""
    keys = _rows_case()
    good = radix_model(_biased_words(keys))
    bad = radix_model(_biased_words(keys), defect)
    assert 1 <= int((good != bad).sum()) <= N, defect.__name__
    with pytest.raises(AssertionError, match="unique rows"):
        sc.check_unique_rows(rows_from_order(keys, bad), keys)


@pytest.mark.parametrize("defect", KEPT_DEFECTS, ids=[d.__name__ for d in KEPT_DEFECTS])
def test_check_first_of_run_reports(defect):
    k, valid, words = _kept_case()
    good = radix_model(words)
    bad = radix_model(words, defect)
    assert 1 <= int((good != bad).sum()) <= N, defect.__name__
    with pytest.raises(AssertionError, match="first of run"):
        sc.check_first_of_run(kept_from_order(k, valid, bad), k, valid)


# ---------------------------------------------------------------------------------------------------------------- the vectorised truth
@pytest.mark.parametrize("name", sorted(chamfer_cases.VOXELS))
def test_vectorised_voxel_downsample_equals_the_loop(name):
    pts, cell = chamfer_cases.VOXELS[name]
    want_pts, want_idx = chamfer_truth.voxel_downsample(pts, cell)
    got_pts, got_idx = sc.voxel_downsample(pts, cell)
    assert got_idx.dtype == np.int32 and np.array_equal(got_idx, want_idx) and np.array_equal(got_pts, want_pts, equal_nan=True)


def test_vectorised_voxel_downsample_raises_out_of_range_like_the_loop():
    for bad in (chamfer_cases.VOXEL_OUT_OF_RANGE, chamfer_cases.VOXEL_JUST_OUT_OF_RANGE):
        with pytest.raises(ValueError, match="range"):
            sc.voxel_downsample(*bad)
