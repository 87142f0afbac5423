"""The device-wide radix sort (gsr_radix_sort_pairs, gs-sr_amd/csrc/gsr_binning.hip; GsrSort, gsr_sort.h) as the tests see it: the element counts at
which its code changes path, a restatement of the decisions that choose the path, seeded key generators and exact checkers.  Pure Python and numpy:
importable without a GPU (tests/test_sort_cases_cpu.py holds it; tests/test_gpu_sort_paths.py, test_gpu_stress.py and test_gpu_view_selection.py use it).

Every constant is READ FROM THE SOURCES by a regular expression -- there is no literal to fall back to, a constant that is not found raises -- so a
test sized by limits() follows the sources, and tests/test_sort_cases_cpu.py::test_limits_are_the_products_written_out fails when one of them moves.

  limits()          the named limits as element counts
  around(limit)     (limit, limit + 1): the last count on the near side and the first on the far side
  path(n, big)      (blocks, groups, row_chunks, digit_major) of a sort of n keys: gsr_sort_blocks and the `dm` decision of gsr_radix_sort_pairs
  passes(bits)      the balanced digit widths, least significant first; len() is the pass count, its parity is where the result stands (GsrSort::advance)
  forward_sorts()   which radix sorts a forward of the rasteriser runs: gsr_depth_order_static_rule, the GSR_DEPTH_ORDER switch, gsr_tile_bucket_chunk
"""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gs-sr_amd", "csrc")

# name -> (file, pattern with one group per value); a name with several groups gives a tuple
PATTERNS = {
    "GSR_SORT_THREADS": ("gsr_common.h", r"^#define\s+GSR_SORT_THREADS\s+(\d+)\s*$"),
    "GSR_SORT_ITEMS": ("gsr_common.h", r"^#define\s+GSR_SORT_ITEMS\s+(\d+)\s*$"),
    "GSR_TB_TILES_MAX": ("gsr_common.h", r"^#define\s+GSR_TB_TILES_MAX\s+(\d+)u?\b"),
    "GSR_TB_ROWS_MAX": ("gsr_common.h", r"^#define\s+GSR_TB_ROWS_MAX\s+(\d+)u?\b"),
    "GSR_SORT_GROUP": ("gsr_sort.h", r"^#define\s+GSR_SORT_GROUP\s+(\d+)\s*$"),
    "GSR_SORT_MAX_GROUPS": ("gsr_sort.h", r"^#ifndef\s+GSR_SORT_MAX_GROUPS\s*\n#define\s+GSR_SORT_MAX_GROUPS\s+(\d+)\b"),
    "BIG_ITEMS": ("gsr_sort.h", r"gsr_sort_blocks\(uint32_t n, bool big_blocks\)\s*\{\s*return gsr_div_up\(n, GSR_SORT_THREADS \* \(big_blocks \? (\d+)u : \(uint32_t\)GSR_SORT_ITEMS\)\);"),
    "GB": ("gsr_binning.hip", r"constexpr int GB = DPT == 1 \? (\d+) : \d+;"),
    "DIGIT_MAJOR_RULE": ("gsr_binning.hip", r"const uint32_t dm = \(ngroups (>) GSR_SORT_MAX_GROUPS\) \? nblk : 0u;"),
    "BITS_PER_PASS_MAX": ("gsr_binning.hip", r"if \(bits_per_pass > (\d+)\) bits_per_pass = \1;"),
    "big_from0": ("gsr_binning.hip", r"const uint32_t big_from0 = (\d+)u;"),
    "BIG_FROM_DEVICE_DIV": ("gsr_binning.hip", r"const uint32_t big_from = n_dev \? big_from0 \+ big_from0 / (\d+) : big_from0;"),
    "BIG_RULE": ("gsr_binning.hip", r"gsr_radix_sort_pairs\(k0, v0, k1, v1, R, n_dev, 0, tile_bits\(T\), \d+, false, b\.hist, &in_b, s, R (>=) big_from, true\)"),
    "STATIC_RULE": ("gsr_binning.hip", r"per_tile = variant == GSR_EWA \? (\d+)ll : \(variant == GSR_PLANE \? (\d+)ll : (\d+)ll\);\s*\n\s*return \(long long\)P > per_tile \* \(long long\)T;"),
    "BUCKET_CHUNKS": ("gsr_api.hip", r"for \(uint32_t chunk = (\d+)u; chunk <= (\d+)u; chunk <<= 1\)\s*\n\s*if \(gsr_div_up\(cap > 0u \? cap : 1u, chunk\) <= GSR_TB_ROWS_MAX\) return chunk;"),
    "BUCKET_RULE": ("gsr_api.hip", r"if \(!switches\(\)\.tile_bucket \|\| global_order \|\| T (>) GSR_TB_TILES_MAX\) return 0u;"),
}


@functools.lru_cache(maxsize=None)
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def constants():
    """{name: int | tuple of int | str}: what PATTERNS finds.  LookupError names the constant that is not where it was."""
    out = {}
    for name, (src, pattern) in PATTERNS.items():
        found = re.findall(pattern, _text(src), flags=re.M)
        if len(found) != 1:
            raise LookupError(f"{name}: expected one match in csrc/{src} but found {len(found)}: the source moved, restate it in tests/sort_cases.py")
        groups = found[0] if isinstance(found[0], tuple) else (found[0],)
        vals = tuple(int(g) if g.isdigit() else g for g in groups)
        out[name] = vals[0] if len(vals) == 1 else vals
    return out


def limits():
    """The named limits as element counts; a sort of exactly that many keys is the LAST on the near side (around())."""
    c = constants()
    block = c["GSR_SORT_THREADS"] * c["GSR_SORT_ITEMS"]
    group = c["GSR_SORT_GROUP"] * block
    big_block = c["GSR_SORT_THREADS"] * c["BIG_ITEMS"]
    return {"block": block, "group": group, "row_chunk": c["GB"] * group, "digit_major": c["GSR_SORT_MAX_GROUPS"] * group,
            "big_block": big_block, "digit_major_big": c["GSR_SORT_MAX_GROUPS"] * c["GSR_SORT_GROUP"] * big_block,
            "big_from0": c["big_from0"], "big_from0_device_count": c["big_from0"] + c["big_from0"] // c["BIG_FROM_DEVICE_DIV"]}


def around(limit):
    return (limit, limit + 1)


def _div_up(a, b):
    return (a + b - 1) // b


Path = collections.namedtuple("Path", "blocks groups row_chunks digit_major")


def path(n, big_blocks=False):
    """gsr_sort_blocks(n, big_blocks), its groups, how many times the scatter kernel's row loop fetches GB group rows (none in the digit-major form,
    which reads k_scan_rows' prefix instead) and the `dm` decision."""
    c, L = constants(), limits()
    blocks = _div_up(n, L["big_block"] if big_blocks else L["block"])
    groups = _div_up(blocks, c["GSR_SORT_GROUP"])
    assert c["DIGIT_MAJOR_RULE"] == ">"
    digit_major = groups > c["GSR_SORT_MAX_GROUPS"]
    return Path(blocks, groups, 0 if digit_major else _div_up(groups, c["GB"]), digit_major)


def tile_sort_big_blocks(R, device_count=False):
    """Whether the forward's tile sort of R instances (R: the arena's capacity when the count is on the device) takes 4096-key blocks."""
    assert constants()["BIG_RULE"] == ">="
    return R >= limits()["big_from0_device_count" if device_count else "big_from0"]


def passes(bits, begin_bit=0, bits_per_pass=8):
    """The digit widths of gsr_radix_sort_pairs(begin_bit, begin_bit + bits), least significant first: balanced over the remaining passes."""
    cap = constants()["BITS_PER_PASS_MAX"]
    per = min(bits_per_pass, cap)
    out, shift, end = [], begin_bit, begin_bit + bits
    while shift < end:
        remaining = end - shift
        left = _div_up(remaining, per)
        out.append(_div_up(remaining, left))
        shift += out[-1]
    return out


def result_swapped(bits):
    """GsrSort::advance: an odd number of passes leaves the result in the other pair of buffers."""
    return len(passes(bits)) % 2 == 1


VARIANTS = ("ewa", "plane", "surfel")


def forward_sorts(variant, P, T, bucket=True, depth_order="auto", cap=None):
    """The radix sorts a forward of P gaussians on T tiles runs, a tuple out of ("depth", "tile"): the depth sort of the P gaussians runs in the global
    order (GSR_DEPTH_ORDER=global, or auto and gsr_depth_order_static_rule); the tile sort of the instances is the radix sort unless the one-pass bucket
    sort applies (gsr_tile_bucket_chunk: per-tile order, at most GSR_TB_TILES_MAX tiles, GSR_TILE_BUCKET not 0, an arena of at most GSR_TB_ROWS_MAX
    chunks of the largest size; cap=None: a small arena).  The long-list feedback of gsr_api.hip can only ADD the global order to what this says."""
    c = constants()
    per_tile = dict(zip(VARIANTS, c["STATIC_RULE"]))[variant]
    global_order = depth_order == "global" or (depth_order == "auto" and P > per_tile * T)
    assert c["BUCKET_RULE"] == ">"
    bucket_applies = bucket and not global_order and not T > c["GSR_TB_TILES_MAX"] and _div_up(max(cap or 1, 1), c["BUCKET_CHUNKS"][1]) <= c["GSR_TB_ROWS_MAX"]
    return (("depth",) if global_order else ()) + (() if bucket_applies else ("tile",))


def tile_bits(T):
    b = 1
    while (1 << b) < T:
        b += 1
    return b


# ---------------------------------------------------------------------------------------------------------------- keys, seeded
def pool(n, seed, words=1, lo=-(1 << 31) + 1, hi=1 << 31):
    """int64 [n, words]: n draws with replacement from max(1, n // 3) DISTINCT random rows of integers in [lo, hi) -- every byte of every word varies,
    every key repeats about three times, in random order."""
    r = np.random.default_rng(seed)
    m = max(1, n // 3)
    rows = np.zeros((0, words), np.int64)
    while len(rows) < m:
        rows = np.unique(np.concatenate([rows, r.integers(lo, hi, (m - len(rows) + 8, words), dtype=np.int64)]), axis=0)
    rows = rows[r.permutation(len(rows))[:m]]
    return rows[r.integers(0, m, n)]


def all_equal(n, row):
    return np.tile(np.asarray(row, np.int64).reshape(1, -1), (n, 1))


def two_values(n, seed, row, flip):
    """`row` and `row` with `flip` added to its first (most significant) word, dealt at random: with flip = the key's top bit they differ in that bit
    only, and every pass but the last sees one digit."""
    r = np.random.default_rng(seed)
    a = np.asarray(row, np.int64).reshape(1, -1)
    b = a.copy()
    b[0, 0] += flip
    return np.where(r.integers(0, 2, (n, 1)) == 1, b, a)


def ascending(n, words=1, radix=32):
    """int64 [n, words], strictly ascending rows (word 0 the most significant), centred on zero so that both signs occur; every word varies from
    radix ** (words - 1) rows on."""
    i = np.arange(n, dtype=np.int64)
    top = radix ** (words - 1)
    cols = [i // top - (n // top) // 2] + [(i // radix ** (words - 1 - w)) % radix - radix // 2 for w in range(1, words)]
    return np.stack(cols, axis=1)


def descending(n, words=1, radix=32):
    return np.ascontiguousarray(ascending(n, words, radix)[::-1])


# ---------------------------------------------------------------------------------------------------------------- checkers
def unique_rows(keys):
    """The distinct rows of int keys [n, w] in ascending order, word 0 the most significant: np.lexsort and a comparison of neighbours (what
    np.unique(keys, axis=0) returns, in two thirds of its time at 1.5 M rows)."""
    k = np.asarray(keys)
    s = k[np.lexsort(k.T[::-1])]
    head = np.ones(len(s), bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    return s[head]


def check_unique_rows(got_rows, keys):
    """got_rows: what the device made of the keys -- one row per distinct key, ascending (any dtype that holds the keys as the caller cast them).
    Raises AssertionError that names the first place that differs."""
    got = np.asarray(got_rows)
    want = unique_rows(keys).astype(got.dtype)
    if got.shape != want.shape:
        n = min(len(got), len(want))
        bad = np.flatnonzero((got[:n] != want[:n]).any(axis=1))
        raise AssertionError(f"unique rows: {len(got)} rows but {len(want)} distinct keys; first difference at row {int(bad[0]) if len(bad) else n}")
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"unique rows: {len(bad)} rows differ, the first at row {i}: got {got[i].tolist()} but expected {want[i].tolist()}")


def first_of_run(keys, valid=None):
    """The lowest index of every distinct key among the valid elements, ascending by index: np.unique(return_index=True), whose index is the first
    occurrence (a stable sort)."""
    k = np.asarray(keys)
    at = np.arange(len(k)) if valid is None else np.flatnonzero(valid)
    return np.sort(at[np.unique(k[at], return_index=True)[1]])


CELL_RANGE = 1 << 20          # gsrast.chamfer.voxel_downsample: cell coordinates in [-2^20, 2^20)


def voxel_keys(points, cell):
    """-> (keys int64 [n], valid bool [n]) of gsrast.chamfer.voxel_downsample: the cell floor(float64(p) / float64(cell)) per axis, packed 21 bits an
    axis; a point with a non-finite coordinate has no cell.  ValueError("range") as tests/chamfer_truth.py raises it."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    valid = np.isfinite(p).all(axis=1)
    c = np.floor(np.where(valid[:, None], p, 0).astype(np.float64) / float(cell))
    if ((c < -CELL_RANGE) | (c >= CELL_RANGE)).any():
        raise ValueError("range")
    c = c.astype(np.int64) + CELL_RANGE
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], valid


def voxel_downsample(points, cell):
    """tests/chamfer_truth.voxel_downsample without its loop over the points: (points_kept, kept_index int32)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    keep = first_of_run(*voxel_keys(p, cell))
    return p[keep], keep.astype(np.int32)


def check_first_of_run(got_index, keys, valid=None):
    """got_index: the indices the device kept -- for every distinct key the element with the lowest index, ascending; elements outside `valid` never."""
    got, want = np.asarray(got_index).astype(np.int64), first_of_run(keys, valid)
    if got.shape != want.shape or not np.array_equal(got, want):
        extra, missing = np.setdiff1d(got, want), np.setdiff1d(want, got)
        raise AssertionError(f"first of run: kept {len(got)} but {len(want)} distinct keys; kept in error {extra[:4].tolist()} ({len(extra)}), "
                             f"not kept {missing[:4].tolist()} ({len(missing)}){'' if len(extra) or len(missing) else '; the order differs'}")
