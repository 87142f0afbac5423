"""Anchor growing + pruning without a device: the torch restatement (tests/ref_anchor_torch.py) against the fixtures the reference's own
ScaffoldGaussian.adjust_anchor produced (tests/golden/make_golden_anchor.py), bit for bit; the header declarations; and the argument errors of
gsrast.anchors, which are raised before any device call."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

import anchor_edge_cases as E
import ref_anchor_torch as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_*.npz")))
SYMBOLS = ["gsr_anchor_level_scratch_bytes", "gsr_anchor_level_find", "gsr_anchor_level_emit", "gsr_rows_compact_scratch_bytes", "gsr_rows_compact_multi"]


def load(path):
    return {k: torch.tensor(v) for k, v in np.load(path).items()}


def test_fixture_set():
    names = {os.path.basename(p)[len("ref_anchor_adjust_"):-4] for p in FIXTURES}
    assert names >= {"default", "skip", "k10", "noprune"}
    for p in FIXTURES:
        assert os.path.getsize(p) < 275 * 1024
    fx = load(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_default.npz"))
    assert int((fx["level_counts"] > 0).sum()) >= 2 and not bool(fx["keep"].all())          # additions on two levels, something pruned
    assert abs(float(fx["voxel_size"]) - 0.01) < 1e-12                                     # not a power of two
    fx = load(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_skip.npz"))
    assert int(fx["level_counts"].sum()) == 0
    fx = load(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_k10.npz"))
    assert int(fx["k"]) == 10 and fx["in_anchor_feat"].shape[1] == 32
    fx = load(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_noprune.npz"))
    assert not bool((fx["in_anchor_demon"] > 80).any()) and bool(fx["keep"].all())


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_restatement_equals_reference_fixture(path):
    fx = load(path)
    out = R.adjust(fx)
    for name, got in out.items():
        want = fx[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert torch.equal(got.to(want.dtype), want), name


def test_skip_rule_hides_real_candidates():
    """The lattice case adds nothing at level 0; its level 1 would add anchors, and only the reference's skip rule keeps it from doing so."""
    fx = load(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_skip.npz"))
    g = torch.nan_to_num(fx["in_offset_gradient_accum"] / fx["in_offset_denom"], nan=0.0).abs().reshape(-1)
    seen = (fx["in_offset_denom"] > 40.0).reshape(-1)
    vs = float(fx["voxel_size"])
    a0, _ = R.grow_level(fx["in_anchor"], fx["in_offset"], fx["scaling_act"], fx["in_anchor_feat"], g, seen, cell=vs * 16, thr_lo=0.0002, rand=fx["rand_0"], rand_thr=0.5)
    a1, _ = R.grow_level(fx["in_anchor"], fx["in_offset"], fx["scaling_act"], fx["in_anchor_feat"], g, seen, cell=vs * 4, thr_lo=0.0004, rand=fx["rand_1"], rand_thr=0.25)
    assert a0.shape[0] == 0 and a1.shape[0] > 0


def test_restatement_order_mask_origin_and_range():
    r = np.random.default_rng(5)
    N, k, F = 300, 3, 5
    anchor = torch.tensor(np.round(r.uniform(-40, 40, (N, 3))).astype(np.float32) * 0.25 + 0.125)
    offset = torch.tensor(r.uniform(-1, 1, (N, k, 3)).astype(np.float32))
    scaling = torch.tensor(r.uniform(0.2, 1.5, (N, 6)).astype(np.float32))
    feat = torch.tensor(r.normal(0, 1, (N, F)).astype(np.float32))
    grads = torch.tensor(r.uniform(0, 1, N * k).astype(np.float32))
    seen = torch.tensor(r.uniform(size=N * k) < 0.8)
    mask = torch.tensor(r.uniform(size=N) < 0.6)
    origin = (0.125, -0.3, 7.0)
    a, f = R.grow_level(anchor, offset, scaling, feat, grads, seen, cell=0.25, thr_lo=0.3, thr_hi=0.9, mask=mask, origin=origin)
    assert a.shape[0] > 10 and f.shape == (a.shape[0], F)
    c = torch.round((a - torch.tensor(origin)) / 0.25).to(torch.int64)
    key = (c[:, 0] + R.BIAS) * (1 << 42) + (c[:, 1] + R.BIAS) * (1 << 21) + c[:, 2] + R.BIAS
    assert bool((key[1:] > key[:-1]).all())                                               # strictly increasing (x, y, z)
    # brute force over the same float32 points
    pts = (anchor[:, None, :] + offset * scaling[:, None, :3]).reshape(-1, 3)
    cand = (grads >= 0.3) & (grads < 0.9) & seen & mask.repeat_interleave(k)
    cells = torch.round((pts - torch.tensor(origin)) / 0.25).to(torch.int64)
    occ = {tuple(v) for v in torch.round((anchor[mask] - torch.tensor(origin)) / 0.25).to(torch.int64).tolist()}
    want = {}
    for j in torch.nonzero(cand).reshape(-1).tolist():
        t = tuple(cells[j].tolist())
        if t not in occ:
            want[t] = torch.maximum(want[t], feat[j // k]) if t in want else feat[j // k]
    assert [tuple(v) for v in c.tolist()] == sorted(want)
    assert torch.equal(f, torch.stack([want[t] for t in sorted(want)]))
    with pytest.raises(RuntimeError, match="packing range"):
        R.grow_level(anchor, offset, scaling, feat, grads, seen, cell=1e-6, thr_lo=0.3)


def test_header_declares_the_anchor_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in decl, f"include/gsrast.h does not declare {s}"
    assert "typedef struct gsr_anchor_level" in src and "typedef struct gsr_rows_tensor" in src
    assert re.search(r"#define GSR_ABI_VERSION 8\b", src)                                  # extended, not changed
    import gsrast
    L = gsrast.lib()
    for s in SYMBOLS:
        assert s in gsrast.EXPORTS and hasattr(L, s)
    mk = open(os.path.join(ROOT, "gs-sr_amd", "csrc", "Makefile")).read()
    assert re.search(r"gsr_anchor\.o: gsr_anchor\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(PRE_FLAGS\)", mk)      # no FMA contraction: cells are integer outputs


def test_library_argument_errors_without_a_device():
    import ctypes as C
    import gsrast
    from gsrast import anchors
    L = gsrast.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)

    def level(**kw):
        base = dict(Na=4, N0=4, k=2, F=3, scaling_stride=6, thr_lo=0.0, thr_hi=1.0, rand_thr=0.5, cell=0.1, origin=(C.c_float * 3)(0, 0, 0),
                    anchor=a, mask=None, offset=a, scaling=a, anchor_feat=a, grads=a, offset_mask=a, rand=None)
        base.update(kw)
        return anchors.Level(**base)

    def find(lv, nbytes=1 << 20):
        return L.gsr_anchor_level_find(C.byref(lv), a, nbytes, a, None)
    assert find(level(N0=5)) != 0 and "bad sizes" in gsrast.last_error()
    assert find(level(k=0)) != 0 and "n_offsets" in gsrast.last_error()
    assert find(level(scaling_stride=2)) != 0 and "scaling_stride" in gsrast.last_error()
    assert find(level(cell=0.0)) != 0 and "cell" in gsrast.last_error()
    assert find(level(grads=None)) != 0 and "grads" in gsrast.last_error()
    assert find(level(), nbytes=16) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_anchor_level_emit(C.byref(level()), a, 1 << 20, 9, a, a, None) != 0 and "count" in gsrast.last_error()
    assert L.gsr_anchor_level_scratch_bytes(1000, 1000, 10) >= 11000 * 28
    assert L.gsr_anchor_level_scratch_bytes(1 << 30, 1 << 30, 10) == 0
    t = (anchors.RowsTensor * 1)(anchors.RowsTensor(a, a + 128, None, 6, 0))
    assert L.gsr_rows_compact_multi(4, a, 1, t, a, 1 << 20, None) != 0 and "row_bytes" in gsrast.last_error()
    t = (anchors.RowsTensor * 1)(anchors.RowsTensor(a, None, None, 8, 0))
    assert L.gsr_rows_compact_multi(4, a, 1, t, a, 1 << 20, None) != 0 and "null pointer" in gsrast.last_error()
    t = (anchors.RowsTensor * 1)(anchors.RowsTensor(a, a + 128, None, 8, 0))
    assert L.gsr_rows_compact_multi(4, a, 1, t, a, 8, None) != 0 and "scratch" in gsrast.last_error()


def test_python_argument_errors_name_the_argument():
    """No CPU fallback: host tensors raise, and so does every malformed argument -- before any device call."""
    from gsrast import anchors
    N, k, F = 6, 2, 3
    z = torch.zeros
    args = lambda: [z(N, 3), z(N, k, 3), z(N, 6), z(N, F), z(N * k), z(N * k, dtype=torch.bool)]
    with pytest.raises(RuntimeError, match="anchor must be a CUDA tensor"):
        anchors.grow_level(*args(), cell=0.1, thr_lo=0.0)
    with pytest.raises(RuntimeError, match="anchor: expected scalar type Float"):
        a = args(); a[0] = a[0].double()
        anchors.grow_level(*a, cell=0.1, thr_lo=0.0)
    with pytest.raises(RuntimeError, match="anchor: expected shape"):
        a = args(); a[0] = z(N, 4)
        anchors.grow_level(*a, cell=0.1, thr_lo=0.0)
    with pytest.raises(RuntimeError, match="anchor must be a CUDA tensor"):
        anchors.anchor_growing(*args(), 0.0002, voxel_size=0.01, n_offsets=k)
    with pytest.raises(RuntimeError, match="keep must be a CUDA tensor"):
        anchors.rows_compact(z(N, dtype=torch.bool), [z(N, 3)])
    with pytest.raises(RuntimeError, match="attribute optimizer is missing"):
        anchors.adjust_anchor_(type("M", (), {n: None for n in list(anchors.PARAM_ATTRS.values()) + ["get_scaling"]})())

    class M:
        pass
    m = M()
    for n in ("_anchor", "_offset", "_anchor_feat", "_opacity", "_scaling", "_rotation", "get_scaling", "opacity_accum", "anchor_demon", "offset_gradient_accum",
              "offset_denom"):
        setattr(m, n, z(N, 3))
    m.optimizer = torch.optim.Adam([torch.nn.Parameter(z(1))])
    m.n_offsets, m.voxel_size, m.update_depth, m.update_init_factor, m.update_hierachy_factor = k, 0.01, 3, 16, 4
    with pytest.raises(RuntimeError, match="model._anchor must be a CUDA tensor"):
        anchors.adjust_anchor_(m)


# ------------------------------------------------------------------------------------------------------------------------ the selection thresholds
# tests/anchor_edge_cases.py: slots named by the comparison they sit on.  Here, without a device: the restatement admits exactly the names the
# literal rule admits, and reversing any one comparison of the rule changes the names -- so the device tests, which demand these names, fail on a
# kernel with that comparison reversed.
BAND = [(0.0002, 0.0009, 0.3)]                                        # the Octree pass A shape: a finite upper threshold
OPEN = [(0.0002, math.inf, 0.3)]                                      # Scaffold-GS and the Octree pass B: no upper threshold
GROWING = [(0.0002 * 2 ** i, math.inf, 0.5 ** (i + 1)) for i in range(3)]   # anchors.anchor_growing: threshold * (4 // 2) ** i, 0.5 ** (i + 1)


def _grow(sc, level, **kw):
    lo, hi, rt = sc["levels"][level]
    return R.grow_level(sc["anchor"], sc["offset"], sc["scaling"], sc["feat"], sc["grads"], sc["seen"], cell=E.CELL, thr_lo=lo, thr_hi=hi,
                        rand=sc["rand"][level], rand_thr=rt, **kw)


@pytest.mark.parametrize("levels", [BAND, OPEN], ids=["band", "open"])
def test_threshold_slots_restatement_equals_the_literal_rule(levels):
    sc = E.scene(levels, seed=11)
    a, f = _grow(sc, 0)
    want = E.expected_names(sc, 0)
    assert E.names_of(sc, 0, a) == want
    q = lambda *n: (0,) + n in want
    assert not q("lo", "below") and q("lo", "on") and q("lo", "above")                       # >=
    assert not q("rand", "below") and not q("rand", "on") and q("rand", "above")             # strict >
    assert not q("nan", "grad") and not q("-inf", "grad") and q("control", "in") and not q("control", "out")
    if levels is BAND:
        assert q("hi", "below") and not q("hi", "on") and not q("hi", "above") and not q("+inf", "grad")      # strict <
    else:
        assert q("+inf", "grad")                                                             # scaffold_gaussian.py:561: grads >= threshold, nothing else
    # every named value sits where its name says, bit for bit
    g, r = sc["grads"].numpy(), sc["rand"][0].numpy()
    lo, hi, rt = (np.float32(v) for v in levels[0])
    for (l, what, side), (_, j) in sc["names"].items():
        v, t = {"lo": (g[j], lo), "hi": (g[j], hi), "rand": (r[j], rt)}.get(what, (None, None))
        if v is not None:
            assert {"below": np.nextafter(t, np.float32(-np.inf)), "on": t, "above": np.nextafter(t, np.float32(np.inf))}[side] == v, (what, side)


def test_infinite_gradient_against_a_literal_mask():
    """+inf with no upper threshold is a candidate (the reference: candidate_mask = grads >= cur_threshold)."""
    sc = E.scene(OPEN, seed=12)
    a, _ = _grow(sc, 0)
    literal = (sc["grads"] >= torch.tensor(0.0002, dtype=torch.float32)) & (sc["rand"][0] > torch.tensor(0.3, dtype=torch.float32))
    named = {j: name for name, (_, j) in sc["names"].items()}
    want = sorted(named[j] for j in torch.nonzero(literal).reshape(-1).tolist() if j in named)
    assert (0, "+inf", "grad") in want and E.names_of(sc, 0, a) == want


@pytest.mark.parametrize("flip", E.FLIPS)
def test_every_admission_comparison_is_observable(flip):
    changed = []
    for tag, levels in (("band", BAND), ("open", OPEN), ("growing", GROWING)):
        sc = E.scene(levels, seed=13)
        for l in range(len(levels)):
            base, other = E.expected_names(sc, l), E.expected_names(sc, l, flip)
            if base != other:
                changed.append((tag, l, sorted(set(base) ^ set(other))))
    print(flip, changed)
    assert changed, flip
    if flip in ("lo", "rand"):
        assert {c[:2] for c in changed} >= {("growing", 0), ("growing", 1), ("growing", 2)}   # at every level's own threshold


def test_anchor_growing_thresholds_per_level():
    sc = E.scene(GROWING, seed=14)
    d, counts = R.anchor_growing(sc["anchor"], sc["offset"], sc["scaling"], sc["feat"], sc["grads"], sc["seen"], 0.0002, voxel_size=E.CELL / 16,
                                 n_offsets=E.K, rand=sc["rand"])
    p = 0
    for l, c in enumerate(counts):
        assert c > 0 and E.names_of(sc, l, d["anchor"][p:p + c]) == E.expected_names(sc, l), l
        p += c


@pytest.mark.parametrize("case", list(E.WEED_CASES))
@pytest.mark.parametrize("mode", ["floor", "round", "ceil"])
def test_weed_out_threshold_cases(case, mode):
    import ref_anchor_octree_torch as RO
    C, t_count, thr = E.WEED_CASES[case]
    pos, lv, cams, visible, il = E.weed_case(C, t_count, seed=C, mode=mode)
    pred = RO.pred_levels(pos, cams, E.WEED["sd"], E.WEED["fork"], torch.float64)
    shift = 0.5 if mode == "round" else 0.0
    assert float((pred - shift - torch.round(pred - shift)).abs().min()) >= 0.2              # the margin of the existing weed-out tests
    count, keep = RO.weed_out(pos, lv, cams, E.WEED["sd"], E.WEED["fork"], E.WEED["levels"], mode, thr)
    assert torch.equal(count, visible)
    want = E.weed_keep(visible.numpy(), C, thr)
    assert np.array_equal(keep.numpy(), want)
    assert np.array_equal(want, visible.numpy() > t_count)                                   # strict: t * C itself is dropped
    assert np.float32(t_count) / np.float32(C) == np.float32(thr)                            # the middle count sits ON the threshold
    assert not np.array_equal(E.weed_keep(visible.numpy(), C, thr, flip=True), want)         # `>=` would keep it
    if C > 256:
        assert (il[256:] >= 1).any() and (il[:256] >= 1).any()                               # the count is carried across the chunks
