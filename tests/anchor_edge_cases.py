"""Anchor scenes whose every slot is NAMED by the comparison it sits on, for test_anchor_cpu.py, test_gpu_anchor.py and test_gpu_anchor_octree.py.

Candidate admission (csrc/gsr_anchor.hip anc_entry):   thr_lo <= g  and  (g < thr_hi  or  thr_hi == +inf)  and  rand > rand_thr
Weed-out (weed_keep):                                  float32(visible) / float32(C) > visible_threshold

A named slot carries a value one float32 below its threshold, on it, or one above (np.nextafter), and points into a cell that no anchor occupies
and no other slot shares: it appears in the level's output iff it is admitted, and its cell names it.  Every other quantity of the slot passes
its own comparison by a wide margin.  `admitted(...)` is the rule written out literally, with one keyword per comparison that flips it; the CPU
test shows that every flip changes the admitted names, so a kernel with that comparison reversed cannot pass the device tests.

The scene is exact in float32: the cell is a power of two, anchors sit on the lattice, scaling is 1, offsets are whole cells."""
import math

import numpy as np
import torch

N_ANCHORS, K, F = 600, 4, 3
CELL = 0.25
SIDES = ("below", "on", "above")


def f32(x):
    return np.float32(x)


def around(thr):
    """{side: float32} one below, on and one above float32(thr)."""
    t = f32(thr)
    return {"below": np.nextafter(t, f32(-np.inf)), "on": t, "above": np.nextafter(t, f32(np.inf))}


def admitted(g, r, thr_lo, thr_hi, rand_thr, flip=None):
    """The admission rule on float32 scalars; flip reverses one comparison."""
    g, r, lo, hi, rt = f32(g), f32(r), f32(thr_lo), f32(thr_hi), f32(rand_thr)
    with np.errstate(invalid="ignore"):
        low = (g > lo) if flip == "lo" else (g >= lo)
        if flip == "inf_is_a_bound":
            high = g < hi
        else:
            high = ((g <= hi) if flip == "hi" else (g < hi)) or hi == f32(np.inf)
        rnd = (r >= rt) if flip == "rand" else (r > rt)
    return bool(low and high and rnd)


FLIPS = ("lo", "hi", "rand", "inf_is_a_bound")


def level_slots(thr_lo, thr_hi, rand_thr):
    """[(name, grad, rand)] of one level: the three sides of each threshold, the special gradients, and two controls."""
    lo, rt = around(thr_lo), around(rand_thr)
    mid = f32(thr_lo * 1.5) if math.isinf(thr_hi) else f32(0.5 * (thr_lo + thr_hi))
    rows = [(("lo", s), lo[s], f32(0.9)) for s in SIDES]
    rows += [(("rand", s), mid, rt[s]) for s in SIDES]
    if not math.isinf(thr_hi):
        hi = around(thr_hi)
        rows += [(("hi", s), hi[s], f32(0.9)) for s in SIDES]
    rows += [(("nan", "grad"), f32(np.nan), f32(0.9)), (("+inf", "grad"), f32(np.inf), f32(0.9)), (("-inf", "grad"), f32(-np.inf), f32(0.9)),
             (("control", "in"), mid, f32(0.9)), (("control", "out"), f32(thr_lo * 0.5), f32(0.9))]
    return rows


def scene(levels, seed):
    """levels: [(thr_lo, thr_hi, rand_thr)].  -> dict of float32 CPU tensors (anchor, offset, scaling, feat, grads, seen, rand: one per level) and
    names: {(level, quantity, side): (cell y, slot)}.  A level's named slots have rand = 0 at every other level, so that they take part in theirs
    alone; unnamed slots have a hot gradient and a zero offset: they sit in their own anchor's cell and never show."""
    r = np.random.default_rng(seed)
    anchor = np.zeros((N_ANCHORS, 3), np.float32)
    anchor[:, 0] = np.arange(N_ANCHORS, dtype=np.float32) * f32(CELL)
    offset = np.zeros((N_ANCHORS, K, 3), np.float32)
    scaling = np.ones((N_ANCHORS, 6), np.float32)
    feat = r.integers(-8, 9, (N_ANCHORS, F)).astype(np.float32)
    grads = np.full(N_ANCHORS * K, 1.0, np.float32)
    rand = [np.full(N_ANCHORS * K, 0.9, np.float32) for _ in levels]
    rows = [((l,) + name, g, rv) for l, (lo, hi, rt) in enumerate(levels) for name, g, rv in level_slots(lo, hi, rt)]
    slots = r.permutation(N_ANCHORS * K)[:len(rows)]
    names = {}
    for n, ((name, g, rv), j) in enumerate(zip(rows, slots)):
        offset[j // K, j % K, 1] = f32((n + 1) * CELL)                 # the point (a, n + 1, 0) * CELL: no anchor has y != 0, no other slot this y
        grads[j] = g
        for l in range(len(levels)):
            rand[l][j] = rv if l == name[0] else f32(0.0)
        names[name] = (n + 1, int(j))
    t = torch.tensor
    return {"anchor": t(anchor), "offset": t(offset), "scaling": t(scaling), "feat": t(feat), "grads": t(grads), "seen": torch.ones(N_ANCHORS * K, dtype=torch.bool),
            "rand": [t(x) for x in rand], "names": names, "levels": levels}


def expected_names(sc, level, flip=None):
    lo, hi, rt = sc["levels"][level]
    g, r = sc["grads"].numpy(), sc["rand"][level].numpy()
    return sorted(name for name, (_, j) in sc["names"].items() if name[0] == level and admitted(g[j], r[j], lo, hi, rt, flip))


def names_of(sc, level, new_anchor):
    """The names whose cell shows in new_anchor [U,3] (a tensor); every row must be the point of a named slot of `level`."""
    by_y = {y: (name, j) for name, (y, j) in sc["names"].items()}
    out = []
    for x, y, z in new_anchor.cpu().numpy().astype(np.float64) / CELL:
        name, j = by_y[int(y)]
        assert y == int(y) and z == 0.0 and x == j // K and name[0] == level, (x, y, z, name)
        out.append(name)
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------------ weed-out
WEED = dict(levels=6, sd=16.0, fork=2)


def weed_case(C, t_count, seed, mode="round"):
    """C cameras of which exactly t_count - 1, t_count and t_count + 1 admit a position of level 3, 2 and 1 (and all of them level 0): camera c has the
    integer level il_c in dist2level `mode`, its pred = il_c + 0.25 (ceil: il_c - 0.25) for positions within 0.005 of the origin (|d pred| < 0.02:
    at least 0.2 from a boundary of the mode).  -> positions [U,3], levels_of [U], cam_infos [C,4], visible [U] (the counts, known by construction)."""
    assert 2 <= t_count and t_count + 1 <= C
    r = np.random.default_rng(seed)
    il = np.zeros(C, np.int64)
    il[:t_count + 1] = 1; il[:t_count] = 2; il[:t_count - 1] = 3
    il = il[r.permutation(C)]
    v = r.normal(size=(C, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    scale = r.choice([1.0, 2.0], C)
    d = WEED["sd"] / 2.0 ** (il + (-0.25 if mode == "ceil" else 0.25)) / scale
    cams = np.concatenate([v * d[:, None], scale[:, None]], 1).astype(np.float32)
    lv = np.tile(np.arange(4, dtype=np.int32), 5)
    pos = r.uniform(-0.0025, 0.0025, (lv.size, 3)).astype(np.float32)
    visible = np.array([C, t_count + 1, t_count, t_count - 1], np.int32)[lv]
    return torch.tensor(pos), torch.tensor(lv), torch.tensor(cams), torch.tensor(visible), il


def weed_keep(visible, C, thr, flip=False):
    q = visible.astype(np.float32) / np.float32(C)
    return (q >= np.float32(thr)) if flip else (q > np.float32(thr))


WEED_CASES = {"C8_quarter": (8, 2, 0.25), "C10_three_tenths": (10, 3, float(np.float32(0.3))), "C260_two_chunks": (260, 65, 0.25)}
