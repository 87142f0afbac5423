"""Hand-placed scenes for the staging loop of the splat-parallel blend backward, and a model of that loop (TEST INFRASTRUCTURE; numpy only;
tests/test_bwd_rounds_cpu.py, tests/test_gpu_bwd_rounds.py).

k_blend_bwd_sp<V> (gs-sr_amd/csrc/gsr_blend_sp.hip) consumes a tile's list from its deep end in chunks of SP_CH entries and trims a chunk at its
shallow end to the longest suffix whose entries fit every wave's SP_CAP_*-row table; one trip through its `while (hi > 0)` loop is a ROUND here.
rounds() restates that loop for one tile; model() feeds it from the CPU oracle's forward (which quadrants an entry's region meets, each quadrant's
deepest contributor), so that a test can say on the CPU which rounds, cuts and row counts a scene produces -- the kernel has no instrumentation.
The scenes are 16x16 one-tile images (two cases differ) of two kinds of splat placed through fwd_queue_scenes.crafted with a long lens:
  broad   centre (7.5, 7.5), sigma 60 px, opacity 0.0045: contributes to every pixel, reaches all four quadrants
  local   centre at a quadrant's middle +- 0.5 px, sigma 1.2 px, opacity 0.03: reaches that quadrant only (2.4 px) and all four of its 4x4 blocks
Every case size is computed from the constants parsed out of the kernel's source: a changed cap moves the cases with it."""
import os
import re
import sys

import numpy as np

import fwd_queue_scenes as fq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

VARIANTS = ["surfel", "ewa", "plane"]
CSRC = os.path.join(ROOT, "gs-sr_amd", "csrc")
BROAD = (7.5, 7.5, 60.0, 60.0, 0.0045)
OPAQUE = (7.5, 7.5, 60.0, 60.0, 0.8)              # a broad splat that takes T down by a factor of five on every pixel
STRONG = (7.5, 7.5, 60.0, 60.0, 0.85)             # fwd_queue_scenes.median_at's median entry


def constants():
    """-> dict(ch=SP_CH, cap={variant: SP_CAP_*}) as the kernel's source defines them; the Makefile must not override them."""
    with open(os.path.join(CSRC, "gsr_blend_sp.hip")) as fh:
        src = fh.read()
    with open(os.path.join(CSRC, "Makefile")) as fh:
        mk = fh.read()
    assert not re.search(r"-D\s*SP_(CAP_|CH)", mk), "the Makefile overrides a constant the cases are computed from"
    one = lambda name: int(re.search(r"^#define %s (\d+)\b" % name, src, flags=re.M).group(1))
    cap = {}
    for v in VARIANTS:
        name = "SP_CAP_" + v.upper()
        assert re.search(r"^#ifndef %s\n#define %s \d+\n#endif" % (name, name), src, flags=re.M), name
        cap[v] = one(name)
    return dict(ch=one("SP_CH"), cap=cap)


def rounds(hits, wmax, cap, ch):
    """The staging loop of k_blend_bwd_sp for one tile.  hits [n, 4] bool in list order (entry reaches quadrant w), wmax [4] each quadrant's deepest
    contributor (1-based position = number of entries its wave may use).  -> one dict per round: cbase, n, cut [4] (the wave's first chunk-local
    entry that fits), branch [4] ('fit' / 'in-group' / 'group-edge'), lo_e, rows [4] (table rows of each wave in the round)."""
    hits = np.asarray(hits, bool); wmax = [int(w) for w in wmax]
    out = []
    hi = max(wmax)                                                   # tile_max: the deepest contributor, not the list length
    while hi > 0:
        n = min(ch, hi); cbase = hi - n
        use = np.stack([hits[cbase:hi, w] & (cbase + np.arange(n) < wmax[w]) for w in range(4)], axis=1)
        cut, branch = [0] * 4, ["fit"] * 4
        for w in range(4):                                           # per wave: 64-entry groups from the deep end
            run = 0
            for e0 in range((n - 1) & ~63, -1, -64):
                am = np.flatnonzero(use[e0:e0 + 64, w])
                if run + am.size > cap:                              # keep the cap - run highest entries of this group
                    am = am[am.size - (cap - run):] if cap > run else am[:0]
                    cut[w] = e0 + (int(am[0]) if am.size else 64)
                    branch[w] = "in-group" if am.size else "group-edge"
                    break
                run += am.size
        lo_e = max(cut)
        out.append(dict(cbase=cbase, n=n, cut=cut, branch=branch, lo_e=lo_e, rows=[int(use[lo_e:, w].sum()) for w in range(4)]))
        hi = cbase + lo_e
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def local(q, k, ox=0.0, oy=0.0):
    """The k-th local splat of quadrant q: its middle +- 0.5 px (a fixed, spread-out sequence)."""
    dx = ((k * 7) % 11) / 10.0 - 0.5; dy = ((k * 3) % 11) / 10.0 - 0.5
    return (ox + 3.5 + 8.0 * (q & 1) + dx, oy + 3.5 + 8.0 * (q >> 1) + dy, 1.2, 1.2, 0.03)


def build(variant, entries, W=16, H=16, seed=13):
    """entries: (u, v, sx, sy, opacity) in list order = depth order = id order."""
    e = np.asarray(entries, np.float64)
    n = e.shape[0]
    return fq.crafted(variant, W, H, e[:, 0], e[:, 1], np.linspace(0.3, 1.0, n), e[:, 2], e[:, 3], e[:, 4], seed=seed, fx=400.0)


def kinds_hits(kinds):
    """The design of a layout: 'B' reaches all four quadrants, an integer q only quadrant q."""
    return np.array([[k == "B" or k == w for w in range(4)] for k in kinds], bool)


def from_kinds(variant, kinds, W=16, H=16, seed=13, replace=None):
    ent = [BROAD if k == "B" else local(k, i) for i, k in enumerate(kinds)]
    for i, e in (replace or {}).items():
        ent[i] = e
    sc = build(variant, ent, W, H, seed)
    sc["_kinds"] = list(kinds)
    return sc


def dealt(n, every, broad=(), first=0):
    """n entries: locals dealt to the four quadrants in turn; every `every`-th entry, the last one and those in `broad` are broad."""
    kinds, q = [], first
    for i in range(n):
        if i % every == every - 1 or i == n - 1 or i in broad:
            kinds.append("B")
        else:
            kinds.append(q % 4); q += 1
    return kinds


def chunk_every(variant, n, broad=()):
    """The smallest spacing of the broad entries at which no wave of any round exceeds its cap (PLANE's 91 rows need fewer broad entries)."""
    K = constants()
    for every in range(2, 65):
        kinds = dealt(n, every, broad)
        r = rounds(kinds_hits(kinds), [n] * 4, K["cap"][variant], K["ch"])
        if all(b == "fit" for x in r for b in x["branch"]):
            return every
    raise AssertionError("no spacing fits")


def n_broad(variant, n):
    return from_kinds(variant, ["B"] * n)


def chunk_case(variant, n):
    return from_kinds(variant, dealt(n, chunk_every(variant, n)))


def group_edge(variant):
    """SP_CH entries.  Group [CH-64, CH): all local to quadrant 0 (the last entry broad); the group below: CAP - 64 local to quadrant 0, spread over
    the group, the others dealt to quadrants 1-3; the groups below that dealt to all four in turn.  Wave 0 has exactly CAP rows after two groups
    and meets more in the third: the cut is the group's edge."""
    K = constants(); cap, ch = K["cap"][variant], K["ch"]
    assert 64 < cap < 128
    kinds = [None] * ch
    for i in range(ch - 64, ch):
        kinds[i] = 0
    kinds[ch - 1] = "B"
    zero = set(int(x) for x in np.round(np.linspace(ch - 128, ch - 65, cap - 64)))
    assert len(zero) == cap - 64
    o = 0
    for i in range(ch - 128, ch - 64):
        if i in zero:
            kinds[i] = 0
        else:
            kinds[i] = 1 + o % 3; o += 1
    for i in range(ch - 128):
        kinds[i] = i % 4
    return from_kinds(variant, kinds)


def dense_kinds(n, broad=()):
    """Three of four entries local to quadrant 2, the fourth dealt to quadrants 0, 1, 3 in turn; the last entry (and `broad`) broad."""
    kinds, o = [], 0
    for i in range(n):
        if i == n - 1 or i in broad:
            kinds.append("B")
        elif i % 4 == 3:
            kinds.append((0, 1, 3)[o % 3]); o += 1
        else:
            kinds.append(2)
    return kinds


def one_dense_quadrant(variant, W=16, H=16):
    return from_kinds(variant, dense_kinds(300), W, H)


def quadrants_end_early(variant, n=300, first=60, count=31):
    """n entries; `count` opaque vertical strips (centre column 11.75, sigma 2.5 px in x, as long as the tile in y) at list positions first ...
    saturate every pixel of the right two quadrants: column 8 sees alpha 0.31 per strip and column 15 0.41, column 7 only 0.16, so the left quadrants
    keep T above 1e-3 to the end of the list.  The strips reach 8 px: all four quadrants, like the broad entries, by more than a pixel (their small
    random tilt moves a strip's ridge by up to a pixel at the tile's top and bottom rows).  Before and after them: three of four entries broad, the
    fourth local to the four quadrants in turn."""
    ent, q = [], 0
    for i in range(n):
        if first <= i < first + count:
            ent.append((11.75, 7.5, 2.5, 60.0, 0.95))
        elif i % 4 == 0 and i != n - 1:
            ent.append(local(q % 4, i)); q += 1
        else:
            ent.append(BROAD)
    return build(variant, ent)


def tile_ends_early(variant, n=400, first=100, count=24):
    ent = [OPAQUE if first <= i < first + count else BROAD for i in range(n)]
    return build(variant, ent)


def cut_of_broad(variant, n):
    """cbase + lo_e of the first round of a list of n broad entries."""
    K = constants()
    r = rounds(np.ones((n, 4), bool), [n] * 4, K["cap"][variant], K["ch"])[0]
    return r["cbase"] + r["lo_e"]


def median_at_the_cut(variant, side):
    """side 0: the median contributor is the last entry of round 2; side 1: the first entry of round 1."""
    n = constants()["cap"][variant] + 20
    return fq.median_at(variant, cut_of_broad(variant, n) - 1 + side, n=n)


def median_at_the_chunk_edge(variant, slot):
    """The chunk_257 layout (SP_CH + 1 entries) with entries 0 and 1 broad and entry `slot` strong: the median on either side of cbase == 1."""
    n = constants()["ch"] + 1
    kinds = dealt(n, chunk_every(variant, n, broad=(0, 1)), broad=(0, 1))
    return from_kinds(variant, kinds, replace={slot: STRONG})


def two_tiles(variant, shared=12):
    """32x16.  Left tile: the one_dense_quadrant layout with `shared` of its entries broad; right tile: CAP + 1 entries, the same `shared` broad ones
    (sigma 60 covers both tiles) and, between them, medium splats (sigma 2.5 at (25.5, 7.5): all four quadrants of the right tile, nothing of the left)."""
    cap = constants()["cap"][variant]
    n = 300
    bpos = set(int(x) for x in np.round(np.linspace(11, n - 1, shared)))
    kinds = dense_kinds(n, broad=bpos)
    ent = []
    extra = cap + 1 - shared
    at = set(int(x) for x in np.round(np.linspace(5, n - 10, extra)))      # list positions behind which a right-only splat is inserted
    assert len(at) == extra and len(bpos) == shared
    tags = []
    for i, k in enumerate(kinds):
        ent.append(BROAD if k == "B" else local(k, i, ox=-0.5)); tags.append(k)      # (half a pixel to the left: the bounding square stays out of the right tile)
        if i in at:
            ent.append((25.5, 7.5, 2.5, 2.5, 0.03)); tags.append("R")
    sc = build(variant, ent, W=32, H=16)
    sc["_kinds"] = tags
    return sc


# name -> (variants, builder(variant)).  The table rows are asserted in tests/test_bwd_rounds_cpu.py.
def _cases():
    K = constants()
    cap, ch = K["cap"], K["ch"]
    allv = VARIANTS
    c = {
        "cap_minus_1": (allv, lambda v: n_broad(v, cap[v] - 1)),
        "cap": (allv, lambda v: n_broad(v, cap[v])),
        "cap_plus_1": (allv, lambda v: n_broad(v, cap[v] + 1)),
        "two_caps_plus_1": (allv, lambda v: n_broad(v, 2 * cap[v] + 1)),
        "chunk_255": (allv, lambda v: chunk_case(v, ch - 1)),
        "chunk_256": (allv, lambda v: chunk_case(v, ch)),
        "chunk_257": (allv, lambda v: chunk_case(v, ch + 1)),
        "chunk_513": (allv, lambda v: chunk_case(v, 2 * ch + 1)),
        "chunk_edge_and_trim": (allv, lambda v: n_broad(v, 2 * ch + 1)),
        "group_edge": (allv, group_edge),
        "one_dense_quadrant": (allv, one_dense_quadrant),
        "quadrants_end_early": (allv, quadrants_end_early),
        "tile_ends_early": (allv, tile_ends_early),
        "median_at_the_cut_0": (["surfel"], lambda v: median_at_the_cut(v, 0)),
        "median_at_the_cut_1": (["surfel"], lambda v: median_at_the_cut(v, 1)),
        "median_at_the_chunk_edge_0": (["surfel"], lambda v: median_at_the_chunk_edge(v, 0)),
        "median_at_the_chunk_edge_1": (["surfel"], lambda v: median_at_the_chunk_edge(v, 1)),
        "partly_outside_cap_plus_1": (allv, lambda v: from_kinds(v, ["B"] * (cap[v] + 1), 13, 11)),
        "partly_outside_one_dense_quadrant": (allv, lambda v: one_dense_quadrant(v, 13, 11)),
        "two_tiles": (allv, two_tiles),
    }
    return c


CASES = _cases()
CASE_IDS = [(name, v) for name, (vs, _) in CASES.items() for v in vs]
_MEMO = {}


def case(name, variant):
    """-> (scene, model), built once per process (the scene and the model are read-only)."""
    if (name, variant) not in _MEMO:
        sc = CASES[name][1](variant)
        _MEMO[(name, variant)] = (sc, model(variant, sc, tiles=2 if name == "two_tiles" else 1))
    return _MEMO[(name, variant)]


# ---------------------------------------------------------------------------------------------------------------- the model
def model(variant, sc, tiles=1):
    """Runs the float32 oracle's forward on the scene and the staging loop on what it finds.  -> dict(P, tiles=[dict(tile, list, hits, wmax, tile_max,
    rounds)], R, ranges, point_list, final_T, n_contrib).  Asserts that the scene is one the model may speak for: `tiles` tiles, every splat in a
    list, and every (entry, quadrant) decision of the region test the same with the quadrant's rectangle grown and shrunk by 0.5 px on every side --
    the kernel reads the forward's float32 ballots, which carry the safety margin of the per-Gaussian stage, the model evaluates in float64."""
    import fwd_queue_counts as fqc
    import oracle
    K = constants()
    W, H = int(sc["W"]), int(sc["H"])
    gx = (W + 15) // 16
    with oracle.Forward(sc, variant) as f:
        t = fqc.region_terms(f, variant)
        lst = f.point_list().astype(np.int64); ranges = f.ranges().astype(np.int64)
        ft, nc = f.image_state()
        R = int(f.R)
    P = sc["means3D"].shape[0]
    assert ranges.shape[0] == tiles and np.array_equal(np.unique(lst), np.arange(P)), "every splat must be in a tile's list"
    out = dict(P=P, R=R, ranges=ranges, point_list=lst, final_T=ft, n_contrib=nc, tiles=[])
    for tile in range(tiles):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        idx = np.arange(r0, r1)
        tx, ty = 16 * (tile % gx), 16 * (tile // gx)
        for d in (0.0, 0.5):                                         # the oracle lists by bounding square, the library by region: the same list only if every entry's region meets the tile
            assert fqc.region_hits(t, tx + d, ty + d, 15.0 - 2 * d, 15.0 - 2 * d, idx).all(), f"tile {tile}: an entry's region does not reach the tile"
        hits = np.zeros((r1 - r0, 4), bool); wmax = [0] * 4
        for q in range(4):
            qx, qy = tx + 8 * (q & 1), ty + 8 * (q >> 1)
            hits[:, q] = fqc.region_hits(t, float(qx), float(qy), 7.0, 7.0, idx)
            for d in (0.5, -0.5):
                other = fqc.region_hits(t, qx - d, qy - d, 7.0 + 2 * d, 7.0 + 2 * d, idx)
                assert np.array_equal(other, hits[:, q]), (f"tile {tile} quadrant {q}: {int((other != hits[:, q]).sum())} decisions change with the rectangle "
                                                             f"moved by {d} px: entries {np.flatnonzero(other != hits[:, q])[:8]}")
            blk = nc[0][qy:qy + 8, qx:qx + 8]                        # the pixels inside the image
            wmax[q] = int(blk.max()) if blk.size else 0
        out["tiles"].append(dict(tile=tile, list=lst[r0:r1], hits=hits, wmax=wmax, tile_max=max(wmax),
                                 rounds=rounds(hits, wmax, K["cap"][variant], K["ch"])))
    return out


def edge_rows(m, k=4):
    """bool [P]: the k list entries on either side of every round boundary cbase + lo_e, and the first and the last entry of each list."""
    mask = np.zeros(m["P"], bool)
    for t in m["tiles"]:
        n = t["list"].shape[0]
        pos = {0, n - 1}
        for r in t["rounds"]:
            b = r["cbase"] + r["lo_e"]
            pos.update(range(max(b - k, 0), min(b + k, n)))
        mask[t["list"][sorted(pos)]] = True
    return mask


def schedule(m):
    """One line per tile: the rounds as 'cbase+lo_e..cbase+n rows r0/r1/r2/r3 cut'."""
    out = []
    for t in m["tiles"]:
        rs = []
        for r in t["rounds"]:
            cuts = ",".join(f"w{w}:{b}@{r['cut'][w]}" for w, b in enumerate(r["branch"]) if b != "fit") or "fit"
            rs.append(f"[{r['cbase'] + r['lo_e']},{r['cbase'] + r['n']}) n={r['n']} rows {'/'.join(map(str, r['rows']))} {cuts}")
        out.append(f"list {t['list'].shape[0]} wmax {t['wmax']}: " + "; ".join(rs))
    return " | ".join(out)
