"""CPU: the scenes of tests/bwd_round_scenes.py reach the edges of the blend backward's staging loop they were built for, and the criterion of
tests/parity_truth.py sees a fault at such an edge.

(1) rounds(), the restatement of the `while (hi > 0)` loop of k_blend_bwd_sp (gs-sr_amd/csrc/gsr_blend_sp.hip), is held to the source's constants and
    statements and to a second implementation that goes wave by wave, entry by entry.
(2) Every case, at every variant it applies to, produces the schedule its docstring states: rounds, cuts, branches, rows per wave -- asserted on the
    model, since the kernel has no instrumentation -- and its float64 truth is one the criterion accepts (robust pixels >= 0.9).
(3) A single mishandled (boundary entry, quadrant) or (boundary entry, 4x4 block) pair trips check_case once the entries at the round boundaries are
    held as a row group of their own; the whole-tensor bars alone barely see the block fault."""
import os
import re

import numpy as np
import pytest

import bwd_round_scenes as br
import oracle
import parity_truth as pt
import scenes

K = br.constants()
CAP, CH = K["cap"], K["ch"]
_ORACLES = {}


def out_grads(variant, sc, seed=1):
    return scenes.random_out_grads(variant, int(sc["W"]), int(sc["H"]), seed=seed, scale=1.0)


def oracles(name, variant):
    """(og, f32, fma, truth) of a case, computed once and left unchanged."""
    if (name, variant) not in _ORACLES:
        sc, _ = br.case(name, variant)
        og = out_grads(variant, sc)
        f32, fma, truth, _ = pt.run_oracles(sc, variant, og)
        _ORACLES[(name, variant)] = (og, f32, fma, truth)
    return _ORACLES[(name, variant)]


# ------------------------------------------------------------------------------------------------------------------ (1) the staging loop
def rounds_brute(hits, wmax, cap, ch):
    """Wave by wave, entry by entry from the deep end of the chunk, counting until the cap."""
    hits = np.asarray(hits, bool)
    out = []
    hi = max(int(w) for w in wmax)
    while hi > 0:
        n = ch if hi > ch else hi
        cbase = hi - n
        cut, branch = [], []
        for w in range(4):
            used = [e for e in range(n - 1, -1, -1) if hits[cbase + e, w] and cbase + e < wmax[w]]      # deepest first
            if len(used) <= cap:
                cut.append(0); branch.append("fit")
                continue
            e_cap, e_over = used[cap - 1], used[cap]            # the last entry that fits, the first that does not
            if e_cap // 64 == e_over // 64:
                cut.append(e_cap); branch.append("in-group")
            else:                                                # the table was full exactly at the end of a 64-entry group: the cut is that group's edge
                cut.append((e_over // 64) * 64 + 64); branch.append("group-edge")
        lo_e = max(cut)
        rows = [sum(1 for e in range(lo_e, n) if hits[cbase + e, w] and cbase + e < wmax[w]) for w in range(4)]
        out.append(dict(cbase=cbase, n=n, cut=cut, branch=branch, lo_e=lo_e, rows=rows))
        hi = cbase + lo_e
    return out


def test_the_staging_loop_model_is_held_to_the_source_and_to_a_brute_force_loop():
    assert 128 < CH <= 256 and CH % 64 == 0 and all(64 < c < 128 for c in CAP.values()), K      # what group_edge's construction and the uint8 queues assume
    with open(os.path.join(br.CSRC, "gsr_blend_sp.hip")) as fh:
        src = fh.read()
    for stmt in ("uint32_t hi = tile_max;", "while (hi > 0) {", "const uint32_t n = min((uint32_t)SP_CH, hi);", "const uint32_t cbase = hi - n;",
                 "for (int e0 = (int)((n - 1u) & ~63u); e0 >= 0; e0 -= 64) {", "(cbase + e < wmax));", "if (run + c > (uint32_t)CAPV) {",
                 "while ((uint32_t)__popcll(am) > (uint32_t)CAPV - run) am &= am - 1ull;",
                 "first = (uint32_t)e0 + (am ? (uint32_t)__ffsll((unsigned long long)am) - 1u : 64u);",
                 "const uint32_t lo_e = max(max(s_lo[0], s_lo[1]), max(s_lo[2], s_lo[3]));", "hi = cbase + lo_e;"):
        assert stmt in src, f"the staging loop changed ({stmt!r}): rounds() restates it and has to follow"
    assert re.search(r"constexpr int CAPV = \(V == GSR_EWA\) \? SP_CAP_EWA : \(V == GSR_PLANE \? SP_CAP_PLANE : SP_CAP_SURFEL\);", src)
    rng = np.random.default_rng(5)
    seen = {"fit": 0, "in-group": 0, "group-edge": 0}
    empty_round_waves = 0
    for i in range(200):
        n = int(rng.integers(1, 701)) if i % 10 else int(rng.choice([1, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1, 700]))
        cap = int(rng.choice(list(CAP.values()) + [5, 64]))
        dens = rng.choice([0.0, 0.05, 0.3, 0.6, 0.9, 1.0], 4)
        hits = rng.uniform(0, 1, (n, 4)) < dens                  # all-false columns among them
        wmax = [int(rng.integers(0, n + 1)) if rng.uniform() < 0.5 else n for _ in range(4)]
        if i % 7 == 0:
            wmax[int(rng.integers(0, 4))] = 0                    # a wave with no contributor at all
        if i % 4 == 1 and n >= 192 and cap > 64:                 # a column that fills its table exactly at a group's edge
            w = int(rng.integers(0, 4)); top = min(n, CH); wmax[w] = n
            base = n - top
            g1 = ((top - 1) // 64) * 64                          # chunk-local start of the first (deepest) group
            hits[base + g1:n, w] = True
            need = cap - (top - g1)
            if 0 < need <= 64:
                hits[base + g1 - 64:base + g1, w] = False
                hits[base + g1 - 64 + rng.choice(64, need, replace=False), w] = True
        a, b = br.rounds(hits, wmax, cap, CH), rounds_brute(hits, wmax, cap, CH)
        assert a == b, (i, n, cap, wmax, a, b)
        assert (len(a) == 0) == (max(wmax) == 0)
        for r in a:
            assert r["lo_e"] < r["n"] and max(r["rows"]) <= cap                              # every round makes progress and fits
            for x in r["branch"]:
                seen[x] += 1
            empty_round_waves += sum(1 for x in r["rows"] if x == 0)
        got = sum(r["n"] - r["lo_e"] for r in a)
        assert got == max(wmax)                                  # the rounds tile [0, tile_max) without gap or overlap
    assert min(seen.values()) >= 10 and empty_round_waves >= 10, (seen, empty_round_waves)


# ------------------------------------------------------------------------------------------------------------------ (2) every case, every variant
def _all_fit(R):
    return all(b == "fit" for r in R for b in r["branch"]) and all(r["lo_e"] == 0 for r in R)


def _deferred_per_quadrant(t, others=(0, 1, 3)):
    """Entries of the first round's chunk in front of its cut that reach quadrant q alone: staged, not taken, staged again with the next chunk."""
    r = t["rounds"][0]
    front = t["hits"][r["cbase"]:r["cbase"] + r["lo_e"]]
    return [int((front[:, q] & (front.sum(axis=1) == 1)).sum()) for q in others]


def _dense(t, cap, bound=14):
    R = t["rounds"]
    assert [r["branch"][2] for r in R].count("in-group") == 2 and R[0]["branch"][2] == R[1]["branch"][2] == "in-group"
    for r in R:
        assert all(r["branch"][w] == "fit" and r["rows"][w] <= bound for w in (0, 1, 3)), r
    assert R[0]["rows"][2] == R[1]["rows"][2] == cap
    assert min(_deferred_per_quadrant(t)) >= 1, _deferred_per_quadrant(t)


def _cap_plus_1(t, cap):
    R = t["rounds"]
    assert len(R) == 2 and R[0]["rows"] == [cap] * 4 and R[1]["n"] == 1 and R[1]["rows"] == [1] * 4 and R[0]["lo_e"] == 1


def expect(name, variant, sc, m):
    cap = CAP[variant]
    t = m["tiles"][0]
    R = t["rounds"]
    n = t["list"].shape[0]
    if name == "cap_minus_1":
        assert len(R) == 1 and _all_fit(R) and R[0]["rows"] == [cap - 1] * 4
    elif name == "cap":
        assert len(R) == 1 and _all_fit(R) and R[0]["rows"] == [cap] * 4
    elif name in ("cap_plus_1", "partly_outside_cap_plus_1"):
        _cap_plus_1(t, cap)
    elif name == "two_caps_plus_1":
        assert [r["rows"] for r in R] == [[cap] * 4, [cap] * 4, [1] * 4] and R[2]["n"] == 1
    elif name in ("chunk_255", "chunk_256"):
        assert n == CH - 1 + (name == "chunk_256") and len(R) == 1 and _all_fit(R) and R[0]["n"] == n and max(R[0]["rows"]) <= cap
    elif name in ("chunk_257", "chunk_513"):
        assert n == {"chunk_257": CH + 1, "chunk_513": 2 * CH + 1}[name]
        assert len(R) == (n - 1) // CH + 1 and _all_fit(R) and all(r["n"] == CH for r in R[:-1])
        assert R[-1]["n"] == 1 and sorted(R[-1]["rows"]) == [0, 0, 0, 1]                       # three waves without a row
    elif name == "chunk_edge_and_trim":
        hi, want = 2 * CH + 1, []
        while hi > 0:                                                                        # all entries reach all quadrants: a round takes CAP of them
            nn = min(CH, hi); want.append((hi - nn, nn, min(nn, cap))); hi -= min(nn, cap)
        assert [(r["cbase"], r["n"], r["rows"][0]) for r in R] == want and all(len(set(r["rows"])) == 1 for r in R)
        assert sum(1 for r in R if r["n"] == CH and r["rows"] == [cap] * 4) >= 3 and R[1]["cbase"] % 64 != 0
    elif name == "group_edge":
        assert n == CH and len(R) == 2 and R[0]["branch"] == ["group-edge", "fit", "fit", "fit"] and R[0]["cut"][0] == R[0]["lo_e"] == CH - 128
        assert R[0]["rows"][0] == cap and _all_fit(R[1:])
    elif name in ("one_dense_quadrant", "partly_outside_one_dense_quadrant"):
        assert n == 300
        _dense(t, cap)
    elif name == "quadrants_end_early":
        assert n == 300 and t["wmax"][0] == t["wmax"][2] == 300 and max(t["wmax"][1], t["wmax"][3]) < 100 and min(t["wmax"][1], t["wmax"][3]) > 60
        assert R[0]["branch"][0] != "fit" and R[0]["branch"][2] != "fit" and max(R[0]["rows"][1], R[0]["rows"][3]) <= 3
        assert any(r["rows"][1] > 3 for r in R[1:])                                           # ... and they do have rows later
    elif name == "tile_ends_early":
        assert n == 400 and t["tile_max"] < 130 and R[0]["cbase"] + R[0]["n"] == t["tile_max"] and t["tile_max"] > 100
    elif name.startswith("median_at_the_cut"):
        side = int(name[-1])
        b = R[0]["cbase"] + R[0]["lo_e"]
        assert len(R) == 2 and 0 < b < n and (m["n_contrib"][1] == b + side).all()           # 1-based: entry b - 1 (last of round 2) / entry b (first of round 1)
    elif name.startswith("median_at_the_chunk_edge"):
        slot = int(name[-1])
        assert n == CH + 1 and len(R) == 2 and _all_fit(R) and R[0]["cbase"] == 1 and (m["n_contrib"][1] == slot + 1).all()
    elif name == "two_tiles":
        _dense(t, cap, bound=20)                                                              # (the shared broad entries are rows of every wave)
        _cap_plus_1(m["tiles"][1], cap)
        assert np.intersect1d(t["list"], m["tiles"][1]["list"]).size >= 10
    else:
        raise AssertionError(name)
    if name.startswith("partly_outside"):
        assert (int(sc["W"]), int(sc["H"])) == (13, 11)
    if name == "two_tiles":
        assert (int(sc["W"]), int(sc["H"])) == (32, 16)


NO_EARLY_END = [n for n in br.CASES if n not in ("quadrants_end_early", "tile_ends_early")]


@pytest.mark.parametrize("name,variant", br.CASE_IDS)
def test_every_case_reaches_the_schedule_it_was_built_for(name, variant):
    sc, m = br.case(name, variant)
    print(name, variant, br.schedule(m))
    expect(name, variant, sc, m)
    assert m["P"] <= 520 and int(sc["W"]) * int(sc["H"]) <= 512
    og, f32, fma, truth = oracles(name, variant)
    robust = float((truth["margin"] > 1.0).mean())
    print("robust pixel fraction", robust, "final_T min", float(m["final_T"][0].min()))
    assert robust >= 0.9
    if name in NO_EARLY_END:
        assert m["final_T"][0].min() > 1e-4
        for t in m["tiles"]:
            assert t["tile_max"] == t["list"].shape[0]
    assert br.edge_rows(m).sum() >= 2


# ------------------------------------------------------------------------------------------------------------------ (3) the criterion has the power
def _part(sc, variant, og, x0, y0, w, h):
    """The part of every gradient that comes from the pixels of a rectangle: the backward is linear in the upstream gradients."""
    og2 = {}
    for k, a in og.items():
        z = np.zeros_like(a); z[..., y0:y0 + h, x0:x0 + w] = a[..., y0:y0 + h, x0:x0 + w]; og2[k] = z
    with oracle.Forward(sc, variant) as f:
        return f.backward(**og2)


def _in_group_ratio(variant, grads, f32, fma, truth, sel):
    """max over the gradient tensors of (relative L2 of the group's rows vs the truth) / (the smaller of check_grad's two bars on it)."""
    worst = 0.0
    keys = [b for _, b in pt.GRAD_PAIRS] + ["dL_dcolors"] + (["dL_dall_map", "dL_dmeans2D_abs"] if variant == "plane" else [])
    for b in keys:
        t = np.asarray(truth["grads"][b], np.float64).reshape(sel.shape[0], -1)[sel]
        rel = lambda x: pt._rel(np.asarray(x, np.float64).reshape(sel.shape[0], -1)[sel], t)
        bar = max(pt.TOL_GRAD, 2.0 * max(rel(f32["grads"][b]), rel(fma["grads"][b])))
        bar = min(bar, max(pt.TOL_GRAD, pt.FLOOR_SLACK * rel(truth["floor"]["grads"][b])))
        worst = max(worst, rel(grads[b]) / bar)
    return worst


@pytest.mark.parametrize("variant", br.VARIANTS)
@pytest.mark.parametrize("name", ["cap_plus_1", "one_dense_quadrant", "group_edge", "chunk_edge_and_trim"])
def test_a_fault_at_a_round_boundary_trips_the_criterion(name, variant):
    sc, m = br.case(name, variant)
    og, f32, fma, truth = oracles(name, variant)
    t = m["tiles"][0]
    groups = {"round edges": br.edge_rows(m)}
    pt.check_case(variant, "precomp", dict(f32), f32, fma, truth, row_groups=groups)          # the unmodified float32 oracle passes
    r0 = t["rounds"][0]
    b = r0["cbase"] + r0["lo_e"]                                                               # first entry of round 1; b - 1 is the last of round 2
    assert 0 < b < t["list"].shape[0]
    q = next(w for w in range(4) if t["hits"][b, w] and b < t["wmax"][w])
    gid, gprev = int(t["list"][b]), int(t["list"][b - 1])
    qx, qy = 8 * (q & 1), 8 * (q >> 1)
    quad = _part(sc, variant, og, qx, qy, 8, 8)
    assert np.abs(quad["dL_dopacity"][gid]).max() > 0
    mutants = {"quadrant dropped": (quad, -1.0, None), "quadrant added twice": (quad, +1.0, None), "first of a round as the last of the next": (quad, -1.0, gprev)}
    for k in range(4):
        blk = _part(sc, variant, og, qx + 4 * (k & 1), qy + 4 * (k >> 1), 4, 4)
        if np.abs(blk["dL_dopacity"][gid]).max() > 0:
            mutants[f"4x4 block {k} dropped"] = (blk, -1.0, None)
    assert len(mutants) >= 4
    rows = pt.robust_rows(truth["splat"], ~(truth["margin"] > 1.0), m["P"]) & groups["round edges"]
    assert rows[gid]
    weakest = (np.inf, None)
    for what, (part, sign, other) in mutants.items():
        g = {k: np.array(v, copy=True) for k, v in f32["grads"].items()}
        for k in g:
            if g[k].shape[0] == m["P"] and g[k].size:
                g[k][gid] += sign * part[k][gid]
                if other is not None:
                    g[k][gid] += part[k][other]
        cand = dict(f32); cand["grads"] = g
        with pytest.raises(AssertionError):
            pt.check_case(variant, "precomp", cand, f32, fma, truth, row_groups=groups)
        ratio = _in_group_ratio(variant, g, f32, fma, truth, rows)
        assert ratio > 1.0, (what, ratio)                                                      # ... and it is the group's L2 bar that it trips
        weakest = min(weakest, (ratio, what))
    print(f"{name} {variant}: boundary {b} quadrant {q}, {len(mutants)} mutants caught; weakest '{weakest[1]}': in-group relative L2 / bar = {weakest[0]:.2f}")
