"""Scenes for densify_and_prune whose rows are NAMED by the comparison they sit on (tests/test_densify_edges_cpu.py, tests/test_gpu_densify_edges.py).

tests/densify_cases.py keeps every compared quantity a relative 1e-5 away from its threshold; these scenes do the opposite.  A named row carries
one quantity on the largest float32 below its threshold, on the threshold, or on the smallest float32 above it (np.nextafter), with the thresholds
rounded to float32 as gsrast/densify.py rounds them (ctypes.c_float), and every other quantity of the row at least 10 % from its own threshold: the
row's outcome hangs on the named comparison alone.  A quotient lands on its value exactly: denom is a power of two and accum = value * denom.

`classify_local` is a plain copy of the classification of csrc/gsr_densify.hip den_classify with one keyword per comparison that reverses it
(FLIPS); the CPU test holds it to tests/ref_densify_torch.py and shows that every flip changes the expected rows of at least one case.

Scaling and opacity are handed over ACTIVATED (densify_cases.Model(activated=...)), so no exp or sigmoid stands between a value and its comparison."""
import ctypes

import numpy as np
import torch

import densify_cases as DC

KINDS = {"vanilla": dict(cols=3, pgsr=False), "twod": dict(cols=2, pgsr=False), "pgsr": dict(cols=3, pgsr=True)}
SIDES = ("below", "on", "above")
P_NAMED = 2049
DEN_BLOCK = 1024
# values far from every threshold (clone/split 0.0002, dense 0.05, opacity 0.005, world 0.5, abs 0.0008, radius 20)
SMALL, BIG, COLD, HOT, SOLID, FAINT, COLD_ABS, HOT_ABS, NEAR_R, FAR_R = 0.02, 0.2, 0.00005, 0.0004, 0.5, 0.001, 0.0001, 0.002, 5.5, 40.5


def f32(v):
    return np.float32(ctypes.c_float(v).value)


def around(t):
    t = np.float32(t)
    return {"below": np.nextafter(t, np.float32(-np.inf)), "on": t, "above": np.nextafter(t, np.float32(np.inf))}


def thresholds(N, rules=DC.RULES):
    """The float32 thresholds of gsrast/densify.py clone_split_prune."""
    return {"grad": f32(rules["max_grad"]), "dense": f32(rules["percent_dense"] * rules["extent"]), "opacity": f32(rules["min_opacity"]),
            "world": f32(0.1 * rules["extent"]), "abs": f32(DC.ABS_RULES["abs_max_grad"]), "radii": f32(DC.ABS_RULES["abs_split_radii2D_threshold"]),
            "div": f32(0.8 * N)}


def child_sides(world, div):
    """The float32 values of max(s) whose float32 quotient by div is just below, on and just above `world`: the largest with q < world, one with
    q == world (None if no float32 gives it), the smallest with q > world; found among the neighbours of world * div."""
    c = np.float32(world * div)
    xs = [c]
    lo = hi = c
    for _ in range(64):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        xs += [lo, hi]
    xs = np.array(sorted(xs), np.float32)
    q = (xs / np.float32(div)).astype(np.float32)
    on = xs[q == world]
    return {"below": xs[q < world].max(), "on": on[len(on) // 2] if len(on) else None, "above": xs[q > world].min()}


def _row(cols, size=SMALL, g=COLD, o=SOLID, ga=COLD_ABS, radii=NEAR_R, s=None, accum=None, denom=8.0, accum_abs=None, denom_abs=8.0):
    s = [np.float32(size)] * cols if s is None else [np.float32(v) for v in s]
    assert len(s) == cols
    return {"s": s, "o": np.float32(o), "accum": np.float32(np.float32(g) * np.float32(denom)) if accum is None else np.float32(accum), "denom": np.float32(denom),
            "accum_abs": np.float32(np.float32(ga) * np.float32(denom_abs)) if accum_abs is None else np.float32(accum_abs), "denom_abs": np.float32(denom_abs),
            "radii": np.float32(radii)}


def named_groups(kind, N):
    """[(name, [row, ...])]: name = (quantity, side); a group's rows stay adjacent in the scene (a follower row has no name)."""
    cols, pgsr = KINDS[kind]["cols"], KINDS[kind]["pgsr"]
    T = thresholds(N)
    R = lambda **kw: _row(cols, **kw)
    G = []
    for side, v in around(T["grad"]).items():
        G.append((("clone_thr", side), [R(size=SMALL, g=v)]))                                  # |g| >= clone_thr on a small Gaussian
        G.append((("clone_thr_negative", side), [R(size=SMALL, g=-v)]))                        # the clone rule takes |g|
        G.append((("split_thr", side), [R(size=BIG, g=v)]))                                    # g >= split_thr on a big one
    for c in range(cols):                                                                      # max(s) against dense_thr, the maximum in each column
        for side, v in around(T["dense"]).items():
            s = [np.float32(SMALL)] * cols
            s[c] = v
            rows = [R(g=HOT, s=s)]
            if cols == 2:                                                                      # the next row's first scaling is huge: a third column read is a split
                rows.append(R(size=0.3))
            G.append(((f"dense_thr_col{c}", side), rows))
    for side, v in around(T["opacity"]).items():                                               # strict <: on a kept original, a clone pair, a split family
        G.append((("opacity_kept", side), [R(o=v)]))
        G.append((("opacity_cloned", side), [R(size=SMALL, g=HOT, o=v)]))
        G.append((("opacity_split", side), [R(size=BIG, g=HOT, o=v)]))
    for side, v in around(T["world"]).items():                                                 # strict >, only with max_screen_size
        s = [np.float32(BIG)] * cols
        s[1] = v
        G.append((("world_thr", side), [R(s=s)]))
    for side, v in child_sides(T["world"], T["div"]).items():                                  # the child's size: max(s) / f32(0.8 N) > world
        if v is not None:
            s = [np.float32(BIG)] * cols
            s[0] = v
            G.append((("child_size", side), [R(g=HOT, s=s)]))
    # special quotients of accum / denom
    G += [(("g_0/0", "small"), [R(size=SMALL, accum=0.0, denom=0.0)]), (("g_0/0", "big"), [R(size=BIG, accum=0.0, denom=0.0)]),
          (("g_x/0", "small"), [R(size=SMALL, accum=3.0, denom=0.0)]), (("g_x/0", "big"), [R(size=BIG, accum=3.0, denom=0.0)]),
          (("g_nan", "small"), [R(size=SMALL, accum=np.nan)]), (("g_nan", "big"), [R(size=BIG, accum=np.nan)]),
          (("g_negative", "small"), [R(size=SMALL, g=-HOT)]), (("g_negative", "big"), [R(size=BIG, g=-HOT)]),
          (("g_denormal", "small"), [R(size=SMALL, accum=1e-40, denom=1.0)]), (("g_denormal", "big"), [R(size=BIG, accum=1e-40, denom=1.0)])]
    if pgsr:
        hot = dict(size=BIG, radii=FAR_R)
        for side, v in around(T["abs"]).items():
            G.append((("abs_thr", side), [R(ga=v, **hot)]))                                    # ga >= abs_thr
        for side, v in around(T["dense"]).items():                                             # the abs rule's own test of max(s) > dense_thr
            G.append((("abs_dense_thr", side), [R(ga=HOT_ABS, radii=FAR_R, s=[np.float32(SMALL), v, np.float32(SMALL)])]))
        for side, v in around(T["radii"]).items():
            G.append((("radius", side), [R(size=BIG, ga=HOT_ABS, radii=v)]))                   # strict >
        G += [(("both_rules", "hot"), [R(g=HOT, ga=HOT_ABS, **hot)]),                          # a gradient split: status word 5
              (("abs_small", "hot"), [R(size=SMALL, ga=HOT_ABS, radii=FAR_R)]),                # the abs rule needs a big Gaussian
              (("ga_0/0", "big"), [R(accum_abs=0.0, denom_abs=0.0, **hot)]), (("ga_x/0", "big"), [R(accum_abs=3.0, denom_abs=0.0, **hot)]),
              (("ga_nan", "big"), [R(accum_abs=np.nan, **hot)]), (("ga_negative", "big"), [R(ga=-HOT_ABS, **hot)]),
              (("ga_denormal", "big"), [R(accum_abs=1e-40, denom_abs=1.0, **hot)])]
    return G


def _pack(rows, seed, cols, pgsr, rest=3):
    """rows -> (p, mom, stats, s_act, o_act) in the shapes of densify_cases.make_inputs; the raw scaling and opacity are only carried."""
    P = len(rows)
    r = np.random.default_rng(seed)
    col = lambda k: np.array([row[k] for row in rows], np.float32)
    s_act = np.array([row["s"] for row in rows], np.float32).reshape(P, cols)
    o_act = col("o").reshape(P, 1)
    p = {"xyz": r.normal(0, 2.0, (P, 3)), "f_dc": r.normal(0, 1, (P, 1, 3)), "f_rest": r.normal(0, 0.2, (P, rest, 3)), "opacity": r.normal(0, 1, (P, 1)),
         "scaling": r.normal(-3, 1, (P, cols)), "rotation": r.normal(0, 1, (P, 4))}
    p = {k: v.astype(np.float32) for k, v in p.items()}
    mom = {k: ((r.integers(-8, 9, v.shape) / 64.0).astype(np.float32), (r.integers(1, 9, v.shape) / 1024.0).astype(np.float32)) for k, v in p.items()}
    stats = {"xyz_gradient_accum": col("accum").reshape(P, 1), "denom": col("denom").reshape(P, 1), "max_radii2D": col("radii")}
    if pgsr:
        stats.update(xyz_gradient_accum_abs=col("accum_abs").reshape(P, 1), denom_abs=col("denom_abs").reshape(P, 1), max_weight=r.uniform(0, 1, P).astype(np.float32))
    return p, mom, stats, s_act, o_act


def named_scene(kind, N, seed, P=P_NAMED):
    """The named groups, tiled to P rows with the groups permuted by seed in every tile.  Row 0, the lane pair 63 | 64 and the rows 1023 | 1024 on
    both sides of the block limit hold selected rows (a clone, a split), so that a rank is carried over every boundary.
    -> (p, mom, stats, s_act, o_act), names [P] (None for a follower or filler row)."""
    cols, pgsr = KINDS[kind]["cols"], KINDS[kind]["pgsr"]
    groups = named_groups(kind, N)
    r = np.random.default_rng(seed)
    rows, names = [], []
    while len(rows) < P:
        for i in r.permutation(len(groups)):
            name, grp = groups[i]
            if len(rows) + len(grp) > P:
                continue
            rows += grp
            names += [name] + [None] * (len(grp) - 1)
    filler = _row(cols)
    while len(rows) < P:
        rows.append(filler); names.append(None)
    clone, split = _row(cols, size=SMALL, g=HOT), _row(cols, size=BIG, g=HOT)
    for at, row in ((0, clone), (63, split), (64, clone), (DEN_BLOCK - 1, clone), (DEN_BLOCK, split), (P - 1, split)):
        rows[at], names[at] = row, ("boundary", "clone" if row is clone else "split")      # the other tiles keep the name that stood here
    return _pack(rows, seed + 1, cols, pgsr), names


def saturated_scene(kind, P, what, seed):
    """Every row cloned, every row split, or every row pruned."""
    cols, pgsr = KINDS[kind]["cols"], KINDS[kind]["pgsr"]
    row = {"clone": _row(cols, size=SMALL, g=HOT), "split": _row(cols, size=BIG, g=HOT), "prune": _row(cols, o=FAINT)}[what]
    return _pack([row] * P, seed, cols, pgsr)


TIE_VALUES, TIE_ROWS, BOTH_ROWS = 5, 20, 16                                                                # 5 distinct masked gradients, 20 rows each


def tie_scene(which, seed):
    """PGSR scenes in which a cap binds and the quantile's interpolation position falls inside a group of equal masked gradients that extends at
    least three ranks to either side: the interpolated threshold is that value bit for bit on any device, and the strict `>` drops the whole group.
      clone: 100 small hot rows, max_all_points = P + 30        -> q = 0.7, the threshold is the 4th value, 20 clones
      split: 100 big hot rows, max_all_points = P + 30          -> the same in the gradient split (no clones: nothing is padded)
      abs:   100 big rows hot under the abs rule alone, one whose abs quotient is NaN (-> 0) and 16 hot under BOTH rules (their masked abs
             gradient is 0: `!s0`), max_abs_split_points = 30   -> P = n = 117, q = 1 - 30/117, position 86.26 inside the 4th value's ranks 77..96
             (without `!s0` the 16 rows top the order and the position falls into the 5th value's ranks 81..100: no abs split is left)
    -> (p, mom, stats, s_act, o_act), caps {max_all_points, max_abs_split_points}, tie value (float32), rows that pass."""
    cols = 3
    r = np.random.default_rng(seed)
    rows = []
    for i in range(TIE_VALUES):
        for _ in range(TIE_ROWS):
            if which == "clone":
                rows.append(_row(cols, size=SMALL, g=HOT * (1 + i)))
            elif which == "split":
                rows.append(_row(cols, size=BIG, g=HOT * (1 + i)))
            else:
                rows.append(_row(cols, size=BIG, ga=HOT_ABS * (1 + i), radii=FAR_R))
    if which == "abs":
        rows.append(_row(cols, size=BIG, accum_abs=np.nan, radii=FAR_R))
        rows += [_row(cols, size=BIG, g=HOT, ga=HOT_ABS * 50, radii=FAR_R)] * BOTH_ROWS
    rows = [rows[i] for i in r.permutation(len(rows))]
    P = len(rows)
    caps = {"clone": dict(max_all_points=P + 30, max_abs_split_points=50_000), "split": dict(max_all_points=P + 30, max_abs_split_points=50_000),
            "abs": dict(max_all_points=6_000_000, max_abs_split_points=30)}[which]
    base = HOT_ABS if which == "abs" else HOT
    tie = np.float32(np.float32(np.float32(base * 4) * np.float32(8.0)) / np.float32(8.0))
    return _pack(rows, seed + 1, cols, True), caps, tie, TIE_ROWS


def rules_for(kind, max_screen_size=20, **caps):
    r = dict(DC.RULES, max_screen_size=max_screen_size, child_rule="quotient")
    if KINDS[kind]["pgsr"]:
        r.update(DC.ABS_RULES, max_all_points=caps.get("max_all_points", 6_000_000), max_abs_split_points=caps.get("max_abs_split_points", 50_000))
    return r


# ------------------------------------------------------------------------------------------------------------------------ the classification, written out
FLIPS = ("clone_ge", "clone_abs_value", "split_ge", "dense_le", "dense_gt", "abs_ge", "radius_gt", "opacity_lt", "world_gt", "child_gt", "nan_to_zero",
         "not_s0", "cap_clone_gt", "cap_split_gt", "cap_abs_gt", "third_column")
UNREACHABLE = ("not_clone",)     # see classify_local


def _quantile(v, pad, q):
    v = torch.tensor(np.concatenate([v, np.zeros(pad, np.float32)]))
    return np.float32(float(torch.quantile(v, q)))


def classify_local(stats, s_act, o_act, rules, N=2, flip=None):
    """den_classify of csrc/gsr_densify.hip and the cap logic of gsrast/densify.py in numpy float32, one comparison per line.
    -> dict(clone, split, split_g, prune_self, prune_child) of bool [P].  flip (one of FLIPS + UNREACHABLE) reverses one comparison:
      X_ge: `>=` becomes `>`;  X_gt: `>` becomes `>=`;  X_le: `<=` becomes `<`;  X_lt: `<` becomes `<=`
      clone_abs_value: the clone rule takes g instead of |g|;  nan_to_zero: a NaN quotient stays NaN;  not_s0: the abs rule's mask loses `!s0`
      third_column: a two-column scaling is read as if it had three (the next row's first value)
      not_clone: `split = (sg || sa) && !clone` loses `!clone`.  With accumulators >= 0 every cap threshold is >= 0, a clone is then small and a
                 split big, and the guard decides nothing: no scene inside the contract can see it (the CPU test asserts that instead)."""
    T = thresholds(N, rules)
    P, cols = s_act.shape
    pgsr = "abs_max_grad" in rules
    gt = lambda a, b, name: (a >= b) if flip == name else (a > b)
    ge = lambda a, b, name: (a > b) if flip == name else (a >= b)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (stats["xyz_gradient_accum"].reshape(-1) / stats["denom"].reshape(-1)).astype(np.float32)
        if flip != "nan_to_zero":
            g = np.where(np.isnan(g), np.float32(0), g)
        ms = s_act.max(1) if P else np.zeros(0, np.float32)
        if flip == "third_column" and cols == 2:
            flat = np.concatenate([s_act.reshape(-1), np.zeros(1, np.float32)])
            ms = np.maximum(ms, flat[2 * np.arange(P) + 2])
        big = gt(ms, T["dense"], "dense_gt")
        small = (ms < T["dense"]) if flip == "dense_le" else (ms <= T["dense"])
        c0 = ge(g if flip == "clone_abs_value" else np.abs(g), T["grad"], "clone_ge") & small
        s0 = ge(g, T["grad"], "split_ge") & big
        vc, vs = np.where(c0, g, np.float32(0)), np.where(s0, g, np.float32(0))
        va = np.zeros(P, np.float32)
        if pgsr:
            ga = (stats["xyz_gradient_accum_abs"].reshape(-1) / stats["denom_abs"].reshape(-1)).astype(np.float32)
            if flip != "nan_to_zero":
                ga = np.where(np.isnan(ga), np.float32(0), ga)
            m = big & gt(stats["max_radii2D"].reshape(-1), T["radii"], "radius_gt")
            if flip != "not_s0":
                m = m & ~s0
            va = np.where(m, ga, np.float32(0))
        clone, sg, sa = c0, s0, np.zeros(P, bool)
        if pgsr:
            sa = ge(va, T["abs"], "abs_ge")
            cap_all, cap_abs = rules.get("max_all_points"), rules.get("max_abs_split_points")
            if cap_all is not None and P:
                if int(clone.sum()) + P > cap_all:
                    clone = gt(vc, _quantile(vc, 0, 1.0 - (cap_all - P) / float(P)), "cap_clone_gt")
                C = int(clone.sum())
                n = P + C
                count_g = lambda: int(((sg | sa) & ~clone & sg).sum())
                if count_g() + n > cap_all:
                    sg, sa = gt(vs, _quantile(vs, C, 1.0 - (cap_all - n) / float(n)), "cap_split_gt"), np.zeros(P, bool)
                else:
                    limited = cap_all - n - count_g()
                    if cap_abs is not None:
                        limited = min(limited, cap_abs)
                    if int(((sg | sa) & ~clone).sum()) - count_g() > limited:
                        sa = gt(va, _quantile(va, C, 1.0 - limited / float(n)), "cap_abs_gt")
        split = sg | sa
        if flip != "not_clone":
            split = split & ~clone
        low = (o_act.reshape(-1) <= T["opacity"]) if flip == "opacity_lt" else (o_act.reshape(-1) < T["opacity"])
        size = bool(rules.get("max_screen_size"))
        prune_self = low | (size & gt(ms, T["world"], "world_gt"))
        prune_child = low | (size & gt((ms / T["div"]).astype(np.float32), T["world"], "child_gt"))
    return {"clone": clone, "split": split, "split_g": split & sg, "prune_self": prune_self, "prune_child": prune_child}


def rows_of(c, N):
    """The layout of DESIGN.md §4.8 from the masks: (src map, status words [clones, splits, originals kept, clones kept, split parents whose children
    are kept, splits by the gradient rule])."""
    idx = lambda m: np.nonzero(m)[0]
    i_o, i_c, i_s = idx(~c["split"] & ~c["prune_self"]), idx(c["clone"] & ~c["prune_self"]), idx(c["split"] & ~c["prune_child"])
    src = np.concatenate([i_o, i_c] + [i_s] * N)
    return src, [int(c["clone"].sum()), int(c["split"].sum()), len(i_o), len(i_c), len(i_s), int(c["split_g"].sum())]


def quantities(stats, s_act, o_act, N, pgsr):
    """Per row, every compared quantity and its threshold: {quantity: (values [P], threshold)}."""
    T = thresholds(N)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (stats["xyz_gradient_accum"].reshape(-1) / stats["denom"].reshape(-1)).astype(np.float32)
        ms = s_act.max(1)
        q = {"g": (np.abs(g), T["grad"]), "dense": (ms, T["dense"]), "world": (ms, T["world"]), "child": ((ms / T["div"]).astype(np.float32), T["world"]),
             "opacity": (o_act.reshape(-1), T["opacity"])}
        if pgsr:
            ga = (stats["xyz_gradient_accum_abs"].reshape(-1) / stats["denom_abs"].reshape(-1)).astype(np.float32)
            q.update(ga=(ga, T["abs"]), radius=(stats["max_radii2D"].reshape(-1), T["radii"]))
    return q


NAMED_QUANTITY = {"clone_thr": "g", "clone_thr_negative": "g", "split_thr": "g", "dense_thr_col0": "dense", "dense_thr_col1": "dense", "dense_thr_col2": "dense",
                  "opacity_kept": "opacity", "opacity_cloned": "opacity", "opacity_split": "opacity", "world_thr": "world", "child_size": "child",
                  "abs_thr": "ga", "radius": "radius", "abs_dense_thr": "dense"}


# ------------------------------------------------------------------------------------------------------------------------ the cases both tests run
def noise(c, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N * int(c["split"].sum()), 3, generator=g).numpy(), torch.randn(int(c["clone"].sum()), 3, generator=g).numpy()


def case_ids():
    ids = [f"named-{kind}-N{N}-size" for kind in KINDS for N in (1, 2, 3, 4)] + [f"named-{kind}-N2-nosize" for kind in KINDS]
    for P in (64, 1024, 1025):
        ids += [f"all-{what}-{kind}-N2-P{P}" for what in ("clone", "prune") for kind in KINDS]
        ids += [f"all-split-{kind}-N{N}-P{P}" for kind, N in (("vanilla", 1), ("twod", 2), ("pgsr", 3), ("vanilla", 4), ("pgsr", 2))]
    return ids + [f"tie-{w}" for w in ("clone", "split", "abs")]


def make_case(cid):
    """-> dict(kind, N, inputs = (p, mom, stats, s_act, o_act), rules, names | None, tie | None)."""
    part = cid.split("-")
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % 100000
    if part[0] == "named":
        kind, N = part[1], int(part[2][1:])
        inputs, names = named_scene(kind, N, seed)
        return dict(kind=kind, N=N, inputs=inputs, rules=rules_for(kind, 20 if part[3] == "size" else None), names=names, tie=None)
    if part[0] == "all":
        kind, N, P = part[2], int(part[3][1:]), int(part[4][1:])
        return dict(kind=kind, N=N, inputs=saturated_scene(kind, P, part[1], seed), rules=rules_for(kind), names=None, tie=None)
    inputs, caps, tie, passing = tie_scene(part[1], seed)
    return dict(kind="pgsr", N=2, inputs=inputs, rules=rules_for("pgsr", **caps), names=None, tie=(part[1], tie, passing))
