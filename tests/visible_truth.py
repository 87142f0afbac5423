"""The visibility stage of the Scaffold-GS / Octree-GS iteration stated plainly in float64 (numpy only): which anchors get decoded.

1. `lod`: the level-of-detail mask of Octree-GS (set_anchor_mask + map_to_int_level): pred = log2(standard_dist / dist) / log2(fork) + extra_level
   with dist = |anchor + half - campos| resolution_scale and half = (voxel_size / 2) / fork^level; the integer level per mode (floor / round
   half-to-even / ceil clamped to [0, cur], or 'progressive': floor of clamp(pred + 1, 0.9999, cur + 0.9999)); anchor_mask = level <= int_level,
   prog_ratio = frac, transition_mask = level == int_level.  The clamp is done in floating point, BEFORE the integer conversion, so that
   pred = +inf (an anchor at the camera, dist = 0) gives level cur and pred = -inf gives 0.
2. `prefilter`: the filter-only preprocess of scaffold-filter: view depth gate z <= 0.2, covariance from scale (times scale_modifier) and the
   un-normalised quaternion or precomputed, EWA projection with the 1.3 tan clamp and the +0.3 low-pass, det == 0, lambda = mid +- sqrt(max(0.1,
   mid^2 - det)), radius = ceil(3 sqrt(lambda_max)), ndc2pix, the 16-pixel tile rect and its emptiness test.

Both take the float32 inputs (and the float32 literals of the formulas: 0.2f, 1.3f, 0.3f, 0.1f, 1e-7f, 0.9999f) widened exactly; everything after
is float64.  A comparison with float32 code is only honest away from the decisions a rounding can flip, so per anchor they also return how far
every gate is from flipping, relative to the size of the numbers the gate is computed from (a float32 error grows with them):
  pred    |p - rint(p)| with p = pred (- 0.5 for 'round'; + 1 for 'progressive' does not move it)         absolute: |pred| < 64 in every case
  depth   |z - 0.2| / (|V02 x| + |V12 y| + |V22 z| + |V32|)
  det     |det| / (a c + b^2)
  radius  |m - rint(m)| / (m + 2.25 (mid^2 + |det|) / (root m)) with m = 3 sqrt(lambda_max), root = sqrt(max(0.1, mid^2 - det)): the second term is
          what the cancellation in mid^2 - det costs (the FMA twin of the oracle is 9e-5 m off on a large isotropic splat, where root sits at its floor)
  rect    per operand o of the four (in tiles), min over the values k = 1 .. grid where trunc-and-clamp changes, |o - k| / (|pix| + r + 16) * 16
An anchor is ROBUST when every margin exceeds its bound in BOUND, FRAGILE otherwise; `check_octree` / `check_filter` hold a device result to the
truth exactly on the robust anchors and let a fragile anchor differ only in what its fragile gates feed.

BOUND is measured, never guessed and never taken from the HIP library: per gate, the largest deviation of the float32 CPU oracle (oracle/gsr_oracle.c
ref_visible_filter_terms, oracle/gsd_oracle.c refd_lod_pred; the -ffp-contract=off build and its FMA-contracting twin) from this truth over every
case of visible_cases.py, in the units of the margin, times 4: two float32 evaluations that round differently lie up to twice that apart, and
the factor 2 on top covers an operation order the oracle does not have.  tests/test_visible_truth_cpu.py::test_bounds_cover_the_oracle_deviation
measures them again on every run and fails if a deviation times 4 exceeds its constant.

Measured (test_visible_truth_cpu.py -s prints them; EXPERIMENTS.md keeps the table), largest oracle deviation -> x 4 -> bound:
  pred    4.60e-7 (float32 against float64 pred; the weed-out test found 3.7e-7 for the same formula)   1.84e-6 -> 2e-6
  depth   1.02e-7 of the sum of the magnitudes that make up z                                             4.1e-7 -> 5e-7
  det     2.08e-6 of a c + b^2                                                                             8.3e-6 -> 1e-5
  radius  6.2e-7 of the scale above (without its cancellation term the FMA twin is 6.7e-5 m off)          2.5e-6 -> 3e-6
  rect    1.12e-6 of (|pix| + r + 16) / 16 tiles                                                           4.5e-6 -> 5e-6
With these bounds the random cases hold 0 to 3 fragile anchors each (at most 0.4 %), the planted rows none.

|det| and the distance of 3 sqrt(lambda_max) to an integer are not used as absolute numbers: one absolute bound cannot serve a splat of radius 3
and one of radius 214, since the largest deviation over all cases is set by the large splats (det 1e9, m 200) and would call every ordinary
anchor fragile.
"""
import numpy as np

MODES = ("floor", "round", "ceil", "progressive")
GATES = ("pred", "depth", "det", "radius", "rect")
TILE = 16
# per gate: the largest measured oracle deviation, and the bound = the next round figure above 4 x that
MEASURED = dict(pred=4.6e-7, depth=1.02e-7, det=2.08e-6, radius=6.2e-7, rect=1.12e-6)
BOUND = dict(pred=2e-6, depth=5e-7, det=1e-5, radius=3e-6, rect=5e-6)
DEFECTS = ("lt", "half_away", "no_half", "stride3", "no_mod")      # planted by test_visible_truth_cpu.py; never set otherwise


def _w(a):
    """float32 value(s), widened exactly"""
    return np.asarray(a, np.float32).astype(np.float64)


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------------- LOD mask
def lod(anchor, level, extra_level, campos, voxel_size, fork, standard_dist, resolution_scale, coarse_index, mode, exact=None, defect=None):
    """-> dict(pred, int_level int64, anchor_mask, prog_ratio | None, transition_mask | None, margin): see the module text.
    exact: bool [Na] or None, rows whose pred is exact in float32 by construction (their margin is +inf)."""
    a, cp = _w(anchor).reshape(-1, 3), _w(campos).reshape(3)
    lv = np.asarray(level).reshape(-1).astype(np.int64)
    vs, fk, sd, rs = (_f32(v) for v in (voxel_size, fork, standard_dist, resolution_scale))
    half = (vs / 2.0) / fk ** lv.astype(np.float64)
    if defect == "no_half":
        half = half * 0.0
    d = (a + half[:, None]) - cp[None, :]
    dist = np.sqrt((d * d).sum(axis=1)) * rs
    with np.errstate(divide="ignore"):
        pred = np.log2(sd / dist) / np.log2(fk)
    if extra_level is not None:
        pred = pred + _w(extra_level).reshape(-1)
    cur = int(coarse_index) - 1
    prog = trans = None
    if mode == "progressive":
        lo, hi = _f32(0.9999), float(np.float32(cur) + np.float32(0.9999))
        p = np.clip(pred + 1.0, lo, hi)
        il = np.floor(p).astype(np.int64)
        prog = p - np.trunc(p)
        trans = lv == il
        shifted = pred
    else:
        if mode == "round":
            r = np.floor(np.abs(pred) + 0.5) * np.sign(pred) if defect == "half_away" else np.rint(pred)      # rint: half to even, as torch.round
        else:
            r = {"floor": np.floor, "ceil": np.ceil}[mode](pred)
        il = np.clip(r, 0.0, float(cur)).astype(np.int64)              # the clamp in floating point, then the conversion
        shifted = pred - 0.5 if mode == "round" else pred
    mask = (lv < il) if defect == "lt" else (lv <= il)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(shifted), np.abs(shifted - np.rint(shifted)), np.inf)
    if exact is not None:
        margin = np.where(np.asarray(exact, bool), np.inf, margin)
    return dict(pred=pred, int_level=il, anchor_mask=mask, prog_ratio=prog, transition_mask=trans, margin=margin)


# ---------------------------------------------------------------------------------------------------------------------------------- prefilter
def _cov3d(scales, mod, rot):
    """Sigma = (S R)^T (S R) with the un-normalised quaternion, as forward.cu computeCov3D: [P,3,3]"""
    s = scales * mod
    r, x, y, z = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]
    # glm is column-major: R's constructor arguments fill columns, so the matrix written row by row here is the transpose of the usual one
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    Rm = R.transpose(0, 2, 1)                   # glm R as a mathematical matrix (columns = constructor triples)
    M = s[:, :, None] * Rm                      # M = S R
    return M.transpose(0, 2, 1) @ M


def _sym(c6):
    c = np.zeros(c6.shape[:1] + (3, 3))
    c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2] = (c6[:, k] for k in range(6))
    c[:, 1, 0], c[:, 2, 0], c[:, 2, 1] = c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]
    return c


def _rect(px, py, r, gx, gy):
    """-> (ops [P,4] in tiles, rect [P,4] int64 (x0, y0, x1, y1), empty [P], margin [P])"""
    ops = np.stack([(px - r) / TILE, (py - r) / TILE, (px + r + (TILE - 1)) / TILE, (py + r + (TILE - 1)) / TILE], 1)
    g = np.array([gx, gy, gx, gy], np.float64)
    with np.errstate(invalid="ignore"):
        rect = np.clip(np.trunc(np.nan_to_num(ops, nan=0.0, posinf=1e9, neginf=-1e9)), 0.0, g[None, :]).astype(np.int64)
        empty = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]) == 0
        # the operand's value changes where it crosses k = 1 .. grid (below 1 it is 0, truncation towards zero included; above grid it is grid)
        k = np.clip(np.rint(ops), 1.0, g[None, :])
        scale = (np.abs(np.stack([px, py, px, py], 1)) + np.abs(r)[:, None] + TILE) / TILE
        margin = (np.abs(ops - k) / scale).min(axis=1)
    return ops, rect, empty, np.where(np.isnan(margin), 0.0, margin)


def prefilter(cam, means3D, scales=None, rotations=None, cov3D=None, scale_modifier=1.0, exact_depth=None, defect=None):
    """cam: dict(W, H, tanfovx, tanfovy, viewmatrix [4,4], projmatrix [4,4]) as tests/scenes.make_camera gives it.  scales [P,3] or get_scaling's
    [P,6] (the first three count) with rotations [P,4], or cov3D [P,6] float32.
    -> dict(radii int64, visible, margins {gate: [P]}, raw int64 (ceil(3 sqrt(lambda_max)) before any gate), other int64 (that ceiling had m come
       out on the other side of its nearest integer), alt int64 (`other` after its own rect test), terms [P,7] in the layout of
       oracle.visible_filter_terms, scales {gate: the sizes the margins are relative to})."""
    P = np.asarray(means3D).shape[0]
    p = _w(means3D).reshape(P, 3)
    V, F = _w(cam["viewmatrix"]).reshape(4, 4), _w(cam["projmatrix"]).reshape(4, 4)
    W, H = int(cam["W"]), int(cam["H"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tx, ty = _f32(cam["tanfovx"]), _f32(cam["tanfovy"])
    fx, fy = W / (2.0 * tx), H / (2.0 * ty)
    mod = 1.0 if defect == "no_mod" else _f32(scale_modifier)
    with np.errstate(all="ignore"):
        t = p @ V[:3, :3] + V[3, :3]                                   # row-vector convention: p_view = [p 1] V
        z = t[:, 2]
        zscale = np.abs(p * V[:3, 2][None, :]).sum(axis=1) + abs(V[3, 2])
        near = _f32(0.2)
        culled = z <= near
        m_depth = np.abs(z - near) / np.maximum(zscale, 1e-300)
        if exact_depth is not None:
            m_depth = np.where(np.asarray(exact_depth, bool), np.inf, m_depth)
        hom = p @ F[:3, :] + F[3, :]
        p_w = 1.0 / (hom[:, 3] + _f32(0.0000001))
        if cov3D is not None:
            Vrk = _sym(_w(cov3D).reshape(P, 6))
        else:
            sc = _w(scales)
            sc = sc.reshape(-1)[:3 * P].reshape(P, 3) if defect == "stride3" else sc.reshape(P, -1)[:, :3]
            Vrk = _cov3d(sc, mod, _w(rotations).reshape(P, 4))
        limx, limy = _f32(1.3) * tx, _f32(1.3) * ty
        tcx = np.clip(t[:, 0] / z, -limx, limx) * z
        tcy = np.clip(t[:, 1] / z, -limy, limy) * z
        J = np.zeros((P, 3, 3))                                        # mathematical matrix: rows (fx/z, 0, -fx tx / z^2), (0, fy/z, -fy ty / z^2), 0
        J[:, 0, 0], J[:, 0, 2] = fx / z, -(fx * tcx) / (z * z)
        J[:, 1, 1], J[:, 1, 2] = fy / z, -(fy * tcy) / (z * z)
        Wm = V[:3, :3].T                                               # world -> view rotation acting on column vectors
        T = J @ Wm[None, :, :]
        c2 = T @ Vrk @ T.transpose(0, 2, 1)
        a, b, c = c2[:, 0, 0] + _f32(0.3), c2[:, 0, 1], c2[:, 1, 1] + _f32(0.3)
        det = a * c - b * b
        m_det = np.abs(det) / (np.abs(a * c) + b * b)
        mid = 0.5 * (a + c)
        root = np.sqrt(np.maximum(_f32(0.1), mid * mid - det))
        m = 3.0 * np.sqrt(np.maximum(mid + root, mid - root))
        raw = np.ceil(m)
        near_int = np.rint(m)
        # float32 loses mid^2 - det to cancellation: an error eps (mid^2 + |det|) there moves the root by that / (2 root) and m by 9 / (2 m) of that
        rad_scale = m + 2.25 * (mid * mid + np.abs(det)) / (root * m)
        m_rad = np.abs(m - near_int) / rad_scale
        other = np.where(m <= near_int, near_int + 1.0, near_int)     # the ceiling, had m come out on the other side of its nearest integer
        px = ((hom[:, 0] * p_w + 1.0) * W - 1.0) * 0.5
        py = ((hom[:, 1] * p_w + 1.0) * H - 1.0) * 0.5
        raw_i = np.nan_to_num(raw, nan=0.0, posinf=2.0e9).astype(np.int64)
        other_i = np.nan_to_num(other, nan=0.0, posinf=2.0e9).astype(np.int64)
        ops, _, empty, m_rect = _rect(px, py, raw_i.astype(np.float64), gx, gy)
        _, _, empty_o, _ = _rect(px, py, other_i.astype(np.float64), gx, gy)
    dead_det = ~culled & (det == 0.0)
    live = ~culled & ~dead_det
    radii = np.where(live & ~empty, raw_i, 0)
    alt = np.where(empty_o, 0, other_i)
    nan_bad = lambda v: np.where(np.isnan(v), 0.0, v)                  # a margin that cannot be evaluated is no margin
    settled = culled & (m_depth > BOUND["depth"])                      # behind the depth gate beyond doubt: the later gates are never reached
    margins = dict(pred=np.full(P, np.inf), depth=nan_bad(m_depth), det=np.where(settled, np.inf, nan_bad(m_det)),
                   radius=np.where(settled, np.inf, nan_bad(m_rad)), rect=np.where(settled, np.inf, m_rect))
    terms = np.full((P, 7), np.nan)
    terms[:, 0] = z
    terms[~culled, 1] = det[~culled]
    terms[live, 2] = m[live]
    terms[live, 3:] = ops[live]
    return dict(radii=radii, visible=radii > 0, margins=margins, raw=raw_i, alt=alt, other=other_i, terms=terms,
                scales=dict(depth=zscale, det=np.abs(a * c) + b * b, radius=rad_scale, rect=(np.abs(np.stack([px, py, px, py], 1)) + raw_i[:, None] + TILE) / TILE))


def fragile_gates(margins):
    """-> bool [P, len(GATES)]: which gates of which anchor lie within their bound"""
    return np.stack([margins[g] <= BOUND[g] for g in GATES], 1)


def closest_gate(margins):
    """-> the name of the gate with the smallest margin / bound per anchor"""
    with np.errstate(invalid="ignore"):
        rel = np.stack([margins[g] / BOUND[g] for g in GATES], 1)
    return np.array(GATES)[np.argmin(np.nan_to_num(rel, nan=0.0), axis=1)]


# ---------------------------------------------------------------------------------------------------------------------------------- checkers
def check_filter(got_radii, pf, in_mask=None, label=""):
    """got_radii [P] against prefilter()'s result `pf` restricted to in_mask (None: all).  Robust anchors: equal.  A fragile anchor may show what
    its fragile gates can turn it into: depth / det / rect switch between 0 and the ungated radius, radius moves to the neighbouring integer
    (with that radius' own rect test).  -> dict gate -> (fragile, differing)."""
    got = np.asarray(got_radii).astype(np.int64).reshape(-1)
    P = got.shape[0]
    keep = np.ones(P, bool) if in_mask is None else np.asarray(in_mask, bool).reshape(-1)
    want = np.where(keep, pf["radii"], 0)
    frag = fragile_gates(pf["margins"]) & keep[:, None]
    gi = {g: i for i, g in enumerate(GATES)}
    onoff = frag[:, gi["depth"]] | frag[:, gi["det"]] | frag[:, gi["rect"]]
    ok = got == want
    ok |= onoff & ((got == 0) | (got == pf["raw"]))
    ok |= frag[:, gi["radius"]] & ((got == pf["alt"]) | (onoff & (got == pf["other"])))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (f"{label}: {bad.size} radii differ from the float64 truth away from every gate; first rows {bad[:8].tolist()}: got {got[bad[:8]].tolist()} "
                           f"want {want[bad[:8]].tolist()} closest gate {closest_gate(pf['margins'])[bad[:8]].tolist()}")
    diff = got != want
    return {g: (int(frag[:, gi[g]].sum()), int((diff & frag[:, gi[g]]).sum())) for g in GATES if g != "pred"}


def check_lod(got, truth, label=""):
    """got: dict(anchor_mask, prog_ratio | None, transition_mask | None) of numpy arrays against lod()'s result.  Robust anchors: masks equal,
    prog_ratio within BOUND['pred']; fragile ones may flip, and their prog_ratio may wrap: within the bound modulo 1.  -> (fragile, flipped)."""
    frag = truth["margin"] <= BOUND["pred"]
    gm = np.asarray(got["anchor_mask"]).astype(bool).reshape(-1)
    flips = gm != truth["anchor_mask"]
    bad = np.nonzero(flips & ~frag)[0]
    assert bad.size == 0, f"{label}: anchor_mask differs on {bad.size} robust anchors, first {bad[:8].tolist()} pred {truth['pred'][bad[:8]].tolist()}"
    if truth["prog_ratio"] is None:
        assert got.get("prog_ratio") is None and got.get("transition_mask") is None, f"{label}: optional outputs must stay None"
        return int(frag.sum()), int(flips.sum())
    gt = np.asarray(got["transition_mask"]).astype(bool).reshape(-1)
    tf = gt != truth["transition_mask"]
    bad = np.nonzero(tf & ~frag)[0]
    assert bad.size == 0, f"{label}: transition_mask differs on {bad.size} robust anchors, first {bad[:8].tolist()}"
    gp = np.asarray(got["prog_ratio"], np.float64).reshape(-1)
    d = np.abs(gp - truth["prog_ratio"])
    d = np.where(frag, np.minimum(d, np.abs(1.0 - d)), d)
    bad = np.nonzero(~(d <= BOUND["pred"]))[0]
    assert bad.size == 0, f"{label}: prog_ratio off by {d[bad[:8]].tolist()} at {bad[:8].tolist()} (bound {BOUND['pred']})"
    return int(frag.sum()), int((flips | tf).sum())


def check_octree(got, truth, pf, label=""):
    """One octree_visible result (numpy arrays) against lod() and prefilter(): the LOD outputs by check_lod, the radii against the prefilter
    truth under the DEVICE's anchor_mask (a flipped mask takes its radius with it), visible_mask == radii > 0.  -> dict gate -> (fragile, differing)."""
    stats = {"pred": check_lod(got, truth, label)}
    gm = np.asarray(got["anchor_mask"]).astype(bool).reshape(-1)
    radii = np.asarray(got["radii"]).reshape(-1)
    stats.update(check_filter(radii, pf, gm, label))
    assert np.array_equal(np.asarray(got["visible_mask"]).astype(bool).reshape(-1), radii > 0), f"{label}: visible_mask is not radii > 0"
    return stats
