"""Inputs of the visibility-stage tests (test_visible_truth_cpu.py, test_gpu_visible_edges.py): small Octree-GS anchor sets in front of, beside and
behind a camera, at the 64-lane and 256-thread edges, plus one set of rows planted at exact gates.  numpy only; deterministic.

A case is a dict: the camera of scenes.make_camera (W, H, tanfovx, tanfovy, viewmatrix, projmatrix, campos), anchor [Na,3], level int32 [Na],
extra_level [Na] | None, scales6 [Na,6] (get_scaling's form: the first three count), rotations [Na,4] (un-normalised), voxel_size, fork,
standard_dist, resolution_scale, coarse_index, levels, scale_modifier, and for the planted case `rows` (name -> index), `exact_pred` /
`exact_depth` (rows whose gate operand is exact in float32 by construction: pinned by hand, never fragile).

Random cases are drawn again, by seed, until they meet `conditions` on the float64 truth alone (what weed_inputs of test_gpu_anchor_octree.py does)."""
import functools
import math

import numpy as np

import scenes
import visible_truth as VT

LEVELS = 6
IMAGES = ((160, 96), (150, 83))
# Na: (image, fork, extra_level given, resolution_scale, coarse_index, scale_modifier) -- every value of the issue's lists occurs, each Na once
RANDOM = {1: (0, 2, True, 1.0, 6, 1.0), 63: (1, 3, False, 0.5, 3, 0.7), 64: (0, 2, True, 1.0, 1, 1.0), 65: (1, 2, False, 1.0, 6, 0.7),
          255: (0, 3, True, 0.5, 6, 1.0), 256: (1, 2, True, 1.0, 3, 0.7), 257: (0, 3, False, 1.0, 1, 1.0), 1025: (1, 2, True, 0.5, 3, 1.0),
          4099: (0, 3, True, 1.0, 6, 0.7)}
NAMES = tuple(f"random{n}" for n in RANDOM) + ("planted",)
MAX_FRAGILE = 0.01


def lod_args(case):
    return (case["anchor"], case["level"], case["extra_level"], case["campos"], case["voxel_size"], case["fork"], case["standard_dist"],
            case["resolution_scale"], case["coarse_index"])


def lod_truth(case, mode, defect=None):
    return VT.lod(*lod_args(case), mode, exact=case.get("exact_pred"), defect=defect)


def filter_truth(case, scale_modifier=None, cov3D=None, scales=None, defect=None):
    mod = case["scale_modifier"] if scale_modifier is None else scale_modifier
    if cov3D is not None:
        return VT.prefilter(case, case["anchor"], cov3D=cov3D, exact_depth=case.get("exact_depth"))
    return VT.prefilter(case, case["anchor"], scales=case["scales6"] if scales is None else scales, rotations=case["rotations"], scale_modifier=mod,
                        exact_depth=case.get("exact_depth"), defect=defect)


def fragile(case, mode):
    """bool [Na]: fragile in the octree_visible call of this mode (any gate)"""
    return VT.fragile_gates(dict(filter_truth(case)["margins"], pred=lod_truth(case, mode)["margin"])).any(axis=1)


def conditions(case):
    """-> list of the conditions the case misses (empty: fit).  Sets with fewer than 63 anchors cannot hold shares and are exempt from them."""
    Na = case["anchor"].shape[0]
    miss = []
    pf = filter_truth(case)
    for mode in VT.MODES:
        t = lod_truth(case, mode)
        if fragile(case, mode).sum() > MAX_FRAGILE * Na:
            miss.append(f"{mode}: more than 1 % fragile")
        if Na >= 63:
            share = t["anchor_mask"].mean()
            if not 0.2 <= share <= 0.8:
                miss.append(f"{mode}: {share:.2f} masked in")
            if mode == "progressive" and (t["transition_mask"].all() or not t["transition_mask"].any()):
                miss.append("transition_mask one-sided")
    if Na >= 63:
        if not ((pf["radii"] == 0).any() and (pf["radii"] > 0).any()):
            miss.append("radii one-sided")
        if case["coarse_index"] < LEVELS and not (case["level"] > case["coarse_index"] - 1).any():
            miss.append("no level above coarse_index - 1")
        if Na >= 255 and set(case["level"].tolist()) != set(range(LEVELS)):
            miss.append("a level is missing")
    return miss


def _draw(Na, seed):
    img, fork, extra, rs, ci, mod = RANDOM[Na]
    W, H = IMAGES[img]
    r = np.random.default_rng(seed)
    fx = W * (1600.0 / 1920.0)
    cam = scenes.make_camera(W, H, fx, fx, yaw_deg=20.0, t=(0.5, 0.2, 0.0))
    # three quarters in and around the frustum (1.4 x its half-width: some beside it), the rest anywhere in a box around the camera, behind it included
    z = r.uniform(0.3, 20.0, Na)
    pc = np.stack([z * cam["tanfovx"] * r.uniform(-1.4, 1.4, Na), z * cam["tanfovy"] * r.uniform(-1.4, 1.4, Na), z], -1)
    box = r.uniform(-12.0, 12.0, (Na, 3))
    pc = np.where((r.uniform(size=Na) < 0.75)[:, None], pc, box)
    V = cam["viewmatrix"].astype(np.float64)
    anchor = (pc - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    s = np.exp(r.normal(math.log(3.0), 0.7, Na)) * np.abs(pc[:, 2]).clip(0.3) / fx
    scales6 = np.concatenate([s[:, None] * r.uniform(0.3, 1.0, (Na, 3)), r.uniform(5.0, 9.0, (Na, 3))], 1)      # the last three must not be read
    q = r.normal(0, 0.7, (Na, 4))
    level = r.choice(LEVELS, Na, p=[0.3, 0.14, 0.14, 0.14, 0.14, 0.14]).astype(np.int32)
    case = dict(cam, name=f"random{Na}", seed=seed, anchor=anchor.astype(np.float32), level=level,
                extra_level=r.uniform(-0.3, 0.3, Na).astype(np.float32) if extra else None, scales6=scales6.astype(np.float32),
                rotations=q.astype(np.float32), voxel_size=0.5, fork=float(fork), standard_dist=12.0 if fork == 2 else 20.0, resolution_scale=rs,
                coarse_index=ci, levels=LEVELS, scale_modifier=mod)
    return case


def _planted():
    """Identity view, 150 x 83, fx = fy = 100: px = 100 x / z + 74.5, py = 100 y / z + 41, grid 10 x 6.  Every row has level 0 (always masked in)
    unless it says otherwise.  An isotropic splat of scale s on the axis at depth z has a = c = (100 s / z)^2 + 0.3, b = 0, so mid^2 - det = 0 and
    lambda_max = a + sqrt(0.1): radius = ceil(3 sqrt(a + 0.31623))."""
    W, H, fx = 150, 83, 100.0
    cam = scenes.make_camera(W, H, fx, fx)
    assert np.array_equal(cam["viewmatrix"], np.eye(4, dtype=np.float32)) and not cam["campos"].any()
    vs, sd = 0.5, 10.0
    rows, A, LV, EX, S, Q = {}, [], [], [], [], []
    near = np.float32(0.2)

    def add(name, xyz, level=0, extra=0.0, s=(1e-4, 1e-4, 1e-4), q=(1.0, 0.0, 0.0, 0.0), minus_half=False):
        h = np.float32(vs / 2 / 2.0 ** level) if minus_half else np.float32(0.0)
        rows[name] = len(A)
        A.append(np.asarray(xyz, np.float32) - h); LV.append(level); EX.append(extra); S.append(s); Q.append(q)

    # depth gate z <= 0.2f: the transform is exact with an identity view (x 1 and + 0 only).  Scale 0.004 at z = 0.2: a = 4.3, radius 7
    for name, zz in (("z_at", near), ("z_above", np.nextafter(near, np.float32(1))), ("z_below", np.nextafter(near, np.float32(0))),
                     ("z_zero", np.float32(0)), ("z_negative", np.float32(-1))):
        add(name, (0, 0, zz), s=(0.004,) * 3)
    # LOD: anchor + half == campos (dist 0, pred +inf -> level cur); far away (pred about -20) and beyond float32's d^2 range (float32 pred -inf)
    add("at_camera", (0, 0, 0), level=5, minus_half=True)
    add("far_in", (0, 0, 1e7), level=0)
    add("far_out", (0, 0, 1e7), level=1)
    add("overflow_out", (0, 0, 3e19), level=1)
    # ties of 'round': dist == standard_dist exactly, so pred == extra_level exactly (log2 1 = 0): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (half to even)
    add("tie05", (0, 0, sd), level=1, extra=0.5, minus_half=True)
    add("tie15", (0, 0, sd), level=2, extra=1.5, minus_half=True)
    add("tie25", (0, 0, sd), level=3, extra=2.5, minus_half=True)
    # image borders at z = 10 with radius 3 (a = 0.3): x1 = trunc((px + 18) / 16), x0 = trunc((px - 3) / 16) clamped to [0, 10]; y likewise to [0, 6]
    px = lambda v: ((v - 74.5) / 10.0, 0.0, 10.0)
    py = lambda v: (0.0, (v - 41.0) / 10.0, 10.0)
    for name, xyz in (("left_out", px(-4.0)), ("left_in", px(0.0)), ("right_out", px(165.0)), ("right_in", px(161.0)),
                      ("top_out", py(-4.0)), ("top_in", py(0.0)), ("bottom_out", py(101.0)), ("bottom_in", py(97.0))):
        add(name, xyz)
    add("huge", (0, 0, 10.0), s=(7.11, 3.0, 7.11))                  # a = 71.1^2 + 0.3 = lambda_max: 3 sqrt = 213.31, radius 214, larger than the image
    add("zero_cov", (0, 0, 10.0), s=(0.0,) * 3)                     # cov 0: a = c = 0.3, det 0.09 (not 0), lambda_max 0.6162, 3 sqrt = 2.355: radius 3
    add("needle", (0.3, -0.2, 10.0), s=(1.0, 1e-4, 1e-4), q=(0.9, 0.2, 0.3, 0.1))
    add("zero_quat", (0, 0, 10.0), s=(0.1,) * 3, q=(0.0,) * 4)      # R = identity: a = 1.3, 3 sqrt(1.6162) = 3.81: radius 4
    Na = len(A)
    s6 = np.concatenate([np.asarray(S, np.float32), np.full((Na, 3), 7.0, np.float32)], 1)
    case = dict(cam, name="planted", seed=0, anchor=np.stack(A).astype(np.float32), level=np.asarray(LV, np.int32), extra_level=np.asarray(EX, np.float32),
                scales6=s6, rotations=np.asarray(Q, np.float32), voxel_size=vs, fork=2.0, standard_dist=sd, resolution_scale=1.0, coarse_index=LEVELS,
                levels=LEVELS, scale_modifier=1.0, rows=rows)
    ex = np.zeros(Na, bool); ex[[rows[n] for n in ("tie05", "tie15", "tie25")]] = True
    ed = np.zeros(Na, bool); ed[[rows[n] for n in ("z_at", "z_above", "z_below", "z_zero", "z_negative", "at_camera")]] = True
    case["exact_pred"], case["exact_depth"] = ex, ed
    return case


# what the planted rows must give, written by hand.  radii: of visible_filter (no LOD mask) with scale_modifier 1
PLANTED_RADII = dict(z_at=0, z_above=7, z_below=0, z_zero=0, z_negative=0, at_camera=0, far_in=3, far_out=3, overflow_out=3,
                     left_out=0, left_in=3, right_out=0, right_in=3, top_out=0, top_in=3, bottom_out=0, bottom_in=3, huge=214, zero_cov=3, zero_quat=4)
PLANTED_MARK_VISIBLE = dict(z_at=False, z_above=True, z_below=False, z_zero=False, z_negative=False)
# anchor_mask per mode (floor, round, ceil, progressive); coarse_index = levels = 6
PLANTED_MASK = dict(at_camera=(True, True, True, True), far_in=(True, True, True, True), far_out=(False, False, False, False),
                    overflow_out=(False, False, False, False),
                    tie05=(False, False, True, True),      # level 1 against floor 0 / round 0 / ceil 1 / floor(1.5) = 1
                    tie15=(False, True, True, True),       # level 2 against 1 / 2 / 2 / floor(2.5) = 2
                    tie25=(False, False, True, True))      # level 3 against 2 / 2 / 3 / floor(3.5) = 3
PLANTED_PROG = dict(tie05=(0.5, True), tie15=(0.5, True), tie25=(0.5, True), at_camera=(float(np.float32(5.0) + np.float32(0.9999)) - 5.0, True),
                    far_in=(float(np.float32(0.9999)), True), far_out=(float(np.float32(0.9999)), False))      # (prog_ratio, transition_mask)


@functools.lru_cache(maxsize=None)
def make(name):
    if name == "planted":
        return _planted()
    Na = int(name[len("random"):])
    for seed in range(1000 * Na, 1000 * Na + 200):
        case = _draw(Na, seed)
        if not conditions(case):
            return case
    raise AssertionError(f"{name}: no seed meets the conditions; the last one misses {conditions(case)}")


def scene_of(case, scale_modifier=None, cov3D=None):
    """The case as the scene dict oracle.visible_filter takes (scales [Na,3])."""
    Na = case["anchor"].shape[0]
    sc = {k: case[k] for k in ("W", "H", "tanfovx", "tanfovy", "viewmatrix", "projmatrix", "campos")}
    sc.update(means3D=case["anchor"], scales=np.ascontiguousarray(case["scales6"][:, :3]), rotations=case["rotations"],
              opacities=np.ones((Na, 1), np.float32), bg=np.zeros(3, np.float32), colors_precomp=np.zeros((Na, 3), np.float32),
              scale_modifier=case["scale_modifier"] if scale_modifier is None else scale_modifier)
    if cov3D is not None:
        sc["cov3D_precomp"] = cov3D
    return sc
