"""Hand-placed scenes for the batch queue of the blend forward (TEST INFRASTRUCTURE; tests/test_gpu_fwd_queues.py, numpy only).

k_blend_fwd<V> (gs-sr_amd/csrc/gsr_blend.hip) consumes a tile's list 64 entries at a time; each 8x8 quadrant's wave walks the queue of the batch's
entries that can reach it.  The scenes put splats at chosen pixels with chosen footprints, depths (= list order) and opacities under the pose-0 camera
(identity view matrix), so that one half of a quadrant saturates while the other goes on, a region meets exactly one 8x2 strip of a quadrant, a list
ends at a batch edge, or the median splat sits in a chosen slot of a chosen batch."""
import numpy as np

import scenes

TILT = 0.06      # quaternion (x, y, z) parts: a few degrees, the footprints stay axis-aligned
# Depths are 0.3 ... 1: the criterion's absolute allowance on a map's L2 error, 1e-7 per pixel, is the float32 spacing there.  Further out one
# unit in the last place of a depth (4.8e-7 at depth 4 ... 8) is beyond it, while on these nearly fronto-parallel splats the float32 oracle's own
# depth error, the other term of the bar, is a third of a unit -- the median-depth map of a 256-pixel image then misses or meets the bar by chance.


def crafted(variant, W, H, u, v, z, sx, sy, opac, seed=0, bg=(0.2, 0.4, 0.6), fx=None):
    """Axis-aligned splats that face the camera up to a small random tilt: centre at pixel (u, v), depth z, footprint sigmas (sx, sy) in pixels, opacity."""
    u, v, z, sx, sy, opac = (np.asarray(a, np.float64) for a in (u, v, z, sx, sy, opac))
    P = u.shape[0]
    sc = scenes.make_scene(variant, P, W, H, seed=seed, bg=bg, fx=fx)
    assert np.allclose(sc["viewmatrix"], np.eye(4), atol=1e-6)      # pose 0
    fx, fy = float(sc["fx"]), float(sc["fy"])
    x = z * (u - 0.5 * (W - 1)) / fx; y = z * (v - 0.5 * (H - 1)) / fy      # ndc2Pix: pixel = ndc W / 2 + (W - 1) / 2
    sc["means3D"] = np.stack([x, y, z], -1).astype(np.float32)
    s = np.stack([sx * z / fx, sy * z / fy], -1)
    if variant != "surfel":
        s = np.concatenate([s, 0.1 * s.min(axis=1, keepdims=True)], axis=1)
    sc["scales"] = s.astype(np.float32)
    # tilted: (nearly) fronto-parallel splats have depths and normals that the float32 oracle reproduces without any rounding error, and
    # the criterion's bars relative to the oracle's own error would then ask for exactness
    q = np.concatenate([np.ones((P, 1)), np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, (P, 3)) * TILT], axis=1)
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc["opacities"] = opac.astype(np.float32)[:, None]
    if variant == "plane":
        sc["all_map"] = scenes.plane_all_map(sc)
    return sc


def one_tile_list(variant, n, seed=3):
    """A 16x16 image = one tile whose list has n entries: broad, translucent splats centred inside the tile (nothing saturates, every batch is walked
    to its end by every quadrant)."""
    r = np.random.default_rng(seed)
    return crafted(variant, 16, 16, r.uniform(1, 14, n), r.uniform(1, 14, n), np.linspace(0.3, 1.0, n), r.uniform(2.5, 6.0, n), r.uniform(2.5, 6.0, n),
                   r.uniform(0.02, 0.12, n), seed=seed)


def half_and_half(variant, opaque_top=True, n_far=40, seed=5):
    """One tile.  Near the camera: opaque splats, thin in y, that cover only the top (or only the bottom) rows of every quadrant and saturate them.
    Behind them: translucent splats over the other rows only, and a few broad ones over the whole tile.  The opaque half's first row terminates
    long before the other half has met its last splat."""
    r = np.random.default_rng(seed)
    rows_op = np.array([0.0, 8.0]) if opaque_top else np.array([7.0, 15.0])        # on the first / last pixel row of the two quadrant rows: reach under 2.4 rows
    rows_tr = np.array([6.0, 14.0]) if opaque_top else np.array([2.0, 10.0])
    u, v, sx, sy, op = [], [], [], [], []
    for k in range(6):                                                               # 6 x 2 x 2 opaque splats, twelve over each quadrant row, as wide as the tile
        for yy in rows_op:
            for xx in (6.5, 8.5):
                u.append(xx + 0.2 * k - 0.5); v.append(yy); sx.append(14.0); sy.append(0.45); op.append(0.8)
    for k in range(n_far):
        yy = rows_tr[k % 2]
        u.append(r.uniform(1, 14)); v.append(yy + r.uniform(-0.3, 0.3)); sx.append(r.uniform(2, 5)); sy.append(0.5); op.append(r.uniform(0.05, 0.3))
    for k in range(6):
        u.append(r.uniform(4, 12)); v.append(r.uniform(4, 12)); sx.append(7.0); sy.append(7.0); op.append(0.1)
    n = len(u)
    return crafted(variant, 16, 16, u, v, np.linspace(0.3, 1.0, n), sx, sy, op, seed=seed)


def one_strip_each(variant, seed=7):
    """One tile: faint pin-point splats whose region {alpha >= 1/255} is under a pixel wide, one on every second pixel row and in both quadrant
    columns, so that each meets exactly one 8x2 strip (and one 8x4 half); a few broad splats behind them."""
    r = np.random.default_rng(seed)
    u, v, sx, sy, op = [], [], [], [], []
    for row in range(0, 16, 2):
        for xx in (2.0, 5.0, 10.0, 13.0):
            u.append(xx); v.append(row + 0.5); sx.append(0.15); sy.append(0.15); op.append(0.0075)      # 2 ln(255 o) = 1.3: reach 0.8 px, the strip's two rows at 0.5
    for k in range(8):
        u.append(r.uniform(3, 13)); v.append(r.uniform(3, 13)); sx.append(5.0); sy.append(5.0); op.append(0.05)      # (T stays above 0.5: no pixel sits at that gate)
    n = len(u)
    return crafted(variant, 16, 16, u, v, np.linspace(0.3, 0.8, n), sx, sy, op, seed=seed)


def median_at(variant, slot, n=130, seed=9):
    """One tile, n flat splats that cover it evenly in list order: faint ones (T stays above 0.75) except entry `slot`, which takes T from above 0.5 to
    below it on every pixel -- the median contributor is entry slot + 1 everywhere."""
    op = np.full(n, 0.0045); op[slot] = 0.85
    sg = np.full(n, 60.0)
    return crafted(variant, 16, 16, np.full(n, 7.5), np.full(n, 7.5), np.linspace(0.3, 1.0, n), sg, sg, op, seed=seed,
                   fx=400.0)      # a long lens: 60-pixel splats stay small against their depth, tilted or not
