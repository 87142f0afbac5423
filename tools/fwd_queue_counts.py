"""How many pair-loop iterations the blend forward would run with NQ sub-tile queues per wave, counted on the CPU.

    python tools/fwd_queue_counts.py [--variant surfel] [--P 300000] [--W 1920] [--H 1080] [--seed 0] [--out profiles/fwd_queue_counts.json]
                                     [--vadd2 3] [--vadd4 N]

k_blend_fwd<V> consumes a tile's list 64 entries at a time; a wave owns an 8x8 quadrant and runs one pair-loop iteration per entry of the batch whose
region {alpha >= 1/255 possible} meets the quadrant.  With NQ queues (two 8x4 halves: the wave's two 32-lane halves, or four 8x2 strips: its four
16-lane rows) it runs max over the queues of the entries that meet the queue's rectangle.  This tool counts, from the CPU oracle's tile lists and
the float64 region test of tests/tile_cull.py restated for a rectangle with separate x and y extents,

    sum over (tile, batch, quadrant) of  |8x8 hits|,  max over the two halves,  max over the four strips

(no early exit: a wave that saturates stops sooner in all three forms), and the change in pair-loop VALU instructions these imply.  (Two and four
queues were built and measured from these counts, EXPERIMENTS.md (93); the kernel keeps one.)  The lists are the
oracle's restricted to the instances whose region meets the tile (the exact region filter; the library's list is that plus a safety margin).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "gs-sr_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PAIR_VALU = 52.5        # VALU per pair-loop iteration of k_blend_fwd<SURFEL> at NQ = 1 (50-55: 28 to the gate, 21 in the accumulation block, the median bookkeeping)
LOOP_SHARE = 0.78       # share of the kernel's VALU instructions that the pair loop issues


def rect_min_conic(A, B, C, X0, Y0, ex, ey):
    """min over [X0, X0+ex] x [Y0, Y0+ey] of A x^2 + 2 B x y + C y^2 (tile_cull._rect_min_conic with separate extents), vectorised float64."""
    X1, Y1 = X0 + ex, Y0 + ey
    inside = (X0 <= 0) & (X1 >= 0) & (Y0 <= 0) & (Y1 >= 0)
    q = np.full(np.shape(A), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for X in (X0, X1):
            y = np.clip(-B * X / C, Y0, Y1)
            q = np.minimum(q, A * X * X + 2 * B * X * y + C * y * y)
        for Y in (Y0, Y1):
            x = np.clip(-B * Y / A, X0, X1)
            q = np.minimum(q, A * x * x + 2 * B * x * Y + C * Y * Y)
    return np.where(inside, 0.0, q)


def region_terms(f, variant):
    """Per instance of the oracle's list: what tile_cull.region_filter64 derives from the per-gaussian state, before any rectangle enters."""
    import tile_cull
    g = f.geom()
    lst = f.point_list().astype(np.int64)
    tile = tile_cull._tiles_of(f.ranges(), f.R)
    co = g["conic_opacity"].astype(np.float64)[lst]
    m2 = g["means2D"].astype(np.float64)[lst]
    opa = co[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = 2.0 * np.log(255.0 * opa)
    t = dict(tile=tile, can=255.0 * opa > 1.0, tt=tt, mx=m2[:, 0], my=m2[:, 1], surfel=variant in ("surfel", 1))
    if not t["surfel"]:
        t.update(A=co[:, 0], B=co[:, 1], C=co[:, 2], cx=m2[:, 0], cy=m2[:, 1], lim=tt,
                 proper=(co[:, 0] > 0) & (co[:, 2] > 0) & (co[:, 0] * co[:, 2] - co[:, 1] ** 2 > 0))
        return t
    Tm = g["cov"].astype(np.float64)[lst]
    Tu, Tv, Tw = Tm[:, 0:3], Tm[:, 3:6], Tm[:, 6:9]
    t3 = np.stack([tt, tt, -np.ones_like(tt)], axis=1)
    qd = lambda X, Y: (t3 * X * Y).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = qd(Tw, Tw)
        cx, cy = qd(Tu, Tw) / w, qd(Tv, Tw) / w
        sxx = cx * cx - qd(Tu, Tu) / w; syy = cy * cy - qd(Tv, Tv) / w; sxy = cx * cy - qd(Tu, Tv) / w
        det = sxx * syy - sxy * sxy
        A, B, C = syy / det, -sxy / det, sxx / det
    t.update(A=A, B=B, C=C, cx=cx, cy=cy, lim=np.ones_like(tt),
             proper=(w < 0) & (Tw[:, 2] > 0) & (sxx > 0) & (syy > 0) & (det > 0))
    return t


def region_hits(t, x0, y0, ex, ey, sel=slice(None)):
    """bool per selected instance: the region meets the rectangle of pixel centres [x0, x0+ex] x [y0, y0+ey] (region_filter64's decision, any rectangle)."""
    g = lambda k: t[k][sel]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = rect_min_conic(g("A"), g("B"), g("C"), x0 - g("cx"), y0 - g("cy"), ex, ey)
    if not t["surfel"]:
        return g("can") & (~g("proper") | ~(q > g("lim")))
    e0x, e0y = x0 - g("mx"), y0 - g("my")
    ddx = np.maximum(np.maximum(e0x, -(e0x + ex)), 0.0); ddy = np.maximum(np.maximum(e0y, -(e0y + ey)), 0.0)
    disc = 2.0 * (ddx * ddx + ddy * ddy) <= g("tt")
    return g("can") & (disc | ~(g("proper") & np.isfinite(q)) | ~(q > 1.0))


def count(f, variant, W, H):
    """-> dict of the three sums over (tile, 64-entry batch, quadrant) and the bookkeeping around them."""
    t = region_terms(f, variant)
    tile = t["tile"]
    gx = (W + 15) // 16
    tx0 = (tile % gx).astype(np.float64) * 16.0; ty0 = (tile // gx).astype(np.float64) * 16.0
    keep = region_hits(t, tx0, ty0, 15.0, 15.0)                       # the tile's filtered list
    idx = np.flatnonzero(keep)
    tl = tile[idx]
    T = int(f.T)
    cnt = np.bincount(tl, minlength=T)
    start = np.cumsum(cnt) - cnt
    rank = np.arange(idx.shape[0], dtype=np.int64) - start[tl]
    nb = (cnt + 63) // 64
    bstart = np.cumsum(nb) - nb
    batch = bstart[tl] + rank // 64                                   # global batch number, ascending
    NB = int(nb.sum())
    s8 = s2 = s4 = 0
    pairs_w = 0
    for q in range(4):
        qx = tx0[idx] + 8.0 * (q & 1); qy = ty0[idx] + 8.0 * (q >> 1)
        on = (qx < W) & (qy < H)                                      # a quadrant outside the image has no wave
        h8 = on & region_hits(t, qx, qy, 7.0, 7.0, idx)
        s8 += int(h8.sum())
        halves = [np.bincount(batch, weights=(on & region_hits(t, qx, qy + 4.0 * k, 7.0, 3.0, idx)), minlength=NB) for k in range(2)]
        s2 += int(np.maximum(halves[0], halves[1]).sum())
        strips = [np.bincount(batch, weights=(on & region_hits(t, qx, qy + 2.0 * k, 7.0, 1.0, idx)), minlength=NB) for k in range(4)]
        s4 += int(np.maximum(np.maximum(strips[0], strips[1]), np.maximum(strips[2], strips[3])).sum())
        pairs_w += int(on.sum())
    return dict(instances_oracle=int(f.R), instances_region=int(idx.shape[0]), batches=NB, wave_pairs_tested=pairs_w,
                iters_8x8=s8, iters_2_halves=s2, iters_4_strips=s4)


def implied(c, vadd2, vadd4):
    out = {}
    for name, key, add in (("nq2", "iters_2_halves", vadd2), ("nq4", "iters_4_strips", vadd4)):
        if add is None:
            continue
        r = c[key] / max(c["iters_8x8"], 1)
        loop = r * (PAIR_VALU + add) / PAIR_VALU
        out[name] = dict(iteration_ratio=round(r, 4), valu_added_per_iteration=add, pair_loop_valu_ratio=round(loop, 4),
                         kernel_valu_ratio=round(1.0 - LOOP_SHARE * (1.0 - loop), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="surfel"); ap.add_argument("--P", type=int, default=300000)
    ap.add_argument("--W", type=int, default=1920); ap.add_argument("--H", type=int, default=1080); ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--vadd2", type=float, default=3.0, help="VALU added per iteration at NQ = 2")
    ap.add_argument("--vadd4", type=float, default=None, help="VALU added per iteration at NQ = 4 (from the listing of the build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_queue_counts.json"))
    a = ap.parse_args()
    import oracle
    from gsrast import workloads
    sc = workloads.make_scene(a.variant, a.P, a.W, a.H, seed=a.seed)
    with oracle.Forward(sc, a.variant) as f:
        c = count(f, a.variant, a.W, a.H)
        evaluated, contributing = f.pair_counts()
    res = dict(scene=dict(variant=a.variant, P=a.P, W=a.W, H=a.H, seed=a.seed), tiles_counted="all", early_exit="not modelled (all three sums)",
               pair_valu_nq1=PAIR_VALU, pair_loop_share_of_kernel_valu=LOOP_SHARE, contributing_pairs=contributing,
               lane_use=dict(nq1=round(contributing / (64.0 * max(c["iters_8x8"], 1)), 4), nq2=round(contributing / (64.0 * max(c["iters_2_halves"], 1)), 4),
                             nq4=round(contributing / (64.0 * max(c["iters_4_strips"], 1)), 4)),
               **c, implied=implied(c, a.vadd2, a.vadd4))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
