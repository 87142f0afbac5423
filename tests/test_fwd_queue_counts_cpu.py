"""CPU: tools/fwd_queue_counts.py (pair-loop iterations of the blend forward with 1 / 2 / 4 queues per wave) against a brute-force loop over tiles, batches,
quadrants and entries on a small scene."""
import os
import sys

import numpy as np
import pytest

import oracle
import scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fwd_queue_counts as fqc  # noqa: E402


@pytest.mark.parametrize("variant,W,H", [("surfel", 64, 64), ("ewa", 56, 40)])
def test_sums_equal_a_brute_force_loop(variant, W, H):
    sc = scenes.make_scene(variant, 400, W, H, seed=4)
    with oracle.Forward(sc, variant) as f:
        got = fqc.count(f, variant, W, H)
        t = fqc.region_terms(f, variant)
        ranges = f.ranges().astype(np.int64)
        gx = (W + 15) // 16
        # the tool's restatement of the region test, at the tile's own rectangle, is tests/tile_cull.py's
        import tile_cull
        tl = tile_cull._tiles_of(ranges, f.R)
        assert np.array_equal(fqc.region_hits(t, 16.0 * (tl % gx), 16.0 * (tl // gx), 15.0, 15.0), tile_cull.region_filter64(f, variant))
        s8 = s2 = s4 = kept = batches = 0
        for tile in range(ranges.shape[0]):
            tx, ty = 16.0 * (tile % gx), 16.0 * (tile // gx)
            idx = np.arange(ranges[tile, 0], ranges[tile, 1])
            idx = idx[fqc.region_hits(t, tx, ty, 15.0, 15.0, idx)] if idx.size else idx
            kept += idx.size
            for b0 in range(0, idx.size, 64):                      # one 64-entry batch of the tile's (filtered) list
                batches += 1
                e = idx[b0:b0 + 64]
                for q in range(4):
                    qx, qy = tx + 8 * (q & 1), ty + 8 * (q >> 1)
                    if qx >= W or qy >= H:
                        continue
                    n8 = 0; nh = [0, 0]; ns = [0, 0, 0, 0]
                    for i in e:                                    # entry by entry
                        one = np.array([i])
                        n8 += int(fqc.region_hits(t, qx, qy, 7.0, 7.0, one)[0])
                        for k in range(2):
                            nh[k] += int(fqc.region_hits(t, qx, qy + 4.0 * k, 7.0, 3.0, one)[0])
                        for k in range(4):
                            ns[k] += int(fqc.region_hits(t, qx, qy + 2.0 * k, 7.0, 1.0, one)[0])
                    s8 += n8; s2 += max(nh); s4 += max(ns)
                    assert max(ns) <= max(nh) <= n8                # a rectangle's hits are hits of every rectangle around it
    assert (got["instances_region"], got["batches"]) == (kept, batches)
    assert (got["iters_8x8"], got["iters_2_halves"], got["iters_4_strips"]) == (s8, s2, s4)
    assert batches > ranges.shape[0] and s4 < s2 < s8              # lists longer than a batch; the queues do shorten the loop on this scene
    imp = fqc.implied(got, 3.0, 5.0)
    assert abs(imp["nq2"]["iteration_ratio"] - s2 / s8) < 1e-4 and imp["nq4"]["pair_loop_valu_ratio"] > imp["nq4"]["iteration_ratio"]
