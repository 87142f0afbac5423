"""GPU: the batch queue of the blend forward (gs-sr_amd/csrc/gsr_blend.hip k_blend_fwd<V>) and the per-batch lookup of "which splat", at their edges.

A wave owns an 8x8 quadrant and walks, per 64-entry batch of the tile's list, the queue of the entries that can reach it; inside the loop a lane keeps
only the slot it blended last and the slot it blended last at T > 0.5, and the list positions, the median splat's id and its normal are resolved from
the staged batch after the batch's loop.  The scenes also cover what sub-quadrant queues (EXPERIMENTS.md (93): built, measured, not kept) would have to
get right: halves and strips of a quadrant outside the image, one half of a quadrant saturated long before the other, regions that meet one 8x2 strip.
Every case is held to the float64 truth with the criterion of tests/parity_truth.py (forward maps and indices on robust pixels, gradients through the
backward that reads the forward's per-(batch, quadrant) word), the HIP tile-instance list against the oracle's included; a second forward of the
same inputs must reproduce the first bit for bit (the forward has no floating-point atomics).  Scenes: tests/fwd_queue_scenes.py."""
import numpy as np
import pytest

import fwd_queue_scenes as fq
import scenes
from test_gpu_parity import _check_against_truth, _hiprun

pytestmark = pytest.mark.gpu

VARIANTS = ["surfel", "ewa", "plane"]
FWD_KEYS = {"surfel": ("color", "others", "final_T", "n_contrib", "radii"), "ewa": ("color", "final_T", "n_contrib", "radii"),
            "plane": ("color", "all_map", "plane_depth", "observe", "final_T", "n_contrib", "radii")}


def _truth_and_repeat(variant, sc, seed=1):
    """-> (report, raw forward state).  The float64-truth criterion, forward and backward; then a second forward, equal to the first."""
    hr = _hiprun()
    og = scenes.random_out_grads(variant, sc["W"], sc["H"], seed=seed, scale=1.0)
    rep = _check_against_truth(hr, variant, "precomp", sc, og)
    a, b = hr.run_raw(variant, sc), hr.run_raw(variant, sc)
    for k in FWD_KEYS[variant]:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{k}: two forwards of the same scene differ"
    return rep, a


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,H,P", [(37, 21, 300), (24, 12, 150)])
def test_quadrants_halves_and_strips_partly_outside_the_image(variant, W, H, P):
    """37x21: the last quadrant column holds 5 of its 8 pixel columns, the last quadrant row 5 of its 8 rows (a half inside, a half with one row, a strip
    with one row, a strip outside).  24x12: a whole quadrant column outside, the lower quadrants keep their top half only."""
    rep, st = _truth_and_repeat(variant, scenes.make_scene(variant, P, W, H, seed=21, bg=(0.2, 0.4, 0.6)))
    assert st["color"].shape == (3, H, W) and np.isfinite(st["color"]).all()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_list_lengths_at_the_batch_edges(variant, n):
    """One tile whose list has 63 / 64 / 65 / 129 entries, none of them saturating: every quadrant walks every batch to its end."""
    rep, st = _truth_and_repeat(variant, fq.one_tile_list(variant, n))
    assert int(st["R"]) == n and st["ranges"].astype(np.int64).tolist() == [[0, n]]
    assert int(st["n_contrib"][0].max()) == n                      # some pixel blends the list's last entry: the last (partial) batch was walked


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("opaque_top", [True, False])
def test_one_half_saturates_while_the_other_goes_on(variant, opaque_top):
    """Opaque splats over the top rows of every quadrant only (they saturate the first row), translucent ones behind them over the bottom rows only --
    and the mirror image: part of a wave's pixels terminate early in the first batch while the rest blend into the second."""
    rep, st = _truth_and_repeat(variant, fq.half_and_half(variant, opaque_top))
    nc = st["n_contrib"][0].astype(np.int64)
    sat, far = (0, 6) if opaque_top else (7, 1)
    assert (nc[sat, 5:11] < 30).all() and (nc[sat + 8, 5:11] < 30).all()      # the saturated row (its middle: the ends see less) stopped inside the opaque splats ...
    assert (nc[far] > 40).all() and (nc[far + 8] > 40).all()        # ... while the other half went on to the end of the list


@pytest.mark.parametrize("variant", VARIANTS)
def test_regions_that_meet_exactly_one_strip(variant):
    rep, st = _truth_and_repeat(variant, fq.one_strip_each(variant))
    assert int(st["R"]) == 40


@pytest.mark.parametrize("slot", [0, 63, 64, 100])
def test_median_in_the_first_and_last_slot_of_a_batch_and_in_the_second_batch(slot):
    """The median splat (last contributor met at T > 0.5) is entry `slot` of a 130-entry list on every pixel: its position, its id and its normal are
    looked up after the batch's pair loop, from the slot the loop kept."""
    variant = "surfel"
    sc = fq.median_at(variant, slot)
    rep, st = _truth_and_repeat(variant, sc)
    assert (st["n_contrib"][1] == slot + 1).all()                   # 1-based position in the tile's list
    assert (st["others"][7] == float(slot)).all()                   # the gaussian's id (list order = depth order = id order here)
    nrm = st["others"][8:11].reshape(3, -1)
    assert (nrm == nrm[:, :1]).all() and abs(float(np.linalg.norm(nrm[:, 0])) - 1.0) < 1e-5      # its normal: one splat's, copied to every pixel
    assert (st["n_contrib"][0] == 130).all()
