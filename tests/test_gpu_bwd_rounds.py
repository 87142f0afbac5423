"""GPU: the staging loop of the splat-parallel blend backward (gs-sr_amd/csrc/gsr_blend_sp.hip k_blend_bwd_sp<V>) at its edges.

The kernel consumes a tile's list from its deep end in chunks of SP_CH entries, trims a chunk to the suffix that fits every wave's SP_CAP_*-row table
(inside a 64-entry group or at a group's edge, the deepest cut of the four waves holds), gates entries per wave, per 4x4 block and per tile by the
deepest contributor, and hands each pixel's (T, S) carry from load to load, round to round and chunk to chunk.  The scenes of
tests/bwd_round_scenes.py sit on both sides of each of these edges; tests/test_bwd_rounds_cpu.py asserts, on a model of the loop held to the source,
that they do, and that one mishandled (entry, quadrant) or (entry, 4x4 block) pair at a round boundary trips the criterion used here.  Every case is
held to the float64 truth with the bars of tests/parity_truth.py -- the whole tensors and, as a row group of their own, the entries at the round
boundaries -- and the forward's integer state must be the one the model was run with."""
import numpy as np
import pytest

import bwd_round_scenes as br
import oracle
import scenes
from test_gpu_parity import _check_against_truth, _hiprun

pytestmark = pytest.mark.gpu

SEED = 1


def _run(variant, sc, m, og=None, label=""):
    """The criterion, whole tensors and round-edge rows, and the assertions that tie the run to the model's schedule.  -> the report."""
    hr = _hiprun()
    W, H = int(sc["W"]), int(sc["H"])
    if og is None:
        og = scenes.random_out_grads(variant, W, H, SEED, scale=1.0)
    rep = _check_against_truth(hr, variant, "precomp", sc, og, row_groups={"round edges": br.edge_rows(m)})
    st = hr.run_raw(variant, sc)
    # the HIP forward kept every instance: list positions are the model's positions
    assert int(st["R"]) == m["R"] and np.array_equal(st["ranges"].astype(np.int64), m["ranges"]) and np.array_equal(st["point_list"].astype(np.int64), m["point_list"])
    nc = st["n_contrib"][0].astype(np.int64)
    gx = (W + 15) // 16
    for t in m["tiles"]:
        tx, ty = 16 * (t["tile"] % gx), 16 * (t["tile"] // gx)
        got = []
        for q in range(4):
            blk = nc[ty + 8 * (q >> 1):ty + 8 * (q >> 1) + 8, tx + 8 * (q & 1):tx + 8 * (q & 1) + 8]
            got.append(int(blk.max()) if blk.size else 0)
        assert got == t["wmax"], (got, t["wmax"])                   # the per-wave gates the model was run with
    g = rep["hip_grads"]
    for k, v in g.items():
        if v is not None:
            assert np.isfinite(v).all(), k
    with oracle.Forward(sc, variant) as f:
        contributes = np.abs(f.backward(**og)["dL_dopacity"]).reshape(m["P"], -1).max(axis=1) > 0
    lost = contributes & ~(np.abs(g["dL_dopacities"]).reshape(m["P"], -1).max(axis=1) > 0)
    assert contributes.sum() >= max(t["tile_max"] for t in m["tiles"]) // 2 and not lost.any(), f"entries {np.flatnonzero(lost)[:8]} received nothing"
    grp = rep["groups"]["round edges"]
    worst = max(((r["rel_l2"] / max(1e-3, 2.0 * r["oracle_rel_l2"]), k, r["rel_l2"], max(1e-3, 2.0 * r["oracle_rel_l2"])) for k, r in grp.items() if isinstance(r, dict)))
    print(f"{label} {variant}: {grp['rows']} round-edge rows; in-group relative L2 vs truth, worst tensor {worst[1]}: {worst[2]:.2e} (bar {worst[3]:.1e}); "
          f"robust pixels {rep['robust_pixel_fraction']:.3f}")
    return rep


@pytest.mark.parametrize("name,variant", br.CASE_IDS)
def test_round_edges_against_the_float64_truth(name, variant):
    sc, m = br.case(name, variant)
    _run(variant, sc, m, label=name)


@pytest.mark.parametrize("mn_pass", [True, False])
@pytest.mark.parametrize("name", ["cap_plus_1", "one_dense_quadrant", "chunk_257"])
def test_surfel_median_normal_pass_on_and_off_in_a_multi_round_list(name, mn_pass):
    """The median-normal pass of a load runs only when some pixel of the wave has a gradient on the median-normal channels; 2DGS training sends none.
    random_out_grads always does: the second run zeroes the three channels, and the pass is skipped in every round."""
    variant = "surfel"
    sc, m = br.case(name, variant)
    og = scenes.random_out_grads(variant, int(sc["W"]), int(sc["H"]), SEED, scale=1.0)
    assert np.abs(og["dL_dothers"][8:11]).min() > 0
    if not mn_pass:
        og["dL_dothers"][8:11] = 0.0
    _run(variant, sc, m, og=og, label=f"{name} mn_pass={mn_pass}")


@pytest.mark.parametrize("variant", br.VARIANTS)
def test_ballots_left_by_an_earlier_scene_stay_behind_the_wave_gate(variant):
    """chunk_edge_and_trim first: every bit of every ballot word is set.  Then, in the same process, quadrants_end_early: the right quadrants' forward
    waves stop testing batches once they are saturated, and the words behind their last batch are whatever the earlier forward left; only the
    `cbase + e < wmax` gate keeps those entries out of the right waves' tables."""
    hr = _hiprun()
    sc0, m0 = br.case("chunk_edge_and_trim", variant)
    assert all(t["hits"].all() for t in m0["tiles"])
    res = hr.run(variant, sc0, scenes.random_out_grads(variant, int(sc0["W"]), int(sc0["H"]), SEED, scale=1.0))
    assert np.isfinite(res["grads"]["dL_dopacities"]).all()
    sc, m = br.case("quadrants_end_early", variant)
    t = m["tiles"][0]
    assert max(t["wmax"][1], t["wmax"][3]) <= 128 < t["list"].shape[0] - 64      # batches the right waves never tested
    _run(variant, sc, m, label="quadrants_end_early after chunk_edge_and_trim")
