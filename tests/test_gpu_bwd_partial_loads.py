"""GPU: the 16-entry loads of the splat-parallel blend backward (csrc/gsr_blend_sp.hip) with empty lanes.

A row of 16 lanes holds 16 entries of one 4x4 block's queue; the last load of a queue of n entries leaves 16 - n % 16 lanes empty.  Those lanes fetch
the library's all-zero record through one pointer select; they must contribute nothing and poison nothing (their u enters the row scan as 0 * u).
n small splats at distinct depths are centred in one 4x4 block of a 32x32 image (four tiles), n on both sides of one, two and three loads; a
second layout puts half of them on the line between two blocks of a quadrant, so that two rows of a wave carry queues of different lengths.  Everything
is compared with the float64 truth exactly as the small truth cases of tests/test_gpu_parity.py are (tests/parity_truth.py run_oracles + check_case),
and no gradient may hold a NaN or an inf."""

import numpy as np
import pytest

import scenes
from test_gpu_parity import _check_against_truth, _hiprun

pytestmark = pytest.mark.gpu

W = H = 32
COUNTS = [1, 15, 16, 17, 31, 32, 33, 48]


def block_scene(variant, n, layout, seed=0):
    """n splats of ~1 px sigma, depths 2.0, 2.1, ... (distinct), opacities low enough that the last one still contributes (no early termination).
    layout "block": all centred on (9.5, 9.5), the middle of the 4x4 block with origin (8, 8); "straddle": every second one on (11.5, 9.5), the line
    between that block and its neighbour (12, 8) in the same 8x8 quadrant."""
    sc = scenes.make_scene(variant, n, W, H, seed=seed, bg=(0.2, 0.4, 0.6))
    rng = np.random.default_rng(100 + seed)
    fx = W * (1600.0 / 1920.0)
    z = 2.0 + 0.1 * np.arange(n)
    cx = np.full(n, 9.5); cy = np.full(n, 9.5)
    if layout == "straddle":
        cx[1::2] = 11.5
    cx = cx + rng.uniform(-0.3, 0.3, n); cy = cy + rng.uniform(-0.3, 0.3, n)
    # pixel centre p <-> ndc (2 p + 1) / W - 1 (auxiliary.h ndc2Pix); pose 0: world space is camera space
    x = ((2.0 * cx + 1.0) / W - 1.0) * sc["tanfovx"] * z
    y = ((2.0 * cy + 1.0) / H - 1.0) * sc["tanfovy"] * z
    sc["means3D"] = np.stack([x, y, z], -1).astype(np.float32)
    nax = 2 if variant == "surfel" else 3
    s = (rng.uniform(0.9, 1.3, (n, 1)) * z[:, None] / fx) * rng.uniform(0.7, 1.0, (n, nax))
    if variant == "plane":
        s[:, 2] *= 0.1
    sc["scales"] = s.astype(np.float32)
    q = np.concatenate([np.ones((n, 1)), rng.uniform(-0.15, 0.15, (n, 3))], 1)      # facing the camera, tilted a little
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc["opacities"] = rng.uniform(0.03, 0.08, (n, 1)).astype(np.float32)
    sc["colors_precomp"] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    if variant == "plane":
        sc["all_map"] = scenes.plane_all_map(sc)
    return sc


@pytest.mark.parametrize("layout", ["block", "straddle"])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("variant", ["ewa", "surfel", "plane"])
def test_partial_loads_against_the_float64_truth(variant, n, layout):
    hr = _hiprun()
    sc = block_scene(variant, n, layout)
    og = scenes.random_out_grads(variant, W, H, seed=n, scale=1.0)
    if variant == "surfel":
        og["dL_dothers"][8:11] = 0.25 * og["dL_dothers"][8:11]      # the median-normal pass of a load runs too
    rep = _check_against_truth(hr, variant, "precomp", sc, og)
    st = hr.run_raw(variant, sc)
    # every splat reaches the block's tile, and the deepest pixel list of the image has all n entries: the block's queue takes ceil(n / 16) loads
    assert (st["radii"] > 0).all()
    assert int(st["n_contrib"][0].max()) == n, (int(st["n_contrib"][0].max()), n)
    for k, v in rep["hip_grads"].items():
        if v is not None:
            assert np.isfinite(v).all(), k
            print(variant, n, layout, k, float(np.abs(v).max()))
    assert all(np.abs(rep["hip_grads"][k]).max() > 0 for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacities", "dL_dcolors_precomp"))
