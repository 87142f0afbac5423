"""GPU: distCUDA2 (csrc/gsr_extra.hip gsr_dist2: Morton order, 256-point boxes, box-pruned exact search) at the sizes and clouds where its pieces
change behaviour: fewer than three neighbours (the bests stay at FLT_MAX), one point more or less than a box, a cloud without extent in one, two or all
three axes (hi == lo in the Morton quantiser), duplicates, and tight pairs whose third neighbour lies in another box.

Reference: tests/glue_truth.dist2_bruteforce (float32 all-pairs, pinned to the C oracle bit for bit by tests/test_glue_truth_cpu.py).  The pruning is
conservative by design, so equality is exact, non-finite values included."""
import numpy as np
import pytest
import torch

import glue_cases
import glue_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = glue_cases.knn_inputs()


def _dist(points_tensor):
    from simple_knn._C import distCUDA2
    return distCUDA2(points_tensor).cpu().numpy()


@pytest.mark.parametrize("name", list(INPUTS))
def test_exactly_the_all_pairs_result(name):
    pts = INPUTS[name]
    ref = glue_truth.dist2_bruteforce(pts)
    got = _dist(torch.from_numpy(pts).to(DEV))
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0]
    assert bad.size == 0 and np.array_equal(got, ref), (name, bad[:8], got[bad[:8]], ref[bad[:8]])


def test_fewer_than_three_neighbours_on_the_device():
    """What the reference's kernel gives too: FLT_MAX stays in the sum.  P = 1, 2: inf; P = 3: ~1.134e38, finite."""
    assert np.array_equal(_dist(torch.from_numpy(INPUTS["P1"]).to(DEV)), [np.inf])
    assert np.array_equal(_dist(torch.from_numpy(INPUTS["P2"]).to(DEV)), [np.inf, np.inf])
    d3 = _dist(torch.from_numpy(INPUTS["P3"]).to(DEV))
    assert np.isfinite(d3).all() and np.allclose(d3, 1.134e38, rtol=1e-3)


def test_third_neighbour_in_another_box():
    """The structure of the `clusters` input, restated here because the case means nothing without it: under the Morton order (the code and a stable
    sort, glue_cases.morton_boxes) each pair point's third neighbour (float64) lies outside the point's own 256-box -- and the device finds it."""
    pts = INPUTS["clusters"]
    box, _ = glue_cases.morton_boxes(pts)
    idx, d2 = glue_truth.dist2_neighbours64(pts)
    assert all(box[idx[i, 2]] != box[i] for i in range(4)) and all(idx[i, 0] == (i ^ 1) for i in range(4))
    got = _dist(torch.from_numpy(pts).to(DEV))
    assert np.array_equal(got[:4], glue_truth.dist2_bruteforce(pts)[:4])
    np.testing.assert_allclose(got[:4], d2[:4].mean(axis=1), rtol=1e-5)


@pytest.mark.parametrize("name", ["P5", "P257", "P1025", "dup300x2"])
def test_input_layout(name):
    """A (P,3) view one float into its storage and a non-contiguous points[:, :3] of a (P,4) tensor give what the contiguous copy gives."""
    pts = INPUTS[name]
    P = pts.shape[0]
    ref = _dist(torch.from_numpy(pts).to(DEV))
    buf = torch.empty(3 * P + 1, device=DEV)
    view = buf[1:].view(P, 3)
    view.copy_(torch.from_numpy(pts))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert np.array_equal(_dist(view), ref)
    wide = torch.full((P, 4), 1e30, device=DEV)
    wide[:, :3] = torch.from_numpy(pts).to(DEV)
    assert not wide[:, :3].is_contiguous()
    assert np.array_equal(_dist(wide[:, :3]), ref)
    assert np.array_equal(ref, glue_truth.dist2_bruteforce(pts))
