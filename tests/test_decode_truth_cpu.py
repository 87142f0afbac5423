"""The decode edge matrix (decode_truth.MATRIX) is well posed, and the float32 C oracle holds against the float64 truth at every shape of it."""
import numpy as np
import pytest

import decode_cases
import decode_truth
import oracle_decode


def test_matrix_covers_the_edges():
    ids = decode_truth.MATRIX_IDS
    assert len(ids) == len(set(ids)) == 14 + 16 + 6 + 16
    assert [m[2] for m in decode_truth.MATRIX] == list(range(101, 153))
    for entry in decode_truth.MATRIX:
        case = decode_truth.matrix_case(entry)
        vis = case["vis_idx"]
        assert vis.size == entry[1] and np.all(np.diff(vis) > 0) and vis.dtype == np.int32
        assert vis.size < case["anchor"].shape[0] <= vis.size + 5          # some anchor is always invisible


def test_matrix_is_well_posed_for_the_gate_tolerance():
    """gate_check lets a gate differ only on a near-zero float64 opacity and only as often as such entries exist.  That hides nothing as long as such
    entries are rare: at most 2 per case, none in a case with fewer than 3000 opacity entries."""
    total = near_total = 0
    smallest = np.inf
    for entry in decode_truth.MATRIX:
        case = decode_truth.matrix_case(entry)
        nop = decode_truth.truth(case, None)[0]["neural_opacity"]
        near = int(decode_truth.near_zero(nop).sum())
        live = np.abs(nop)[nop != 0.0]                                      # opacity_scale never is 0 in the matrix; exact zeros would be exact on both sides
        total += nop.size; near_total += near; smallest = min(smallest, float(live.min()))
        assert near <= 2, (entry[0], near)
        assert near == 0 or nop.size >= 3000, (entry[0], near, nop.size)
        assert 0 < int((nop > 0).sum()) < nop.size or nop.size < 20, entry[0]   # the gate is mixed in every case that is not tiny
    print(f"near-zero entries {near_total} of {total}, smallest |nop| {smallest:.2e}")
    assert near_total <= 10


@pytest.mark.parametrize("entry", decode_truth.MATRIX, ids=decode_truth.MATRIX_IDS)
def test_oracle_matches_truth_over_the_matrix(entry):
    """oracle/gsd_oracle.c (float32, the reference of the other GPU decode tests) against the float64 chain evaluated with the oracle's own gate."""
    case = decode_truth.matrix_case(entry)
    o = oracle_decode.forward(case)
    mask = o["mask"].astype(bool)
    decode_truth.gate_check(mask, decode_truth.truth(case, None)[0]["neural_opacity"])
    assert o["P"] == int(mask.sum())
    dL = decode_cases.make_out_grads(o["P"], seed=entry[2])
    decode_truth.compare("oracle " + entry[0], o, oracle_decode.backward(case, mask, dL), case, mask, dL)


def test_special_cases_are_what_they_claim():
    """all gates closed / open with a clear margin, and the float64 chain of the closed case returns exact zero gradients; the `holes` case leaves 133
    of its 333 visible anchors (two whole 16-row tiles among them) without a row."""
    for name, want in (("closed", False), ("open", True)):
        case = decode_truth.special_case(name)
        nop = decode_truth.truth(case, None)[0]["neural_opacity"]
        assert np.all((nop > 0) == want) and np.abs(nop).min() > 0.5, (name, np.abs(nop).min())
    case = decode_truth.special_case("closed")
    out, g = decode_truth.truth(case, None, decode_cases.make_out_grads(0))
    assert out["xyz"].shape == (0, 3) and set(g) >= {"anchor", "feat", "offset", "scaling", "W1o", "W2c", "b2k", "app"}
    assert all(v.shape == np.shape(case.get(n, case["params"].get(n))) and not np.any(v) for n, v in g.items())
    case = decode_truth.special_case("holes")
    nop = decode_truth.truth(case, None)[0]["neural_opacity"].reshape(333, -1)
    empty = ~(nop > 0).any(axis=1)
    assert empty[16:48].all() and empty[::3].all() and 133 <= int(empty.sum()) <= 135      # 133 by construction; an anchor may close all its gates by itself
    assert decode_truth.near_zero(nop[nop != 0.0]).sum() == 0
    case = decode_truth.camera_centre_case()
    assert 0 not in case["vis_idx"] and np.array_equal(case["anchor"][0], case["campos"]) and case["vis_idx"].size == 17


def test_large_case_is_beyond_every_cap_and_clear_of_the_relu_kink():
    case = decode_truth.large_case()
    Nv = case["vis_idx"].size
    assert Nv >= 270000 and (Nv + 1023) // 1024 > 64 + 1 and (Nv + 255) // 256 > 1024 and np.all(np.diff(case["vis_idx"]) > 0)
    assert decode_truth.hidden_margin(case).min() >= decode_truth.RELU_EPS
    full = decode_cases.make_case(Na=380000, seed=401, vis_frac=0.72)["vis_idx"].size
    assert 0 < full - Nv < 0.005 * full                                          # a few anchors in a thousand are left out, nothing more


def test_gate_check_bites():
    nop = np.array([0.5, -0.5, 3e-6, -2e-6, 0.2])
    assert decode_truth.gate_check(nop > 0, nop) == 0
    assert decode_truth.gate_check(np.array([1, 0, 0, 1, 1]), nop) == 2          # both near-zero gates flipped: allowed
    with pytest.raises(AssertionError):
        decode_truth.gate_check(np.array([1, 1, 1, 0, 1]), nop)                  # a clear gate flipped
    with pytest.raises(AssertionError):
        decode_truth.gate_check(np.array([1, 0, 1, 0]), nop)


def test_training_statis64_matches_the_c_oracle():
    case = decode_truth.edge_case(257, 77)
    o = oracle_decode.forward(case)
    k, Na = case["k"], case["anchor"].shape[0]
    r = np.random.default_rng(5)
    grad = r.normal(0, 1, (o["P"], 3)).astype(np.float32); upd = r.uniform(size=o["P"]) < 0.6
    acc32 = [r.uniform(0, 2, n).astype(np.float32) for n in (Na, Na, Na * k, Na * k)]
    acc64 = [a.astype(np.float64) for a in acc32]
    oracle_decode.training_stats(case["vis_idx"], k, o["neural_opacity"], o["mask"], upd, grad, *acc32)
    decode_truth.training_statis64(acc64, k, case["vis_idx"], o["neural_opacity"], o["mask"], upd, grad)
    for a, b in zip(acc32, acc64):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=0)
