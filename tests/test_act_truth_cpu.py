"""The bars of tests/act_truth.py without a device: a float32 numpy evaluation of the kernels' formulas, op by op, meets every bar on every case
of tests/test_gpu_activations.py, and three planted defects each miss one."""
import numpy as np
import pytest

import act_truth as A

CASES = [(P, S, absent) for P in A.SIZES for S in (1, 2, 3) for absent in (None,)] + [(257, 3, a) for a in ("scaling", "rotation", "opacity")]


@pytest.mark.parametrize("P,S,absent", CASES)
def test_float32_evaluation_meets_every_bar(P, S, absent):
    c = A.make_case(P, S, seed=100 * P + S, absent=absent)
    worst = A.check(c, A.eval_f32(c))
    print(P, S, absent, {k: round(v, 3) for k, v in worst.items()})
    if absent is not None:
        assert not A.eval_f32(c)["d_" + absent].any()


def test_cases_hold_what_they_claim():
    c = A.make_case(4099, 3, seed=7)
    tr, clamped, fragile, _ = A.truth(c)
    n = A.norm_f32(c["q"])
    assert 1 <= int(fragile.sum()) <= 4 and int(clamped.sum()) >= 3                         # the clamp from both sides, the zero quaternion
    assert (n == A.EPS).any() and (n == np.nextafter(A.EPS, np.float32(0))).any() and (n == np.nextafter(A.EPS, np.float32(1))).any() and (n == 0).any()
    assert n.max() > 5e17 and 0 < n[n > 0].min() < 2e-18
    assert set(A.SCALING_SPECIAL) <= set(c["s"].reshape(-1).tolist()) and {np.float32(v) for v in A.OPACITY_SPECIAL} <= set(c["o"].reshape(-1).tolist())
    e = A.eval_f32(c)["scaling"]
    assert np.isinf(e[c["s"] == 89.0]).all() and (e[c["s"] == -104.0] == 0).all() and np.isfinite(e[c["s"] == 88.0]).all()
    rr = tr["rotation"][0][-1]                                                                # the parallel upstream gradient: the projection cancels
    assert np.abs(tr["d_rotation"][0][-1]).max() < 1e-6 * np.abs(c["g"]["rotation"][-1]).max() / n[-1] and np.abs(rr).max() > 0
    seeds = {tuple(A.make_case(1, 3, seed=s)["o"].reshape(-1).tolist()) for s in range(7)}    # P = 1 sees another special row per seed
    assert len(seeds) == 7


@pytest.mark.parametrize("defect,output", [("no_projection", "d_rotation"), ("clamp_1e-6", "rotation"), ("a_not_a(1-a)", "d_opacity")])
def test_planted_defects_miss_a_bar(defect, output):
    c = A.make_case(4099, 3, seed=7)
    worst = A.check(c, A.eval_f32(c, defect=defect), raise_on_miss=False)
    print(defect, {k: round(v, 3) for k, v in worst.items()})
    assert worst[output] > 1.0
    assert all(v <= 1.0 for k, v in worst.items() if k not in (output, "d_rotation" if defect == "clamp_1e-6" else output))
