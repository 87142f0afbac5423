"""tests/visible_truth.py (the float64 statement of the LOD mask and the visibility prefilter) held to the float32 CPU oracles, to the torch
restatement of the reference's level formula, to hand-written answers at the planted gate rows and to its own conditions; and its checkers shown
to trip on planted defects.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import oracle
import oracle_decode
import ref_anchor_octree_torch as R
import visible_cases as VC
import visible_truth as VT

MODS = (1.0, 0.7)


@functools.lru_cache(maxsize=None)
def oracle_filter(name, mod, precomp, fma=False):
    """-> (radii, terms, cov3D | None) of the float32 oracle (or its FMA twin) on a case"""
    case = VC.make(name)
    cov = oracle.cov3d(case["scales6"], mod, case["rotations"]) if precomp else None       # always the plain build's: the input of both twins
    if fma:
        with oracle.fma_twin():
            radii, terms = oracle.visible_filter_terms(VC.scene_of(case, mod, cov))
    else:
        radii, terms = oracle.visible_filter_terms(VC.scene_of(case, mod, cov))
    return radii, terms, cov


def oracle_pred(case, fma=False):
    args = VC.lod_args(case)[:-1]
    if fma:
        with oracle.fma_twin():
            return oracle_decode.lod_pred(*args)
    return oracle_decode.lod_pred(*args)


def measure():
    """-> {gate: largest deviation of a float32 oracle from the truth, in the units of the gate's margin} over every case, both builds of the
    oracle, both scale modifiers and both covariance paths"""
    worst = dict.fromkeys(VT.GATES, 0.0)
    for name in VC.NAMES:
        case = VC.make(name)
        t = VC.lod_truth(case, "floor")
        for fma in (False, True):
            p32 = oracle_pred(case, fma).astype(np.float64)
            fin = np.isfinite(t["pred"]) & np.isfinite(p32)
            if fin.any():
                worst["pred"] = max(worst["pred"], float(np.abs(p32 - t["pred"])[fin].max()))
            for mod in MODS:
                for precomp in (False, True):
                    radii, terms, cov = oracle_filter(name, mod, precomp, fma)
                    pf = VC.filter_truth(case, mod, cov3D=cov)
                    d = np.abs(terms.astype(np.float64) - pf["terms"])
                    same_r = np.ceil(terms[:, 2].astype(np.float64)) == pf["raw"]            # the rect operands hold the radius: compare like with like
                    for gate, col, ok in (("depth", d[:, 0], None), ("det", d[:, 1], None), ("radius", d[:, 2], None)):
                        v = col / pf["scales"][gate]
                        v = v[np.isfinite(v)]
                        if v.size:
                            worst[gate] = max(worst[gate], float(v.max()))
                    v = (d[:, 3:] / pf["scales"]["rect"])[same_r]
                    v = v[np.isfinite(v)]
                    if v.size:
                        worst["rect"] = max(worst["rect"], float(v.max()))
    return worst


def test_bounds_cover_the_oracle_deviation():
    """Every bound of visible_truth is at least 4 x the largest deviation of the float32 oracles from the truth, and not idly wide: at most 8 x."""
    worst = measure()
    for g in VT.GATES:
        print(f"gate {g}: largest oracle deviation {worst[g]:.3e}, x4 = {4 * worst[g]:.3e}, bound {VT.BOUND[g]:.3e}, recorded {VT.MEASURED[g]:.3e}")
    for g in VT.GATES:
        assert 4 * worst[g] <= VT.BOUND[g] <= 8 * max(worst[g], VT.MEASURED[g]), g


@pytest.mark.parametrize("name", VC.NAMES)
def test_cases_meet_their_conditions(name):
    case = VC.make(name)
    Na = case["anchor"].shape[0]
    assert VC.conditions(case) == []
    pf = VC.filter_truth(case)
    for mode in VT.MODES:
        f = VC.fragile(case, mode)
        t = VC.lod_truth(case, mode)
        print(f"{name} (seed {case['seed']}) {mode}: fragile {int(f.sum())} / {Na} = {f.mean():.4f}, masked in {t['anchor_mask'].mean():.2f}, "
              f"visible {pf['visible'].mean():.2f}")
        assert f.sum() <= VC.MAX_FRAGILE * Na


@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("name", VC.NAMES)
def test_truth_equals_the_oracles_on_robust_anchors(name, fma):
    case = VC.make(name)
    for mode in VT.MODES:
        t = VC.lod_truth(case, mode)
        args = VC.lod_args(case) + (VT.MODES.index(mode),)
        if fma:
            with oracle.fma_twin():
                m, pr, tr = oracle_decode.lod_mask(*args)
        else:
            m, pr, tr = oracle_decode.lod_mask(*args)
        got = dict(anchor_mask=m, prog_ratio=pr if mode == "progressive" else None, transition_mask=tr if mode == "progressive" else None)
        VT.check_lod(got, t, f"{name} {mode}")
    for mod in MODS:
        for precomp in (False, True):
            radii, _, cov = oracle_filter(name, mod, precomp, fma)
            stats = VT.check_filter(radii, VC.filter_truth(case, mod, cov3D=cov), None, f"{name} mod {mod} precomp {precomp}")
            assert sum(n for n, _ in stats.values()) <= VC.MAX_FRAGILE * max(case["anchor"].shape[0], 100)


@pytest.mark.parametrize("name", VC.NAMES)
def test_lod_truth_equals_the_reference_formula_in_float64_torch(name):
    """ref_anchor_octree_torch.pred_levels / int_levels restate the reference's Python (weed_out's use of map_to_int_level): with the camera
    'scale' = resolution_scale and the position = anchor + half they evaluate set_anchor_mask's formula."""
    case = VC.make(name)
    lv = case["level"].astype(np.int64)
    half = (np.float32(case["voxel_size"]).astype(np.float64) / 2) / float(case["fork"]) ** lv
    pos = torch.tensor(case["anchor"].astype(np.float64) + half[:, None])
    cam = torch.tensor(np.concatenate([case["campos"].astype(np.float64), [np.float64(np.float32(case["resolution_scale"]))]])[None, :])
    pred = R.pred_levels(pos, cam, float(np.float32(case["standard_dist"])), case["fork"], torch.float64)[:, 0]
    if case["extra_level"] is not None:
        pred = pred + torch.tensor(case["extra_level"].astype(np.float64))
    for mode in ("floor", "round", "ceil"):
        t = VC.lod_truth(case, mode)
        fin = np.isfinite(t["pred"])
        assert np.abs(pred.numpy() - t["pred"])[fin].max() < 1e-12 if fin.any() else True
        il = R.int_levels(pred[torch.tensor(fin)], case["coarse_index"], mode).numpy()
        near = t["margin"][fin] < 1e-9                                  # the two float64 evaluations differ by 1e-15: not at a tie
        assert np.array_equal(il[~near], t["int_level"][fin][~near])
        assert np.array_equal((lv[fin] <= il)[~near], t["anchor_mask"][fin][~near])


def test_planted_rows_give_their_hand_written_answers():
    case = VC.make("planted")
    rows = case["rows"]
    pf = VC.filter_truth(case)
    fr = VT.fragile_gates(pf["margins"]).any(axis=1)
    for n, want in VC.PLANTED_RADII.items():
        assert pf["radii"][rows[n]] == want and not fr[rows[n]], (n, int(pf["radii"][rows[n]]), want)
    assert 20 < pf["radii"][rows["needle"]] <= 31 and not fr[rows["needle"]]        # a 10-pixel sigma along its long axis (|q|^2 = 0.95), 1e-3 across
    zero = np.zeros((len(rows), 6), np.float32)
    assert (VC.filter_truth(case, cov3D=zero)["radii"][pf["terms"][:, 0] > 0.3] == np.where(pf["radii"] > 0, 3, 0)[pf["terms"][:, 0] > 0.3]).all()
    z = pf["terms"][:, 0]
    for n, want in VC.PLANTED_MARK_VISIBLE.items():
        assert bool(z[rows[n]] > np.float64(np.float32(0.2))) == want, n
    for k, mode in enumerate(VT.MODES):
        t = VC.lod_truth(case, mode)
        assert (t["margin"][[rows[n] for n in VC.PLANTED_MASK]] > VT.BOUND["pred"]).all()
        for n, want in VC.PLANTED_MASK.items():
            assert bool(t["anchor_mask"][rows[n]]) == want[k], (mode, n)
        if mode == "progressive":
            for n, (ratio, trans) in VC.PLANTED_PROG.items():
                assert abs(t["prog_ratio"][rows[n]] - ratio) < 1e-12 and bool(t["transition_mask"][rows[n]]) == trans, n
    assert np.isposinf(VC.lod_truth(case, "round")["pred"][rows["at_camera"]])
    # the float32 oracle meets the same rows (its d^2 overflows on the last: pred -inf)
    assert np.isneginf(oracle_decode.lod_pred(*VC.lod_args(case)[:-1])[rows["overflow_out"]])
    for k, mode in enumerate(VT.MODES):
        m, _, _ = oracle_decode.lod_mask(*VC.lod_args(case), k)
        for n, want in VC.PLANTED_MASK.items():
            assert bool(m[rows[n]]) == want[k], ("oracle", mode, n)
    assert np.array_equal(oracle.mark_visible(case["anchor"], case["viewmatrix"], case["projmatrix"]), z > np.float64(np.float32(0.2)))


DEFECT_CASE = {"lt": "random1025", "half_away": "planted", "no_half": "random1025", "stride3": "random1025", "no_mod": "random4099"}


@pytest.mark.parametrize("defect", VT.DEFECTS)
def test_a_planted_defect_trips_the_checker(defect):
    """A copy of the truth with one defect, handed to the checkers as if it were a device result, is refused; without the defect it passes."""
    case = VC.make(DEFECT_CASE[defect])
    mode = "progressive" if defect == "no_half" else "round"
    t, pf = VC.lod_truth(case, mode), VC.filter_truth(case)

    def result(d):
        lt = VC.lod_truth(case, mode, defect=d if d in ("lt", "half_away", "no_half") else None)
        f = VC.filter_truth(case, defect=d if d in ("stride3", "no_mod") else None)
        radii = np.where(lt["anchor_mask"], f["radii"], 0)
        return dict(anchor_mask=lt["anchor_mask"], prog_ratio=lt["prog_ratio"], transition_mask=lt["transition_mask"], radii=radii, visible_mask=radii > 0)

    VT.check_octree(result(None), t, pf, "clean")
    with pytest.raises(AssertionError):
        VT.check_octree(result(defect), t, pf, defect)
