"""Everything the GPU cases of test_gpu_tsdf_edges.py rest on, without a GPU: the float64 truth (tsdf_truth) against the float32 CPU restatement
(oracle.SparseTSDF) on every scene used there, the conditions each scene must meet to exercise its branch -- asserted on the truth's own output, so that
a scene that stops doing so fails here and not silently -- and the host restatement of the hash with the coordinate lists built from it."""
import numpy as np
import pytest

import oracle
import tsdf_cases
import tsdf_truth

from tsdf_truth import COLOUR_BAR, TSDF_BAR, robust_errors


def _oracle_units(case):
    frs, vl, tr, stride, dt, quant, tv = tsdf_cases.small_truth(case)
    v = oracle.SparseTSDF(vl, tr)
    for f in frs:
        col = tsdf_cases.rgb8(f["rgb"]) if quant == 2 else (np.clip(f["rgb"], 0, 1) * np.float32(255)).astype(np.float32)
        v.integrate(col, f["depth"], f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=dt, stride=stride)
    return v.units()


@pytest.mark.parametrize("case", sorted(tsdf_cases.TRUTH_CASES))
def test_truth_equals_the_float32_restatement_on_robust_voxels(case):
    tv = tsdf_cases.small_truth(case)[-1]
    assert not any(s["fragile"].any() for s in tv.samples)                  # allocation is exact, and so is every unit's first frame
    nw, et, ec, nrob, share = robust_errors(_oracle_units(case), tv)
    print(f"{case}: {len(tv.index)} units, {nrob} robust updated voxels, fragile share {100 * share:.2f} %, weight mismatches {nw}, "
          f"tsdf error {et:.1e}, colour error {ec:.1e}")
    assert nw == 0 and et <= TSDF_BAR and ec <= COLOUR_BAR
    assert share <= 0.03                                                    # a cap, not a measurement
    assert nrob >= 5000
    assert len(tv.index) <= 400
    assert all(len(rows) > opened for rows, opened in tv.touched[1:])       # later frames list units again that are not fresh


def _wave_kinds(s):
    """{workgroup: {wave: True if every valid sample of the wave opens at most 2 units per axis}} for the waves that hold a valid sample."""
    small = ((s["hi"] - s["lo"]) <= 1).all(axis=1)
    out = {}
    for i, sm in zip(s["i"].tolist(), small.tolist()):
        w = out.setdefault(i // 256, {})
        w[i // 64] = w.get(i // 64, True) and sm
    return out


def test_scenes_reach_the_branches_they_are_for():
    span = lambda case: [int((s["hi"] - s["lo"]).max()) for s in tsdf_cases.small_truth(case)[-1].samples]
    assert span("t5") == [1, 1, 1]                                          # the leader path alone
    s9 = tsdf_cases.small_truth("t9")[-1].samples
    for s in s9:                                                            # 96 x 72 at stride 4: 432 samples, 2 workgroups, 7 waves, both kinds of wave in workgroup 0
        assert s["n"] == 432 and (s["n"] + 255) // 256 == 2 and (s["n"] + 63) // 64 == 7
        kinds = _wave_kinds(s)
        assert any(True in k.values() and False in k.values() for k in kinds.values()), kinds
    assert all(True in _wave_kinds(s)[0].values() and False in _wave_kinds(s)[0].values() for s in s9)
    assert max(span("t12")) == 2 and not any(True in k.values() for s in tsdf_cases.small_truth("t12")[-1].samples for k in _wave_kinds(s).values())
    assert span("t24") == [3, 3, 3]                                         # 4 units on an axis
    near = tsdf_cases.small_truth("near")[-1]
    assert near.behind.sum() > 100 and near.outside.sum() > 100             # voxels of opened units behind the camera, and projecting outside the image
    # the sample rows wrap in the middle of a wave; fewer samples than a wave; a sample count that is no multiple of 256
    # (47 pixels at stride 3 are 16 samples a row, which divides a wave: that case is there for W % stride != 0)
    for case, n, nu in (("s1", 1645, 47), ("s3", 192, 16), ("s4", 108, 12), ("w5x3", 2, 2), ("w7x5", 35, 7)):
        s = tsdf_cases.small_truth(case)[-1].samples[0]
        assert s["n"] == n and (64 % nu != 0 or case in ("s3", "w5x3")) and n % 256 != 0
    assert 47 % 3 != 0 and 47 % 4 != 0
    # every kind of pixel the kernels must skip is among the SAMPLED ones
    f = tsdf_cases.small_scene("t5")[0][0]
    d = f["depth"][0, ::4, ::4]
    assert np.isnan(d).any() and (d < 0).any() and (d == 0).any() and (d > tsdf_cases.SMALL_DT).any()
    assert f["rgb"].min() < 0 and f["rgb"].max() > 1
    assert len(tsdf_cases.small_truth("t5_inf")[-1].index) > len(tsdf_cases.small_truth("t5")[-1].index)      # the far block is a surface again


def test_host_hash_and_probe_lists():
    """ts_pack / ts_hash of gsr_tsdf_view.h on the host; the lists of the probing tests wrap the table they target."""
    assert tsdf_truth.ts_pack(0, 0, 0) == (1 << 62) | (1 << 41) | (1 << 20)
    assert tsdf_truth.ts_pack(tsdf_truth.KEY_LO, tsdf_truth.KEY_HI, -1) == (1 << 42) | (((1 << 21) - 2) << 21) | ((1 << 20) - 1)
    assert tsdf_truth.ts_pack(tsdf_truth.KEY_HI + 1, tsdf_truth.KEY_HI + 1, tsdf_truth.KEY_HI + 1) == (1 << 63) - 1      # one past the range: all 63 key bits set
    assert tsdf_truth.ts_hash(1, 5) == 0x9E3779B97F4A7C15 >> 59 and tsdf_truth.ts_hash((1 << 64) - 1, 6) == ((1 << 64) - 0x9E3779B97F4A7C15) >> 58
    first, more = tsdf_cases.probe_wrap_lists()
    both = np.concatenate([first, more])
    assert len({tuple(c) for c in both.tolist()}) == 20
    assert [h for h, _ in tsdf_truth.probe_positions(first, 5)] == [29, 30, 31, 31, 31, 0, 0, 1, 2, 2, 5, 9]
    assert sorted(p for _, p in tsdf_truth.probe_positions(first, 5)) == [0, 1, 2, 3, 4, 5, 6, 7, 9, 29, 30, 31]
    assert tsdf_truth.probe_wraps(first, 5) and tsdf_truth.probe_wraps(first, 6) and tsdf_truth.probe_wraps(both, 6)
    assert tsdf_truth.probe_wraps(first[::-1], 5)                           # whatever the order of insertion
    # an out-of-range coordinate aliases another unit's key: what k_ts_insert_list must refuse
    assert tsdf_truth.ts_pack(0, 0, tsdf_truth.KEY_HI + 2) == tsdf_truth.ts_pack(0, 1, tsdf_truth.KEY_LO - 1)
