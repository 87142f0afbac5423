"""Octree-GS anchor growing + pruning without a device: the torch restatement (tests/ref_anchor_octree_torch.py) against the fixtures the
reference's own OctreeGaussian.adjust_anchor produced (tests/golden/make_golden_anchor_octree.py), bit for bit; what each fixture is named for;
the header declarations and exports; and the argument errors of the Python entry points, which are raised before any device call."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_anchor_octree_torch as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_anchor_octree_*.npz")))
SYMBOLS = ["gsr_anchor_level_find_weed", "gsr_octree_weed_out"]
KEPT = ["gsr_anchor_level_scratch_bytes", "gsr_anchor_level_find", "gsr_anchor_level_emit", "gsr_rows_compact_scratch_bytes", "gsr_rows_compact_multi"]


def load(path):
    return {k: torch.tensor(v) for k, v in np.load(path).items()}


def fixture(name):
    return load(os.path.join(ROOT, "tests", "golden", f"ref_anchor_octree_{name}.npz"))


def test_fixture_set_holds_what_the_cases_are_named_for():
    names = {os.path.basename(p)[len("ref_anchor_octree_"):-4] for p in FIXTURES}
    assert names >= {"default", "gap", "k10", "noprune"}
    for p in FIXTURES:
        assert os.path.getsize(p) < 400 * 1024
    fx = fixture("default")
    found, kept = fx["pass_found"], fx["pass_kept"]
    assert int(kept[:, 0].sum()) > 0 and int(kept[:, 1].sum()) > 0                          # additions from pass A and from pass B
    mixed = ((kept > 0) & (kept < found)).any(dim=1)
    assert int(mixed.sum()) >= 2                                                            # at two levels, weeding keeps some and drops some
    assert int(found[-1, 0]) > 0 and int(found[-1, 1]) == 0                                 # the last level: pass A only
    assert int(fx["dist2level"]) == 1 and not bool(fx["keep"].all())                        # round; something pruned
    assert fx["out_level"].dtype == torch.float32 and fx["in_level"].dtype == torch.int32
    assert 7 <= fx["cam_infos"].shape[0] <= 24
    fx = fixture("gap")
    lv = fx["in_level"].reshape(-1)
    assert int(fx["levels"]) == 4 and not bool((lv == 2).any()) and bool((lv == 3).any())   # level 2 holds no anchor: its turn is skipped
    assert int(fx["pass_found"][1, 1]) == 0 and int(fx["pass_found"][2].sum()) == 0         # pass B of level 1 adds nothing, although ...
    g = torch.nan_to_num(fx["in_offset_gradient_accum"] / fx["in_offset_denom"], nan=0.0).abs().reshape(-1)
    g[~(fx["in_offset_denom"] > 40.0).reshape(-1)] = 0.0
    assert bool(((g >= 0.0002 * 2.0) & (lv == 1).repeat_interleave(int(fx["k"]))).any())    # ... candidates exist
    own3 = (lv == 3).repeat_interleave(int(fx["k"]))
    assert bool(((g >= 0.0002 * 2 ** 1.5) & (g < 0.0002 * 4) & own3).any()) and int(fx["pass_found"][3, 0]) == 0     # candidates that are all occupied
    assert bool(((fx["pass_found"] > 0) & (fx["pass_kept"] == 0)).any())                    # a pass weeded to nothing
    assert int(fx["dist2level"]) == 0                                                       # floor
    fx = fixture("k10")
    assert int(fx["k"]) == 10 and fx["in_anchor_feat"].shape[1] == 32
    fx = fixture("noprune")
    assert not bool((fx["in_anchor_demon"] > 80).any()) and bool(fx["keep"].all())
    assert bool(fx["progressive"]) and int(fx["iteration"]) <= float(fx["coarse_intervals"][-1]) and int(fx["pass_found"][:, 1].sum()) == 0
    assert torch.equal(fx["out_extra_level"][:fx["in_extra_level"].shape[0]], fx["in_extra_level"])      # coarse phase: no extra level is raised


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_restatement_equals_reference_fixture(path):
    fx = load(path)
    out = R.adjust(fx)
    for name, got in out.items():
        want = fx[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if name in ("out_level", "new_level"):
            assert got.dtype == want.dtype, name
        assert torch.equal(got.to(want.dtype), want), name


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixture_margins(path):
    """What keeps exact equality honest: no (new position, camera) pred within 1e-5 of its rounding boundary, in float64."""
    fx = load(path)
    pos, lv = fx["new_anchor"], fx["new_level"].reshape(-1)
    if pos.shape[0] == 0:
        return
    pred = R.pred_levels(pos, fx["cam_infos"], float(fx["standard_dist"]), int(fx["fork"]), torch.float64)
    shift = 0.5 if int(fx["dist2level"]) == 1 else 0.0
    assert float((pred - shift - torch.round(pred - shift)).abs().min()) >= 1e-5
    mode = ("floor", "round", "ceil")[int(fx["dist2level"])]
    vis, keep = R.weed_out(pos, lv, fx["cam_infos"], float(fx["standard_dist"]), int(fx["fork"]), int(fx["levels"]), mode, float(fx["visible_threshold"]))
    assert bool(keep.all())                                                                 # every appended anchor survived its own weed-out
    vis64, _ = R.weed_out(pos, lv, fx["cam_infos"], float(fx["standard_dist"]), int(fx["fork"]), int(fx["levels"]), mode, float(fx["visible_threshold"]),
                          torch.float64)
    assert torch.equal(vis, vis64)


def test_restatement_weed_out_against_a_camera_loop():
    r = np.random.default_rng(3)
    U, Cn, levels = 200, 9, 5
    pos = torch.tensor(r.uniform(-1, 1, (U, 3)).astype(np.float32))
    lv = torch.tensor(r.integers(0, levels, U).astype(np.int32))
    cams = torch.tensor(np.concatenate([r.normal(0, 3, (Cn, 3)), r.choice([1.0, 2.0], (Cn, 1))], 1).astype(np.float32))
    for mode, fn in (("floor", torch.floor), ("round", torch.round), ("ceil", torch.ceil)):
        count = torch.zeros(U, dtype=torch.int32)
        for cam in cams:
            dist = torch.sqrt(torch.sum((pos - cam[:3]) ** 2, dim=1)) * cam[3]
            il = torch.clamp(fn(torch.log2(torch.tensor(4.0) / dist) / np.log2(2)).int(), min=0, max=levels - 1)
            count += (lv <= il).int()
        vis, keep = R.weed_out(pos, lv, cams, 4.0, 2, levels, mode, 0.4)
        assert torch.equal(vis, count) and torch.equal(keep, count / Cn > 0.4) and 0 < int(keep.sum()) < U


def test_header_exports_and_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS + KEPT:
        assert s in decl, f"include/gsrast.h does not declare {s}"
    assert "typedef struct gsr_octree_weed" in src
    assert re.search(r"#define GSR_ABI_VERSION 8\b", src)                                   # extended, not changed
    import gsrast
    from gsrast import _rows, anchors, octree
    L = gsrast.lib()
    for s in SYMBOLS + KEPT:
        assert s in gsrast.EXPORTS and hasattr(L, s)
    assert callable(anchors.octree_adjust_anchor_) and callable(octree.weed_out)
    m = re.search(r"#define GSR_OCTREE_WEED_CHUNK (\d+)", src)
    assert m and int(m.group(1)) == _rows.WEED_CHUNK


def test_library_argument_errors_without_a_device():
    import ctypes as C
    import gsrast
    from gsrast import _rows, anchors
    L = gsrast.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    lv = anchors.Level(Na=4, N0=4, k=2, F=3, scaling_stride=6, thr_lo=0.0, thr_hi=1.0, rand_thr=0.5, cell=0.1, origin=(C.c_float * 3)(0, 0, 0),
                       anchor=a, mask=None, offset=a, scaling=a, anchor_feat=a, grads=a, offset_mask=a, rand=None)

    def weed(**kw):
        base = dict(cam_infos=a, C=3, levels=4, mode=1, lv=0, standard_dist=2.0, fork=2.0, visible_threshold=0.2)
        base.update(kw)
        return _rows.Weed(**base)

    def find(w, nbytes=1 << 20):
        return L.gsr_anchor_level_find_weed(C.byref(lv), None, C.byref(w), a, nbytes, a, None)
    assert find(weed(mode=3)) != 0 and "progressive" in gsrast.last_error()
    assert find(weed(mode=7)) != 0 and "dist2level" in gsrast.last_error()
    assert find(weed(C=0)) != 0 and "camera" in gsrast.last_error()
    assert find(weed(levels=0)) != 0 and "levels" in gsrast.last_error()
    assert find(weed(fork=1.0)) != 0 and "fork" in gsrast.last_error()
    assert find(weed(), nbytes=16) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_octree_weed_out(a, a, 4, C.byref(weed(mode=3)), a, a, None) != 0 and "progressive" in gsrast.last_error()
    assert L.gsr_octree_weed_out(a, None, 4, C.byref(weed()), a, a, None) != 0 and "NULL" in gsrast.last_error()
    assert L.gsr_octree_weed_out(a, a, 1 << 31, C.byref(weed()), a, a, None) != 0 and "out of range" in gsrast.last_error()


def test_python_argument_errors_name_the_argument():
    from gsrast import anchors, octree
    N, k = 6, 2
    z = torch.zeros

    class M:
        pass
    m = M()
    with pytest.raises(RuntimeError, match="attribute _anchor is missing"):
        anchors.octree_adjust_anchor_(m, 3000)
    for n in list(anchors.PARAM_ATTRS.values()) + ["get_scaling", "opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"]:
        setattr(m, n, z(N, 3))
    m.optimizer = torch.optim.Adam([torch.nn.Parameter(z(1))])
    m.n_offsets = k
    with pytest.raises(RuntimeError, match="attribute _level is missing"):
        anchors.octree_adjust_anchor_(m, 3000)
    m._level, m._extra_level, m.levels, m.fork, m.voxel_size, m.init_pos, m.standard_dist = z(N, 1, dtype=torch.int32), z(N), 3, 2, 0.1, z(3), 2.0
    m.cam_infos, m.visible_threshold, m.progressive, m.coarse_intervals = z(4, 4), 0.2, False, []
    with pytest.raises(RuntimeError, match="attribute dist2level is missing"):
        anchors.octree_adjust_anchor_(m, 3000)
    m.dist2level = "progressive"
    with pytest.raises(RuntimeError, match="progressive"):
        anchors.octree_adjust_anchor_(m, 3000)
    m.dist2level = "round"
    with pytest.raises(RuntimeError, match="model._anchor must be a CUDA tensor"):
        anchors.octree_adjust_anchor_(m, 3000)
    with pytest.raises(RuntimeError, match="positions must be a CUDA tensor"):
        octree.weed_out(z(5, 3), z(5, dtype=torch.int32), z(4, 4), 2.0, 2, 3)
