"""The visibility stage on the device (gsr_octree_visible = k_lod_mask + the masked k_preprocess_ewa<true>, gsr_visible_filter, gsr_mark_visible;
csrc/gsr_preprocess.hip) held to the float64 truth of tests/visible_truth.py on the cases of tests/visible_cases.py: exactly on every anchor the
truth calls robust, and on a fragile one only in what its fragile gates feed.  No forgiven fraction."""
import functools

import numpy as np
import pytest
import torch

import oracle
import visible_cases as VC
import visible_truth as VT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODS = (1.0, 0.7)


def _t(a, dtype=None):
    return None if a is None else torch.tensor(a, device=DEV, dtype=dtype)


def settings(case, scale_modifier=None):
    import scaffold_filter
    return scaffold_filter.GaussianRasterizationSettings(
        image_height=int(case["H"]), image_width=int(case["W"]), tanfovx=float(case["tanfovx"]), tanfovy=float(case["tanfovy"]),
        bg=torch.zeros(3, device=DEV), scale_modifier=float(case["scale_modifier"] if scale_modifier is None else scale_modifier),
        viewmatrix=_t(case["viewmatrix"]), projmatrix=_t(case["projmatrix"]), sh_degree=0, campos=_t(case["campos"]), prefiltered=False, debug=False)


def run_octree(case, mode, scales=None, extra="case"):
    from gsrast import octree
    sc = case["scales6"] if scales is None else scales
    ex = case["extra_level"] if extra == "case" else extra
    out = octree.octree_visible(settings(case), _t(case["anchor"]), _t(case["level"]).unsqueeze(1), _t(sc), _t(case["rotations"]), case["voxel_size"],
                                case["fork"], case["standard_dist"], case["coarse_index"], dist2level=mode, extra_level=_t(ex),
                                resolution_scale=case["resolution_scale"])
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def run_filter(case, mod, cov3D=None, means=None):
    import scaffold_filter
    r = scaffold_filter.GaussianRasterizer(settings(case, mod))
    m = _t(case["anchor"]) if means is None else means
    if cov3D is not None:
        return r.visible_filter(m, cov3D_precomp=_t(cov3D)).cpu().numpy()
    return r.visible_filter(m, scales=_t(np.ascontiguousarray(case["scales6"][:, :3])), rotations=_t(case["rotations"])).cpu().numpy()


@functools.lru_cache(maxsize=None)
def truths(name, mode):
    case = VC.make(name)
    return VC.lod_truth(case, mode), VC.filter_truth(case)


@pytest.mark.parametrize("mode", VT.MODES)
@pytest.mark.parametrize("name", VC.NAMES)
def test_octree_visible_against_float64(name, mode):
    case = VC.make(name)
    Na = case["anchor"].shape[0]
    t, pf = truths(name, mode)
    got = run_octree(case, mode)
    assert got["anchor_mask"].dtype == np.bool_ and got["radii"].dtype == np.int32 and got["radii"].shape == (Na,)
    if mode == "progressive":
        assert got["prog_ratio"].shape == (Na, 1) and got["prog_ratio"].dtype == np.float32 and got["transition_mask"].dtype == np.bool_
    else:
        assert got["prog_ratio"] is None and got["transition_mask"] is None          # the optional outputs are not produced
    stats = VT.check_octree(got, t, pf, f"{name} {mode}")
    print(f"{name} {mode}: Na {Na}, per gate (fragile, differing) {stats}")
    assert not (got["radii"][~got["anchor_mask"]] != 0).any()                          # masked out by the LOD: radius 0 whatever the geometry
    # the (Na,3) scale form reads the same three numbers: identical output
    got3 = run_octree(case, mode, scales=np.ascontiguousarray(case["scales6"][:, :3]))
    for k, v in got.items():
        assert (v is None and got3[k] is None) or np.array_equal(v, got3[k]), k
    # octree_visible == visible_filter restricted to the device's own anchor_mask, bit for bit
    flt = run_filter(case, case["scale_modifier"])
    assert np.array_equal(got["radii"], np.where(got["anchor_mask"], flt, 0))


@pytest.mark.parametrize("name", ["planted", "random257", "random4099"])
def test_masked_out_anchors_are_not_read(name):
    """Anchors the LOD removes get radius 0 without their scales or rotations being looked at: non-finite values there change nothing."""
    case = VC.make(name)
    for mode in VT.MODES:
        t, _ = truths(name, mode)
        clean = run_octree(case, mode)
        out = ~clean["anchor_mask"] & (t["margin"] > VT.BOUND["pred"])
        assert out.any()
        bad = dict(case, scales6=case["scales6"].copy(), rotations=case["rotations"].copy())
        bad["scales6"][out] = np.array([np.nan, np.inf, -np.inf, np.nan, np.nan, np.nan], np.float32)
        bad["rotations"][out] = np.nan
        got = run_octree(bad, mode)
        for k, v in clean.items():
            assert (v is None and got[k] is None) or np.array_equal(v, got[k]), (mode, k)
        assert not got["radii"][out].any()


@pytest.mark.parametrize("name", VC.NAMES)
def test_visible_filter_against_float64(name):
    """Both covariance paths and both scale modifiers; the precomputed covariance is the float32 oracle's, and the truth consumes those numbers."""
    case = VC.make(name)
    for mod in MODS:
        cov = oracle.cov3d(case["scales6"], mod, case["rotations"])
        for path, c in (("scales", None), ("precomp", cov)):
            got = run_filter(case, mod, c)
            stats = VT.check_filter(got, VC.filter_truth(case, mod, cov3D=c), None, f"{name} mod {mod} {path}")
            print(f"{name} visible_filter mod {mod} {path}: per gate (fragile, differing) {stats}")


def test_planted_rows_on_the_device():
    """The hand-written answers of visible_cases: depth rows at 0.2f and its neighbours, an anchor at the camera (pred +inf), far ones (pred -20,
    -inf), ties of 'round', splats at the four image borders, a radius larger than the image, a zero covariance, a zero quaternion."""
    import diff_gaussian_rasterization as dgr
    case = VC.make("planted")
    rows = case["rows"]
    radii = run_filter(case, 1.0)
    for n, want in VC.PLANTED_RADII.items():
        assert radii[rows[n]] == want, (n, int(radii[rows[n]]), want)
    zero = run_filter(case, 1.0, np.zeros((len(rows), 6), np.float32))
    assert zero[rows["zero_cov"]] == 3 and zero[rows["huge"]] == 3 and zero[rows["left_out"]] == 0 and zero[rows["z_at"]] == 0
    s = settings(case)
    mv = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**s._asdict())).markVisible(_t(case["anchor"])).cpu().numpy()
    for n, want in VC.PLANTED_MARK_VISIBLE.items():
        assert bool(mv[rows[n]]) == want, n
    for k, mode in enumerate(VT.MODES):
        got = run_octree(case, mode)
        for n, want in VC.PLANTED_MASK.items():
            assert bool(got["anchor_mask"][rows[n]]) == want[k], (mode, n)
        if mode == "progressive":
            for n, (ratio, trans) in VC.PLANTED_PROG.items():
                assert abs(float(got["prog_ratio"][rows[n], 0]) - ratio) <= 1.2e-7 and bool(got["transition_mask"][rows[n]]) == trans, n      # one float32 ulp below 1


@pytest.mark.parametrize("name", ["planted", "random256", "random4099"])
def test_mark_visible_against_float64(name):
    import diff_gaussian_rasterization as dgr
    case = VC.make(name)
    pf = VC.filter_truth(case)
    z = pf["terms"][:, 0]
    want = z > np.float64(np.float32(0.2))
    s = settings(case)
    mv = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**s._asdict())).markVisible(_t(case["anchor"])).cpu().numpy()
    frag = pf["margins"]["depth"] <= VT.BOUND["depth"]
    print(f"{name} markVisible: fragile {int(frag.sum())}, differing {int((mv != want).sum())}")
    assert np.array_equal(mv[~frag], want[~frag]) and want.any() and not want.all()


def test_no_anchors():
    import diff_gaussian_rasterization as dgr
    from gsrast import octree
    case = VC.make("random64")
    s = settings(case)
    e = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=DEV)
    assert run_filter(case, 1.0, means=e(0, 3)).shape == (0,)
    mv = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**s._asdict())).markVisible(e(0, 3))
    assert mv.shape == (0,) and mv.dtype == torch.bool
    for mode in VT.MODES:
        out = octree.octree_visible(s, e(0, 3), e(0, 1, dt=torch.int32), e(0, 6), e(0, 4), 0.5, 2.0, 10.0, 6, dist2level=mode, extra_level=e(0))
        assert out["anchor_mask"].shape == (0,) and out["anchor_mask"].dtype == torch.bool and out["radii"].shape == (0,)
        assert out["radii"].dtype == torch.int32 and out["visible_mask"].shape == (0,)
        if mode == "progressive":
            assert out["prog_ratio"].shape == (0, 1) and out["transition_mask"].shape == (0,)
        else:
            assert out["prog_ratio"] is None and out["transition_mask"] is None
