"""CPU tests of the registration feature (gsrast.register): the restatements of tests/register_truth.py by hand and against independent
formulations (an SVD Kabsch / Umeyama fit, a winding-number point-in-polygon), the structure the named cases of tests/register_cases.py rest on,
the bar the device's ICP transformation is held to, and what can be held without a GPU of the binding: exports, ABI version, constants, the
host-side argument errors."""
import re

import numpy as np
import pytest

import register_cases as cases
import register_truth as truth

F = np.float32
ICP_MAIN = ("exact_copy", "partial_overlap", "different_sampling", "with_scaling")


# ---------------------------------------------------------------------------------------------------------------- the truth, by hand
def test_transform_by_hand():
    M = np.eye(4); M[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 2]]; M[:3, 3] = [1, 2, 3]
    assert truth.transform([[1, 2, 3], [0, 0, 0]], M).tolist() == [[-1, 3, 9], [1, 2, 3]]
    M = np.eye(4); M[0, 0] = 1 + 2.0 ** -30; M[0, 3] = 2.0 ** -40            # float64 inside, one rounding to float32 at the end
    assert truth.transform([[1, 0, 0]], M)[0, 0] == F(1) and truth.transform([[2.0 ** 24, 0, 0]], M)[0, 0] == F(2.0 ** 24 + 2.0 ** -6 + 2.0 ** -40)
    out = truth.transform(cases.NONFINITE_ROWS, cases.MOTION)
    assert np.isnan(out[0]).all() and not np.isfinite(out[3]).any() and np.isnan(out[3]).any() and np.isfinite(out[5]).all() and out.dtype == F
    assert truth.transform(np.zeros((0, 3)), M).shape == (0, 3)


def test_sums_by_hand():
    s = cases.a3([[0, 0, 0], [2, 0, 0], [0, 2, 0], [9, 9, 9]]); t = cases.a3([[1, 1, 1], [1, 3, 1], [-1, 1, 1]])
    r = truth.sums(s, t, [0, 1, 2, -1])                                       # a quarter turn about z and a move
    assert r["n"] == 3 and r["status"] == 0 and r["sum_p"].tolist() == [2, 2, 0] and r["sum_q"].tolist() == [1, 5, 3]
    assert np.allclose(r["H"], [[4 / 3, 8 / 3, 0], [-8 / 3, -4 / 3, 0], [0, 0, 0]]) and abs(r["spp"] - 16 / 3) < 1e-15 and abs(r["sqq"] - 16 / 3) < 1e-15
    M, st = truth.solve(r)
    assert st == 0 and np.abs(M - [[0, -1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]]).max() < 1e-15
    assert truth.sums(s, t, [0, 3, -2, -1])["status"] == truth.ERR_INDEX and truth.sums(s, t, [0, 3, -2, -1])["n"] == 1
    empty = truth.sums(s, t, [-1] * 4)
    assert empty["n"] == 0 and not empty["H"].any() and truth.solve(empty) == (None, truth.ERR_DEGENERATE)


def test_two_passes_keep_the_digits_one_pass_loses():
    s, t = cases.OFFSET_1E4
    idx = np.arange(len(s))
    two = truth.sums(s, t, idx)
    H1, spp1, sqq1 = truth.sums_one_pass(s, t, idx)
    back = truth.sums(s - F(1e4), t - F(1e4), idx)                            # the same cloud at the origin: the subtraction of 1e4 is exact in float32 here
    assert np.array_equal((s - F(1e4)).astype(np.float64) + 1e4, s.astype(np.float64))
    err2, err1 = np.abs(two["H"] - back["H"]).max(), np.abs(H1 - back["H"]).max()
    print(f"two-pass error {err2:.2e}, one-pass error {err1:.2e}")
    assert not np.array_equal(H1, two["H"]) and spp1 != two["spp"] and err1 > 1e3 * max(err2, 1e-16) and err2 < 1e-11


# ---------------------------------------------------------------------------------------------------------------- against independent formulations
def test_solve_against_an_svd_fit():
    worst = 0.0
    for name, (s, t, scaling) in cases.SOLVE.items():
        M, st = truth.solve(truth.sums(s, t, np.arange(len(s))), scaling)
        if name in cases.SOLVE_DEGENERATE:
            assert M is None and st == truth.ERR_DEGENERATE, name
            continue
        R = M[:3, :3] / (np.cbrt(np.linalg.det(M[:3, :3])) if scaling else 1.0)
        assert st == 0 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0.999999, name
        assert M[3].tolist() == [0, 0, 0, 1]
        if name == "collinear":                           # the turn about the line is free: only the line's image is determined
            assert np.abs(truth.transform(s, M).astype(np.float64) - t).max() < 1e-6
            continue
        d = np.abs(M - truth.kabsch(s, t, scaling)).max()
        worst = max(worst, d)
        print(f"{name}: |Horn - SVD| = {d:.2e}")
        assert d <= 1e-13, name
    print(f"largest difference {worst:.2e}")
    M, _ = truth.solve(truth.sums(*cases.SOLVE["half_turn"][:2], np.arange(40)))
    assert np.abs(M - np.diag([-1.0, -1, 1, 1])).max() < 1e-15               # quaternion (0, 0, 0, 1): w = 0
    refl = truth.sums(*cases.SOLVE["reflection"][:2], np.arange(40))
    U, _, Vt = np.linalg.svd(refl["H"].T)
    assert np.linalg.det(U @ Vt) < 0                      # the unconstrained SVD answer IS a reflection
    for scaling, want in (("scale_half", 0.5), ("scale_three", 3.0)):
        M, _ = truth.solve(truth.sums(*cases.SOLVE[scaling][:2], np.arange(40)), True)
        assert abs(np.cbrt(np.linalg.det(M[:3, :3])) - want) < 1e-6


def test_solve_ends_before_the_sweep_limit():
    """Every case diagonalises to exact zeros well inside GSR_REG_SWEEPS sweeps: the limit is a guard, not the usual exit."""
    for name, (s, t, _) in cases.SOLVE.items():
        if name in cases.SOLVE_DEGENERATE:
            continue
        saved, truth.SWEEPS = truth.SWEEPS, 12
        try:
            short = truth.solve(truth.sums(s, t, np.arange(len(s))))[0]
        finally:
            truth.SWEEPS = saved
        assert np.array_equal(short, truth.solve(truth.sums(s, t, np.arange(len(s))))[0]), name


@pytest.mark.parametrize("name", sorted(cases.POLYGONS))
def test_crop_against_a_winding_number(name):
    poly = cases.POLYGONS[name]
    r = np.random.default_rng(3)
    pts = np.stack([r.uniform(-1.3, 1.3, 4000), r.uniform(-1.3, 1.3, 4000), r.uniform(-1, 1, 4000)], 1).astype(F)
    for axis in "XYZ":
        ax = "XYZ".index(axis)
        p = np.empty_like(pts)
        iu, iv = [a for a in range(3) if a != ax]
        p[:, iu], p[:, iv], p[:, ax] = pts[:, 0], pts[:, 1], pts[:, 2]
        got, want = truth.crop(p, poly, axis, -0.5, 0.25), truth.crop_by_angles(p, poly, axis, -0.5, 0.25)
        assert np.array_equal(got, want) and 0.05 < got.mean() < 0.6, (name, axis, int((got != want).sum()))


def test_crop_by_hand():
    sq = cases.SQUARE
    pts = cases.a3([[0, 0, 0], [-0.5, 0, 0], [0.75, 0, 0], [0, -0.5, 0], [0, 0.5, 0], [-0.5, -0.5, 0], [0.75, 0.5, 0], [0, 0, 1], [0, 0, -1], [0, 0, np.nextafter(F(1), F(2))],
                    [np.nan, 0, 0], [2, 0, 0]])
    # inside; the left edge is in and the right one out (u < x); the lower edge is in and the upper one out (half-open in v); the slab's ends are in
    assert truth.crop(pts, sq, "Z", -1.0, 1.0).tolist() == [True, True, False, True, False, True, False, True, True, False, False, False]
    three = np.concatenate([sq[:, :1], sq[:, 1:], np.full((4, 1), 77.0)], 1)  # [K,3] as the crop file stores it: the coordinate along the axis is ignored
    assert np.array_equal(truth.crop(pts, three, "Z", -1.0, 1.0), truth.crop(pts, sq, "Z", -1.0, 1.0))
    ell = truth.crop(cases.a3([[0.5, 0.5, 0], [-0.5, 0.5, 0], [0.5, -0.5, 0]]), cases.ELL, "Z", -1, 1)
    assert ell.tolist() == [False, True, True]            # the notch of the L is outside


@pytest.mark.parametrize("name", sorted(cases.POLYGONS))
def test_crop_points_hit_what_they_are_there_for(name):
    poly = cases.POLYGONS[name]
    p = cases.crop_points(poly, "Y", -0.5, 0.25)
    assert p.shape == (257, 3) and (p[:, 1] == F(-0.5)).any() and (p[:, 1] == F(0.25)).any() and not np.isfinite(p).all()
    on_v = np.isin(p[:, 2].astype(np.float64), poly[:, 1].astype(F).astype(np.float64))
    keep = truth.crop(p, poly, "Y", -0.5, 0.25)
    assert on_v.sum() >= 3 and keep.any() and not keep.all()
    assert not keep[~np.isfinite(p).all(axis=1)].any()


# ---------------------------------------------------------------------------------------------------------------- the structure of the ICP cases
@pytest.mark.parametrize("name", sorted(cases.ICP))
def test_icp_cases_end_as_stated_and_stay_clear_of_their_thresholds(name):
    c = cases.ICP[name]
    r = cases.icp_truth(name)
    trace = r["trace"]
    print(name, r["iterations"], r["converged"], r["status"], [n for n, _, _ in trace], [f"{e:.2e}" for _, _, e in trace])
    assert (r["iterations"], r["converged"], r["status"]) == (c["iterations"], c["converged"], c["status"])
    assert len(trace) == r["iterations"] + 1
    rf, rr = c["kw"].get("relative_fitness", 1e-6), c["kw"].get("relative_rmse", 1e-6)
    for k in range(1, len(trace)):                        # no delta within a factor 8 of its threshold: a last-bit difference of the device's sums decides nothing
        for delta, tau in ((abs(trace[k][1] - trace[k - 1][1]), rf), (abs(trace[k][2] - trace[k - 1][2]), rr)):
            assert not tau / 8 <= delta <= 8 * tau, (name, k, delta, tau)
    if r["status"]:
        init = c["kw"].get("init")
        assert np.array_equal(r["transformation"], np.eye(4) if init is None else init)


def test_icp_case_structure():
    exact = cases.icp_truth("exact_copy")
    assert np.abs(exact["transformation"] - cases.MOTION).max() < 1e-6 and exact["fitness"] == 1.0 and exact["inlier_rmse"] < 1e-7
    part = cases.icp_truth("partial_overlap")
    counts = {n for n, _, _ in part["trace"]}
    assert len(counts) > 1 and max(counts) < 1300 and part["n_inliers"] >= 1200         # the inlier set changes on the way; the floaters never count
    assert np.abs(part["transformation"] - cases.MOTION).max() < 0.05
    slide = cases.icp_truth("different_sampling")
    assert slide["inlier_rmse"] > 1e-2 and not slide["converged"]                       # independent samples: point-to-point ICP is still sliding
    scaled = cases.icp_truth("with_scaling")
    assert abs(np.cbrt(np.linalg.det(scaled["transformation"][:3, :3])) - 1.1) < 1e-5
    zero = cases.icp_truth("max_iteration_0")
    assert zero["iterations"] == 0 and np.array_equal(zero["transformation"], np.eye(4)) and zero["trace"][0] == exact["trace"][0]
    none = cases.icp_truth("no_inliers")
    assert none["fitness"] == 0.0 and none["n_inliers"] == 0 and none["inlier_rmse"] == 0.0
    c = cases.ICP["exact_copy"]
    again = truth.icp(c["source"], c["target"], c["cap"], init=exact["transformation"], **c["kw"])
    assert again["iterations"] == 1 and again["converged"]                              # the with_init case of the GPU tests


def test_the_transformation_bar_is_eight_times_what_the_sums_bar_moves():
    worst = 0.0
    for name in ICP_MAIN:
        a, b = cases.icp_truth(name), cases.icp_truth(name, 1e-12)
        assert [n for n, _, _ in a["trace"]] == [n for n, _, _ in b["trace"]] and a["iterations"] == b["iterations"], name      # identical inlier traces
        d = float(np.abs(a["transformation"] - b["transformation"]).max())
        print(f"{name}: {d:.2e}")
        worst = max(worst, d)
    print(f"largest {worst:.2e}, bar {cases.TRANSFORM_BAR:.2e}")
    assert 8 * worst <= cases.TRANSFORM_BAR <= 16 * worst


# ---------------------------------------------------------------------------------------------------------------- the binding, without a GPU
NAMES = ["gsr_nearest_grid_scratch_bytes", "gsr_nearest_grid_build", "gsr_nearest_grid_query", "gsr_transform_points", "gsr_correspondence_sums_scratch_bytes",
         "gsr_correspondence_sums", "gsr_solve_transform", "gsr_icp_scratch_bytes", "gsr_icp", "gsr_crop_polygon_scratch_bytes", "gsr_crop_polygon_volume"]


def test_library_exports_the_entry_points_and_the_abi_stays_8():
    import gsrast
    L = gsrast.lib()
    assert L.gsr_abi_version() == 8 == gsrast.ABI_VERSION
    for name in NAMES:
        assert name in gsrast.EXPORTS and getattr(L, name).argtypes is not None, name
    from gsrast import chamfer, register
    for f in ("transform_points", "correspondence_sums", "solve_transform", "fit_transform", "icp", "evaluate_registration", "crop_polygon_volume", "RegistrationResult"):
        assert getattr(gsrast, f) is getattr(register, f), f
    assert gsrast.NearestGrid is chamfer.NearestGrid is register.NearestGrid
    assert "NOT" in register.transform_points.__doc__ and "full_proj_transform" in register.__doc__ and "Collinear" in register.solve_transform.__doc__


def test_constants_equal_the_header():
    import abi_header as H
    from gsrast import register
    c = H.constants(H.source("gsrast.h"))
    assert (register.ERR_INDEX, register.ERR_DEGENERATE) == (c["GSR_REG_ERR_INDEX"], c["GSR_REG_ERR_DEGENERATE"]) == (truth.ERR_INDEX, truth.ERR_DEGENERATE)
    assert register.SWEEPS == c["GSR_REG_SWEEPS"] == truth.SWEEPS and register.MAX_POLYGON == c["GSR_REG_MAX_POLYGON"] == truth.MAX_POLYGON
    assert register.MAX_ITERATION == c["GSR_REG_MAX_ITERATION"] and register.RECORD_WORDS == c["GSR_REG_RECORD_WORDS"]
    words = {k[len("GSR_REG_R_"):]: v for k, v in c.items() if k.startswith("GSR_REG_R_")}
    assert len(words) == 17 and all(getattr(register, "R_" + k) == v for k, v in words.items())
    assert max(words.values()) == register.RECORD_WORDS - 1


def test_scratch_queries_and_host_side_refusals():
    """What the library answers before it touches a device: sizes, and the argument errors of every entry point."""
    import ctypes as C
    import gsrast
    L = gsrast.lib()
    for q in (L.gsr_nearest_grid_scratch_bytes, L.gsr_correspondence_sums_scratch_bytes):
        assert q(1 << 31) == 0 and q(-1) == 0 and q(0) > 0 and q((1 << 31) - 1) > 0
    assert L.gsr_icp_scratch_bytes(1 << 31, 5) == 0 and L.gsr_icp_scratch_bytes(5, -1) == 0 and L.gsr_icp_scratch_bytes(5, 0) > 0
    assert L.gsr_nearest_grid_scratch_bytes(1000) == L.gsr_nearest_points_scratch_bytes(7, 1000)
    assert L.gsr_icp_scratch_bytes(1000000, 1000000) - L.gsr_nearest_grid_scratch_bytes(1000000) < 21 * 1000000 + (1 << 20)      # 20 bytes a source point above the grid
    assert L.gsr_crop_polygon_scratch_bytes() == 16 * 1024
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    eye = (C.c_double * 16)(*np.eye(4).reshape(-1))
    nan = (C.c_double * 16)(*([float("nan")] + [0.0] * 15))
    tri = (C.c_double * 6)(0, 0, 1, 0, 0, 1)
    big = 1 << 24
    for refused, word in ((lambda: L.gsr_nearest_grid_build(p, 1 << 31, -1.0, p, 4096, None), "out of range"),
                          (lambda: L.gsr_nearest_grid_build(p, 1, float("nan"), p, 4096, None), "NaN"),
                          (lambda: L.gsr_nearest_grid_build(None, 1, -1.0, p, 4096, None), "null"),
                          (lambda: L.gsr_nearest_grid_build(p, 1, -1.0, p, 16, None), "scratch too small"),
                          (lambda: L.gsr_nearest_grid_query(p, 1 << 31, 1, -1.0, p, 4096, p, p, None, None), "out of range"),
                          (lambda: L.gsr_nearest_grid_query(p, 1, 1, float("nan"), p, 4096, p, p, None, None), "NaN"),
                          (lambda: L.gsr_nearest_grid_query(p, 1, 1, -1.0, p, 4096, None, p, None, None), "null"),
                          (lambda: L.gsr_nearest_grid_query(p, 1, 1, -1.0, p, 16, p, p, None, None), "scratch too small"),
                          (lambda: L.gsr_transform_points(p, 1 << 31, eye, p, None), "out of range"),
                          (lambda: L.gsr_transform_points(p, 1, None, p, None), "null transformation"),
                          (lambda: L.gsr_transform_points(p, 1, nan, p, None), "non-finite"),
                          (lambda: L.gsr_transform_points(p, 1, eye, None, None), "null pointer"),
                          (lambda: L.gsr_correspondence_sums(p, -1, p, 1, p, p, p, big, None), "out of range"),
                          (lambda: L.gsr_correspondence_sums(p, 1, p, 1, p, None, p, big, None), "null"),
                          (lambda: L.gsr_correspondence_sums(p, 1, p, 1, None, p, p, big, None), "null"),
                          (lambda: L.gsr_correspondence_sums(p, 1, p, 1, p, p, p, 16, None), "scratch too small"),
                          (lambda: L.gsr_solve_transform(None, 0, None), "null record"),
                          (lambda: L.gsr_icp(p, 0, p, 1, 0.1, eye, 3, 1e-6, 1e-6, 0, p, p, big, None), "out of range"),
                          (lambda: L.gsr_icp(p, 1, p, 1, float("nan"), eye, 3, 1e-6, 1e-6, 0, p, p, big, None), "NaN"),
                          (lambda: L.gsr_icp(p, 1, p, 1, -1.0, eye, 3, 1e-6, 1e-6, 0, p, p, big, None), "negative"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, eye, 3, float("nan"), 1e-6, 0, p, p, big, None), "threshold"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, eye, 3, 1e-6, -1.0, 0, p, p, big, None), "threshold"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, eye, -1, 1e-6, 1e-6, 0, p, p, big, None), "max_iteration"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, nan, 3, 1e-6, 1e-6, 0, p, p, big, None), "non-finite"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, eye, 3, 1e-6, 1e-6, 0, None, p, big, None), "null"),
                          (lambda: L.gsr_icp(p, 1, p, 1, 0.1, eye, 3, 1e-6, 1e-6, 0, p, p, 16, None), "scratch too small"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1 << 31, tri, 3, 2, 0.0, 1.0, p, p, big, None), "out of range"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, tri, 2, 2, 0.0, 1.0, p, p, big, None), "vertices"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, tri, 1025, 2, 0.0, 1.0, p, p, big, None), "vertices"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, tri, 3, 3, 0.0, 1.0, p, p, big, None), "axis"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, tri, 3, 2, float("nan"), 1.0, p, p, big, None), "NaN"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, None, 3, 2, 0.0, 1.0, p, p, big, None), "null"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, (C.c_double * 6)(0, 0, 1, float("inf"), 0, 1), 3, 2, 0.0, 1.0, p, p, big, None), "non-finite"),
                          (lambda: L.gsr_crop_polygon_volume(p, 1, tri, 3, 2, 0.0, 1.0, p, p, 16, None), "scratch too small")):
        assert refused() == 1
        assert re.search(word, gsrast.last_error()), (word, gsrast.last_error())


def test_python_argument_errors():
    import torch
    from gsrast import chamfer, register
    from gsrast.tsdf import TriangleMesh
    pts = torch.zeros((4, 3))
    eye = torch.eye(4, dtype=torch.float64)
    for call in (lambda: register.transform_points(pts, eye), lambda: register.icp(pts, pts, 0.1), lambda: register.fit_transform(pts, pts),
                 lambda: register.evaluate_registration(pts, pts, 0.1, eye), lambda: register.crop_polygon_volume(pts, cases.SQUARE, "Z", 0, 1),
                 lambda: register.correspondence_sums(pts, pts, torch.zeros(4, dtype=torch.int32)), lambda: chamfer.NearestGrid(pts),
                 lambda: TriangleMesh(pts, pts, torch.zeros((1, 3), dtype=torch.int32)).transform(eye)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="max_dist|max_correspondence_distance"):
            register.icp(pts, pts, bad)
    for kw in (dict(relative_fitness=-1e-6), dict(relative_rmse=float("nan")), dict(relative_rmse=float("inf")), dict(relative_fitness="x")):
        with pytest.raises(ValueError, match="relative_"):
            register.icp(pts, pts, 0.1, **kw)
    for it in (-1, 2.5, 3.0, "3", None, True, 4097):
        with pytest.raises(ValueError, match="max_iteration"):
            register.icp(pts, pts, 0.1, max_iteration=it)
    for init in (torch.eye(3), [[1, 2], [3, 4]], torch.full((4, 4), float("nan")), "x", torch.eye(4).tolist()[:3]):
        with pytest.raises(ValueError, match="init"):
            register.icp(pts, pts, 0.1, init=init)
    with pytest.raises(ValueError, match="transformation"):
        register.transform_points(pts, torch.eye(3))
    for axis in ("W", 2, None, "XY"):
        with pytest.raises(ValueError, match="orthogonal_axis"):
            register.crop_polygon_volume(pts, cases.SQUARE, axis, 0, 1)
    for poly in (cases.SQUARE[:2], np.zeros((4, 4)), np.zeros(8), cases.star(1025), np.array([[0, 0], [1, np.nan], [0, 1]])):
        with pytest.raises(ValueError, match="bounding_polygon"):
            register.crop_polygon_volume(pts, poly, "Z", 0, 1)
    with pytest.raises(ValueError, match="NaN"):
        register.crop_polygon_volume(pts, cases.SQUARE, "Z", float("nan"), 1)
    with pytest.raises(RuntimeError, match="record"):
        register.solve_transform(torch.zeros(48, dtype=torch.int64))
