"""tests/glue_truth.py pinned, without a GPU, against the C oracles and the reference-run fixtures -- so that the GPU edge tests
(test_gpu_optim_edges / knn_edges / tsdf_point_edges / plane_prep_edges) read the kernels against references that are themselves held in place --
and the structural claims of tests/glue_cases.py that need no device."""
import numpy as np
import pytest

import glue_cases
import glue_truth
import golden_ref
import oracle
import oracle_multiview as om
import oracle_optim


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_chain_is_the_oracle_chained():
    p, sc, grads = glue_cases.adam_case(37)
    q, m, v = p.copy(), np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        q, m, v = oracle_optim.adam_step(q, g, m, v, t, 1.0, eps=1e-15, lr_scale=sc)
    got = glue_truth.adam_chain(p, grads, 1.0, sc, eps=1e-15)
    assert all(np.array_equal(a, b) for a, b in zip(got, (q, m, v)))
    # continued from a state, with one rate per step
    a = glue_truth.adam_chain(p, grads[:2], [1.0, 0.5], sc, eps=1e-15)
    b = glue_truth.adam_chain(a[0], grads[2:], 0.5, sc, eps=1e-15, m0=a[1], v0=a[2], t0=2)
    c = glue_truth.adam_chain(p, grads, [1.0] + [0.5] * 5, sc, eps=1e-15)
    assert all(np.array_equal(x, y) for x, y in zip(b, c))


@pytest.mark.parametrize("n", glue_cases.ADAM_SIZES)
def test_adam_case_tells_a_wrong_lr_scale_index_from_the_right_one(n):
    """The condition under which the GPU test means anything: the chain run with lr_scale rolled by one element leaves the bound by a factor of ten
    (n = 1 has nothing to roll: there the wrong run is the one that ignores lr_scale)."""
    p, sc, grads = glue_cases.adam_case(n)
    right = glue_truth.adam_chain(p, grads, 1.0, sc, eps=1e-15)[0]
    wrong = glue_truth.adam_chain(p, grads, 1.0, np.roll(sc, 1) if n > 1 else None, eps=1e-15)[0]
    far = np.abs(wrong.astype(np.float64) - right) > 10 * glue_truth.adam_bounds(1.0, sc)
    assert far.all() if n <= 4 else far.mean() >= 0.95, far.mean()


# ------------------------------------------------------------------------------------------------------------------------------ distCUDA2
def test_dist2_bruteforce_equals_the_oracle_exactly():
    for name, pts in glue_cases.knn_inputs().items():
        assert np.array_equal(glue_truth.dist2_bruteforce(pts), oracle.dist2(pts)), name
    r = np.random.default_rng(1)
    big = (r.normal(0, 1, (900, 3)) * 1e19).astype(np.float32)                    # squared distances overflow to inf: never "smaller than FLT_MAX"
    assert np.array_equal(glue_truth.dist2_bruteforce(big), oracle.dist2(big))


def test_dist2_with_fewer_than_three_neighbours():
    ins = glue_cases.knn_inputs()
    assert np.array_equal(glue_truth.dist2_bruteforce(ins["P1"]), [np.inf])
    assert np.array_equal(glue_truth.dist2_bruteforce(ins["P2"]), [np.inf, np.inf])
    d3 = glue_truth.dist2_bruteforce(ins["P3"])
    assert np.isfinite(d3).all() and np.allclose(d3, 1.134e38, rtol=1e-3)
    assert np.isfinite(glue_truth.dist2_bruteforce(ins["P4"])).all()
    assert not glue_truth.dist2_bruteforce(ins["identical600"]).any()


def test_dist2_float64_neighbours_agree_with_float32_values():
    pts = glue_cases.knn_inputs()["P513"]
    idx, d2 = glue_truth.dist2_neighbours64(pts)
    assert idx.shape == (513, 3) and (idx != np.arange(513)[:, None]).all()
    np.testing.assert_allclose(d2.mean(axis=1), glue_truth.dist2_bruteforce(pts), rtol=1e-5)


def test_cluster_case_has_its_third_neighbour_in_another_box():
    """The claim of knn_cluster_case, on the float64 neighbours and the restated Morton boxes: two boxes; each pair point's nearest is its twin; for at
    least one pair point of each pair the THIRD neighbour lies outside its own box."""
    pts = glue_cases.knn_cluster_case()
    box, order = glue_cases.morton_boxes(pts)
    assert pts.shape == (512, 3) and set(box.tolist()) == {0, 1} and sorted(order.tolist()) == list(range(512))
    idx, d2 = glue_truth.dist2_neighbours64(pts)
    assert [int(idx[i, 0]) for i in range(4)] == [1, 0, 3, 2] and (d2[:4, 0] < 1.1e-6).all() and (d2[:4, 1] > 1.5 ** 2).all()
    crossing = [i for i in range(4) if box[idx[i, 2]] != box[i]]
    assert {i // 2 for i in crossing} == {0, 1}, crossing


def test_morton_boxes_of_degenerate_clouds():
    ins = glue_cases.knn_inputs()
    box, order = glue_cases.morton_boxes(ins["identical600"])
    assert np.array_equal(order, np.arange(600))                                  # one code: the stable sort keeps the input order
    assert np.array_equal(box, np.arange(600) // 256)


# ------------------------------------------------------------------------------------------------------------------------------ TSDF
def _oracle_tsdf(pts, cams, depth, rgb, trunc):
    V = pts.shape[0]
    t = np.ones(V, np.float32); w = np.ones(V, np.float32); c = np.zeros((V, 3), np.float32)
    for cam, d, col in zip(cams, depth, rgb):
        if np.ndim(trunc):
            oracle.tsdf_integrate(pts, cam["projmatrix"], d, col, 0.0, t, w, c, trunc_pp=trunc)
        else:
            oracle.tsdf_integrate(pts, cam["projmatrix"], d, col, trunc, t, w, c)
    return t, w, c


@pytest.mark.parametrize("per_point", [False, True])
@pytest.mark.parametrize("V", [8, 1027])
def test_tsdf_frame_agrees_with_the_oracle(V, per_point):
    """Weights exactly (the float32 decisions are the oracle's own expressions); values within 1e-4, the project's bound for this update: float32 (d - z)
    cancellation at depth 5 (ulp 4.8e-7, a few of them) divided by a truncation of at least 0.1."""
    trunc = glue_cases.tsdf_trunc_pp(V) if per_point else glue_cases.TSDF_TRUNC
    pts, cams, depth, rgb, (t, w, c), info = glue_cases.tsdf_truth(V, 2, trunc)
    ot, ow, oc = _oracle_tsdf(pts, cams, depth, rgb, trunc)
    assert np.array_equal(ow, w)
    assert np.abs(ot - t).max() < 1e-4 and np.abs(oc - c).max() < 1e-4, (np.abs(ot - t).max(), np.abs(oc - c).max())
    assert (w > 1).mean() >= 0.25


@pytest.mark.parametrize("V", [v for v in glue_cases.TSDF_SIZES if v >= 8])
def test_tsdf_scene_has_every_kind_of_point(V):
    for trunc in (glue_cases.TSDF_TRUNC, glue_cases.tsdf_trunc_pp(V)):
        _check_tsdf_kinds(*glue_cases.tsdf_truth(V, 1, trunc)[4:])


def _check_tsdf_kinds(state, info):
    """At least a quarter of the points updated; at least one point outside the frustum, one behind the camera, one behind the surface beyond the
    truncation, and one updated point whose float32 pixel column is exactly W - 1."""
    t, w, c = state
    upd = info["updated"]
    assert np.array_equal(w > 1, upd) and upd.mean() >= 0.25
    assert (info["behind"]).any()
    assert (~info["in_frustum"] & ~info["behind"]).any()
    assert (info["in_frustum"] & ~(info["sdf32"] > -info["trunc32"])).any()
    assert (upd & (info["x_pix"] == glue_cases.TSDF_W - 1)).any()


def test_tsdf_frame_matches_reference_run():
    """The ref_tsdf_unbounded fixture (compute_unbounded_tsdf through extract_mesh_unbounded, 3 frames): the adaptive-truncation pass and the texturing
    pass, with tests/test_golden_ref_cpu.py's bounds."""
    z = golden_ref.load("ref_tsdf_unbounded")
    V = z["points"].shape[0]
    t = np.ones(V); w = np.ones(V); c = np.zeros((V, 3))
    for F, d, col in zip(z["full_proj"], z["depth"], z["rgb"]):
        glue_truth.tsdf_frame(z["points"], F, d, col, z["sdf_trunc"], t, w, c)
    assert np.abs(t - z["tsdf"]).max() < 2e-4 and (t != 1).mean() > 0.2
    Vv = z["verts"].shape[0]
    t = np.ones(Vv); w = np.ones(Vv); c = np.zeros((Vv, 3))
    for F, d, col in zip(z["full_proj"], z["depth"], z["rgb"]):
        glue_truth.tsdf_frame(z["verts"], F, d, col, 5 * float(z["voxel_size"]), t, w, c)
    assert np.abs(c - z["vert_rgb"]).max() < 2e-4 and (c != 0).mean() > 0.2


# ------------------------------------------------------------------------------------------------------------------------------ plane all_map
def test_plane_allmap_autograd_matches_reference_run():
    z = golden_ref.load("ref_plane_allmap")
    t = glue_truth.plane_allmap_autograd(z["means3D"], z["rotations"], z["scales"], z["viewmatrix"], z["campos"], z["dL_dall_map"])
    np.testing.assert_allclose(t["all_map"], z["all_map"], rtol=2e-5, atol=2e-6)
    assert (t["all_map"][:, 3] == 1).all()
    assert np.abs(t["d_xyz"] - z["d_means3D"]).max() <= 2e-5 * np.abs(z["d_means3D"]).max()
    assert np.abs(t["d_q"] - z["d_rotations"]).max() <= 5e-5 * np.abs(z["d_rotations"]).max()


@pytest.mark.parametrize("cols", [3, 6])
def test_plane_allmap_autograd_agrees_with_the_oracle(cols):
    xyz, q, sc, V, cp, dL = glue_cases.plane_random(1000, cols)
    t = glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp, dL)
    assert glue_cases.plane_margins_ok(t, sc).all()
    assert 0.2 < (t["dot"] < 0).mean() < 0.8 and set(t["k"].tolist()) == {0, 1, 2}
    am, dx, dq = om.plane_allmap(xyz, q, sc[:, :3], V, cp, dL)
    np.testing.assert_allclose(am, t["all_map"], rtol=2e-5, atol=2e-6)
    assert np.abs(dx - t["d_xyz"]).max() <= 2e-5 * np.abs(t["d_xyz"]).max()
    assert np.abs(dq - t["d_q"]).max() <= 5e-5 * np.abs(t["d_q"]).max()


def test_plane_edge_rows_are_exact_and_sit_on_their_edges():
    xyz, q, sc, V, camposes, tags, want_k = glue_cases.plane_edge_rows()
    g4 = np.zeros((xyz.shape[0], 5), np.float32); g4[:, 4] = 1.0
    seen = {"dot0_sd_nonzero": 0, "sd0_dot_nonzero": 0, "both0": 0, "flip": 0}
    for cp in camposes:
        t = glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp, g4)
        am = om.plane_allmap(xyz, q, sc, V, cp)
        assert np.array_equal(am.astype(np.float64), t["all_map"])                 # exact in float32: the oracle gives the float64 value
        assert np.array_equal(t["k"], want_k)                                      # the first minimum
        seen["dot0_sd_nonzero"] += int(((t["dot"] == 0) & (t["sd"] != 0)).sum()); seen["sd0_dot_nonzero"] += int(((t["sd"] == 0) & (t["dot"] != 0)).sum())
        seen["both0"] += int(((t["dot"] == 0) & (t["sd"] == 0)).sum()); seen["flip"] += int((t["dot"] < 0).sum())
        zero = t["sd"] == 0
        assert not t["d_xyz"][zero].any() and not t["d_q"][zero].any()            # |.| sends nothing through at 0
        assert (t["all_map"][zero, 4] == 0).all()
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------------------------ densification statistics
def test_densify_stats_matches_reference_run():
    z = golden_ref.load("ref_densify_stats")
    for tag, names in (("vanilla", ("max_radii2D", "xyz_gradient_accum", "denom")),
                       ("pgsr", ("max_radii2D", "xyz_gradient_accum", "denom", "xyz_gradient_accum_abs", "denom_abs"))):
        a = {n: z["init_" + n].reshape(-1).astype(np.float32).copy() for n in names}
        if tag == "vanilla":
            glue_truth.densify_stats(z["visibility_filter"], z["radii"], z["grad"], a["max_radii2D"], a["xyz_gradient_accum"], a["denom"])
        else:
            glue_truth.densify_stats(z["visibility_filter"], z["radii"], z["grad"], a["max_radii2D"], a["xyz_gradient_accum"], a["denom"], z["out_observe"],
                                     z["grad_abs"], a["xyz_gradient_accum_abs"], a["denom_abs"])
        for n in names:
            np.testing.assert_allclose(a[n], z[f"{tag}_{n}"].reshape(-1), rtol=1e-6, atol=1e-6, err_msg=f"{tag}:{n}")


@pytest.mark.parametrize("filt", ["none", "all", "random"])
def test_densify_stats_agrees_with_the_oracle(filt):
    for P in glue_cases.DENSIFY_SIZES:
        for stride in (2, 3, 4):
            for use_obs in (False, True):
                c = glue_cases.densify_case(P, filt)
                names = ("max_radii2D", "accum", "denom", "accum_abs", "denom_abs")
                a = {n: c[n].copy() for n in names}; b = {n: c[n].copy() for n in names}
                g, ga = np.ascontiguousarray(c["grad"][:, :stride]), np.ascontiguousarray(c["grad_abs"][:, :stride])
                ob = c["observe"] if use_obs else None
                for _ in range(2):
                    glue_truth.densify_stats(c["filter"], c["radii"], g, a["max_radii2D"], a["accum"], a["denom"], ob, ga, a["accum_abs"], a["denom_abs"])
                    om.densify_stats(c["filter"], c["radii"], g, b["max_radii2D"], b["accum"], b["denom"], ob, ga, b["accum_abs"], b["denom_abs"])
                for n in names:
                    assert np.array_equal(a[n], b[n]), (P, stride, use_obs, n)
                    assert np.isfinite(a[n]).all()
                    if filt == "none":
                        assert np.array_equal(a[n], c[n]), (P, n)                  # an all-false filter leaves everything as it was
                assert filt == "none" or P == 1 or not np.array_equal(a["denom"], c["denom"])
