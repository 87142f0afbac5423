"""Scenes that reach the branches of the per-Gaussian stages (csrc/gsr_preprocess.hip, gsr_math.h) that scenes.make_scene never enters.
TEST INFRASTRUCTURE ONLY; pure numpy, deterministic.

make_scene draws camera-space z ~ U[1, 20], |x/z|, |y/z| <= 1.1 tanfov and unit quaternions.  The builders below keep its camera (pose 0: the view
matrix is the identity, world space is camera space) and overwrite the fields that decide a branch:

  beyond_clamp     splats whose centre lies at 1.35 ... 1.7 tanfov, beyond the 1.3 tanfov clamp of the EWA / PLANE Jacobian (cov2d_project) and its
                   backward masks; large enough (14 px sigma) to reach into the image from there
  near_plane       depths on both sides of the p_view.z <= 0.2f cull, to the float, and right behind it where 1/z ... 1/z^3 are large
  raw_quaternions  |q| in [0.5, 2]: EWA / PLANE build Sigma from the raw quaternion, the surfel normalises
  truncated_size   surfels at an image size where the backward's float32 re-derivation of W, H truncates to W - 1, H - 1

Each returns (scene, out_grads, groups); groups maps a name to a boolean row mask over the Gaussians (tests/parity_truth.py check_case row_groups).
tests/test_pregauss_cases_cpu.py asserts on the oracles alone that every scene meets the condition it was built for."""
import numpy as np

import scenes

W, H = 96, 64
BG = (0.2, 0.4, 0.6)
F32 = np.float32
NEAR = F32(0.2)                                   # the cull compares p_view.z <= 0.2f
# class name -> depth; the first three are culled (z <= 0.2f), the rest rendered
NEAR_Z = {"z0.19": F32(0.19), "below": np.nextafter(NEAR, F32(0)), "z0.2f": NEAR, "above": np.nextafter(NEAR, F32(1)), "z0.21": F32(0.21),
          "z0.25": F32(0.25), "z0.3": F32(0.3), "z0.5": F32(0.5)}
NEAR_CULLED = ("z0.19", "below", "z0.2f")


def _place(sc, u, v, z):
    """Direction (u, v) in units of tanfov at depth z -> means3D (pose 0: world space is camera space)."""
    assert np.array_equal(sc["viewmatrix"], np.eye(4, dtype=F32))
    return np.stack([u * sc["tanfovx"] * z, v * sc["tanfovy"] * z, z], -1).astype(F32)


def _finish(sc, variant, rng, sigma_px, z):
    """Pixel sigma sigma_px * U[0.5, 1] per axis (PLANE: third axis x 0.1), opacities U[0.05, 0.3], all_map rebuilt."""
    P = z.shape[0]
    nax = 2 if variant == "surfel" else 3
    s = (sigma_px * z / sc["fx"])[:, None] * rng.uniform(0.5, 1.0, (P, nax))
    if variant == "plane":
        s[:, 2] *= 0.1
    sc["scales"] = s.astype(F32)
    sc["opacities"] = rng.uniform(0.05, 0.3, (P, 1)).astype(F32)
    if variant == "plane":
        sc["all_map"] = scenes.plane_all_map(sc)
    return sc


def beyond_clamp(variant):
    P = 400
    sc = scenes.make_scene(variant, P, W, H, seed=1, sigma_px=14.0, bg=BG)
    rng = np.random.default_rng(21)               # (a draw at which each clamped group, the corner one included, carries >= 10 % of the geometric gradients)
    z = rng.uniform(1.0, 6.0, P)
    u = rng.uniform(-1.0, 1.0, P); v = rng.uniform(-1.0, 1.0, P)
    k = np.arange(P) % 4                          # 0 inside, 1 x beyond the clamp, 2 y, 3 both
    su = rng.choice([-1.0, 1.0], P); sv = rng.choice([-1.0, 1.0], P)
    u = np.where((k == 1) | (k == 3), su * rng.uniform(1.35, 1.7, P), u)
    v = np.where((k == 2) | (k == 3), sv * rng.uniform(1.35, 1.7, P), v)
    sc["means3D"] = _place(sc, u, v, z)
    _finish(sc, variant, rng, 14.0, z)
    og = scenes.random_out_grads(variant, W, H, seed=1, scale=1.0)
    return sc, og, dict(inside=k == 0, x_clamped=k == 1, y_clamped=k == 2, both_clamped=k == 3)


def near_plane(variant, color_mode):
    P = 256
    sc = scenes.make_scene(variant, P, W, H, seed=2, sigma_px=4.0, bg=BG, color_mode=color_mode, sh_degree=3)
    if color_mode == "sh":
        sc["shs"][:, 1:] *= 8.0                   # the higher bands carry weight, as in test_sh_degrees_and_coefficient_counts
    rng = np.random.default_rng(6)
    names = list(NEAR_Z)
    cls = np.arange(P) % len(names)
    z32 = np.array([NEAR_Z[n] for n in names], F32)[cls]
    z = z32.astype(np.float64)
    u = rng.uniform(-0.9, 0.9, P); v = rng.uniform(-0.9, 0.9, P)
    sc["means3D"] = _place(sc, u, v, z)
    sc["means3D"][:, 2] = z32                     # the float itself: p_view.z is exactly it under the identity view matrix
    q = np.concatenate([np.ones((P, 1)), rng.uniform(-0.15, 0.15, (P, 3))], 1)      # facing the camera, tilted a little
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    _finish(sc, variant, rng, 4.0, z)
    og = scenes.random_out_grads(variant, W, H, seed=1, scale=1.0)
    return sc, og, {n: cls == i for i, n in enumerate(names)}


def without_rows(sc, drop):
    """The scene without the Gaussians of the row mask `drop`."""
    P = sc["means3D"].shape[0]
    return {k: (v[~drop] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == P and k not in ("bg", "campos") else v) for k, v in sc.items()}


def raw_quaternions(variant):
    P = 400
    sc = scenes.make_scene(variant, P, W, H, seed=3, sigma_px=4.0, bg=BG)
    rng = np.random.default_rng(8)
    sc["rotations"] = (sc["rotations"] * rng.uniform(0.5, 2.0, (P, 1))).astype(F32)
    sc["opacities"] = rng.uniform(0.05, 0.3, (P, 1)).astype(F32)
    if variant == "plane":
        sc["all_map"] = scenes.plane_all_map(sc)
    n = np.linalg.norm(sc["rotations"].astype(np.float64), axis=1)
    og = scenes.random_out_grads(variant, W, H, seed=1, scale=1.0)
    return sc, og, dict(short=n < 0.8, long=n > 1.25, near_unit=(n >= 0.8) & (n <= 1.25))


def unit_quaternions(sc):
    """The scene with rotations / |q|, rounded to float32."""
    q = sc["rotations"].astype(np.float64)
    return dict(sc, rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32))


def backward_size(sc):
    """(Wb, Hb) as k_preprocess_bwd_surfel re-derives them: (int)(fx * tanfovx * 2) with fx = W / (2 tanfovx), every operation in float32."""
    out = []
    for n, tan in ((sc["W"], F32(sc["tanfovx"])), (sc["H"], F32(sc["tanfovy"]))):
        f = F32(n) / (F32(2.0) * tan)
        out.append(int(F32(F32(f * tan) * F32(2.0))))
    return tuple(out)


TRUNCATED_SIZES = [(63, 31), (64, 48)]            # Wb, Hb = 62, 30 at the first; the second is the control


def truncated_size(Wt, Ht):
    """-> (scene, out_grads, groups, (Wb, Hb)); surfel."""
    P = 300
    sc = scenes.make_scene("surfel", P, Wt, Ht, seed=4, sigma_px=3.0, bg=BG)
    rng = np.random.default_rng(9)
    sc["opacities"] = rng.uniform(0.05, 0.3, (P, 1)).astype(F32)
    og = scenes.random_out_grads("surfel", Wt, Ht, seed=4, scale=1.0)
    return sc, og, dict(all=np.ones(P, bool)), backward_size(sc)
