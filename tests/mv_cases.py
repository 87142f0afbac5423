"""Seeded two-view inputs for the PGSR multi-view losses: two cameras looking at a textured world plane, analytic plane depth / normal /
distance / gray texture, with a smooth depth perturbation so that the reprojection error straddles the noise threshold.

`plane_pair` is the generic scene; `make(name)` the named edge cases of tests/test_mv_truth_cpu.py and tests/test_gpu_mvloss_edges.py (near
size and intrinsics of their own, ncc_scale != 1 with the gray images at floor(W/s) x floor(H/s), every patch size, sample lists with unused
slots / weight-0 pixels / image corners, the border columns of k_mv_geo with depths solved in float64, identical cameras, degenerate inputs)."""
import functools
import math
import types

import numpy as np

import scenes


def _view(W, H, yaw, t, n_w, c_w, phase, amp, fscale=0.9, tex=1.0, gray_size=None, s=1.0, contrast=1.0):
    cam = scenes.make_camera(W, H, fscale * W, fscale * W, yaw_deg=yaw, t=t)
    wvt = cam["viewmatrix"].astype(np.float64)
    R, T = wvt[:3, :3].copy(), wvt[3, :3].copy()
    c = dict(R=R, T=T, Fx=fscale * W, Fy=fscale * W, Cx=0.5 * W, Cy=0.5 * H)
    n_c = n_w @ R; c_c = c_w + n_c @ T

    def on_plane(xx, yy):
        ray = np.stack([(xx - c["Cx"]) / c["Fx"], (yy - c["Cy"]) / c["Fy"], np.ones_like(xx)], -1)
        d0 = c_c / (ray @ n_c)
        return ray, d0, (ray * d0[..., None] - T) @ R.T

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ray, d0, Xw = on_plane(xx, yy)
    Wg, Hg = gray_size or (W, H)
    gy, gx = np.mgrid[0:Hg, 0:Wg].astype(np.float64)
    _, _, Xg = on_plane(gx * s, gy * s)              # gray texel (i, j) shows what full-resolution pixel (i s, j s) sees
    a, b = Xg[..., 0], Xg[..., 1]
    gray = 0.5 + contrast * (0.2 * np.sin(5 * tex * a) + 0.2 * np.cos(7 * tex * b) + 0.1 * np.sin(11 * tex * (a + b)))
    depth = d0 * (1 + amp * np.sin(xx / 5.0 + phase) * np.cos(yy / 4.0))
    sgn = -1.0 if (ray[H // 2, W // 2] @ n_c) > 0 else 1.0
    return c, depth.astype(np.float32), (sgn * n_c).astype(np.float32), float(abs(c_c)), gray.astype(np.float32)


def plane_pair(W=72, H=54, seed=0, amp=0.12, near_yaw=-5.0, near_t=(-0.25, 0.04, 0.03), tex=1.0, near_size=None, ncc_scale=1.0, contrast=1.0,
               patch=3, noise_th=1.0, gray_size=None, gray_noise=0.0):
    r = np.random.default_rng(seed)
    n_w = np.array([0.12, -0.2, -1.0]) + r.normal(0, 0.05, 3); n_w /= np.linalg.norm(n_w)
    c_w = float(n_w @ np.array([0.0, 0.0, 3.0]))
    Wn, Hn = near_size or (W, H)
    gs = gray_size or (int(math.floor(W / ncc_scale)), int(math.floor(H / ncc_scale)))
    vc, dv, nv, distv, gv = _view(W, H, 4.0, (0.05, 0.0, 0.0), n_w, c_w, 0.0, amp, tex=tex, gray_size=gs, s=ncc_scale, contrast=contrast)
    nc, dn, _, _, gn = _view(Wn, Hn, near_yaw, near_t, n_w, c_w, 1.3, amp, tex=tex, gray_size=gs, s=ncc_scale, contrast=contrast)
    normal = (nv[:, None, None] + r.normal(0, 0.01, (3, H, W))).astype(np.float32)
    dist = (distv * (1 + r.normal(0, 0.002, (H, W)))).astype(np.float32)
    if gray_noise:                     # independent sensor noise, in units of the texture's contrast: keeps ncc off its floor at 0
        gn = (gn + contrast * gray_noise * r.normal(0, 1, gn.shape)).astype(np.float32)
    return dict(W=W, H=H, view=vc, near=nc, plane_depth=dv[None], near_plane_depth=dn[None], rendered_normal=normal, rendered_distance=dist[None],
                gray=gv[None], near_gray=gn[None], ncc_scale=float(ncc_scale), patch=patch, noise_th=noise_th)


def cam_ns(c, ncc_scale=1.0):
    return types.SimpleNamespace(**c, ncc_scale=ncc_scale)


# ------------------------------------------------------------------------------------------------------------------------- sample lists
def sample_list(case, N, seed=0):
    """N slots: the four image corners and the middle of each edge first (their reference taps hit the zero padding), then distinct random
    pixels of the WHOLE image (so that some lie outside d_mask: weight 0), every fifth slot unused (-1).  No pixel twice."""
    W, H = case["W"], case["H"]
    r = np.random.default_rng(1000 + seed)
    first = [0, W - 1, (H - 1) * W, H * W - 1, W // 2, (H // 2) * W, (H // 2) * W + W - 1, (H - 1) * W + W // 2]
    rest = [int(p) for p in r.permutation(W * H) if int(p) not in set(first)]
    pool = first + rest
    out, k = [], 0
    for i in range(N):
        if i % 5 == 4 and N > 1:
            out.append(-1)
        else:
            out.append(pool[k]); k += 1
    return np.asarray(out, np.int32)


# ------------------------------------------------------------------------------------------------------- the border columns of k_mv_geo
BORDER_WN, BORDER_HN = 24, 12
_EPS_OUT = 4e-6           # "just outside": a few float32 ulps of a coordinate of this size beyond the frustum edge
# target coordinate per column.  Half- and quarter-cell offsets are robust; the others sit on a decision (tie) on purpose.
BORDER_TARGETS = [-1.5, -0.5, -_EPS_OUT, 0.0, 0.5, 1.5, 2.25, 3.0, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 10.0, 10.5, 11.5, 12.5, 13.5, 14.5, 15.5,
                  16.5, 18.5, 20.5, 22.5, BORDER_WN - 1.0, BORDER_WN - 0.5, float(BORDER_WN), BORDER_WN + _EPS_OUT, BORDER_WN + 0.5, BORDER_WN + 1.5]
BORDER_TIED_LINES = 8
BORDER_TIES = {2: "frustum", 3: "frustum", 7: "cell", 15: "cell", 26: "clamp", 28: "frustum", 29: "frustum"}      # column -> gate it sits on


def border(axis):
    """Identity relative rotation, unit translation along `axis` (0: x, 1: y), focal lengths 64 / 32 (powers of two), the neighbour's principal
    point outside its image at -10 so that every target is reached with a positive depth: along the axis the projection is
    u = (x - 16) / 2 - 10 + 32 / d, so column (row) k gets d = 32 / (target_k + 10 - (k - 16) / 2), solved in float64 and rounded to float32.
    Across the axis the projection is v = j / 2 + 2.25: quarter-cell offsets, robust.  The neighbour's depth map follows the solved depths to
    a few per cent, so that the reprojection error stays below noise_th = 4."""
    n, m = 32, 16                                                  # pixels along / across the axis
    k = np.arange(n, dtype=np.float64)
    tgt = np.asarray(BORDER_TARGETS, np.float64)
    d = 32.0 / (tgt + 10.0 - (k - 16.0) / 2.0)
    assert (d > 0.5).all() and (np.diff(tgt) > 0).all()
    # a tied column holds its tie in the first eight lines across only; the other eight take a robust target a quarter cell away, so that the
    # near-map texels they feed are shared with no tied pixel and their scatter can be held to the truth
    alt = np.where(np.isin(k, list(BORDER_TIES)), np.where(tgt < 12, tgt + 0.25, tgt - 0.25), tgt)
    tgt2 = np.where(np.arange(m)[:, None] < BORDER_TIED_LINES, tgt[None, :], alt[None, :])
    depth = 32.0 / (tgt2 + 10.0 - (k[None, :] - 16.0) / 2.0)
    i = np.arange(BORDER_WN, dtype=np.float64)
    D = np.interp(i, tgt, d)
    j = np.arange(BORDER_HN, dtype=np.float64)
    near_map = D[None, :] * (1 + 0.02 * np.sin(1.3 * i[None, :] + 0.7 * j[:, None]))          # [across, along]
    eye = np.eye(3)
    T = np.zeros(3); T[axis] = 1.0
    if axis == 0:
        W, H, Wn, Hn = n, m, BORDER_WN, BORDER_HN
        view = dict(R=eye, T=np.zeros(3), Fx=64.0, Fy=64.0, Cx=16.0, Cy=8.0)
        near = dict(R=eye, T=T, Fx=32.0, Fy=32.0, Cx=-10.0, Cy=6.25)
        pd, nd = depth, near_map
    else:
        W, H, Wn, Hn = m, n, BORDER_HN, BORDER_WN
        view = dict(R=eye, T=np.zeros(3), Fx=64.0, Fy=64.0, Cx=8.0, Cy=16.0)
        near = dict(R=eye, T=T, Fx=32.0, Fy=32.0, Cx=6.25, Cy=-10.0)
        pd, nd = depth.T, near_map.T
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.random.default_rng(5)
    normal = (np.array([0.05, -0.1, -1.0])[:, None, None] + r.normal(0, 0.01, (3, H, W))).astype(np.float32)
    gray = (0.5 + 0.3 * np.sin(0.9 * xx) * np.cos(0.7 * yy)).astype(np.float32)
    return dict(W=W, H=H, view=view, near=near, plane_depth=np.ascontiguousarray(pd, np.float32)[None],
                near_plane_depth=np.ascontiguousarray(nd, np.float32)[None], rendered_normal=normal,
                rendered_distance=np.full((1, H, W), 3.0, np.float32), gray=gray[None], near_gray=gray[None].copy(), ncc_scale=1.0, patch=1, noise_th=4.0,
                axis=axis, ties={c: g for c, g in BORDER_TIES.items()})


def border_line(case, pix):
    """column (axis 0) or row (axis 1) index of flat pixel indices: the position in BORDER_TARGETS"""
    return np.asarray(pix) % case["W"] if case["axis"] == 0 else np.asarray(pix) // case["W"]


def tied_pixels(case):
    """bool [W*H]: the pixels placed on a decision on purpose (none outside the border cases)"""
    pix = np.arange(case["W"] * case["H"])
    if "ties" not in case:
        return np.zeros(pix.size, bool)
    across = pix // case["W"] if case["axis"] == 0 else pix % case["W"]
    return np.isin(border_line(case, pix), list(case["ties"])) & (across < BORDER_TIED_LINES)


# ------------------------------------------------------------------------------------------------------------------ degenerate inputs
def degenerate():
    """-> (base, planted, rows).  `planted` is the default scene with inputs that must switch a pixel / sample off; in `base` the same pixels
    are switched off by ordinary means (plane_depth = -1: behind the neighbour, q.z < 0.1; the sample slot unused), so that the two runs must
    agree bit for bit everywhere else.  rows: name -> flat pixel index (geo) or sample slot (ncc)."""
    base = plane_pair(seed=2)
    W, H = base["W"], base["H"]
    planted = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    base = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    A = base["view"]["R"].T @ base["near"]["R"]; b = base["near"]["T"] - base["view"]["T"] @ A
    rows = {}
    geo_pix = {"depth_zero": (20, 20), "depth_negative": (22, 20), "depth_nan": (24, 20), "depth_inf": (26, 20), "qz_zero": (28, 20), "qz_below": (30, 20)}
    val = {"depth_zero": 0.0, "depth_negative": -0.7, "depth_nan": np.nan, "depth_inf": np.inf}
    for name, (x, y) in geo_pix.items():
        p = y * W + x
        rows[name] = p
        if name.startswith("qz"):
            rx, ry = (x - base["view"]["Cx"]) / base["view"]["Fx"], (y - base["view"]["Cy"]) / base["view"]["Fy"]
            target = 0.0 if name == "qz_zero" else 0.05
            v = (target - b[2]) / (rx * A[0, 2] + ry * A[1, 2] + A[2, 2])
        else:
            v = val[name]
        planted["plane_depth"].reshape(-1)[p] = v
        base["plane_depth"].reshape(-1)[p] = -1.0
    # a NaN texel of the neighbour's depth map: the pixels whose bilinear footprint may hold it (projection within one cell of it, a hair
    # added) keep their depth in `planted`, valid but for the NaN, and are switched off by depth -1 in `base`
    Hn, Wn = base["near_plane_depth"].shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = planted["plane_depth"][0].astype(np.float64)
    nd = base["near_plane_depth"][0].astype(np.float64)
    Ai = base["near"]["R"].T @ base["view"]["R"]; bi = base["view"]["T"] - base["near"]["T"] @ Ai
    with np.errstate(all="ignore"):
        pc = np.stack([(xx - base["view"]["Cx"]) / base["view"]["Fx"] * d, (yy - base["view"]["Cy"]) / base["view"]["Fy"] * d, d], -1)
        q = pc @ A + b
        u, v = q[..., 0] * base["near"]["Fx"] / q[..., 2] + base["near"]["Cx"], q[..., 1] * base["near"]["Fy"] / q[..., 2] + base["near"]["Cy"]
        inside = (u > 1) & (u < Wn - 2) & (v > 1) & (v < Hn - 2) & (q[..., 2] > 0.2)
        uc, vc = np.clip(np.nan_to_num(u), 0, Wn - 2), np.clip(np.nan_to_num(v), 0, Hn - 2)
        x0, y0 = np.floor(uc).astype(int), np.floor(vc).astype(int)
        ax, ay = uc - x0, vc - y0
        mz = nd[y0, x0] * (1 - ax) * (1 - ay) + nd[y0, x0 + 1] * ax * (1 - ay) + nd[y0 + 1, x0] * (1 - ax) * ay + nd[y0 + 1, x0 + 1] * ax * ay
        r = (q / q[..., 2:3] * mz[..., None]) @ Ai + bi
        noise = np.hypot(r[..., 0] * base["view"]["Fx"] / r[..., 2] + base["view"]["Cx"] - xx, r[..., 1] * base["view"]["Fy"] / r[..., 2] + base["view"]["Cy"] - yy)
    valid = inside & (noise < 0.8)                       # valid with room to spare: in the frustum, reprojection error well below the threshold 1
    # the texel nearest the middle of the map that at least three such pixels tap
    best = None
    for ty in range(2, Hn - 2):
        for tx in range(2, Wn - 2):
            f = (np.abs(u - tx) < 1.001) & (np.abs(v - ty) < 1.001)
            if (f & valid).sum() >= 3 and (best is None or abs(tx - Wn / 2) + abs(ty - Hn / 2) < best[0]):
                best = (abs(tx - Wn / 2) + abs(ty - Hn / 2), tx, ty, np.nonzero(f.reshape(-1))[0])
    _, tx, ty, feeders = best
    planted["near_plane_depth"][0, ty, tx] = np.nan
    base["plane_depth"].reshape(-1)[feeders] = -1.0
    rows["near_nan_texel"] = ty * Wn + tx
    rows["near_nan_feeders"] = feeders
    # NCC rows: sample slots 3 and 6 of the list of degenerate_indices()
    idx = degenerate_indices(base)
    pd, pn = int(idx[3]), int(idx[6])
    assert pd >= 0 and pn >= 0
    planted["rendered_distance"].reshape(-1)[pd] = 0.0
    planted["rendered_normal"].reshape(3, -1)[1, pn] = np.nan
    rows["dist_zero_slot"], rows["normal_nan_slot"] = 3, 6
    base_idx = idx.copy(); base_idx[[3, 6]] = -1
    base["indices"], planted["indices"] = base_idx, idx
    return base, planted, rows


def degenerate_indices(case):
    return sample_list(case, 40, seed=3)


# ----------------------------------------------------------------------------------------------------------------------- named cases
def _constant_patch(case, p, half):
    """gray made constant over the reference patch of pixel p (and a margin): rvar == 0 there"""
    W = case["W"]
    x, y = p % W, p // W
    case["gray"][0, max(y - half - 1, 0):y + half + 2, max(x - half - 1, 0):x + half + 2] = 0.5
    return case


GN = 0.1          # gray_noise of the new cases (the texture's own deviation is 0.2): ncc of a good match sits near 1e-1, clear of 0 and of 0.9
SPECS = {
    # name: (plane_pair arguments, number of sample slots or None = every pixel of the truth's d_mask)
    "default": (dict(gray_noise=GN), None),
    "near_50x38": (dict(near_size=(50, 38), seed=1, gray_noise=GN), None),
    "near_64x48_of_33x17": (dict(W=33, H=17, near_size=(64, 48), gray_size=(64, 48), seed=2, patch=1, gray_noise=GN), None),
    "scale2_patch2": (dict(ncc_scale=2.0, patch=2, seed=3, gray_noise=GN), None),
    "scale1p5_near_50x38": (dict(near_size=(50, 38), ncc_scale=1.5, seed=5, gray_noise=GN), None),
    "low_contrast": (dict(W=48, H=36, contrast=0.06, seed=6, gray_noise=GN), None),
    "patch0": (dict(W=48, H=36, patch=0, seed=7), 17),
    "patch1_n1": (dict(W=48, H=36, patch=1, seed=7, gray_noise=GN), 1),
    "patch2_n15": (dict(W=48, H=36, patch=2, seed=8, gray_noise=GN), 15),
    "patch3_n16": (dict(W=48, H=36, patch=3, seed=8, gray_noise=GN), 16),
    "patch4_n17": (dict(W=48, H=36, patch=4, seed=9, gray_noise=GN), 17),
    "patch8_n17": (dict(W=48, H=36, patch=8, seed=9, gray_noise=GN), 17),
    "n4097": (dict(W=96, H=64, seed=10, tex=2.0, gray_noise=GN), 4097),
    "shifted_near": (dict(W=64, H=48, seed=4, near_t=(-1.6, 0.3, 0.0), noise_th=1e9, gray_noise=GN), 600),
    "constant_patch": (dict(W=48, H=36, seed=11, gray_noise=GN), 16),
}
NAMES = tuple(SPECS) + ("border_u", "border_v", "identical")
MAX_FRAGILE, MAX_VALUE_FRAGILE_SAMPLES, MAX_GRAD_FRAGILE_SAMPLES = 0.02, 0.01, 0.05


@functools.lru_cache(maxsize=None)
def make(name):
    """-> case dict (arrays must not be modified) with `indices` (int32 sample slots) or None"""
    if name in ("border_u", "border_v"):
        case = border(0 if name == "border_u" else 1)
        case["indices"] = sample_list(case, 33, seed=1)
    elif name == "identical":
        case = plane_pair(W=40, H=30, seed=12)
        case["near"] = case["view"]
        case["near_plane_depth"] = case["plane_depth"].copy()
        case["near_gray"] = case["gray"].copy()
        case["indices"] = sample_list(case, 16, seed=2)
    else:
        kw, n = SPECS[name]
        case = plane_pair(**kw)
        case["indices"] = None if n is None else sample_list(case, n, seed=len(name))
        if name == "constant_patch":
            _constant_patch(case, int(case["indices"][9]), case["patch"])
    case["name"] = name
    return case
