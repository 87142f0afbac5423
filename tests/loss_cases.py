"""Inputs of the image-space loss tests (tests/loss_truth.py, test_loss_truth_cpu.py, test_gpu_loss_edges.py): numpy only, deterministic.
Every structural claim a builder makes is returned with the case (`claims`) and asserted by test_loss_truth_cpu.py.

SSIM: the kernels tile 32 wide x 30 high with a halo of 5 under an 11-tap window; the shapes put one-row / one-column tiles behind the seams, an
exact tile, images smaller than the window, and single rows / columns.  The geometric losses tile 64 x 4 with a halo of 2; the shapes do the
same there and add the four without an interior pixel."""
import numpy as np

f32 = np.float32

# --------------------------------------------------------------------------------------------------------------------------------- SSIM
SSIM_MAIN = (1, 61, 65)               # tiles of 30 / 30 / 1 rows and 32 / 32 / 1 columns
SSIM_SHAPES = (SSIM_MAIN, (3, 30, 32), (1, 31, 33), (2, 5, 11), (1, 11, 4), (1, 1, 70), (1, 70, 1))
# regime -> ((shape, lambda), ...): the first entry is the regime's first case
SSIM_PLAN = {
    "white":     ((SSIM_MAIN, 0.2), ((3, 30, 32), 1.0), (SSIM_MAIN, 0.0), ((2, 5, 11), 0.2), ((1, 1, 70), 1.0), ((1, 70, 1), 0.2), ((1, 11, 4), 0.2), ((1, 31, 33), 1.0)),
    "smooth_2":  ((SSIM_MAIN, 0.2), ((1, 31, 33), 1.0)),
    "smooth_3":  ((SSIM_MAIN, 1.0), ((1, 70, 1), 0.2), ((3, 30, 32), 0.2)),
    "affine":    ((SSIM_MAIN, 0.2), ((1, 11, 4), 1.0)),
    "constant":  ((SSIM_MAIN, 1.0), ((2, 5, 11), 0.2)),
    "bright":    ((SSIM_MAIN, 0.2), ((3, 30, 32), 1.0)),
    "black":     ((SSIM_MAIN, 0.2), ((1, 1, 70), 1.0)),
    "identical": ((SSIM_MAIN, 0.2), ((1, 31, 33), 0.0), ((2, 5, 11), 1.0)),
    "bit_equal": ((SSIM_MAIN, 0.2), ((3, 30, 32), 0.0)),
    "over_one":  ((SSIM_MAIN, 1.0), ((1, 70, 1), 0.2), ((1, 11, 4), 0.0)),
}
SSIM_NAMES = [f"{reg}-{c}x{h}x{w}-lam{lam:g}" for reg, plan in SSIM_PLAN.items() for (c, h, w), lam in plan]


def _smooth(shape, r):
    C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = r.uniform(0, 6.28, (C, 1, 1))
    return 0.5 + 0.25 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 - ph) + 0.1 * np.sin((xx + yy) / 23.0 + 2 * ph)


def make_ssim(name):
    """-> dict(img, gt (float32 (C, H, W)), lam, regime, claims)"""
    reg, shp, lam = name.split("-")
    shape = tuple(int(v) for v in shp.split("x"))
    lam = float(lam[3:])
    r = np.random.default_rng(sum(ord(ch) for ch in name))
    claims = {}
    if reg == "white":
        gt = r.uniform(0, 1, shape)
        img = np.clip(gt + r.normal(0, 0.15, shape), 0, 1)
    elif reg in ("smooth_2", "smooth_3"):
        gt = _smooth(shape, r)
        img = gt + r.normal(0, 1e-2 if reg == "smooth_2" else 1e-3, shape)
    elif reg == "affine":
        gt = _smooth(shape, r)
        img = gt * 0.97 + 0.01
    elif reg == "constant":
        gt, img = np.full(shape, 0.8), np.full(shape, 0.9)
    elif reg == "bright":
        gt = np.ones(shape)
        img = 1.0 - np.abs(r.normal(0, 1e-3, shape))
    elif reg == "black":
        gt = r.uniform(0, 0.02, shape)
        img = np.clip(gt + r.normal(0, 2e-3, shape), 0, None)
    elif reg == "identical":
        gt = _smooth(shape, r) + r.normal(0, 0.02, shape)
        img = gt
    elif reg == "bit_equal":                   # a block of bit-equal pixels, and pixels clipped to 0 and to 1 on both sides
        gt = np.clip(_smooth(shape, r) * 2.4 - 0.7 + r.normal(0, 0.05, shape), 0, 1)
        img = np.clip(gt + r.normal(0, 0.05, shape), 0, 1)
        H, W = shape[1:]
        blk = (slice(None), slice(H // 4, max(H // 4 + 1, 3 * H // 4)), slice(W // 4, max(W // 4 + 1, 3 * W // 4)))
        img[blk] = gt[blk]
        claims = dict(block=blk)
    elif reg == "over_one":
        gt = r.uniform(0, 1.5, shape)
        img = gt + r.normal(0, 0.1, shape)
    else:
        raise KeyError(name)
    return dict(img=np.ascontiguousarray(img, f32), gt=np.ascontiguousarray(gt, f32), lam=lam, regime=reg, shape=shape, claims=claims)


# ----------------------------------------------------------------------------------------------------------------------- cameras, planes
GEO_MAIN = (9, 129)                   # tiles of 4 / 4 / 1 rows and 64 / 64 / 1 columns
GEO_SHAPES = (GEO_MAIN, (4, 64), (5, 65), (3, 3), (1, 7), (2, 5), (7, 1), (6, 2))
NO_INTERIOR = ((1, 7), (2, 5), (7, 1), (6, 2))
FOCAL = 30.0                          # pixels: |P| / |P(x+1) - P(x-1)| ~ FOCAL / 2, the cancellation every depth normal carries


def kinv_t(H, W):
    """inverse(K^T) of a pinhole camera with the principal point off the pixel grid"""
    cx, cy = W / 2 + 0.25, H / 2 - 0.125
    return np.array([[1 / FOCAL, 0, 0], [0, 1 / FOCAL, 0], [-cx / FOCAL, -cy / FOCAL, 1]], np.float64)


def rotation():
    """a rotation about a skew axis: far from symmetric, so its transpose is another matrix"""
    ax = np.array([0.3, -0.8, 0.52]); ax /= np.linalg.norm(ax)
    t = 0.7
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def surfel_matrices(H, W):
    """-> ray_mat, normal_rot as float32 (3, 3): rays_d = [x y 1] @ ray_mat (world), normal_world = normal_view @ normal_rot"""
    Rw = rotation()
    return (kinv_t(H, W) @ Rw).astype(f32), Rw.astype(f32)


def depth_normal(depth, rm):
    """float64 numpy: normalize((P(y+1) - P(y-1)) x (P(x+1) - P(x-1))) on the interior, 0 on the border -> (3, H, W)"""
    H, W = depth.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rm = np.asarray(rm, np.float64)
    P = depth[..., None] * (xx[..., None] * rm[0] + yy[..., None] * rm[1] + rm[2])
    out = np.zeros((H, W, 3))
    if H > 2 and W > 2:
        c = np.cross(P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2])
        out[1:-1, 1:-1] = c / np.maximum(np.linalg.norm(c, axis=2, keepdims=True), 1e-12)
    return out.transpose(2, 0, 1)


def _wavy(H, W, r, noise):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return 3.0 + 0.5 * np.sin(xx / 7.0) + 0.3 * np.cos(yy / 5.0) + r.normal(0, noise, (H, W))


def _tilted(H, W, rm, world=False):
    """depth of the plane <nrm, X> = 4 along the rays of rm (nrm given in camera space; world: turned with the camera)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = xx[..., None] * rm[0] + yy[..., None] * rm[1] + rm[2]
    nrm = np.array([0.2, -0.1, 1.0]); nrm /= np.linalg.norm(nrm)
    return 4.0 / (ray @ (nrm @ rotation() if world else nrm))


# ------------------------------------------------------------------------------------------------------------------------------- 2DGS geo
# regime -> ((shape, depth_ratio, lambda_dist), ...)
SURFEL_PLAN = {
    "noisy":     ((GEO_MAIN, 0.0, 100.0), ((4, 64), 1.0, 0.0), ((5, 65), 0.3, 100.0), ((3, 3), 0.0, 0.0), ((1, 7), 0.3, 100.0), ((2, 5), 0.0, 0.0), ((7, 1), 1.0, 100.0),
                  ((6, 2), 0.3, 0.0), (GEO_MAIN, 0.3, 0.0)),
    "converged": ((GEO_MAIN, 0.0, 0.0), ((5, 65), 1.0, 100.0), (GEO_MAIN, 0.3, 100.0)),
    "empty":     ((GEO_MAIN, 0.3, 0.0), (GEO_MAIN, 1.0, 100.0)),
    "specials":  ((GEO_MAIN, 0.3, 0.0), ((5, 65), 0.0, 100.0), ((3, 3), 1.0, 0.0), (GEO_MAIN, 0.0, 0.0)),
}
SURFEL_NAMES = [f"{reg}-{h}x{w}-r{ratio:g}-d{ld:g}" for reg, plan in SURFEL_PLAN.items() for (h, w), ratio, ld in plan]
LAMBDA_NORMAL = 0.05
EMPTY_RECT = (slice(2, 8), slice(30, 101))           # 6 x 71 pixels over the seams at row 4 and column 64
TINY_NORMAL, TINY_SUBNORMAL = f32(2.0 ** -126), f32(2.0 ** -130)


def make_surfel(name):
    """-> dict(allmap (11, H, W), ray_mat, normal_rot, depth_ratio, lambda_normal, lambda_dist, regime, claims)"""
    reg, shp, ratio, ld = name.split("-")
    H, W = (int(v) for v in shp.split("x"))
    ratio, ld = float(ratio[1:]), float(ld[1:])
    r = np.random.default_rng(sum(ord(ch) for ch in name))
    rm, nr = surfel_matrices(H, W)
    am = np.zeros((11, H, W), np.float64)
    claims = {}
    if reg == "converged":
        depth = _tilted(H, W, rm.astype(np.float64), world=True)
        alpha = 1.0 - r.uniform(0, 1e-3, (H, W))
        med = depth
    else:
        depth = _wavy(H, W, r, 0.02)
        alpha = r.uniform(0.3, 1.0, (H, W))
        alpha[r.uniform(size=(H, W)) < 0.05] = 0.0                # isolated holes: 0 / 0 -> nan -> 0
        med = depth + r.normal(0, 0.05, (H, W))
    am[1] = alpha
    am[0] = f32(depth) * f32(alpha)
    am[5] = med
    am[6] = r.uniform(0, 0.1, (H, W))
    am[7:] = r.normal(0, 1, (4, H, W))
    if reg == "converged":
        am = am.astype(f32).astype(np.float64)
        with np.errstate(all="ignore"):
            d = (1 - ratio) * np.nan_to_num(am[0] / am[1]) + ratio * am[5]
        nd = depth_normal(d, rm.astype(np.float64))                # (3, H, W) world
        pert = r.normal(0, 1e-3, (3, H, W))
        am[2:5] = np.einsum("chw,dc->dhw", nd + pert, nr.astype(np.float64))          # view = world @ normal_rot^T
    else:
        n = r.normal(0, 1, (3, H, W)); n /= np.linalg.norm(n, axis=0, keepdims=True)
        am[2:5] = n * alpha
    am = am.astype(f32)
    if reg == "empty":
        am[(slice(None),) + EMPTY_RECT] = 0.0
        claims = dict(rect=EMPTY_RECT)
    if reg == "specials":
        px = [(y, x) for y in range(H) for x in range(W)]
        pick = [px[i] for i in r.permutation(len(px))[:min(8, len(px))]]
        kinds = ["a0_alpha0", "med_inf", "med_nan", "alpha_normal", "alpha_subnormal", "med_ninf", "a0_alpha0", "alpha_subnormal_a0_normal"]
        claims = dict(pixels={})
        for (y, x), kind in zip(pick, kinds):
            if kind == "a0_alpha0":
                am[0, y, x], am[1, y, x] = 2.5, 0.0
            elif kind.startswith("med_"):
                am[5, y, x] = dict(med_inf=np.inf, med_ninf=-np.inf, med_nan=np.nan)[kind]
            elif kind == "alpha_normal":
                am[1, y, x] = TINY_NORMAL; am[0, y, x] = f32(3.0) * TINY_NORMAL; am[2:5, y, x] *= TINY_NORMAL
            elif kind == "alpha_subnormal":
                am[1, y, x] = TINY_SUBNORMAL; am[0, y, x] = f32(3.0) * TINY_SUBNORMAL; am[2:5, y, x] *= TINY_SUBNORMAL
            else:                                                   # the quotient overflows float32, not float64
                am[1, y, x] = TINY_SUBNORMAL; am[0, y, x] = 2.5
            claims["pixels"].setdefault(kind, []).append((y, x))
    return dict(allmap=am, ray_mat=rm, normal_rot=nr, depth_ratio=ratio, lambda_normal=LAMBDA_NORMAL, lambda_dist=ld, regime=reg, shape=(H, W), claims=claims)


# ------------------------------------------------------------------------------------------------------------------------------- PGSR geo
# regime -> ((shape, weight kind), ...)
PLANE_PLAN = {
    "noisy":       ((GEO_MAIN, "random"), ((4, 64), None), ((5, 65), "zero_region"), ((3, 3), "random"), ((1, 7), "random"), ((2, 5), None), ((7, 1), "random"),
                    ((6, 2), "zero_region")),
    "conv_pert":   ((GEO_MAIN, None), ((5, 65), "random")),
    "conv_zero":   ((GEO_MAIN, "random"), ((4, 64), None)),
    "conv_ulps":   ((GEO_MAIN, None),),
    "alpha0":      ((GEO_MAIN, "random"), ((5, 65), None)),
    "depth0":      ((GEO_MAIN, "zero_region"), ((5, 65), "random")),
}
PLANE_NAMES = [f"{reg}-{h}x{w}-{wk}" for reg, plan in PLANE_PLAN.items() for (h, w), wk in plan]
PLANE_LAMBDA = 0.015
FRAGILE_BY_CONSTRUCTION = ("conv_ulps",)
MAX_FRAGILE = 0.02


def block(H, W):
    """a rectangle over the tile seams where the image has them"""
    return (slice(min(2, H - 1), max(min(2, H - 1) + 1, H - 2)), slice(W // 4, max(W // 4 + 1, 3 * W // 4)))


def make_plane(name):
    """-> dict(depth (H, W), all_map (5, H, W): normal 0:3, alpha 3, distance 4; weight or None, ray_mat, lam, regime, claims)"""
    reg, shp, wk = name.split("-", 2)
    H, W = (int(v) for v in shp.split("x"))
    r = np.random.default_rng(sum(ord(ch) for ch in name))
    rm = kinv_t(H, W).astype(f32)
    rm64 = rm.astype(np.float64)
    am = np.zeros((5, H, W), np.float64)
    claims = {}
    alpha = r.uniform(0.2, 1.0, (H, W))
    if reg in ("noisy", "alpha0", "depth0"):
        depth = _wavy(H, W, r, 0.02).astype(f32)
        n = r.normal(0, 1, (3, H, W)); n /= np.linalg.norm(n, axis=0, keepdims=True)
        am[0:3] = n * alpha
    elif reg == "conv_zero":                  # a fronto-parallel plane: depth_normal = (0, 0, -1) with the two zeros exact in any arithmetic
        depth = np.full((H, W), 2.75, f32)
        am[2] = -alpha.astype(f32).astype(np.float64) + 1e-2 * r.choice([-1.0, 1.0], (H, W))
        claims = dict(exact_zero_components=(0, 1))
    else:
        depth = _tilted(H, W, rm64).astype(f32)
        dn = depth_normal(depth.astype(np.float64), rm64) * alpha.astype(f32).astype(np.float64)
        if reg == "conv_pert":
            am[0:3] = dn + 1e-2 * r.choice([-1.0, 1.0], (3, H, W))
        else:                                   # a few ulps off: every sign is within the float32 error of the depth normal
            am[0:3] = dn.astype(f32).astype(np.float64) * (1.0 + r.integers(-3, 4, (3, H, W)) * 2.0 ** -23)
    am[3] = alpha
    am[4] = r.uniform(1, 3, (H, W))
    am = am.astype(f32)
    blk = block(H, W)
    if reg == "alpha0":
        am[(3,) + blk] = 0.0
        claims = dict(block=blk)
    if reg == "depth0":
        depth[blk] = 0.0
        claims = dict(block=blk)
    weight = None
    if wk != "None":
        weight = r.uniform(0, 1, (H, W)).astype(f32)
        if wk == "zero_region":
            weight[:, : max(W // 3, 1)] = 0.0
    return dict(depth=depth, all_map=am, weight=weight, ray_mat=rm, lam=PLANE_LAMBDA, regime=reg, shape=(H, W), claims=claims)

