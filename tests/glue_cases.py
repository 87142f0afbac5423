"""Inputs of the edge tests of csrc/gsr_extra.hip (tests/test_glue_truth_cpu.py and the test_gpu_*_edges.py files).  TEST INFRASTRUCTURE ONLY.
numpy only; every builder is deterministic, and every structural claim a builder makes is asserted by the test that uses it."""
import numpy as np

import glue_truth
import scenes

# ------------------------------------------------------------------------------------------------------------------------------ Adam
ADAM_SIZES = (1, 3, 4, 4095, 4096, 4097, 8191, 8197, 3 * 4096 + 2)       # GSR_ADAM_CHUNK = 4096: below, at, above; float4 body with 0..3 tail elements
ADAM_STEPS = 6


def adam_case(n, seed=0):
    """The flat-parameter form of bench.py: p ~ N(0,1) clipped to |p| <= 2, lr_scale log-uniform in [1e-4, 5e-2] (different at every element),
    six gradients whose scale alternates 0.1 / 3.0 (tests/test_gpu_optim.py)."""
    r = np.random.default_rng(1000 + 17 * n + seed)
    p = np.clip(r.normal(0, 1, n), -2, 2).astype(np.float32)
    sc = np.exp(r.uniform(np.log(1e-4), np.log(5e-2), n)).astype(np.float32)
    grads = [(r.normal(0, 1, n) * (0.1 if t % 2 else 3.0)).astype(np.float32) for t in range(1, ADAM_STEPS + 1)]
    return p, sc, grads


# ------------------------------------------------------------------------------------------------------------------------------ distCUDA2
KNN_BOX = 256


def morton_boxes(points):
    """The 256-point box of every point under the kernel's ordering, restated: per-axis float32 min / max, t = (p - lo) / (hi - lo) (0 when hi == lo),
    10-bit cell (uint32)(t * 1023), bits interleaved x | y << 1 | z << 2, STABLE sort by the 30-bit code, boxes of 256 consecutive points.
    -> (box [P], order [P])"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    code = np.zeros(p.shape[0], np.uint32)
    for c in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(hi[c] > lo[c], (p[:, c] - lo[c]) / (hi[c] - lo[c]), np.float32(0)).astype(np.float32)
        cell = (t * np.float32(1023)).astype(np.uint32)
        spread = np.zeros_like(cell)
        for b in range(10):
            spread |= ((cell >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
        code |= spread << np.uint32(c)
    order = np.argsort(code, kind="stable")
    box = np.empty(p.shape[0], np.int64); box[order] = np.arange(p.shape[0]) // KNN_BOX
    return box, order


def knn_cluster_case(seed=16):
    """512 points = two boxes: two tight pairs (1e-3 apart inside a pair, the pairs 10 apart) on the z = 0 mid-plane, where the top Morton bit
    splits the cloud, and 508 scattered points that keep 1.5 clear of both pairs.  A pair point's nearest neighbour is its twin; its second and third
    are scattered points 1.5 or more away, on either side of the split.  With the default seed the second lies in the pair's own box and the third in
    the OTHER one, for all four pair points (tests/test_glue_truth_cpu.py checks it)."""
    r = np.random.default_rng(4200 + seed)
    pairs = np.array([[0, 0, 0], [1e-3, 0, 0], [10, 0, 0], [10 + 1e-3, 0, 0]], np.float64)
    pts = []
    while len(pts) < 508:
        q = r.uniform([-2, -3, -3], [12, 3, 3])
        if min(np.linalg.norm(q - pairs[0]), np.linalg.norm(q - pairs[2])) > 1.5:
            pts.append(q)
    return np.concatenate([pairs, np.array(pts)]).astype(np.float32)


def knn_inputs():
    """name -> points of the exact-equality matrix."""
    r = np.random.default_rng(31)
    out = {f"P{P}": r.normal(0, 1, (P, 3)).astype(np.float32) for P in (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1025)}
    out["identical600"] = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (600, 1))
    plane = r.normal(0, 1, (700, 3)).astype(np.float32); plane[:, 2] = 0.25
    out["plane700"] = plane
    line = np.zeros((700, 3), np.float32); line[:, 0] = r.normal(0, 1, 700); line[:, 1] = -0.5; line[:, 2] = 2.0
    out["line700"] = line
    base = r.normal(0, 1, (300, 3)).astype(np.float32)
    out["dup300x2"] = np.concatenate([base, base])
    out["clusters"] = knn_cluster_case()
    return out


# ------------------------------------------------------------------------------------------------------------------------------ TSDF point update
TSDF_W, TSDF_H = 48, 32
TSDF_SIZES = (1, 3, 4, 5, 8, 1023, 1024, 1027)
TSDF_TRUNC = 0.3
KINDS = ("front", "outside", "straddle", "behind", "front", "beyond", "border", "straddle")       # by index % 8


def tsdf_cameras(frames=2):
    """The camera of tests/test_gpu_parity.py's TSDF case at half size (48 x 32, focal 40); frame 0 is the identity pose."""
    return [scenes.make_camera(TSDF_W, TSDF_H, 40.0, 40.0, yaw_deg=5.0 * fr, t=(0.1 * fr, 0, 0)) for fr in range(frames)]


def tsdf_maps(frames=2):
    """Smooth depth (5 + 0.3 sin cos: at most 0.06 per pixel, so a float32 pixel coordinate off by 1e-5 moves the depth by < 1e-6) and random colour."""
    r = np.random.default_rng(77)
    yy, xx = np.mgrid[0:TSDF_H, 0:TSDF_W].astype(np.float64)
    depth = [(5.0 + 0.3 * np.sin(0.2 * xx + fr) * np.cos(0.15 * yy) + 0.02 * fr).astype(np.float32)[None] for fr in range(frames)]
    rgb = [r.uniform(0, 1, (3, TSDF_H, TSDF_W)).astype(np.float32) for _ in range(frames)]
    return depth, rgb


def _border_points(F, count):
    """Points whose float32 pixel coordinate is EXACTLY W - 1 while u < 1 still holds: u = 1 - 2^-24, for which (u + 1) rounds to 2.  There the right-hand
    corners of the bilinear stencil lie outside the image (x1 = W) and must be left out, not read.  A quotient of two floats of one binade cannot be
    that close to 1, so q.w = z = 4 exactly and q.x = x F[0][0] the float just below 4; y is free."""
    target = np.nextafter(np.float32(1), np.float32(0))
    x0 = np.float32(4.0) / np.float32(F[0][0])
    cand = [x0]
    for _ in range(8):
        cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(8))]
    ok = [x for x in cand if glue_truth.tsdf_project32(np.array([[x, 0, 4.0]], np.float32), F)[0][0] == target]
    assert ok, "no float32 x projects to u = 1 - 2^-24"
    p = np.zeros((count, 3), np.float32)
    p[:, 0] = ok[0]; p[:, 2] = 4.0
    p[:, 1] = 4.0 * (TSDF_H / 2 / 40.0) * np.random.default_rng(5).uniform(-0.9, 0.9, count)
    return p


def tsdf_points(V, F0):
    """V points in the space of frame 0's camera, their kind dealt by index % 8 (KINDS): in front of the surface (always updated), outside the
    frustum sideways, straddling the surface within +-0.5, behind the camera, far behind the surface (z ~ 8: beyond any truncation <= 2), and on the last
    texel column.  From V = 8 on every kind is present and 5 of 8 points are in front of or on the surface."""
    r = np.random.default_rng(900 + V)
    tx, ty = TSDF_W / 2 / 40.0, TSDF_H / 2 / 40.0
    p = np.zeros((V, 3), np.float64)
    for i in range(V):
        kind = KINDS[i % 8]
        z = {"front": r.uniform(4.0, 4.6), "straddle": r.uniform(4.6, 5.5), "beyond": r.uniform(7.5, 8.5), "behind": -r.uniform(0.5, 3.0),
             "outside": r.uniform(4.0, 5.5), "border": 0.0}[kind]
        a, b = r.uniform(-0.9, 0.9), r.uniform(-0.9, 0.9)
        if kind == "outside":
            a = r.choice([-1.0, 1.0]) * r.uniform(1.05, 1.5)
        p[i] = (z * tx * a, z * ty * b, z) if kind != "behind" else (tx * a, ty * b, z)
    p = p.astype(np.float32)
    idx = np.nonzero(np.arange(V) % 8 == 6)[0]
    if idx.size:
        p[idx] = _border_points(F0, idx.size)
    return p


def tsdf_trunc_pp(V):
    """A truncation that really varies: log-uniform in [0.1, 2.0] (a factor of 20)."""
    return np.exp(np.random.default_rng(600 + V).uniform(np.log(0.1), np.log(2.0), V)).astype(np.float32)


def tsdf_truth(V, frames, trunc):
    """-> (points, cams, depth, rgb, (tsdf, weight, rgb) float64 after `frames` frames from the reference's initial state (1, 1, 0), info of frame 0)"""
    cams = tsdf_cameras(frames); depth, rgb = tsdf_maps(frames)
    pts = tsdf_points(V, cams[0]["projmatrix"])
    t = np.ones(V); w = np.ones(V); c = np.zeros((V, 3))
    info = None
    for fr in range(frames):
        i = glue_truth.tsdf_frame(pts, cams[fr]["projmatrix"], depth[fr], rgb[fr], trunc, t, w, c)
        info = info or i
    return pts, cams, depth, rgb, (t, w, c), info


# ------------------------------------------------------------------------------------------------------------------------------ plane all_map
PLANE_SIZES = (1, 255, 256, 257, 1000)


def plane_view():
    cam = scenes.make_camera(64, 48, 50.0, 50.0, yaw_deg=20.0, t=(0.5, 0.2, 0.0))
    return cam["viewmatrix"], cam["campos"]


def plane_random(P, scale_cols, seed=0):
    """P Gaussians with non-unit quaternions (norms 0.3 .. 3) and (P, scale_cols) scales, kept clear of every decision: |dot| and |signed distance|
    above 1e-3, pairwise gaps of the first three scales above 1e-4 relative (the tests assert it on the truth's intermediates)."""
    V, cp = plane_view()
    r = np.random.default_rng(300 + 7 * P + scale_cols + seed)
    n = 2 * P + 64
    xyz = r.uniform(-5, 5, (n, 3)).astype(np.float32)
    q = r.normal(0, 1, (n, 4)); q = (q / np.linalg.norm(q, axis=1, keepdims=True) * r.uniform(0.3, 3.0, (n, 1))).astype(np.float32)
    sc = np.exp(r.normal(-2, 0.7, (n, scale_cols))).astype(np.float32)
    t = glue_truth.plane_allmap_autograd(xyz, q, sc, V, cp)
    keep = np.nonzero(plane_margins_ok(t, sc))[0][:P]
    assert keep.size == P
    dL = r.normal(0, 1, (P, 5)).astype(np.float32)
    return xyz[keep], q[keep], sc[keep], V, cp, dL


def plane_margins_ok(truth, scale):
    s = np.asarray(scale, np.float64)[:, :3]
    gap = np.min(np.abs(np.stack([s[:, 0] - s[:, 1], s[:, 0] - s[:, 2], s[:, 1] - s[:, 2]], -1)), axis=1) / s.max(axis=1)
    return (np.abs(truth["dot"]) > 1e-3) & (np.abs(truth["sd"]) > 1e-3) & (gap > 1e-4)


def plane_edge_rows():
    """Rows of small integers and half-integers, quaternions whose rotation matrices are signed permutations ((1,0,0,0): identity; (0,1,0,0): half turn
    about x; (1,1,0,0): quarter turn about x, two_s = 1; (2,0,2,0): quarter turn about y, two_s = 1/4) and an axis-swapping view matrix with integer
    translation: every intermediate is exact in float32, so the float64 truth is what the kernel owes bit for bit.
    Two camera centres: the view matrix's own (-T R^T: then dot == -signed distance, both zero together) and a shifted one (dot == 0 with a
    non-zero distance, distance 0 with a non-zero dot).  -> (xyz, q, scales3, V, [campos_own, campos_shifted], tags, the column each row must pick)"""
    V = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [1, -2, 3, 1]], np.float32)           # p_view = p_world @ V[:3,:3] + V[3,:3]
    own = (-(V[3, :3].astype(np.float64)) @ V[:3, :3].astype(np.float64).T).astype(np.float32)
    shifted = own + np.array([1.5, -0.5, 2.0], np.float32)
    quats = [(1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (2, 0, 2, 0), (0.5, 0, 0, 0), (0, 0, 0, 2)]
    scales = [("s0=s1<s2", (0.5, 0.5, 2.0), 0), ("s0=s2<s1", (0.5, 2.0, 0.5), 0), ("all-equal", (0.25, 0.25, 0.25), 0), ("s1=s2<s0", (2.0, 0.5, 0.5), 1),
              ("s2-least", (2.0, 1.0, 0.5), 2), ("s1-least", (2.0, 0.5, 1.0), 1)]       # (name, scales, the column that must be picked)
    coords = [-3.0, -1.5, -1.0, 0.5, 2.0, 4.0]                     # own and shifted camera coordinates are among them, per axis, below
    rows, tags, want_k = [], [], []
    r = np.random.default_rng(8)
    for qi, q in enumerate(quats):
        for name, s, k in scales:
            for rep in range(6):
                x = np.array([r.choice(coords + [float(own[a]), float(shifted[a])]) for a in range(3)])
                rows.append((x, q, s)); tags.append(f"q{qi}:{name}"); want_k.append(k)
    xyz = np.array([x for x, _, _ in rows], np.float32); qq = np.array([q for _, q, _ in rows], np.float32)
    sc = np.array([s for _, _, s in rows], np.float32)
    return xyz, qq, sc, V, [own, shifted], tags, np.array(want_k)


# ------------------------------------------------------------------------------------------------------------------------------ densification statistics
DENSIFY_SIZES = (1, 255, 256, 257, 1000)


def densify_case(P, filt, seed=0):
    """filt: 'none' | 'all' | 'random'.  The gradients are (P,4) with 1e30 in the last two columns: a kernel that mixed up grad_stride would read them."""
    r = np.random.default_rng(50 + P + seed)
    f = {"none": np.zeros(P, bool), "all": np.ones(P, bool), "random": r.uniform(size=P) < 0.6}[filt]
    g = r.normal(0, 1, (P, 4)).astype(np.float32); g[:, 2:] = 1e30
    ga = np.abs(r.normal(0, 1, (P, 4))).astype(np.float32); ga[:, 2:] = 1e30
    return dict(filter=f, radii=r.integers(0, 40, P).astype(np.int32), observe=r.integers(0, 3, P).astype(np.int32), grad=g, grad_abs=ga,
                max_radii2D=r.integers(0, 30, P).astype(np.float32), accum=r.uniform(0, 1, P).astype(np.float32),
                denom=r.integers(0, 5, P).astype(np.float32), accum_abs=r.uniform(0, 1, P).astype(np.float32),
                denom_abs=r.integers(0, 5, P).astype(np.float32))
