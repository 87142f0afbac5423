"""Plain references for the trainer-side kernels of csrc/gsr_extra.hip: the fused Adam step, distCUDA2, the per-point TSDF update, the plane
`all_map` prepare and the densification statistics.  TEST INFRASTRUCTURE ONLY.

Written from the formulas in numpy / float64 torch; nothing here loads a library or imports gsrast.  tests/test_glue_truth_cpu.py pins every
function against the C oracles and the reference-run fixtures before a GPU result is read against it.

Which precision is the truth, and why:
  adam_chain         float32 (oracle_optim.adam_step chained).  The parameter itself is stored in float32 after every step, and that rounding alone
                     moves a six-step chain 5e-7 away from a float64 one at |p| <= 2 -- as much as the whole absolute term of the project's bound.
  dist2_bruteforce   float32, operation for operation as oracle/gsr_oracle.c ref_dist2: the kernel's box pruning is conservative, so it owes the
                     all-pairs result bit for bit (FLT_MAX-initialised bests included: P <= 3 gives inf / 1.13e38).  dist2_neighbours64 is the
                     float64 view of the same search, for checking WHICH points are the neighbours.
  tsdf_frame         float64 values; the mask decisions (u, v, qw, sdf > -tr) in float32 with the kernel's expressions, so that a point on a
                     boundary cannot change sides between truth and kernel.
  plane_allmap_autograd  float64 torch, gradients from autograd.
  densify_stats      float32 numpy (five masked updates)."""
import numpy as np

import oracle_optim

FLT_MAX = np.float32(3.402823466e+38)


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def adam_chain(p0, grads, lr, lr_scale=None, beta1=0.9, beta2=0.999, eps=1e-8, m0=None, v0=None, t0=0):
    """oracle_optim.adam_step over the list `grads` (steps t0+1, t0+2, ...), float32 throughout.  `lr`: one rate or one per step.
    -> (p, exp_avg, exp_avg_sq) after the last step."""
    p = np.asarray(p0, np.float32).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float32).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float32).copy()
    lrs = list(lr) if np.ndim(lr) else [lr] * len(grads)
    assert len(lrs) == len(grads)
    for k, (g, a) in enumerate(zip(grads, lrs)):
        p, m, v = oracle_optim.adam_step(p, g, m, v, t0 + k + 1, a, beta1=beta1, beta2=beta2, eps=eps, lr_scale=lr_scale)
    return p, m, v


def adam_bounds(lr, lr_scale=None):
    """The project's bounds (tests/test_gpu_optim.py) with the learning rate taken per element: |p - ref| <= 1e-4 lr scale_i + 5e-7."""
    sc = 1.0 if lr_scale is None else np.asarray(lr_scale, np.float64)
    return 1e-4 * float(lr) * sc + 5e-7


# ------------------------------------------------------------------------------------------------------------------------------ distCUDA2
def _pair_d2(pts, dtype):
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3).astype(dtype)
    dx = p[:, None, 0] - p[None, :, 0]; dy = p[:, None, 1] - p[None, :, 1]; dz = p[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz                       # every operation rounded on its own, in ref_dist2's order


def dist2_bruteforce(points):
    """All-pairs mean squared distance to the 3 nearest OTHER points (another index: an exact duplicate is a neighbour at distance 0), float32.
    The three bests start at FLT_MAX and a distance replaces one only when strictly smaller, so with fewer than three other points FLT_MAX stays in
    the sum: P = 1, 2 -> inf (FLT_MAX + FLT_MAX overflows), P = 3 -> (d0 + d1 + FLT_MAX) / 3 ~ 1.134e38."""
    P = np.asarray(points).reshape(-1, 3).shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        d = _pair_d2(points, np.float32)
        d[np.arange(P), np.arange(P)] = FLT_MAX                # j == i is skipped: one more FLT_MAX among the three appended changes nothing
        d = np.concatenate([d, np.full((P, 3), FLT_MAX, np.float32)], axis=1)
        d = np.where(d < FLT_MAX, d, FLT_MAX)                  # `d < best` is never true for d >= FLT_MAX (inf from an overflow included)
        b = np.sort(d, axis=1)[:, :3]
        return (((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3)).astype(np.float32)


def dist2_neighbours64(points):
    """float64 all-pairs: -> (idx [P, min(3, P-1)] the nearest other points in ascending distance (ties: lower index first), d2 likewise)."""
    P = np.asarray(points).reshape(-1, 3).shape[0]
    d = _pair_d2(points, np.float64)
    d[np.arange(P), np.arange(P)] = np.inf
    k = min(3, P - 1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(d, idx, axis=1)


# ------------------------------------------------------------------------------------------------------------------------------ TSDF
def _bilinear32(img, W, H, u, v):
    """grid_sample(bilinear, border, align_corners=True) in float32 with the kernel's expressions -> (value, x, y) (x, y: clamped pixel coordinates)."""
    f = np.float32
    x = ((u + f(1)) / f(2)) * f(W - 1); y = ((v + f(1)) / f(2)) * f(H - 1)
    x = np.minimum(np.maximum(x, f(0)), f(W - 1)); y = np.minimum(np.maximum(y, f(0)), f(H - 1))
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64); x1 = x0 + 1; y1 = y0 + 1
    wx1 = x - x0.astype(f); wy1 = y - y0.astype(f); wx0 = x1.astype(f) - x; wy0 = y1.astype(f) - y
    acc = np.zeros(x.shape, f)
    for xx, yy, w in ((x0, y0, wx0 * wy0), (x1, y0, wx1 * wy0), (x0, y1, wx0 * wy1), (x1, y1, wx1 * wy1)):
        ok = (xx < W) & (yy < H)
        t = img[np.minimum(yy, H - 1), np.minimum(xx, W - 1)]
        acc = np.where(ok, acc + t * w, acc).astype(f)
    return acc, x, y


def _bilinear64(img, W, H, u, v):
    x = np.clip((u + 1.0) / 2.0 * (W - 1), 0.0, W - 1.0); y = np.clip((v + 1.0) / 2.0 * (H - 1), 0.0, H - 1.0)
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    wx = x - x0; wy = y - y0
    xa = np.minimum(x0 + 1, W - 1); ya = np.minimum(y0 + 1, H - 1)      # a clamped corner carries weight 0
    im = img.astype(np.float64)
    return (im[y0, x0] * (1 - wx) + im[y0, xa] * wx) * (1 - wy) + (im[ya, x0] * (1 - wx) + im[ya, xa] * wx) * wy


def tsdf_project32(points, F):
    """[x y z 1] @ F in float32 with the kernel's expressions -> (u, v, q.w)."""
    f = np.float32
    p = np.ascontiguousarray(points, dtype=f).reshape(-1, 3); Fm = np.ascontiguousarray(F, dtype=f).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = [((x * Fm[0, k] + y * Fm[1, k]) + z * Fm[2, k]) + Fm[3, k] for k in (0, 1, 3)]
        return q[0] / q[2], q[1] / q[2], q[2]


def tsdf_frame(points, F, depth, rgb, trunc, tsdf, weight, rgb_acc):
    """One frame of compute_unbounded_tsdf into the float64 state (tsdf [V], weight [V], rgb_acc [V,3]), IN PLACE:
        q = [x y z 1] @ F;  (u, v) = q.xy / q.w;  mask = -1 < u, v < 1 and q.w > 0 and sdf > -trunc,  sdf = depth(u, v) - q.w
        tsdf = (tsdf w + clip(sdf / trunc, -1, 1)) / (w + 1),  rgb likewise with rgb(u, v),  w += 1          (masked points only)
    depth(u, v), rgb(u, v): bilinear, border padding, align_corners=True.  trunc: a scalar or one value per point.
    -> dict of the float32 decisions: updated, in_frustum (u, v inside and q.w > 0), behind (q.w <= 0), sdf32, x_pix, y_pix."""
    f = np.float32
    p = np.ascontiguousarray(points, dtype=f).reshape(-1, 3); Fm = np.ascontiguousarray(F, dtype=f).reshape(4, 4)
    d = np.ascontiguousarray(depth, dtype=f); H, W = d.shape[-2:]; d = d.reshape(H, W)
    c = np.ascontiguousarray(rgb, dtype=f).reshape(3, H, W)
    V = p.shape[0]
    tr32 = np.broadcast_to(np.asarray(trunc, f).reshape(-1), (V,)) if np.ndim(trunc) else np.full(V, f(trunc), f)
    u32, v32, qw32 = tsdf_project32(p, Fm)
    with np.errstate(invalid="ignore"):
        front = (u32 > -1) & (u32 < 1) & (v32 > -1) & (v32 < 1) & (qw32 > 0)
        us = np.where(front, u32, f(0)); vs = np.where(front, v32, f(0))
        d32, xp, yp = _bilinear32(d, W, H, us, vs)
        sdf32 = d32 - qw32
        upd = front & (sdf32 > -tr32)
    P64 = p.astype(np.float64); F64 = Fm.astype(np.float64)
    q = np.concatenate([P64, np.ones((V, 1))], axis=1) @ F64
    i = np.nonzero(upd)[0]
    u = q[i, 0] / q[i, 3]; v = q[i, 1] / q[i, 3]
    s = np.clip((_bilinear64(d, W, H, u, v) - q[i, 3]) / tr32[i].astype(np.float64), -1.0, 1.0)
    w = weight[i].copy()
    tsdf[i] = (tsdf[i] * w + s) / (w + 1)
    for ch in range(3):
        rgb_acc[i, ch] = (rgb_acc[i, ch] * w + _bilinear64(c[ch], W, H, u, v)) / (w + 1)
    weight[i] = w + 1
    return dict(updated=upd, in_frustum=front, behind=~(qw32 > 0), sdf32=sdf32, trunc32=tr32, x_pix=np.where(front, xp, np.nan),
                y_pix=np.where(front, yp, np.nan))


# ------------------------------------------------------------------------------------------------------------------------------ plane all_map
def first_argmin3(scale):
    """Index of the smallest of the first three columns, the FIRST one among equals (torch.min's choice on the reference's path)."""
    s = np.asarray(scale)[:, :3]
    k = np.zeros(s.shape[0], np.int64); sm = s[:, 0].copy()
    k[s[:, 1] < sm] = 1; sm = np.minimum(sm, s[:, 1])
    k[s[:, 2] < sm] = 2
    return k


def plane_allmap_autograd(xyz, q, scale, V, campos, dL=None):
    """float64 torch: R = quaternion_to_matrix(q) (pytorch3d: real part first, two_s = 2 / q.q, NO normalisation of q beforehand);
    n = R[:, argmin(scale)] (first minimum), flipped towards the camera with no gradient through the flip;
    local_normal = n @ V[:3,:3];  local_distance = |local_normal . (xyz @ V[:3,:3] + V[3,:3])|;  all_map = [local_normal, 1, local_distance].
    -> dict(all_map [P,5], k, dot, sd (the signed distance) and, when dL is given, d_xyz, d_q from autograd)."""
    import torch
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32).astype(np.float64))
    x = t(xyz).requires_grad_(True); qq = t(q).requires_grad_(True); Vm = t(V).reshape(4, 4); cp = t(campos).reshape(3)
    r, i, j, k = qq.unbind(-1)
    two_s = 2.0 / (qq * qq).sum(-1)
    R = torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], dim=-1).reshape(-1, 3, 3)
    kk = torch.from_numpy(first_argmin3(np.ascontiguousarray(scale, dtype=np.float32)))
    n = torch.gather(R, 2, kk.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(-1)
    dot = (n * (cp - x)).sum(-1)
    n = torch.where((dot.detach() < 0).unsqueeze(-1), -n, n)
    ln = n @ Vm[:3, :3]
    pc = x @ Vm[:3, :3] + Vm[3, :3]
    sd = (ln * pc).sum(-1)
    am = torch.cat([ln, torch.ones_like(sd).unsqueeze(-1), sd.abs().unsqueeze(-1)], dim=-1)
    out = dict(all_map=am.detach().numpy(), k=kk.numpy(), dot=dot.detach().numpy(), sd=sd.detach().numpy())
    if dL is not None:
        (am * t(dL)).sum().backward()
        out["d_xyz"] = x.grad.numpy(); out["d_q"] = qq.grad.numpy()
    return out


# ------------------------------------------------------------------------------------------------------------------------------ densification statistics
def densify_stats(filt, radii, grad, max_radii2D, accum, denom, out_observe=None, grad_abs=None, accum_abs=None, denom_abs=None):
    """The five masked updates of VanillaGaussian.densify / PGSRGaussian.densify, IN PLACE on float32 arrays [P]:
        max_radii2D[m] = max(max_radii2D[m], radii[m])       m = filter (PGSR: filter & out_observe > 0)
        accum[filter] += |grad[filter, :2]|;  denom[filter] += 1;  the _abs pair likewise from grad_abs.  Columns past the second are never read."""
    f = np.float32
    fl = np.asarray(filt).reshape(-1).astype(bool)
    r = np.asarray(radii).reshape(-1).astype(f)
    m = fl if out_observe is None else fl & (np.asarray(out_observe).reshape(-1) > 0)
    max_radii2D[m] = np.maximum(max_radii2D[m], r[m])
    norm = lambda g: np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(f)
    g = np.asarray(grad, f)
    accum[fl] += norm(g)[fl]; denom[fl] += f(1)
    if grad_abs is not None:
        ga = np.asarray(grad_abs, f)
        accum_abs[fl] += norm(ga)[fl]; denom_abs[fl] += f(1)
