"""numpy float32 restatement of the unbounded mesh path as include/gsrast.h defines it (gsr_unbounded_*): the lattice with its un-contraction and
adaptive truncation, the per-frame update rule fused over the frames, marching cubes over a dense non-uniform lattice in canonical order, the finish
and the texturing pass.  Every float32 operation is rounded on its own, in the order of the contract."""
import numpy as np

from ref_mesh_numpy import CORNER_OFF, EDGE_AXIS, EDGE_CORNER, TABLE

f32 = np.float32


def uncontract(c, center, radius, voxel_size=None):
    """c [n,3] contracted float32 -> (world [n,3], truncation [n] or None)."""
    c = np.asarray(c, f32)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(all="ignore"):
        mag = np.sqrt(x * x + y * y + z * z)
        s = f32(1) / (f32(2) - mag)
        p = np.where((mag < 1)[:, None], c, s[:, None] * (c / mag[:, None])).astype(f32)
        world = p * f32(radius) + np.asarray(center, f32)[None, :]
        if voxel_size is None:
            return world.astype(f32), None
        t = np.full(mag.shape, f32(5) * f32(voxel_size), f32)
        t = np.where(mag > 1, t * (f32(1) / (f32(2) - np.minimum(mag, f32(1.9)))), t).astype(f32)
    return world.astype(f32), t


def lattice_points(xs, ys, zs, center, radius, voxel_size):
    X, Y, Z = np.meshgrid(np.asarray(xs, f32), np.asarray(ys, f32), np.asarray(zs, f32), indexing="ij")
    return uncontract(np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1), center, radius, voxel_size)


def _bilinear(img, u, v):
    """grid_sample(bilinear, border, align_corners=True) of img [H,W] at u, v [n]: clamped coordinates, ATen's corner weights and order."""
    H, W = img.shape
    x = ((u + f32(1)) / f32(2)) * f32(W - 1)
    y = ((v + f32(1)) / f32(2)) * f32(H - 1)
    x = np.minimum(np.maximum(x, f32(0)), f32(W - 1)); y = np.minimum(np.maximum(y, f32(0)), f32(H - 1))
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    wx1, wy1 = x - x0.astype(f32), y - y0.astype(f32)
    wx0, wy0 = x1.astype(f32) - x, y1.astype(f32) - y
    acc = np.zeros(x.shape, f32)
    for xx, yy, w in ((x0, y0, wx0 * wy0), (x1, y0, wx1 * wy0), (x0, y1, wx0 * wy1), (x1, y1, wx1 * wy1)):
        ok = (xx < W) & (yy < H)
        acc = np.where(ok, acc + img[np.minimum(yy, H - 1), np.minimum(xx, W - 1)] * w, acc).astype(f32)
    return acc


def fuse(points, trunc, full_proj, depth, rgb=None):
    """The update rule of compute_unbounded_tsdf over the frames in order: points [n,3] world, trunc [n] or scalar, full_proj [F,4,4], depth [F,1,H,W]
    or [F,H,W], rgb [F,3,H,W] or None -> tsdf [n] (and colours [n,3])."""
    pts = np.asarray(points, f32)
    n = pts.shape[0]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    tr = np.broadcast_to(np.asarray(trunc, f32), (n,))
    tsdf, w = np.ones(n, f32), np.ones(n, f32)
    col = np.zeros((n, 3), f32)
    with np.errstate(all="ignore"):
        for f in range(len(full_proj)):
            P = np.asarray(full_proj[f], f32).reshape(16)
            d = np.asarray(depth[f], f32).reshape(depth[f].shape[-2:])
            qx = x * P[0] + y * P[4] + z * P[8] + P[12]
            qy = x * P[1] + y * P[5] + z * P[9] + P[13]
            qw = x * P[3] + y * P[7] + z * P[11] + P[15]
            u, v = qx / qw, qy / qw
            mask = (u > -1) & (u < 1) & (v > -1) & (v < 1) & (qw > 0)
            us, vs = np.where(mask, u, f32(0)), np.where(mask, v, f32(0))
            sdf = _bilinear(d, us, vs) - qw
            mask &= sdf > -tr
            s = np.minimum(np.maximum(sdf / tr, f32(-1)), f32(1))
            wp = w + f32(1)
            tsdf = np.where(mask, (tsdf * w + s) / wp, tsdf).astype(f32)
            if rgb is not None:
                for ch in range(3):
                    smp = _bilinear(np.asarray(rgb[f][ch], f32), us, vs)
                    col[:, ch] = np.where(mask, (col[:, ch] * w + smp) / wp, col[:, ch])
            w = np.where(mask, wp, w).astype(f32)
    return tsdf if rgb is None else (tsdf, col)


def lattice_tsdf(xs, ys, zs, center, radius, voxel_size, full_proj, depth):
    pts, tr = lattice_points(xs, ys, zs, center, radius, voxel_size)
    return fuse(pts, tr, full_proj, depth).reshape(len(xs), len(ys), len(zs))


def marching_cubes(f, xs, ys, zs):
    """f [nx,ny,nz], ascending axes -> (vertices [V,3] float32 contracted, triangles [T,3] int32) in canonical order: vertices by (gx, gy, gz, axis),
    triangles by cube (gx, gy, gz), then table order.  Case bit i = (f_i < 0); one vertex per lattice edge whose ends differ in sign."""
    f = np.asarray(f, f32)
    ax = [np.asarray(a, f32) for a in (xs, ys, zs)]
    n = f.shape
    inside = f < 0
    edge = np.zeros(n + (3,), bool)
    edge[:-1, :, :, 0] = inside[:-1] != inside[1:]
    edge[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    edge[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid = np.full(n + (3,), -1, np.int64)
    where = np.argwhere(edge)                                  # C order: gx, gy, gz, axis
    vid[edge] = np.arange(len(where))
    g, a = where[:, :3], where[:, 3]
    g1 = g + np.eye(3, dtype=np.int64)[a]
    f0, f1 = f[g[:, 0], g[:, 1], g[:, 2]], f[g1[:, 0], g1[:, 1], g1[:, 2]]
    with np.errstate(all="ignore"):
        t = (f0 / (f0 - f1)).astype(f32)
    verts = np.stack([ax[0][g[:, 0]], ax[1][g[:, 1]], ax[2][g[:, 2]]], 1).astype(f32)
    k = np.arange(len(where))
    for d in range(3):
        sel = a == d
        lo, hi = ax[d][g[sel, d]], ax[d][g1[sel, d]]
        verts[k[sel], d] = lo + t[sel] * (hi - lo)
    case = np.zeros(tuple(v - 1 for v in n), np.int64)
    for i, d in enumerate(CORNER_OFF):
        case |= inside[d[0]:n[0] - 1 + d[0], d[1]:n[1] - 1 + d[1], d[2]:n[2] - 1 + d[2]].astype(np.int64) << i
    pc = np.argwhere(TABLE[case, 15] > 0)
    rows = TABLE[case[pc[:, 0], pc[:, 1], pc[:, 2]]]
    e = rows[:, :15].reshape(-1, 5, 3)
    keep = np.arange(5)[None, :] < rows[:, 15:16]
    e = np.where(keep[..., None], e, 0)
    q = pc[:, None, None, :] + CORNER_OFF[EDGE_CORNER[e]]
    tris = vid[q[..., 0], q[..., 1], q[..., 2], EDGE_AXIS[e]][keep]
    assert (tris >= 0).all(), "a triangle names an edge without a vertex"
    return verts, tris.astype(np.int32).reshape(-1, 3)


def finish(verts, center, radius, max_range=32.0):
    world, _ = uncontract(verts, center, radius)
    return np.clip(world, f32(-max_range), f32(max_range)).astype(f32)


def texture(verts, voxel_size, full_proj, depth, rgb):
    return fuse(verts, f32(5) * f32(voxel_size), full_proj, depth, rgb)[1]
