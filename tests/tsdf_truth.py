"""The block-sparse TSDF volume stated plainly in float64 (numpy only): the operation as the header comment of csrc/gsr_tsdf_sparse.hip states it,
not a port of oracle/gsr_oracle.c (which follows the kernel's float32 operation order).

Per frame: every `stride`-th pixel with 0 < d <= depth_trunc is back-projected with the float32-rounded inverse extrinsic; the units of 16^3 voxels
overlapping [p - trunc, p + trunc] are opened; every unit opened or touched again this frame gets the voxel rule ONCE: voxel centre
(16 coord + i + 0.5) voxel_length, pixel floor(x fx / z + cx + 0.5), sdf = (d - z) |ray|, update where sdf > -trunc with min(1, sdf / trunc), running
means of tsdf and colour, weight + 1.  Colours: quant 0 as given, 1 clamp to [0,1] x 255, 2 additionally truncated to an integer.
Float32 inputs (voxel_length, sdf_trunc, intrinsics, extrinsic, depth, colours, depth_trunc) are converted exactly; everything after is float64.

A comparison against float32 code is only honest away from the decisions a rounding can flip, so the truth also says where those are:
  * a voxel is FRAGILE if in any frame |z| < Z_EPS, its pixel coordinate uf or vf lies within PIX_EPS of an integer, or |sdf + trunc| < SDF_EPS trunc;
  * a sample is fragile if (p -+ trunc) / unit_len lies within UNIT_EPS of an integer (it might open another set of units);
  * per frame and sample: its index i (wave i // 64 and workgroup i // 256 of the two touch kernels) and the unit box lo..hi it opens."""
import numpy as np

RES = 16
Z_EPS, PIX_EPS, SDF_EPS, UNIT_EPS = 1e-4, 1e-3, 1e-4, 1e-4
KEY_LO, KEY_HI = -(1 << 20) + 1, (1 << 20) - 2      # the unit coordinates a 21-bit key field holds (all-ones is the empty key)


def _f32(x):
    return float(np.float32(x))


def frame_samples(depth, fx, fy, cx, cy, extrinsic, voxel_length, sdf_trunc, depth_trunc=float("inf"), stride=4):
    """The sampled pixels of one frame -> dict(n: samples the touch kernels launch over, i [m]: indices of the valid ones, p [m,3] world points,
    lo / hi [m,3] unit boxes, fragile [m])."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    d = d.reshape(d.shape[-2], d.shape[-1])
    H, W = d.shape
    fx, fy, cx, cy, vl, trunc = (_f32(v) for v in (fx, fy, cx, cy, voxel_length, sdf_trunc))
    dtrunc = _f32(min(depth_trunc, 3.0e38))
    unit_len = RES * vl
    E = np.asarray(extrinsic, np.float32).astype(np.float64).reshape(4, 4)
    P = np.linalg.inv(E).astype(np.float32).astype(np.float64)
    nu, nv = (W + stride - 1) // stride, (H + stride - 1) // stride
    i = np.arange(nu * nv)
    u, v = (i % nu) * stride, (i // nu) * stride
    dd = d[v, u]
    with np.errstate(invalid="ignore"):
        ok = (dd > 0) & (dd <= dtrunc)
    i, u, v, dd = i[ok], u[ok], v[ok], dd[ok]
    pc = np.stack([(u - cx) * dd / fx, (v - cy) * dd / fy, dd], axis=1)
    p = pc @ P[:3, :3].T + P[:3, 3]
    a, b = (p - trunc) / unit_len, (p + trunc) / unit_len
    lo, hi = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    fragile = ((np.abs(a - np.round(a)) < UNIT_EPS) | (np.abs(b - np.round(b)) < UNIT_EPS)).any(axis=1)
    if len(i) and (lo.min() < KEY_LO or hi.max() > KEY_HI or (hi - lo).max() > 3):
        raise ValueError("a sample lies outside the addressable volume or opens more than 4 units on an axis")
    return dict(n=nu * nv, i=i, p=p, lo=lo, hi=hi, fragile=fragile)


def texel_colours(rgb, quant):
    """[3,H,W] float32 -> [H,W,3] float64 on the scale the volume stores."""
    c = np.asarray(rgb, np.float32).astype(np.float64)
    c = np.moveaxis(c.reshape(3, c.shape[-2], c.shape[-1]), 0, -1)
    if quant:
        c = np.clip(c, 0.0, 1.0) * 255.0
        if quant == 2:
            c = np.floor(c)
    return c


class SparseTruth:
    def __init__(self, voxel_length, sdf_trunc, stride=4):
        self.vl, self.trunc, self.stride = _f32(voxel_length), _f32(sdf_trunc), int(stride)
        self.index = {}                                            # unit coordinate -> row, in first-touch order
        self.tsdf = np.zeros((0, RES, RES, RES)); self.weight = np.zeros((0, RES, RES, RES)); self.color = np.zeros((0, RES, RES, RES, 3))
        self.fragile = np.zeros((0, RES, RES, RES), bool)
        self.behind = np.zeros((0, RES, RES, RES), bool)           # z <= 0 in some frame that integrated the unit
        self.outside = np.zeros((0, RES, RES, RES), bool)          # z > 0 and projected outside the image in some such frame
        self.samples = []                                          # frame_samples() of every frame
        self.touched = []                                          # per frame: (rows of the units it integrated, how many of them it opened)

    def integrate(self, rgb, depth, fx, fy, cx, cy, extrinsic, depth_trunc=float("inf"), quant=2):
        s = frame_samples(depth, fx, fy, cx, cy, extrinsic, self.vl, self.trunc, depth_trunc, self.stride)
        self.samples.append(s)
        n0, rows = len(self.index), []
        seen = set()
        for lo, hi in zip(s["lo"].tolist(), s["hi"].tolist()):
            for x in range(lo[0], hi[0] + 1):
                for y in range(lo[1], hi[1] + 1):
                    for z in range(lo[2], hi[2] + 1):
                        k = (x, y, z)
                        if k not in seen:
                            seen.add(k)
                            rows.append(self.index.setdefault(k, len(self.index)))
        grow = len(self.index) - n0
        if grow:
            pad = lambda a: np.concatenate([a, np.zeros((grow,) + a.shape[1:], a.dtype)])
            self.tsdf, self.weight, self.color = pad(self.tsdf), pad(self.weight), pad(self.color)
            self.fragile, self.behind, self.outside = pad(self.fragile), pad(self.behind), pad(self.outside)
        self.touched.append((np.array(rows, np.int64), grow))
        if rows:
            self._voxel_rule(np.array(rows, np.int64), rgb, depth, fx, fy, cx, cy, extrinsic, depth_trunc, quant)
        return self

    def _voxel_rule(self, rows, rgb, depth, fx, fy, cx, cy, extrinsic, depth_trunc, quant):
        d = np.asarray(depth, np.float32).astype(np.float64)
        d = d.reshape(d.shape[-2], d.shape[-1])
        H, W = d.shape
        col = texel_colours(rgb, quant)
        fx, fy, cx, cy = (_f32(v) for v in (fx, fy, cx, cy))
        dtrunc = _f32(min(depth_trunc, 3.0e38))
        E = np.asarray(extrinsic, np.float32).astype(np.float64).reshape(4, 4)
        coords = np.array(list(self.index), np.int64)[rows]                              # [m, 3]
        g = np.arange(RES)
        local = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1)                    # [16,16,16,3] indexed [x, y, z]
        centre = (RES * coords[:, None, None, None, :] + local[None] + 0.5) * self.vl    # [m,16,16,16,3]
        cam = centre @ E[:3, :3].T + E[:3, 3]
        xc, yc, zc = cam[..., 0], cam[..., 1], cam[..., 2]
        front = zc > 0
        fragile = np.abs(zc) < Z_EPS
        zs = np.where(front, zc, 1.0)
        uf, vf = xc * fx / zs + cx + 0.5, yc * fy / zs + cy + 0.5
        fragile |= front & ((np.abs(uf - np.round(uf)) < PIX_EPS) | (np.abs(vf - np.round(vf)) < PIX_EPS))
        inside = front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        u, v = np.where(inside, np.floor(uf), 0).astype(np.int64), np.where(inside, np.floor(vf), 0).astype(np.int64)
        dd = d[v, u]
        with np.errstate(invalid="ignore"):
            ok = inside & (dd > 0) & (dd <= dtrunc)
        dd = np.where(ok, dd, 0.0)
        ray = np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0)
        sdf = (dd - zc) * ray
        fragile |= ok & (np.abs(sdf + self.trunc) < SDF_EPS * self.trunc)
        upd = ok & (sdf > -self.trunc)
        t = np.minimum(1.0, sdf / self.trunc)
        w0 = self.weight[rows]
        w1 = w0 + 1.0
        self.tsdf[rows] = np.where(upd, (self.tsdf[rows] * w0 + t) / w1, self.tsdf[rows])
        self.color[rows] = np.where(upd[..., None], (self.color[rows] * w0[..., None] + col[v, u]) / w1[..., None], self.color[rows])
        self.weight[rows] = np.where(upd, w1, w0)
        self.fragile[rows] |= fragile
        self.behind[rows] |= ~front
        self.outside[rows] |= front & ~inside

    def units(self):
        """-> (coords [n,3] int32, tsdf, weight [n,16,16,16] float64, color [n,16,16,16,3] float64, fragile [n,16,16,16] bool), x-major like units()."""
        return np.array(list(self.index), np.int32).reshape(-1, 3), self.tsdf, self.weight, self.color, self.fragile


TSDF_BAR, COLOUR_BAR = 1e-4, 0.05      # the bars of test_gpu_tsdf._compare, here without a forgiven fraction


def robust_errors(got, tv):
    """Units (coords, tsdf, weight, color) as numpy arrays against a SparseTruth -> (weight mismatches, worst |tsdf| error, worst colour error, robust
    updated voxels, fragile share) over the ROBUST voxels; the unit sets must be equal; what the truth never updated must read exactly 0."""
    co, t, w, c = got
    rco, rt, rw, rc, frag = tv.units()
    want = {tuple(k): i for i, k in enumerate(rco.tolist())}
    have = [tuple(k) for k in co.tolist()]
    assert len(set(have)) == len(have) and set(have) == set(want), (len(have), len(want), len(set(have) ^ set(want)))
    order = np.array([want[k] for k in have], np.int64)
    rt, rw, rc, ok = rt[order], rw[order], rc[order], ~frag[order]
    nw = int((w[ok] != rw[ok]).sum())
    same = ok & (w == rw)
    et = float(np.abs(t - rt)[same].max()) if same.any() else 0.0
    ec = float(np.abs(c - rc)[same].max()) if same.any() else 0.0
    never = ok & (rw == 0)
    assert not t[never].any() and not w[never].any() and not c[never].any()
    return nw, et, ec, int((ok & (rw > 0)).sum()), float(frag.mean())


# ---- the hash of csrc/gsr_tsdf_view.h on the host (python integers): keys, first probe positions, and where linear probing puts a list of units
def ts_pack(x, y, z):
    return ((x + (1 << 20)) << 42) | ((y + (1 << 20)) << 21) | (z + (1 << 20))


def ts_hash(key, log2cap):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - log2cap)


def probe_positions(coords, log2cap):
    """Linear probing of the list in order -> [(first probe position, final position)].  The SET of occupied entries does not depend on the order the
    device's threads insert in, so neither does whether the cluster runs over the end of the table."""
    used, out = set(), []
    for c in coords:
        h0 = h = ts_hash(ts_pack(*(int(v) for v in c)), log2cap)
        while h in used:
            h = (h + 1) & ((1 << log2cap) - 1)
        used.add(h)
        out.append((h0, h))
    return out


def probe_wraps(coords, log2cap):
    return any(h < h0 for h0, h in probe_positions(coords, log2cap))
