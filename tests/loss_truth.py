"""The fused image-space losses (L1 + SSIM, the 2DGS normal + distortion regulariser, the PGSR single-view normal loss) stated in float64, with a
per-element error scale for every output, every float32 decision named and measured, and the checker that holds a float32 result -- the HIP
kernels', the C oracle's -- to it element by element.  TEST INFRASTRUCTURE ONLY: numpy and float64 torch, no library, no gsrast.

The truth.  Values and gradients are torch autograd of tests/ref_loss_torch.py and tests/ref_geo_torch.py in float64 on the float32 inputs
widened exactly (the scalar parameters lambda, depth_ratio as the float32 the C ABI receives).  The geometric losses take ray_mat / normal_rot,
as the kernels do, not a camera: the 2DGS composition is restated here from ref_geo_torch's lattice and stencil, the PGSR one is
ref_geo_torch.plane_geo_loss with K = inverse(ray_mat^T).  One documented deviation: where autograd gives NaN on channels 0 / 1 of
allmap at alpha = 0 (0 * inf in the backward of the division) the truth is 0.

The scale.  Next to autograd, every loss is evaluated a second time with plain numpy in float64, each intermediate carried as a pair (value v,
error e): a RUNNING ERROR ANALYSIS (Higham, Accuracy and Stability of Numerical Algorithms, 3.3).  e is, in units of 2^-24, a first-order bound
on what one float32 evaluation of the same expression can be off by:
      inputs                      e = 0 (they are float32 numbers)
      s = a +- b                  e = e_a + e_b + |s|                                      the operands' errors pass, the result is rounded once
      p = a b                     e = |a| e_b + |b| e_a + |p|
      q = a / b                   e = (e_a + |q| e_b) / |b| + |q|
      r = sqrt(a)                 e = e_a / (2 r) + |r|
      f = window * a              e = window * e_a + 2 window * |a|                        (zero-padded 11 x 11 Gaussian; two passes of eleven taps)
      S = sum of n terms          e = sum e_i + (ceil(log2 n) + 4) sum |t_i|               a tree of float32 additions behind a short serial run
Unrolled, e of an output element is the sum of the absolute values of the terms whose signed sum is that element, each term multiplied by the
amplification of every cancelling subtraction on the way into one of its denominators -- which is the form the bounds take:
  dL/dimg   = w_l1 sign(x - y) - w_ssim (F[dS/dmu1] + 2 x F[dS/dE[x^2]] + y F[dS/dE[xy]])          (F = the window; it is its own adjoint)
      B2 = (E[x^2] - mu1^2) + (E[y^2] - mu2^2) + C2 carries e = E[x^2] + E[y^2] + mu1^2 + mu2^2 (+ lower order), so every map that divides by B2
      -- all three do -- has e = |map| (E[x^2] + E[y^2] + mu1^2 + mu2^2) / B2 + ...: on a smooth image B2 -> C2 = 9e-4 and the factor is in the
      thousands.  A2 = 2 (E[xy] - mu1 mu2) + C2 enters the numerators with the same absolute error.  dS/dmu1 is itself a difference of four terms
      (2 mu2 A2 / (B1 B2), 2 mu2 A1 / (B1 B2), 2 S mu1 / B1, 2 S mu1 / B2: they cancel exactly when img == gt) and is carried term by term.  Then
      scale(dL/dimg) = w_ssim (F[e(dS/dmu1)] + 2 |x| F[e(dS/dE[x^2])] + |y| F[e(dS/dE[xy])] + the magnitudes of the three products) + w_l1 |sign|.
  geo gradients.  P = depth * ray; dx = P(y+1) - P(y-1), dy = P(x+1) - P(x-1) carry e = e(P+) + e(P-) + |dx|: the cancellation of two points
      a pixel apart, |P| / |dx| ~ the focal length in pixels.  It passes through c = dx x dy (six products, term by term), len = |c|,
      inv = 1 / max(len, 1e-12), n = c inv, the projection dc = (dn - n (n . dn)) inv -- a second cancellation where the rendered normal
      agrees with n -- the cross products g_dx = dy x dc, g_dy = dc x dx, and the gather dP = g_dx(y-1) - g_dx(y+1) + g_dy(x-1) - g_dy(x+1):
      e(dP) = the four-stencil gather of e(g) + |g|.  dd = dP . ray, and the channels: dd (1-r) / alpha, -dd (1-r) allmap0 / alpha^2, dd r.
      A difference of two P that are the same float32 number in any evaluation order (equal depth inputs, and a ray component that does not
      depend on the coordinate that differs: its ray_mat coefficient is 0) has e = 0: that is how a fronto-parallel plane has exact zeros.
  scalars.  Sum of the per-pixel e plus the summation term above, over N.  loss = (1 - lambda) l1 + lambda (1 - ssim) carries the e of ssim
      against the difference from 1.
An element's bound is  K[quantity] * 2^-24 * e.  Where e == 0 the value is the same in every arithmetic (0 in all such places here) and a candidate
must hit it exactly: allmap channels 7-10, the border of the normal maps, dA[3:], every gradient of an image without interior pixels.

K is measured, never taken from the HIP library: per quantity, the largest deviation (in units of 2^-24 e) of the float32 C oracle
(oracle/gsl_oracle.c, the -ffp-contract=off build and its FMA twin) over every case of loss_cases, times 4, rounded up to a power of two (not
below 1: e is a worst-case bound for ONE operation order, and a K below 1 would promise more than that of another): the margin of mv_truth.BOUND, for its reason -- the kernels' operation order differs from both builds.  tests/test_loss_truth_cpu.py
measures again on every run and fails when 4 x a deviation exceeds its K.  EXPERIMENTS.md keeps the table.

Gates.  A pixel / element is ROBUST when every decision that feeds it is beyond its bound, FRAGILE otherwise, with the gate's name:
  nan0   allmap0 / alpha is taken with float32 semantics (a quotient that overflows float32 is inf -> 0 although float64 holds it).  Fragile when
         the float64 quotient is within 2^-22 (relative) of the float32 overflow threshold.  Feeds P of the pixel: everything within two pixels.
  len    |len - 1e-12| <= K e(len) 2^-24 (not where len == 0 with e == 0: an empty region is robustly clamped).  Feeds the n . dn term of the
         pixel's adjoint: the depth gradients within two pixels.
  sign   of the plane loss: |alpha n_c - normal_c| <= K[depth_normal] e 2^-24 (not where both are exact zeros).  Feeds dL_dnormal of the element,
         and, through dn and the adjoint, dL_ddepth of the pixel's four neighbours: those are fragile too.
  The L1 sign of the photometric loss is no gate: x - y has the exact sign in float32.
check() accepts a fragile element that is within its bound of the truth or of the value the OTHER side of its gate gives (within the bound that
side's own scale gives: other signs make other terms): for the sign gate the side the candidate took is read from its own dL_dnormal and dL_ddepth
is evaluated again with those signs on the fragile elements.
Underflow: below 2^-126 float32 numbers are 2^-149 apart whatever their size, so every bound of an element with e > 0 carries 2^-146 on top.
"""
import math

import numpy as np
import torch

import ref_geo_torch
import ref_loss_torch

EPS24 = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
UNDERFLOW = 2.0 ** -146      # below 2^-126 float32 numbers are 2^-149 apart whatever their size: eight spacings for a handful of operations down there
# quantity -> largest measured deviation of the two oracle builds, in units of 2^-24 * scale (test_loss_truth_cpu.py -s prints them; EXPERIMENTS.md keeps
# the table), and K >= 4 x that, a power of two, at least 1
MEASURED = dict(ssim_l1=0.05316, ssim_mean=0.02025, ssim_loss=0.02196, dL_dimg=0.1,
                surfel_err=0.03365, surfel_dist=0.09059, surfel_loss=0.09359, surfel_g_depth=0.04359, surfel_g_normal=0.1054, surfel_g_dist=0.3125, surfel_g_zero=0,
                surf_depth=0.5433, normal_world=0.8057, surf_normal=0.2343,
                plane_l1=0.06048, plane_loss=0.09681, plane_dL_ddepth=0.2419, plane_dL_dnormal=0.5726, depth_normal=0.3914)
K = dict(ssim_l1=1.0, ssim_mean=1.0, ssim_loss=1.0, dL_dimg=1.0,
         surfel_err=1.0, surfel_dist=1.0, surfel_loss=1.0, surfel_g_depth=1.0, surfel_g_normal=1.0, surfel_g_dist=2.0, surfel_g_zero=1.0,
         surf_depth=4.0, normal_world=4.0, surf_normal=1.0,
         plane_l1=1.0, plane_loss=1.0, plane_dL_ddepth=1.0, plane_dL_dnormal=4.0, depth_normal=2.0)


def k_for(dev):
    """the smallest power of two >= 4 x dev, not below 1"""
    return 1.0 if dev <= 0.25 else 2.0 ** math.ceil(math.log2(4.0 * dev))


# ------------------------------------------------------------------------------------------------------------ values with a running error
class R:
    """value v and first-order float32 error e (units of 2^-24) of the expression that produced it (module text)"""
    __slots__ = ("v", "e")
    __array_ufunc__ = None               # numpy scalars and arrays on the left defer to __radd__ & co.

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.array(np.broadcast_to(np.asarray(e, np.float64), self.v.shape))

    @staticmethod
    def of(x):
        return x if isinstance(x, R) else R(x)

    def __add__(self, o):
        o = R.of(o); v = self.v + o.v
        return R(v, self.e + o.e + np.abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        o = R.of(o); v = self.v - o.v
        return R(v, self.e + o.e + np.abs(v))

    def __rsub__(self, o):
        return R.of(o) - self

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = R.of(o); v = self.v * o.v
        return R(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return R(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + np.abs(v))

    def __rtruediv__(self, o):
        return R.of(o) / self

    def __getitem__(self, k):
        return R(self.v[k], self.e[k])

    def abs(self):
        return R(np.abs(self.v), self.e)

    def sqrt(self):
        v = np.sqrt(self.v)
        with np.errstate(all="ignore"):
            return R(v, np.where(v > 0, self.e / (2 * np.where(v > 0, v, 1.0)), np.sqrt(self.e * EPS24) / EPS24) + v)

    def where(self, mask, other=0.0):
        o = R.of(other)
        return R(np.where(mask, self.v, o.v), np.where(mask, self.e, o.e))

    def sum(self):
        n = max(self.v.size, 1)
        return R(self.v.sum(), self.e.sum() + (math.ceil(math.log2(n)) + 4) * np.abs(self.v).sum())

    def padded(self, shape, at):
        """zeros of `shape` with self at the slices `at`"""
        v, e = np.zeros(shape), np.zeros(shape)
        v[at] = self.v; e[at] = self.e
        return R(v, e)


def f32(x):
    """a Python scalar as the float32 the C ABI hands the kernel, widened"""
    return float(np.float32(x))


def _w64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------ L1 + SSIM
C1, C2 = ref_loss_torch.C1, ref_loss_torch.C2


def taps(sigma=ref_loss_torch.SIGMA):
    x = np.arange(ref_loss_torch.WIN, dtype=np.float64) - ref_loss_torch.WIN // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def window(a, g=None, mode="constant"):
    """the separable 11 x 11 window over the last two dims (zero padding unless `mode` says otherwise: a mutation)"""
    g = taps() if g is None else g
    r = g.size // 2
    H, W = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode=mode)
    rows = sum(g[k] * p[..., :, k:k + W] for k in range(g.size))
    return sum(g[k] * rows[..., k:k + H, :] for k in range(g.size))


def _F(r, g=None, mode="constant"):
    return R(window(r.v, g, mode), window(r.e, g, mode) + 2.0 * window(np.abs(r.v), g, mode))


def ssim_analytic(img, gt, lam, mut=None):
    """The photometric loss and dL/dimg in float64 numpy with running errors -> dict name -> R.  mut: a planted error (test_loss_truth_cpu.py):
    'edge_pad', 'sigma16', 'gt_for_img', 'seam_shift'."""
    x, y = R(_w64(img)), R(_w64(gt))
    lam = f32(lam)
    N = x.v.size
    g = taps(1.6) if mut == "sigma16" else taps()
    mode = "edge" if mut == "edge_pad" else "constant"
    mu1, mu2, e11, e22, e12 = _F(x, g, mode), _F(y, g, mode), _F(x * x, g, mode), _F(y * y, g, mode), _F(x * y, g, mode)
    c1, c2 = R(C1, C1), R(C2, C2)
    mu1s, mu2s, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1s, e22 - mu2s, e12 - mu12
    A1, A2, B1, B2 = 2.0 * mu12 + c1, 2.0 * s12 + c2, mu1s + mu2s + c1, s1 + s2 + c2
    inv = 1.0 / (B1 * B2)
    S = A1 * A2 * inv
    dmu = 2.0 * mu2 * A2 * inv - 2.0 * mu2 * A1 * inv - (S * 2.0 * mu1 / B1 - S * 2.0 * mu1 / B2)
    d11 = -(S / B2)
    d12 = 2.0 * A1 * inv
    Fm, F11, F12 = _F(dmu, g), _F(d11, g), _F(d12, g)
    if mut == "seam_shift":                  # the filtered maps of the tiles behind the first seam taken one pixel off
        for f in (Fm, F11, F12):
            for a in (f.v, f.e):
                a[..., 30:, 32:] = np.roll(a, 1, axis=-1)[..., 30:, 32:]
    sgn = np.sign(x.v - y.v)
    inv_n = R(1.0) / float(N)
    w_l1, w_ss = (1.0 - R(lam)) * inv_n, R(lam) * inv_n
    xs = y if mut == "gt_for_img" else x
    dimg = w_l1 * sgn - w_ss * (Fm + 2.0 * xs * F11 + y * F12)
    l1 = (x - y).abs().sum() / float(N)
    ss = S.sum() / float(N)
    loss = (1.0 - R(lam)) * l1 + R(lam) * (1.0 - ss)
    return dict(l1=l1, ssim=ss, loss=loss, dL_dimg=dimg, B2=B2, amp=(e11.v + e22.v + mu1s.v + mu2s.v) / B2.v)


SSIM_Q = dict(l1="ssim_l1", ssim="ssim_mean", loss="ssim_loss", dL_dimg="dL_dimg")


def ssim_truth(img, gt, lam):
    x = torch.tensor(_w64(img), requires_grad=True)
    L, l1, s = ref_loss_torch.loss(x, torch.tensor(_w64(gt)), f32(lam))
    L.backward()
    an = ssim_analytic(img, gt, lam)
    out = dict(l1=np.float64(l1.item()), ssim=np.float64(s.item()), loss=np.float64(L.item()), dL_dimg=x.grad.numpy())
    return _truth("ssim", out, an, SSIM_Q, {}, {}, extra=dict(amp=an["amp"], lam=f32(lam)))


# ------------------------------------------------------------------------------------------------------------------------ the stencil
_UP, _DN = (slice(None, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
_LF, _RT = (slice(1, -1), slice(None, -2)), (slice(1, -1), slice(2, None))
_IN = (slice(1, -1), slice(1, -1))


def _rays(H, W, rm):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return [R(xs) * rm[c] + R(ys) * rm[3 + c] + rm[6 + c] for c in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _stencil(P, keys, rm):
    """depth_to_normal on the interior -> dict(dx, dy, len, inv, n): c = (down - up) x (right - left), the vector both losses use"""
    with np.errstate(all="ignore"):
        eqv = np.all([k[_DN] == k[_UP] for k in keys], axis=0)
        eqh = np.all([k[_RT] == k[_LF] for k in keys], axis=0)
    dx, dy = [], []
    for c in range(3):
        a, b = P[c][_DN] - P[c][_UP], P[c][_RT] - P[c][_LF]
        dx.append(a.where(~(eqv & (rm[3 + c] == 0))))          # the same float32 number twice: 0 in any arithmetic
        dy.append(b.where(~(eqh & (rm[c] == 0))))
    cr = _cross(dx, dy)
    ln = (cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]).sqrt()
    on = ln.v > 1e-12
    inv = 1.0 / ln.where(on, 1e-12)
    return dict(dx=dx, dy=dy, len=ln, inv=inv, on=on, n=[cr[c] * inv for c in range(3)])


def _adjoint(st, dn, H, W, len_on=None):
    """dn = d loss / d n on the interior -> d loss / d P on the whole image (list of 3 R)"""
    n, inv, dx, dy = st["n"], st["inv"], st["dx"], st["dy"]
    on = st["on"] if len_on is None else len_on
    nd = (n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2]).where(on)
    dc = [(dn[c] - n[c] * nd) * inv for c in range(3)]
    gdx, gdy = _cross(dy, dc), _cross(dc, dx)
    out = []
    for c in range(3):
        Gx, Gy = gdx[c].padded((H + 2, W + 2), (slice(2, H), slice(2, W))), gdy[c].padded((H + 2, W + 2), (slice(2, H), slice(2, W)))
        out.append(((Gx[0:H, 1:W + 1] - Gx[2:H + 2, 1:W + 1]) + Gy[1:H + 1, 0:W]) - Gy[1:H + 1, 2:W + 2])
    return out


def _full(r, H, W):
    return r.padded((H, W), _IN) if H > 2 and W > 2 else R(np.zeros((H, W)))


def _stack(rs):
    return R(np.stack([r.v for r in rs]), np.stack([r.e for r in rs]))


def _dilate(m, r):
    H, W = m.shape
    p = np.pad(m, r)
    return np.any([p[i:i + H, j:j + W] for i in range(2 * r + 1) for j in range(2 * r + 1)], axis=0)


# ------------------------------------------------------------------------------------------------------------------------------- 2DGS geo
def _okq32(a0, a):
    with np.errstate(all="ignore"):
        return np.isfinite(np.asarray(a0, np.float32) / np.asarray(a, np.float32))


def surfel_analytic(allmap, ray_mat, normal_rot, depth_ratio, lambda_normal, lambda_dist, mut=None, flip_q=None, flip_len=None):
    """The 2DGS regulariser in float64 numpy with running errors.  mut: 'rot_transposed', 'normal_0p8', 'depth_1p01', 'ratio_swapped'.
    flip_q / flip_len: boolean maps of pixels whose nan0 / len decision is taken the other way (the other side of a fragile gate)."""
    am = _w64(allmap)
    rm, nr = _w64(ray_mat).reshape(-1), _w64(normal_rot).reshape(-1)
    _, H, W = am.shape
    N = H * W
    r, ln_, ld_ = f32(depth_ratio), f32(lambda_normal), f32(lambda_dist)
    a0, a, m = am[0], am[1], am[5]
    okq, okm = _okq32(allmap[0], allmap[1]), np.isfinite(m)
    if flip_q is not None:
        okq = okq ^ flip_q
    q = (R(np.where(okq, a0, 0.0)) / np.where(okq, a, 1.0)).where(okq)
    med = R(np.where(okm, m, 0.0))
    one_r = 1.0 - R(r)
    d = (q * r + one_r * med) if mut == "ratio_swapped" else (q * one_r + R(r) * med)
    ray = _rays(H, W, rm)
    P = [d * ray[c] for c in range(3)]
    keys = [np.where(okq, a0, 0.0), np.where(okq, a, 1.0), np.where(okm, m, 0.0)]
    st = _stencil(P, keys, rm)
    nv = [R(am[2 + i]) for i in range(3)]
    nw = [nv[0] * nr[c] + nv[1] * nr[3 + c] + nv[2] * nr[6 + c] for c in range(3)]
    wn, wd = R(ln_) / float(N), R(ld_) / float(N)
    ai = a[_IN]
    n = st["n"]
    dot = R(ai) * (nw[0][_IN] * n[0] + nw[1][_IN] * n[1] + nw[2][_IN] * n[2])
    err = 1.0 - _full(dot, H, W)
    dn = [-(wn * ai) * nw[c][_IN] for c in range(3)]
    on = st["on"] if flip_len is None else st["on"] ^ flip_len[_IN]
    dP = _adjoint(st, dn, H, W, on)
    dd = dP[0] * ray[0] + dP[1] * ray[1] + dP[2] * ray[2]
    asafe = np.where(okq, a, 1.0)
    g0 = (dd * one_r / asafe).where(okq)
    g1 = (-(dd * one_r) * np.where(okq, a0, 0.0) / (R(asafe) * asafe)).where(okq)
    g5 = (dd * r).where(okm)
    sn = [_full(n[c] * ai, H, W) for c in range(3)]
    k = 0.8 if mut == "normal_0p8" else 1.0
    if mut == "rot_transposed":
        gn = [-(wn * (nr[i] * sn[0] + nr[3 + i] * sn[1] + nr[6 + i] * sn[2])) for i in range(3)]
    else:
        gn = [-(wn * (nr[3 * i] * sn[0] + nr[3 * i + 1] * sn[1] + nr[3 * i + 2] * sn[2])) * k for i in range(3)]
    gd = _stack([g0, g1, g5])
    if mut == "depth_1p01":
        gd = gd * 1.01
    e_mean, d_mean = err.sum() / float(N), R(np.where(np.isfinite(am[6]), am[6], 0.0)).sum() / float(N)
    return dict(err=e_mean, dist=d_mean, loss=R(ln_) * e_mean + R(ld_) * d_mean, g_depth=gd, g_normal=_stack(gn),
                g_dist=R(np.zeros((H, W))) + wd, g_zero=R(np.zeros((4, H, W))), surf_depth=d, normal_world=_stack(nw), surf_normal=_stack(sn),
                len=_full(st["len"], H, W), q64=np.where(okq, a0, 0.0) / asafe, okq=okq)


SURFEL_Q = dict(err="surfel_err", dist="surfel_dist", loss="surfel_loss", g_depth="surfel_g_depth", g_normal="surfel_g_normal", g_dist="surfel_g_dist",
                g_zero="surfel_g_zero", surf_depth="surf_depth", normal_world="normal_world", surf_normal="surf_normal")


def _surfel_autograd(allmap, ray_mat, normal_rot, depth_ratio, lambda_normal, lambda_dist):
    am = torch.tensor(_w64(allmap), requires_grad=True)
    M, Rn = torch.tensor(_w64(ray_mat).reshape(3, 3)), torch.tensor(_w64(normal_rot).reshape(3, 3))
    _, H, W = am.shape
    r = f32(depth_ratio)
    okq = torch.tensor(_okq32(allmap[0], allmap[1]))
    alpha = am[1]
    expected = torch.where(okq, am[0] / alpha, torch.zeros_like(alpha))          # nan0 with the float32 decision
    median = torch.nan_to_num(am[5], nan=0.0, posinf=0.0, neginf=0.0)
    D = (1 - r) * expected + r * median
    X = D.unsqueeze(2) * (ref_geo_torch._lattice(H, W, am) @ M)                 # the camera centre cancels in the differences
    n_depth = ref_geo_torch._central_normals(X, flip=False) * alpha.detach().unsqueeze(2)
    n_world = torch.einsum("chw,cd->hwd", am[2:5], Rn)
    err = (1 - (n_world * n_depth).sum(dim=2)).mean()
    dist = am[6].mean()
    L = f32(lambda_normal) * err + f32(lambda_dist) * dist
    L.backward()
    g = am.grad.numpy()
    bad = ~np.isfinite(g)
    assert not bad[2:].any() and (~okq.numpy())[bad[0] | bad[1]].all(), "autograd NaN outside the documented place"
    g = np.where(bad, 0.0, g)
    return dict(err=np.float64(err.item()), dist=np.float64(dist.item()), loss=np.float64(L.item()), g_depth=g[[0, 1, 5]], g_normal=g[2:5], g_dist=g[6],
                g_zero=g[7:11], surf_depth=D.detach().numpy(), normal_world=n_world.detach().permute(2, 0, 1).numpy(),
                surf_normal=n_depth.detach().permute(2, 0, 1).numpy())


def surfel_truth(allmap, ray_mat, normal_rot, depth_ratio, lambda_normal, lambda_dist):
    args = (allmap, ray_mat, normal_rot, depth_ratio, lambda_normal, lambda_dist)
    out = _surfel_autograd(*args)
    an = surfel_analytic(*args)
    _, H, W = np.shape(allmap)
    with np.errstate(all="ignore"):
        q64 = np.abs(_w64(allmap[0]) / _w64(allmap[1]))
        frag_q = np.isfinite(q64) & (np.abs(q64 / (FLT_MAX * (1 + 2.0 ** -25)) - 1.0) < 2.0 ** -22)
    ln = an["len"]
    interior = np.zeros((H, W), bool); interior[_IN] = True
    frag_len = interior & (np.abs(ln.v - 1e-12) <= K["surfel_g_depth"] * EPS24 * ln.e) & (ln.e > 0)
    fragile, gate = {}, {}
    if frag_q.any() or frag_len.any():
        near = _dilate(frag_q | frag_len, 2)
        name = np.where(_dilate(frag_q, 2), "nan0", "len")
        for k, v in out.items():
            fragile[k] = np.broadcast_to(near, v.shape) if v.ndim else np.bool_(True)
            gate[k] = np.broadcast_to(name, v.shape) if v.ndim else "nan0/len"

    def other(_cand):
        alt = surfel_analytic(*args, flip_q=frag_q, flip_len=frag_len)
        return {k: alt[k] for k in out}
    return _truth("surfel", out, an, SURFEL_Q, fragile, gate, other if fragile else None,
                  extra=dict(len=ln.v, okq=an["okq"], frag_pixels=frag_q | frag_len))


# ------------------------------------------------------------------------------------------------------------------------------- PGSR geo
def plane_analytic(depth, alpha, normal, weight, ray_mat, lam, mut=None, signs=None, flip_len=None):
    """The PGSR single-view normal loss in float64 numpy with running errors.  signs: (3, H, W) array replacing sign(alpha n - normal);
    flip_len: pixels whose len > 1e-12 decision is taken the other way."""
    d, a, nm = _w64(depth).reshape(np.shape(alpha)), _w64(alpha), _w64(normal)
    H, W = a.shape
    N = H * W
    rm = _w64(ray_mat).reshape(-1)
    w = np.ones((H, W)) if weight is None else _w64(weight)
    lam = f32(lam)
    ray = _rays(H, W, rm)
    P = [R(d) * ray[c] for c in range(3)]
    st = _stencil(P, [d], rm)
    sn = [_full(st["n"][c] * a[_IN], H, W) for c in range(3)]
    s = [sn[c] - nm[c] for c in range(3)]
    for c in range(3):                                   # 0 - normal and x - 0 are exact
        exact = (sn[c].v == 0) & (sn[c].e == 0) | (nm[c] == 0)
        s[c] = R(s[c].v, np.where(exact, sn[c].e, s[c].e))
    sg = np.stack([np.sign(t.v) for t in s]) if signs is None else np.asarray(signs, np.float64)
    wl = (R(lam) / float(N)) * w
    dn = [(wl[_IN] * a[_IN]) * sg[c][_IN] for c in range(3)]
    dP = _adjoint(st, dn, H, W, None if flip_len is None else st["on"] ^ flip_len[_IN])
    dd = dP[0] * ray[0] + dP[1] * ray[1] + dP[2] * ray[2]
    if mut == "depth_1p01":
        dd = dd * 1.01
    l1 = ((s[0].abs() + s[1].abs() + s[2].abs()) * w).sum() / float(N)
    return dict(l1=l1, loss=R(lam) * l1, dL_ddepth=dd, dL_dnormal=_stack([wl * (-sg[c]) for c in range(3)]), depth_normal=_stack(sn), s=_stack(s),
                len=_full(st["len"], H, W), wl=wl.v)


PLANE_Q = dict(l1="plane_l1", loss="plane_loss", dL_ddepth="plane_dL_ddepth", dL_dnormal="plane_dL_dnormal", depth_normal="depth_normal")


def plane_truth(depth, alpha, normal, weight, ray_mat, lam):
    H, W = np.shape(alpha)
    d = torch.tensor(_w64(depth).reshape(H, W), requires_grad=True)
    am = torch.tensor(np.concatenate([_w64(normal), _w64(alpha)[None], np.zeros((1, H, W))]), requires_grad=True)
    K64 = torch.linalg.inv(torch.tensor(_w64(ray_mat).reshape(3, 3)).T)
    wt = None if weight is None else torch.tensor(_w64(weight))
    L, m, dn = ref_geo_torch.plane_geo_loss(d, am, K64, wt, f32(lam))
    L.backward()
    out = dict(l1=np.float64(m.item()), loss=np.float64(L.item()), dL_ddepth=d.grad.numpy(), dL_dnormal=am.grad.numpy()[0:3], depth_normal=dn.detach().numpy())
    args = (depth, alpha, normal, weight, ray_mat, lam)
    an = plane_analytic(*args)
    s = an["s"]
    frag_s = (np.abs(s.v) <= K["depth_normal"] * EPS24 * s.e) & (s.e > 0)
    px = frag_s.any(axis=0) & (an["wl"] * np.abs(_w64(alpha)) > 0)               # a pixel whose dn is 0 whatever the sign re-routes nothing
    nb = np.zeros((H, W), bool)
    nb[1:] |= px[:-1]; nb[:-1] |= px[1:]; nb[:, 1:] |= px[:, :-1]; nb[:, :-1] |= px[:, 1:]
    ln = an["len"]
    interior = np.zeros((H, W), bool); interior[_IN] = True
    frag_len = interior & (np.abs(ln.v - 1e-12) <= K["plane_dL_ddepth"] * EPS24 * ln.e) & (ln.e > 0)
    nb |= _dilate(frag_len, 1)
    fragile = dict(dL_dnormal=frag_s, dL_ddepth=nb)
    gate = dict(dL_dnormal=np.where(frag_s, "sign", ""), dL_ddepth=np.where(_dilate(frag_len, 1), "len", np.where(nb, "sign", "")))
    sg_truth = np.sign(s.v)

    def other(cand):
        g = np.asarray(cand["dL_dnormal"], np.float64).reshape(3, H, W)
        sg = np.where(frag_s, -np.sign(g) * np.sign(an["wl"]), sg_truth)
        alt = plane_analytic(*args, signs=sg, flip_len=frag_len if frag_len.any() else None)
        return dict(dL_ddepth=alt["dL_ddepth"], dL_dnormal=alt["dL_dnormal"])
    return _truth("plane", out, an, PLANE_Q, fragile, gate, other, extra=dict(s=s.v, s_err=s.e, len=ln.v, frag_pixels=px | frag_len))


# ----------------------------------------------------------------------------------------------------------------------- the checker
def _truth(kind, out, an, quantity, fragile, gate, other=None, extra=None):
    scale, analytic = {}, {}
    for k, v in out.items():
        out[k] = np.asarray(v, np.float64)
        scale[k] = np.asarray(an[k].e, np.float64).reshape(out[k].shape)
        analytic[k] = np.asarray(an[k].v, np.float64).reshape(out[k].shape)
    return dict(kind=kind, out=out, scale=scale, analytic=analytic, quantity=dict(quantity), fragile=fragile, gate=gate, other=other, **(extra or {}))


def split_allmap_grad(g):
    """(11, H, W) -> the four quantities of the surfel gradient"""
    g = np.asarray(g)
    return dict(g_depth=g[[0, 1, 5]], g_normal=g[2:5], g_dist=g[6], g_zero=g[7:11])


def check(cand, truth, label=""):
    """cand: dict name -> array / scalar (a subset of truth['out']; the gradients without any upstream factor).  -> (report, problems).
    report[name] = dict(worst: largest deviation of a robust element in units of 2^-24 * scale, K, fragile, took_other_side);
    report['fragile_share'] = the largest share of fragile elements of any output.  problems: what no bound forgives."""
    report, problems = {}, []
    alt = None
    share = 0.0
    for name, tv in truth["out"].items():
        if name not in cand or cand[name] is None:
            continue
        q = truth["quantity"][name]
        c = np.asarray(cand[name], np.float64).reshape(tv.shape)
        scale = truth["scale"][name]
        frag = np.broadcast_to(truth["fragile"].get(name, False), tv.shape)
        if not np.isfinite(c).all():
            problems.append(f"{label} {name}: {int((~np.isfinite(c)).sum())} non-finite values")
            c = np.nan_to_num(c, nan=np.inf)
        bound = K[q] * EPS24 * scale + np.where(scale > 0, UNDERFLOW, 0.0)
        with np.errstate(all="ignore"):
            dev = np.abs(c - tv)
            units = np.where(scale > 0, np.maximum(dev - UNDERFLOW, 0.0) / (EPS24 * np.where(scale > 0, scale, 1.0)), np.where(dev > 0, np.inf, 0.0))
        ok = dev <= bound
        exact = (scale == 0) & ~frag
        if (c[exact] != 0).any():
            problems.append(f"{label} {name}: {int((c[exact] != 0).sum())} non-zeros where every arithmetic gives 0")
        bad = ~ok & ~frag & ~exact
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, units, 0)), tv.shape)
            problems.append(f"{label} {name}: {int(bad.sum())} robust elements beyond K={K[q]:g}, worst {units[i]:.3g} units at {tuple(int(j) for j in i)} "
                            f"(got {c[i]:.9g}, truth {tv[i]:.9g})")
        took = 0
        if (frag & ~ok).any():
            if alt is None:
                alt = truth["other"](cand)
            av, ae = (np.asarray(x, np.float64).reshape(tv.shape) for x in (alt[name].v, alt[name].e))       # the other side with ITS scale: other signs, other terms
            ok2 = np.abs(c - av) <= K[q] * EPS24 * ae + np.where(ae > 0, UNDERFLOW, 0.0)
            lost = frag & ~ok & ~ok2
            took = int((frag & ~ok & ok2).sum())
            if lost.any():
                i = np.unravel_index(np.argmax(lost), tv.shape)
                problems.append(f"{label} {name}: {int(lost.sum())} fragile elements on neither side of their gate "
                                f"({np.broadcast_to(truth['gate'][name], tv.shape)[i]}), first at {tuple(int(j) for j in i)}")
        report[name] = dict(worst=float(units[~frag].max(initial=0.0)), K=K[q], fragile=int(frag.sum()), took_other_side=took)
        share = max(share, float(frag.mean()) if tv.ndim else 0.0)
    report["fragile_share"] = share
    return report, problems
