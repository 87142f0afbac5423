"""Torch restatement of PGSR's multi-view losses (gssr/scene/pgsr_scene.py:113-204 + helpers), device-agnostic, for timing the op chain
the fused kernels replace, for full-size parity and -- with dtype=torch.float64 -- as the truth of tests/mv_truth.py.  Like the reference it
walks through world coordinates (it never composes the two rigid transforms).  Cameras are the dicts of mv_cases (R, T, Fx, Fy, Cx, Cy); the
intrinsics are rounded to float32 first (what the reference's tensors and the kernels' configuration hold), then widened to `dtype`.
`ncc_scale` is the view camera's, used for both intrinsics.  TEST INFRASTRUCTURE."""
import numpy as np
import torch
import torch.nn.functional as F


def _f32(v):
    return float(np.float32(v))


def _cam32(cam):
    return {k: (_f32(cam[k]) if k in ("Fx", "Fy", "Cx", "Cy") else cam[k]) for k in cam}


def _rays(cam, W, H, dev, dtype=torch.float32):
    ix, iy = torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy")
    ix, iy = ix.to(dtype), iy.to(dtype)
    return torch.stack([(ix - cam["Cx"]) / cam["Fx"], (iy - cam["Cy"]) / cam["Fy"], torch.ones_like(ix)], -1)


def _lncc(ref, nea, parts=None):
    tps = nea.shape[1]
    rs, ns = ref.sum(1), nea.sum(1)
    r2, n2, rn = (ref * ref).sum(1), (nea * nea).sum(1), (ref * nea).sum(1)
    ravg, navg = rs / tps, ns / tps
    cross = rn - navg * rs
    rvar = r2 - ravg * rs
    nvar = n2 - navg * ns
    raw = 1 - cross * cross / (rvar * nvar + _f32(1e-8))
    ncc = torch.clamp(raw, 0.0, 2.0)
    if parts is not None:
        parts.update(r2=r2.detach(), n2=n2.detach(), rvar=rvar.detach(), nvar=nvar.detach(), ncc_raw=raw)
    return ncc, ncc < _f32(0.9)


def multiview_loss(plane_depth, near_plane_depth, normal, distance, gray, near_gray, vc, nc, lambda_geo=0.03, lambda_ncc=0.15, patch=3, th=1.0,
                   indices=None, aux=None, dtype=torch.float32, ncc_scale=1.0, parts=None, guarded=False):
    """-> (geo_loss, ncc_loss).  The maps may have three different sizes: plane_depth / normal / distance (H,W), near_plane_depth (Hn,Wn), both
    gray images (Hg,Wg).  `indices`: sampled pixels.  guarded=True (the float64 truth; off for the timing tools, which pass clean inputs and
    complete lists) drops entries < 0 and keeps non-finite coordinates away from grid_sample, whose CPU kernels index out of bounds on them:
    such a coordinate samples NaN (border padding: the pixel is off, as every comparison with NaN is false) or 0 (zero padding: what the
    kernel documents for a tap it cannot place).  `parts` (a dict) receives the intermediate tensors, those
    that carry gradient still attached to the graph: geo_sum / ncc_sum are the UNSCALED sums whose means the losses are."""
    dev = plane_depth.device
    H, W = plane_depth.shape[-2:]
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64) if not torch.is_tensor(a) else a, device=dev).to(dtype)
    vc, nc = _cam32(vc), _cam32(nc)
    s = _f32(ncc_scale)
    Rv, Tv, Rn, Tn = t(vc["R"]), t(vc["T"]), t(nc["R"]), t(nc["T"])
    ix, iy = torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy")
    pixels = torch.stack([ix, iy], -1).to(dtype)
    pts = (_rays(vc, W, H, dev, dtype) * plane_depth.squeeze()[..., None]).reshape(-1, 3)
    pts = (pts - Tv) @ Rv.t()
    q = pts @ Rn + Tn
    Hn, Wn = near_plane_depth.shape[-2:]
    proj = torch.stack([q[:, 0] * nc["Fx"] / q[:, 2] + nc["Cx"], q[:, 1] * nc["Fy"] / q[:, 2] + nc["Cy"]], -1)
    mask = (proj[:, 0] > 0) & (proj[:, 0] < Wn) & (proj[:, 1] > 0) & (proj[:, 1] < Hn) & (q[:, 2] > _f32(0.1))
    grid = torch.stack([proj[:, 0] / ((Wn - 1) / 2) - 1, proj[:, 1] / ((Hn - 1) / 2) - 1], -1).view(1, -1, 1, 2)
    if guarded:
        placed = torch.isfinite(grid).all(dim=-1, keepdim=True)
        grid = torch.where(placed, grid, torch.zeros_like(grid))
    map_z = F.grid_sample(near_plane_depth.reshape(1, 1, Hn, Wn), grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0]
    if guarded:
        map_z = torch.where(placed.view(1, -1), map_z, torch.full_like(map_z, float("nan")))
    qz = q[:, 2]
    q = q / q[:, 2:3] * map_z.squeeze()[..., None]
    back = ((q - Tn) @ Rn.t()) @ Rv + Tv
    bp = torch.stack([back[:, 0] * vc["Fx"] / back[:, 2] + vc["Cx"], back[:, 1] * vc["Fy"] / back[:, 2] + vc["Cy"]], -1)
    err = bp - pixels.reshape(-1, 2)
    noise = torch.norm(err, dim=-1)
    if aux is not None:          # per-pixel reprojection error and projection into the neighbour (callers that judge conditioning)
        aux.update(noise=noise.detach(), proj=proj.detach())
    d_mask = mask & (noise < _f32(th))
    weights = (1.0 / torch.exp(noise)).detach()
    weights = torch.where(d_mask, weights, torch.zeros_like(weights))
    zero = plane_depth.sum() * 0
    geo_sum = (weights * noise)[d_mask].sum()
    if parts is not None:
        parts.update(noise=noise, err=err, proj=proj, qz=qz, map_z=map_z, frustum=mask, d_mask=d_mask, weights=weights, geo_sum=geo_sum,
                     geo_count=int(d_mask.sum()), ncc_sum=zero, ncc_count=0)
    count = d_mask.sum()
    if count == 0:
        if parts is None:
            return zero, zero
        geo = zero
    else:
        geo = lambda_geo * geo_sum / count
    with torch.no_grad():
        valid = torch.nonzero(d_mask).squeeze(1) if indices is None else torch.as_tensor(indices, device=dev).long()
        if guarded:
            valid = valid[valid >= 0]
        if valid.numel() == 0:
            return geo, zero
        w = weights[valid]
        off = torch.arange(-patch, patch + 1, device=dev)
        oy, ox = torch.meshgrid(off, off, indexing="ij")
        offsets = torch.stack([ox, oy], -1).view(1, -1, 2).to(dtype)
        ori = pixels.reshape(-1, 2)[valid].reshape(-1, 1, 2) / s + offsets
        Hg, Wg = gray.shape[-2:]
        g = ori.clone()
        g[..., 0] = 2 * g[..., 0] / (Wg - 1) - 1.0
        g[..., 1] = 2 * g[..., 1] / (Hg - 1) - 1.0
        ref_val = F.grid_sample(gray.reshape(1, 1, Hg, Wg), g.view(1, -1, 1, 2), align_corners=True).reshape(-1, offsets.shape[1])
        r = Rn.t() @ Rv
        tt = -r @ Tv + Tn
    n = normal.permute(1, 2, 0).reshape(-1, 3)[valid]
    d = distance.reshape(-1)[valid]
    Hm = r[None] - (tt[None, :, None] * n[:, None, :]) / d[:, None, None]
    Kn = t([[nc["Fx"] / s, 0, nc["Cx"] / s], [0, nc["Fy"] / s, nc["Cy"] / s], [0, 0, 1]])
    Kvi = t([[s / vc["Fx"], 0, -vc["Cx"] / vc["Fx"]], [0, s / vc["Fy"], -vc["Cy"] / vc["Fy"]], [0, 0, 1]])
    Hk = Kn[None] @ Hm @ Kvi[None]
    homo = torch.cat([ori, torch.ones_like(ori[..., :1])], -1)
    gt_ = torch.einsum("bik,bpk->bpi", Hk, homo)
    grid2 = gt_[..., :2] / (gt_[..., 2:] + _f32(1e-10))
    gx = 2 * grid2[..., 0] / (Wg - 1) - 1.0
    gy = 2 * grid2[..., 1] / (Hg - 1) - 1.0
    if guarded:
        ok = torch.isfinite(gx) & torch.isfinite(gy)
        gx, gy = torch.where(ok, gx, torch.full_like(gx, -3.0)), torch.where(ok, gy, torch.full_like(gy, -3.0))      # far in the zero padding
    samp = F.grid_sample(near_gray.reshape(1, 1, Hg, Wg), torch.stack([gx, gy], -1).reshape(1, -1, 1, 2), align_corners=True).reshape(-1, offsets.shape[1])
    ncc, m = _lncc(ref_val, samp, parts)
    ncc_sum = (ncc * w)[m].sum()
    if parts is not None:
        parts.update(valid=valid, ncc=ncc.detach(), ncc_mask=m, ncc_sum=ncc_sum, ncc_count=int(m.sum()), warp=grid2, g2=gt_[..., 2].detach(),
                     ref_val=ref_val, samp=samp.detach())
    if m.sum() == 0:
        return geo, zero
    return geo, lambda_ncc * ncc_sum / m.sum()
