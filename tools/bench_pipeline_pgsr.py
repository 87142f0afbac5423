"""End-to-end PGSR iteration after step 7000 on a synthetic scene (two cameras, P Gaussians, 1920x1080):
    activations -> per-Gaussian all_map -> diff_plane_rasterization fwd (view) -> same for the neighbour camera ->
    L1+SSIM + single-view normal loss + multi-view geometric / NCC losses -> backward -> fused Adam.
--glue hip   : gsrast.plane_prep / gsrast.losses (fused HIP kernels) around the HIP rasterizer: the product iteration, gsrast.methods.pgsr
--glue torch : the reference's torch op chains (tests/ref_*_torch.py restatements, each checked against reference-run fixtures) around
               the SAME HIP rasterizer -- what a user gets by swapping only the rasterizer extension (`baseline` below).  One JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
import diff_plane_rasterization as dpr   # noqa: E402
from gsrast import methods             # noqa: E402
from bench_pipeline import timed       # noqa: E402


def q2m(q):
    r, i, j, k = torch.unbind(q, -1); two_s = 2.0 / (q * q).sum(-1)
    return torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r), two_s * (i * j + k * r),
                        1 - two_s * (i * i + k * k), two_s * (j * k - i * r), two_s * (i * k - j * r), two_s * (j * k + i * r),
                        1 - two_s * (i * i + j * j)), -1).reshape(-1, 3, 3)


def torch_all_map(xyz, rot, scl, V, cpos):
    R = q2m(rot)
    idx = scl.min(dim=-1)[1][..., None, None].expand(-1, 3, -1)
    n = R.gather(2, idx).squeeze(2)
    neg = (n * (cpos - xyz)).sum(-1) < 0.0
    n = torch.where(neg[:, None], -n, n)
    ln = n @ V[:3, :3]
    pc = xyz @ V[:3, :3] + V[3, :3]
    am = torch.zeros(xyz.shape[0], 5, device=xyz.device)
    am[:, :3] = ln; am[:, 3] = 1.0; am[:, 4] = (ln * pc).sum(-1).abs()
    return am


def build(a, dev):
    """-> (step, st): one PGSR training iteration after step 7000 (two plane renders + single-view + multi-view losses); a has .glue, .P."""
    return methods.pgsr(dev, a.P) if a.glue == "hip" else baseline(a, dev)


def baseline(a, dev):
    """The iteration of gsrast.methods.pgsr with the reference's torch op chains around the rasterizer: one set of leaves (autograd adds the two
    renders' gradients), fresh gradient carriers per render, one summed loss."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_geo_torch, ref_loss_torch, ref_mv_torch
    S = methods.pgsr_setup(dev, a.P)
    (xyz, scl_log, rot_raw, op_raw, col), opt, T = S.first, S.opt, S.T
    with torch.no_grad():                                                 # a fixed sample set of the reference's size: the reference draws its <= 102400
        idx = torch.randperm(methods.W * methods.H, device=dev)[:102400]  # samples with np.random.choice on the host; here only the op chain is timed

    def render(tt, rs, scl, rot, op):
        am = torch_all_map(xyz, rot, scl, tt["viewmatrix"], tt["campos"])
        m2 = torch.zeros_like(xyz, requires_grad=True); m2a = torch.zeros_like(xyz, requires_grad=True)
        return dpr.GaussianRasterizer(rs)(means3D=xyz, means2D=m2, means2D_abs=m2a, opacities=op, colors_precomp=col, scales=scl, rotations=rot, all_map=am)

    def step():
        scl = torch.exp(scl_log); rot = torch.nn.functional.normalize(rot_raw); op = torch.sigmoid(op_raw)
        img, radii, obs, oam, pd = render(*S.views[0], scl, rot, op)
        pd2 = render(*S.views[1], scl, rot, op)[4]
        loss = ref_loss_torch.loss(img.unsqueeze(0), T.gt.unsqueeze(0), 0.2)[0] + ref_geo_torch.plane_geo_loss(pd.squeeze(0), oam, T.K1, T.weight, 0.015)[0]
        geo, ncc = ref_mv_torch.multiview_loss(pd, pd2, oam[0:3], oam[4:5], T.gray1, T.gray2, T.c1, T.c2, indices=idx)
        (loss + geo + ncc).backward()
        opt.step(); opt.zero_grad(set_to_none=True)

    return step, {"P": a.P, "optimizers": [opt], "idx": idx}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--glue", default="hip", choices=["hip", "torch"])
    ap.add_argument("--P", type=int, default=methods.SIZES["pgsr"]["P"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    st, dt = timed(a, build)
    print(json.dumps({"pipeline": "pgsr (step > 7000: two renders + single-view + multi-view losses)", "glue": a.glue, "P": a.P, "steps": a.steps,
                      "ms_per_iter": round(1e3 * dt / a.steps, 3), "iters_per_s": round(a.steps / dt, 1)}))


if __name__ == "__main__":
    main()
