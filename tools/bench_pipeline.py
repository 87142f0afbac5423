"""End-to-end scaffold-2dgs iteration on synthetic anchors (BASELINE.json configs[1] with its neural-Gaussian decode in front):
    prefilter (scaffold_filter.visible_filter) -> neural-Gaussian decode -> diff_surfel_rasterization fwd -> loss -> backward -> fused Adam.
--decode hip   : gsrast.decode (fused HIP, include/gsdecode.h); with --loss bench | full-hip this is the product iteration, gsrast.methods.scaffold
--decode torch : the reference's torch op chain for the decode (tests/ref_decode_torch.py transcription), same rasterizer
--loss full-torch : the reference's torch loss formulas.  The two torch baselines are `baseline` below, on the product's set-up.
Na anchors x k=10 offsets sized so that ~300k Gaussians reach the rasterizer at 1920x1080.  One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
import diff_surfel_rasterization as dsr   # noqa: E402
from gsrast import decode, methods     # noqa: E402
from gsrast.losses import scaling_prod_mean, l1_plus_linear, l1_ssim, surfel_geo_loss  # noqa: E402


def build(a, dev, seed=0):
    """-> (step, st): one scaffold-2dgs (a.lod: octree-2dgs) training iteration; a has .decode, .loss, .Na and optionally .static, .lod, .stop_after."""
    kw = dict(lod=bool(getattr(a, "lod", False)), static=bool(getattr(a, "static", False)), seed=seed)
    if a.decode == "hip" and a.loss != "full-torch":
        return methods.scaffold(dev, a.Na, loss=a.loss, stop_after=getattr(a, "stop_after", None), **kw)
    return baseline(a, dev, **kw)


def baseline(a, dev, lod, static, seed):
    """The iteration of gsrast.methods.scaffold with the reference's torch op chains in place of the fused decode (and its statistics and scaling
    loss: x*y on unbound columns -- prod's backward synchronises the host when an entry is 0, slices cost one zero-filled (P,3) gradient each)
    and / or of the fused losses."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_decode_torch, ref_geo_torch, ref_loss_torch
    S = methods.scaffold_setup(dev, a.Na, lod, seed)
    L, opt, hip = S.L, S.opt, a.decode == "hip"
    heads = {w + n: getattr(L["mlp_" + n][i], "weight" if w[0] == "W" else "bias") for n in "ock" for w, i in (("W1", 0), ("b1", 0), ("W2", 2), ("b2", 2))}
    st, carriers = {"optimizers": [opt]}, {}

    def step():
        scaling = torch.exp(L["scaling_log"])
        with torch.no_grad():
            vmask = S.visible(scaling)
        app, count = L["emb"].weight[1], None
        if hip:
            vis_idx = decode.compact_visible(vmask, padded=True)
            out = decode.neural_gaussians(L["anchor"], L["feat"], L["offset"], scaling, L["mlp_o"], L["mlp_c"], L["mlp_k"], S.campos, vis_idx=vis_idx,
                                          appearance=app, static_rows=static, deferred=not static)
            xyz, color, opacity, scl, rot, nop, mask, count = out if static else (*out.finish(), None)
            reg = scaling_prod_mean(scl, 0.01, cols=2, count=count, unit_upstream=True)
        else:
            o, _ = ref_decode_torch.decode_live({"k": methods.K, "dist_o": False, "dist_c": False, "dist_k": False},
                                                {"anchor": L["anchor"], "feat": L["feat"], "offset": L["offset"], "scaling": scaling},
                                                {**heads, "app": app}, torch.nonzero(vmask).view(-1), S.campos)
            xyz, color, opacity, scl, rot = o["xyz"], o["color"], o["opacity"].view(-1, 1), o["scaling"], o["rot"]
            sx, sy, _sz = scl.unbind(dim=1)
            reg = 0.01 * (sx * sy).mean()
        means2D = methods.carriers_for(carriers, 0, xyz, True, n=1)[0] if static else torch.zeros_like(xyz, requires_grad=True)
        img, rad, allmap = dsr.GaussianRasterizer(S.rs)(means3D=xyz, means2D=means2D, opacities=opacity, colors_precomp=color,
                                                        scales=scl[:, :2].contiguous(), rotations=rot)
        if a.loss == "bench":
            loss = l1_plus_linear(img, S.gt, allmap, S.wmap) + reg
        elif a.loss == "full-hip":
            loss = l1_ssim(img, S.gt, 0.2, unit_upstream=True) + surfel_geo_loss(allmap, S.rm, S.nr, 0.0, 0.05, 100.0, unit_upstream=True)[0] + reg
        else:
            loss = ref_loss_torch.loss(img.unsqueeze(0), S.gt.unsqueeze(0), 0.2)[0] + ref_geo_torch.geo_loss(allmap, S.wvt, S.fpt, 0.0, 0.05, 100.0)[0] + reg
        loss.backward()
        if a.loss != "bench":                                    # densify(): training_statis every iteration (scaffold_gaussian.py:707-712)
            if hip:
                decode.training_stats_(*S.acc.values(), means2D.grad, nop, rad > 0, mask, vis_idx=vis_idx)
            else:
                ref_decode_torch.training_statis(S.acc, methods.K, means2D.grad, o["neural_opacity"].view(-1, 1), rad > 0, o["mask"], vmask)
        opt.step(); opt.zero_grad(set_to_none=True)
        if "Nv" not in st:
            st["Nv"] = int(vmask.sum())
            st["P"] = xyz.shape[0] if count is None else int(count[0])
        st["rows"] = xyz.shape[0]
        return loss

    return step, st


def timed(a, build):
    """Builds the iteration (a.graph: its static form, recorded into a HIP graph and replayed -- gsrast.graphs.GraphedStep), warms it up and
    times a.steps of it -> (st, seconds)."""
    graph = getattr(a, "graph", False)
    a.static = graph or getattr(a, "static", False)
    step, st = build(a, torch.device("cuda:0"))
    if graph:
        from gsrast.graphs import GraphedStep
        step = GraphedStep(step, optimizers=st["optimizers"], warmup=max(3, a.warmup))
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    if graph:
        st["async_status"] = step.check()
    st["mode"] = "graph" if graph else ("static" if a.static else "eager")
    return st, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", default="hip", choices=["hip", "torch"])
    ap.add_argument("--loss", default="bench", choices=["bench", "full-hip", "full-torch"],
                    help="bench: L1 + linear aux (bench.py's loss); full-*: the reference's L1+SSIM + normal/dist regularisers + scaling loss, "
                         "fused HIP kernels or the reference's torch formulas")
    ap.add_argument("--Na", type=int, default=methods.SIZES["scaffold-2dgs"]["Na"])
    ap.add_argument("--lod", action="store_true", help=f"octree-2dgs: level-of-detail mask + prefilter (use --Na {methods.SIZES['octree-2dgs']['Na']} for ~300k Gaussians)")
    ap.add_argument("--static", action="store_true", help="sync-free static-shape iteration (decode static_rows)")
    ap.add_argument("--graph", action="store_true", help="record the (static) iteration into a HIP graph and replay it (gsrast.graphs.GraphedStep)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    st, dt = timed(a, build)
    print(json.dumps({"pipeline": "octree-2dgs" if a.lod else "scaffold-2dgs", "mode": st["mode"],
                      "rows": st.get("rows"), "async_status": st.get("async_status"), "decode": a.decode, "loss": a.loss, "Na": a.Na, "Nv": st["Nv"], "P": st["P"], "steps": a.steps,
                      "ms_per_iter": 1e3 * dt / a.steps, "iters_per_s": a.steps / dt}))


if __name__ == "__main__":
    main()
