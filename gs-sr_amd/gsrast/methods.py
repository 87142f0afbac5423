"""The complete training iterations of the four methods on synthetic 1920x1080 scenes (BASELINE.json configs): how the package's ops compose
into the reference's training loop.  build(name, dev) -> (step, st); bench.py --full reports them as `method_iteration`.
    scaffold-2dgs: prefilter (scaffold_filter.visible_filter) -> neural-Gaussian decode -> diff_surfel_rasterization -> L1+SSIM + normal /
        distortion regularisers + scaling loss -> backward -> training statistics -> fused Adam (configs[1]).
    octree-2dgs:   the same behind OctreeScene's level-of-detail mask + prefilter (gsr_octree_visible), anchors on 6 levels (configs[3]/[4]).
    octree-pgsr:   after step 7000 (OctreePGSRScene.get_train_loss_dict, octree_pgsr_scene.py:26-45), for the view camera AND its neighbour:
        LOD mask + prefilter -> decode -> per-Gaussian all_map -> diff_plane_rasterization; then L1+SSIM + single-view normal + multi-view
        geometric / NCC + scaling losses -> backward (both renders, both decodes) -> training statistics -> fused Adam (configs[2]).
    pgsr:          the same two renders and losses on P explicit Gaussians (activations as one kernel each way, no decode).
What replaces what, in the order an iteration meets it:
  * eager (reference-shaped rows) decodes are DEFERRED (decode.PendingDecode): the count is read once the opacity head and its scan are done,
    while the emit kernel runs and the host enqueues what follows; with two cameras both decodes are in flight before the first count is read.
  * static=True is the sync-free, static-shape form (decode static_rows) that gsrast.graphs.GraphedStep records into a HIP graph.
  * the neighbour camera's pass reads a second set of leaves over the same storage (optim.shadow_parameters) and the optimizer adds the two
    passes' gradients inside its update kernel: with one set autograd sums them with one `add` launch per shared tensor (27 per octree-pgsr
    iteration, 130 us; five of the nine adds of the explicit iteration).
  * a loss that is a SUM of terms is backpropagated as roots with unit gradients (backward_unit).
  * the screen-space gradient carriers are persistent (carriers_for) where the reference fills fresh (P,3) zeros per render.
Nothing here reads the environment or imports from tests/ or tools/; the torch baselines of these iterations live in tools/bench_pipeline*.py."""
import types

import torch

import diff_plane_rasterization as dpr
import diff_surfel_rasterization as dsr
import scaffold_filter as sf
from . import decode, octree, runner, workloads
from .activations import gaussian_activations
from .losses import camera_ray_matrices, l1_plus_linear, l1_ssim, multiview_cfg, plane_losses, scaling_prod_mean, surfel_geo_loss
from .optim import Adam, shadow_parameters
from .plane_prep import plane_input_all_map

W, H, K, A, LEVELS, FORK = 1920, 1080, 10, 32, 6, 2.0
SIZES = {"scaffold-2dgs": {"Na": 72000}, "octree-2dgs": {"Na": 87000}, "octree-pgsr": {"Na": 74000}, "pgsr": {"P": 300000}}   # BASELINE: ~300k Gaussians rendered


def build(name, dev, static=False, **size):
    """-> (step, st): one training iteration of method `name` at its BASELINE size (override: Na= / P=) and st with `optimizers`, `P`, and, where
    the method has anchors, `Nv` (both read on the first call) and `rows`.  static=True: the HIP-graph-recordable form (pgsr's shapes are always static)."""
    size = {**SIZES[name], **size}
    if name == "pgsr":
        return pgsr(dev, **size)
    if name == "octree-pgsr":
        return octree_pgsr(dev, static=static, **size)
    return scaffold(dev, lod=name == "octree-2dgs", static=static, **size)


def scene(variant, n, dev, seed=0):
    sc = workloads.make_scene(variant, n, W, H, seed=seed, color_mode="precomp")
    return sc, runner.to_dev(sc, dev)


def second_camera(sc, t, dev):
    """The neighbour camera of the PGSR multi-view losses: 3 degrees of yaw and a small baseline away from the scene's own."""
    cam2 = workloads.make_camera(W, H, W / (2 * sc["tanfovx"]), H / (2 * sc["tanfovy"]), yaw_deg=3.0, t=(-0.15, 0.02, 0.0))
    t2 = dict(t); t2.update({n: torch.tensor(cam2[n], device=dev) for n in ("viewmatrix", "projmatrix", "campos")})
    return t2


def anchor_model(t, Na, dev, g, scaling_log):
    """The synthetic anchor model on the scene's points -> (leaves, rot_anchor, opt, acc).  Draws feat, offset, rot_anchor from `g`, in this order,
    and mlp_o, mlp_c, mlp_k, emb from torch.manual_seed(3); `scaling_log` (Na,6) is the method's own initialiser.  acc = the statistics accumulators
    in training_stats_'s argument order."""
    L = {"anchor": t["means3D"].clone().requires_grad_(True), "scaling_log": scaling_log.requires_grad_(True),
         "feat": torch.randn(Na, 32, generator=g).to(dev).requires_grad_(True),
         "offset": (0.5 * torch.randn(Na, K, 3, generator=g)).to(dev).requires_grad_(True)}
    rot_anchor = torch.nn.functional.normalize(torch.randn(Na, 4, generator=g), dim=1).to(dev)
    mlp = lambda i, o, act: torch.nn.Sequential(torch.nn.Linear(i, 32), torch.nn.ReLU(True), torch.nn.Linear(32, o), act).to(dev)
    torch.manual_seed(3)
    mlp_o, mlp_c, mlp_k = mlp(35, K, torch.nn.Tanh()), mlp(35, 7 * K, torch.nn.Identity()), mlp(35 + A, 3 * K, torch.nn.Sigmoid())
    L.update(emb=torch.nn.Embedding(4, A).to(dev), mlp_o=mlp_o, mlp_c=mlp_c, mlp_k=mlp_k)
    params = [L["anchor"], L["scaling_log"], L["feat"], L["offset"], L["emb"].weight] + [p for m in (mlp_o, mlp_c, mlp_k) for p in m.parameters()]
    acc = {"opacity_accum": torch.zeros(Na, 1, device=dev), "anchor_demon": torch.zeros(Na, 1, device=dev),
           "offset_gradient_accum": torch.zeros(Na * K, 1, device=dev), "offset_denom": torch.zeros(Na * K, 1, device=dev)}
    return L, rot_anchor, Adam(params, lr=1e-4, eps=1e-15), acc


def lod_mask(t, ext, Na, dev, g, dtype):
    """Draws the anchors' octree levels from `g` -> visible(fs, anchor, scaling, rot_anchor): set_anchor_mask + prefilter_voxel of the Octree model in
    one call, no host sync.  dtype: int32 is what the kernels read (an int64 buffer costs a conversion launch per render)."""
    level = torch.randint(0, LEVELS, (Na, 1), generator=g).to(dev).to(dtype)
    extra_level = torch.zeros(Na, device=dev)
    standard_dist = float((t["means3D"] - t["campos"]).norm(dim=1).median()) * FORK ** 3.5   # the median anchor predicts level 3.5: levels 0..3 or 0..4 of 0..5 pass
    voxel_size = float(ext.median()) * 8.0
    return lambda fs, anchor, scaling, rot_anchor: octree.octree_visible(fs, anchor, level, scaling, rot_anchor, voxel_size, FORK, standard_dist, LEVELS,
                                                                         dist2level="round", extra_level=extra_level)["visible_mask"]


def cam_of(t):
    V = t["viewmatrix"].double().cpu().numpy()
    return dict(R=V[:3, :3].copy(), T=V[3, :3].copy(), Fx=W / (2 * float(t["tanfovx"])), Fy=H / (2 * float(t["tanfovy"])), Cx=W / 2.0, Cy=H / 2.0)


def pgsr_targets(t, t2, dev, g):
    """Ground truth and per-pair constants of the PGSR losses; draws gt, gray2, weight from `g`, in this order."""
    T = types.SimpleNamespace(gt=torch.rand((3, H, W), generator=g).to(dev), gray2=torch.rand((1, H, W), generator=g).to(dev), c1=cam_of(t), c2=cam_of(t2))
    T.gray1 = T.gt.mean(0, keepdim=True).contiguous()
    T.K1 = torch.tensor([[T.c1["Fx"], 0, T.c1["Cx"]], [0, T.c1["Fy"], T.c1["Cy"]], [0, 0, 1]], device=dev)
    T.rm1 = torch.inverse(T.K1.double().t()).float()
    T.weight = torch.rand((H, W), generator=g).to(dev)                      # the detached image-gradient weight map (cached per camera)
    cam = lambda c: types.SimpleNamespace(**c, ncc_scale=1.0)              # the attributes multiview_cfg reads of a reference Camera
    T.mcfg = multiview_cfg(cam(T.c1), cam(T.c2), W, H, near_size=(W, H))
    return T


def carriers_for(store, cam, xyz, static, n=2):
    """-> n screen-space gradient carriers for `cam`.  The rasterizer only uses their .grad slot and never reads or writes their values, so persistent
    zero buffers serve every iteration.  Static shapes: the leaves themselves.  Reference shapes (P changes every iteration): fresh leaves that
    VIEW the first P rows of a zero buffer grown on demand (the reference fills two (P,3) tensors per render, pgsr_scene.py:287-288)."""
    P = xyz.shape[0]
    if static:
        if (cam, P) not in store:
            store[cam, P] = tuple(torch.zeros_like(xyz, requires_grad=True) for _ in range(n))
        for m in store[cam, P]:
            m.grad = None
        return store[cam, P]
    if cam not in store or store[cam][0].shape[0] < P:
        store[cam] = tuple(torch.zeros(int(P * 1.25) + 1024, 3, device=xyz.device) for _ in range(n))
    return tuple(b[:P].detach().requires_grad_(True) for b in store[cam])


def backward_unit(roots, st):
    """The total loss is the SUM of `roots`; its backward sends 1 to each: roots with unit gradients are the same backward pass without the scalar
    add launches (and their autograd nodes) of `(a + b + ...).backward()`."""
    if "ones" not in st:
        st["ones"] = [torch.ones_like(r) for r in roots]
    torch.autograd.backward(roots, st["ones"])


def scaffold_setup(dev, Na, lod=False, seed=0):
    """Scene, anchor model, targets and prefilter of the scaffold-2dgs / octree-2dgs iteration (draws gt, gtn and only then the levels)."""
    sc, t = scene("surfel", Na, dev, seed)
    S = types.SimpleNamespace(t=t, rs=runner.settings("surfel", t), campos=t["campos"], wvt=t["viewmatrix"], fpt=t["projmatrix"])
    fs = sf.GaussianRasterizationSettings(**S.rs._asdict())
    g = torch.Generator(device="cpu").manual_seed(7)
    s2 = t["scales"]                                         # (Na,2) world-space sigma of the synthetic scene
    ext = s2.mean(dim=1, keepdim=True)
    S.L, S.rot_anchor, S.opt, S.acc = anchor_model(t, Na, dev, g, torch.log(torch.cat([3.0 * ext.expand(-1, 3), 2.0 * s2, 2.0 * s2[:, :1]], dim=1)))
    S.gt = torch.rand((3, H, W), generator=g).to(dev)
    N = float(W * H)
    gtn = torch.nn.functional.normalize(torch.randn((3, H, W), generator=g), dim=0)
    wmap = torch.zeros((11, H, W))
    wmap[0] = 0.01 / N; wmap[1] = 0.01 / N; wmap[2:5] = -0.05 * gtn / N; wmap[5] = 0.01 / N; wmap[6] = 100.0 / N
    S.wmap = wmap.to(dev)
    S.rm, S.nr = camera_ray_matrices(S.wvt, S.fpt, W, H)
    if lod:
        mask = lod_mask(t, ext, Na, dev, g, torch.int64)      # int64 as drawn: this iteration pays the conversion launch octree-pgsr avoids
        S.visible = lambda scaling: mask(fs, S.L["anchor"], scaling, S.rot_anchor)
    else:                                                     # prefilter_voxel (scaffold_scene.py:122-155)
        S.visible = lambda scaling: sf.GaussianRasterizer(fs).visible_filter(means3D=S.L["anchor"], scales=scaling[:, :3], rotations=S.rot_anchor, cov3D_precomp=None) > 0
    return S


def scaffold(dev, Na, lod=False, static=False, loss="full-hip", stop_after=None, seed=0):
    """loss: "full-hip" = the reference's L1+SSIM + normal / distortion regularisers + scaling loss; "bench" = L1 + linear aux (bench.py's loss),
    no statistics.  stop_after (tools/debug_graph.py): return the intermediates of a prefix of the iteration."""
    S = scaffold_setup(dev, Na, lod, seed)
    L, opt, stop, params = S.L, S.opt, stop_after, S.opt.param_groups[0]["params"]
    anchor, scaling_log, feat, offset, emb, mlp_o, mlp_c, mlp_k = (L[n] for n in ("anchor", "scaling_log", "feat", "offset", "emb", "mlp_o", "mlp_c", "mlp_k"))
    st, carriers = {"optimizers": [opt]}, {}

    def stopped(out):
        opt.zero_grad(set_to_none=True)
        return out

    def step():
        scaling = torch.exp(scaling_log)
        with torch.no_grad():
            vmask = S.visible(scaling)
        app = emb.weight[1]
        vis_idx = decode.compact_visible(vmask, padded=True)   # once per iteration, shared by the decode and the statistics; no host sync
        if stop == "prefilter":
            return [vmask.clone(), vis_idx.clone()]
        out = decode.neural_gaussians(anchor, feat, offset, scaling, mlp_o, mlp_c, mlp_k, S.campos, vis_idx=vis_idx, appearance=app,
                                      static_rows=static, deferred=not static)
        xyz, color, opacity, scl, rot, nop, mask, count = out if static else (*out.finish(), None)
        if stop == "decode":
            return [xyz.clone(), opacity.clone(), scl.clone(), rot.clone(), color.clone()] + ([count.clone()] if static else [])
        means2D = carriers_for(carriers, 0, xyz, True, n=1)[0] if static else torch.zeros_like(xyz, requires_grad=True)
        img, rad, allmap = dsr.GaussianRasterizer(S.rs)(means3D=xyz, means2D=means2D, opacities=opacity, colors_precomp=color,
                                                        scales=scl[:, :2].contiguous(), rotations=rot)
        if stop == "raster":
            return [img.clone(), rad.clone(), allmap.clone()]
        # scaling_loss (scaffold_2dgs_scene.py:25: lambda_scaling * scaling.prod(dim=1).mean(), two columns for 2DGS), value and gradient in one kernel
        reg = scaling_prod_mean(scl, 0.01, cols=2, count=count, unit_upstream=True)
        if loss == "bench":
            total = l1_plus_linear(img, S.gt, allmap, S.wmap) + reg
        else:
            total = l1_ssim(img, S.gt, 0.2, unit_upstream=True) + surfel_geo_loss(allmap, S.rm, S.nr, 0.0, 0.05, 100.0, unit_upstream=True)[0] + reg
        if stop == "loss":
            return [total.detach().clone()]
        total.backward()
        if stop == "backward":
            return stopped([p.grad.clone() for p in params if p.grad is not None] + [means2D.grad.clone()])
        if loss != "bench":                                    # densify(): training_statis every iteration (scaffold_gaussian.py:707-712)
            decode.training_stats_(*S.acc.values(), means2D.grad, nop, rad > 0, mask, vis_idx=vis_idx)
        if stop == "stats":
            return stopped([S.acc["opacity_accum"].clone()])
        opt.step()
        if stop == "step":
            return stopped([p.detach().clone() for p in params])
        opt.zero_grad(set_to_none=True)
        if "Nv" not in st:                       # once (first eager call): host reads for the report
            st["Nv"] = int(vmask.sum())
            st["P"] = int(count[0]) if static else xyz.shape[0]
        st["rows"] = xyz.shape[0]
        return total

    return step, st


def octree_pgsr(dev, Na, static=False, seed=0):
    sc, t = scene("plane", Na, dev, seed)
    t2 = second_camera(sc, t, dev)
    views = [(tt, runner.settings("plane", tt), sf.GaussianRasterizationSettings(**runner.settings("ewa", tt)._asdict())) for tt in (t, t2)]
    g = torch.Generator(device="cpu").manual_seed(7)
    s3 = t["scales"]                                          # (Na,3) world-space sigma of the synthetic scene (one axis flat)
    ext = s3.max(dim=1, keepdim=True)[0]
    first, rot_anchor, opt, acc = anchor_model(t, Na, dev, g, torch.log(torch.cat([3.0 * ext.expand(-1, 3), 2.0 * s3], dim=1)))
    visible = lod_mask(t, ext, Na, dev, g, torch.int32)
    second = shadow_parameters(first)
    opt.add_shadows(first, second)
    T = pgsr_targets(t, t2, dev, g)
    st, carriers = {"optimizers": [opt]}, {}

    def render_begin(cam, L):
        """LOD mask + prefilter + decode of camera `cam`, enqueued (eager: deferred, the count is read in render_finish)."""
        tt, rs, fs = views[cam]
        scaling = torch.exp(L["scaling_log"])
        vmask = visible(fs, L["anchor"], scaling, rot_anchor)
        vis_idx = decode.compact_visible(vmask, padded=True)
        out = decode.neural_gaussians(L["anchor"], L["feat"], L["offset"], scaling, L["mlp_o"], L["mlp_c"], L["mlp_k"], tt["campos"], vis_idx=vis_idx,
                                      appearance=L["emb"].weight[cam + 1], static_rows=static, deferred=not static)
        return cam, vmask, vis_idx, out

    def render_finish(begun):
        cam, vmask, vis_idx, out = begun
        tt, rs, fs = views[cam]
        xyz, color, opacity, scl, rot, nop, mask, count = out if static else (*out.finish(), None)
        am = plane_input_all_map(xyz, rot, scl, tt["viewmatrix"], tt["campos"])
        m2, m2a = carriers_for(carriers, cam, xyz, static)
        img, radii, obs, oam, pd = dpr.GaussianRasterizer(rs)(means3D=xyz, means2D=m2, means2D_abs=m2a, opacities=opacity, colors_precomp=color,
                                                             scales=scl, rotations=rot, all_map=am)
        return img, radii, oam, pd, scl, m2, nop, mask, vis_idx, vmask, count

    def step():
        b1, b2 = render_begin(0, first), render_begin(1, second)       # both decodes in flight before the first count is read
        img, radii, oam, pd, scl, m2, nop, mask, vis_idx, vmask, count = render_finish(b1)
        pd2 = render_finish(b2)[3]
        reg = scaling_prod_mean(scl, 0.01, count=count, unit_upstream=True)      # scaling_loss (octree_pgsr_scene.py:23), value and gradient in one kernel
        nrm, geo, ncc = plane_losses(pd, pd2, oam, T.gray1, T.gray2, T.mcfg, T.rm1, T.weight, 0.015, 0.03, 0.15)      # one node: gradients to pd / oam leave it summed
        backward_unit([l1_ssim(img, T.gt, 0.2, unit_upstream=True), nrm, reg, geo, ncc], st)
        decode.training_stats_(*acc.values(), m2.grad, nop, radii > 0, mask, vis_idx=vis_idx)
        opt.step(); opt.zero_grad(set_to_none=True)
        if "P" not in st:
            st["P"] = int(mask.sum()); st["Nv"] = int(vmask.sum())

    return step, st


def pgsr_setup(dev, P):
    """Scene, two cameras, the explicit model's raw leaves [xyz, scl_log, rot_raw, op_raw, col], their optimizer and the targets."""
    sc, t = scene("plane", P, dev)
    S = types.SimpleNamespace(views=[(tt, runner.settings("plane", tt)) for tt in (t, second_camera(sc, t, dev))])
    g = torch.Generator(device="cpu").manual_seed(7)
    S.first = [x.requires_grad_(True) for x in (t["means3D"].clone(), torch.log(t["scales"]), t["rotations"].clone(),
                                                torch.logit(t["opacities"].clamp(1e-4, 1 - 1e-4)), t["colors_precomp"].clone())]
    S.opt = Adam(S.first, lr=1e-4, eps=1e-15)
    S.T = pgsr_targets(t, S.views[1][0], dev, g)
    return S


def pgsr(dev, P):
    S = pgsr_setup(dev, P)
    first, opt, T = S.first, S.opt, S.T
    second = shadow_parameters(first)                     # the neighbour's pass also runs its own activation kernel
    opt.add_shadows(first, second)
    st, carriers = {"P": P, "optimizers": [opt]}, {}

    def render(cam, L):
        tt, rs = S.views[cam]
        means, scl_log, rot_raw, op_raw, col = L
        scl, rot, op = gaussian_activations(scl_log, rot_raw, op_raw)     # get_scaling / get_rotation / get_opacity (vanilla_gaussian.py:250-269) as one kernel each way
        am = plane_input_all_map(means, rot, scl, tt["viewmatrix"], tt["campos"])
        m2, m2a = carriers_for(carriers, cam, means, True)
        return dpr.GaussianRasterizer(rs)(means3D=means, means2D=m2, means2D_abs=m2a, opacities=op, colors_precomp=col, scales=scl, rotations=rot, all_map=am)

    def step():
        img, radii, obs, oam, pd = render(0, first)
        pd2 = render(1, second)[4]
        nrm, geo, ncc = plane_losses(pd, pd2, oam, T.gray1, T.gray2, T.mcfg, T.rm1, T.weight, 0.015, 0.03, 0.15)      # one node: gradients to pd / oam leave it summed
        backward_unit([l1_ssim(img, T.gt, 0.2, unit_upstream=True), nrm, geo, ncc], st)
        opt.step(); opt.zero_grad(set_to_none=True)

    return step, st
