"""The unbounded mesh path on the device: gsrast.unbounded.extract_mesh_unbounded, stage by stage, and its frame-fused lattice pass against the only
way the parent commit could run that pass.

    python tools/bench_unbounded.py [--resolution 1024 --crop 512 --frames 100 --width 1920 --height 1080] [--out profiles/unbounded_mesh.json]

Workload: a seeded smooth scene -- a wavy height field z = 2.6 + 0.3 sin(1.5 x) cos(1.2 y) seen by cameras near the origin (yaw within +-25 degrees,
small translations), its depth maps ray-cast analytically, colours a smooth function of the hit point -- and Gaussians sampled on the surface for the
contraction bound.  resolution 1024 with crop 512 is a 1023^3 lattice.
Measured: HIP-event time of the whole call and of its stages (the call's own slab loop re-run with events around every piece: lattice, cubes, finish,
texture), kernel launches (torch profiler) and host synchronisations (torch's sync debug mode) of one whole call, peak memory (caching allocator),
algorithmic bytes from the shapes.  The comparison: the lattice pass of every slab, fused, against the chain `lattice_points` of a 256^3-point chunk
(the reference's chunk: points and per-point truncation in memory) followed by one `tsdf_integrate_` per frame per chunk, in the same process,
alternating, --reps times; both produce the whole lattice.  The fused pass must be the faster one: anything else fails the run.  Prints and writes JSON."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from gsrast import unbounded as ub      # noqa: E402
from gsrast.tsdf import tsdf_integrate_  # noqa: E402
from gsrast.workloads import make_camera  # noqa: E402

CENTER, RADIUS = (0.0, 0.0, 2.6), 1.7


def height(x, y):
    return 2.6 + 0.3 * torch.sin(1.5 * x) * torch.cos(1.2 * y)


def make_frames(F, W, H, dev, seed=0):
    """-> (full_proj [F,4,4], depth [F,1,H,W], rgb [F,3,H,W]) on the device."""
    rng = np.random.default_rng(seed)
    P, D, Cc = [], [], []
    u = (torch.arange(W, device=dev, dtype=torch.float32) * (2.0 / (W - 1)) - 1.0)[None, :].expand(H, W)
    v = (torch.arange(H, device=dev, dtype=torch.float32) * (2.0 / (H - 1)) - 1.0)[:, None].expand(H, W)
    for i in range(F):
        cam = make_camera(W, H, 0.9 * W, 0.9 * W, yaw_deg=float(rng.uniform(-25, 25)), t=tuple(rng.uniform(-0.4, 0.4, 3) * np.array([1.0, 0.5, 0.5])))
        wvt = torch.tensor(cam["viewmatrix"], device=dev, dtype=torch.float32)
        Rinv, tw = torch.linalg.inv(wvt[:3, :3]), wvt[3, :3]
        ray = torch.stack([u * cam["tanfovx"], v * cam["tanfovy"], torch.ones_like(u)], -1)      # camera space, z = 1: the ray parameter is the depth
        rw = ray @ Rinv
        ow = -tw @ Rinv
        s = torch.full((H, W), 2.6, device=dev)
        for _ in range(12):                                                                      # fixed-point ray cast of the gentle height field
            p = ow + s[..., None] * rw
            s = s + (height(p[..., 0], p[..., 1]) - p[..., 2]) / rw[..., 2]
        p = ow + s[..., None] * rw
        P.append(torch.tensor(cam["projmatrix"], device=dev)); D.append(s[None].contiguous())
        Cc.append(torch.stack([0.5 + 0.5 * torch.sin(2 * p[..., 0]), 0.5 + 0.5 * torch.cos(3 * p[..., 1]), 0.5 + 0.5 * torch.sin(p[..., 0] + p[..., 1])]))
    return torch.stack(P), torch.stack(D), torch.stack(Cc)


def make_xyz(n, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xy = (torch.rand((n, 2), generator=g) * 2 - 1) * 4.0
    return torch.cat([xy, height(xy[:, 0], xy[:, 1])[:, None]], 1).to(dev)


def warm_clocks(dev, seconds=1.0):
    a = torch.randn(4096, 4096, device=dev)
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    spent = 0.0
    while spent < seconds * 1e3:
        t0.record()
        for _ in range(10):
            a = torch.nn.functional.normalize(a @ a)
        t1.record(); t1.synchronize()
        spent += t0.elapsed_time(t1)


class Stages:
    """HIP events around the pieces of a call; ms per label after read()."""
    def __init__(self):
        self.ev = []

    def run(self, label, fn):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        self.ev.append((label, a, b))
        return out

    def read(self):
        torch.cuda.synchronize()
        ms = {}
        for label, a, b in self.ev:
            ms[label] = ms.get(label, 0.0) + a.elapsed_time(b)
        return ms


def staged_extract(P, D, Cc, xyz, res, crop, slab):
    """extract_mesh_unbounded through its own stage hook, with events around every piece."""
    st = Stages()
    mesh = ub.extract_mesh_unbounded(P, D, Cc, xyz, CENTER, RADIUS, resolution=res, crop=crop, slab=slab, stage=st.run)
    return st.read(), mesh


def fused_lattice(P, D, axes, vox, slab, keep=None):
    """The lattice pass of every slab of the plan extract_mesh_unbounded follows; keep: a [nx,ny,nz] tensor that receives the owned planes."""
    xs, ys, zs = axes
    for x0, own, np_ in ub.slab_plan(xs.numel(), slab):
        f = ub.lattice_tsdf(xs[x0:x0 + np_].contiguous(), ys, zs, CENTER, RADIUS, vox, P, D, device=P.device)
        if keep is not None:
            keep[x0:x0 + own] = f[:own]


def chain_lattice(P, D, Cc, axes, vox, keep=None):
    """The parent commit's way: per chunk of about 256^3 points, points and truncations in memory, then the per-frame op once per frame."""
    xs, ys, zs = axes
    planes = max(2, (256 ** 3) // (ys.numel() * zs.numel()))
    bounds = list(range(0, xs.numel(), planes)) + [xs.numel()]
    if len(bounds) > 2 and bounds[-1] - bounds[-2] < 2:      # the op wants two planes: a single last one rides with its neighbour
        del bounds[-2]
    for x0, x1 in zip(bounds[:-1], bounds[1:]):
        pts, tr = ub.lattice_points(xs[x0:x1].contiguous(), ys, zs, CENTER, RADIUS, vox, device=P.device)
        n = int(pts.shape[0])
        t = torch.ones(n, device=P.device); w = torch.ones(n, device=P.device); c = torch.zeros((n, 3), device=P.device)
        for f in range(int(P.shape[0])):
            tsdf_integrate_(pts, P[f], D[f], Cc[f], tr, t, c, w)
        if keep is not None:
            keep[x0:x1] = t.reshape(x1 - x0, ys.numel(), zs.numel())


def ms_of(fn):
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def profile_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n, per = 0, {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            n += 1
            try:
                us = e.time_range.elapsed_us()
            except Exception:
                us = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)
            k = e.name.split("(")[0]
            per[k] = per.get(k, 0.0) + float(us)
    return n, per


def count_syncs(fn):
    """-> (host synchronisations torch's sync debug mode sees, calls of the library's count entry point: each reads its two totals, once)."""
    L = ub.lib()
    real, calls = L.gsr_unbounded_mc_count, [0]

    def counted(*args):
        calls[0] += 1
        return real(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    L.gsr_unbounded_mc_count = counted
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        L.gsr_unbounded_mc_count = real
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower()), calls[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--slab", type=int, default=ub.DEFAULT_SLAB)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="also compare the fused lattice with the chain's, bit for bit (holds both in memory)")
    ap.add_argument("--report-only", action="store_true", help="record the ratio without failing the run on it (sizes too small to fill the device)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unbounded_mesh.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unbounded.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    P, D, Cc = make_frames(a.frames, a.width, a.height, dev)
    xyz = make_xyz(200000, dev)
    vox = np.float32(RADIUS * 2 / a.resolution)
    R = ub.contraction_bound(xyz, CENTER, RADIUS)
    axes = [torch.from_numpy(x).to(dev) for x in ub.lattice_axes((-R,) * 3, (R,) * 3, a.resolution, a.crop)]
    n = axes[0].numel()
    S = n ** 3
    res = {"device": torch.cuda.get_device_name(0), "resolution": a.resolution, "crop": a.crop, "lattice": [n, n, n], "samples": S, "frames": a.frames,
           "frame_size": [a.width, a.height], "slab": a.slab, "contraction_bound": R, "timing": "HIP events, ms"}
    warm_clocks(dev)
    call = lambda: ub.extract_mesh_unbounded(P, D, Cc, xyz, CENTER, RADIUS, resolution=a.resolution, crop=a.crop, slab=a.slab)
    mesh = call()                                                       # warms every shape
    V, T = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    res["vertices"], res["triangles"] = V, T
    whole, stages = [], []
    for _ in range(a.reps):
        whole.append(ms_of(call))
        ms, again = staged_extract(P, D, Cc, xyz, a.resolution, a.crop, a.slab)
        stages.append(ms)
    assert torch.equal(again.vertices, mesh.vertices) and torch.equal(again.triangles, mesh.triangles) and torch.equal(again.vertex_colors, mesh.vertex_colors)
    res["extract_ms"] = [round(x, 2) for x in whole]
    res["stage_ms"] = {k: [round(s[k], 2) for s in stages] for k in stages[0]}
    try:
        res["kernel_launches"], per = profile_launches(call)
        res["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])[:12]}
    except Exception as e:                                              # the profiler is optional equipment
        res["kernel_launches"] = f"not measured ({type(e).__name__})"
    plan = ub.slab_plan(n, a.slab)
    res["slabs"] = len(plan)
    seen, counted = count_syncs(call)
    # torch's debug mode sees torch's own host reads (the contraction bound's); the library's reads are counted at its entry point: one per count call
    res["host_synchronisations"] = {"seen_by_torch": seen, "library_count_calls": counted, "total": seen + counted}
    del mesh, again
    torch.cuda.empty_cache(); torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    res["bytes_inputs"], res["bytes_peak"] = int(before), int(torch.cuda.max_memory_allocated())
    # algorithmic bytes, from the shapes
    planes = sum(np_ for _, _, np_ in plan)
    res["algorithmic_bytes"] = {
        "lattice_fused": {"written": 4 * planes * n * n, "per_sample": 4, "note": "slabs re-evaluate the two planes they share with the next one"},
        "lattice_chain": {"points_and_truncations_written": 16 * S, "read_per_frame": 12 * S * a.frames,
                          "read_modify_written_per_touched_sample_per_frame": 40, "note": "12 B read per sample per frame + up to 40 B per touched sample"},
        "cubes": {"read": 4 * planes * n * n, "scratch_per_numbered_point": 4, "vertices_written": 12 * V, "triangles_written": 12 * T},
        "finish": {"read_and_written": 24 * V}, "texture": {"read": 12 * V, "written": 12 * V}}
    # fused lattice pass against the chain: same process, alternating
    fused, chain = [], []
    fused_lattice(P, D, axes, vox, a.slab); chain_lattice(P[:1], D[:1], Cc[:1], axes, vox)      # shapes warmed
    for _ in range(a.reps):
        fused.append(ms_of(lambda: fused_lattice(P, D, axes, vox, a.slab)))
        chain.append(ms_of(lambda: chain_lattice(P, D, Cc, axes, vox)))
    ratios = [c / f for c, f in zip(chain, fused)]
    res["lattice_fused_ms"] = [round(x, 2) for x in fused]
    res["lattice_chain_ms"] = [round(x, 2) for x in chain]
    res["chain_over_fused"] = {"per_rep": [round(x, 2) for x in ratios], "median": round(float(np.median(ratios)), 2),
                               "min": round(min(ratios), 2), "max": round(max(ratios), 2)}
    if a.check:
        kf = torch.empty((n, n, n), device=dev); kc = torch.empty((n, n, n), device=dev)
        fused_lattice(P, D, axes, vox, a.slab, keep=kf); chain_lattice(P, D, Cc, axes, vox, keep=kc)
        res["fused_equals_chain"] = bool(torch.equal(kf, kc))
    res["fused_is_faster"] = bool(max(fused) < min(chain))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if (not res["fused_is_faster"] and not a.report_only) or res.get("fused_equals_chain") is False:
        raise SystemExit("bench_unbounded.py: the fused lattice pass must beat the per-frame chain and equal it")


if __name__ == "__main__":
    main()
