"""One ScaffoldGaussian.adjust_anchor call on the device: gsrast.anchors.adjust_anchor_ against the reference-shaped torch chain, same device, same inputs.

    python tools/bench_anchor.py [--sizes 100000 300000 1000000] [--out profiles/anchor_adjust.json]

The torch chain below is this repository's restatement of the literal algorithm of gssr/gaussian/scaffold_gaussian.py:555-705 -- per level: candidate mask,
torch.unique(dim=0), the all-pairs occupancy test in chunks of 4096 anchors, the feature maximum (torch_scatter is absent: Tensor.scatter_reduce "amax" stands
in for scatter_max), one cat per tensor; then boolean-index pruning of every parameter, moment and accumulator.  Inputs are the statistics of a synthetic
surface scene (anchors on a voxel lattice over a height field, k = 10 offsets, 32 features).  Times are HIP-event times of one whole call (host
synchronisations included: they are part of the call), clocks warmed, each path warmed once on the same shape; launches are counted by the torch profiler,
host synchronisations by torch's sync debug mode, each in a run of its own.  Prints and writes JSON."""
import argparse
import json
import math
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from gsrast import anchors   # noqa: E402
from gsrast.optim import Adam   # noqa: E402

NAMES = ("anchor", "offset", "anchor_feat", "opacity", "scaling", "rotation")
ACCS = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")
K, F, VS = 10, 32, 0.01


def scene(N, seed=0):
    r = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(N)))
    ix, iy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    x, y = (ix.reshape(-1)[:N] - side / 2) * VS, (iy.reshape(-1)[:N] - side / 2) * VS
    z = np.round(0.5 * np.sin(x) * np.cos(0.7 * y) / VS) * VS
    p = {"anchor": np.stack([x, y, z], 1).astype(np.float32), "offset": r.uniform(-1, 1, (N, K, 3)).astype(np.float32),
         "anchor_feat": r.normal(0, 1, (N, F)).astype(np.float32), "opacity": r.normal(0, 1, (N, 1)).astype(np.float32),
         "scaling": np.log(r.uniform(2.0, 14.0, (N, 6)) * VS).astype(np.float32), "rotation": r.normal(0, 1, (N, 4)).astype(np.float32)}
    denom = r.integers(0, 100, (N * K, 1)).astype(np.float32)
    a = {"offset_denom": denom, "offset_gradient_accum": (denom * np.exp(r.normal(math.log(2e-4), 1.0, (N * K, 1)))).astype(np.float32),
         "anchor_demon": r.integers(0, 121, (N, 1)).astype(np.float32)}
    a["opacity_accum"] = (a["anchor_demon"] * r.uniform(0.0, 0.05, (N, 1))).astype(np.float32)
    return p, a


class Model:
    pass


def make_model(p, a, dev, opt_cls):
    m = Model()
    for n in NAMES:
        setattr(m, "_" + n, torch.nn.Parameter(torch.tensor(p[n], device=dev)))
    for n in ACCS:
        setattr(m, n, torch.tensor(a[n], device=dev))
    m.optimizer = opt_cls([{"params": [getattr(m, "_" + n)], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        q = getattr(m, "_" + n)
        m.optimizer.state[q] = {"step": torch.tensor(1.0), "exp_avg": torch.full_like(q, 0.01), "exp_avg_sq": torch.full_like(q, 1e-4)}
    m.get_scaling = torch.exp(m._scaling.detach())
    m.n_offsets, m.voxel_size, m.update_depth, m.update_init_factor, m.update_hierachy_factor = K, VS, 3, 16, 4
    m.max_radii2D = torch.zeros(p["anchor"].shape[0], device=dev)
    return m


def _cat_to_optimizer(m, d):
    for g in m.optimizer.param_groups:
        ext = d[g["name"]]
        old = g["params"][0]
        st = m.optimizer.state.pop(old)
        st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
        st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
        new = torch.nn.Parameter(torch.cat((old, ext), dim=0).requires_grad_(True))
        g["params"][0] = new
        m.optimizer.state[new] = st
        setattr(m, "_" + g["name"], new)


def _prune_optimizer(m, keep):
    for g in m.optimizer.param_groups:
        old = g["params"][0]
        st = m.optimizer.state.pop(old)
        st["exp_avg"] = st["exp_avg"][keep]; st["exp_avg_sq"] = st["exp_avg_sq"][keep]
        new = torch.nn.Parameter(old[keep].requires_grad_(True))
        if g["name"] == "scaling":
            t = new[:, 3:]; t[t > 0.05] = 0.05; new[:, 3:] = t
        g["params"][0] = new
        m.optimizer.state[new] = st
        setattr(m, "_" + g["name"], new)


@torch.no_grad()
def torch_adjust(m, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005):
    """The reference-shaped chain (see the module docstring)."""
    dev = m._anchor.device
    k = m.n_offsets
    grads = m.offset_gradient_accum / m.offset_denom
    grads[grads.isnan()] = 0.0
    grads = torch.norm(grads, dim=-1)
    offset_mask = (m.offset_denom > check_interval * success_threshold * 0.5).squeeze(dim=1)
    init_length = m._anchor.shape[0] * k
    for i in range(m.update_depth):
        cand = torch.logical_and(grads >= grad_threshold * ((m.update_hierachy_factor // 2) ** i), offset_mask)
        cand = torch.logical_and(cand, torch.rand_like(cand.float()) > (0.5 ** (i + 1)))
        inc = m._anchor.shape[0] * k - init_length
        if inc == 0:
            if i > 0:
                continue
        else:
            cand = torch.cat([cand, torch.zeros(inc, dtype=torch.bool, device=dev)], dim=0)
        all_xyz = m._anchor.unsqueeze(dim=1) + m._offset * torch.exp(m._scaling)[:, :3].unsqueeze(dim=1)
        cur_size = m.voxel_size * (m.update_init_factor // (m.update_hierachy_factor ** i))
        grid = torch.round(m._anchor / cur_size).int()
        sel = torch.round(all_xyz.view([-1, 3])[cand] / cur_size).int()
        uniq, inverse = torch.unique(sel, return_inverse=True, dim=0)
        dup = torch.zeros(uniq.shape[0], dtype=torch.bool, device=dev)
        for c in range(0, grid.shape[0], 4096):                   # the O(U N) term
            dup |= (uniq.unsqueeze(1) == grid[c:c + 4096, :]).all(-1).any(-1).view(-1)
        new_anchor = uniq[~dup] * cur_size
        if new_anchor.shape[0] > 0:
            U = new_anchor.shape[0]
            feat = m._anchor_feat.unsqueeze(dim=1).repeat([1, k, 1]).view([-1, m._anchor_feat.shape[1]])[cand]
            feat = torch.zeros(uniq.shape[0], feat.shape[1], device=dev).scatter_reduce(0, inverse.unsqueeze(1).expand(-1, feat.size(1)), feat, "amax",
                                                                                         include_self=False)[~dup]
            rot = torch.zeros([U, 4], device=dev); rot[:, 0] = 1.0
            tenth = 0.1 * torch.ones((U, 1), device=dev)
            d = {"anchor": new_anchor, "scaling": torch.log(torch.ones_like(new_anchor).repeat([1, 2]) * cur_size), "rotation": rot, "anchor_feat": feat,
                 "offset": torch.zeros_like(new_anchor).unsqueeze(dim=1).repeat([1, k, 1]), "opacity": torch.log(tenth / (1 - tenth))}
            m.anchor_demon = torch.cat([m.anchor_demon, torch.zeros([U, 1], device=dev)], dim=0)
            m.opacity_accum = torch.cat([m.opacity_accum, torch.zeros([U, 1], device=dev)], dim=0)
            _cat_to_optimizer(m, d)
    Na = m._anchor.shape[0]
    m.offset_denom[offset_mask] = 0
    m.offset_denom = torch.cat([m.offset_denom, torch.zeros([Na * k - m.offset_denom.shape[0], 1], device=dev)], dim=0)
    m.offset_gradient_accum[offset_mask] = 0
    m.offset_gradient_accum = torch.cat([m.offset_gradient_accum, torch.zeros([Na * k - m.offset_gradient_accum.shape[0], 1], device=dev)], dim=0)
    prune = (m.opacity_accum < min_opacity * m.anchor_demon).squeeze(dim=1)
    often = (m.anchor_demon > check_interval * success_threshold).squeeze(dim=1)
    prune = torch.logical_and(prune, often)
    m.offset_denom = m.offset_denom.view([-1, k])[~prune].view([-1, 1])
    m.offset_gradient_accum = m.offset_gradient_accum.view([-1, k])[~prune].view([-1, 1])
    if often.sum() > 0:
        m.opacity_accum[often] = torch.zeros([int(often.sum()), 1], device=dev)
        m.anchor_demon[often] = torch.zeros([int(often.sum()), 1], device=dev)
    m.opacity_accum = m.opacity_accum[~prune]
    m.anchor_demon = m.anchor_demon[~prune]
    _prune_optimizer(m, ~prune)
    m.max_radii2D = torch.zeros(m._anchor.shape[0], device=dev)
    return m._anchor.shape[0]


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


def timed(fn, build, reps):
    ms = []
    for _ in range(reps + 1):                                    # the first repetition is the warm-up of this shape
        m = build()
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); n = fn(m); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms[1:], n


def count_launches(fn, build):
    from torch.profiler import ProfilerActivity, profile
    m = build()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(m)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def count_syncs(fn, build):
    m = build()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(m)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 300000, 1000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--torch-max", type=int, default=1000000, help="largest size the torch chain is run at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_adjust.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anchor.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "k": K, "feat_dim": F, "voxel_size": VS, "timing": "HIP events around one whole call, ms", "sizes": []}
    warm_clocks(dev)
    for N in a.sizes:
        p, acc = scene(N)
        row = {"Na": N}
        for tag, fn, cls, reps in (("hip", lambda m: anchors.adjust_anchor_(m), Adam, a.reps), ("torch_chain", torch_adjust, torch.optim.Adam, a.torch_reps)):
            if tag == "torch_chain" and N > a.torch_max:
                row[tag] = "not measured"
                continue
            build = lambda: make_model(p, acc, dev, cls)
            torch.manual_seed(0)
            ms, n_out = timed(fn, build, reps)
            ent = {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "anchors_after": int(n_out)}
            try:
                ent["kernel_launches"] = count_launches(fn, build)
            except Exception as e:                                # the profiler is optional equipment
                ent["kernel_launches"] = f"not measured ({type(e).__name__})"
            try:
                ent["host_synchronisations"] = count_syncs(fn, build)
            except Exception as e:
                ent["host_synchronisations"] = f"not measured ({type(e).__name__})"
            row[tag] = ent
            print(json.dumps({"Na": N, tag: ent}), flush=True)
        if isinstance(row.get("torch_chain"), dict):
            row["speedup"] = round(row["torch_chain"]["ms_median"] / row["hip"]["ms_median"], 1)
        res["sizes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
