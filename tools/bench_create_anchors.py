"""Measures the first anchors on the device against the reference-shaped torch chain on the same device -> profiles/create_anchors.json.

    python tools/bench_create_anchors.py [--points 1000000 5000000] [--cameras 300 3000] [--scales 1 2] [--reps 2] [--chain-cameras 32]

Per (N points, C cameras per scale, S resolution scales): one gsrast.init.set_level alone and one gsrast.anchors.octree_create_from_data_, and the
torch chain the reference runs for set_level (per camera: distance of all points, torch.quantile twice, two torch.cat; its steps live here).  The
chain costs two sorts of N values per camera, so it is timed on the first --chain-cameras cameras only and scaled to all of them (recorded as
measured / extrapolated; its cost per camera does not depend on the camera).  Recorded: wall time (HIP events around the whole call, host reads
included), kernel time and launches from the profiler, host synchronisations from torch's sync debug mode, peak memory from the caching allocator,
and the select kernels' rate in point-camera pairs per second per pass.  Each kind of measurement is a run of its own.  No ratio is asserted."""
import argparse
import json
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
from gsrast import anchors, init  # noqa: E402


def scene(N, C, S, dev, seed=0):
    """A wavy surface in [-3, 3]^2 and cameras at log-spread distances around it."""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    p = torch.rand(N, 2, device=dev, generator=g) * 6.0 - 3.0
    z = 0.4 * torch.sin(1.7 * p[:, 0]) * torch.cos(1.3 * p[:, 1]) + 0.02 * torch.randn(N, device=dev, generator=g)
    pts = torch.cat([p, z[:, None]], 1).contiguous()
    cams = {}
    for s in range(S):
        d = torch.exp(torch.rand(C, device=dev, generator=g) * math.log(12.0 / 0.8) + math.log(0.8))
        v = torch.randn(C, 3, device=dev, generator=g); v[:, 2] = v[:, 2].abs() + 0.3
        cams[float(2 ** s)] = (v / v.norm(dim=1, keepdim=True) * d[:, None]).contiguous()
    return pts, cams


def torch_set_level_chain(points, cameras, dist_ratio, limit):
    """The reference's set_level loop (octree_gaussian.py:152-172) over the first `limit` cameras; -> cameras visited."""
    all_dist = torch.tensor([], device=points.device)
    cam_infos = torch.empty(0, 4, device=points.device)
    n = 0
    for scale, centres in cameras.items():
        for cam_center in centres:
            if n == limit:
                return n
            cam_info = torch.tensor([cam_center[0], cam_center[1], cam_center[2], scale]).float().to(points.device)
            cam_infos = torch.cat((cam_infos, cam_info.unsqueeze(dim=0)), dim=0)
            dist = torch.sqrt(torch.sum((points - cam_center) ** 2, dim=1))
            dist_max = torch.quantile(dist, dist_ratio)
            dist_min = torch.quantile(dist, 1 - dist_ratio)
            new_dist = torch.tensor([dist_min, dist_max]).float().to(points.device) * scale
            all_dist = torch.cat((all_dist, new_dist), dim=0)
            n += 1
    return n


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):                                    # the first repetition warms the shape up
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); out = fn(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms[1:], out


def profile_kernels(fn):
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
            per[e.name] = per.get(e.name, 0.0) + float(us)
    return n, per


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower())


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return before, torch.cuda.max_memory_allocated()


def measure(fn, reps, kernels=None):
    ms, _ = timed(fn, reps)
    ent = {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3)}
    try:
        ent["kernel_launches"], per = profile_kernels(fn)
        ent["kernel_ms"] = round(sum(per.values()) / 1e3, 3)
        if kernels:
            ent["kernel_us"] = {k.split("(")[0][:60]: round(v, 1) for k, v in per.items() if any(s in k for s in kernels)}
    except Exception as e:                                        # the profiler is optional equipment
        ent["kernel_launches"] = f"not measured ({type(e).__name__})"
    try:
        ent["host_synchronisations"] = count_syncs(fn)
    except Exception as e:
        ent["host_synchronisations"] = f"not measured ({type(e).__name__})"
    before, peak = peak_memory(fn)
    ent["bytes_inputs"], ent["bytes_peak_above_inputs"] = before, peak - before
    return ent


def model(dev):
    return types.SimpleNamespace(config=types.SimpleNamespace(sampling_ratio=1), device=dev, dist_ratio=0.999, levels=-1, init_level=-1, fork=2, extend=1.1,
                                 base_layer=-1, visible_threshold=-1, dist2level="round", n_offsets=10, feat_dim=32,
                                 inverse_opacity_activation=lambda x: torch.log(x / (1 - x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 5000000])
    ap.add_argument("--cameras", type=int, nargs="+", default=[300, 3000])
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chain-cameras", type=int, default=32)
    ap.add_argument("--no-create", action="store_true", help="set_level only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "create_anchors.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_create_anchors.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "timing": "HIP events around one whole call, ms", "dist_ratio": 0.999, "rows": []}
    for N in a.points:
        for S in a.scales:
            for C in a.cameras:
                pts, cams = scene(N, C, S, dev, seed=N % 997 + C + S)
                row = {"N": N, "cameras_per_scale": C, "scales": S, "cameras": C * S}
                ent = measure(lambda: init.set_level(pts, cams, 0.999, 2), a.reps, kernels=("k_cq_", "k_sel_"))
                pairs = float(N) * C * S
                for k, us in ent.get("kernel_us", {}).items():
                    if "k_cq_hist" in k and us > 0:
                        passes = 1 if ("<true>" in k or "Lb1" in k) else 3
                        ent.setdefault("pairs_per_s_per_pass", {})["first_pass" if passes == 1 else "later_passes"] = round(pairs * passes / (us * 1e-6), 0)
                ent["bytes_scratch"] = int(init.lib().gsr_cam_dist_quantiles_scratch_bytes(N, C * S))
                row["set_level_hip"] = ent
                lim = min(a.chain_cameras, C * S)
                ms, _ = timed(lambda: torch_set_level_chain(pts, cams, 0.999, lim), 1)
                chain = {"cameras_measured": lim, "ms_measured": round(ms[0], 3), "ms_per_camera": round(ms[0] / lim, 4),
                         "ms_all_cameras_extrapolated": round(ms[0] / lim * C * S, 1),
                         "host_synchronisations_measured": count_syncs(lambda: torch_set_level_chain(pts, cams, 0.999, lim))}
                before, peak = peak_memory(lambda: torch_set_level_chain(pts, cams, 0.999, min(lim, 2)))
                chain["bytes_peak_above_inputs"] = peak - before
                row["set_level_torch_chain"] = chain
                print(json.dumps(row), flush=True)
                if not a.no_create:
                    pcd = types.SimpleNamespace(points=pts)
                    ms, U = timed(lambda: anchors.octree_create_from_data_(model(dev), pcd, cams, 1.0), 1)
                    m = model(dev)
                    ent = {"ms": round(ms[0], 3), "anchors": int(U)}
                    try:
                        ent["kernel_launches"], per = profile_kernels(lambda: anchors.octree_create_from_data_(m, pcd, cams, 1.0))
                        ent["kernel_ms"] = round(sum(per.values()) / 1e3, 3)
                        top = sorted(per.items(), key=lambda kv: -kv[1])[:8]
                        ent["kernel_us_top"] = {k.split("(")[0][:60]: round(v, 1) for k, v in top}
                    except Exception as e:
                        ent["kernel_launches"] = f"not measured ({type(e).__name__})"
                    ent["levels"], ent["host_synchronisations"] = int(m.levels), count_syncs(lambda: anchors.octree_create_from_data_(model(dev), pcd, cams, 1.0))
                    before, peak = peak_memory(lambda: anchors.octree_create_from_data_(model(dev), pcd, cams, 1.0))
                    ent["bytes_inputs"], ent["bytes_peak_above_inputs"] = before, peak - before
                    row["octree_create_from_data_hip"] = ent
                    print(json.dumps({"N": N, "cameras": C * S, "octree_create_from_data_hip": ent}), flush=True)
                res["rows"].append(row)
                del pts, cams
                torch.cuda.empty_cache()
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as f:                          # after every row: a long grid leaves what it has measured
                    json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
