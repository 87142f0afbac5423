"""Measures the surface-distance evaluation on the device against a KD-tree on the host -> profiles/chamfer.json.

    python tools/bench_chamfer.py [--points 1000000 10000000] [--max-dist 0.02] [--reps 2] [--no-host]

The scene: two independently jittered samplings (prediction, ground truth) of one synthetic sheet z = 0.05 sin(3x) cos(2y) over [0,10]^2, the
prediction with 0.1 % floaters spread over [0,10]^2 x [-1,1].  Per size N x N and per cap (none, --max-dist): one gsrast.chamfer.surface_distance
call on the two clouds (both directions, 2 N queries, four thresholds).  Recorded: wall time (HIP events around the whole call, host reads
included), kernel time and launches from the profiler, host synchronisations from torch's sync debug mode, peak memory above the inputs from the
caching allocator, queries per second, and the ratio of the 10 M to the 1 M time -- per query that ratio over 10 is what says whether the work per
query grows with the number of targets.  Each kind of measurement is a run of its own.  No ratio is asserted.
Baseline: scipy.spatial.cKDTree (float64, all usable cores) where scipy imports, both directions measured in full; otherwise a chunked numpy
all-pairs search timed on a sample of queries and scaled to the size, labelled as an extrapolation."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
from gsrast import chamfer  # noqa: E402

TAUS = (0.002, 0.005, 0.01, 0.05)


def sheet(N, seed, floaters):
    r = np.random.default_rng(seed)
    side = int(np.sqrt(N))
    n = side * side
    i = np.arange(n)
    x = ((i % side) + r.random(n)) * (10.0 / side)
    y = ((i // side) + r.random(n)) * (10.0 / side)
    p = np.stack([x, y, 0.05 * np.sin(3 * x) * np.cos(2 * y)], axis=1)
    k = int(n * floaters)
    if k:
        p[r.choice(n, k, replace=False)] = r.uniform([0, 0, -1], [10, 10, 1], (k, 3))
    return p.astype(np.float32)


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):                             # the first repetition warms the shapes up
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
            name = e.name.split("(")[0].replace("void ", "")
            per[name] = per.get(name, 0.0) + float(us)
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


def host_kdtree(pred, gt, m):
    from scipy.spatial import cKDTree
    out = {}
    t0 = time.perf_counter()
    means = []
    for src, dst in ((pred, gt), (gt, pred)):
        tree = cKDTree(dst.astype(np.float64))
        d, _ = tree.query(src.astype(np.float64), k=1, workers=-1, **({} if m is None else {"distance_upper_bound": m}))
        if m is not None:
            d = np.minimum(d, m)
        means.append(float(d.mean()))
    out.update(kind="scipy.spatial.cKDTree, float64, build + query, both directions, workers=-1", seconds=round(time.perf_counter() - t0, 3), measured=True,
               accuracy=means[0], completeness=means[1])
    return out


def host_all_pairs(pred, gt, m, sample=2000, chunk=64):
    q = pred[:: max(len(pred) // sample, 1)][:sample]
    t0 = time.perf_counter()
    for a in range(0, len(q), chunk):
        d = ((q[a:a + chunk, None, :] - gt[None, :, :]) ** 2).sum(axis=2)
        d.argmin(axis=1)
    per_query = (time.perf_counter() - t0) / len(q)
    return dict(kind="numpy all-pairs, float32, chunked", queries_sampled=len(q), seconds_per_query=per_query, measured=False,
                extrapolated_seconds=per_query * (len(pred) + len(gt)),
                label="EXTRAPOLATED from the sample: an all-pairs search costs the same per query, the full size was not run on the host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--max-dist", type=float, default=0.02)
    ap.add_argument("--floaters", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    rows = []
    for N in a.points:
        pred_h, gt_h = sheet(N, 1, a.floaters), sheet(N, 2, 0.0)
        pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
        for m in (None, a.max_dist):
            fn = lambda: chamfer.surface_distance(pred, gt, max_dist=m, thresholds=TAUS)
            ms, out = timed(fn, a.reps)
            launches, per = profile_kernels(fn)
            syncs = count_syncs(fn)
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            med = float(np.median(ms))
            row = dict(N_pred=len(pred_h), N_gt=len(gt_h), max_dist=m,
                       device=dict(ms=[round(x, 3) for x in ms], ms_median=round(med, 3), queries_per_second=round((len(pred_h) + len(gt_h)) / (med / 1e3)),
                                   kernel_launches=launches, kernel_ms=round(sum(per.values()) / 1e3, 3),
                                   kernel_us_top={k: round(v, 1) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]},
                                   host_synchronisations=syncs, bytes_inputs=int(before), bytes_peak_above_inputs=int(peak - before)),
                       result={k: out[k] for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore")})
            if not a.no_host:
                row["host"] = host_kdtree(pred_h, gt_h, m) if have_scipy else host_all_pairs(pred_h, gt_h, m)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del pred, gt
        torch.cuda.empty_cache()
    ratios = {}
    for m in (None, a.max_dist):
        by_n = {r["N_pred"]: r["device"]["ms_median"] for r in rows if r["max_dist"] == m}
        if len(by_n) >= 2:
            lo, hi = min(by_n), max(by_n)
            ratios["none" if m is None else str(m)] = dict(sizes=[lo, hi], time_ratio=round(by_n[hi] / by_n[lo], 3), per_query_ratio=round(by_n[hi] / by_n[lo] / (hi / lo), 3))
    doc = dict(device=torch.cuda.get_device_name(0), timing="HIP events around one whole surface_distance call on two point clouds (both directions), ms; host in seconds",
               host_cores=os.cpu_count(), host_cores_usable=len(os.sched_getaffinity(0)), thresholds=list(TAUS), floaters=a.floaters, time_ratio_large_over_small=ratios,
               rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
