"""Measures the registration of a cloud to its ground truth on the device against a KD-tree ICP on the host -> profiles/register.json.

    python tools/bench_register.py [--points 1000000 10000000] [--cap 0.05] [--max-iteration 30] [--reps 2] [--no-host] [--host-full-up-to 1000000]

The scene: two independently jittered samplings of one synthetic sheet z = 0.05 sin(3x) cos(2y) over [0,10]^2 (tools/bench_chamfer.py's); the target
is the second one, the source is the first one with 0.1 % floaters spread over [0,10]^2 x [-1,1], taken through the inverse of a known rigid motion
(0.3 degrees about (1,2,3) and a move of (0.012, -0.008, 0.005)), so that the registration has to find that motion.  Per size N x N: one whole
gsrast.register.icp call (wall time by HIP events around the call, the host read included; kernel time and launches from the profiler; host
synchronisations from torch's sync debug mode -- the file says whether that was 1; peak memory above the inputs from the caching allocator), what
it found, and ONE iteration taken apart with the public functions: the grid's build, transform_points, NearestGrid.query, correspondence_sums,
solve_transform (the last with its host read).  At the smallest size also the launch count at two values of max_iteration: their difference over
the difference of the iterations done is the launches of one iteration, and what is left is the build, once.  Each kind of measurement is a run of
its own.  No time or ratio is asserted.
Baseline: scipy.spatial.cKDTree (float64, workers=-1) + a numpy SVD fit on the host, the same loop and the same stop rule.  Up to --host-full-up-to
points it is measured in full; above, the tree's build and ONE iteration are measured and scaled to the device's number of iterations, labelled as
an extrapolation.  Without scipy there is no host figure."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gsrast import chamfer, register  # noqa: E402
from bench_chamfer import count_syncs, profile_kernels, sheet, timed  # noqa: E402


def motion():
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.radians(0.3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = [0.012, -0.008, 0.005]
    return M


def host_fit(p, q):
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    U, _, Vt = np.linalg.svd((q - qm).T @ (p - pm))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, qm - R @ pm
    return M


def host_icp(src, tgt, cap, max_iteration, rf, rr, full, device_iterations):
    from scipy.spatial import cKDTree
    src64 = src.astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(tgt.astype(np.float64))
    build = time.perf_counter() - t0
    M, prev, k, per_iteration = np.eye(4), None, 0, []
    while True:
        t1 = time.perf_counter()
        moved = src64 @ M[:3, :3].T + M[:3, 3]
        d, i = tree.query(moved, k=1, workers=-1, distance_upper_bound=cap)
        ok = np.isfinite(d)
        n = int(ok.sum())
        fit, rmse = n / len(src), (float(np.sqrt((d[ok] ** 2).sum() / n)) if n else 0.0)
        stop = (prev is not None and abs(fit - prev[0]) < rf and abs(rmse - prev[1]) < rr) or k == max_iteration or n < 3
        if not stop:
            M = host_fit(src64[ok], tree.data[i[ok]])
            k += 1
        per_iteration.append(time.perf_counter() - t1)
        prev = (fit, rmse)
        if stop or not full:
            break
    kind = "scipy.spatial.cKDTree (float64, workers=-1) + numpy SVD fit on the host, the device's loop and stop rule"
    if full:
        return dict(kind=kind, measured=True, seconds=round(time.perf_counter() - t0, 3), build_seconds=round(build, 3), iterations=k, fitness=fit, inlier_rmse=rmse)
    return dict(kind=kind, measured=False, build_seconds=round(build, 3), one_iteration_seconds=round(per_iteration[0], 3), iterations_assumed=device_iterations,
                extrapolated_seconds=round(build + per_iteration[0] * (device_iterations + 1), 3),
                label="EXTRAPOLATED: the tree's build and one iteration (query + fit) were measured in full, the loop was not run; scaled to the device's iteration count + 1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--cap", type=float, default=0.05)
    ap.add_argument("--max-iteration", type=int, default=30)
    ap.add_argument("--floaters", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-full-up-to", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    rf = rr = 1e-6
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    M_true = motion()
    inv = np.linalg.inv(M_true)
    rows, launch_rows = [], []
    for n_i, N in enumerate(a.points):
        first, tgt_h = sheet(N, 1, a.floaters), sheet(N, 2, 0.0)
        src_h = (first.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
        fn = lambda it=a.max_iteration: register.icp(src, tgt, a.cap, max_iteration=it, relative_fitness=rf, relative_rmse=rr)
        ms, out = timed(fn, a.reps)
        launches, per = profile_kernels(fn)
        syncs = count_syncs(fn)
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        # one iteration, taken apart
        build_ms, grid = timed(lambda: chamfer.NearestGrid(tgt, a.cap), a.reps)
        tr_ms, moved = timed(lambda: register.transform_points(src, out.transformation), a.reps)
        q_ms, (d2, idx) = timed(lambda: grid.query(moved), a.reps)
        s_ms, record = timed(lambda: register.correspondence_sums(src, tgt, idx), a.reps)
        so_ms, _ = timed(lambda: register.solve_transform(record), a.reps)
        med = lambda x: round(float(np.median(x)), 3)
        err = float(np.abs(out.transformation.numpy() - M_true).max())
        row = dict(N_source=len(src_h), N_target=len(tgt_h), cap=a.cap, max_iteration=a.max_iteration,
                   device=dict(ms=[round(x, 3) for x in ms], ms_median=med(ms), kernel_launches=launches, kernel_ms=round(sum(per.values()) / 1e3, 3),
                               kernel_us_top={k: round(v, 1) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]},
                               host_syncs=syncs, host_syncs_is_1=syncs == 1, bytes_inputs=int(before), bytes_peak_above_inputs=int(peak - before)),
                   one_iteration_ms=dict(grid_build_once=med(build_ms), transform=med(tr_ms), query=med(q_ms), sums=med(s_ms), solve_with_its_host_read=med(so_ms)),
                   result=dict(iterations=out.iterations, converged=out.converged, status=out.status, fitness=out.fitness, inlier_rmse=out.inlier_rmse,
                               n_inliers=out.n_inliers, max_abs_difference_from_the_known_motion=err))
        if n_i == 0:                                      # the build happens once: the launch count at two values of max_iteration
            for it in sorted({min(3, a.max_iteration), a.max_iteration}):
                n_launch, _ = profile_kernels(lambda: fn(it))
                launch_rows.append(dict(N=len(src_h), max_iteration=it, iterations_done=fn(it).iterations, kernel_launches=n_launch))
        if not a.no_host and have_scipy:
            row["host"] = host_icp(src_h, tgt_h, a.cap, a.max_iteration, rf, rr, N <= a.host_full_up_to, out.iterations)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del src, tgt, grid, moved, d2, idx, record
        torch.cuda.empty_cache()
    note = None
    if len(launch_rows) == 2:
        lo, hi = launch_rows
        note = dict(launches_enqueued_per_iteration=(hi["kernel_launches"] - lo["kernel_launches"]) / max(hi["max_iteration"] - lo["max_iteration"], 1),
                    expected_per_iteration=register.LAUNCHES_PER_ITERATION,
                    meaning="every launch of max_iteration iterations is enqueued whatever the stop; the difference between the two rows is iterations only, the build is in both once")
    doc = dict(device=torch.cuda.get_device_name(0), timing="HIP events around one whole icp call (host read included), ms; host in seconds",
               host_cores=os.cpu_count(), host_cores_usable=len(os.sched_getaffinity(0)), floaters=a.floaters, relative_fitness=rf, relative_rmse=rr,
               host_baseline=("scipy" if have_scipy else "none: scipy is not installed, no host figure was taken"),
               launches_at_two_max_iterations=launch_rows, launches_note=note, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
