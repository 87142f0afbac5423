"""The mesh rasterizer on the device: one view of gsrast.rasterize_mesh and a 100-view gsrast.triangle_view_counts at 1920 x 1080.

    python tools/bench_mesh_raster.py [--sizes 1000000 10000000] [--views 100] [--out profiles/mesh_raster.json]

The mesh is tools/bench_simplify.py's: one large welded sheet, a gently rolling height field with unit edge length (90 % of the triangles), and small
tetrahedra scattered above and below it.  The cameras stand on a ring above the sheet and look at its centre from a height at which the sheet
about fills the image, so that a triangle of the sheet covers a pixel or less at 10 M triangles and a few pixels at 1 M.  The baseline is the numpy
restatement of the definition (tests/raster_truth.py) on the host: it is timed on the first --host-sample triangles of the mesh in ONE view and the
figure is labelled as an extrapolation, linear in the triangles and the views, with the host's core count (one core used).  Times are HIP-event times
of one whole call (its host read-back included), clocks warmed, the shape warmed once; launches and per-kernel device times come from the torch
profiler, host synchronisations from torch's sync debug mode, each in a run of its own.  The small / large split is counted on the host from the
restatement's set-up (vectorised) on a sample of the triangles in the first view.  The atomics that the plain load in front of them skips are NOT
counted: the kernel keeps no counter.  A last block sweeps `_large_from` over one view of coarser meshes of the same kind (--sweep-sizes), whose
triangles cover tens to hundreds of pixels, and checks that the maps do not change.  The host-synchronisation count is a condition: anything but 1 fails the run.  Prints and writes JSON."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np      # noqa: E402

W, H = 1920, 1080


def cameras(n_views, extent):
    """n_views cameras on a ring above the sheet [0, extent]^2, looking at its centre."""
    import raster_cases as RC
    c = np.array([extent / 2, extent / 2, 0.0])
    out = []
    for k in range(n_views):
        a = 2 * np.pi * k / max(n_views, 1) + 0.1
        eye = c + np.array([0.25 * extent * np.cos(a), 0.25 * extent * np.sin(a), 0.75 * extent])
        out.append(RC.camera(eye, target=c, up=(0.0, 1.0, 0.0), fov_x=1.0, aspect=W / H, znear=0.01, zfar=10.0 * extent))
    return np.stack(out)


def split(v, t, M, large_from, sample):
    """-> (live, small, large) shares among the first `sample` triangles in view M, from the restatement's set-up."""
    import raster_truth as RT
    t = t[:sample]
    state, X, Y, *_ = RT.setup(v, t, M, W, H, 0.01, 0)
    c0, c1 = np.maximum(-((-X.min(1)) // 256), 0), np.minimum(X.max(1) // 256, W - 1)
    r0, r1 = np.maximum(-((-Y.min(1)) // 256), 0), np.minimum(Y.max(1) // 256, H - 1)
    live = (state == RT.OK) & (c0 <= c1) & (r0 <= r1)
    box = np.where(live, (c1 - c0 + 1) * (r1 - r0 + 1), 0)
    n = float(len(t))
    return float(live.sum() / n), float((live & (box <= large_from)).sum() / n), float((box > large_from).sum() / n), float(box[live].mean()) if live.any() else 0.0


def main():
    import torch
    import bench_post_mesh as B
    import bench_simplify as S
    import gsrast
    import raster_truth as RT
    from gsrast import mesh as M
    from gsrast.tsdf import TriangleMesh
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--sweep-sizes", type=int, nargs="*", default=[10000, 100000, 1000000], help="meshes for the large_from sweep")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_raster.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_raster.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "timing": "HIP events around one whole call, ms", "width": W, "height": H,
           "large_from": M.LARGE_FROM, "atomics_skipped_by_the_plain_load": "not counted: the kernel keeps no counter",
           "host_path": "tests/raster_truth.py (numpy, a triangle loop with vectorised boxes) on arrays on the host, one thread", "rows": []}
    B.warm_clocks(dev)
    ok = True
    for T in a.sizes:
        v, c, t = S.make_mesh(T, seed=T % 997)
        extent = float(int(np.sqrt(0.45 * T)))
        mats = cameras(a.views, extent)
        m = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (v, c, t)))
        md = torch.from_numpy(mats).to(dev)
        live, small, large, mean_box = split(v, t, mats[0], M.LARGE_FROM, min(T, 1000000))
        ns = min(a.host_sample, T)
        t1 = time.perf_counter()
        RT.rasterize(v, t[:ns], mats[0], W, H)
        host_view_ms = (time.perf_counter() - t1) * 1e3 * T / ns
        for what, n_views, call in (("rasterize_mesh", 1, lambda: gsrast.rasterize_mesh(m, md[0], W, H)),
                                    ("triangle_view_counts", 1, lambda: gsrast.triangle_view_counts(m, md[:1], W, H, depth_tolerance=0.05)),
                                    ("triangle_view_counts", a.views, lambda: gsrast.triangle_view_counts(m, md, W, H, depth_tolerance=0.05))):
            ms, out = B.timed(call, a.reps)
            med = float(np.median(ms))
            row = {"call": what, "triangles": int(T), "vertices": int(len(v)), "views": n_views, "ms": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                   "triangle_views_per_second": round(T * n_views / (med * 1e-3)), "share_with_candidate_pixels": round(live, 4), "share_small": round(small, 4),
                   "share_large": round(large, 6), "mean_candidate_box": round(mean_box, 2), "split_is": f"counted on the host on the first {min(T, 1000000)} triangles, first view"}
            if what == "rasterize_mesh":
                row["pixels_covered"] = int((out.triangle_id >= 0).sum())
            else:
                row["triangles_seen"] = int((out > 0).sum())
            del out
            try:
                row["kernel_launches"], per = B.profile_kernels(call)
                row["kernel_ms_total"] = round(sum(per.values()) / 1e3, 3)
                row["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])}
            except Exception as e:                            # the profiler is optional equipment
                row["kernel_launches"] = f"not measured ({type(e).__name__})"
            row["host_synchronisations"] = B.count_syncs(call)
            ok = ok and row["host_synchronisations"] == 1
            row["bytes_scratch"] = int(gsrast.lib().gsr_mesh_raster_scratch_bytes(T, len(v), n_views, W, H))
            row["host_truth_ms"] = round(host_view_ms * n_views, 1)
            row["host_truth_ms_is"] = (f"an extrapolation from {ns} triangles in one view, linear in triangles and views, {os.cpu_count()} host cores (one used); "
                                       f"the maps only, without the vertex test")
            row["speedup_over_host"] = round(row["host_truth_ms"] / med, 1)
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
        del m, md
        torch.cuda.empty_cache()
    # the threshold between the two paths: one view of rasterize_mesh on coarser meshes of the same kind, whose triangles cover tens to hundreds of pixels
    res["large_from_sweep"] = []
    for T in a.sweep_sizes:
        v, c, t = S.make_mesh(T, seed=T % 997)
        mats = cameras(1, float(int(np.sqrt(0.45 * T))))
        m = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (v, c, t)))
        md = torch.from_numpy(mats).to(dev)
        live, _, _, mean_box = split(v, t, mats[0], M.LARGE_FROM, min(T, 1000000))
        row = {"triangles": int(T), "share_with_candidate_pixels": round(live, 4), "mean_candidate_box": round(mean_box, 2), "ms_median_by_large_from": {}}
        base = None
        for lf in (0, 4, 16, 64, 256, 1024, 2 ** 31 - 1):
            ms, out = B.timed(lambda: gsrast.rasterize_mesh(m, md, W, H, _large_from=lf), a.reps)
            row["ms_median_by_large_from"][str(lf)] = round(float(np.median(ms)), 3)
            got = out.triangle_id.cpu().numpy().tobytes() + out.depth.cpu().numpy().tobytes()
            base = base or got
            ok = ok and got == base                           # the outputs do not depend on the threshold
        row["share_large_at_default"] = round(split(v, t, mats[0], M.LARGE_FROM, min(T, 1000000))[2], 4)
        print(json.dumps(row), flush=True)
        res["large_from_sweep"].append(row)
        del m, md
        torch.cuda.empty_cache()
    res["host_synchronisations_is_1"] = bool(all(r["host_synchronisations"] == 1 for r in res["rows"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not ok:
        raise SystemExit("bench_mesh_raster.py: every call must make exactly one host synchronisation and the maps must not depend on large_from")


if __name__ == "__main__":
    main()
