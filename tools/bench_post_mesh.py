"""One post_process_mesh call on the device: gsrast.mesh.post_process_mesh against the numpy / scipy restatement of the same filter on the host.

    python tools/bench_post_mesh.py [--sizes 1000000 10000000] [--out profiles/post_mesh.json]

The mesh is synthetic: one large welded sheet (a square grid, 90 % of the triangles) and many small floaters (tetrahedra on vertices of their own),
with the floaters' triangles dealt into the sheet's in runs, the way a TSDF mesh of a Gaussian scene carries them.  cluster_to_keep = 1: the sheet
stays.  The host path is tests/ref_post_mesh_numpy.post_process_mesh on the arrays copied to the host (the copies are timed apart) -- what a user
without this module would do with Open3D in its place; it is the baseline and the check (results must be byte-identical), never the code under
test.  Times are HIP-event times of one whole call (its host read-back included), clocks warmed, the shape warmed once; launches and per-kernel
device times come from the torch profiler, host synchronisations from torch's sync debug mode, peak memory from the caching allocator, each in a
run of its own.  The host-synchronisation count is a condition: anything but 1 fails the run.  Prints and writes JSON."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
import post_mesh_cases as PC        # noqa: E402
import ref_post_mesh_numpy as R     # noqa: E402
import gsrast                      # noqa: E402
from gsrast import mesh as M        # noqa: E402
from gsrast.tsdf import TriangleMesh   # noqa: E402

K = 1


def make_mesh(T, seed=0):
    """-> (vertices, colours, triangles) numpy, exactly T triangles: a grid of 2 n^2 ~ 0.9 T triangles, tetrahedra for the rest (the last one cut short)."""
    n = int(np.sqrt(0.45 * T))
    sheet = PC.grid(n)
    nv = (n + 1) ** 2
    rest = T - len(sheet)
    nt = (rest + 3) // 4
    tets = (PC.tetrahedron()[None] + (nv + 4 * np.arange(nt, dtype=np.int64))[:, None, None]).reshape(-1, 3)[:rest].astype(np.int32)
    # runs of 4096 sheet triangles, each followed by its share of the floaters
    runs = max(1, len(sheet) // 4096)
    parts = []
    for a, b in zip(np.array_split(np.arange(len(sheet)), runs), np.array_split(np.arange(len(tets)), runs)):
        parts += [sheet[a], tets[b]]
    return PC.with_attributes(np.concatenate(parts), nv + 4 * nt, seed)


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


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):                                    # the first repetition is the warm-up of this shape
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); out = fn(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms[1:], out


def profile_kernels(fn):
    """-> (launches, {kernel name: device microseconds})."""
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
            per[e.name.split("(")[0]] = per.get(e.name.split("(")[0], 0.0) + float(us)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_mesh.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_post_mesh.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "cluster_to_keep": K, "timing": "HIP events around one whole call, ms",
           "host_path": "numpy + scipy.sparse.csgraph restatement on arrays copied to the host", "sizes": []}
    warm_clocks(dev)
    ok = True
    for T in a.sizes:
        v, c, t = make_mesh(T, seed=T % 997)
        m = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (v, c, t)))
        call = lambda: M.post_process_mesh(m, K)
        ms, out = timed(call, a.reps)
        row = {"triangles": int(T), "vertices": int(len(v)), "ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3),
               "triangles_after": int(out.triangles.shape[0]), "vertices_after": int(out.vertices.shape[0])}
        try:
            row["kernel_launches"], per = profile_kernels(call)
            row["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])}
        except Exception as e:                                    # the profiler is optional equipment
            row["kernel_launches"] = f"not measured ({type(e).__name__})"
        row["host_synchronisations"] = count_syncs(call)
        ok = ok and row["host_synchronisations"] == 1
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        row["bytes_inputs"], row["bytes_peak"] = int(before), int(torch.cuda.max_memory_allocated())
        row["bytes_outputs"] = int(sum(x.numel() * x.element_size() for x in (out.vertices, out.vertex_colors, out.triangles)))
        row["bytes_scratch"] = int(gsrast.lib().gsr_mesh_post_scratch_bytes(T, len(v)))
        # the host path: copy down, filter, (a user would then copy up or write the file from the host)
        t0 = time.perf_counter()
        hv, hc, ht = (x.cpu().numpy() for x in (m.vertices, m.vertex_colors, m.triangles))
        t1 = time.perf_counter()
        want = R.post_process_mesh(hv, hc, ht, K)[:3]
        t2 = time.perf_counter()
        row["host_copy_ms"], row["host_filter_ms"] = round((t1 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
        got = tuple(x.cpu().numpy() for x in (out.vertices, out.vertex_colors, out.triangles))
        row["equals_host_restatement"] = bool(all(g.tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want)))
        ok = ok and row["equals_host_restatement"]
        row["speedup_over_host"] = round((row["host_copy_ms"] + row["host_filter_ms"]) / row["ms_median"], 1)
        print(json.dumps(row), flush=True)
        res["sizes"].append(row)
        del m, out, got, want
        torch.cuda.empty_cache()
    res["host_synchronisations_is_1"] = bool(all(r["host_synchronisations"] == 1 for r in res["sizes"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not ok:
        raise SystemExit("bench_post_mesh.py: the call must make exactly one host synchronisation and equal the host restatement")


if __name__ == "__main__":
    main()
