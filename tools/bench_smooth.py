"""The smoothing filters and the vertex normals on the device against a vectorised numpy restatement on the host.

    python tools/bench_smooth.py [--sizes 1000000 10000000] [--out profiles/smooth.json]

The mesh is the sheet + height-field mesh of tools/bench_simplify.py (one large welded sheet with unit edge length, 90 % of the triangles, and many
small floaters).  Per size: compute_vertex_normals, and ITERATIONS iterations of each filter in both scopes.  Recorded per row: the whole call (HIP
events around it, its host read-back included), the kernel time, launches and per-kernel device times from the torch profiler, host synchronisations
from torch's sync debug mode, peak memory above the inputs from the caching allocator -- each in a run of its own --, the adjacency build (everything
in front of the first step) apart from the per-step time, and the step's rate against its ALGORITHMIC bytes: 4 B of `start` per vertex, 4 B of index
and one row (24 B in scope "vertex", 48 B in scope "all") per directed edge, one row read and one written per vertex.  Beside it, one step on a
5000-spoke fan, where one thread walks the hub's list.

The host path (host_smooth / host_vertex_normals below) is the baseline and the check, never the code under test: what a user without this module would
write around numpy with Open3D's calls in its place.  The adjacency is built with scipy.sparse where the machine has it (np.unique over the directed
pairs otherwise; the file says which), the per-vertex sums are np.bincount with weights, which adds in input order -- the order of the definition --
so its bits are expected to be the device's.  It is measured in full at every size, on one core of the host's os.cpu_count().  The host-synchronisation
count is a condition (anything but 1 fails the run), and so is the agreement with the host path within the bars of tests/test_gpu_smooth.py."""
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

ITERATIONS = 10
LAMBDA, MU = 0.5, -0.53
try:
    import scipy.sparse as _sp
except Exception:                                         # the baseline says which it used
    _sp = None


def host_adjacency(t, V):
    """-> (src int64 [E], dst int64 [E], start int64 [V + 1]), the directed pairs in ascending (src, dst)."""
    pairs = np.concatenate([t[:, [a, b]] for a in range(3) for b in range(3) if a != b]).astype(np.int64)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    if _sp is not None:
        A = _sp.coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(V, V)).tocsr()
        A.sum_duplicates()
        A.sort_indices()
        start, dst = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    else:
        key = np.unique(pairs[:, 0] * V + pairs[:, 1])
        dst = key % V
        start = np.concatenate([[0], np.cumsum(np.bincount(key // V, minlength=V))])
    return np.repeat(np.arange(V), np.diff(start)), dst, start


def host_smooth(v, c, adj, kind, iterations, scope):
    src, dst, start = adj
    V = len(v)
    p = np.concatenate([v.astype(np.float64), c.astype(np.float64)], axis=1) if scope == "all" else v.astype(np.float64)
    deg = np.diff(start)
    some = deg > 0

    def step(p, lam):
        r = p[dst]
        if lam is None:
            s = np.stack([np.bincount(src, weights=r[:, a], minlength=V) for a in range(p.shape[1])], axis=1)
            # bincount starts from 0 where the definition starts from p: (0 + r0) + r1 ... against (p + r0) + r1 ...; the check below allows the last bit
            return (p + s) / (deg + 1.0)[:, None]
        d = p[src, :3] - r[:, :3]
        w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
        W = np.bincount(src, weights=w, minlength=V)
        s = np.stack([np.bincount(src, weights=w * r[:, a], minlength=V) for a in range(p.shape[1])], axis=1)
        q = p.copy()
        q[some] = p[some] + lam * (s[some] / W[some, None] - p[some])
        return q
    for _ in range(iterations):
        if kind == "simple":
            p = step(p, None)
        else:
            p = step(p, LAMBDA)
            if kind == "taubin":
                p = step(p, MU)
    return p[:, :3].astype(np.float32), (p[:, 3:].astype(np.float32) if scope == "all" else c.copy())


def host_vertex_normals(v, t):
    p = v.astype(np.float64)
    e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    corner = t.reshape(-1).astype(np.int64)                # corner 3 t + k in input order: bincount adds in ascending corner index
    s = np.stack([np.bincount(corner, weights=np.repeat(n[:, a], 3), minlength=len(v)) for a in range(3)], axis=1)
    L = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    ok = (L > 0.0) & np.isfinite(L)
    out = s / np.where(ok, L, 1.0)[:, None]
    out[~ok] = (0.0, 0.0, 1.0)
    return out.astype(np.float32)


def fan(spokes):
    a = 2 * np.pi * np.arange(spokes) / spokes
    v = np.concatenate([[(0.0, 0.0, 0.3)], np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(5 * a)], axis=1)]).astype(np.float32)
    t = np.array([(0, 1 + k, 1 + (k + 1) % spokes) for k in range(spokes)], dtype=np.int32)
    return v, np.full_like(v, 0.5), t


def step_bytes(V, E, scope):
    row = 48 if scope == "all" else 24
    return 4 * V + (4 + row) * E + 2 * row * V


def main():
    import torch
    import bench_post_mesh as B
    import bench_simplify
    import gsrast
    from gsrast import mesh as M
    from gsrast.tsdf import TriangleMesh
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "timing": "HIP events around one whole call, ms", "iterations": ITERATIONS,
           "lambda_filter": LAMBDA, "mu": MU,
           "host_path": "vectorised numpy restatement on arrays copied to the host, one thread: adjacency by "
                        + ("scipy.sparse (coo -> csr, sum_duplicates)" if _sp is not None else "np.unique over the directed pairs (no scipy here)")
                        + ", per-vertex sums by np.bincount with weights",
           "step_bytes_model": "4 B of start per vertex + (4 B index + one row) per directed edge + one row read and one written per vertex; row = 24 B (vertex) or 48 B (all)",
           "not_done": "a float32 state between the steps would halve the gathered bytes: out of scope", "rows": []}
    B.warm_clocks(dev)
    ok = True
    filters = {"simple": lambda m, n, s: M.filter_smooth_simple(m, n, s), "laplacian": lambda m, n, s: M.filter_smooth_laplacian(m, n, LAMBDA, s),
               "taubin": lambda m, n, s: M.filter_smooth_taubin(m, n, LAMBDA, MU, s)}

    def kernel_split(call):
        """-> (launches, total kernel ms, step kernel ms, {kernel: us})."""
        n, per = B.profile_kernels(call)
        step = sum(us for k, us in per.items() if "k_sm_step" in k)
        return n, sum(per.values()) / 1e3, step / 1e3, per

    def peak_above_inputs(call):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        peak = int(torch.cuda.max_memory_allocated() - before)
        del out
        return int(before), peak

    for T in a.sizes:
        v, c, t = bench_simplify.make_mesh(T, seed=T % 997)
        V = len(v)
        m = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (v, c, t)))
        t0 = time.perf_counter()
        hv, hc, ht = (x.cpu().numpy() for x in (m.vertices, m.vertex_colors, m.triangles))
        copy_ms = (time.perf_counter() - t0) * 1e3
        # ---- the adjacency on its own, and the host's
        ms, (start, nb) = B.timed(lambda: M.vertex_adjacency(m), a.reps)
        E = int(nb.shape[0])
        t1 = time.perf_counter()
        adj = host_adjacency(ht, V)
        host_adj_ms = (time.perf_counter() - t1) * 1e3
        same_adj = bool(np.array_equal(start.cpu().numpy(), adj[2]) and np.array_equal(nb.cpu().numpy(), adj[1]))
        ok = ok and same_adj
        deg = np.diff(adj[2])
        row = {"what": "vertex_adjacency", "triangles": int(T), "vertices": int(V), "directed_edges": E, "largest_degree": int(deg.max()),
               "ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "host_ms": round(host_adj_ms, 1), "host_copy_ms": round(copy_ms, 1),
               "equals_host_restatement": same_adj, "host_synchronisations": B.count_syncs(lambda: M.vertex_adjacency(m)),
               "bytes_scratch": int(gsrast.lib().gsr_mesh_adjacency_scratch_bytes(T, V))}
        row["kernel_launches"], row["kernel_ms_total"], _, _ = kernel_split(lambda: M.vertex_adjacency(m))
        row["bytes_inputs"], row["bytes_peak_above_inputs"] = peak_above_inputs(lambda: M.vertex_adjacency(m))
        ok = ok and row["host_synchronisations"] == 1
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del start, nb
        # ---- the vertex normals
        call = lambda: M.compute_vertex_normals(m)
        ms, out = B.timed(call, a.reps)
        t1 = time.perf_counter()
        want = host_vertex_normals(hv, ht)
        host_ms = (time.perf_counter() - t1) * 1e3
        got = out.cpu().numpy()
        del out
        row = {"what": "compute_vertex_normals", "triangles": int(T), "vertices": int(V), "ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3),
               "host_ms": round(host_ms, 1), "host_copy_ms": round(copy_ms, 1), "components_not_bit_equal_to_host": int((got.view(np.int32) != want.view(np.int32)).sum()),
               "max_abs_difference_to_host": float(np.abs(got.astype(np.float64) - want).max()), "host_synchronisations": B.count_syncs(call),
               "bytes_scratch": int(gsrast.lib().gsr_mesh_normals_scratch_bytes(T, V))}
        row["kernel_launches"], row["kernel_ms_total"], _, per = kernel_split(call)
        row["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])}
        row["bytes_inputs"], row["bytes_peak_above_inputs"] = peak_above_inputs(call)
        row["speedup_over_host"] = round((copy_ms + host_ms) / row["ms_median"], 1)
        ok = ok and row["host_synchronisations"] == 1 and row["max_abs_difference_to_host"] <= 2.0 ** -23
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        # ---- the filters
        for kind in ("simple", "laplacian", "taubin"):
            steps = ITERATIONS * (2 if kind == "taubin" else 1)
            for scope in ("all", "vertex"):
                call = lambda: filters[kind](m, ITERATIONS, scope)
                ms, out = B.timed(call, a.reps)
                gv, gc = out.vertices.cpu().numpy(), out.vertex_colors.cpu().numpy()
                del out
                row = {"what": f"filter_smooth_{kind}", "scope": scope, "iterations": ITERATIONS, "steps": steps, "triangles": int(T), "vertices": int(V), "directed_edges": E,
                       "ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "host_synchronisations": B.count_syncs(call),
                       "bytes_scratch": int(gsrast.lib().gsr_mesh_smooth_scratch_bytes(T, V, M.SCOPES[scope]))}
                n, total, step, per = kernel_split(call)
                row["kernel_launches"], row["kernel_ms_total"], row["kernel_ms_steps"] = n, round(total, 3), round(step, 3)
                row["kernel_ms_adjacency_build_and_rest"] = round(total - step, 3)
                row["step_ms"] = round(step / steps, 4)
                row["step_algorithmic_bytes"] = step_bytes(V, E, scope)
                row["step_GBps_against_algorithmic_bytes"] = round(step_bytes(V, E, scope) / (step / steps * 1e-3) / 1e9, 1) if step > 0 else None
                row["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])}
                row["bytes_inputs"], row["bytes_peak_above_inputs"] = peak_above_inputs(call)
                t1 = time.perf_counter()
                wv, wc = host_smooth(hv, hc, adj, kind, ITERATIONS, scope)
                row["host_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
                row["host_ms_is"] = f"the steps alone; the host adjacency ({round(host_adj_ms, 1)} ms) and the copy to the host ({round(copy_ms, 1)} ms) come on top"
                bar = float(np.spacing(np.float32(max(np.abs(hv).max(), np.abs(wv).max()))))
                row["components_not_bit_equal_to_host"] = int((gv.view(np.int32) != wv.view(np.int32)).sum() + (gc.view(np.int32) != wc.view(np.int32)).sum())
                row["max_abs_difference_to_host"] = [float(np.abs(gv.astype(np.float64) - wv).max()), float(np.abs(gc.astype(np.float64) - wc).max())]
                row["within_the_bars"] = bool(row["max_abs_difference_to_host"][0] <= bar and row["max_abs_difference_to_host"][1] <= 2.0 ** -23)
                row["speedup_over_host"] = round((copy_ms + host_adj_ms + row["host_ms"]) / row["ms_median"], 1)
                ok = ok and row["host_synchronisations"] == 1 and row["within_the_bars"]
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
        del m
        torch.cuda.empty_cache()
    # ---- one step on a 5000-spoke fan: one thread walks the hub's list
    fv, fc, ft = fan(5000)
    fm = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (fv, fc, ft)))
    for kind in ("simple", "laplacian"):
        for scope in ("all", "vertex"):
            call = lambda: filters[kind](fm, 1, scope)
            call()
            n, total, step, per = kernel_split(call)
            row = {"what": f"one {kind} step on a 5000-spoke fan", "scope": scope, "vertices": len(fv), "largest_degree": 5000, "step_ms": round(step, 4),
                   "kernel_ms_total": round(total, 3), "kernel_launches": n}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    res["host_synchronisations_is_1"] = bool(all(r.get("host_synchronisations", 1) == 1 for r in res["rows"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not ok:
        raise SystemExit("bench_smooth.py: every call must make exactly one host synchronisation and agree with the host restatement")


if __name__ == "__main__":
    main()
