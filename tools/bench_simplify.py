"""One simplify_vertex_clustering call on the device: gsrast.mesh.simplify_vertex_clustering against a vectorised numpy restatement on the host.

    python tools/bench_simplify.py [--sizes 1000000 10000000] [--out profiles/simplify.json]

The mesh has the topology of tools/bench_post_mesh.py -- one large welded sheet (a square grid, 90 % of the triangles) and many small floaters
(tetrahedra on vertices of their own), the floaters' triangles dealt into the sheet's in runs -- and a geometry: the sheet is a gently rolling height
field with unit edge length, the floaters are small tetrahedra scattered above and below it.  voxel_size is 2 x and 4 x the sheet's edge length, both
contractions run.  The host path (host_simplify below: np.unique for the cells, np.bincount for the sums -- it adds in input order, so the bits are
those of the definition --, the quadrics as array expressions in the definition's operation order) on the arrays copied to the host is the baseline and
the check (results must be byte-identical), never the code under test; it is what a user without this module would write around numpy, with Open3D's
call in its place.  It is measured in full at every size here; --host-sample N measures it on the first N triangles' worth of a larger mesh instead and
labels the figure as an extrapolation.  Times are HIP-event times of one whole call (its host read-back included), clocks warmed, the shape warmed
once; launches and per-kernel device times come from the torch profiler, host synchronisations from torch's sync debug mode, peak memory from the
caching allocator, each in a run of its own.  The largest cell population is recorded because the per-cell sums are sequential: one thread walks
one cell.  The host-synchronisation count is a condition: anything but 1 fails the run.  Prints and writes JSON."""
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


def make_mesh(T, seed=0):
    """-> (vertices, colours, triangles) numpy, exactly T triangles: bench_post_mesh's index buffer with positions under it."""
    import bench_post_mesh as B
    _, c, t = B.make_mesh(T, seed)
    n = int(np.sqrt(0.45 * T))
    nv = (n + 1) ** 2
    r = np.random.default_rng(seed + 1)
    v = np.empty((len(c), 3), np.float64)
    i, j = np.divmod(np.arange(nv), n + 1)
    v[:nv] = np.stack([i + r.uniform(-0.2, 0.2, nv), j + r.uniform(-0.2, 0.2, nv), 6.0 * np.sin(i / 23.0) * np.cos(j / 31.0) + r.normal(0.0, 0.05, nv)], axis=1)
    nt = (len(c) - nv) // 4
    centre = np.stack([r.uniform(0, n, nt), r.uniform(0, n, nt), r.uniform(-30.0, 30.0, nt)], axis=1)
    corners = np.array([(0, 0, 0), (0.4, 0, 0), (0, 0.4, 0), (0, 0, 0.4)])
    v[nv:] = (centre[:, None, :] + corners[None]).reshape(-1, 3)
    return v.astype(np.float32), c, t


def host_simplify(v, c, t, voxel_size, contraction="average"):
    """The definition of include/gsrast.h ("mesh simplification") with numpy arrays, bit for bit: -> (vertices, colours, triangles, vertex_map,
    quadric cells, largest cell population).  Inputs must be finite, in range and within the 2^21 cells per axis."""
    vs = float(voxel_size)
    v64 = v.astype(np.float64)
    o = v.min(axis=0).astype(np.float64) - 0.5 * vs
    cell = np.floor((v64 - o) / vs).astype(np.int64)
    key = cell[:, 0] | (cell[:, 1] << 21) | (cell[:, 2] << 42)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))      # cells numbered by their lowest member
    vmap = rank[inv.reshape(-1)]
    n = len(first)
    count = np.bincount(vmap, minlength=n)
    cnt = count.astype(np.float64)
    with np.errstate(all="ignore"):
        nv = np.stack([np.bincount(vmap, weights=v64[:, a], minlength=n) / cnt for a in range(3)], axis=1).astype(np.float32)      # bincount adds in input order
        nc = np.stack([np.bincount(vmap, weights=c[:, a].astype(np.float64), minlength=n) / cnt for a in range(3)], axis=1).astype(np.float32)
    took = np.zeros(n, bool)
    if contraction == "quadric" and len(t):
        with np.errstate(all="ignore"):
            A = v64[t[:, 0]] - o
            e1 = (v64[t[:, 1]] - o) - A
            e2 = (v64[t[:, 2]] - o) - A
            N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
            good = np.isfinite(L) & (L > 0.0)
            p = np.empty((len(t), 4))
            p[:, :3] = N / L[:, None]
            p[:, 3] = -((p[:, 0] * A[:, 0] + p[:, 1] * A[:, 1]) + p[:, 2] * A[:, 2])
            w = L * 0.5
            corner_cell = vmap[t[good]].reshape(-1)              # (triangle, corner) order
            Q = []
            for a in range(4):
                for b in range(a, 4):
                    q = (w * (p[:, a] * p[:, b]))[good]
                    Q.append(np.bincount(corner_cell, weights=np.repeat(q, 3), minlength=n))
            a00, a01, a02, a11, a12, a22 = Q[0], Q[1], Q[2], Q[4], Q[5], Q[7]
            r0, r1, r2 = -Q[3], -Q[6], -Q[8]
            c00 = a11 * a22 - a12 * a12
            c01 = a02 * a12 - a01 * a22
            c02 = a01 * a12 - a02 * a11
            c11 = a00 * a22 - a02 * a02
            c12 = a01 * a02 - a00 * a12
            c22 = a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
            cc = cell[first[np.argsort(first, kind="stable")]].astype(np.float64)
            took = np.isfinite(det) & (det > 0.0) & np.isfinite(x).all(1) & ((x >= cc * vs) & (x <= (cc + 1.0) * vs)).all(1)
            nv[took] = (o + x[took]).astype(np.float32)
    m = vmap[t] if len(t) else np.zeros((0, 3), np.int64)
    live = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 2] != m[:, 0])
    k = np.argmin(m, axis=1)
    rows = np.arange(len(m))
    rot = np.stack([m[rows, k], m[rows, (k + 1) % 3], m[rows, (k + 2) % 3]], axis=1)[live]
    if n ** 3 < 2 ** 63:
        _, keep = np.unique((rot[:, 0] * n + rot[:, 1]) * n + rot[:, 2], return_index=True)
    else:
        _, keep = np.unique(rot, axis=0, return_index=True)
    tris = rot[np.sort(keep)].astype(np.int32)
    return nv, nc, tris, vmap.astype(np.int32), int(took.sum()), int(count.max()) if n else 0


def main():
    import torch
    import bench_post_mesh as B
    import gsrast
    from gsrast import mesh as M
    from gsrast.tsdf import TriangleMesh
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=0, help="measure the host path on a mesh of this many triangles and extrapolate linearly (0: in full)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "timing": "HIP events around one whole call, ms",
           "edge_length": 1.0, "host_path": "vectorised numpy restatement (np.unique, np.bincount) on arrays copied to the host, one thread", "rows": []}
    B.warm_clocks(dev)
    ok = True
    for T in a.sizes:
        v, c, t = make_mesh(T, seed=T % 997)
        m = TriangleMesh(*(torch.from_numpy(x).to(dev) for x in (v, c, t)))
        t0 = time.perf_counter()
        hv, hc, ht = (x.cpu().numpy() for x in (m.vertices, m.vertex_colors, m.triangles))
        copy_ms = (time.perf_counter() - t0) * 1e3
        for factor in (2.0, 4.0):
            for mode in ("average", "quadric"):
                call = lambda: M._simplify(m, factor, mode, True)
                ms, out = B.timed(call, a.reps)
                rec = out[4]
                row = {"triangles": int(T), "vertices": int(len(v)), "voxel_size": factor, "contraction": mode, "ms": [round(x, 3) for x in ms],
                       "ms_median": round(float(np.median(ms)), 3), "vertices_after": rec[1], "triangles_after": rec[2], "quadric_cells": rec[3],
                       "largest_cell_population": int(torch.bincount(out[3].long()).max())}
                try:
                    row["kernel_launches"], per = B.profile_kernels(call)
                    row["kernel_ms_total"] = round(sum(per.values()) / 1e3, 3)
                    row["kernel_us"] = {k: round(x, 1) for k, x in sorted(per.items(), key=lambda kv: -kv[1])}
                except Exception as e:                            # the profiler is optional equipment
                    row["kernel_launches"] = f"not measured ({type(e).__name__})"
                row["host_synchronisations"] = B.count_syncs(call)
                ok = ok and row["host_synchronisations"] == 1
                del out
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                out = call()
                torch.cuda.synchronize()
                row["bytes_inputs"], row["bytes_peak_above_inputs"] = int(before), int(torch.cuda.max_memory_allocated() - before)
                row["bytes_outputs"] = int(sum(x.numel() * x.element_size() for x in out[:4]))
                row["bytes_scratch"] = int(gsrast.lib().gsr_mesh_simplify_scratch_bytes(T, len(v), M.CONTRACTIONS[mode]))
                got = tuple(x.cpu().numpy() for x in out[:4])
                del out
                if a.host_sample and a.host_sample < T:
                    sv, sc, st = make_mesh(a.host_sample, seed=T % 997)
                    t1 = time.perf_counter()
                    host_simplify(sv, sc, st, factor, mode)
                    row["host_simplify_ms"] = round((time.perf_counter() - t1) * 1e3 * T / a.host_sample, 1)
                    row["host_simplify_ms_is"] = f"an extrapolation from {a.host_sample} triangles, linear in T, {os.cpu_count()} host cores (one used)"
                    row["equals_host_restatement"] = "not compared (sampled host path)"
                else:
                    t1 = time.perf_counter()
                    want = host_simplify(hv, hc, ht, factor, mode)
                    row["host_simplify_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
                    row["equals_host_restatement"] = bool(all(g.tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want[:4])) and
                                                          want[4] == rec[3] and want[5] == row["largest_cell_population"])
                    ok = ok and row["equals_host_restatement"]
                row["host_copy_ms"] = round(copy_ms, 1)
                row["speedup_over_host"] = round((row["host_copy_ms"] + row["host_simplify_ms"]) / row["ms_median"], 1)
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
        del m
        torch.cuda.empty_cache()
    res["host_synchronisations_is_1"] = bool(all(r["host_synchronisations"] == 1 for r in res["rows"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not ok:
        raise SystemExit("bench_simplify.py: the call must make exactly one host synchronisation and equal the host restatement")


if __name__ == "__main__":
    main()
