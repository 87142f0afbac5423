"""Measures the scene split on the device against a numpy restatement of the reference's loops on the host -> profiles/partition.json.

    python tools/bench_partition.py [--points 1000000 5000000] [--images 300 3000] [--tiles 8 64] [--reps 2] [--obs 400]

Per (N points, C images, T tiles) on a synthetic aerial scene (a ground cloud, a grid of low oblique cameras, T grid tiles): one
gsrast.partition.partition_tensors (steps 2 to 4; step 1 is host work in both versions and is left out), and the reference's loops restated here:
per tile a Python loop over every camera centre and every point, per (tile, image outside it) a scipy hull and an exact convex clip, per tile np.unique
over its images' ids and one dict lookup per id.  The reference's distCUDA2 call is left out of the host side (it runs on the device there too).  The host loops
are timed on a sample (--host-points points, --host-pairs (tile, image) pairs, two tiles' coverage) and scaled to the scene: recorded as measured and as
extrapolated, and labelled so.  Recorded: wall time (HIP events around the whole call, host reads included), kernel time and launches from the
profiler, host synchronisations from torch's sync debug mode, peak memory from the caching allocator, the host's core count.  Each kind of measurement
is a run of its own.  No ratio is asserted."""
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
from gsrast import partition  # noqa: E402

EXTENT = 100.0


def scene(N, C, T, obs, seed=0):
    """-> dict of numpy arrays: a ground cloud over [0, EXTENT]^2 generated cell by cell (a cell's points are contiguous), a jittered grid of cameras at
    heights comparable with a tile's size looking obliquely at the ground, T tiles by cutting the cameras' x and y into equal counts."""
    r = np.random.default_rng(seed)
    G = 32
    per = N // (G * G)
    N = per * G * G
    cell = np.repeat(np.arange(G * G), per)
    xyz = np.stack([(cell % G + r.random(N)) * EXTENT / G, (cell // G + r.random(N)) * EXTENT / G, r.normal(0, 0.3, N)], axis=1)
    side = int(np.ceil(np.sqrt(C)))
    k = r.permutation(side * side)[:C]
    tile_size = EXTENT / np.sqrt(T)
    cen = np.stack([(k % side + r.uniform(0.2, 0.8, C)) * EXTENT / side, (k // side + r.uniform(0.2, 0.8, C)) * EXTENT / side, r.uniform(0.15, 0.35, C) * tile_size], axis=1)
    ang, rad = r.uniform(0, 2 * np.pi, C), r.uniform(0.2, 0.6, C) * tile_size
    target = np.stack([np.clip(cen[:, 0] + rad * np.cos(ang), 0, EXTENT - 1e-6), np.clip(cen[:, 1] + rad * np.sin(ang), 0, EXTENT - 1e-6), np.zeros(C)], axis=1)
    f = target - cen
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    right = np.cross(np.array([0.0, 0.0, -1.0]), f); right /= np.linalg.norm(right, axis=1, keepdims=True)
    up = np.cross(f, right)
    R = np.stack([right, up, f], axis=1)
    E = np.concatenate([R, -(R @ cen[:, :, None])], axis=2)
    intr = np.tile(np.array([[600.0, 600.0, 1000.0, 750.0]]), (C, 1))
    tc = np.minimum((target[:, 0] * G / EXTENT).astype(np.int64), G - 1) + G * np.minimum((target[:, 1] * G / EXTENT).astype(np.int64), G - 1)
    ids = (tc[:, None] * per + r.integers(0, per, (C, obs))).astype(np.int64)
    ids[r.random(ids.shape) < 0.05] = -1
    cols = max(d for d in range(1, int(np.sqrt(T)) + 1) if T % d == 0)
    rows = T // cols
    order = np.argsort(cen[:, 0], kind="stable")
    boxes = []
    for col in np.array_split(order, cols):
        for t in np.array_split(col[np.argsort(cen[col, 1], kind="stable")], rows):
            boxes.append([cen[t, 0].min(), cen[t, 0].max(), cen[t, 1].min(), cen[t, 1].max()])
    return dict(xyz=xyz, cen=cen, E=E, intr=intr, obs_offsets=np.arange(C + 1, dtype=np.int64) * obs, obs_ids=ids.reshape(-1), point_ids=np.arange(N, dtype=np.int64),
                boxes=np.array(boxes, np.float64))


# ---------------------------------------------------------------------------------------------------------------- the reference's loops on the host
def clip_area(poly, w, h):
    pts = [tuple(p) for p in poly]
    for axis, bound, ge in ((0, 0.0, True), (0, w, False), (1, 0.0, True), (1, h, False)):
        out = []
        for i, cur in enumerate(pts):
            prev = pts[i - 1]
            cin = cur[axis] >= bound if ge else cur[axis] <= bound
            pin = prev[axis] >= bound if ge else prev[axis] <= bound
            if cin != pin:
                g = (bound - prev[axis]) / (cur[axis] - prev[axis])
                o = prev[1 - axis] + g * (cur[1 - axis] - prev[1 - axis])
                out.append((bound, o) if axis == 0 else (o, bound))
            if cin:
                out.append(cur)
        pts = out
    if len(pts) < 3:
        return 0.0
    return 0.5 * abs(sum(pts[i][0] * pts[(i + 1) % len(pts)][1] - pts[(i + 1) % len(pts)][0] * pts[i][1] for i in range(len(pts))))


def host_loops(sc, ratio, host_points, host_pairs):
    """-> dict of seconds: measured on the sample, and scaled to the scene."""
    from scipy.spatial import ConvexHull
    N, C, T = len(sc["xyz"]), len(sc["cen"]), len(sc["boxes"])
    b = sc["boxes"]
    dw, dh = (b[:, 1] - b[:, 0]) * ratio / 2.0, (b[:, 3] - b[:, 2]) * ratio / 2.0
    grown = np.stack([b[:, 0] - dw, b[:, 1] + dw, b[:, 2] - dh, b[:, 3] + dh], axis=1)
    n = min(host_points, N)
    pts = {i: sc["xyz"][i] for i in range(0, N, max(N // n, 1))}
    t0 = time.perf_counter()
    for box in grown[:2]:                                 # box_based_update's loop over the points dict
        inside = []
        for i, xyz in pts.items():
            if (xyz[0] >= box[0]) & (xyz[0] <= box[1]) & (xyz[1] >= box[2]) & (xyz[1] <= box[3]):
                inside.append(i)
    s_box = (time.perf_counter() - t0) / (2 * len(pts))   # per (point, tile)
    pairs = min(host_pairs, T * C)
    t0 = time.perf_counter()
    for k in range(pairs):                                # visibility_based_camera_selection's loop body
        t, c = k % T, (k * 7919) % C
        mx, Mx, my, My = b[t]
        cor = np.array([[x, y, z, 1.0] for x in (mx, Mx) for y in (my, My) for z in (-1.0, 1.0)])
        w2c = np.concatenate([sc["E"][c], [[0, 0, 0, 1.0]]])
        fx, fy, w, h = sc["intr"][c]
        K = np.array([[fx, 0.0, w / 2.0], [0.0, fy, h / 2.0], [0, 0, 1]])
        pc = (w2c @ cor.T).T
        pc = pc[:, :3] / pc[:, 3:4]
        uv = (K @ pc.T).T
        uv = uv[:, :2] / uv[:, 2:3]
        hull = uv[ConvexHull(uv).vertices.tolist()]
        _ = clip_area(hull, w, h) / (w * h)
        _ = np.mean(np.sum(np.sqrt(np.power(cor[:, :3] - sc["cen"][c][np.newaxis, :], 2)), axis=1))
    s_pair = (time.perf_counter() - t0) / pairs
    table = {int(i): i for i in sc["point_ids"][:min(N, 2_000_000)]}
    per_tile = max(C // T, 1)
    obs = sc["obs_offsets"][1]
    t0 = time.perf_counter()
    looked = 0
    for t in range(min(T, 2)):                            # coverage_based_point_selection's loop body
        ids = [sc["obs_ids"][a * obs:(a + 1) * obs] for a in range(t * per_tile, (t + 1) * per_tile)]
        ids = np.unique(np.concatenate([i[i != -1] for i in ids]))
        for i in ids:
            looked += int(i) in table
    s_cover = (time.perf_counter() - t0) / min(T, 2)      # per tile of C / T images
    return dict(measured=dict(points_sampled=len(pts), seconds_per_point_and_tile=s_box, pairs_sampled=pairs, seconds_per_tile_image_pair=s_pair,
                              coverage_tiles_sampled=min(T, 2), seconds_per_tile_coverage=s_cover),
                extrapolated_seconds=dict(step2_points=s_box * N * T, step2_cameras=s_box * C * T, step3_pairs=s_pair * T * C * (1 - 1.0 / T), step4_coverage=s_cover * T,
                                          total=s_box * (N + C) * T + s_pair * T * C * (1 - 1.0 / T) + s_cover * T),
                label="EXTRAPOLATED from the sample: the loops cost the same per element, the scene was not run in full on the host")


# ---------------------------------------------------------------------------------------------------------------- measurement
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
            per[e.name.split("(")[0].replace("void ", "")] = per.get(e.name.split("(")[0].replace("void ", ""), 0.0) + float(us)
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
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--images", type=int, nargs="+", default=[300, 3000])
    ap.add_argument("--tiles", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--obs", type=int, default=400, help="observations per image")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--host-points", type=int, default=100_000)
    ap.add_argument("--host-pairs", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for N in a.points:
        for C in a.images:
            for T in a.tiles:
                sc = scene(N, C, T, a.obs)
                t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                args = (t(sc["boxes"]), t(sc["cen"]), t(sc["E"]), t(sc["intr"]), t(sc["xyz"]), t(sc["obs_offsets"]), t(sc["obs_ids"]), t(sc["point_ids"]))
                fn = lambda: partition.partition_tensors(*args, ratio=a.ratio, threshold=a.threshold)
                ms, out = timed(fn, a.reps)
                launches, per = profile_kernels(fn)
                syncs = count_syncs(fn)
                torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                del out
                out = fn()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated()
                off = out["tile_offsets"].numpy()
                row = dict(N=len(sc["xyz"]), C=C, T=len(sc["boxes"]), observations=int(len(sc["obs_ids"])),
                           device=dict(ms=[round(m, 3) for m in ms], ms_median=round(float(np.median(ms)), 3), kernel_launches=launches,
                                       kernel_ms=round(sum(per.values()) / 1e3, 3), kernel_us_top={k: round(v, 1) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]},
                                       host_synchronisations=syncs, bytes_inputs=int(before), bytes_peak_above_inputs=int(peak - before)),
                           result=dict(images_added=int(out["add"].sum().item()), points_in_boxes=int(out["in_box_counts"].sum().item()), points_covered=int(off[-1])),
                           host_restatement=host_loops(sc, a.ratio, a.host_points, a.host_pairs))
                print(json.dumps(row), flush=True)
                rows.append(row)
                del out, args
                torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), timing="HIP events around one whole partition_tensors call (steps 2 to 4), ms; host loops in seconds",
               host_cores=os.cpu_count(), host_cores_usable=len(os.sched_getaffinity(0)), ratio=a.ratio, threshold=a.threshold, observations_per_image=a.obs, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
