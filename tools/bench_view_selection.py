"""Measures the PGSR neighbour-view selection on the device against a numpy restatement of the reference on the host -> profiles/view_selection.json.

    python tools/bench_view_selection.py [--images 300 1000 3000] [--observations 8000] [--reps 2] [--baseline-images 60] [--out FILE]

Per C images x about --observations keypoints each on synthetic tracks (a camera path around a cloud; a point is seen by a window of consecutive
images with drop-outs, a fifth of the keypoints have no point): one gsrast.views.select_views call.  Recorded: wall time (HIP events around the whole
call, the host read included), kernel time and launches from the profiler, host synchronisations from torch's sync debug mode, peak memory from the
caching allocator, the number of terms evaluated (sum over tracks of t (t - 1), both directions) and their rate.  Each kind of measurement is a run
of its own.

The baseline is the reference's calc_score restated with numpy set operations (np.isin on whole id arrays, the terms of a pair vectorised) in ONE
host process.  That is far kinder to the reference than its own `[it for it in id_i if it in id_j]`, a linear search per element.  It is timed at
--baseline-images images of the same density and recorded as measured, with the host's core count beside it (the reference spreads its pairs over a
process pool); the figure for a larger C is that time scaled by the number of pairs and is labelled as an extrapolation.  At the baseline size the
device's scores are also compared with the baseline's.  No ratio is asserted."""
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
from gsrast import lib, views  # noqa: E402

PARAMS = (5.0, 1.0, 10.0)


def scene(C, per_image, seed=0, mean_track=6.0, no_point=0.2):
    """-> centers [C,3], obs_offsets [C+1], obs_ids [M], point_ids [Np], point_xyz [Np,3] (numpy), and the number of terms the scores hold."""
    r = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(C) + 0.3 * r.uniform(-1, 1, C)) / C
    centers = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), r.uniform(-0.5, 0.5, C)], axis=1)
    valid = int(per_image * (1 - no_point))
    n_points = max(int(C * valid / mean_track), 1)
    length = np.minimum(1 + r.geometric(1.0 / (mean_track / 0.8 - 1), n_points), C)      # the window; four fifths of it observed
    start = r.integers(0, C, n_points)
    rep = np.repeat(np.arange(n_points), length)
    img = (np.repeat(start, length) + (np.arange(len(rep)) - np.repeat(np.cumsum(length) - length, length))) % C
    keep = r.uniform(size=len(rep)) < 0.8
    rep, img = rep[keep], img[keep]
    point_ids = np.sort(r.choice(np.arange(1, 8 * n_points), n_points, replace=False)).astype(np.int64)
    none = int(len(rep) * no_point / (1 - no_point))
    img = np.concatenate([img, r.integers(0, C, none)])
    ids = np.concatenate([point_ids[rep], np.full(none, -1, np.int64)])
    order = np.lexsort((r.uniform(size=len(img)), img))                                   # image-major, keypoints in no particular order
    img, ids = img[order], ids[order]
    offsets = np.zeros(C + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(img, minlength=C))
    t = np.bincount(rep)
    return centers, offsets, ids, point_ids, r.normal(0, 0.5, (n_points, 3)), int((t * (t - 1)).sum())


def numpy_baseline(centers, offsets, ids, point_ids, xyz, theta0, sigma1, sigma2):
    """calc_score for every pair with numpy set operations; -> score [C,C]."""
    C = len(centers)
    rows = [ids[offsets[a]:offsets[a + 1]] for a in range(C)]
    rows = [a[a != -1] for a in rows]
    score = np.zeros((C, C))
    for i in range(C):
        for j in range(i + 1, C):
            shared = rows[i][np.isin(rows[i], rows[j])]
            if not len(shared):
                continue
            p = xyz[np.searchsorted(point_ids, shared)]
            a, b = centers[i] - p, centers[j] - p
            theta = (180 / np.pi) * np.arccos((a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1))
            s = np.where(theta <= theta0, sigma1, sigma2)
            score[i, j] = score[j, i] = np.exp(-(theta - theta0) ** 2 / (2 * s ** 2)).sum()
    return score


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


def measure(fn, reps):
    ms, _ = timed(fn, reps)
    ent = {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3)}
    try:
        ent["kernel_launches"], per = profile_kernels(fn)
        ent["kernel_ms"] = round(sum(per.values()) / 1e3, 3)
        top = sorted(per.items(), key=lambda kv: -kv[1])[:6]
        ent["kernel_us_top"] = {k.split("(")[0][:60]: round(v, 1) for k, v in top}
    except Exception as e:                                        # the profiler is optional equipment
        ent["kernel_launches"] = f"not measured ({type(e).__name__})"
    try:
        ent["host_synchronisations"] = count_syncs(fn)
    except Exception as e:
        ent["host_synchronisations"] = f"not measured ({type(e).__name__})"
    before, peak = peak_memory(fn)
    ent["bytes_inputs"], ent["bytes_peak_above_inputs"] = before, peak - before
    return ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[300, 1000, 3000])
    ap.add_argument("--observations", type=int, default=8000)
    ap.add_argument("--num-views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--baseline-images", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_selection.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_view_selection.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "timing": "HIP events around one whole select_views call, ms", "observations_per_image": a.observations,
           "num_views": a.num_views, "rows": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    Cb = a.baseline_images
    sc = scene(Cb, a.observations, seed=Cb)
    t0 = time.perf_counter()
    want = numpy_baseline(*sc[:5], *PARAMS)
    sec = time.perf_counter() - t0
    args = [torch.from_numpy(x).to(dev) for x in sc[:5]]
    _, _, got = views.select_views(*args, *PARAMS, num_views=a.num_views, return_scores=True, wide_ids=False)
    got = got.cpu().numpy()
    pos = want > 0
    res["numpy_baseline"] = {"what": "calc_score restated with np.isin per pair, one host process", "images_measured": Cb, "pairs": Cb * (Cb - 1) // 2,
                             "seconds_measured": round(sec, 3), "ms_per_pair": round(sec * 1e3 / max(Cb * (Cb - 1) // 2, 1), 4), "host_cores": os.cpu_count(),
                             "max_relative_difference_of_device_scores": float((np.abs(got - want)[pos] / want[pos]).max()) if pos.any() else 0.0}
    print(json.dumps(res["numpy_baseline"]), flush=True)
    write()
    for C in a.images:
        centers, offsets, ids, point_ids, xyz, terms = scene(C, a.observations, seed=C)
        args = [torch.from_numpy(x).to(dev) for x in (centers, offsets, ids, point_ids, xyz)]
        row = {"images": C, "observations": int(len(ids)), "observations_with_a_point": int((ids != -1).sum()), "points": int(len(point_ids)), "terms": terms,
               "bytes_scratch": int(lib().gsr_view_select_scratch_bytes(len(ids), C))}
        ent = measure(lambda: views.select_views(*args, *PARAMS, num_views=a.num_views, wide_ids=False), a.reps)
        ent["terms_per_s"] = round(terms / (ent["ms_median"] * 1e-3), 0)
        row["select_views_hip"] = ent
        ms, _ = timed(lambda: views.select_views(*args, *PARAMS, num_views=a.num_views), 1)
        row["select_views_hip_wide_ids_ms"] = round(ms[0], 3)
        row["numpy_baseline_seconds_extrapolated_by_pairs"] = round(res["numpy_baseline"]["ms_per_pair"] * 1e-3 * C * (C - 1) / 2, 1)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del args
        torch.cuda.empty_cache()
        write()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
