"""Measures the preparation of a training photograph on the device against Pillow on the host -> profiles/images.json.

    python tools/bench_images.py [--reps 5] [--no-host] [--out profiles/images.json]

Per case (a seeded random RGB photograph of the size named, resized as loadCam would): one gsrast.images.camera_images call.  Recorded: the time of
the whole call on an image that is already on the device and on a numpy image on the host (pageable memory: the call then includes the
host-to-device copy), HIP events and a host clock around a synchronise respectively; kernel time per kernel and launches from the profiler, in a
run of its own; host synchronisations from torch's sync debug mode (on the device-resident image); the scratch bytes.  The output is compared with
the host's bytes once per case.  Baseline: PILtoTorch as the reference runs it -- Image.resize and the division by 255 on the host, measured in
full -- with the host's core count and Pillow's version; where Pillow does not import, the numpy restatement of tests/images_truth.py is timed
instead and labelled so.  No ratio is asserted."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsrast  # noqa: E402
from gsrast import images  # noqa: E402

CASES = ((5472, 3648), (4000, 3000), (1920, 1080))


def timed_events(fn, reps):
    ms = []
    for _ in range(reps + 1):                             # the first repetition warms the shapes up
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); out = fn(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms[1:], out


def timed_host(fn, reps, sync=True):
    ms = []
    for _ in range(reps + 1):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
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


def host_pillow(img, size):
    from PIL import Image
    pil = Image.fromarray(img)

    def piltotorch():
        resized = torch.from_numpy(np.array(pil.resize(size))) / 255.0
        return resized.permute(2, 0, 1)
    return piltotorch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "images.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    rows = []
    for w, h in CASES:
        size = images.load_resolution(w, h, 1.0)
        img = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        d = torch.from_numpy(img).to(dev)
        on_device = lambda: images.camera_images(d, size)
        from_host = lambda: images.camera_images(img, size, device=dev)
        ms_dev, out = timed_events(on_device, a.reps)
        ms_host_in, _ = timed_host(from_host, a.reps)
        ms_copy, _ = timed_host(lambda: torch.from_numpy(img).to(dev), a.reps)
        launches, per = profile_kernels(on_device)
        syncs = count_syncs(on_device)
        row = dict(input=[w, h], output=list(size), channels=3, input_bytes=int(img.nbytes), output_bytes=int(4 * 4 * size[0] * size[1]),
                   device=dict(call_ms_image_on_device=[round(x, 3) for x in ms_dev], call_ms_image_on_device_median=round(float(np.median(ms_dev)), 3),
                               call_ms_image_on_host=[round(x, 3) for x in ms_host_in], call_ms_image_on_host_median=round(float(np.median(ms_host_in)), 3),
                               host_to_device_copy_alone_ms_median=round(float(np.median(ms_copy)), 3),
                               kernel_launches=launches, kernel_ms=round(sum(per.values()) / 1e3, 4), kernel_us={k: round(v, 1) for k, v in sorted(per.items())},
                               host_synchronisations=syncs, scratch_bytes=int(gsrast.lib().gsr_image_resample_scratch_bytes(w, h, 3, size[0], size[1]))))
        if not a.no_host:
            if pillow:
                fn = host_pillow(img, size)
                ms, ref = timed_host(fn, min(a.reps, 3), sync=False)
                row["host"] = dict(kind="PILtoTorch: PIL.Image.resize (bicubic) + torch.from_numpy / 255.0, measured in full", ms=[round(x, 2) for x in ms],
                                   ms_median=round(float(np.median(ms)), 2))
                row["device_equals_host_bytes"] = bool(torch.equal(out[0].cpu(), ref.contiguous()))
            else:
                import images_truth
                ms, ref = timed_host(lambda: images_truth.pil_to_torch(img, size), 1, sync=False)
                row["host"] = dict(kind="NOT Pillow (it does not import here): the numpy restatement tests/images_truth.py, measured in full", ms=[round(x, 2) for x in ms],
                                   ms_median=round(float(np.median(ms)), 2))
                row["device_equals_host_bytes"] = bool(np.array_equal(out[0].cpu().numpy(), ref))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d
    doc = dict(device=torch.cuda.get_device_name(0),
               timing="one gsrast.images.camera_images call (original_image, gray_image) per row, ms: HIP events for the image on the device, a host clock around "
                      "a synchronise for the numpy image on the host (pageable memory, copy included) and for the host baseline",
               host_cores=os.cpu_count(), host_cores_usable=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(), pillow_version=pillow, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
