"""One densify_and_prune call on the device: gsrast.densify.densify_and_prune_ against the reference-shaped torch chain, same device, same inputs.

    python tools/bench_densify.py [--sizes 300000 1000000 3000000] [--out profiles/densify.json]

The torch chain is tests/ref_densify_torch.chain run on the device and installed into the model the way the reference does it: the clones are
appended with one cat per tensor, the children with another, the split parents and then the pruned rows are dropped with one boolean gather per
tensor, over 6 parameters and 12 Adam moments.  It is the baseline; the code under test never is.  Inputs: tests/densify_cases.make_inputs at SH
degree 3 (15 rest coefficients), about 10 % cloned, 10 % split, 5 % pruned.  Times are HIP-event times of one whole call (host synchronisations
included), clocks warmed, each path warmed once on the same shape; launches and per-kernel device times come from the torch profiler, host
synchronisations from torch's sync debug mode, peak memory from the caching allocator's statistics, each in a run of its own.  The copy kernel
(the row mover, k_rows_move) is reported with its algorithmic rate: the bytes it must read and write over its device time.  Prints and writes JSON."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
import densify_cases as DC          # noqa: E402
import ref_densify_torch as R       # noqa: E402
import gsrast                # noqa: E402
from gsrast import densify   # noqa: E402

HBM = 8.0e12
RULES = dict(DC.RULES, max_screen_size=20)


def hip_call(m):
    return densify.densify_and_prune_(m, RULES["max_grad"], RULES["min_opacity"], RULES["extent"], RULES["max_screen_size"], generator=m.generator)


@torch.no_grad()
def torch_call(m):
    """The reference-shaped chain, installed into the model and its optimizer."""
    st, mo, stats = R.chain(m.tensors(), m.moments(), m.xyz_gradient_accum, m.denom, torch.exp, torch.sigmoid, m.max_radii2D, z_split=None,
                            generator=m.generator, **RULES)
    for g in m.optimizer.param_groups:
        k = g["name"]
        old = g["params"][0]
        s = m.optimizer.state.pop(old)
        s["exp_avg"], s["exp_avg_sq"] = mo[k]
        new = torch.nn.Parameter(st[k].requires_grad_(True))
        g["params"][0] = new
        m.optimizer.state[new] = s
        setattr(m, DC.ATTRS[k], new)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = stats["accum"], stats["denom"], stats["radii"]
    return m._xyz.shape[0]


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


def timed(fn, build, reps):
    ms = []
    for _ in range(reps + 1):                                    # the first repetition is the warm-up of this shape
        m = build()
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); n = fn(m); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
        del m
    return ms[1:], n


def profile_kernels(fn, build):
    """-> (launches, {kernel name: device microseconds})."""
    from torch.profiler import ProfilerActivity, profile
    m = build()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(m)
        torch.cuda.synchronize()
    n, per = 0, {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            n += 1
            try:
                us = e.time_range.elapsed_us()                   # a device event's own span
            except Exception:
                us = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)
            per[e.name] = per.get(e.name, 0.0) + float(us)
    return n, per


def count_syncs(fn, build):
    m = build()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(m)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower())


def peak_memory(fn, build):
    """Bytes: allocated before the call (the inputs), the peak during it, and what the model holds afterwards."""
    m = build()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(m)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return before, peak, m


def tensor_bytes(m):
    n = sum(t.numel() * 4 for t in m.tensors().values()) + sum(t.numel() * 4 for pair in m.moments().values() for t in pair)
    return n + sum(getattr(m, k).numel() * 4 for k in ("xyz_gradient_accum", "denom", "max_radii2D"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[300000, 1000000, 3000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "sh_rest": 15, "timing": "HIP events around one whole call, ms", "hbm_bytes_per_s": HBM, "sizes": []}
    warm_clocks(dev)
    for P in a.sizes:
        p, mom, stats = DC.make_inputs(P, seed=P % 997, rest=15, device=dev)
        row = {"P": P}

        def build(cls):
            m = DC.Model(p, mom, stats, dev, optimizer=cls)
            m.generator = torch.Generator(device=dev); m.generator.manual_seed(1)
            return m
        for tag, fn, cls in (("hip", hip_call, "gsrast"), ("torch_chain", torch_call, "torch")):
            b = lambda: build(cls)
            ms, n_out = timed(fn, b, a.reps)
            ent = {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "rows_after": int(n_out)}
            try:
                ent["kernel_launches"], per = profile_kernels(fn, b)
                if tag == "hip":
                    ent["kernel_us"] = {k: round(v, 1) for k, v in per.items() if "k_den_" in k or "k_rows_move" in k}
            except Exception as e:                                # the profiler is optional equipment
                ent["kernel_launches"] = f"not measured ({type(e).__name__})"
            try:
                ent["host_synchronisations"] = count_syncs(fn, b)
            except Exception as e:
                ent["host_synchronisations"] = f"not measured ({type(e).__name__})"
            before, peak, m = peak_memory(fn, b)
            ent["bytes_inputs"], ent["bytes_peak"], ent["bytes_outputs"] = before, peak, tensor_bytes(m)
            if tag == "hip":
                rows = m._xyz.shape[0]
                ent["bytes_scratch"] = int(gsrast.lib().gsr_densify_plan_scratch_bytes(P, 2)) + 32
                ent["bytes_activated_and_noise"] = P * 16 + 2 * P * 12            # get_scaling + get_opacity, and an upper bound of the draws
                ent["peak_within_inputs_outputs_scratch"] = bool(peak <= before + ent["bytes_outputs"] + ent["bytes_scratch"] + ent["bytes_activated_and_noise"] + (1 << 20))
                # algorithmic bytes of the copy: every output row written once; a parameter row read once, a moment row read only where it is carried
                ent["row_bytes_params"] = sum(v.numel() // max(rows, 1) * 4 for v in m.tensors().values())
            del m
            row[tag] = ent
            print(json.dumps({"P": P, tag: ent}), flush=True)
        # the copy kernel's algorithmic bytes -- parameters: read + write every output row; moments: read the carried rows, write all
        m = build("gsrast")
        _, split, prune_self, _ = R.classify(m.xyz_gradient_accum, m.denom, m.get_scaling.detach(), m.get_opacity.detach(), m.max_radii2D, **RULES)
        n_o = int((~split & ~prune_self).sum())
        del m
        rb, rows = row["hip"]["row_bytes_params"], row["hip"]["rows_after"]
        bytes_emit = rb * (rows + rows) + 2 * rb * (n_o + rows)
        us_emit = sum(v for k, v in row["hip"].get("kernel_us", {}).items() if "k_rows_move" in k)
        cmp_ = {"rows_carried": n_o, "emit_us": round(us_emit, 1), "emit_bytes": bytes_emit}
        if us_emit > 0:
            cmp_["emit_TBps"] = round(bytes_emit / us_emit / 1e6, 3)
            cmp_["emit_hbm_fraction"] = round(bytes_emit / (us_emit * 1e-6) / HBM, 3)
        cmp_["call_hbm_fraction"] = round(bytes_emit / (row["hip"]["ms_median"] * 1e-3) / HBM, 3)
        row["copy_kernel"] = cmp_
        row["speedup"] = round(row["torch_chain"]["ms_median"] / row["hip"]["ms_median"], 2)
        row["not_slower_than_chain"] = bool(row["hip"]["ms_median"] <= row["torch_chain"]["ms_median"])
        print(json.dumps({"P": P, "copy_kernel": row["copy_kernel"], "speedup": row["speedup"]}), flush=True)
        res["sizes"].append(row)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
