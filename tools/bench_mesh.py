"""Mesh extraction from the block-sparse TSDF volume (ScalableTSDFVolume.extract_triangle_mesh) on the volume tools/bench_tsdf_sparse.py builds: its twelve
smooth 1920x1080 frames at the reference's default resolution (voxel = depth_trunc / 1024, sdf_trunc = 5 voxels).  HIP-event times of the count pass
(with its scan and the read-back of the two totals), of the emit pass and of the whole call (sort of the unit keys and allocations included), GB/s on
the algorithmic bytes -- the tsdf and weight planes of every unit once per pass, plus the three output arrays -- and, beside it, what the only path
without this method costs for the same volume: units() and the copy of its arrays to the host, in front of a CPU marching cubes that is not counted.
Writes profiles/mesh_extract.json and prints it as one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
from gsrast.tsdf import ScalableTSDFVolume      # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); t0 = time.perf_counter(); e0.record()
    out = fn()
    e1.record(); torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)


def main():
    W, H = 1920, 1080
    depth_trunc = 8.0
    vl = depth_trunc / 1024
    vol = ScalableTSDFVolume(vl, 5 * vl, capacity_units=1 << 17)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    f = 0.8 * W
    for k in range(12):
        depth = (4.0 + 0.4 * np.sin(u / 160.0 + 0.3 * k) + 0.3 * np.cos(v / 120.0)).astype(np.float32)[None]
        rgb = np.random.default_rng(k).uniform(0, 1, (3, H, W)).astype(np.float32)
        E = np.eye(4, dtype=np.float32); E[0, 3] = 0.03 * k
        vol.integrate(torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda(), f, f, W / 2, H / 2, E, depth_trunc=depth_trunc)
    n = vol.num_units
    reps = 5
    count_ms, emit_ms, call_ms, call_wall = [], [], [], []
    for i in range(reps + 1):
        (nn, order, scratch, V, T), c_ms, _ = timed(lambda: vol._mesh_count(0.0))
        mesh, e_ms, _ = timed(lambda: vol._mesh_emit(nn, order, scratch, V, T, 0.0))
        del mesh, order, scratch
        mesh, a_ms, a_wall = timed(lambda: vol.extract_triangle_mesh())
        if i:          # the first round warms the allocator up
            count_ms.append(c_ms); emit_ms.append(e_ms); call_ms.append(a_ms); call_wall.append(a_wall)
    V, T = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    del mesh
    planes = n * 2 * 4096 * 4                          # tsdf + weight plane of every unit
    outputs = V * 24 + T * 12
    cm, em, am = float(np.median(count_ms)), float(np.median(emit_ms)), float(np.median(call_ms))

    def old_path():
        return [x.cpu() for x in vol.units()]
    arrays, _, old_wall = timed(old_path)
    old_bytes = sum(a.numel() * a.element_size() for a in arrays)
    del arrays
    res = {"what": "ScalableTSDFVolume.extract_triangle_mesh on the volume of tools/bench_tsdf_sparse.py (12 smooth 1920x1080 frames, voxel 7.8 mm, sdf_trunc 5 voxels)",
           "units": n, "vertices": V, "triangles": T,
           "count_pass_ms_gpu_events": round(cm, 3), "emit_pass_ms_gpu_events": round(em, 3), "whole_call_ms_gpu_events": round(am, 3),
           "whole_call_ms_wall": round(float(np.median(call_wall)), 3),
           "algorithmic_bytes_count": planes, "algorithmic_bytes_emit": planes + outputs,
           "count_pass_GBps": round(planes / (cm * 1e-3) / 1e9, 1), "emit_pass_GBps": round((planes + outputs) / (em * 1e-3) / 1e9, 1),
           "whole_call_GBps": round((2 * planes + outputs) / (am * 1e-3) / 1e9, 1),
           "scratch_bytes_per_unit": round(int(__import__("gsrast").lib().gsr_tsdf_sparse_mesh_scratch_bytes(n)) / n, 1),
           "units_plus_host_copy_ms_wall": round(old_wall, 1), "units_plus_host_copy_bytes": old_bytes,
           "note": "medians of 5 after one warm-up round; count pass = count kernel + scan + 16-byte read-back, whole call = finish() + key sort + both passes + "
                   "allocations; algorithmic bytes = the tsdf and weight planes of every unit once per pass plus the outputs (an emit pass skips units "
                   "without a vertex or triangle, so its GB/s on these bytes overstates what it moves); units() + host copy is a LOWER bound of the only "
                   "path without this method (a CPU marching cubes would follow) and it materialises the pools, so it runs last"}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_extract.json"), "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
