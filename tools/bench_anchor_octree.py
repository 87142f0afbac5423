"""One OctreeGaussian.adjust_anchor call on the device: gsrast.anchors.octree_adjust_anchor_ against the torch restatement with the reference's per-camera loop.

    python tools/bench_anchor_octree.py [--sizes 100000 300000] [--cameras 300] [--out profiles/anchor_adjust_octree.json]

The torch chain is tests/ref_anchor_octree_torch.adjust run on the device, with its vectorised weed-out replaced by the loop of
gssr/gaussian/octree_gaussian.py:203-214 (per camera: distance, log2, rounding, clamp, compare, add -- about eight launches).  It is kinder than the reference
in two ways: cells are matched by sort + searchsorted instead of the all-pairs comparison in chunks of 4096, and it computes the new rows and the pruned
accumulators but performs no surgery on the parameters or the optimizer.  Inputs: anchors of 6 levels on the octree lattice of a box (k = 10 offsets, 32
features), 300 cameras at log-spread distances around it, statistics with candidates at every level.  Times are HIP-event times of one whole call (host
synchronisations included), clocks warmed, each path warmed once on the same shape; launches are counted by the torch profiler, host synchronisations by torch's
sync debug mode, each in a run of its own (tools/bench_anchor.py's helpers).  Prints and writes JSON."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
import ref_anchor_octree_torch as R   # noqa: E402
from bench_anchor import count_launches, count_syncs, timed, warm_clocks   # noqa: E402
from gsrast import anchors   # noqa: E402
from gsrast.optim import Adam   # noqa: E402

NAMES, ACCS = R.NAMES, R.ACCS
K, F, LEVELS, FORK, VS = 10, 32, 6, 2, 0.64
MODES = ("floor", "round", "ceil")


def scene(N, C, seed=0):
    r = np.random.default_rng(seed)
    init_pos = np.array([-3.3, 0.7, 11.0], np.float32)
    lvl = r.integers(0, LEVELS, N).astype(np.int32)
    size = (np.float32(VS) / np.float32(2.0) ** lvl.astype(np.float32)).astype(np.float32)
    side = max(4, int(round((N / LEVELS * 6) ** (1 / 3))))
    anchor = (np.round(r.uniform(0, side, (N, 3))) * size[:, None] + init_pos).astype(np.float32)
    scaling = (r.uniform(0.5, 3.0, (N, 6)) * size[:, None]).astype(np.float32)
    denom = r.integers(0, 100, (N * K, 1)).astype(np.float32)
    demon = r.integers(0, 121, (N, 1)).astype(np.float32)
    lo, hi = anchor.min(0), anchor.max(0)
    extent = float(np.linalg.norm(hi - lo))
    v = r.normal(size=(C, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = np.exp(r.uniform(np.log(0.6 * extent), np.log(20.0 * extent), C))
    cams = np.concatenate([(lo + hi) / 2 + v * d[:, None], np.ones((C, 1))], 1).astype(np.float32)
    fx = {"k": K, "levels": LEVELS, "fork": FORK, "voxel_size": np.float32(VS), "init_pos": init_pos, "standard_dist": np.float32(16.0 * extent),
          "visible_threshold": 0.3, "dist2level": 1, "progressive": 0, "iteration": 3000, "coarse_intervals": np.array([0.0]), "cam_infos": cams,
          "scaling_act": scaling, "in_level": lvl.reshape(-1, 1), "in_extra_level": np.zeros(N, np.float32), "in_anchor": anchor,
          "in_offset": r.uniform(-1, 1, (N, K, 3)).astype(np.float32), "in_anchor_feat": r.normal(0, 1, (N, F)).astype(np.float32),
          "in_opacity": r.normal(0, 1, (N, 1)).astype(np.float32), "in_scaling": np.log(scaling), "in_rotation": r.normal(0, 1, (N, 4)).astype(np.float32),
          "in_offset_denom": denom, "in_offset_gradient_accum": (denom * np.exp(r.normal(math.log(4e-4), 1.0, (N * K, 1)))).astype(np.float32),
          "in_anchor_demon": demon, "in_opacity_accum": (demon * r.uniform(0.0, 0.02, (N, 1))).astype(np.float32)}
    return fx


class Model:
    pass


def make_model(fx, dev):
    t = lambda x: torch.tensor(x, device=dev)
    m = Model()
    for n in NAMES:
        setattr(m, "_" + n, torch.nn.Parameter(t(fx["in_" + n])))
    for n in ACCS:
        setattr(m, n, t(fx["in_" + n]))
    m.get_scaling = t(fx["scaling_act"])
    m.n_offsets, m.levels, m.fork = K, LEVELS, FORK
    m.voxel_size, m.init_pos, m.standard_dist = t(fx["voxel_size"]), t(fx["init_pos"]), t(fx["standard_dist"])
    m.cam_infos, m.visible_threshold, m.dist2level, m.progressive, m.coarse_intervals = t(fx["cam_infos"]), fx["visible_threshold"], "round", False, []
    m._level, m._extra_level = t(fx["in_level"]), t(fx["in_extra_level"])
    m.optimizer = Adam([{"params": [getattr(m, "_" + n)], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        q = getattr(m, "_" + n)
        m.optimizer.state[q] = {"step": torch.tensor(1.0), "exp_avg": torch.full_like(q, 0.01), "exp_avg_sq": torch.full_like(q, 1e-4)}
    return m


def weed_out_per_camera(positions, levels_of, cam_infos, standard_dist, fork, levels, dist2level, visible_threshold, dtype=None):
    """The reference's loop (octree_gaussian.py:203-214)."""
    fn = {"floor": torch.floor, "round": torch.round, "ceil": torch.ceil}[dist2level]
    count = torch.zeros(positions.shape[0], dtype=torch.int, device=positions.device)
    for cam in cam_infos:
        dist = torch.sqrt(torch.sum((positions - cam[:3]) ** 2, dim=1)) * cam[3]
        pred = torch.log2(standard_dist / dist) / math.log2(fork)
        count += (levels_of <= torch.clamp(fn(pred).int(), min=0, max=levels - 1)).int()
    return count, count / len(cam_infos) > visible_threshold


def torch_chain(fx_dev):
    out = R.adjust(fx_dev)
    return int(out["keep"].sum()) + out["new_anchor"].shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 300000])
    ap.add_argument("--cameras", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_adjust_octree.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anchor_octree.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    R.weed_out = weed_out_per_camera
    res = {"device": torch.cuda.get_device_name(0), "k": K, "feat_dim": F, "levels": LEVELS, "cameras": a.cameras, "voxel_size": VS,
           "timing": "HIP events around one whole call, ms", "sizes": []}
    warm_clocks(dev)
    for N in a.sizes:
        fx = scene(N, a.cameras)
        row = {"Na": N}
        scalars = ("k", "levels", "fork", "voxel_size", "standard_dist", "visible_threshold", "dist2level", "progressive", "iteration", "coarse_intervals", "init_pos")
        for tag, fn, build, reps in (
                ("hip", lambda m: anchors.octree_adjust_anchor_(m, 3000), lambda: make_model(fx, dev), a.reps),
                ("torch_chain", torch_chain, lambda: {n: (torch.tensor(x) if n in scalars else torch.tensor(x, device=dev)) for n, x in fx.items()}, a.torch_reps)):
            ms, n_out = timed(fn, build, reps)
            ent = {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "anchors_after": int(n_out)}
            try:
                ent["kernel_launches"] = count_launches(fn, build)
            except Exception as e:                                # the profiler is optional equipment
                ent["kernel_launches"] = f"not measured ({type(e).__name__})"
            try:
                ent["host_synchronisations"] = count_syncs(fn, build)
            except Exception as e:
                ent["host_synchronisations"] = f"not measured ({type(e).__name__})"
            row[tag] = ent
            print(json.dumps({"Na": N, tag: ent}), flush=True)
        row["ratio"] = round(row["torch_chain"]["ms_median"] / row["hip"]["ms_median"], 1)
        res["sizes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
