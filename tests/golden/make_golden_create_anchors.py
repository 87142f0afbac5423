"""Golden vectors of the first anchors, produced by RUNNING the reference's own OctreeGaussian.create_from_data and ScaffoldGaussian.create_from_data
(torch / numpy, CPU).

    python tests/golden/make_golden_create_anchors.py <reference checkout>     # writes tests/golden/ref_create_anchors_*.npz

Pinned: gssr/gaussian/octree_gaussian.py:152-172 set_level, :174-182 octree_sample, :203-214 weed_out, :216-253 create_from_data;
gssr/gaussian/scaffold_gaussian.py:257-260 voxelize_sample, :262-298 create_from_data.  The technique is make_golden_anchor_octree.py's: absent packages
become inert MagicMock stand-ins and the hard-coded device="cuda" is redirected to the CPU.  distCUDA2 (a CUDA extension, absent) is replaced by its
published semantics, the mean squared distance to the three nearest neighbours by brute force (tests/glue_truth.dist2_bruteforce, which
tests/test_gpu_knn_edges.py holds the device kernel to bit for bit).  all_dist, a local of set_level, is caught as the argument of its last
torch.quantile call; every weed_out call is recorded with its positions before and after.

ATen's CPU lerp depends on the dispatch level: the AVX2 / AVX512 kernels evaluate fma(w, b - a, a), the DEFAULT level evaluates Lerp.h's
a + w * (b - a) operation by operation (8 of 700 random torch.quantile calls differ in the last bit).  The project pins the unfused form, so the
generator runs the reference at the DEFAULT level.

The files hold arrays only: the cloud, the camera centres per resolution scale, the configuration scalars, and what the reference left behind.

Margins that keep exact equality honest (asserted; the cameras are redrawn by seed until they hold): every (position, camera) pred of a weed-out lies at
least 1e-5 from its rounding boundary; no visible / C lies within 1e-5 of the threshold in force (the pass at threshold 0 decides count > 0, which
no rounding can move); the float32 torch.mean that fixes the threshold lies
within 1e-6 of the exact mean; the level count and base_layer are rounded from values at least 1e-3 from a half.
"""
import importlib
import math
import os

os.environ["ATEN_CPU_CAPABILITY"] = "default"      # before torch loads: ATen's scalar kernels, where lerp is Lerp.h operation by operation (see below)
import sys
import types
import warnings
from unittest import mock

import numpy as np
import torch

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : glue_truth
import glue_truth  # noqa: E402


def ref_import(name):
    while True:
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            if e.name.startswith("gssr"):
                raise
            sys.modules[e.name] = mock.MagicMock()
            for k in [k for k in sys.modules if k.startswith("gssr")]:
                del sys.modules[k]


ref_import("gssr.configs.method_config")
mod = ref_import("gssr.gaussian.octree_gaussian")
mod_s = sys.modules["gssr.gaussian.scaffold_gaussian"]


def _cpu(fn):
    return lambda *a, **k: fn(*a, **{kk: ("cpu" if kk == "device" and isinstance(v, str) and v.startswith("cuda") else v) for kk, v in k.items()})


for _n in ("zeros", "ones", "zeros_like", "ones_like", "tensor", "arange", "empty"):
    setattr(torch, _n, _cpu(getattr(torch, _n)))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.empty_cache = lambda: None


def _dist2(points):
    return torch.tensor(glue_truth.dist2_bruteforce(points.detach().numpy()))


mod.distCUDA2 = _dist2
mod_s.distCUDA2 = _dist2
MODES = ("floor", "round", "ceil")


class Redraw(Exception):
    pass


def cloud(r, n, lo, hi):
    """A wavy surface inside the box [lo, hi]^3 with a few exact duplicates."""
    p = r.uniform(0.0, 1.0, (n, 2))
    z = 0.5 + 0.2 * np.sin(5.0 * p[:, 0]) * np.cos(4.0 * p[:, 1])
    pts = lo + (hi - lo) * np.concatenate([p, z[:, None]], 1)
    pts[-5:] = pts[:5]
    return pts


def camera_sets(r, scales, n_per, focus, near, far):
    out = {}
    for s, n in zip(scales, n_per):
        d = np.exp(r.uniform(np.log(near), np.log(far), n))
        v = r.normal(size=(n, 3)); v[:, 2] = np.abs(v[:, 2]) + 0.3
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        out[s] = (focus + v * d[:, None]).astype(np.float32)
    return out


def octree_case(name, seed, cam_seed, *, n, lo, hi, scales, n_per, near, far, mode, fork, levels, init_level, base_layer, vthr, dist_ratio=0.999):
    r = np.random.default_rng(seed)
    pts = cloud(r, n, lo, hi).astype(np.float32)
    cams = camera_sets(np.random.default_rng(cam_seed), scales, n_per, np.full(3, 0.5 * (lo + hi)), near, far)
    cfg = mod.OctreeGaussianConfig(); cfg.fork = fork; cfg.dist2level = mode; cfg.levels = levels; cfg.init_level = init_level
    cfg.base_layer = base_layer; cfg.visible_threshold = vthr; cfg.dist_ratio = dist_ratio; cfg.sampling_ratio = 1; cfg.n_offsets = 4; cfg.feat_dim = 8
    g = mod.OctreeGaussian(cfg, device="cpu")
    cameras = {s: [types.SimpleNamespace(camera_center=torch.tensor(c)) for c in cams[s]] for s in scales}
    C = sum(n_per)

    caught = {}
    quant = torch.quantile

    def recording_quantile(x, q, *a, **k):
        caught["last"] = x.detach().numpy().copy()
        return quant(x, q, *a, **k)

    calls = []
    weed = g.weed_out
    bound = {"floor": 0.0, "round": 0.5, "ceil": 0.0}[mode]

    def recording_weed_out(pos, lv):
        thr = float(g.visible_threshold)
        out = weed(pos, lv)
        d = torch.sqrt(((pos.double()[:, None, :] - g.cam_infos[None, :, :3].double()) ** 2).sum(-1)) * g.cam_infos[None, :, 3].double()
        pred = torch.log2(float(g.standard_dist) / d) / math.log2(fork)
        if float((torch.abs(pred - bound - torch.round(pred - bound))).min()) < 1e-5:
            raise Redraw("a pred within 1e-5 of its rounding boundary")
        il = {"floor": torch.floor, "round": torch.round, "ceil": torch.ceil}[mode](pred).clamp(0, g.levels - 1)
        vis = (lv.double()[:, None] <= il).sum(1)
        if thr != 0.0 and float(torch.abs(vis / C - thr).min()) < 1e-5:          # at threshold 0 the decision is count > 0, exact in any precision
            raise Redraw("a visible fraction within 1e-5 of the threshold")
        assert torch.equal(vis / C > thr, out[3]), "the float64 chain decides as the reference did"
        if abs(float(out[2]) - float(vis.sum()) / (pos.shape[0] * C)) > 1e-6:
            raise Redraw("the float32 mean strays from the exact mean")
        calls.append((pos.numpy().copy(), lv.numpy().copy(), out[0].numpy().copy(), out[1].numpy().copy(), float(out[2])))
        return out

    g.weed_out = recording_weed_out
    torch.quantile = recording_quantile
    try:
        with torch.no_grad():
            g.create_from_data(types.SimpleNamespace(points=pts.copy()), cameras, 1.0)
    finally:
        torch.quantile = quant
    all_dist = caught["last"]
    assert all_dist.shape == (2 * C,)
    dmax, dmin = float(quant(torch.tensor(all_dist), dist_ratio)), float(quant(torch.tensor(all_dist), 1 - dist_ratio))
    for x in (math.log2(dmax / dmin) / math.log2(fork), math.log2((float(pts.max()) * g.extend - float(pts.min()) * g.extend) / 0.02)):
        if abs(abs(x - math.floor(x)) - 0.5) < 1e-3:
            raise Redraw("levels or base_layer rounded from a value near a half")
    assert len(calls) == (2 if vthr < 0 else 1)
    assert float(g.init_pos[0]) > pts.min() or pts.min() <= 0, "a positive minimum puts init_pos above the cloud: negative keys"
    out = {"points": pts, "scales": np.array(scales, np.float64), "dist_ratio": dist_ratio, "fork": fork, "extend": float(g.extend),
           "dist2level": MODES.index(mode), "cfg_levels": levels, "cfg_init_level": init_level, "cfg_base_layer": base_layer, "cfg_visible_threshold": float(vthr),
           "n_offsets": 4, "feat_dim": 8, "cam_infos": g.cam_infos.numpy(), "all_dist": all_dist, "standard_dist": np.float32(g.standard_dist),
           "levels": int(g.levels), "init_level": int(g.init_level), "base_layer": int(g.base_layer), "voxel_size": g.voxel_size.numpy(),
           "init_pos": g.init_pos.numpy(), "positions0": calls[0][0], "level0": calls[0][1], "visible_threshold": np.float64(float(g.visible_threshold)),
           "anchor": g._anchor.detach().numpy(), "level": g._level.numpy(), "scaling": g._scaling.detach().numpy()}
    for i, s in enumerate(scales):
        out[f"centres_{i}"] = cams[s]
    if vthr < 0:
        out["positions1"], out["level1"] = calls[0][2], calls[0][3]
    assert out["voxel_size"].dtype == np.float32 and out["voxel_size"].shape == () and out["level"].dtype == np.int32
    assert np.array_equal(calls[-1][2], out["anchor"]) and out["level"].shape == (out["anchor"].shape[0], 1)
    neg = bool((np.round((pts - out["init_pos"]) / out["voxel_size"]) < 0).any())
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}: {os.path.getsize(path) // 1024} KiB, N {n} C {C} levels {out['levels']} init_level {out['init_level']} base_layer {out['base_layer']} "
          f"voxel_size {float(out['voxel_size']):.5f} cells {calls[0][0].shape[0]} -> {out['anchor'].shape[0]} threshold {float(g.visible_threshold):.6f} negative keys {neg}")
    return neg


def scaffold_case(name, seed, *, n, lo, hi, dtype, voxel_size):
    r = np.random.default_rng(seed)
    np.random.seed(seed)                               # the reference shuffles with numpy's global generator
    pts = cloud(r, n, lo, hi).astype(dtype)
    cfg = mod_s.ScaffoldGaussianConfig(); cfg.voxel_size = voxel_size; cfg.sampling_ratio = 1; cfg.n_offsets = 4; cfg.feat_dim = 8
    g = mod_s.ScaffoldGaussian(cfg, device="cpu")
    given = pts.copy()
    with torch.no_grad():
        g.create_from_data(types.SimpleNamespace(points=given), {}, 1.0)
    assert not np.array_equal(given, pts) and np.array_equal(np.sort(given, axis=0), np.sort(pts, axis=0)), "the reference shuffled its input in place"
    anchor = g._anchor.detach().numpy()
    assert anchor.dtype == np.float32 and 1 < anchor.shape[0] < n
    path = os.path.join(HERE, name)
    np.savez_compressed(path, points=pts, cfg_voxel_size=np.float64(voxel_size), voxel_size=np.float64(g.voxel_size), anchor=anchor,
                        scaling=g._scaling.detach().numpy(), n_offsets=4, feat_dim=8)
    print(f"wrote {name}: {os.path.getsize(path) // 1024} KiB, {pts.dtype} N {n} voxel_size {g.voxel_size:.6g} -> {anchor.shape[0]} anchors")


def case(name, seed, **kw):
    for cam_seed in range(100 * seed, 100 * seed + 60):
        try:
            return octree_case(name, seed, cam_seed, **kw)
        except Redraw as e:
            print(f"{name}: cameras of seed {cam_seed} redrawn: {e}")
    raise SystemExit(f"{name}: no camera seed holds the margins")


if __name__ == "__main__":
    # round, fork 2, everything adaptive, a cloud with a positive minimum (init_pos = 1.1 * min lies above it: negative keys)
    neg = case("ref_create_anchors_octree_round.npz", 31, n=420, lo=0.6, hi=2.2, scales=(1.0,), n_per=(9,), near=0.4, far=5.0, mode="round", fork=2,
               levels=-1, init_level=-1, base_layer=-1, vthr=-1)
    assert neg
    # floor, fork 3, levels / init_level / base_layer / threshold given, two resolution scales, a cloud around the origin
    case("ref_create_anchors_octree_floor_fork3.npz", 32, n=400, lo=-1.0, hi=0.8, scales=(1.0, 2.0), n_per=(6, 4), near=0.5, far=5.0, mode="floor", fork=3,
         levels=4, init_level=1, base_layer=3, vthr=0.25)
    # ceil, fork 2, adaptive levels with the threshold fixed by the first weed-out, two scales
    case("ref_create_anchors_octree_ceil.npz", 33, n=380, lo=-0.7, hi=1.1, scales=(1.0, 4.0), n_per=(5, 5), near=0.4, far=6.0, mode="ceil", fork=2,
         levels=-1, init_level=-1, base_layer=-1, vthr=-1)
    scaffold_case("ref_create_anchors_scaffold_f32.npz", 41, n=900, lo=-1.0, hi=1.0, dtype=np.float32, voxel_size=0.05)
    scaffold_case("ref_create_anchors_scaffold_f32_median.npz", 42, n=900, lo=-1.0, hi=1.0, dtype=np.float32, voxel_size=-1.0)
    scaffold_case("ref_create_anchors_scaffold_f64.npz", 43, n=900, lo=0.3, hi=2.0, dtype=np.float64, voxel_size=0.04)
    scaffold_case("ref_create_anchors_scaffold_f64_median.npz", 44, n=900, lo=-1.0, hi=1.0, dtype=np.float64, voxel_size=0.0)
