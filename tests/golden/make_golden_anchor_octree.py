"""Golden vectors of the Octree-GS anchor growing + pruning, produced by RUNNING the reference's own OctreeGaussian.adjust_anchor (torch, CPU).

    python tests/golden/make_golden_anchor_octree.py <reference checkout>     # writes tests/golden/ref_anchor_octree_*.npz

Pinned: gssr/gaussian/octree_gaussian.py:536-588 adjust_anchor, :401-534 anchor_growing, :203-214 weed_out, :184-201 map_to_int_level, :374-385
get_remove_duplicates, and the optimizer surgery it inherits (scaffold_gaussian.py:460-484, :510-541), called on the reference's own model object
with a real torch.optim.Adam (one named group per tensor, lr = 0, stepped once so that moments exist).  The technique is make_golden_anchor.py's:
absent packages become inert MagicMock stand-ins, the hard-coded device="cuda" is redirected to the CPU, and torch_scatter (third-party, absent)
is replaced by its published semantics: scatter_max(src, index, dim=0)[0] = zeros(U, F).scatter_reduce(0, index, src, "amax", include_self=False).
levels, voxel_size (0-dim float32), init_pos, standard_dist, cam_infos, visible_threshold, _level and _extra_level are set by hand, as
create_from_data would leave them.  weed_out is wrapped so that every pass's count before and after weeding is recorded.

The files hold arrays only: inputs (parameters, moments, accumulators, levels, the activated scaling as the reference computed it, cameras, the
model's scalars) and results (keep mask, counts per pass, the new rows of every parameter, _level with its dtype, _extra_level, the four
accumulators); the generator asserts that [old[keep] ; new rows] IS the reference's final state.

Margins that keep exact equality honest (asserted; the cameras are redrawn by seed until they hold): every (new position, camera) pred lies at
least 1e-5 from its rounding boundary -- the float32 and float64 chains differ by at most 3.7e-7 on such scenes and one ulp of a device log2 at
|pred| < 16 is 9.5e-7, 1e-5 is ten times their sum; no visible / C lies within 1e-6 of visible_threshold; no anchor_grads lies within 1e-6
relative of an extra threshold.
"""
import importlib
import math
import os
import sys
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
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : ref_anchor_octree_torch


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


def _cpu(fn):
    return lambda *a, **k: fn(*a, **{kk: ("cpu" if kk == "device" and isinstance(v, str) and v.startswith("cuda") else v) for kk, v in k.items()})


for _n in ("zeros", "ones", "zeros_like", "ones_like", "tensor", "arange", "empty"):
    setattr(torch, _n, _cpu(getattr(torch, _n)))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.empty_cache = lambda: None


def _scatter_max(src, index, dim=0):
    U = int(index.max()) + 1 if index.numel() else 0
    out = torch.zeros(U, src.shape[1], dtype=src.dtype).scatter_reduce(0, index, src, "amax", include_self=False)
    return out, None


mod.scatter_max = _scatter_max
NAMES = ("anchor", "offset", "anchor_feat", "opacity", "scaling", "rotation")
ACCS = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")
MODES = ("floor", "round", "ceil")


class Redraw(Exception):
    pass


def octree_anchors(r, n_pts, vs, init_pos, levels, fork, fill, empty_levels=()):
    """Anchors on the octree lattice of a wavy surface: per level the cells of the sampled points, thinned to `fill` so that free cells remain."""
    p = r.uniform(-0.6, 0.6, (n_pts, 2))
    z = 0.15 * np.sin(3.0 * p[:, 0]) * np.cos(2.0 * p[:, 1])
    pts = np.concatenate([p, z[:, None]], 1).astype(np.float32)
    pos, lvl = [], []
    for l in range(levels):
        if l in empty_levels:
            continue
        size = np.float32(vs) / np.float32(float(fork) ** l)
        c = np.unique(np.round((pts - init_pos) / size), axis=0)
        c = c[r.uniform(size=c.shape[0]) < fill[l]]
        pos.append((c * size + init_pos).astype(np.float32)); lvl.append(np.full(c.shape[0], l, np.int32))
    return np.concatenate(pos), np.concatenate(lvl)


FOCUS = np.array([0.5, 0.5, 0.0])


def cameras(r, C, near, far):
    """C cameras at log-spread distances from one corner of the scene, scales 1 (and a few 2): near ones tell the two ends of the surface apart."""
    d = np.exp(r.uniform(np.log(near), np.log(far), C))
    v = r.normal(size=(C, 3)); v[:, 2] = np.abs(v[:, 2]) + 0.3
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    s = np.where(r.uniform(size=C) < 0.25, 2.0, 1.0)
    return np.concatenate([FOCUS + v * d[:, None], s[:, None]], 1).astype(np.float32)


def run_case(name, seed, cam_seed, *, vs, k, F, n_pts, levels, fill, C, near, far, sd, vthr, mode, prune=True, empty_levels=(), still_levels=(),
             progressive=False, iteration=3000, expect=()):
    r = np.random.default_rng(seed)
    torch.manual_seed(seed)
    fork = 2
    cfg = mod.OctreeGaussianConfig(); cfg.n_offsets = k; cfg.feat_dim = F; cfg.fork = fork; cfg.levels = levels; cfg.dist2level = mode
    cfg.visible_threshold = vthr; cfg.progressive = progressive
    g = mod.OctreeGaussian(cfg, device="cpu")
    init_pos = np.array([-0.66, -0.66, -0.66], np.float32)
    anchor, lvl = octree_anchors(r, n_pts, vs, init_pos, levels, fork, fill, empty_levels)
    N = anchor.shape[0]
    size_of = (np.float32(vs) / np.float32(fork) ** lvl.astype(np.float32)).astype(np.float32)
    scaling = np.log(size_of[:, None] * r.uniform(0.8, 2.5, (N, 6))).astype(np.float32)
    offset = r.uniform(-1, 1, (N, k, 3)).astype(np.float32)
    offset[np.isin(lvl, still_levels)] = 0.0                                              # every candidate of these levels stays in its own anchor's cell
    p = {"anchor": anchor, "offset": offset, "anchor_feat": r.normal(0, 1, (N, F)).astype(np.float32),
         "opacity": r.normal(0, 1, (N, 1)).astype(np.float32), "scaling": scaling, "rotation": r.normal(0, 1, (N, 4)).astype(np.float32)}
    for nme in NAMES:
        setattr(g, "_" + nme, torch.nn.Parameter(torch.tensor(p[nme])))
    g.optimizer = torch.optim.Adam([{"params": [getattr(g, "_" + nme)], "lr": 0.0, "name": nme} for nme in NAMES], lr=0.0, eps=1e-15)
    for nme in NAMES:                                                                     # gradients from a few values: the moments compress
        getattr(g, "_" + nme).grad = torch.tensor((r.integers(-8, 9, p[nme].shape) / 64.0).astype(np.float32))
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    for nme in NAMES:
        assert np.array_equal(getattr(g, "_" + nme).detach().numpy(), p[nme]), "lr = 0: the step must leave the parameters alone"
    denom = r.integers(0, 100, (N * k, 1)).astype(np.float32)
    accum = (denom * np.exp(r.normal(np.log(3.5e-4), 0.8, (N * k, 1)))).astype(np.float32)
    demon = r.integers(0, 121 if prune else 81, (N, 1)).astype(np.float32)
    opac = (demon * r.uniform(0.0, 0.02, (N, 1))).astype(np.float32)
    a = {"opacity_accum": opac, "anchor_demon": demon, "offset_gradient_accum": accum, "offset_denom": denom}
    for nme in ACCS:
        setattr(g, nme, torch.tensor(a[nme]))
    extra0 = (r.integers(0, 4, N) * 0.25).astype(np.float32)
    cam = cameras(np.random.default_rng(cam_seed), C, near, far)
    g.levels, g.voxel_size, g.init_pos = levels, torch.tensor(vs, dtype=torch.float32), torch.tensor(init_pos)
    g.standard_dist, g.cam_infos, g.visible_threshold = torch.tensor(sd, dtype=torch.float32), torch.tensor(cam), vthr
    g._level, g._extra_level = torch.tensor(lvl).unsqueeze(1), torch.tensor(extra0)
    g.coarse_intervals = [5000.0] if progressive else []
    moments = {}
    for nme in NAMES:
        st = g.optimizer.state[getattr(g, "_" + nme)]
        moments["m_" + nme] = st["exp_avg"].numpy().copy(); moments["v_" + nme] = st["exp_avg_sq"].numpy().copy()
    scaling_act = g.get_scaling.detach().numpy().copy()

    # every weed_out call is one pass: its level, the cells before and after, and the margins of the case
    calls = []
    weed = g.weed_out
    bound = {"floor": 0.0, "round": 0.5, "ceil": 0.0}[mode]

    def recording_weed_out(pos, lv):
        out = weed(pos, lv)
        if pos.shape[0]:
            d = torch.sqrt(((pos.double()[:, None, :] - g.cam_infos[None, :, :3].double()) ** 2).sum(-1)) * g.cam_infos[None, :, 3].double()
            pred = torch.log2(float(g.standard_dist) / d) / math.log2(fork)
            if float((torch.abs(pred - bound - torch.round(pred - bound))).min()) < 1e-5:
                raise Redraw("a pred within 1e-5 of its rounding boundary")
            il = {"floor": torch.floor, "round": torch.round, "ceil": torch.ceil}[mode](pred).clamp(0, levels - 1)
            frac = (lv.double()[:, None] <= il).sum(1) / cam.shape[0]
            if float(torch.abs(frac - vthr).min()) < 1e-6:
                raise Redraw("a visible fraction within 1e-6 of the threshold")
            assert torch.equal(frac > vthr, out[3]), "the float64 chain decides as the reference did"
        calls.append((int(lv[0]) if lv.numel() else -1, pos.shape[0], int(out[3].sum())))
        return out

    g.weed_out = recording_weed_out
    with torch.no_grad():
        g.adjust_anchor(iteration=iteration)
    # which call was which pass: replay the loop's conditions over the reference's own final levels
    found, kept = np.zeros((levels, 2), np.int64), np.zeros((levels, 2), np.int64)
    grow_ds = (not progressive) or iteration > g.coarse_intervals[-1]
    gr = np.abs(np.nan_to_num(accum / np.where(denom == 0, np.nan, denom))).reshape(-1).astype(np.float32)
    seen = denom.reshape(-1) > 40.0
    gr[~seen] = 0.0
    it = iter(calls)
    uv = fork ** 0.5
    empty_calls, skipped_b = 0, 0
    for l in range(levels):
        if not (lvl == l).any():                                                          # appended anchors of level l presuppose original ones
            continue
        own = np.repeat(lvl == l, k)
        ct, dt = np.float32(0.0002 * uv ** l), np.float32(0.0002 * uv ** l * uv)
        if ((gr >= ct) & (gr < dt) & own).any():
            lv, f_, k_ = next(it)
            assert lv in (l, -1); found[l, 0], kept[l, 0] = f_, k_; empty_calls += f_ == 0
        if grow_ds and l < levels - 1 and ((gr >= dt) & own).any():
            if (lvl == l + 1).any():
                lv, f_, k_ = next(it)
                assert lv in (l + 1, -1); found[l, 1], kept[l, 1] = f_, k_; empty_calls += f_ == 0
            else:
                skipped_b += 1
    assert next(it, None) is None, "every weed_out call is accounted for"
    U = int(kept.sum())
    anchors_mask = demon > 80.0
    keep = ~((opac < np.float32(0.005) * demon) & anchors_mask).reshape(-1)
    nk = int(keep.sum())
    out = {}
    for nme in NAMES:
        fin = getattr(g, "_" + nme).detach().numpy()
        st = g.optimizer.state[getattr(g, "_" + nme)]
        assert fin.shape[0] == nk + U and np.array_equal(fin[:nk], p[nme][keep]), nme
        for key, src in (("exp_avg", moments["m_" + nme]), ("exp_avg_sq", moments["v_" + nme])):
            mv = st[key].numpy()
            assert np.array_equal(mv[:nk], src[keep]) and not mv[nk:].any() and mv.shape == fin.shape, (nme, key)
        assert float(st["step"]) == 1.0
        out["new_" + nme] = fin[nk:].copy()
    for nme in ACCS:
        out["out_" + nme] = getattr(g, nme).numpy().copy()
    out["out_level"] = g._level.numpy().copy()
    out["out_extra_level"] = g._extra_level.numpy().copy()
    assert out["out_level"].shape == (nk + U, 1) and out["out_extra_level"].shape == (nk + U,)
    assert out["out_level"].dtype == (np.float32 if U else np.int32)
    out["new_level"] = out["out_level"][nk:].astype(np.float32)
    # no anchor_grads within 1e-6 relative of an extra threshold
    ag = gr.reshape(N, k).astype(np.float64).sum(1) / (seen.reshape(N, k).sum(1) + 1e-6)
    for l in range(levels):
        et = 0.0002 * uv ** l * 4.0
        if float(np.abs(ag / et - 1.0).min()) < 1e-6:
            raise Redraw("an anchor_grads on an extra threshold")
    # the case holds what it is named for
    both = [(l, s) for l in range(levels) for s in (0, 1) if 0 < kept[l, s] < found[l, s]]
    facts = {"A": kept[:, 0].sum() > 0, "B": kept[:, 1].sum() > 0, "mixed2": len({l for l, _ in both}) >= 2,
             "skipped_level": any(not (lvl == l).any() for l in range(levels)), "skipped_b": skipped_b > 0,
             "last_level": found[levels - 1, 0] > 0, "all_occupied": empty_calls > 0, "weeded_to_nothing": bool(((found > 0) & (kept == 0)).any()),
             "prune": nk < N, "noprune": nk == N and not anchors_mask.any(), "no_ds": not grow_ds and found[:, 1].sum() == 0}
    missing = [e for e in expect if not facts[e]]
    print(f"{name}: N {N} levels {np.bincount(lvl, minlength=levels).tolist()} found {found.tolist()} kept {kept.tolist()} "
          f"empty calls {empty_calls} skipped B {skipped_b} kept rows {nk}")
    assert not missing, (name, missing)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, k=k, levels=levels, fork=fork, voxel_size=np.float32(vs), init_pos=init_pos, standard_dist=np.float32(sd),
                        visible_threshold=np.float64(vthr), dist2level=MODES.index(mode), progressive=int(progressive), iteration=iteration,
                        coarse_intervals=np.array(g.coarse_intervals or [0.0]), cam_infos=cam, scaling_act=scaling_act, keep=keep, pass_found=found,
                        pass_kept=kept, in_level=lvl.reshape(-1, 1), in_extra_level=extra0, **{"in_" + nme: v for nme, v in p.items()},
                        **{"in_" + nme: v for nme, v in a.items()}, **moments, **out)
    print(f"wrote {name}: {os.path.getsize(path) // 1024} KiB, {N} anchors -> {nk + U} (kept {nk}, added {U})")


def case(name, seed, **kw):
    for cam_seed in range(100 * seed, 100 * seed + 40):
        try:
            return run_case(name, seed, cam_seed, **kw)
        except Redraw as e:
            print(f"{name}: cameras of seed {cam_seed} redrawn: {e}")
    raise SystemExit(f"{name}: no camera seed holds the margins")


if __name__ == "__main__":
    case("ref_anchor_octree_default.npz", 21, vs=0.11, k=4, F=4, n_pts=900, levels=3, fill=(0.7, 0.6, 0.5), C=24, near=0.3, far=6.0, sd=2.0, vthr=0.2,
         mode="round", expect=("A", "B", "mixed2", "last_level", "prune"))
    case("ref_anchor_octree_gap.npz", 22, vs=0.15, k=4, F=4, n_pts=500, levels=4, fill=(0.7, 0.6, 0.0, 0.5), C=7, near=1.6, far=8.0, sd=2.0, vthr=0.25,
         mode="floor", empty_levels=(2,), still_levels=(3,), expect=("A", "skipped_level", "skipped_b", "all_occupied", "weeded_to_nothing", "prune"))
    case("ref_anchor_octree_k10.npz", 23, vs=0.13, k=10, F=32, n_pts=250, levels=3, fill=(0.6, 0.5, 0.4), C=12, near=0.3, far=6.0, sd=2.0, vthr=0.2,
         mode="round", expect=("A", "B", "prune"))
    case("ref_anchor_octree_noprune.npz", 24, vs=0.12, k=5, F=6, n_pts=600, levels=3, fill=(0.7, 0.6, 0.5), C=9, near=0.3, far=6.0, sd=2.0, vthr=0.2,
         mode="round", prune=False, progressive=True, iteration=3000, expect=("A", "noprune", "no_ds"))
