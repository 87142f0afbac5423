"""Golden vectors of anchor growing + pruning, produced by RUNNING the reference's own ScaffoldGaussian.adjust_anchor (torch, CPU).

    python tests/golden/make_golden_anchor.py       # needs /root/reference; writes tests/golden/ref_anchor_adjust_*.npz

Pinned: gssr/gaussian/scaffold_gaussian.py:651-705 adjust_anchor, :555-649 anchor_growing, :460-484 cat_tensors_to_optimizer, :510-552 prune_anchor,
called on the reference's own model object with a real torch.optim.Adam (one named group per tensor, stepped once so that moments exist).  The
technique is make_golden_ref.py's: absent packages become inert MagicMock stand-ins, the hard-coded device="cuda" is redirected to the CPU.
torch_scatter (third-party, absent) is replaced by its published semantics: scatter_max(src, index, dim=0)[0] = zeros(U, F).scatter_reduce(0, index,
src, "amax", include_self=False) -- a stated stand-in, as pytorch3d's quaternion_to_matrix is in make_golden_ref.py.  torch.rand_like is wrapped so
that every level's draw is recorded.  The files hold arrays only: inputs (parameters, moments, accumulators, the activated scaling as the reference
computed it, the draws) and results (keep mask, the new rows of every parameter, the four accumulators, additions per level); the generator
asserts that [old[keep] ; new rows] IS the reference's final state, so nothing is lost by not storing every tensor twice.
"""
import importlib
import os
import sys
import warnings
from unittest import mock

import numpy as np
import torch

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : ref_anchor_torch


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
mod = ref_import("gssr.gaussian.scaffold_gaussian")


def _cpu(fn):
    return lambda *a, **k: fn(*a, **{kk: ("cpu" if kk == "device" and isinstance(v, str) and v.startswith("cuda") else v) for kk, v in k.items()})


for _n in ("zeros", "ones", "zeros_like", "ones_like", "tensor", "arange"):
    setattr(torch, _n, _cpu(getattr(torch, _n)))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.empty_cache = lambda: None
DRAWS = []
_rand_like = torch.rand_like


def _recording_rand_like(t, **k):
    r = _rand_like(t, **k)
    DRAWS.append(r.clone())
    return r


torch.rand_like = _recording_rand_like


def _scatter_max(src, index, dim=0):
    U = int(index.max()) + 1 if index.numel() else 0
    out = torch.zeros(U, src.shape[1], dtype=src.dtype).scatter_reduce(0, index, src, "amax", include_self=False)
    return out, None


mod.scatter_max = _scatter_max
NAMES = ("anchor", "offset", "anchor_feat", "opacity", "scaling", "rotation")
ACCS = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")


def surface_anchors(r, n, vs, extent):
    p = r.uniform(-extent, extent, (n, 2))
    z = 0.15 * np.sin(3.0 * p[:, 0]) * np.cos(2.0 * p[:, 1])
    pts = np.concatenate([p, z[:, None]], 1)
    return (np.unique(np.round(pts / vs), axis=0) * vs).astype(np.float32)


def lattice_anchors(vs, init_factor, half):
    c = np.arange(-half, half)
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return (g * (vs * init_factor)).astype(np.float32), (np.abs(g + 0.5) < half - 1.5).all(1)      # positions, interior flag


def run_case(name, seed, vs, k, F, n, kind="surface", prune=True):
    r = np.random.default_rng(seed)
    torch.manual_seed(seed)
    cfg = mod.ScaffoldGaussianConfig(); cfg.n_offsets = k; cfg.feat_dim = F; cfg.voxel_size = vs
    g = mod.ScaffoldGaussian(cfg, device="cpu")
    interior = None
    if kind == "surface":
        anchor = surface_anchors(r, n, vs, 0.6)
        spread = r.uniform(2.0, 14.0, (anchor.shape[0], 1)) * vs
    else:
        anchor, interior = lattice_anchors(vs, cfg.update_init_factor, n)
        spread = np.full((anchor.shape[0], 1), 0.45 * vs * cfg.update_init_factor)       # |offset * scale| stays below one coarse cell
    N = anchor.shape[0]
    scaling = np.log(spread * r.uniform(0.7, 1.0, (N, 6))).astype(np.float32)
    scaling[r.uniform(size=N) < 0.2, 3:] = 0.3                                             # raw values above the 0.05 clamp
    offset = r.uniform(-1, 1, (N, k, 3)).astype(np.float32)
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
    if interior is not None:
        denom[~np.repeat(interior, k)] = 0.0                                              # only interior anchors propose: every proposal lands on the lattice block
    accum = (denom * np.exp(r.normal(np.log(3e-4), 1.0, (N * k, 1)))).astype(np.float32)
    demon = r.integers(0, 121 if prune else 81, (N, 1)).astype(np.float32)
    opac = (demon * r.uniform(0.0, 0.02, (N, 1))).astype(np.float32)
    a = {"opacity_accum": opac, "anchor_demon": demon, "offset_gradient_accum": accum, "offset_denom": denom}
    for nme in ACCS:
        setattr(g, nme, torch.tensor(a[nme]))
    moments = {}
    for nme in NAMES:
        st = g.optimizer.state[getattr(g, "_" + nme)]
        moments["m_" + nme] = st["exp_avg"].numpy().copy(); moments["v_" + nme] = st["exp_avg_sq"].numpy().copy()
    scaling_act = g.get_scaling.detach().numpy().copy()
    levels = []
    cat = g.cat_tensors_to_optimizer
    g.cat_tensors_to_optimizer = lambda d: (levels.append((len(DRAWS) - 1, d["anchor"].shape[0])), cat(d))[1]
    del DRAWS[:]
    with torch.no_grad():
        g.adjust_anchor(check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005)
    assert len(DRAWS) == g.update_depth
    counts = np.zeros(g.update_depth, np.int64)
    for lvl, c in levels:
        counts[lvl] = c
    U = int(counts.sum())
    anchors_mask = demon > 80.0
    keep = ~((opac < np.float32(0.005) * demon) & anchors_mask).reshape(-1)
    nk = int(keep.sum())
    out = {}
    for nme in NAMES:
        fin = getattr(g, "_" + nme).detach().numpy()
        st = g.optimizer.state[getattr(g, "_" + nme)]
        old = p[nme][keep]
        if nme == "scaling":
            old = old.copy(); old[:, 3:] = np.minimum(old[:, 3:], np.float32(0.05))
        assert fin.shape[0] == nk + U and np.array_equal(fin[:nk], old), nme
        for key, src in (("exp_avg", moments["m_" + nme]), ("exp_avg_sq", moments["v_" + nme])):
            mv = st[key].numpy()
            assert np.array_equal(mv[:nk], src[keep]) and not mv[nk:].any() and mv.shape == fin.shape, (nme, key)
        assert float(st["step"]) == 1.0
        out["new_" + nme] = fin[nk:].copy()
    for nme in ACCS:
        out["out_" + nme] = getattr(g, nme).numpy().copy()
    assert g.max_radii2D.shape == (nk + U,) and not g.max_radii2D.any()
    # the case holds what it is named for
    if kind == "lattice":
        import ref_anchor_torch as R
        assert U == 0 and counts[0] == 0, counts
        grads = np.nan_to_num(accum / np.where(denom == 0, np.nan, denom)).reshape(-1)
        later, _ = R.grow_level(torch.tensor(anchor), torch.tensor(offset), torch.tensor(scaling_act), torch.tensor(p["anchor_feat"]), torch.tensor(np.abs(grads)),
                                torch.tensor(denom.reshape(-1) > 40.0), cell=vs * 4, thr_lo=0.0004, rand=DRAWS[1].reshape(-1), rand_thr=0.25)
        assert later.shape[0] > 0, "level 1 would have added anchors had it not been skipped"
    else:
        assert (counts > 0).sum() >= 2, counts
    assert (nk < N) == prune and (prune or not anchors_mask.any())
    path = os.path.join(HERE, name)
    np.savez_compressed(path, k=k, voxel_size=vs, update_depth=g.update_depth, update_init_factor=g.update_init_factor,
                        update_hierachy_factor=g.update_hierachy_factor, scaling_act=scaling_act, keep=keep, level_counts=counts,
                        **{f"rand_{i}": d.numpy().reshape(-1) for i, d in enumerate(DRAWS)}, **{"in_" + nme: v for nme, v in p.items()},
                        **{"in_" + nme: v for nme, v in a.items()}, **moments, **out)
    print(f"wrote {name}: {os.path.getsize(path) // 1024} KiB, {N} anchors -> {nk + U} (kept {nk}, added {counts.tolist()})")


if __name__ == "__main__":
    run_case("ref_anchor_adjust_default.npz", seed=11, vs=0.01, k=4, F=4, n=700)
    run_case("ref_anchor_adjust_skip.npz", seed=12, vs=0.01, k=4, F=4, n=4, kind="lattice")
    run_case("ref_anchor_adjust_k10.npz", seed=13, vs=0.003, k=10, F=32, n=150)
    run_case("ref_anchor_adjust_noprune.npz", seed=14, vs=0.02, k=5, F=6, n=400, prune=False)
