"""Golden vectors of densify_and_prune for the explicit Gaussians, produced by RUNNING the reference's own VanillaGaussian, TwoDGaussian and
PGSRGaussian.densify_and_prune (torch, CPU).

    python tests/golden/make_golden_densify.py       # needs /root/reference; writes tests/golden/ref_densify_prune_*.npz

Pinned: gssr/gaussian/vanilla_gaussian.py:295-426, twod_gaussian.py:22-46, pgsr_gaussian.py:43-155, called on the reference's own model objects
with a real torch.optim.Adam (one named group per tensor, with moments).  The technique is make_golden_anchor.py's: absent packages become inert
MagicMock stand-ins, the hard-coded device="cuda" is redirected to the CPU, torch.cuda.empty_cache is stubbed.  torch.normal is wrapped: it draws
z = randn(std.shape), records z and returns mean + z * std, which is what the CPU kernel computes.  torch.quantile is wrapped to record the
thresholds of the PGSR caps.  The files hold arrays only: inputs, Adam moments, get_scaling / get_opacity as the reference computed them, the
recorded z, every output tensor and the counts.

The generator ASSERTS A MARGIN: no gradient, abs-gradient, scale (against percent_dense * extent, and against 0.1 * extent for parents and for
s / (0.8 N)), opacity or radius lies within relative 1e-5 of its threshold, the cap quantiles included (tests/densify_cases.py redraws offenders).
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
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : densify_cases


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
van = ref_import("gssr.gaussian.vanilla_gaussian")
twod = ref_import("gssr.gaussian.twod_gaussian")
pgsr_mod = ref_import("gssr.gaussian.pgsr_gaussian")
import densify_cases as DC  # noqa: E402


def _cpu(fn):
    return lambda *a, **k: fn(*a, **{kk: ("cpu" if kk == "device" and isinstance(v, str) and v.startswith("cuda") else v) for kk, v in k.items()})


for _n in ("zeros", "ones", "zeros_like", "ones_like", "tensor", "arange"):
    setattr(torch, _n, _cpu(getattr(torch, _n)))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.empty_cache = lambda: None
DRAWS, QUANTILES = [], []


def _recording_normal(mean, std, **k):
    z = torch.randn(std.shape)
    DRAWS.append(z.clone())
    return mean + z * std


_quantile = torch.quantile


def _recording_quantile(x, q, *a, **k):
    t = _quantile(x, q, *a, **k)
    QUANTILES.append((float(t), x.clone(), float(q)))
    return t


torch.normal = _recording_normal
torch.quantile = _recording_quantile
NAMES = DC.NAMES


def run_case(name, kind, seed, P, rest=3, max_screen_size=20, frac=(0.10, 0.10, 0.05), cap=None, need=(10, 10, 5)):
    torch.manual_seed(seed)
    is_pgsr = kind == "pgsr"
    cols = 2 if kind == "twod" else 3
    p, mom, stats = DC.make_inputs(P, seed, cols=cols, rest=rest, pgsr=is_pgsr, frac=frac)
    cls, ccls = {"vanilla": (van.VanillaGaussian, van.VanillaGaussianConfig), "twod": (twod.TwoDGaussian, twod.TwoDGaussianConfig),
                 "pgsr": (pgsr_mod.PGSRGaussian, pgsr_mod.PGSRGaussianConfig)}[kind]
    cfg = ccls(); cfg.percent_dense = DC.RULES["percent_dense"]
    g = cls(cfg, device="cpu")
    for k in NAMES:
        setattr(g, DC.ATTRS[k], torch.nn.Parameter(torch.tensor(p[k])))
    g.optimizer = torch.optim.Adam([{"params": [getattr(g, DC.ATTRS[k])], "lr": 0.0, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    for k in NAMES:
        g.optimizer.state[getattr(g, DC.ATTRS[k])] = {"step": torch.tensor(7.0), "exp_avg": torch.tensor(mom[k][0]), "exp_avg_sq": torch.tensor(mom[k][1])}
    for k, v in stats.items():
        setattr(g, k, torch.tensor(v))
    s_act, o_act = g.get_scaling.detach().numpy().copy(), g.get_opacity.detach().numpy().copy()
    quot = lambda a, d: np.nan_to_num((torch.tensor(a) / torch.tensor(d)).numpy(), nan=0.0).reshape(-1)
    gr = quot(stats["xyz_gradient_accum"], stats["denom"])
    ga = quot(stats["xyz_gradient_accum_abs"], stats["denom_abs"]) if is_pgsr else None
    bad = DC.margin_violations(gr, ga, s_act, o_act.reshape(-1), stats["max_radii2D"])
    assert not any(b.any() for b in bad.values()), {k: int(b.sum()) for k, b in bad.items()}
    extra = {}
    import ref_densify_torch as R
    clone, split, _, _ = R.classify(torch.tensor(stats["xyz_gradient_accum"]), torch.tensor(stats["denom"]), torch.tensor(s_act), torch.tensor(o_act),
                                    torch.tensor(stats["max_radii2D"]), max_screen_size=max_screen_size, **DC.RULES)
    if is_pgsr:
        C, Sg = int(clone.sum()), int(split.sum())
        if cap == "all":
            g.max_all_points = P + C + Sg // 2                    # the gradient split alone overflows: quantile branch, no abs rule
        elif cap == "abs":
            g.max_abs_split_points = 4
        elif cap == "clone":
            g.max_all_points = P + C // 2
        extra = dict(max_all_points=g.max_all_points, max_abs_split_points=g.max_abs_split_points, abs_split_radii2D_threshold=g.abs_split_radii2D_threshold)
    del DRAWS[:], QUANTILES[:]
    with torch.no_grad():
        if is_pgsr:
            g.densify_and_prune(DC.RULES["max_grad"], DC.ABS_RULES["abs_max_grad"], DC.RULES["min_opacity"], DC.RULES["extent"], max_screen_size)
        else:
            g.densify_and_prune(DC.RULES["max_grad"], DC.RULES["min_opacity"], DC.RULES["extent"], max_screen_size)
    for thr, x, q in QUANTILES:                                   # a cap's quantile keeps the same margin from every value it is compared with
        x = x.numpy()
        if q >= 1.0:                                              # no room left: the threshold IS the maximum and `> max` selects nothing, whatever the rounding
            assert thr == x.max()
            continue
        assert not (np.abs(x - np.float32(thr)) <= DC.MARGIN * abs(thr)).any(), (name, thr)
    assert bool(QUANTILES) == (cap is not None), (name, len(QUANTILES))
    z_clone = DRAWS[0].numpy() if is_pgsr and len(DRAWS) == 2 else np.zeros((0, 3), np.float32)
    z_split = DRAWS[-1].numpy() if DRAWS else np.zeros((0, 3), np.float32)
    if not is_pgsr:
        assert len(DRAWS) == 1
    out = {}
    for k in NAMES:
        q = getattr(g, DC.ATTRS[k])
        st = g.optimizer.state[q]
        assert float(st["step"]) == 7.0
        out["out_" + k] = q.detach().numpy().copy(); out["out_m_" + k] = st["exp_avg"].numpy().copy(); out["out_v_" + k] = st["exp_avg_sq"].numpy().copy()
    n = out["out_xyz"].shape[0]
    for k in stats:
        v = getattr(g, k).numpy()
        assert v.shape == ((n,) if k in ("max_radii2D", "max_weight") else (n, 1)) and not v.any(), k
    N = 2
    S = z_split.shape[0] // N
    C = z_clone.shape[0] if is_pgsr else int(clone.sum())        # 3DGS / 2DGS draw nothing for a clone: counted by the uncapped rule
    pruned = P + C + (N - 1) * S - n
    counts = np.array([C, S, pruned, n], np.int64)                # clones, splits, rows the final mask removed, rows
    assert C >= need[0] and S >= need[1] and pruned >= need[2], (name, counts)
    if frac == (0.0, 0.0, 0.0):
        assert C == 0 and S == 0 and n == P
    if max_screen_size:                                           # the kept quirk: rows whose input radius exceeds the screen-size threshold survive
        assert int(((stats["max_radii2D"] > max_screen_size) & ~split.numpy()).sum()) > pruned
    path = os.path.join(HERE, name)
    np.savez_compressed(path, kind=kind, cols=cols, max_screen_size=0 if max_screen_size is None else max_screen_size, counts=counts,
                        quantiles=np.array([t for t, _, _ in QUANTILES], np.float64), scaling_act=s_act, opacity_act=o_act, z_split=z_split, z_clone=z_clone,
                        **{k: np.array(v) for k, v in extra.items()}, **{"in_" + k: v for k, v in p.items()}, **{"in_m_" + k: v[0] for k, v in mom.items()},
                        **{"in_v_" + k: v[1] for k, v in mom.items()}, **{"in_" + k: v for k, v in stats.items()}, **out)
    print(f"wrote {name}: {os.path.getsize(path) // 1024} KiB, {P} -> {n} rows, splits {S}, clones {C}, pruned {pruned}, caps {len(QUANTILES)}")


if __name__ == "__main__":
    run_case("ref_densify_prune_vanilla.npz", "vanilla", 21, 320)
    run_case("ref_densify_prune_vanilla_nosize.npz", "vanilla", 22, 300, max_screen_size=None)
    run_case("ref_densify_prune_vanilla_sh3.npz", "vanilla", 23, 120, rest=15, need=(3, 3, 1))
    run_case("ref_densify_prune_twod.npz", "twod", 24, 300)
    run_case("ref_densify_prune_pgsr.npz", "pgsr", 25, 320)
    run_case("ref_densify_prune_pgsr_cap_all.npz", "pgsr", 26, 320, cap="all")
    run_case("ref_densify_prune_pgsr_cap_abs.npz", "pgsr", 27, 320, cap="abs")
    run_case("ref_densify_prune_pgsr_cap_clone.npz", "pgsr", 28, 320, cap="clone", need=(5, 0, 1))
    run_case("ref_densify_prune_empty.npz", "vanilla", 29, 200, frac=(0.0, 0.0, 0.0), need=(0, 0, 0))
