"""Inputs for the densify_and_prune tests and tools: random scenes whose every compared quantity keeps a relative distance of 1e-5 from its
threshold (so that no selection hangs on the last bit of an exp, a sigmoid or a quotient), and a model object with the reference's attributes.
The thresholds themselves are met by tests/densify_edge_cases.py, which hands the activated tensors over."""
import types

import numpy as np
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
MARGIN = 1e-5
RULES = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01)          # dense threshold 0.05, world-size threshold 0.5
ABS_RULES = dict(abs_max_grad=0.0008, abs_split_radii2D_threshold=20.0)


def near(v, thr):
    return np.abs(v - np.float32(thr)) <= MARGIN * abs(thr)


def margin_violations(g, ga, s_act, o_act, radii, N=2, rules=RULES, extra_grad_thresholds=(), extra_abs_thresholds=()):
    """Rows (bool [P]) with a compared quantity within MARGIN of its threshold, per quantity."""
    ms = s_act.max(1)
    dense, world = rules["percent_dense"] * rules["extent"], 0.1 * rules["extent"]
    bad = {"grad": near(g, rules["max_grad"]), "scale_dense": near(ms, dense), "scale_world": near(ms, world) | near(ms / np.float32(0.8 * N), world),
           "opacity": near(o_act, rules["min_opacity"]), "radius": near(radii, 20.0)}
    if ga is not None:
        bad["grad_abs"] = near(ga, ABS_RULES["abs_max_grad"])
    for t in extra_grad_thresholds:
        bad["grad"] = bad["grad"] | near(g, t)
    for t in extra_abs_thresholds:
        bad["grad_abs"] = bad["grad_abs"] | near(ga, t)
    return bad


def _quot(a, d):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (a / d).astype(np.float32)
    return np.where(np.isnan(q), np.float32(0), q)


def make_inputs(P, seed, cols=3, rest=15, pgsr=False, device="cpu", frac=(0.10, 0.10, 0.05), N=2):
    """Raw parameters, Adam moments and statistics of P Gaussians as float32 arrays on `device`, about frac = (cloned, split, pruned).
    Activations are taken with torch on `device`, where the margins are enforced; offending values are redrawn."""
    r = np.random.default_rng(seed)
    f_clone, f_split, f_prune = frac
    t = lambda a: torch.tensor(a, device=device)
    act_s = lambda raw: torch.exp(t(raw)).cpu().numpy()
    act_o = lambda raw: torch.sigmoid(t(raw)).cpu().numpy()

    def draw_scale(n):
        big = r.uniform(size=(n, 1)) < 0.5
        top = np.where(big, r.uniform(0.06, 0.45, (n, 1)), r.uniform(0.004, 0.045, (n, 1)))
        huge = r.uniform(size=(n, 1)) < f_prune * 0.6                                          # world-size prunes of parents (> 0.5) and of children (> 0.8)
        top = np.where(huge, r.uniform(0.52, 1.3, (n, 1)), top)
        return np.log(top * r.uniform(0.3, 1.0, (n, cols)) ** (r.uniform(size=(n, cols)) < 0.7)).astype(np.float32)

    def draw_accum(n, den, hi_frac, lo, thr):
        hot = r.uniform(size=n) < hi_frac
        g = np.where(hot, thr * r.uniform(1.2, 6.0, n), thr * r.uniform(0.01, 0.8, n))
        return (den * g).astype(np.float32)

    def draw_opacity(n):
        low = r.uniform(size=(n, 1)) < f_prune * 0.6
        return np.where(low, r.uniform(-9.0, -5.6, (n, 1)), r.uniform(-4.5, 4.0, (n, 1))).astype(np.float32)

    scaling = draw_scale(P)
    opacity = draw_opacity(P)
    denom = r.integers(0, 40, P).astype(np.float32)
    hot = 2.0 * max(f_clone, f_split) / 0.975 if P else 0.0                                    # half of the hot rows are small (clones), half big (splits)
    accum = draw_accum(P, denom, hot, 0.0, RULES["max_grad"])
    radii = (r.integers(0, 60, P) + 0.5).astype(np.float32)
    denom_abs = accum_abs = None
    hot_abs = 0.15 if f_split else 0.0                                                         # share of rows above the abs-gradient threshold
    if pgsr:
        denom_abs = denom.copy()
        accum_abs = draw_accum(P, denom_abs, hot_abs, 0.0, ABS_RULES["abs_max_grad"])
    for _ in range(64):
        bad = margin_violations(_quot(accum, denom), _quot(accum_abs, denom_abs) if pgsr else None, act_s(scaling), act_o(opacity).reshape(-1), radii, N=N)
        rows = bad["scale_dense"] | bad["scale_world"]
        if not any(b.any() for b in bad.values()):
            break
        if rows.any():
            scaling[rows] = draw_scale(int(rows.sum()))
        if bad["grad"].any():
            accum[bad["grad"]] = draw_accum(int(bad["grad"].sum()), denom[bad["grad"]], hot, 0.0, RULES["max_grad"])
        if pgsr and bad["grad_abs"].any():
            accum_abs[bad["grad_abs"]] = draw_accum(int(bad["grad_abs"].sum()), denom_abs[bad["grad_abs"]], hot_abs, 0.0, ABS_RULES["abs_max_grad"])
        if bad["opacity"].any():
            opacity[bad["opacity"]] = draw_opacity(int(bad["opacity"].sum()))
    else:
        raise AssertionError("margins not reached")
    p = {"xyz": r.normal(0, 2.0, (P, 3)), "f_dc": r.normal(0, 1, (P, 1, 3)), "f_rest": r.normal(0, 0.2, (P, rest, 3)), "opacity": opacity,
         "scaling": scaling, "rotation": r.normal(0, 1, (P, 4))}
    p = {k: v.astype(np.float32) for k, v in p.items()}
    mom = {}
    for k, v in p.items():                                                                    # few distinct values: the fixtures compress
        mom[k] = ((r.integers(-8, 9, v.shape) / 64.0).astype(np.float32), (r.integers(0, 9, v.shape) / 1024.0).astype(np.float32))
    stats = {"xyz_gradient_accum": accum.reshape(P, 1), "denom": denom.reshape(P, 1), "max_radii2D": radii}
    if pgsr:
        stats.update(xyz_gradient_accum_abs=accum_abs.reshape(P, 1), denom_abs=denom_abs.reshape(P, 1), max_weight=r.uniform(0, 1, P).astype(np.float32))
    return p, mom, stats


class Model:
    """An object with the attributes of the reference's VanillaGaussian / TwoDGaussian / PGSRGaussian that gsrast.densify reads and writes."""

    def __init__(self, p, mom, stats, device, optimizer="torch", pgsr=False, with_state=True, percent_dense=RULES["percent_dense"],
                 max_all_points=6_000_000, max_abs_split_points=50_000, config=None, activated=None):
        self._activated = activated          # (get_scaling, get_opacity) as another device computed them: served while the model has their length
        for k in NAMES:
            setattr(self, ATTRS[k], torch.nn.Parameter(torch.tensor(p[k], device=device)))
        for k, v in stats.items():
            setattr(self, k, torch.tensor(v, device=device))
        self.percent_dense = percent_dense
        self.spatial_lr_scale = RULES["extent"]
        self.config = config
        if pgsr:
            self.abs_split_radii2D_threshold, self.max_abs_split_points, self.max_all_points = ABS_RULES["abs_split_radii2D_threshold"], max_abs_split_points, max_all_points
        groups = [{"params": [getattr(self, ATTRS[k])], "lr": 1e-3, "name": k} for k in NAMES]
        if optimizer == "torch":
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        else:
            from gsrast.optim import Adam
            self.optimizer = Adam(groups, lr=0.0, eps=1e-15)
        if with_state:
            for k in NAMES:
                q = getattr(self, ATTRS[k])
                self.optimizer.state[q] = {"step": torch.tensor(7.0), "exp_avg": torch.tensor(mom[k][0], device=device), "exp_avg_sq": torch.tensor(mom[k][1], device=device)}

    @property
    def get_scaling(self):
        if self._activated is not None and self._activated[0].shape[0] == self._scaling.shape[0]:
            return self._activated[0]
        return torch.exp(self._scaling)

    @property
    def get_opacity(self):
        if self._activated is not None and self._activated[1].shape[0] == self._opacity.shape[0]:
            return self._activated[1]
        return torch.sigmoid(self._opacity)

    def tensors(self):
        return {k: getattr(self, ATTRS[k]).detach() for k in NAMES}

    def moments(self):
        out = {}
        for k in NAMES:
            st = self.optimizer.state.get(getattr(self, ATTRS[k]), None)
            if st is not None and "exp_avg" in st:
                out[k] = (st["exp_avg"], st["exp_avg_sq"])
        return out


def config(**kw):
    base = dict(densification_interval=100, opacity_reset_interval=3000, densify_from_iter=500, densify_until_iter=15000, densify_grad_threshold=RULES["max_grad"],
                opacity_cull_threshold=RULES["min_opacity"], densify_abs_grad_threshold=ABS_RULES["abs_max_grad"])
    base.update(kw)
    return types.SimpleNamespace(**base)


# ---------------------------------------------------------------------------------------------------------------- fixtures and checks
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("vanilla", "vanilla_nosize", "vanilla_sh3", "twod", "pgsr", "pgsr_cap_all", "pgsr_cap_abs", "pgsr_cap_clone", "empty")
MINIMUM = {"vanilla": (10, 10, 5), "vanilla_nosize": (10, 10, 5), "vanilla_sh3": (3, 3, 1), "twod": (10, 10, 5), "pgsr": (10, 10, 5), "pgsr_cap_all": (10, 10, 5),
           "pgsr_cap_abs": (10, 10, 5), "pgsr_cap_clone": (5, 0, 1), "empty": (0, 0, 0)}          # clones, splits, pruned


def load_fixture(case):
    path = os.path.join(GOLDEN, f"ref_densify_prune_{case}.npz")
    d = dict(np.load(path))
    d["path"] = path
    return d


def fixture_inputs(d):
    """-> (p, mom, stats, pgsr, rules) of a fixture, as make_inputs returns them plus the rules of its call."""
    pgsr = str(d["kind"]) == "pgsr"
    p = {k: d["in_" + k] for k in NAMES}
    mom = {k: (d["in_m_" + k], d["in_v_" + k]) for k in NAMES}
    stats = {k: d["in_" + k] for k in ("xyz_gradient_accum", "denom", "max_radii2D") + (("xyz_gradient_accum_abs", "denom_abs", "max_weight") if pgsr else ())}
    rules = dict(RULES, max_screen_size=int(d["max_screen_size"]) or None)
    if pgsr:
        rules.update(ABS_RULES, max_all_points=int(d["max_all_points"]), max_abs_split_points=int(d["max_abs_split_points"]))
    return p, mom, stats, pgsr, rules


def run_layout(p, mom, stats, s_act, o_act, z_split, z_clone, pgsr, rules, device="cpu", N=2):
    """tests/ref_densify_torch.layout on numpy / tensor inputs."""
    import ref_densify_torch as R
    t = lambda a: a.to(device) if isinstance(a, torch.Tensor) else torch.tensor(a, device=device)
    kw = dict(rules)
    if pgsr:
        kw.update(accum_abs=t(stats["xyz_gradient_accum_abs"]), denom_abs=t(stats["denom_abs"]))
    return R.layout({k: t(v) for k, v in p.items()}, {k: (t(m), t(v)) for k, (m, v) in mom.items()}, t(stats["xyz_gradient_accum"]), t(stats["denom"]),
                    t(s_act), t(o_act), t(stats["max_radii2D"]), z_split=t(z_split), z_clone=t(z_clone) if pgsr else None, N=N, **kw)


def check_against_layout(got_p, got_m, L, p, s_act, z_split, z_clone, pgsr, N=2, what=""):
    """got_p / got_m (tensors) against the layout L of the same inputs: exact equality of every copied row of every parameter and moment, and the
    float64 bounds of DESIGN.md §4.8 for the computed columns:
        |d xyz_i| <= 32 * 2^-24 * (|xyz_i| + sum_j |z_j s_j|),   |d scaling| <= 8 * 2^-24 * max(1, |want|)
    against a float64 evaluation of the formula on the float32 inputs.  Returns the largest errors in units of those bounds."""
    import ref_densify_torch as R
    dev = L["src"].device
    t = lambda a: a.to(dev) if isinstance(a, torch.Tensor) else torch.tensor(a, device=dev)
    n_o, n_c, n_s = L["parts"]
    rows = L["src"].numel()
    src = L["src"]
    S = L["counts"]["splits"]
    computed_xyz = torch.zeros(rows, dtype=torch.bool, device=dev)
    computed_xyz[n_o + n_c:] = True
    if pgsr:
        computed_xyz[n_o:n_o + n_c] = True
    child = torch.zeros(rows, dtype=torch.bool, device=dev)
    child[n_o + n_c:] = True
    for k in NAMES:
        g, w = t(got_p[k]), L["params"][k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        mask = computed_xyz if k == "xyz" else (child if k == "scaling" else torch.zeros_like(child))
        assert torch.equal(g[~mask], t(p[k])[src][~mask]), (what, k, "copied rows")
        assert torch.equal(g[~mask], w[~mask]), (what, k, "copied rows against the restatement")
        if k in L["moments"]:
            for j in range(2):
                assert torch.equal(t(got_m[k][j]), L["moments"][k][j]), (what, k, "moment", j)
        else:
            assert k not in got_m
    worst = [0.0, 0.0]
    if computed_xyz.any():
        clone_rank = torch.cumsum(L["clone"].long(), 0) - 1
        split_rank = torch.cumsum(L["split"].long(), 0) - 1
        z = torch.zeros(rows, 3, dtype=torch.float32, device=dev)
        if pgsr and n_c:
            z[n_o:n_o + n_c] = t(z_clone)[clone_rank[src[n_o:n_o + n_c]]]
        for r in range(N):
            b = n_o + n_c + r * n_s
            z[b:b + n_s] = t(z_split)[r * S + split_rank[src[b:b + n_s]]]
        par = src[computed_xyz]
        want, mag = R.sample_xyz_f64(t(p["xyz"])[par], t(p["rotation"])[par], t(s_act)[par], z[computed_xyz])
        err = (t(got_p["xyz"])[computed_xyz].double() - want).abs()
        bound = 32 * 2.0 ** -24 * (t(p["xyz"])[par].double().abs() + mag)
        assert (err <= bound).all(), (what, "xyz", float((err / bound).max()))
        worst[0] = float((err / bound.clamp_min(1e-300)).max())
    if child.any():
        want = torch.log(t(s_act)[src[child]].double() / (0.8 * N))
        err = (t(got_p["scaling"])[child].double() - want).abs()
        bound = 8 * 2.0 ** -24 * want.abs().clamp_min(1.0)
        assert (err <= bound).all(), (what, "scaling", float((err / bound).max()))
        worst[1] = float((err / bound).max())
    return worst
