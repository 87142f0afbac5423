"""densify_and_prune_ on both sides of every selection threshold (gsrast.densify; gs-sr_amd/csrc/gsr_densify.hip den_classify).

tests/test_gpu_densify.py keeps every compared quantity 1e-5 away from its threshold; the scenes of tests/densify_edge_cases.py put rows one float32
below, on and one float32 above each of them, give the special quotients (0/0, x/0, NaN, negative, denormal), saturate the map (every row cloned,
split N ways, pruned) around the wave and block sizes, and bind each PGSR cap inside a group of tied gradients.  Expected: the torch restatement
on the CPU (tests/ref_densify_torch.layout, child_rule="quotient"): counts, the source map, every copied row and moment and the zeroed
statistics exactly, the computed columns within the float64 bounds of densify_cases.check_against_layout, and the six status words of the plan
against the written-out classification.  tests/test_densify_edges_cpu.py shows that reversing any comparison changes these expectations."""
import pytest
import torch

import densify_cases as DC
import densify_edge_cases as E
from test_gpu_densify import _check_model_state, _run_random

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = E.case_ids()


@pytest.fixture
def plan_status(monkeypatch):
    """The status words of every gsr_densify_plan call, in order."""
    from gsrast import densify
    seen, inner = [], densify.call

    def call(name, dev, *args):
        out = inner(name, dev, *args)
        if name == "gsr_densify_plan":
            seen.append(args[-1].tolist())
        return out
    monkeypatch.setattr(densify, "call", call)
    return seen


def _run(cid, opt, plan_status):
    from gsrast import densify
    c = E.make_case(cid)
    kind, N, rules = c["kind"], c["N"], c["rules"]
    pgsr = E.KINDS[kind]["pgsr"]
    p, mom, stats, s_act, o_act = c["inputs"]
    P = s_act.shape[0]
    loc = E.classify_local(stats, s_act, o_act, rules, N)
    src, status = E.rows_of(loc, N)
    z_split, z_clone = E.noise(loc, N, 5)
    L = DC.run_layout(p, mom, stats, s_act, o_act, z_split, z_clone, pgsr, rules, device="cpu", N=N)
    assert L["src"].tolist() == src.tolist()
    caps = dict(max_all_points=rules["max_all_points"], max_abs_split_points=rules["max_abs_split_points"]) if pgsr else {}
    m = DC.Model(p, mom, stats, DEV, optimizer=opt, pgsr=pgsr, activated=(torch.tensor(s_act, device=DEV), torch.tensor(o_act, device=DEV)), **caps)
    n = densify.densify_and_prune_(m, rules["max_grad"], rules["min_opacity"], rules["extent"], rules["max_screen_size"],
                                   abs_max_grad=rules["abs_max_grad"] if pgsr else None, N=N, noise_split=torch.tensor(z_split, device=DEV),
                                   noise_clone=torch.tensor(z_clone, device=DEV) if pgsr else None)
    assert plan_status[-1][:6] == status, (cid, plan_status[-1], status)
    assert n == L["counts"]["rows"] == len(src), (cid, n, L["counts"])
    _check_model_state(m, n, pgsr)
    got_p = {k: v.cpu() for k, v in m.tensors().items()}
    got_m = {k: (a.cpu(), b.cpu()) for k, (a, b) in m.moments().items()}
    worst = DC.check_against_layout(got_p, got_m, L, p, s_act, z_split, z_clone, pgsr, N=N, what=cid)
    print(cid, opt, "status", status, "worst error in units of the bounds (xyz, scaling):", worst)
    if c["tie"] is not None:                                        # the cap bound: the plan ran again with the quantile
        assert len(plan_status) >= 3
    return c, L


@pytest.mark.parametrize("opt", ["gsrast", "torch"])
@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("named")])
def test_named_rows(cid, opt, plan_status):
    c, L = _run(cid, opt, plan_status)
    assert L["counts"]["clones"] > 100 and L["counts"]["splits"] > 100 and L["counts"]["pruned"] > 100


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("all")])
def test_saturated_scenes(cid, plan_status):
    c, L = _run(cid, "gsrast", plan_status)
    P, N = c["inputs"][3].shape[0], c["N"]
    want = {"clone": 2 * P, "split": N * P, "prune": 0}[cid.split("-")[1]]
    assert L["counts"]["rows"] == want


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("tie")])
def test_caps_with_ties(cid, plan_status):
    """The quantile's interpolation position lies inside a group of equal masked gradients: the threshold is that value on any device and the strict
    `>` drops the whole group -- 20 rows pass, not 40."""
    c, L = _run(cid, "gsrast", plan_status)
    which, tie, passing = c["tie"]
    want = {"clone": (passing, 0), "split": (0, passing), "abs": (0, passing + E.BOTH_ROWS)}[which]
    assert (L["counts"]["clones"], L["counts"]["splits"]) == want


@pytest.mark.parametrize("kind", list(E.KINDS))
@pytest.mark.parametrize("N", [1, 3, 4])
def test_random_scene_with_N_children(kind, N):
    m, L, worst = _run_random(kind, 2500, seed=40 + N, rest=3, N=N)
    c = L["counts"]
    print(kind, N, c, "worst error in units of the bounds (xyz, scaling):", worst)
    assert c["clones"] > 100 and c["splits"] > 100 and c["pruned"] > 50 and c["rows"] == 2500 + c["clones"] + (N - 1) * c["splits"] - c["pruned"]
