"""CPU checks of gsrast.densify (no GPU): the fixtures produced by the reference's own VanillaGaussian / TwoDGaussian / PGSRGaussian
.densify_and_prune equal the independent torch restatement tests/ref_densify_torch.py, hold what they are named for, the header declares the
new entry points, and argument errors are raised before any device call."""
import os
import re

import numpy as np
import pytest
import torch

import densify_cases as DC
import ref_densify_torch as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_out(d):
    got_p = {k: torch.tensor(d["out_" + k]) for k in DC.NAMES}
    got_m = {k: (torch.tensor(d["out_m_" + k]), torch.tensor(d["out_v_" + k])) for k in DC.NAMES}
    return got_p, got_m


@pytest.mark.parametrize("case", DC.FIXTURES)
def test_restatement_equals_fixture(case):
    d = DC.load_fixture(case)
    p, mom, stats, pgsr, rules = DC.fixture_inputs(d)
    L = DC.run_layout(p, mom, stats, d["scaling_act"], d["opacity_act"], d["z_split"], d["z_clone"], pgsr, rules)
    C, S, pruned, rows = (int(v) for v in d["counts"])
    assert L["counts"] == {"clones": C, "splits": S, "pruned": pruned, "rows": rows}
    got_p, got_m = _fixture_out(d)
    # the reference's float32 chain and the restatement's both stay inside the float64 bounds; every copied row is equal bit for bit
    w1 = DC.check_against_layout(got_p, got_m, L, p, d["scaling_act"], d["z_split"], d["z_clone"], pgsr, what=case + " fixture")
    w2 = DC.check_against_layout(L["params"], L["moments"], L, p, d["scaling_act"], d["z_split"], d["z_clone"], pgsr, what=case + " restatement")
    print(case, "worst error in units of the bounds (xyz, scaling): fixture", w1, "restatement", w2)
    # on one device the restatement's computed columns are the reference's, bit for bit
    assert torch.equal(L["params"]["xyz"], got_p["xyz"]) and torch.equal(L["params"]["scaling"], got_p["scaling"])


@pytest.mark.parametrize("case", [c for c in DC.FIXTURES if not c.startswith("pgsr_cap")])
def test_chain_equals_layout(case):
    """The reference-shaped chain (the timing baseline of tools/bench_densify.py) and the one-gather layout are the same function."""
    d = DC.load_fixture(case)
    p, mom, stats, pgsr, rules = DC.fixture_inputs(d)
    t = torch.tensor
    kw = {k: v for k, v in rules.items() if k not in ("max_all_points", "max_abs_split_points")}
    if pgsr:
        kw.update(accum_abs=t(stats["xyz_gradient_accum_abs"]), denom_abs=t(stats["denom_abs"]))
    st, mo, stats_out = R.chain({k: t(v) for k, v in p.items()}, {k: (t(m), t(v)) for k, (m, v) in mom.items()}, t(stats["xyz_gradient_accum"]),
                                t(stats["denom"]), torch.exp, torch.sigmoid, t(stats["max_radii2D"]), z_split=t(d["z_split"]),
                                z_clone=t(d["z_clone"]) if pgsr else None, **kw)
    for k in DC.NAMES:
        assert torch.equal(st[k], t(d["out_" + k])), k
        assert torch.equal(mo[k][0], t(d["out_m_" + k])) and torch.equal(mo[k][1], t(d["out_v_" + k])), k
    for v in stats_out.values():
        assert v.shape[0] == st["xyz"].shape[0] and not v.any()


@pytest.mark.parametrize("case", DC.FIXTURES)
def test_fixture_holds_what_it_is_named_for(case):
    d = DC.load_fixture(case)
    assert os.path.getsize(d["path"]) < 275 * 1024
    C, S, pruned, rows = (int(v) for v in d["counts"])
    need = DC.MINIMUM[case]
    assert C >= need[0] and S >= need[1] and pruned >= need[2], (C, S, pruned)
    p, mom, stats, pgsr, rules = DC.fixture_inputs(d)
    P = p["xyz"].shape[0]
    assert d["out_xyz"].shape[0] == rows == P + C + S - pruned
    if case == "empty":
        assert C == 0 and S == 0 and pruned == 0
        for k in DC.NAMES:
            assert np.array_equal(d["out_" + k], p[k])
    if case == "twod":
        assert p["scaling"].shape[1] == 2 and d["out_scaling"].shape[1] == 2
    if case == "vanilla_sh3":
        assert p["f_rest"].shape[1:] == (15, 3)
    if case == "vanilla_nosize":
        assert rules["max_screen_size"] is None and (d["scaling_act"].max(1) > 0.5).any()         # rows a size rule would have pruned
    if case.startswith("pgsr_cap"):
        assert len(d["quantiles"]) >= 1
    elif pgsr:
        assert len(d["quantiles"]) == 0 and d["z_clone"].shape[0] == C > 0
    # the margin the generator asserted
    quot = lambda a, b: np.nan_to_num((torch.tensor(a) / torch.tensor(b)).numpy(), nan=0.0).reshape(-1)
    bad = DC.margin_violations(quot(stats["xyz_gradient_accum"], stats["denom"]),
                               quot(stats["xyz_gradient_accum_abs"], stats["denom_abs"]) if pgsr else None, d["scaling_act"], d["opacity_act"].reshape(-1),
                               stats["max_radii2D"])
    assert not any(b.any() for b in bad.values())


@pytest.mark.parametrize("case", ["vanilla", "twod", "pgsr"])
def test_size_quirk_rows_are_kept(case):
    """The screen-size term of the final prune compares freshly zeroed statistics: rows whose INPUT max_radii2D exceeds max_screen_size = 20
    survive in the reference's own output (they are pruned only for their opacity or world size)."""
    d = DC.load_fixture(case)
    p, mom, stats, pgsr, rules = DC.fixture_inputs(d)
    assert rules["max_screen_size"] == 20
    L = DC.run_layout(p, mom, stats, d["scaling_act"], d["opacity_act"], d["z_split"], d["z_clone"], pgsr, rules)
    n_o = L["parts"][0]
    big = torch.tensor(stats["max_radii2D"])[L["src"][:n_o]] > 20
    assert int(big.sum()) >= 20
    assert np.array_equal(d["out_xyz"][:n_o], p["xyz"][L["src"][:n_o].numpy()])


def test_header_declares_the_entry_points():
    import gsrast
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    for s in ("gsr_densify_plan_scratch_bytes", "gsr_densify_plan", "gsr_densify_emit"):
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert s in gsrast.EXPORTS and hasattr(gsrast.lib(), s)
    assert "#define GSR_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "gsrast.h")).read()


def test_entry_points_validate_before_the_device():
    import ctypes as C
    import gsrast
    from gsrast import densify
    L = gsrast.lib()
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)

    def args(**kw):
        a = densify.Args()
        a.P, a.scaling_cols, a.N, a.child_div = 8, 3, 2, 1.6
        for n in ("accum", "denom", "scaling", "opacity", "max_radii2D"):
            setattr(a, n, addr)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    big = 1 << 20
    assert L.gsr_densify_plan(C.byref(args(scaling_cols=4)), addr, big, addr, None) != 0 and "scaling_cols" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args(P=-1)), addr, big, addr, None) != 0 and "P=" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args(N=0)), addr, big, addr, None) != 0 and "N=" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args(P=(1 << 30) + 5)), addr, big, addr, None) != 0 and "2^31" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args(accum=None)), addr, big, addr, None) != 0 and "null pointer" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args(accum_abs=addr)), addr, big, addr, None) != 0 and "go together" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args()), addr, 16, addr, None) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_densify_plan(C.byref(args()), addr, big, None, None) != 0 and "status_dev" in gsrast.last_error()
    counts = (C.c_uint32 * 8)(9, 0, 0, 0, 0, 0, 0, 0)
    assert L.gsr_densify_emit(C.byref(args()), addr, big, counts, 0, None, None, None) != 0 and "counts" in gsrast.last_error()
    counts = (C.c_uint32 * 8)(0, 0, 8, 0, 0, 0, 0, 0)
    t = (densify.Tensor * 1)(densify.Tensor(addr, addr, 6, 0, 0))
    assert L.gsr_densify_emit(C.byref(args()), addr, big, counts, 1, t, None, None) != 0 and "multiple of 4" in gsrast.last_error()
    assert L.gsr_densify_plan_scratch_bytes(-1, 2) == 0 and L.gsr_densify_plan_scratch_bytes(1 << 30, 3) == 0
    b1, b2 = L.gsr_densify_plan_scratch_bytes(1_000_000, 2), L.gsr_densify_plan_scratch_bytes(2_000_000, 2)
    assert 13 * 1_000_000 <= b1 <= 14 * 1_000_000 and 1.9 < b2 / b1 < 2.1        # flags 1 B + rank 4 B + map 8 B per Gaussian


def _host_model(**kw):
    p, mom, stats = DC.make_inputs(16, 3, rest=3, pgsr=kw.get("pgsr", False))
    return DC.Model(p, mom, stats, "cpu", **kw)


def test_argument_errors_without_a_device():
    from gsrast import densify
    with pytest.raises(RuntimeError, match="_xyz must be a CUDA tensor|xyz must be a CUDA tensor"):
        densify.densify_and_prune_(_host_model(), 0.0002, 0.005, 5.0, 20)
    with pytest.raises(RuntimeError, match="max_grad"):
        densify.densify_and_prune_(_host_model(), 0.0, 0.005, 5.0, 20)
    with pytest.raises(RuntimeError, match="abs_max_grad"):
        densify.densify_and_prune_(_host_model(pgsr=True), 0.0002, 0.005, 5.0, 20, abs_max_grad=-1.0)
    m = _host_model()
    del m.percent_dense
    with pytest.raises(RuntimeError, match="attribute percent_dense is missing"):
        densify.densify_and_prune_(m, 0.0002, 0.005, 5.0, 20)
    with pytest.raises(RuntimeError, match="attribute xyz_gradient_accum_abs is missing"):
        densify.densify_and_prune_(_host_model(), 0.0002, 0.005, 5.0, 20, abs_max_grad=0.0008)
    m = _host_model()
    m.optimizer.param_groups[2]["name"] = "features"
    with pytest.raises(RuntimeError, match="unknown group name 'features'"):
        densify.densify_and_prune_(m, 0.0002, 0.005, 5.0, 20)
    m = _host_model()
    m._opacity = torch.nn.Parameter(m._opacity.detach().double())
    m.optimizer.param_groups[3]["params"][0] = m._opacity
    with pytest.raises(RuntimeError, match="opacity: expected scalar type Float"):
        densify.densify_and_prune_(m, 0.0002, 0.005, 5.0, 20)
    with pytest.raises(RuntimeError, match=r"noise_split: expected 2 \* \(number of selected Gaussians\) rows"):
        densify.densify_and_prune_(_host_model(), 0.0002, 0.005, 5.0, 20, noise_split=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="noise_split: expected shape"):
        densify.densify_and_prune_(_host_model(), 0.0002, 0.005, 5.0, 20, noise_split=torch.zeros(4, 2))
    z = torch.zeros(16, 3)
    with pytest.raises(RuntimeError, match="unknown group name 'sh'"):
        densify.clone_split_prune({"xyz": z, "scaling": z, "rotation": torch.zeros(16, 4), "sh": z}, {}, z[:, 0], z[:, 0], z, z[:, 0], z[:, 0],
                                  max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01)
    with pytest.raises(RuntimeError, match="scaling: expected 2 or 3 columns"):
        densify.clone_split_prune({"xyz": z, "scaling": torch.zeros(16, 4), "rotation": torch.zeros(16, 4)}, {}, z[:, 0], z[:, 0], torch.zeros(16, 4), z[:, 0],
                                  z[:, 0], max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01)
    with pytest.raises(RuntimeError, match="denom: expected 16 entries"):
        densify.clone_split_prune({"xyz": z, "scaling": z, "rotation": torch.zeros(16, 4)}, {}, z[:, 0], z[:5, 0], z, z[:, 0], z[:, 0],
                                  max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01)
    with pytest.raises(RuntimeError, match="get_opacity must be a CUDA tensor"):
        densify.reset_opacity_(_host_model())
    with pytest.raises(RuntimeError, match="keyword argument radii is missing"):
        m = _host_model(); m.config = DC.config()
        densify.densify_(m, 600, visibility_filter=None, viewspace_points=None)
