"""GPU parity of the fused neural-Gaussian decode (gsrast.decode -> include/gsdecode.h) against the C oracle and, at full size, against
the torch transcription of the reference's op chain running on the same device."""
import numpy as np
import pytest
import torch

import decode_cases
import decode_truth
import oracle_decode
import ref_decode_torch
import visible_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_LEAVES = ("anchor", "feat", "offset", "scaling")


def _run_hip(case, dL=None):
    from gsrast import decode
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    leaves = {n: t(case[n]).requires_grad_(True) for n in GRAD_LEAVES}
    par = {n: (None if v is None else t(v).requires_grad_(True)) for n, v in case["params"].items()}
    vis = torch.tensor(case["vis_idx"], dtype=torch.int32, device=DEV)
    out = decode.neural_gaussians(leaves["anchor"], leaves["feat"], leaves["offset"], leaves["scaling"],
                                  (par["W1o"], par["b1o"], par["W2o"], par["b2o"]), (par["W1c"], par["b1c"], par["W2c"], par["b2c"]),
                                  (par["W1k"], par["b1k"], par["W2k"], par["b2k"]), t(case["campos"]), vis_idx=vis, appearance=par["app"],
                                  level=t(case["level"]), opacity_scale=t(case["opacity_scale"]), add_opacity_dist=case["dist_o"],
                                  add_cov_dist=case["dist_c"], add_color_dist=case["dist_k"], use_feat_bank="W1b" in par,
                                  mlp_feature_bank=(par["W1b"], par["b1b"], par["W2b"], par["b2b"]) if "W1b" in par else None)
    names = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity", "mask")
    res = dict(zip(names, out))
    grads = None
    if dL is not None:
        loss = sum((res[n].reshape(dL[n].shape) * torch.tensor(dL[n], device=DEV)).sum() for n in ("xyz", "color", "opacity", "scaling", "rot"))
        loss.backward()
        grads = {n: leaves[n].grad.cpu().numpy() for n in GRAD_LEAVES}
        grads.update({n: p.grad.cpu().numpy() for n, p in par.items() if p is not None})
    return {n: v.detach().cpu().numpy() for n, v in res.items()}, grads


CASES = [dict(), dict(A=0, k=5), dict(dist_o=True, dist_c=True, dist_k=True, seed=1), dict(level=True, progressive=True, seed=2),
         dict(dist_k=True, level=True, A=16, k=12, seed=3), dict(k=16, A=64, seed=4), dict(k=1, seed=5, vis_frac=1.0)]


@pytest.mark.parametrize("kw", CASES)
def test_decode_matches_oracle(kw):
    case = decode_cases.make_case(Na=3000, **kw)
    o = oracle_decode.forward(case)
    dL = decode_cases.make_out_grads(o["P"], seed=kw.get("seed", 0))
    h, _ = _run_hip(case)
    hip_mask = h["mask"].reshape(-1).astype(bool)
    mism = hip_mask != o["mask"].astype(bool)
    assert not (mism & (np.abs(o["neural_opacity"]) > 1e-5)).any()          # the gate may only differ where tanh(.) is ~0
    np.testing.assert_allclose(h["neural_opacity"].reshape(-1), o["neural_opacity"], rtol=1e-5, atol=2e-6)
    if mism.any():      # a gate flipped on a ~0 value: the compaction differs by construction, so the comparison runs WITH THE KERNEL'S GATE -- the forward
        # against the float64 chain (the C oracle's forward cannot take a gate), the gradients against the oracle's backward, which takes one
        decode_truth.gate_check(hip_mask, decode_truth.truth(case, None)[0]["neural_opacity"])
        o = dict(decode_truth.truth(case, hip_mask)[0], P=int(hip_mask.sum()))
        dL = decode_cases.make_out_grads(o["P"], seed=kw.get("seed", 0))
    assert h["xyz"].shape[0] == o["P"]
    for n in ("xyz", "color", "scaling", "rot"):
        np.testing.assert_allclose(h[n], o[n], rtol=1e-5, atol=2e-6, err_msg=n)
    np.testing.assert_allclose(h["opacity"].reshape(-1), o["opacity"], rtol=1e-5, atol=2e-6)
    _, g = _run_hip(case, dL)
    go = oracle_decode.backward(case, hip_mask, dL)
    for n, r in go.items():
        scale = np.abs(r).max() + 1e-12
        err = np.abs(g[n].reshape(r.shape) - r).max() / scale
        assert err < 1e-4, (n, err)


def test_decode_compact_visible_and_empty():
    from gsrast import decode
    g = torch.Generator().manual_seed(3)
    m = (torch.rand(100003, generator=g) < 0.37).to(DEV)
    idx = decode.compact_visible(m)
    assert torch.equal(idx.long(), torch.nonzero(m).view(-1))
    assert decode.compact_visible(torch.zeros(77, dtype=torch.bool, device=DEV)).numel() == 0
    # no visible anchors: empty outputs, zero gradients
    case = decode_cases.make_case(Na=50, seed=9)
    case["vis_idx"] = np.zeros(0, np.int32)
    h, g_ = _run_hip(case, decode_cases.make_out_grads(0))
    assert h["xyz"].shape == (0, 3) and h["mask"].size == 0
    assert all(not np.any(v) for v in g_.values())


def test_decode_full_size_vs_torch_chain():
    """100k anchors / 1M candidate Gaussians: the HIP decode against the reference's op chain run by torch on the same GPU (fp32)."""
    case = decode_cases.make_case(Na=100000, seed=11, vis_frac=0.6)
    h, _ = _run_hip(case)
    mask = h["mask"].astype(bool)
    ref, leaves = ref_decode_torch.decode(case, dtype=torch.float32, mask_override=mask, device=DEV)
    P = int(mask.sum())
    assert h["xyz"].shape[0] == P and 0.3 < P / mask.size < 0.7
    nop = ref["neural_opacity"].detach().cpu().numpy()
    assert not ((nop > 0) != mask)[np.abs(nop) > 1e-5].any()
    for n in ("xyz", "color", "scaling", "rot"):
        np.testing.assert_allclose(h[n], ref[n].detach().cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
    dL = decode_cases.make_out_grads(P, seed=11)
    _, g = _run_hip(case, dL)
    gr = ref_decode_torch.backward(ref, leaves, dL, device=DEV)
    for n, v in g.items():
        r = gr[n]
        rel = np.linalg.norm((v.reshape(r.shape) - r).ravel()) / (np.linalg.norm(r.ravel()) + 1e-20)
        assert rel < 1e-4, (n, rel)


@pytest.mark.parametrize("mode", ["floor", "round", "ceil", "progressive"])
def test_octree_visible_matches_oracle(mode):
    """gsr_octree_visible = LOD mask (oracle refd_lod_mask) composed with the prefilter (oracle ref_visible_filter on the masked anchors)."""
    import oracle
    import scenes
    import hiprun
    import scaffold_filter
    from gsrast import octree
    W, H, Na, levels = 640, 368, 30000, 6
    sc = scenes.make_scene("ewa", Na, W, H, seed=17)
    r = np.random.default_rng(17)
    level = r.integers(0, levels, Na).astype(np.int32); extra = r.uniform(-0.3, 0.3, Na).astype(np.float32)
    vs, fork, sd = 0.5, 2.0, 10.0
    m, pr, tr = oracle_decode.lod_mask(sc["means3D"], level, extra, sc["campos"], vs, fork, sd, 1.0, levels,
                                       ["floor", "round", "ceil", "progressive"].index(mode))
    sub = dict(sc); sub["means3D"] = sc["means3D"][m]; sub["scales"] = sc["scales"][m]; sub["rotations"] = sc["rotations"][m]
    sub["opacities"] = sc["opacities"][m]
    for k in ("colors_precomp", "shs"):
        if sub.get(k) is not None:
            sub[k] = sub[k][m]
    rad = np.zeros(Na, np.int32); rad[m] = oracle.visible_filter(sub)
    t = hiprun.to_dev(sc, DEV)
    rs = hiprun.settings("ewa", t)
    fs = scaffold_filter.GaussianRasterizationSettings(**rs._asdict())
    scal6 = torch.cat([t["scales"], t["scales"]], dim=1)                      # get_scaling-shaped (Na,6): the kernel reads the first three
    out = octree.octree_visible(fs, t["means3D"], torch.tensor(level, device=DEV).unsqueeze(1), scal6, t["rotations"], vs, fork, sd, levels,
                                dist2level=mode, extra_level=torch.tensor(extra, device=DEV))
    hm = out["anchor_mask"].cpu().numpy()
    flips = hm != m
    # a flip is allowed only where the float64 truth puts pred within its measured float32 bound of a rounding boundary (tests/visible_truth.py)
    truth = visible_truth.lod(sc["means3D"], level, extra, sc["campos"], vs, fork, sd, 1.0, levels, mode)
    frag = truth["margin"] <= visible_truth.BOUND["pred"]
    print(f"{mode}: fragile {int(frag.sum())} of {Na}, device flips against the oracle {int(flips.sum())}")
    assert frag.mean() < 2e-4 and not (flips & ~frag).any()
    assert np.array_equal(hm[~frag], truth["anchor_mask"][~frag])
    ok = ~flips
    assert np.array_equal(out["radii"].cpu().numpy()[ok], rad[ok])
    assert np.array_equal(out["visible_mask"].cpu().numpy()[ok], (rad > 0)[ok]) and out["visible_mask"].any()
    if mode == "progressive":
        assert np.abs(out["prog_ratio"].cpu().numpy().ravel() - pr)[~frag].max() < 1e-3
        assert not ((out["transition_mask"].cpu().numpy() != tr) & ~frag).any()


def test_padded_visible_list_gives_identical_gaussians_without_the_count_sync():
    """compact_visible(mask, padded=True): Na entries, -1 behind the visible indices, no host synchronisation.  The decode must emit exactly
    the Gaussians of the exact list (bit-identical outputs, equal gradients), write zero neural_opacity / mask rows for the padding, and the
    statistics kernel must skip the padding rows."""
    from gsrast import decode
    case = decode_cases.make_case(Na=5000, seed=9, vis_frac=0.6)
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    vmask = torch.zeros(5000, dtype=torch.bool, device=DEV); vmask[torch.tensor(case["vis_idx"], dtype=torch.long, device=DEV)] = True
    res = []
    for padded in (False, True):
        leaves = {n: t(case[n]).requires_grad_(True) for n in GRAD_LEAVES}
        par = {n: (None if v is None else t(v).requires_grad_(True)) for n, v in case["params"].items()}
        vis = decode.compact_visible(vmask, padded=padded)
        out = decode.neural_gaussians(leaves["anchor"], leaves["feat"], leaves["offset"], leaves["scaling"],
                                      (par["W1o"], par["b1o"], par["W2o"], par["b2o"]), (par["W1c"], par["b1c"], par["W2c"], par["b2c"]),
                                      (par["W1k"], par["b1k"], par["W2k"], par["b2k"]), t(case["campos"]), vis_idx=vis, appearance=par["app"])
        loss = sum((o * (i + 1.0)).sum() for i, o in enumerate(out[:5]))
        loss.backward()
        acc = [torch.zeros(5000, 1, device=DEV), torch.zeros(5000, 1, device=DEV), torch.zeros(5000 * case["k"], 1, device=DEV), torch.zeros(5000 * case["k"], 1, device=DEV)]
        P = out[0].shape[0]
        g2 = torch.rand(P, 3, generator=torch.Generator().manual_seed(1)).to(DEV); upd = (torch.arange(P, device=DEV) % 3) != 0
        decode.training_stats_(*acc, g2, out[5], upd, out[6], vis_idx=vis)
        res.append((vis, [o.detach() for o in out], {n: v.grad for n, v in leaves.items()}, {n: v.grad for n, v in par.items() if v is not None}, acc))
    (v0, o0, gl0, gp0, a0), (v1, o1, gl1, gp1, a1) = res
    Nv, k = v0.numel(), case["k"]
    assert v1.numel() == 5000 and torch.equal(v1[:Nv], v0) and bool((v1[Nv:] == -1).all())
    for a, b in zip(o0[:5], o1[:5]):
        assert torch.equal(a, b)
    assert torch.equal(o1[5][:Nv * k], o0[5]) and float(o1[5][Nv * k:].abs().max()) == 0.0 and not bool(o1[6][Nv * k:].any())
    for n in gl0:
        assert torch.allclose(gl0[n], gl1[n], rtol=1e-5, atol=1e-6), n
    for n in gp0:
        assert torch.allclose(gp0[n], gp1[n], rtol=1e-4, atol=1e-5), n
    for a, b in zip(a0, a1):
        assert torch.equal(a, b)


def test_deferred_decode_two_in_flight_equal_the_synchronous_calls():
    """neural_gaussians(..., deferred=True): the kernels are enqueued, the count is read at finish().  Two decodes of different cameras / visible sets
    in flight at once, finished in order, give bit-identical outputs and the same gradients as two synchronous calls; finish() twice is an error."""
    from gsrast import decode
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    cases = [decode_cases.make_case(Na=6000, seed=21, vis_frac=0.55), decode_cases.make_case(Na=6000, seed=22, vis_frac=0.8)]

    def run(deferred):
        leaves, pars, pend = [], [], []
        for case in cases:
            lv = {n: t(case[n]).requires_grad_(True) for n in GRAD_LEAVES}
            par = {n: (None if v is None else t(v).requires_grad_(True)) for n, v in case["params"].items()}
            vis = torch.tensor(case["vis_idx"], dtype=torch.int32, device=DEV)
            out = decode.neural_gaussians(lv["anchor"], lv["feat"], lv["offset"], lv["scaling"],
                                          (par["W1o"], par["b1o"], par["W2o"], par["b2o"]), (par["W1c"], par["b1c"], par["W2c"], par["b2c"]),
                                          (par["W1k"], par["b1k"], par["W2k"], par["b2k"]), t(case["campos"]), vis_idx=vis, appearance=par["app"],
                                          deferred=deferred)
            leaves.append(lv); pars.append(par); pend.append(out)
        if deferred:
            assert all(isinstance(p, decode.PendingDecode) for p in pend)
            outs = [p.finish() for p in pend]
            with pytest.raises(RuntimeError, match="twice"):
                pend[0].finish()
        else:
            outs = pend
        loss = sum((o * (i + 1.0)).sum() for out in outs for i, o in enumerate(out[:5]))
        loss.backward()
        return outs, leaves, pars

    o0, l0, p0 = run(False)
    o1, l1, p1 = run(True)
    for a, b in zip(o0, o1):
        assert len(a) == len(b) == 7 and a[0].shape[0] > 1000
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y)
    for a, b in zip(l0 + p0, l1 + p1):
        for n in a:
            if a[n] is not None:
                assert torch.allclose(a[n].grad, b[n].grad, rtol=1e-5, atol=1e-6), n


def test_deferred_decode_saves_the_buffers_its_kernels_read_and_returns_its_slot():
    """ADVICE r4.  (1) With arguments that need a copy (non-contiguous anchor and feat views) the deferred decode's autograd node keeps the very
    copies its enqueued kernels read -- modifying the ORIGINALS between the launch and finish() changes neither the outputs nor the gradients (the node no
    longer converts the arguments a second time at finish()).  (2) A PendingDecode that is dropped unfinished gives its pinned count slot back."""
    import gc
    from gsrast import decode
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    case = decode_cases.make_case(Na=5000, seed=31, vis_frac=0.6)
    par = {n: (None if v is None else t(v)) for n, v in case["params"].items()}
    vis = torch.tensor(case["vis_idx"], dtype=torch.int32, device=DEV)
    heads = ((par["W1o"], par["b1o"], par["W2o"], par["b2o"]), (par["W1c"], par["b1c"], par["W2c"], par["b2c"]), (par["W1k"], par["b1k"], par["W2k"], par["b2k"]))

    def leaves():
        anchor64 = torch.zeros(case["anchor"].shape[0], 6, device=DEV)                     # the anchors are every other column of this one: a strided view
        anchor64[:, ::2] = t(case["anchor"]); anchor64.requires_grad_(True)
        wide = torch.zeros(case["feat"].shape[0], 2 * case["feat"].shape[1], device=DEV)
        wide[:, ::2] = t(case["feat"]); wide.requires_grad_(True)
        return anchor64, wide, t(case["offset"]).requires_grad_(True), t(case["scaling"]).requires_grad_(True)

    def run(deferred, clobber):
        anchor64, wide, offset, scaling = leaves()
        feat_view = wide[:, ::2]                                                           # non-contiguous
        out = decode.neural_gaussians(anchor64[:, ::2], feat_view, offset, scaling, *heads, t(case["campos"]), vis_idx=vis, appearance=par["app"], deferred=deferred)
        if deferred:
            if clobber:
                with torch.no_grad():
                    anchor64.add_(100.0); wide.mul_(0.0)                                   # the originals change; the launched copies must not care
            out = out.finish()
        sum((o * (i + 1.0)).sum() for i, o in enumerate(out[:5])).backward()
        return out, (anchor64.grad.clone(), wide.grad.clone(), offset.grad.clone(), scaling.grad.clone())

    o0, g0 = run(False, False)
    o1, g1 = run(True, True)
    for x, y in zip(o0, o1):
        assert torch.equal(x, y)
    for a, b in zip(g0, g1):
        assert torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)
    dev = torch.cuda.current_device()
    free0 = len(decode._count_slots.get(dev, []))
    anchor64, wide, offset, scaling = leaves()
    pend = decode.neural_gaussians(anchor64[:, ::2].contiguous(), wide[:, ::2].contiguous(), offset, scaling, *heads, t(case["campos"]), vis_idx=vis, appearance=par["app"], deferred=True)
    assert len(decode._count_slots.get(dev, [])) == max(free0 - 1, 0)
    del pend; gc.collect()
    assert len(decode._count_slots.get(dev, [])) == max(free0, 1)
