"""The fused neural-Gaussian decode (csrc/gsd_decode.hip through gsrast.decode) against the float64 truth of decode_truth at the edges of its
fixed-size pieces: 16-anchor tiles, 64-anchor weight-gradient chunks, 256-row backward padding, 1024-word scan workgroups and their 64-wide look-back,
the grid caps of the tile kernels, every k and the odd appearance widths, all flag combinations, gates all closed / all open / closed by whole tiles,
an invisible anchor at the camera centre, and the padded / deferred / static entry points at ragged sizes.  Every figure is printed (pytest -s)
beside the float32 floor before it is asserted."""
import numpy as np
import pytest
import torch

import decode_cases
import decode_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_LEAVES = ("anchor", "feat", "offset", "scaling")
OUT7 = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity", "mask")


def _t(a):
    return None if a is None else torch.tensor(a, device=DEV)


def _launch(case, vis=None, **kw):
    """-> (the tuple neural_gaussians returns, leaves, parameters).  vis: int32 device tensor (default: the case's exact list)"""
    from gsrast import decode
    leaves = {n: _t(case[n]).requires_grad_(True) for n in GRAD_LEAVES}
    par = {n: (None if v is None else _t(v).requires_grad_(True)) for n, v in case["params"].items()}
    if vis is None:
        vis = torch.tensor(case["vis_idx"], dtype=torch.int32, device=DEV)
    out = decode.neural_gaussians(leaves["anchor"], leaves["feat"], leaves["offset"], leaves["scaling"],
                                  (par["W1o"], par["b1o"], par["W2o"], par["b2o"]), (par["W1c"], par["b1c"], par["W2c"], par["b2c"]),
                                  (par["W1k"], par["b1k"], par["W2k"], par["b2k"]), _t(case["campos"]), vis_idx=vis, appearance=par["app"],
                                  level=_t(case["level"]), opacity_scale=_t(case["opacity_scale"]), add_opacity_dist=case["dist_o"],
                                  add_cov_dist=case["dist_c"], add_color_dist=case["dist_k"], **kw)
    return out, leaves, par


def _backward(out, P, dL, leaves, par):
    """loss = sum <out[:P], dL> over the five Gaussian tensors -> gradients of every leaf and parameter (numpy)"""
    loss = sum((out[i][:P].reshape(dL[n].shape) * _t(dL[n])).sum() for i, n in enumerate(decode_truth.OUT_NAMES))
    loss.backward()
    g = {n: leaves[n].grad.cpu().numpy() for n in GRAD_LEAVES}
    g.update({n: p.grad.cpu().numpy() for n, p in par.items() if p is not None})
    return g


def _np(out, Nvk=None):
    """the returned tuple as numpy; neural_opacity / mask cut to the Nv*k rows of the visible anchors (the padded forms carry zero rows behind them)"""
    d = {n: v.detach().cpu().numpy() for n, v in zip(OUT7, out)}
    d["neural_opacity"] = d["neural_opacity"].reshape(-1); d["mask"] = d["mask"].reshape(-1).astype(bool)
    if Nvk is not None:
        assert not d["neural_opacity"][Nvk:].any() and not d["mask"][Nvk:].any()
        d["neural_opacity"] = d["neural_opacity"][:Nvk]; d["mask"] = d["mask"][:Nvk]
    d["opacity"] = d["opacity"].reshape(-1)
    return d


def _decode_and_compare(label, case, seed, vis=None, large=False, device="cpu"):
    """one forward + one backward of the sync path, everything against truth(case, the kernel's own gate) -> (outputs, gradients, P)"""
    Nvk = case["vis_idx"].size * case["k"]
    out, leaves, par = _launch(case, vis)
    h = _np(out, Nvk)
    P = int(h["mask"].sum())
    assert h["mask"].size == Nvk and h["xyz"].shape == (P, 3) and h["rot"].shape == (P, 4) and h["opacity"].shape == (P,)
    flips = decode_truth.gate_check(h["mask"], decode_truth.truth(case, None, device=device)[0]["neural_opacity"])
    print(f"DECODE-TRUTH {label}: Nv {case['vis_idx'].size} k {case['k']} P {P} gates differing from float64 {flips}")
    dL = decode_cases.make_out_grads(P, seed=seed)
    g = _backward(out, P, dL, leaves, par)
    for n, v in list(h.items()) + list(g.items()):
        assert np.isfinite(v).all(), (label, n, int((~np.isfinite(v)).sum()))
    decode_truth.compare(label, h, g, case, h["mask"], dL, large=large, device=device)
    return h, g, P, dL


@pytest.mark.parametrize("entry", decode_truth.MATRIX, ids=decode_truth.MATRIX_IDS)
def test_matrix_case_matches_float64_truth(entry):
    case = decode_truth.matrix_case(entry)
    _, g, P, _ = _decode_and_compare(entry[0], case, entry[2])
    hidden = np.setdiff1d(np.arange(case["anchor"].shape[0]), case["vis_idx"])
    assert hidden.size and all(not g[n][hidden].any() for n in GRAD_LEAVES)          # invisible anchors: exact zero rows


def test_all_gates_closed_gives_empty_outputs_and_exact_zero_gradients():
    """P = 0 with Nv > 0.  The float64 chain returns zero gradients for every leaf and parameter (test_decode_truth_cpu); so must the backward."""
    case = decode_truth.special_case("closed")
    out, leaves, par = _launch(case)
    h = _np(out)
    assert not h["mask"].any() and h["mask"].size == 333 * case["k"]
    assert all(h[n].shape[0] == 0 for n in decode_truth.OUT_NAMES)
    t_out, _ = decode_truth.truth(case, h["mask"])
    e, x = decode_truth.fwd_err(h["neural_opacity"], t_out["neural_opacity"])
    print(f"DECODE-TRUTH closed fwd neural_opacity: max|d| {e:.3e} of-bar {x:.3f}")
    assert x <= 1.0
    g = _backward(out, 0, decode_cases.make_out_grads(0), leaves, par)
    assert set(g) == set(GRAD_LEAVES) | {n for n, v in case["params"].items() if v is not None}
    for n, v in g.items():
        assert v.shape == np.shape(case[n] if n in GRAD_LEAVES else case["params"][n]) and not np.any(v), n      # exact zeros (NaN counts as non-zero)


def test_all_gates_open_emits_every_offset_in_order():
    case = decode_truth.special_case("open")
    h, _, P, _ = _decode_and_compare("open", case, 202)
    k = case["k"]
    assert P == 333 * k and h["mask"].all()
    a = np.repeat(case["vis_idx"], k); j = np.tile(np.arange(k), 333)                 # rows in (v, j) order
    np.testing.assert_allclose(h["xyz"], case["anchor"][a] + case["offset"][a, j] * case["scaling"][a, :3], rtol=1e-6, atol=1e-6)


def test_whole_anchors_and_whole_tiles_closed():
    """opacity_scale = 0 (exact on both sides) on visible rows 16..47 and every third row elsewhere: row_offset across empty anchors and empty tiles"""
    case = decode_truth.special_case("holes")
    h, _, P, _ = _decode_and_compare("holes", case, 203)
    per_anchor = h["mask"].reshape(333, -1).sum(1)
    assert not per_anchor[16:48].any() and not per_anchor[::3].any() and (per_anchor == 0).sum() >= 133 and P == per_anchor.sum() > 0


@pytest.mark.parametrize("padded", [False, True], ids=["exact", "padded"])
def test_invisible_anchor_at_the_camera_centre_is_never_read(padded):
    """Inactive rows (past Nv in the last tile, -1 rows of a padded list, the backward's padding to 256 rows) point at anchor 0.  With anchor 0 at the
    camera centre its view vector is 0/0; nothing of it may reach an output or a gradient (the truth never touches an invisible anchor)."""
    from gsrast import decode
    case = decode_truth.camera_centre_case()
    vis = None
    if padded:
        m = torch.zeros(case["anchor"].shape[0], dtype=torch.bool, device=DEV)
        m[torch.tensor(case["vis_idx"], dtype=torch.long, device=DEV)] = True
        vis = decode.compact_visible(m, padded=True)
        assert vis.numel() == case["anchor"].shape[0] and int((vis >= 0).sum()) == 17
    _, g, _, _ = _decode_and_compare("camera-centre " + ("padded" if padded else "exact"), case, 204, vis=vis)
    assert not any(g[n][0].any() for n in GRAD_LEAVES)


@pytest.mark.parametrize("Nv", [17, 1025])
@pytest.mark.parametrize("mode", ["padded", "deferred", "static_rows"])
def test_other_entry_points_at_ragged_sizes(mode, Nv):
    """The padded list, the deferred count and the static-row form against the sync path with the exact list: the first P rows bit for bit, the
    gradients within the gradient bar; the static form parks its surplus rows at the camera centre and reports count == P."""
    from gsrast import decode
    case = decode_truth.edge_case(Nv, 300 + Nv)
    Na, k = case["anchor"].shape[0], case["k"]
    out0, lv0, par0 = _launch(case)
    h0 = _np(out0, Nv * k)
    P = int(h0["mask"].sum())
    dL = decode_cases.make_out_grads(P, seed=Nv)
    g0 = _backward(out0, P, dL, lv0, par0)
    m = torch.zeros(Na, dtype=torch.bool, device=DEV); m[torch.tensor(case["vis_idx"], dtype=torch.long, device=DEV)] = True
    if mode == "padded":
        vis = decode.compact_visible(m, padded=True)
        assert vis.numel() == Na and torch.equal(vis[:Nv].cpu(), torch.tensor(case["vis_idx"])) and bool((vis[Nv:] == -1).all())
        out1, lv1, par1 = _launch(case, vis)
    elif mode == "deferred":
        pend, lv1, par1 = _launch(case, deferred=True)
        assert isinstance(pend, decode.PendingDecode)
        out1 = pend.finish()
    else:
        out1, lv1, par1 = _launch(case, decode.compact_visible(m, padded=True), static_rows=True)
        assert len(out1) == 8 and int(out1[7].item()) == P and out1[7].dtype == torch.int32
        cap = Na * k
        assert all(out1[i].shape[0] == cap for i in range(5))
        campos = _t(case["campos"])
        assert torch.equal(out1[0][P:], campos.expand(cap - P, 3)) and not bool(out1[2][P:].any()) and not bool(out1[1][P:].any()) and not bool(out1[3][P:].any())
        assert torch.equal(out1[4][P:], torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).expand(cap - P, 4))
    h1 = _np(out1[:7], Nv * k)
    assert np.array_equal(h1["mask"], h0["mask"]) and np.array_equal(h1["neural_opacity"], h0["neural_opacity"])
    for n in decode_truth.OUT_NAMES:
        assert h1[n].shape[0] == (P if mode != "static_rows" else Na * k)
        assert np.array_equal(h1[n][:P], h0[n]), (mode, n)
    g1 = _backward(out1, P, dL, lv1, par1)
    assert set(g1) == set(g0)
    for n in g0:
        e = decode_truth.grad_err(g1[n], g0[n])
        print(f"DECODE-TRUTH {mode} Nv{Nv} grad {n} vs sync path: max|d|/max|ref| {e:.3e}")
        assert e < decode_truth.GRAD_BAR, (mode, n, e)


def _stats_check(label, case, h, P, vis=None):
    """decode.training_stats_ on the decode's own neural_opacity / mask against the float64 restatement of training_statis.  Counts are exact.  Sums: the
    kernel adds k <= 16 non-negative float32 terms one after the other and then adds that to the accumulator (a float32 sqrt of a sum of two squares for
    the gradient norm): at most (k + 1) roundings of 2^-24 relative to the non-negative result, < 2e-6."""
    from gsrast import decode
    k, Na = case["k"], case["anchor"].shape[0]
    r = np.random.default_rng(P + 1)
    grad = r.normal(0, 1, (P, 3)).astype(np.float32); upd = r.uniform(size=P) < 0.6
    acc0 = [r.uniform(0, 2, n).astype(np.float32) for n in (Na, Na, Na * k, Na * k)]
    acc0[1] = np.floor(acc0[1] * 8).astype(np.float32); acc0[3] = np.floor(acc0[3] * 8).astype(np.float32)       # the two counters hold integers
    dev = [_t(a).reshape(-1, 1) for a in acc0]
    v = torch.tensor(case["vis_idx"], dtype=torch.int32, device=DEV) if vis is None else vis
    decode.training_stats_(*dev, _t(grad), _t(h["neural_opacity"]), _t(upd), _t(h["mask"]), vis_idx=v)
    acc64 = [a.astype(np.float64) for a in acc0]
    decode_truth.training_statis64(acc64, k, case["vis_idx"], h["neural_opacity"], h["mask"], upd, grad)
    got = [d.cpu().numpy().reshape(-1) for d in dev]
    assert np.array_equal(got[1], acc64[1]) and np.array_equal(got[3], acc64[3]), label
    for i in (0, 2):
        e = np.abs(got[i] - acc64[i]) / np.abs(acc64[i]).clip(1e-30)
        print(f"DECODE-TRUTH {label} training_stats accumulator {i}: max relative error {e.max():.3e}")
        np.testing.assert_allclose(got[i], acc64[i], rtol=2e-6, atol=0)
    assert int((acc64[3] != acc0[3]).sum()) > 0 or P == 0


@pytest.mark.parametrize("Nv", [255, 256, 257])
def test_training_stats_at_the_block_edge(Nv):
    entry = decode_truth.MATRIX[decode_truth.MATRIX_IDS.index(f"Nv{Nv}")]
    case = decode_truth.matrix_case(entry)
    out, _, _ = _launch(case)
    h = _np(out, Nv * case["k"])
    _stats_check(f"Nv{Nv}", case, h, int(h["mask"].sum()))


def test_beyond_every_grid_cap_and_scan_sweep():
    """Nv >= 270 000 visible anchors: more than 131 072 rows for stage 1 (2048 blocks x 4 tiles x 16), 65 536 for the emit kernel, 32 768 for the
    backward heads -- every tile kernel takes its grid-stride loop again; 264+ scan workgroups, i.e. more than 64 look-back predecessors (the q += 64
    step); more than 1024 block sums for the statistics scan (k_scan_small: two per thread).  Truth: the float64 chain run by torch on the device; floor: the float32 chain there.  The case leaves out the
    anchors whose float64 hidden pre-activations touch the ReLU kink (decode_truth.large_case says why and what was measured with them in)."""
    case = decode_truth.large_case()
    Nv = case["vis_idx"].size
    assert Nv >= 270000 and (Nv + 1023) // 1024 > 64 + 1 and (Nv + 255) // 256 > 1024
    h, _, P, _ = _decode_and_compare("large", case, 401, large=True, device=DEV)
    assert 0.3 < P / h["mask"].size < 0.7
    torch.cuda.empty_cache()
    _stats_check("large", case, h, P)
