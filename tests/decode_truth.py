"""Edge-case matrix and float64 truth for the fused neural-Gaussian decode (csrc/gsd_decode.hip).  TEST INFRASTRUCTURE ONLY.

The kernels are built from fixed-size pieces: 16-anchor MFMA tiles, 64-anchor weight-gradient chunks, a backward padded to 256 rows, 1024-word scan
workgroups, offsets handled in lane pairs / groups of four, an appearance vector folded into a bias column, a column map for the optional inputs.  MATRIX
walks each of those axes one at a time across its edges; `truth` is the float64 torch transcription of the reference's op chain
(ref_decode_torch) evaluated WITH THE GATE OF THE CODE UNDER TEST (mask_override), so outputs and gradients are comparable for every seed, and
`gate_check` bounds how far that gate may differ from the float64 one.  `floor` is the same chain in float32: what plain float32 arithmetic costs.

Bars (tests/test_gpu_decode.py's own, here against float64): forward rtol 1e-5 / atol 2e-6; gradients max|d| / max|ref| < 1e-4; the large case
relative L2 < 1e-4."""
import itertools

import numpy as np
import torch

import decode_cases
import ref_decode_torch

FWD_RTOL, FWD_ATOL, GRAD_BAR, L2_BAR = 1e-5, 2e-6, 1e-4, 1e-4
GATE_EPS = 1e-5          # a gate may differ from the float64 one only where |tanh(.) * scale| is below this
OUT_NAMES = ("xyz", "color", "opacity", "scaling", "rot")
FWD_NAMES = ("neural_opacity",) + OUT_NAMES


def edge_case(Nv, seed, **kw):
    """make_case with Na = Nv + 1 + seed % 5 anchors of which exactly Nv (a sorted random subset) are visible."""
    Na = Nv + 1 + seed % 5
    case = decode_cases.make_case(Na=Na, seed=seed, **kw)
    r = np.random.default_rng(7000 + seed)
    case["vis_idx"] = np.sort(r.choice(Na, Nv, replace=False)).astype(np.int32)
    return case


def _matrix():
    rows = []
    for Nv in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):       # tile 16, chunk 64, backward padding 256, scan workgroup 1024
        rows.append((f"Nv{Nv}", Nv, {}))
    for k in range(1, 17):                                                               # lane pairs of the cov head, (k+1)>>1 / (k+3)>>2 output tiles
        rows.append((f"k{k}", 333, dict(k=k)))
    for A in (0, 1, 3, 31, 33, 64):                                                      # appearance width folded into the bias column
        rows.append((f"A{A}", 333, dict(A=A)))
    for do, dc, dk, lv in itertools.product((False, True), repeat=4):                    # the column map of the optional inputs
        rows.append((f"flags{int(do)}{int(dc)}{int(dk)}{int(lv)}", 333, dict(dist_o=do, dist_c=dc, dist_k=dk, level=lv, progressive=lv)))
    return [(name, Nv, 101 + i, kw) for i, (name, Nv, kw) in enumerate(rows)]


MATRIX = _matrix()
MATRIX_IDS = [m[0] for m in MATRIX]


def matrix_case(entry):
    _, Nv, seed, kw = entry
    return edge_case(Nv, seed, **kw)


def special_case(name):
    """The gate pushed to its ends.  The bias is +-1.5 (|tanh| ~ 0.9), not larger: with a bias like +-10 tanhf saturates to +-1 in float32, the opacity
    head's gradient becomes 0 against ~1e-8 and a relative comparison of dW2o means nothing."""
    if name in ("closed", "open"):
        case = edge_case(333, 201 if name == "closed" else 202)
        p = case["params"]
        p["W2o"] = (p["W2o"] * 0.1).astype(np.float32)
        p["b2o"] = np.full_like(p["b2o"], -1.5 if name == "closed" else 1.5)
        return case
    if name == "holes":       # visible rows 16..47 (two whole 16-row tiles) and every third row elsewhere emit nothing: opacity_scale is exactly 0 there
        case = edge_case(333, 203, level=True, progressive=True)
        v = np.arange(333)
        shut = ((v >= 16) & (v < 48)) | (v % 3 == 0)
        case["opacity_scale"][case["vis_idx"][shut]] = 0.0
        return case
    raise KeyError(name)


def camera_centre_case():
    """Nv = 17 (a ragged tile); anchor 0 is NOT visible and sits exactly at the camera centre, so its view vector is 0/0."""
    case = edge_case(17, 204)
    r = np.random.default_rng(204)
    case["vis_idx"] = np.sort(r.choice(np.arange(1, case["anchor"].shape[0]), 17, replace=False)).astype(np.int32)
    case["anchor"][0] = case["campos"]
    return case


def hidden_margin(case):
    """float64: per visible anchor, the smallest |pre-activation| over the 3 x 32 hidden units of the three heads.  ReLU' jumps at 0, so a unit whose
    float64 pre-activation is within float32 rounding of 0 may legitimately sit on the other side in the kernel; the gradients then differ by that unit's
    whole contribution -- the hidden layer's counterpart of the opacity gate."""
    vis = np.asarray(case["vis_idx"], np.int64)
    p = {n: np.asarray(v, np.float64) for n, v in case["params"].items() if v is not None}
    ob = case["anchor"][vis].astype(np.float64) - case["campos"].astype(np.float64)
    dist = np.linalg.norm(ob, axis=1, keepdims=True)
    lvl = [] if case["level"] is None else [case["level"][vis].astype(np.float64)[:, None]]
    base = [case["feat"][vis].astype(np.float64), ob / dist]
    margin = np.full(vis.size, np.inf)
    for hd, flag in (("o", case["dist_o"]), ("c", case["dist_c"]), ("k", case["dist_k"])):
        x = np.concatenate(base + ([dist] if flag else []) + lvl, axis=1)
        if hd == "k" and "app" in p:
            x = np.concatenate([x, np.broadcast_to(p["app"], (vis.size, p["app"].size))], axis=1)
        margin = np.minimum(margin, np.abs(x @ p["W1" + hd].T + p["b1" + hd]).min(axis=1))
    return margin


RELU_EPS = 1e-5          # = GATE_EPS: far above the float32 rounding of a 35..100-term dot product of O(1) values (~1e-6), far below the spread of the
                         # pre-activations (std ~0.5): about 1.6 anchors in 1000 have a unit that close to 0


def large_case():
    """Beyond every grid cap and scan sweep: 380 000 anchors, ~273 000 visible (k = 10).  With 26 million hidden units a handful have a float64
    pre-activation below 1e-7, i.e. inside float32 rounding of the ReLU kink, and ONE such unit on the other side moves db1 / dW1 of its head by
    |dh| / ||db1|| ~ 0.1 / (37 sqrt(32)) ~ 5e-4 (relative L2) -- the reference is not well defined there.  Measured on an MI355X with all 273 705 anchors
    in: W1k 3.1e-4, b1k 4.0e-4, app 4.1e-4 (bar 1e-4; float32 chain 4.7e-6, 2.5e-7, 2.9e-7), feat 2.0e-5, every other gradient and output at
    1e-7..1e-6; the float64 chain has one colour-head unit at |pre| = 7.6e-8 (visible row 266 508).  So the anchors with a hidden unit within RELU_EPS
    of 0 in float64 (a property of the inputs alone, ~0.16 % of them) are taken out of the visible list; the bar is unchanged."""
    case = decode_cases.make_case(Na=380000, seed=401, vis_frac=0.72)
    keep = hidden_margin(case) >= RELU_EPS
    assert keep.mean() > 0.995, keep.mean()
    case["vis_idx"] = case["vis_idx"][keep]
    return case


def _chain(case, mask, dL, dtype, device):
    out, leaves = ref_decode_torch.decode(case, dtype=dtype, mask_override=None if mask is None else np.asarray(mask, dtype=bool), device=device)
    outs = {n: v.detach().cpu().numpy() for n, v in out.items()}
    grads = None
    if dL is not None:
        grads = ref_decode_torch.backward(out, leaves, dL, device=device)
        grads = {n: (np.zeros(tuple(leaves[n].shape), outs["xyz"].dtype) if g is None else g) for n, g in grads.items()}
    return outs, grads


def truth(case, mask, dL=None, device="cpu"):
    """float64 chain with the given gate (None: its own) -> (outputs, autograd gradients for the output gradients dL or None)."""
    return _chain(case, mask, dL, torch.float64, device)


def floor(case, mask, dL=None, device="cpu"):
    """the same chain in float32"""
    return _chain(case, mask, dL, torch.float32, device)


def near_zero(nop64):
    return np.abs(np.asarray(nop64).reshape(-1)) < GATE_EPS


def gate_check(mask_hip, nop64):
    """The gate under test against the float64 pre-gate opacity: it may differ from nop64 > 0 only where |nop64| < 1e-5, and no more gates may differ
    than the float64 reference has such near-zero entries.  -> number of differing gates."""
    nop64 = np.asarray(nop64).reshape(-1)
    m = np.asarray(mask_hip).reshape(-1).astype(bool)
    assert m.shape == nop64.shape, (m.shape, nop64.shape)
    diff = m != (nop64 > 0)
    near = near_zero(nop64)
    assert not (diff & ~near).any(), f"{int((diff & ~near).sum())} gates differ where |nop64| >= {GATE_EPS}"
    assert int(diff.sum()) <= int(near.sum()), (int(diff.sum()), int(near.sum()))
    return int(diff.sum())


def fwd_err(a, ref):
    """-> (max |a - ref|, max |a - ref| / (atol + rtol |ref|)): the second is <= 1 exactly when assert_allclose(rtol, atol) passes"""
    a = np.asarray(a, np.float64).reshape(-1); ref = np.asarray(ref, np.float64).reshape(-1)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0, 0.0
    d = np.abs(a - ref)
    return float(np.nan_to_num(d, nan=np.inf).max()), float(np.nan_to_num(d / (FWD_ATOL + FWD_RTOL * np.abs(ref)), nan=np.inf).max())


def grad_err(a, ref):
    """max |a - ref| / max |ref|"""
    a = np.asarray(a, np.float64).reshape(-1); ref = np.asarray(ref, np.float64).reshape(-1)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.nan_to_num(np.abs(a - ref), nan=np.inf).max() / (np.abs(ref).max() + 1e-12)) if a.size else 0.0


def l2_err(a, ref):
    a = np.asarray(a, np.float64).reshape(-1); ref = np.asarray(ref, np.float64).reshape(-1)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = np.linalg.norm(a - ref)
    return float(d / (np.linalg.norm(ref) + 1e-20)) if np.isfinite(d) else float("inf")


def compare(label, got, got_grads, case, mask, dL, large=False, device="cpu"):
    """Outputs `got` (neural_opacity, the five Gaussian tensors) and gradients `got_grads` of the code under test against truth(case, mask, dL), with
    the float32 floor printed beside every figure.  All figures are printed before anything is asserted.  large=True: relative L2 for everything."""
    t_out, t_g = truth(case, mask, dL, device)
    f_out, f_g = floor(case, mask, dL, device)
    bad = []
    for n in FWD_NAMES:
        if large:
            e, fl = l2_err(got[n], t_out[n]), l2_err(f_out[n], t_out[n])
            print(f"DECODE-TRUTH {label} fwd {n}: relL2 {e:.3e} (float32 floor {fl:.3e})")
            ok = e < L2_BAR
        else:
            (e, x), (fl, fx) = fwd_err(got[n], t_out[n]), fwd_err(f_out[n], t_out[n])
            print(f"DECODE-TRUTH {label} fwd {n}: max|d| {e:.3e} of-bar {x:.3f} (float32 floor {fl:.3e} of-bar {fx:.3f})")
            ok = x <= 1.0
        if not ok:
            bad.append(("fwd", n, e))
    if got_grads is not None:
        assert set(got_grads) == set(t_g), (sorted(got_grads), sorted(t_g))
        for n in sorted(t_g):
            err = l2_err if large else grad_err
            e, fl = err(got_grads[n], t_g[n]), err(f_g[n], t_g[n])
            print(f"DECODE-TRUTH {label} grad {n}: {'relL2' if large else 'max|d|/max|ref|'} {e:.3e} (float32 floor {fl:.3e})")
            if not e < (L2_BAR if large else GRAD_BAR):
                bad.append(("grad", n, e))
    assert not bad, (label, bad)


def training_statis64(acc, k, vis_idx, nop, mask, update_filter, grad):
    """numpy float64 restatement of ScaffoldGaussian.training_statis: acc = four float64 accumulators (Na, Na, Na*k, Na*k), updated in place."""
    opacity_accum, anchor_demon, off_grad, off_den = acc
    vis = np.asarray(vis_idx, np.int64)
    live = vis >= 0                                                   # a padded list has -1 behind the visible anchors
    temp = np.clip(np.asarray(nop, np.float64).reshape(-1, k), 0.0, None).sum(1)
    opacity_accum[vis[live]] += temp[live]
    anchor_demon[vis[live]] += 1.0
    rows = np.nonzero(np.asarray(mask).reshape(-1))[0]                # the p-th generated Gaussian sits in slot (v, j) = divmod(rows[p], k)
    upd = np.asarray(update_filter).reshape(-1).astype(bool)
    slot = vis[rows // k] * k + rows % k
    g = np.asarray(grad, np.float64)
    off_grad[slot[upd]] += np.sqrt(g[upd, 0] ** 2 + g[upd, 1] ** 2)
    off_den[slot[upd]] += 1.0
