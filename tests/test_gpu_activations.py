"""GPU test (pytest -m gpu): gsrast.activations.gaussian_activations (include/gsrast.h gsr_gauss_activations[_backward]) against the reference's own
formulation -- torch.exp / torch.nn.functional.normalize / torch.sigmoid on the three parameter tensors
(/root/reference/gssr/gaussian/vanilla_gaussian.py:86-90,250-269) -- values and gradients, incl. a zero quaternion (normalize's eps clamp), an output
the loss never touches (null upstream gradient) and the 2-axis scaling of the surfel models."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P,S", [(1, 3), (257, 2), (100003, 3)])
def test_gaussian_activations_match_torch(P, S):
    from gsrast.activations import gaussian_activations
    g = torch.Generator().manual_seed(P)
    s0 = (torch.randn(P, S, generator=g) * 1.5 - 3.0).cuda()
    q0 = torch.randn(P, 4, generator=g).cuda()
    o0 = (torch.randn(P, 1, generator=g) * 2.0).cuda()
    if P > 3:
        q0[3] = 0.0                                     # F.normalize: x / max(|x|, 1e-12) -> 0, gradient g / 1e-12
        q0[2] *= 1e-3
    w = [torch.randn(P, S, generator=g).cuda(), torch.randn(P, 4, generator=g).cuda(), torch.randn(P, 1, generator=g).cuda()]

    def run(fn, use=(True, True, True)):
        leaves = [t.clone().requires_grad_(True) for t in (s0, q0, o0)]
        outs = fn(*leaves)
        loss = sum((o * ww).sum() for o, ww, u in zip(outs, w, use) if u)
        loss.backward()
        return [o.detach() for o in outs], [l.grad for l in leaves]
    ref = lambda s, q, o: (torch.exp(s), torch.nn.functional.normalize(q), torch.sigmoid(o))
    for use in ((True, True, True), (True, False, True), (False, True, False)):
        (a, ga), (b, gb) = run(gaussian_activations, use), run(ref, use)
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=2e-6, atol=1e-7), (x - y).abs().max().item()
        for k, (x, y) in enumerate(zip(ga, gb)):
            if y is None:
                assert x is None or float(x.abs().max()) == 0.0
                continue
            ok = torch.isfinite(y).all(dim=-1) if y.dim() > 1 else torch.isfinite(y)
            assert torch.allclose(x[ok], y[ok], rtol=1e-5, atol=1e-6 * float(y[ok].abs().max() + 1)), (k, (x[ok] - y[ok]).abs().max().item())


# ------------------------------------------------------------------------------------------------------------------------ float64 truth, per-element bars
# tests/act_truth.py: cases at the block size (256) and its neighbours, one to three scaling columns, the float32 range of exp and sigmoid, the 1e-12
# clamp of normalize from both sides, an upstream gradient parallel to r, each upstream gradient absent in turn.  The worst observed error in units
# of the bars is printed per case and recorded in the docstring of act_truth.py.
import numpy as np                                                  # noqa: E402

import act_truth as A                                               # noqa: E402

DEV = "cuda:0"
NAMES = ("scaling", "rotation", "opacity")


def _offset_view(a, off):
    """a (numpy) as a device tensor that starts `off` floats into its storage."""
    base = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    v = base[off:off + a.size].view(a.shape)
    v.copy_(torch.tensor(a))
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


def _run(c, fn, off=0):
    """fn on the case's tensors (views `off` floats into their storage), backward with the case's upstream gradients -> {output: numpy float32}."""
    leaves = [_offset_view(c[k], off).requires_grad_(True) for k in ("s", "q", "o")]
    outs = fn(*leaves)
    use = [(o, _offset_view(c["g"][n], off)) for o, n in zip(outs, NAMES) if c["g"][n] is not None]
    torch.autograd.backward([o for o, _ in use], [g for _, g in use])
    res = {n: o.detach().cpu().numpy() for n, o in zip(NAMES, outs)}
    for n, l in zip(NAMES, leaves):
        res["d_" + n] = (torch.zeros_like(l) if l.grad is None else l.grad).cpu().numpy()
    return res


def _torch_formulation(s, q, o):
    return torch.exp(s), torch.nn.functional.normalize(q), torch.sigmoid(o)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("P", A.SIZES)
def test_against_float64_truth(P, S):
    from gsrast.activations import gaussian_activations
    c = A.make_case(P, S, seed=100 * P + S)
    got = _run(c, gaussian_activations)
    yard = _run(c, _torch_formulation)
    yard["d_rotation"] = np.where(np.isfinite(yard["d_rotation"]), yard["d_rotation"], np.nan)
    print(P, S, "torch in units of the bars:", {k: round(v, 3) for k, v in A.check(c, yard, raise_on_miss=False).items()})
    worst = A.check(c, got, yard=yard)
    print(P, S, "kernel in units of the bars:", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("absent", NAMES)
def test_an_absent_upstream_gradient(absent):
    from gsrast.activations import gaussian_activations
    c = A.make_case(257, 3, seed=25703, absent=absent)
    got = _run(c, gaussian_activations)
    assert not got["d_" + absent].any()
    A.check(c, got, yard=_run(c, _torch_formulation))


@pytest.mark.parametrize("off", [1, 2])
def test_input_layout(off):
    """Inputs and upstream gradients that are views 4 and 8 bytes into their storage give the bits of the aligned copy (the kernels read a
    quaternion as one 16-byte word; the wrapper copies a view that is not aligned)."""
    from gsrast.activations import gaussian_activations
    c = A.make_case(257, 3, seed=25703)
    want, got = _run(c, gaussian_activations), _run(c, gaussian_activations, off=off)
    for k in want:
        assert np.array_equal(want[k].view(np.int32), got[k].view(np.int32)), k
