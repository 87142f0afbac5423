"""GPU: the fused Adam kernels (csrc/gsr_extra.hip k_adam, k_adam_multi) on the paths the suite never entered: the per-element `lr_scale` that
bench.py trains through, the unaligned branch (E.vec == 0), element counts around GSR_ADAM_CHUNK = 4096, shadow gradients with a ragged tail on an
unaligned tensor, graph replay with lr_scale, and the exported single-tensor entry gsr_adam_step.

Reference: tests/glue_truth.adam_chain (the float32 numpy oracle chained).  Bounds: tests/test_gpu_optim.py's, the learning rate taken per element:
|p - ref| <= 1e-4 lr scale_i + 5e-7; exp_avg rtol 1e-5 / atol 2e-6; exp_avg_sq rtol 1e-5 / atol 1e-12.  tests/test_glue_truth_cpu.py shows that these
inputs tell a wrong lr_scale index from the right one by ten times that bound.  Aligned against unaligned runs are compared with torch.equal:
gsr_extra.hip is built without FMA contraction and every branch evaluates the same expression per element with IEEE sqrtf and division."""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_cases
import glue_truth
import oracle_optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-15


def _shifted(a):
    """`a` (numpy or tensor) as a device view one float into its storage: 4 bytes past a 16-byte boundary."""
    a = torch.as_tensor(a, dtype=torch.float32).reshape(-1)
    buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:]
    v.copy_(a)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dev(a, shift=False):
    if shift:
        return _shifted(a)
    t = torch.as_tensor(a, dtype=torch.float32).reshape(-1).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _run_flat(n, shift=(), steps=glue_cases.ADAM_STEPS):
    """Six steps of gsrast.optim.Adam on ONE flat parameter with lr = 1 and a per-element lr_scale, as bench.py does.  shift: which of
    'param', 'grad', 'moments', 'lr_scale' live one float off alignment.  -> (p, exp_avg, exp_avg_sq) numpy, and the tensors."""
    from gsrast.optim import Adam
    p0, sc, grads = glue_cases.adam_case(n)
    p = torch.nn.Parameter(_dev(p0, "param" in shift))
    s = _dev(sc, "lr_scale" in shift)
    opt = Adam([{"params": [p], "lr": 1.0, "lr_scale": s}], lr=0.0, eps=EPS)
    if "moments" in shift:
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": _shifted(np.zeros(n, np.float32)), "exp_avg_sq": _shifted(np.zeros(n, np.float32))}
    for g in grads[:steps]:
        p.grad = _dev(g, "grad" in shift)
        opt.step()
        opt.zero_grad(set_to_none=True)
    st = opt.state[p]
    assert float(st["step"]) == steps
    if "param" in shift:
        assert p.data_ptr() % 16 == 4
    if "moments" in shift:
        assert st["exp_avg"].data_ptr() % 16 == 4 and st["exp_avg_sq"].data_ptr() % 16 == 4
    return tuple(t.detach().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


def _assert_close(got, ref, bound, what):
    p, m, v = got; rp, rm, rv = ref
    ep = np.abs(p.astype(np.float64) - rp)
    print(f"ADAM-EDGE {what}: max |p - ref| / bound {float((ep / bound).max()):.3f}, max |m - ref| {float(np.abs(m - rm).max()):.2e}")
    assert (ep <= bound).all(), (what, float((ep / bound).max()), int(np.argmax(ep / bound)))
    np.testing.assert_allclose(m, rm, rtol=1e-5, atol=2e-6, err_msg=what)
    np.testing.assert_allclose(v, rv, rtol=1e-5, atol=1e-12, err_msg=what)


@pytest.mark.parametrize("n", glue_cases.ADAM_SIZES)
def test_lr_scale_reaches_every_element(n):
    p0, sc, grads = glue_cases.adam_case(n)
    ref = glue_truth.adam_chain(p0, grads, 1.0, sc, eps=EPS)
    bound = glue_truth.adam_bounds(1.0, sc)
    wrong = glue_truth.adam_chain(p0, grads, 1.0, np.roll(sc, 1) if n > 1 else None, eps=EPS)[0]      # n = 1: nothing to roll; the wrong run ignores lr_scale
    far = np.abs(wrong.astype(np.float64) - ref[0]) > 10 * bound
    assert far.all() if n <= 4 else far.mean() >= 0.95, far.mean()
    _assert_close(_run_flat(n), ref, bound, f"n={n}")


def test_flat_model_with_lr_scale_equals_one_group_per_block():
    """bench.py in small: three column blocks (3P, 4P, P), P = 1367, as ONE flat tensor whose lr_scale carries the blocks' rates at lr = 1, and as three
    tensors in three param groups with those rates.  Not bit-identical: float(lr / (1 - b1^t)) and float(1 / (1 - b1^t)) * lr round differently."""
    from gsrast.optim import Adam
    P, rates = 1367, (1.6e-4, 1e-3, 5e-2)
    sizes = [3 * P, 4 * P, P]
    r = np.random.default_rng(12)
    p0 = np.clip(r.normal(0, 1, sum(sizes)), -2, 2).astype(np.float32)
    sc = np.concatenate([np.full(k, lr, np.float32) for k, lr in zip(sizes, rates)])
    z = torch.nn.Parameter(_dev(p0))
    flat = Adam([{"params": [z], "lr": 1.0, "lr_scale": _dev(sc)}], lr=0.0, eps=EPS)
    parts = [torch.nn.Parameter(_dev(a)) for a in np.split(p0, np.cumsum(sizes)[:-1])]
    grouped = Adam([{"params": [q], "lr": lr} for q, lr in zip(parts, rates)], lr=0.0, eps=EPS)
    grads = []
    for t in range(1, 7):
        g = (r.normal(0, 1, sum(sizes)) * (0.1 if t % 2 else 3.0)).astype(np.float32)
        grads.append(g)
        z.grad = _dev(g)
        for q, a in zip(parts, np.split(g, np.cumsum(sizes)[:-1])):
            q.grad = _dev(a)
        flat.step(); grouped.step()
    a = z.detach().cpu().numpy(); b = np.concatenate([q.detach().cpu().numpy() for q in parts])
    bound = glue_truth.adam_bounds(1.0, sc)
    assert (np.abs(a.astype(np.float64) - b) <= bound).all(), float((np.abs(a.astype(np.float64) - b) / bound).max())
    ma = flat.state[z]["exp_avg"].cpu().numpy(); mb = np.concatenate([grouped.state[q]["exp_avg"].cpu().numpy() for q in parts])
    va = flat.state[z]["exp_avg_sq"].cpu().numpy(); vb = np.concatenate([grouped.state[q]["exp_avg_sq"].cpu().numpy() for q in parts])
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)                        # the moments do not see the learning rate
    _assert_close((a, ma, va), glue_truth.adam_chain(p0, grads, 1.0, sc, eps=EPS), bound, "flat 8P")
    assert np.abs(a - p0).max() > 100 * bound.max()                                 # the parameters did move


def test_unaligned_tensors_take_the_scalar_branch_to_the_same_bits():
    """n = 8197 (two chunks and a five-element third; float4 body plus one tail element when aligned): the parameter, only the gradient, only the two
    moments, only lr_scale one float off a 16-byte boundary -- any of them sends k_adam_multi down its scalar branch."""
    n = 8197
    base = _run_flat(n)
    for shift in (("param",), ("grad",), ("moments",), ("lr_scale",), ("param", "grad", "moments", "lr_scale")):
        got = _run_flat(n, shift)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, base):
            diff = np.nonzero(a != b)[0]
            assert diff.size == 0, (shift, name, diff[:8], a[diff[:8]], b[diff[:8]])


def test_shadow_gradient_with_a_ragged_tail_on_an_unaligned_tensor():
    """tests/test_gpu_optim.py's shadow case on a tensor of 4099 elements (one chunk plus three) that sits one float off alignment: grad + grad2 inside the
    scalar branch is bit-identical to the autograd-summed form, and to both forms on an aligned tensor."""
    from gsrast.optim import Adam, shadow_parameters
    n = 4099
    g = torch.Generator().manual_seed(21)
    w0 = torch.randn(n, generator=g)

    def run(shift, shadows):
        w = _dev(w0, shift).requires_grad_(True)
        opt = Adam([w], lr=1e-2, eps=EPS)
        s = shadow_parameters(w) if shadows else w
        if shadows:
            assert s.data_ptr() == w.data_ptr() and s is not w
            opt.add_shadows([w], [s])
        gen = torch.Generator().manual_seed(22)
        for t in range(5):
            x1 = torch.randn(n, generator=gen).to(DEV); x2 = torch.randn(n, generator=gen).to(DEV)
            ((x1 * w).tanh().sum() * 0.01 + ((x2 * s).sin() * 0.02).sum()).backward()
            if shadows:
                assert s.grad is not None and w.grad is not None
            opt.step(); opt.zero_grad(set_to_none=True)
        if shift:
            assert w.data_ptr() % 16 == 4
        st = opt.state[w]
        return w.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()

    ref = run(False, False)
    assert not torch.equal(ref[0].cpu(), w0)
    for shift, shadows in ((True, True), (True, False), (False, True)):
        got = run(shift, shadows)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), (shift, shadows)


def test_graph_replay_with_lr_scale():
    """One eager step, capture, five replays behind prepare_replay(): the captured launch multiplies the step size it reads from device memory by the
    per-element scale.  n = 4097: one full chunk and a one-element second block."""
    from gsrast.optim import Adam
    n = 4097
    p0, sc, grads = glue_cases.adam_case(n)
    p = torch.nn.Parameter(_dev(p0))
    opt = Adam([{"params": [p], "lr": 1.0, "lr_scale": _dev(sc)}], lr=0.0, eps=EPS)
    slot = torch.zeros(n, device=DEV)
    p.grad = slot
    slot.copy_(_dev(grads[0])); opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for g in grads[1:]:
        slot.copy_(_dev(g))
        opt.prepare_replay(); graph.replay()
    torch.cuda.synchronize()
    st = opt.state[p]
    assert float(st["step"]) == len(grads)
    got = tuple(t.detach().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))
    _assert_close(got, glue_truth.adam_chain(p0, grads, 1.0, sc, eps=EPS), glue_truth.adam_bounds(1.0, sc), "graph n=4097")


# 256 * 16 blocks of 256 threads, four elements each: from 4 194 305 elements on the grid-stride loop of the aligned launch takes a second trip
@pytest.mark.parametrize("n", [1, 5, 1024 * 4, 256 * 16 * 256 * 4 + 7])
def test_single_tensor_entry(n):
    """gsr_adam_step through the C ABI: one step from a non-trivial state, with and without lr_scale, aligned and one float off (k_adam's float4 body
    plus tail against its scalar loop), against one step of the oracle; aligned against unaligned bit for bit."""
    import gsrast
    L = gsrast.lib()
    r = np.random.default_rng(n % 1000)
    p0 = np.clip(r.normal(0, 1, n), -2, 2).astype(np.float32); g = (r.normal(0, 1, n) * 3.0).astype(np.float32)
    m0 = r.normal(0, 0.5, n).astype(np.float32); v0 = (r.normal(0, 1, n) ** 2).astype(np.float32)
    sc = np.exp(r.uniform(np.log(1e-4), np.log(5e-2), n)).astype(np.float32)
    t, b1, b2 = 3, 0.9, 0.999
    for lr, scale in ((1.0, sc), (2e-3, None)):
        ref = oracle_optim.adam_step(p0, g, m0, v0, t, lr, beta1=b1, beta2=b2, eps=EPS, lr_scale=scale)
        step_size = float(np.float32(lr / (1.0 - b1 ** t))); bc2 = float(np.float32(np.sqrt(1.0 - b2 ** t)))
        runs = []
        for shift in (False, True):
            p, gg, m, v = (_dev(a, shift) for a in (p0, g, m0, v0))
            s = None if scale is None else _dev(scale, shift)
            rc = L.gsr_adam_step(n, p.data_ptr(), gg.data_ptr(), m.data_ptr(), v.data_ptr(), step_size, b1, b2, bc2, EPS,
                                 None if s is None else s.data_ptr(), gsrast.stream_ptr(torch.device(DEV)))
            assert rc == 0, gsrast.last_error()
            runs.append(tuple(x.cpu().numpy() for x in (p, m, v)))
            assert torch.equal(gg.cpu(), torch.from_numpy(g))
        _assert_close(runs[0], ref, glue_truth.adam_bounds(lr, scale), f"adam_step n={n} scale={scale is not None}")
        for a, b in zip(*runs):
            diff = np.nonzero(a != b)[0]
            assert diff.size == 0, (n, diff[:8])


def test_single_tensor_entry_refuses_step_zero():
    """bias_correction2_sqrt = 0 (step 0) is refused on the host, before any launch: non-zero return, a message, buffers untouched."""
    import gsrast
    L = gsrast.lib()
    n = 1000
    r = np.random.default_rng(3)
    host = [r.normal(0, 1, n).astype(np.float32) for _ in range(4)]
    p, g, m, v = (_dev(a) for a in host)
    rc = L.gsr_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 0.0, EPS, None, gsrast.stream_ptr(torch.device(DEV)))
    assert rc != 0 and "bias_correction2_sqrt" in gsrast.last_error()
    torch.cuda.synchronize()
    for t, a in zip((p, g, m, v), host):
        assert np.array_equal(t.cpu().numpy(), a)
