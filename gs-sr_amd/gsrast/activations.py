"""Activations of the explicit-Gaussian models in front of the rasterizer (include/gsrast.h gsr_gauss_activations[_backward]).

`VanillaGaussianModel.get_scaling / get_rotation / get_opacity` (gssr/gaussian/vanilla_gaussian.py:86-90,250-269) are exp, F.normalize and sigmoid of
three parameter tensors: three torch kernels forward (normalize alone is three) and ~8 in autograd, every iteration of vanilla-3dgs / 2dgs / pgsr.
Here: one streaming HIP kernel each way."""
import torch

from . import call, dev_f32


def _aligned16(t):
    """The kernels read a quaternion as one 16-byte word: a contiguous view that starts 4 or 8 bytes into its storage is copied."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _GaussActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling_raw, rotation_raw, opacity_raw):
        s = dev_f32(scaling_raw, "scaling", allow_empty=False)
        q = _aligned16(dev_f32(rotation_raw, "rotation", allow_empty=False))
        o = dev_f32(opacity_raw, "opacity", allow_empty=False)
        P = s.shape[0]
        if s.dim() != 2 or not (1 <= s.shape[1] <= 3) or q.shape != (P, 4) or o.numel() != P:
            raise RuntimeError("gaussian_activations: scaling (P, 1..3), rotation (P, 4), opacity (P, 1) expected")
        so, qo, oo = torch.empty_like(s), torch.empty_like(q), torch.empty_like(o)
        call("gsr_gauss_activations", s.device, P, int(s.shape[1]), s, q, o, so, qo, oo)
        ctx.save_for_backward(so, q, qo, oo)
        ctx.set_materialize_grads(False)
        return so, qo, oo

    @staticmethod
    def backward(ctx, gs, gq, go):
        so, q, qo, oo = ctx.saved_tensors
        P = so.shape[0]
        c = lambda g: None if g is None else g.contiguous()
        gs, gq, go = c(gs), _aligned16(c(gq)), c(go)
        ds, dq, do = torch.empty_like(so), torch.empty_like(q), torch.empty_like(oo)
        call("gsr_gauss_activations_backward", so.device, P, int(so.shape[1]), so, q, qo, oo, gs, gq, go, ds, dq, do)
        return ds, dq, do


def gaussian_activations(scaling_raw, rotation_raw, opacity_raw):
    """-> (exp(scaling_raw), F.normalize(rotation_raw), sigmoid(opacity_raw)), differentiable, one HIP kernel forward and one backward."""
    return _GaussActivations.apply(scaling_raw, rotation_raw, opacity_raw)
