"""What gsrast.anchors and gsrast.densify share: argument checks, the structs of include/gsrast.h's gsr_anchor_level_*, gsr_rows_* and
gsr_densify_* entry points under their short names, and the surgery on a model and its optimizer (param groups by name, Adam moments, fresh leaf Parameters)."""
import torch

from ._abi import gsr_anchor_level as Level, gsr_octree_weed as Weed, gsr_rows_tensor as RowsTensor  # noqa: F401
from ._abi import gsr_densify_args as Args, gsr_densify_tensor as Tensor, gsr_densify_compute as Compute  # noqa: F401

WEED_MODES = {"floor": 0, "round": 1, "ceil": 2}
WEED_CHUNK = 256                          # include/gsrast.h GSR_OCTREE_WEED_CHUNK


def make_weed(cam_infos, standard_dist, fork, levels, dist2level, visible_threshold, lv=0):
    """(gsr_octree_weed, the camera tensor it points to) for cam_infos [C,4] (centre, scale) on the device; `lv` is the level of a growing pass."""
    if dist2level == "progressive":
        raise RuntimeError("dist2level 'progressive' is not supported by the weed-out: the reference's own weed_out cannot run in that mode")
    if dist2level not in WEED_MODES:
        raise RuntimeError(f"Unknown dist2level: {dist2level}")
    cams = _f32(cam_infos, "cam_infos", (None, 4))
    if cams.shape[0] < 1:
        raise RuntimeError("cam_infos: expected at least one camera")
    if int(levels) < 1:
        raise RuntimeError(f"levels: expected a positive number but found {levels}")
    return Weed(cams.data_ptr(), cams.shape[0], int(levels), WEED_MODES[dist2level], int(lv), float(standard_dist), float(fork), float(visible_threshold)), cams


def _f32(t, name, shape=None, device_check=True, wild=None):
    """A contiguous float32 HIP tensor, or a RuntimeError that names the argument.  A None in `shape` matches any size and prints as `wild`;
    device_check False leaves the device to the caller (densify checks every tensor's device in one place, after the shapes)."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected scalar type Float but found {t.dtype}")
    if shape is not None and (t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise RuntimeError(f"{name}: expected shape {[(wild if s is None else s) for s in shape]} but found {list(t.shape)}")
    if device_check and not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    return t.detach().contiguous()


def _bytes(t, name, n, like):
    """bool / uint8 mask of n entries on the device of `like`, as bytes."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda or t.device != like.device:
        raise RuntimeError(f"{name} must be a CUDA tensor on the device of the other arguments")
    if t.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{name}: expected a bool or uint8 mask but found {t.dtype}")
    if t.numel() != n:
        raise RuntimeError(f"{name}: expected {n} entries but found {t.numel()}")
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def groups(model, attrs, skip=()):
    """{group name: param group} of model.optimizer for attrs = {group name: model attribute}: every name once, each group holding the model's
    tensor alone.  Groups whose name contains one of `skip` are left out and alone."""
    found = {}
    for g in model.optimizer.param_groups:
        name = g.get("name", "")
        if any(s in name for s in skip):
            continue
        if name not in attrs:
            raise RuntimeError(f"model.optimizer: unknown group name '{name}', expected one of {sorted(attrs)}")
        if len(g["params"]) != 1 or g["params"][0] is not getattr(model, attrs[name]):
            raise RuntimeError(f"model.optimizer: param group '{name}' must hold model.{attrs[name]} alone")
        found[name] = g
    missing = sorted(set(attrs) - set(found))
    if missing:
        raise RuntimeError(f"model.optimizer: no param group named {missing}")
    return found


def moments(optimizer, p):
    """(exp_avg, exp_avg_sq) of parameter p, or None where the optimizer holds no Adam state for it."""
    st = optimizer.state.get(p, None)
    return (st["exp_avg"], st["exp_avg_sq"]) if st is not None and "exp_avg" in st else None


def install_(model, group, attr, data, moments=None):
    """A fresh leaf Parameter in the place of the group's tensor model.<attr>; the Adam state moves to it (`step` untouched), with `moments`
    as its (exp_avg, exp_avg_sq) where it has any.  A group without state stays without."""
    old = group["params"][0]
    new = torch.nn.Parameter(data.requires_grad_(True))
    st = model.optimizer.state.get(old, None)
    if st is not None:
        if moments is not None and "exp_avg" in st:
            st["exp_avg"], st["exp_avg_sq"] = moments
        del model.optimizer.state[old]
        model.optimizer.state[new] = st
    group["params"][0] = new
    setattr(model, attr, new)
