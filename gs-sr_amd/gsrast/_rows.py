"""What gsrast.anchors and gsrast.densify share: argument checks, the ctypes side of include/gsrast.h's gsr_anchor_level_*, gsr_rows_* and
gsr_densify_* entry points, and the surgery on a model and its optimizer (param groups by name, Adam moments, fresh leaf Parameters)."""
import ctypes as C

import torch

from . import lib

_vp = C.c_void_p


class Level(C.Structure):                 # include/gsrast.h gsr_anchor_level
    _fields_ = [("Na", C.c_int32), ("N0", C.c_int32), ("k", C.c_int32), ("F", C.c_int32), ("scaling_stride", C.c_int32),
                ("thr_lo", C.c_float), ("thr_hi", C.c_float), ("rand_thr", C.c_float), ("cell", C.c_float), ("origin", C.c_float * 3),
                ("anchor", _vp), ("mask", _vp), ("offset", _vp), ("scaling", _vp), ("anchor_feat", _vp), ("grads", _vp), ("offset_mask", _vp), ("rand", _vp)]


class Weed(C.Structure):                  # include/gsrast.h gsr_octree_weed
    _fields_ = [("cam_infos", _vp), ("C", C.c_int32), ("levels", C.c_int32), ("mode", C.c_int32), ("lv", C.c_int32),
                ("standard_dist", C.c_float), ("fork", C.c_float), ("visible_threshold", C.c_float)]


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


class RowsTensor(C.Structure):            # include/gsrast.h gsr_rows_tensor
    _fields_ = [("src", _vp), ("dst", _vp), ("tail", _vp), ("row_bytes", C.c_int64), ("n_tail", C.c_int64)]


class Args(C.Structure):                  # include/gsrast.h gsr_densify_args
    _fields_ = [("P", C.c_int32), ("scaling_cols", C.c_int32), ("N", C.c_int32), ("flags", C.c_int32)] + \
               [(n, C.c_float) for n in ("clone_thr", "split_thr", "abs_thr", "dense_thr", "min_opacity", "world_thr", "abs_radii_thr", "child_div",
                                         "clone_cap", "split_cap", "abs_cap")] + \
               [(n, _vp) for n in ("accum", "denom", "accum_abs", "denom_abs", "scaling", "opacity", "max_radii2D", "masked_out")]


class Tensor(C.Structure):                # include/gsrast.h gsr_densify_tensor
    _fields_ = [("src", _vp), ("dst", _vp), ("row_bytes", C.c_int64), ("zero_new", C.c_int32), ("pad_", C.c_int32)]


class Compute(C.Structure):               # include/gsrast.h gsr_densify_compute
    _fields_ = [(n, _vp) for n in ("xyz", "rotation", "xyz_dst", "scaling_dst", "noise_split", "noise_clone")]


_bound = False


def _lib():
    global _bound
    L = lib()
    if not _bound:
        sz = C.c_size_t
        for name, res, args in (
                ("gsr_anchor_level_scratch_bytes", sz, [C.c_int32] * 3),
                ("gsr_anchor_level_find", C.c_int, [C.POINTER(Level), _vp, sz, _vp, _vp]),
                ("gsr_anchor_level_emit", C.c_int, [C.POINTER(Level), _vp, sz, C.c_uint32, _vp, _vp, _vp]),
                ("gsr_anchor_level_find_weed", C.c_int, [C.POINTER(Level), _vp, C.POINTER(Weed), _vp, sz, _vp, _vp]),
                ("gsr_octree_weed_out", C.c_int, [_vp, _vp, C.c_int64, C.POINTER(Weed), _vp, _vp, _vp]),
                ("gsr_rows_compact_scratch_bytes", sz, [C.c_int64]),
                ("gsr_rows_compact_multi", C.c_int, [C.c_int64, _vp, C.c_int32, C.POINTER(RowsTensor), _vp, sz, _vp]),
                ("gsr_densify_plan_scratch_bytes", sz, [C.c_int32, C.c_int32]),
                ("gsr_densify_plan", C.c_int, [C.POINTER(Args), _vp, sz, _vp, _vp]),
                ("gsr_densify_emit", C.c_int, [C.POINTER(Args), _vp, sz, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(Tensor), C.POINTER(Compute), _vp])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _bound = True
    return L


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
