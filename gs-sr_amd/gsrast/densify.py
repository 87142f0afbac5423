"""Densify / clone / split / prune of the explicit Gaussians on the device (include/gsrast.h gsr_densify_plan, gsr_densify_emit).

`densify_and_prune_(model, ...)` replaces `VanillaGaussian.densify_and_prune` (gssr/gaussian/vanilla_gaussian.py:295-426), the two-column
split of `TwoDGaussian` (twod_gaussian.py:22-46) and `PGSRGaussian.densify_and_prune` (pgsr_gaussian.py:43-155): the consumer of the statistics
`gsrast.stats.densification_stats_` accumulates.  The reference rebuilds the 6 parameters and their 12 Adam moments four times (a cat for the
clones, a cat for the children, two boolean gathers, each with a nonzero() host synchronisation); here one pass classifies every Gaussian and
one launch writes every surviving or new row once.  `reset_opacity_` and `densify_` complete the schedule of `VanillaGaussian.densify` /
`PGSRGaussian.densify`.

Kept quirk: the reference's densification_postfix zeroes max_radii2D before the final prune reads it, so `max_radii2D > max_screen_size` never
prunes anything; max_screen_size only switches the world-size test on.  DESIGN.md §4.8 lists this and the deviations.

There is no CPU fallback: host tensors raise."""
import ctypes as C
import functools

import torch

from . import call, lib, scratch
from ._rows import Args, Compute, Tensor, groups, install_
from ._rows import _f32 as _rows_f32, moments as _moments

_f32 = functools.partial(_rows_f32, wild="*")                # a free dimension prints as '*'

GROUPS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
SIZE_PRUNE, CLONE_CAP, SPLIT_CAP, ABS_CAP = 1, 2, 4, 8


def _noise(t, name, N):
    if t is None:
        return None
    t = _f32(t, name, (None, 3), device_check=False)
    if t.shape[0] % N:
        raise RuntimeError(f"{name}: expected {N} * (number of selected Gaussians) rows of 3 draws but found {t.shape[0]} rows")
    return t


def clone_split_prune(params, moments, xyz_gradient_accum, denom, scaling_act, opacity_act, max_radii2D, *, max_grad, min_opacity, extent, percent_dense,
                      max_screen_size=None, N=2, xyz_gradient_accum_abs=None, denom_abs=None, abs_max_grad=None, abs_split_radii2D_threshold=20.0,
                      max_abs_split_points=None, max_all_points=None, noise_split=None, noise_clone=None, generator=None):
    """The whole of densify_and_prune on plain tensors -> (new_params, new_moments, counts).

    params: {group name: tensor [P, ...]} with at least xyz [P,3], scaling [P,2|3] and rotation [P,4]; moments: {group name: (exp_avg, exp_avg_sq)}
    for the groups that have Adam state.  scaling_act / opacity_act are the ACTIVATED tensors as the model's own get_scaling / get_opacity computed
    them, which makes every selection bit-identical to torch's.  abs_max_grad not None selects the PGSR rules (abs-gradient split, noisy clone,
    the max_all_points / max_abs_split_points caps).  noise_split [N*S,3] / noise_clone [C,3]: standard-normal draws, row r*S + j for repetition r
    of the j-th split Gaussian; None: drawn on the device from `generator` once the counts are known.
    Result rows: [originals neither split nor pruned][their clones][children, repetition 0]...[repetition N-1]; carried rows keep their moments,
    new rows get zeros.  counts: clones, splits (selected), pruned (rows of the reference's intermediate state that its final mask removes), rows.
    One host synchronisation when no cap binds."""
    # ---- arguments, before any device call
    N = int(N)
    if N < 1:
        raise RuntimeError(f"N: expected a positive number of children but found {N}")
    if not float(max_grad) > 0.0:
        raise RuntimeError(f"max_grad: expected a positive threshold but found {max_grad} (a clone's padded gradient of 0 must not reach it)")
    pgsr = abs_max_grad is not None
    if pgsr and not float(abs_max_grad) > 0.0:
        raise RuntimeError(f"abs_max_grad: expected a positive threshold but found {abs_max_grad}")
    if pgsr and (xyz_gradient_accum_abs is None or denom_abs is None):
        raise RuntimeError("xyz_gradient_accum_abs / denom_abs: the abs-gradient split needs both accumulators")
    for name in params:
        if name not in GROUPS:
            raise RuntimeError(f"params: unknown group name '{name}', expected one of {sorted(GROUPS)}")
    for name in moments:
        if name not in params:
            raise RuntimeError(f"moments: group '{name}' has no parameter")
    for name in ("xyz", "scaling", "rotation"):
        if name not in params:
            raise RuntimeError(f"params: group '{name}' is missing")
    noise_split = _noise(noise_split, "noise_split", N)
    noise_clone = _noise(noise_clone, "noise_clone", 1)
    xyz = _f32(params["xyz"], "xyz", (None, 3), device_check=False)
    P = xyz.shape[0]
    scaling = _f32(params["scaling"], "scaling", (P, None), device_check=False)
    cols = scaling.shape[1]
    if cols not in (2, 3):
        raise RuntimeError(f"scaling: expected 2 or 3 columns but found {cols}")
    if P * max(2, N) >= 1 << 31:
        raise RuntimeError(f"xyz: P + clones + N * splits can reach {P * max(2, N)} rows, which exceed 2^31")
    srcs = {}
    for name, t in params.items():
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != P:
            raise RuntimeError(f"{name}: expected a tensor of {P} rows")
        t = _f32(t, name, device_check=False)
        rb = 4 * (t.numel() // P if P else int(torch.Size(t.shape[1:]).numel()))
        srcs[name] = (t, rb)
        if name in moments:
            m = moments[name]
            if len(m) != 2:
                raise RuntimeError(f"moments['{name}']: expected (exp_avg, exp_avg_sq)")
            for key, mt in zip(("exp_avg", "exp_avg_sq"), m):
                _f32(mt, f"{name}.{key}", tuple(t.shape), device_check=False)
    _f32(params["rotation"], "rotation", (P, 4), device_check=False)
    stats = {"xyz_gradient_accum": xyz_gradient_accum, "denom": denom, "opacity_act": opacity_act, "max_radii2D": max_radii2D}
    if pgsr:
        stats.update(xyz_gradient_accum_abs=xyz_gradient_accum_abs, denom_abs=denom_abs)
    for name, t in list(stats.items()):
        t = _f32(t, name, device_check=False)
        if t.numel() != P:
            raise RuntimeError(f"{name}: expected {P} entries but found {t.numel()}")
        stats[name] = t
    scaling_act = _f32(scaling_act, "scaling_act", (P, cols), device_check=False)
    # ---- devices: no CPU fallback
    dev = xyz.device
    everything = [("xyz", xyz), ("scaling_act", scaling_act)] + list(stats.items()) + [(n, t) for n, (t, _) in srcs.items()] + \
                 [(f"{n}.moment", mt) for n, m in moments.items() for mt in m] + [("noise_split", noise_split), ("noise_clone", noise_clone)]
    for name, t in everything:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on the device of xyz")
    moments = {n: tuple(mt.detach().contiguous() for mt in m) for n, m in moments.items()}

    L = lib()
    f32 = lambda v: C.c_float(v).value                           # the reference compares float32 tensors with Python scalars: the scalar is rounded to float32
    a = Args()
    a.P, a.scaling_cols, a.N = P, cols, N
    a.flags = SIZE_PRUNE if max_screen_size else 0
    a.clone_thr = a.split_thr = f32(max_grad)
    a.abs_thr = f32(abs_max_grad) if pgsr else 0.0
    a.dense_thr = f32(percent_dense * extent)
    a.min_opacity = f32(min_opacity)
    a.world_thr = f32(0.1 * extent)
    a.abs_radii_thr = f32(abs_split_radii2D_threshold)
    a.child_div = f32(0.8 * N)
    a.accum, a.denom = stats["xyz_gradient_accum"].data_ptr(), stats["denom"].data_ptr()
    if pgsr:
        a.accum_abs, a.denom_abs = stats["xyz_gradient_accum_abs"].data_ptr(), stats["denom_abs"].data_ptr()
    a.scaling, a.opacity, a.max_radii2D = scaling_act.data_ptr(), stats["opacity_act"].data_ptr(), stats["max_radii2D"].data_ptr()
    nbytes = L.gsr_densify_plan_scratch_bytes(P, N)
    work = scratch(nbytes, dev)
    status = torch.empty(8, dtype=torch.int32, device=dev)

    def plan(masked=False):
        m = torch.empty(3, P, dtype=torch.float32, device=dev) if masked else None
        a.masked_out = m.data_ptr() if masked else None
        call("gsr_densify_plan", dev, C.byref(a), work, nbytes, status)
        a.masked_out = None
        return status.tolist(), m                            # the host synchronisation

    c, _ = plan()
    if pgsr and max_all_points is not None and P:
        # pgsr_gaussian.py:69-86,111-117: a cap that binds replaces a threshold by a quantile of the masked gradients and a strict `>`
        def cap(masked_row, pad, limited, n):
            v = torch.cat((masked_row, torch.zeros(pad, dtype=torch.float32, device=dev))) if pad else masked_row
            return float(torch.quantile(v, 1.0 - limited / float(n)))
        if c[0] + P > max_all_points:
            _, m = plan(masked=True)
            a.clone_cap = cap(m[0], 0, max_all_points - P, P); a.flags |= CLONE_CAP
            c, _ = plan()
        n = P + c[0]
        if c[5] + n > max_all_points:
            _, m = plan(masked=True)
            a.split_cap = cap(m[1], c[0], max_all_points - n, n); a.flags |= SPLIT_CAP
            c, _ = plan()
        else:
            limited = max_all_points - n - c[5]
            if max_abs_split_points is not None:
                limited = min(limited, max_abs_split_points)
            if c[1] - c[5] > limited:
                _, m = plan(masked=True)
                a.abs_cap = cap(m[2], c[0], limited, n); a.flags |= ABS_CAP
                c, _ = plan()
    n_clone, n_split, n_o, n_c, n_s = c[0], c[1], c[2], c[3], c[4]
    rows = n_o + n_c + N * n_s
    if noise_split is not None and noise_split.shape[0] != N * n_split:
        raise RuntimeError(f"noise_split: expected {N * n_split} rows (N = {N} draws for each of {n_split} split Gaussians) but found {noise_split.shape[0]}")
    if noise_clone is not None and noise_clone.shape[0] != n_clone:
        raise RuntimeError(f"noise_clone: expected {n_clone} rows (one draw per cloned Gaussian) but found {noise_clone.shape[0]}")
    if noise_split is None:
        noise_split = torch.randn(N * n_split, 3, dtype=torch.float32, device=dev, generator=generator)
    if pgsr and noise_clone is None:
        noise_clone = torch.randn(n_clone, 3, dtype=torch.float32, device=dev, generator=generator)
    if not pgsr:
        noise_clone = None                                   # 3DGS / 2DGS clone in place
    out_p, out_m = {}, {}
    table = (Tensor * (3 * len(srcs)))()
    k = 0
    for name, (t, rb) in srcs.items():
        o = torch.empty((rows,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        out_p[name] = o
        outs = [(t, o, 0)]
        if name in moments:
            mo = tuple(torch.empty_like(o) for _ in range(2))
            out_m[name] = mo
            outs += [(moments[name][0], mo[0], 1), (moments[name][1], mo[1], 1)]
        if rb and rows and P:                                # a zero-width tensor (f_rest at degree 0) keeps its shape and copies nothing
            for s, d, z in outs:
                table[k] = Tensor(s.data_ptr(), d.data_ptr(), rb, z, 0); k += 1
    if rows:
        cc = Compute(xyz.data_ptr(), srcs["rotation"][0].data_ptr(), out_p["xyz"].data_ptr(), out_p["scaling"].data_ptr(),
                     noise_split.data_ptr() if noise_split.numel() else None, noise_clone.data_ptr() if noise_clone is not None and noise_clone.numel() else None)
        counts = (C.c_uint32 * 8)(*c)
        call("gsr_densify_emit", dev, C.byref(a), work, nbytes, counts, k, table, C.byref(cc))
    return out_p, out_m, {"clones": n_clone, "splits": n_split, "pruned": P + n_clone + (N - 1) * n_split - rows, "rows": rows}


def _get(model, name):
    v = getattr(model, name)
    return v() if callable(v) and not isinstance(v, torch.Tensor) else v


@torch.no_grad()
def densify_and_prune_(model, max_grad, min_opacity, extent, max_screen_size, abs_max_grad=None, N=2, noise_split=None, noise_clone=None, generator=None):
    """VanillaGaussian / TwoDGaussian.densify_and_prune (abs_max_grad None) or PGSRGaussian.densify_and_prune on the device, for any object with
    the reference's attributes.  Installs fresh Parameters, carries the Adam moments (gsrast.optim.Adam or torch.optim.Adam), zeroes the
    statistics and returns the number of Gaussians."""
    pgsr = abs_max_grad is not None
    need = list(GROUPS.values()) + ["get_scaling", "get_opacity", "optimizer", "xyz_gradient_accum", "denom", "max_radii2D", "percent_dense"]
    if pgsr:
        need += ["xyz_gradient_accum_abs", "denom_abs", "max_weight", "abs_split_radii2D_threshold", "max_abs_split_points", "max_all_points"]
    for name in need:
        if not hasattr(model, name):
            raise RuntimeError(f"model: attribute {name} is missing")
    grp = groups(model, GROUPS)
    params = {n: g["params"][0] for n, g in grp.items()}
    moments = {n: m for n, m in ((n, _moments(model.optimizer, p)) for n, p in params.items()) if m is not None}
    kw = {}
    if pgsr:
        kw = dict(xyz_gradient_accum_abs=model.xyz_gradient_accum_abs, denom_abs=model.denom_abs, abs_max_grad=abs_max_grad,
                  abs_split_radii2D_threshold=model.abs_split_radii2D_threshold, max_abs_split_points=model.max_abs_split_points,
                  max_all_points=model.max_all_points)
    out_p, out_m, counts = clone_split_prune(params, moments, model.xyz_gradient_accum, model.denom, _get(model, "get_scaling"), _get(model, "get_opacity"),
                                             model.max_radii2D, max_grad=max_grad, min_opacity=min_opacity, extent=extent, percent_dense=model.percent_dense,
                                             max_screen_size=max_screen_size, N=N, noise_split=noise_split, noise_clone=noise_clone, generator=generator, **kw)
    for n, g in grp.items():
        install_(model, g, GROUPS[n], out_p[n], out_m.get(n))
    rows = counts["rows"]
    dev = out_p["xyz"].device
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    model.xyz_gradient_accum, model.denom, model.max_radii2D = z(rows, 1), z(rows, 1), z(rows)
    if pgsr:
        model.xyz_gradient_accum_abs, model.denom_abs, model.max_weight = z(rows, 1), z(rows, 1), z(rows)
    return rows


@torch.no_grad()
def reset_opacity_(model):
    """VanillaGaussian.reset_opacity: opacity = inverse_sigmoid(min(get_opacity, 0.01)), zeroed moments, a fresh Parameter."""
    for name in ("_opacity", "get_opacity", "optimizer"):
        if not hasattr(model, name):
            raise RuntimeError(f"model: attribute {name} is missing")
    op = _get(model, "get_opacity")
    _f32(op, "model.get_opacity")
    x = torch.min(op, torch.ones_like(op) * 0.01)
    new = torch.log(x / (1 - x))
    for g in model.optimizer.param_groups:
        if g.get("name", "") == "opacity":
            if g["params"][0] is not model._opacity:
                raise RuntimeError("model.optimizer: param group 'opacity' must hold model._opacity alone")
            install_(model, g, "_opacity", new, (torch.zeros_like(new), torch.zeros_like(new)))
            return
    raise RuntimeError("model.optimizer: no param group named ['opacity']")


@torch.no_grad()
def densify_(model, step, **kwargs):
    """The schedule of VanillaGaussian.densify (vanilla_gaussian.py:467-479) / PGSRGaussian.densify (pgsr_gaussian.py:164-182): accumulate the
    statistics (gsrast.stats.densification_stats_), densify and prune every densification_interval steps after densify_from_iter, reset the
    opacity every opacity_reset_interval steps; intervals from model.config.  kwargs: visibility_filter, radii, viewspace_points (PGSR: also
    out_observe, viewspace_points_abs) as the reference's renderer returns them; noise_split / noise_clone / generator are handed on."""
    from .stats import densification_stats_
    for name in ("config", "spatial_lr_scale"):
        if not hasattr(model, name):
            raise RuntimeError(f"model: attribute {name} is missing")
    for name in ("visibility_filter", "radii", "viewspace_points"):
        if name not in kwargs:
            raise RuntimeError(f"densify_: keyword argument {name} is missing")
    cfg = model.config
    pgsr = hasattr(model, "xyz_gradient_accum_abs")
    if pgsr:
        for name in ("out_observe", "viewspace_points_abs"):
            if name not in kwargs:
                raise RuntimeError(f"densify_: keyword argument {name} is missing")
    done = {"densified": False, "reset": False}
    if step < cfg.densify_until_iter:
        n = model.max_radii2D.shape[0]
        if pgsr:
            densification_stats_(model.max_radii2D, model.xyz_gradient_accum.view(n), model.denom.view(n), kwargs["viewspace_points"].grad,
                                 kwargs["visibility_filter"], kwargs["radii"], kwargs["out_observe"], kwargs["viewspace_points_abs"].grad,
                                 model.xyz_gradient_accum_abs.view(n), model.denom_abs.view(n))
        else:
            densification_stats_(model.max_radii2D, model.xyz_gradient_accum.view(n), model.denom.view(n), kwargs["viewspace_points"].grad,
                                 kwargs["visibility_filter"], kwargs["radii"])
        if step > cfg.densify_from_iter and step % cfg.densification_interval == 0:
            size_threshold = 20 if step > cfg.opacity_reset_interval else None
            densify_and_prune_(model, cfg.densify_grad_threshold, cfg.opacity_cull_threshold, model.spatial_lr_scale, size_threshold,
                               abs_max_grad=cfg.densify_abs_grad_threshold if pgsr else None, noise_split=kwargs.get("noise_split"),
                               noise_clone=kwargs.get("noise_clone"), generator=kwargs.get("generator"))
            done["densified"] = True
        if step % cfg.opacity_reset_interval == 0:
            reset_opacity_(model)
            done["reset"] = True
    return done
