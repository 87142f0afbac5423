"""Torch restatements of densify_and_prune for the explicit Gaussians (3DGS / 2DGS / PGSR), on any device.

`layout(...)` is written from the layout rule of DESIGN.md §4.8, not from the reference's text: classify every original, then gather
    [originals neither split nor pruned][their clones][children, repetition 0]...[repetition N-1]
once.  The fixtures under tests/golden/ref_densify_prune_*.npz (made by the reference's own classes) equal it; the GPU tests compare the
device code with it on large random scenes.

`chain(...)` does the same work in the reference's SHAPE (append the clones with one cat per tensor, append the children with another, drop the
split parents with a boolean gather per tensor, drop the pruned rows with another; statistics re-allocated as zeros after every append).  It is
the timing baseline of tools/bench_densify.py and a second, differently built check of `layout`.  It has no caps.
"""
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def rotation_matrix(q):
    """Rotation of the normalised quaternion (r, x, y, z)."""
    n = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / n[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros(q.shape[0], 3, 3, dtype=q.dtype, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def sample_xyz(xyz, rot, s_act, z):
    """R(rot) . (z * s) + xyz; a two-column scaling has a third standard deviation of 0."""
    if s_act.shape[1] == 2:
        s_act = torch.cat((s_act, torch.zeros_like(s_act[:, :1])), 1)
    return torch.bmm(rotation_matrix(rot), (z * s_act).unsqueeze(-1)).squeeze(-1) + xyz


def sample_xyz_f64(xyz, rot, s_act, z):
    """The same formula evaluated in float64 on the float32 inputs, and the sum of |z_j s_j| its error bound is stated in."""
    xyz, rot, s_act, z = (t.double() for t in (xyz, rot, s_act, z))
    if s_act.shape[1] == 2:
        s_act = torch.cat((s_act, torch.zeros_like(s_act[:, :1])), 1)
    return sample_xyz(xyz, rot, s_act, z), (z * s_act).abs().sum(1, keepdim=True)


def _grads(accum, denom):
    g = accum.reshape(-1) / denom.reshape(-1)
    return torch.where(g.isnan(), torch.zeros_like(g), g)


def classify(accum, denom, s_act, o_act, radii, *, max_grad, min_opacity, extent, percent_dense, max_screen_size, N=2, accum_abs=None, denom_abs=None,
             abs_max_grad=None, abs_split_radii2D_threshold=20.0, max_abs_split_points=None, max_all_points=None, child_rule="reference"):
    """-> clone, split, prune_self, prune_child masks over the originals (bool [P]).
    child_rule: how a child's world-size test is taken.  "reference": max(exp(log(s / (0.8 N)))) > 0.1 extent, the reference's own chain of torch
    operations; "quotient": max(s) / float32(0.8 N) > 0.1 extent, one IEEE division -- the contract of include/gsrast.h.  The two
    agree except within a few float32 steps of the threshold (measured: tests/test_densify_edges_cpu.py)."""
    if child_rule not in ("reference", "quotient"):
        raise ValueError(f"child_rule: expected 'reference' or 'quotient' but found {child_rule!r}")
    P = s_act.shape[0]
    g = _grads(accum, denom)
    ms = s_act.max(dim=1).values if P else s_act.new_zeros(0)
    big = ms > percent_dense * extent
    clone = (g.abs() >= max_grad) & (ms <= percent_dense * extent)
    split = (g >= max_grad) & big
    if abs_max_grad is not None:
        if max_all_points is not None and int(clone.sum()) + P > max_all_points:
            v = torch.where(clone, g, torch.zeros_like(g))
            clone = v > torch.quantile(v, 1.0 - (max_all_points - P) / float(P))
        C = int(clone.sum())
        n = P + C
        pad = torch.zeros(C, dtype=g.dtype, device=g.device)
        if max_all_points is not None and int(split.sum()) + n > max_all_points:
            v = torch.where(split, g, torch.zeros_like(g))
            split = v > torch.quantile(torch.cat((v, pad)), 1.0 - (max_all_points - n) / float(n))
        else:
            ga = _grads(accum_abs, denom_abs)
            v = torch.where(~split & big & (radii.reshape(-1) > abs_split_radii2D_threshold), ga, torch.zeros_like(ga))
            by_abs = v >= abs_max_grad
            if max_all_points is not None:
                limited = max_all_points - n - int(split.sum())
                if max_abs_split_points is not None:
                    limited = min(limited, max_abs_split_points)
                if int(by_abs.sum()) > limited:
                    by_abs = v > torch.quantile(torch.cat((v, pad)), 1.0 - limited / float(n))
            split = split | by_abs
    low = o_act.reshape(-1) < min_opacity
    prune_self, prune_child = low, low
    if max_screen_size:
        # the screen-size term compares statistics that were re-allocated as zeros: it never holds
        prune_self = low | (ms > 0.1 * extent)
        if child_rule == "reference":
            child_act = torch.exp(torch.log(s_act / (0.8 * N)))
            child_ms = child_act.max(dim=1).values if P else ms
        else:
            child_ms = ms / torch.tensor(0.8 * N, dtype=torch.float32, device=ms.device)
        prune_child = low | (child_ms > 0.1 * extent)
    return clone, split, prune_self, prune_child


def layout(params, moments, accum, denom, s_act, o_act, radii, *, z_split, z_clone=None, N=2, **rules):
    """-> dict(params, moments, src, counts, clone, split).  z_split [N*S,3], z_clone [C,3] (PGSR; None: clones stay in place)."""
    clone, split, prune_self, prune_child = classify(accum, denom, s_act, o_act, radii, N=N, **rules)
    P = s_act.shape[0]
    idx = lambda m: torch.nonzero(m).reshape(-1)
    i_o, i_c, i_s = idx(~split & ~prune_self), idx(clone & ~prune_self), idx(split & ~prune_child)
    src = torch.cat([i_o, i_c] + [i_s] * N)
    n_o, n_c, n_s, S, C = i_o.numel(), i_c.numel(), i_s.numel(), int(split.sum()), int(clone.sum())
    assert z_split.shape[0] == N * S and (z_clone is None or z_clone.shape[0] == C)
    out = {k: v.detach()[src] for k, v in params.items()}
    mom = {}
    for k, (m, v) in moments.items():
        m2, v2 = m[src], v[src]
        m2[n_o:] = 0; v2[n_o:] = 0
        mom[k] = (m2, v2)
    rank_s = torch.cumsum(split.long(), 0) - 1
    rank_c = torch.cumsum(clone.long(), 0) - 1
    xyz, rot = params["xyz"].detach(), params["rotation"].detach()
    if n_s:
        par = torch.cat([i_s] * N)
        zi = torch.cat([r * S + rank_s[i_s] for r in range(N)])
        out["xyz"][n_o + n_c:] = sample_xyz(xyz[par], rot[par], s_act[par], z_split[zi])
        out["scaling"][n_o + n_c:] = torch.log(s_act[par] / (0.8 * N))
    if z_clone is not None and n_c:
        out["xyz"][n_o:n_o + n_c] = sample_xyz(xyz[i_c], rot[i_c], s_act[i_c], z_clone[rank_c[i_c]])
    rows = src.numel()
    return {"params": out, "moments": mom, "src": src, "clone": clone, "split": split,
            "counts": {"clones": C, "splits": S, "pruned": P + C + (N - 1) * S - rows, "rows": rows}, "parts": (n_o, n_c, n_s)}


def chain(params, moments, accum, denom, s_act_fn, o_act_fn, radii, *, z_split, z_clone=None, N=2, max_grad, min_opacity, extent, percent_dense,
          max_screen_size, accum_abs=None, denom_abs=None, abs_max_grad=None, abs_split_radii2D_threshold=20.0, generator=None):
    """The reference-shaped sequence: append clones, append children, drop the split parents, drop the pruned rows -- every tensor rebuilt each
    time.  s_act_fn / o_act_fn activate the raw scaling / opacity (the state changes between the steps); z_split None: drawn here from `generator`.
    -> (params, moments, statistics)"""
    st = {k: v.detach() for k, v in params.items()}
    mo = {k: tuple(moments[k]) for k in moments}
    dev = st["xyz"].device
    pgsr = abs_max_grad is not None
    stat_names = ["accum", "denom", "radii"] + (["accum_abs", "denom_abs", "max_weight"] if pgsr else [])
    stats = {}

    def fresh_stats():
        n = st["xyz"].shape[0]
        for k in stat_names:
            stats[k] = torch.zeros((n,) if k in ("radii", "max_weight") else (n, 1), device=dev)

    def append(new):
        for k in list(st):
            if k in mo:
                mo[k] = tuple(torch.cat((m, torch.zeros_like(new[k])), dim=0) for m in mo[k])
            st[k] = torch.cat((st[k], new[k]), dim=0)
        fresh_stats()

    def drop(mask):
        keep = ~mask
        for k in list(st):
            if k in mo:
                mo[k] = tuple(m[keep] for m in mo[k])
            st[k] = st[k][keep]
        for k in stat_names:
            stats[k] = stats[k][keep]

    g = accum / denom
    g[g.isnan()] = 0.0
    radii0 = radii.clone()
    if pgsr:
        ga = accum_abs / denom_abs
        ga[ga.isnan()] = 0.0
    dense = percent_dense * extent
    # clones
    sel = (torch.norm(g, dim=-1) >= max_grad) & (torch.max(s_act_fn(st["scaling"]), dim=1).values <= dense)
    new = {k: v[sel] for k, v in st.items()}
    if z_clone is not None:
        new["xyz"] = sample_xyz(st["xyz"][sel], st["rotation"][sel], s_act_fn(st["scaling"])[sel], z_clone)
    append(new)
    # children
    n = st["xyz"].shape[0]
    padded = torch.zeros(n, device=dev)
    padded[:g.shape[0]] = g.squeeze()
    ms = torch.max(s_act_fn(st["scaling"]), dim=1).values
    sel = (padded >= max_grad) & (ms > dense)
    if pgsr:
        pa = torch.zeros(n, device=dev); pa[:ga.shape[0]] = ga.squeeze()
        pr = torch.zeros(n, device=dev); pr[:radii0.shape[0]] = radii0
        pa[sel] = 0
        pa[~((ms > dense) & (pr > abs_split_radii2D_threshold))] = 0
        sel = sel | (pa >= abs_max_grad)
    s_sel = s_act_fn(st["scaling"])[sel].repeat(N, 1)
    new = {k: v[sel].repeat(N, *([1] * (v.dim() - 1))) for k, v in st.items()}
    if z_split is None:
        z_split = torch.randn(s_sel.shape[0], 3, device=dev, generator=generator)
    new["xyz"] = sample_xyz(new["xyz"], new["rotation"], s_sel, z_split)
    new["scaling"] = torch.log(s_sel / (0.8 * N))
    append(new)
    drop(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=dev, dtype=torch.bool))))
    # final prune
    mask = (o_act_fn(st["opacity"]) < min_opacity).squeeze(-1)
    if max_screen_size:
        mask = mask | (stats["radii"] > max_screen_size) | (s_act_fn(st["scaling"]).max(dim=1).values > 0.1 * extent)
    drop(mask)
    return st, mo, stats
