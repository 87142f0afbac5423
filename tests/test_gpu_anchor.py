"""Anchor growing + pruning on the device (gsrast.anchors; gs-sr_amd/csrc/gsr_anchor.hip).  Every comparison is exact equality:
against the fixtures the reference's own ScaffoldGaussian.adjust_anchor produced (tests/golden/make_golden_anchor.py) and, on randomised scenes,
against the torch restatement that test_anchor_cpu.py holds to those fixtures (tests/ref_anchor_torch.py).  The randomised scenes do not meet a
threshold; the last section puts slots one float32 below, on and above each of them (tests/anchor_edge_cases.py)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import ref_anchor_torch as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_anchor_adjust_*.npz")))
DEV = "cuda:0"
NAMES = R.NAMES
ACCS = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")


class Model:
    pass


def _optimizers():
    from gsrast.optim import Adam
    return {"gsrast": Adam, "torch": torch.optim.Adam}


def make_model(fx, opt_cls):
    m = Model()
    for n in NAMES:
        setattr(m, "_" + n, torch.nn.Parameter(fx["in_" + n].to(DEV)))
    for n in ACCS:
        setattr(m, n, fx["in_" + n].to(DEV))
    m.get_scaling = fx["scaling_act"].to(DEV)                       # the activated tensor as the reference computed it
    m.n_offsets, m.voxel_size = int(fx["k"]), float(fx["voxel_size"])
    m.update_depth, m.update_init_factor, m.update_hierachy_factor = int(fx["update_depth"]), int(fx["update_init_factor"]), int(fx["update_hierachy_factor"])
    m.max_radii2D = torch.ones(fx["in_anchor"].shape[0], device=DEV)
    m.optimizer = opt_cls([{"params": [getattr(m, "_" + n)], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        m.optimizer.state[getattr(m, "_" + n)] = {"step": torch.tensor(1.0), "exp_avg": fx["m_" + n].to(DEV), "exp_avg_sq": fx["v_" + n].to(DEV)}
    return m


@pytest.mark.parametrize("opt", ["gsrast", "torch"])
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_adjust_anchor_equals_reference_fixture(path, opt):
    from gsrast import anchors
    fx = {k: torch.tensor(v) for k, v in np.load(path).items()}
    m = make_model(fx, _optimizers()[opt])
    depth = int(fx["update_depth"])
    Na = anchors.adjust_anchor_(m, rand=[fx[f"rand_{i}"].to(DEV) for i in range(depth)])
    keep = fx["keep"]
    U = int(fx["level_counts"].sum())
    assert Na == int(keep.sum()) + U
    for n in NAMES:
        p = getattr(m, "_" + n)
        old = fx["in_" + n][keep]
        if n == "scaling":
            old = old.clone(); old[:, 3:] = old[:, 3:].clamp(max=0.05)
        want = torch.cat((old, fx["new_" + n]))
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert p.shape == want.shape and torch.equal(p.detach().cpu(), want), n
        group = [g for g in m.optimizer.param_groups if g["name"] == n][0]
        assert group["params"][0] is p and len(m.optimizer.state) == len(NAMES)
        st = m.optimizer.state[p]
        assert float(st["step"]) == 1.0
        for key, src in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            wm = torch.cat((fx[src + n][keep], torch.zeros_like(fx["new_" + n])))
            assert st[key].shape == p.shape and torch.equal(st[key].cpu(), wm), (n, key)
    for n in ACCS:
        assert torch.equal(getattr(m, n).cpu(), fx["out_" + n]), n
    assert m.max_radii2D.shape == (Na,) and not bool(m.max_radii2D.any())
    for n in NAMES:                                                  # the carried state serves a following step
        getattr(m, "_" + n).grad = torch.ones_like(getattr(m, "_" + n))
    m.optimizer.step()
    torch.cuda.synchronize()
    for n in NAMES:
        st = m.optimizer.state[getattr(m, "_" + n)]
        assert float(st["step"]) == 2.0 and bool(torch.isfinite(st["exp_avg"]).all())


def random_scene(N, k, F, seed, cell):
    """Anchors on the cell lattice around the origin (cells of both signs), offsets that reach a few cells."""
    r = np.random.default_rng(seed)
    side = max(4, int(round((N * 6) ** (1 / 3))))
    anchor = (np.round(r.uniform(-side / 2, side / 2, (N, 3))) * cell + r.uniform(-0.3, 0.3, (N, 3)) * cell).astype(np.float32)
    return {"anchor": torch.tensor(anchor), "offset": torch.tensor(r.uniform(-1, 1, (N, k, 3)).astype(np.float32)),
            "scaling": torch.tensor((r.uniform(0.5, 3.0, (N, 6)) * cell).astype(np.float32)), "feat": torch.tensor(r.normal(0, 1, (N, F)).astype(np.float32)),
            "grads": torch.tensor(np.exp(r.normal(math.log(3e-4), 1.0, N * k)).astype(np.float32)), "seen": torch.tensor(r.uniform(size=N * k) < 0.7),
            "mask": torch.tensor(r.uniform(size=N) < 0.6), "rand": [torch.tensor(r.uniform(size=N * k).astype(np.float32)) for _ in range(3)]}


def cell_order_keys(a, origin, cell):
    c = torch.round((a - torch.tensor(origin)) / torch.tensor(cell, dtype=torch.float32)).to(torch.int64) + R.BIAS
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


# the last four: N * (1 + k) = 1023, 1024, 1025 and 2049 entries in the first level -- a last workgroup of the compaction one short, exactly full, one
# over, and a third workgroup that holds one entry
@pytest.mark.parametrize("N,k,F", [(300000, 10, 32), (77777, 3, 5), (341, 2, 5), (512, 1, 5), (205, 4, 5), (683, 2, 5)])
def test_anchor_growing_equals_restatement(N, k, F):
    growing_equals_restatement(N, k, F)


def growing_equals_restatement(N, k, F):
    """-> (the scene, the levels' counts); tests/test_gpu_sort_paths.py runs it on both sides of the sort's digit-major switch."""
    from gsrast import anchors
    vs = 0.01
    s = random_scene(N, k, F, seed=N % 97, cell=vs * 4)
    d = {n: v.to(DEV) if torch.is_tensor(v) else [x.to(DEV) for x in v] for n, v in s.items()}
    kw = dict(voxel_size=vs, n_offsets=k)
    got = anchors.anchor_growing(d["anchor"], d["offset"], d["scaling"], d["feat"], d["grads"], d["seen"], 0.0002, rand=d["rand"], **kw)
    again = anchors.anchor_growing(d["anchor"], d["offset"], d["scaling"], d["feat"], d["grads"], d["seen"], 0.0002, rand=d["rand"], **kw)
    want, counts = R.anchor_growing(s["anchor"], s["offset"], s["scaling"], s["feat"], s["grads"], s["seen"], 0.0002, rand=s["rand"], **kw)
    assert sum(c > 0 for c in counts) >= 2, counts
    for n in NAMES:
        assert got[n].shape == want[n].shape and torch.equal(got[n].cpu(), want[n]), n
        assert torch.equal(got[n], again[n]), n                      # bitwise deterministic
    p = 0
    for i, c in enumerate(counts):                                   # every level's anchors strictly increase in (x, y, z) cell order
        key = cell_order_keys(got["anchor"][p:p + c].cpu(), (0.0, 0.0, 0.0), vs * (16 // 4 ** i))
        assert bool((key[1:] > key[:-1]).all()), i
        p += c
    return s, counts


@pytest.mark.parametrize("N,k,F", [(300000, 10, 32), (77777, 3, 5)])
def test_grow_level_mask_origin_band(N, k, F):
    """The Octree shape of the level: per-anchor mask, origin, finite upper threshold, later anchors that only occupy."""
    from gsrast import anchors
    cell, origin = 0.07, (0.013, -0.4, 2.5)
    s = random_scene(N + 1000, k, F, seed=3 + N % 89, cell=cell)
    n0 = N
    a = dict(cell=cell, thr_lo=0.0002, thr_hi=0.0009, rand_thr=0.3, origin=origin, n0=n0)
    cut = lambda t, rows: t[:rows]
    host = (s["anchor"], cut(s["offset"], n0), cut(s["scaling"], n0), cut(s["feat"], n0), cut(s["grads"], n0 * k), cut(s["seen"], n0 * k))
    want_a, want_f = R.grow_level(*host, rand=cut(s["rand"][0], n0 * k), mask=cut(s["mask"], n0), **a)
    dev = [t.to(DEV) for t in host]
    for _ in range(2):
        got_a, got_f = anchors.grow_level(*dev, rand=cut(s["rand"][0], n0 * k).to(DEV), mask=cut(s["mask"], n0).to(DEV), **a)
        assert want_a.shape[0] > 100 and got_a.shape == want_a.shape
        assert torch.equal(got_a.cpu(), want_a) and torch.equal(got_f.cpu(), want_f)
    key = cell_order_keys(got_a.cpu(), origin, cell)
    assert bool((key[1:] > key[:-1]).all())
    # without rand and mask
    want_a, want_f = R.grow_level(*host, **a)
    got_a, got_f = anchors.grow_level(*dev, **a)
    assert torch.equal(got_a.cpu(), want_a) and torch.equal(got_f.cpu(), want_f)


def test_empty_results_and_range_error():
    from gsrast import anchors
    N, k, F = 5000, 4, 8
    s = random_scene(N, k, F, seed=2, cell=0.05)
    dev = [s[n].to(DEV) for n in ("anchor", "offset", "scaling", "feat", "grads", "seen")]
    a, f = anchors.grow_level(*dev, cell=0.05, thr_lo=1e9)                               # no candidate
    assert a.shape == (0, 3) and f.shape == (0, F)
    zero = [dev[0], torch.zeros_like(dev[1])] + dev[2:]
    a, f = anchors.grow_level(*zero, cell=0.05, thr_lo=0.0)                              # every candidate sits in its own anchor's cell
    assert a.shape == (0, 3) and f.shape == (0, F)
    d = anchors.anchor_growing(*zero, 0.0, voxel_size=0.05 / 16, n_offsets=k)            # level 0 empty: the later levels are skipped
    assert d["anchor"].shape == (0, 3) and d["offset"].shape == (0, k, 3) and d["scaling"].shape == (0, 6)
    e = torch.zeros(0, device=DEV)
    a, f = anchors.grow_level(e.reshape(0, 3), e.reshape(0, k, 3), e.reshape(0, 6), e.reshape(0, F), e, e.bool(), cell=0.05, thr_lo=0.0)   # no anchors at all
    assert a.shape == (0, 3) and f.shape == (0, F)
    with pytest.raises(RuntimeError, match="packing range"):                              # +-2^20 cells of 1e-7: the scene does not fit
        anchors.grow_level(*dev, cell=1e-7, thr_lo=0.0)
    far = dev[0].clone(); far[7:40] = 3.0e5                                                # one candidate owner far outside, a cell that would wrap in 21 bits
    with pytest.raises(RuntimeError, match="packing range"):
        anchors.grow_level(far, *dev[1:], cell=0.05, thr_lo=0.0)


def knife_edge_points(n_want=16, seed=123, cell=np.float32(0.01)):
    """Seeded search for (anchor, offset, scale) whose point anchor + offset * scale lands in ANOTHER cell when the multiply-add is fused (product and
    sum exact in float64, rounded once) than when the product is rounded to float32 first -- what -ffp-contract=off protects."""
    r = np.random.default_rng(seed)
    found = []
    for _ in range(400):
        n = r.integers(-3000, 3000, 4096)
        o = r.uniform(-1, 1, 4096).astype(np.float32)
        s = r.uniform(0.02, 0.3, 4096).astype(np.float32)
        edge = (n + 0.5) * np.float64(cell)                                               # a half-integer cell boundary
        a0 = (edge - o.astype(np.float64) * s.astype(np.float64)).astype(np.float32)
        for ulps in (0, 1, -1, 2, -2):
            a = a0 if ulps == 0 else np.nextafter(a0, np.float32(np.sign(ulps) * np.inf)) if abs(ulps) == 1 else \
                np.nextafter(np.nextafter(a0, np.float32(np.sign(ulps) * np.inf)), np.float32(np.sign(ulps) * np.inf))
            a = a.astype(np.float32)
            split = a + (o * s).astype(np.float32)                                        # float32 multiply, then float32 add
            fused = (a.astype(np.float64) + o.astype(np.float64) * s.astype(np.float64)).astype(np.float32)
            c1, c2 = np.rint(split / cell), np.rint(fused / cell)
            hit = np.nonzero(c1 != c2)[0]
            found += [(a[i], o[i], s[i]) for i in hit]
        if len(found) >= 4 * n_want:
            break
    assert len(found) >= n_want, len(found)
    return np.array(found, np.float32), float(cell)


def test_knife_edge_points_follow_multiply_then_add():
    from gsrast import anchors
    pts, cell = knife_edge_points()
    M = pts.shape[0]
    assert M >= 16
    r = np.random.default_rng(9)
    for axis in range(3):
        anchor = np.zeros((M, 3), np.float32); offset = np.zeros((M, 1, 3), np.float32); scaling = np.ones((M, 6), np.float32)
        anchor[:, axis], offset[:, 0, axis], scaling[:, axis] = pts[:, 0], pts[:, 1], pts[:, 2]
        other = [c for c in range(3) if c != axis]
        anchor[:, other] = (np.round(r.uniform(-50, 50, (M, 2))) * cell).astype(np.float32)
        host = (torch.tensor(anchor), torch.tensor(offset), torch.tensor(scaling), torch.arange(M, dtype=torch.float32).reshape(M, 1),
                torch.ones(M), torch.ones(M, dtype=torch.bool))
        want_a, want_f = R.grow_level(*host, cell=cell, thr_lo=0.5)
        got_a, got_f = anchors.grow_level(*[t.to(DEV) for t in host], cell=cell, thr_lo=0.5)
        assert want_a.shape[0] >= 8
        assert got_a.shape == want_a.shape and torch.equal(got_a.cpu(), want_a) and torch.equal(got_f.cpu(), want_f), axis


@pytest.mark.parametrize("N", [0, 1, 1000, 70001])
def test_rows_compact_multi_equals_cat(N):
    from gsrast import anchors
    k = 10
    g = torch.Generator().manual_seed(N)
    widths = [(1,), (3,), (6,), (32,), (k, 3)]                      # rows of 4, 12, 24, 128, 4*k*3 bytes
    xs = [torch.randn((N,) + w, generator=g) for w in widths] + [torch.randint(-9, 9, (N, 2), generator=g, dtype=torch.int32)]
    for mode in ("random", "all", "none"):
        keep = {"random": torch.rand(N, generator=g) < 0.7, "all": torch.ones(N, dtype=torch.bool), "none": torch.zeros(N, dtype=torch.bool)}[mode]
        for tails in ([torch.randn((37,) + w, generator=g) for w in widths] + [torch.randint(-9, 9, (37, 2), generator=g, dtype=torch.int32)],
                      [37] * len(xs), [0] * len(xs), None):
            dev_tails = None if tails is None else [t.to(DEV) if torch.is_tensor(t) else t for t in tails]
            outs = anchors.rows_compact(keep.to(DEV), [x.to(DEV) for x in xs], dev_tails)
            for i, (x, o) in enumerate(zip(xs, outs)):
                t = 0 if tails is None else tails[i]
                tail = t if torch.is_tensor(t) else torch.zeros((t,) + tuple(x.shape[1:]), dtype=x.dtype)
                want = torch.cat((x[keep], tail))
                assert o.shape == want.shape and o.dtype == want.dtype and torch.equal(o.cpu(), want), (mode, i)


def test_short_training_loop_with_densification():
    """decode -> surfel rasterizer -> L1 -> backward -> training_stats_ -> Adam for 250 iterations, adjust_anchor_ at 100 and 200."""
    import diff_surfel_rasterization as dsr
    import scaffold_filter as sf
    import hiprun
    import scenes
    from gsrast import anchors, decode
    from gsrast.losses import l1_plus_linear
    from gsrast.optim import Adam
    W, H, k, Na0 = 160, 112, 10, 1500
    sc = scenes.make_scene("surfel", Na0, W, H, seed=0, color_mode="precomp")
    t = hiprun.to_dev(sc, DEV)
    rs = hiprun.settings("surfel", t)
    fs = sf.GaussianRasterizationSettings(**rs._asdict())
    g = torch.Generator(device="cpu").manual_seed(7)
    torch.manual_seed(3)
    s2 = t["scales"]
    ext = s2.mean(dim=1, keepdim=True)
    m = Model()
    m._anchor = torch.nn.Parameter(t["means3D"].clone())
    m._scaling = torch.nn.Parameter(torch.log(torch.cat([3.0 * ext.expand(-1, 3), 2.0 * s2, 2.0 * s2[:, :1]], dim=1)))
    m._anchor_feat = torch.nn.Parameter(torch.randn(Na0, 32, generator=g).to(DEV))
    m._offset = torch.nn.Parameter((0.5 * torch.randn(Na0, k, 3, generator=g)).to(DEV))
    m._rotation = torch.nn.Parameter(torch.nn.functional.normalize(torch.randn(Na0, 4, generator=g), dim=1).to(DEV))
    m._opacity = torch.nn.Parameter(torch.zeros(Na0, 1, device=DEV))
    mlp = lambda i, o, act: torch.nn.Sequential(torch.nn.Linear(i, 32), torch.nn.ReLU(True), torch.nn.Linear(32, o), act).to(DEV)
    mlp_o, mlp_c, mlp_k = mlp(35, k, torch.nn.Tanh()), mlp(35, 7 * k, torch.nn.Identity()), mlp(35, 3 * k, torch.nn.Sigmoid())
    lrs = {"anchor": 1e-4, "offset": 1e-3, "anchor_feat": 5e-3, "opacity": 1e-2, "scaling": 1e-3, "rotation": 1e-3}
    m.optimizer = Adam([{"params": [getattr(m, "_" + n)], "lr": lr, "name": n} for n, lr in lrs.items()] +
                       [{"params": list(net.parameters()), "lr": 2e-3, "name": "mlp_" + n} for n, net in (("opacity", mlp_o), ("cov", mlp_c), ("color", mlp_k))],
                       lr=0.0, eps=1e-15)
    m.opacity_accum, m.anchor_demon = torch.zeros(Na0, 1, device=DEV), torch.zeros(Na0, 1, device=DEV)
    m.offset_gradient_accum, m.offset_denom = torch.zeros(Na0 * k, 1, device=DEV), torch.zeros(Na0 * k, 1, device=DEV)
    m.n_offsets, m.voxel_size, m.update_depth, m.update_init_factor, m.update_hierachy_factor = k, float(ext.median()) * 0.25, 3, 16, 4
    m.max_radii2D = torch.zeros(Na0, device=DEV)
    m.get_scaling = None
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = torch.stack([0.5 + 0.3 * torch.sin(xx / 20.0 + c) * torch.cos(yy / 15.0) for c in range(3)]).to(DEV)
    campos = t["campos"]
    losses, counts = [], [Na0]
    for it in range(1, 251):
        scaling = torch.exp(m._scaling)
        with torch.no_grad():
            radii = sf.GaussianRasterizer(fs).visible_filter(means3D=m._anchor, scales=scaling[:, :3], rotations=torch.nn.functional.normalize(m._rotation, dim=1),
                                                             cov3D_precomp=None)
            vis_idx = decode.compact_visible(radii > 0, padded=True)
        xyz, color, opacity, scl, rot, nop, mask = decode.neural_gaussians(m._anchor, m._anchor_feat, m._offset, scaling, mlp_o, mlp_c, mlp_k, campos, vis_idx=vis_idx)
        means2D = torch.zeros_like(xyz, requires_grad=True)
        img, rad, _allmap = dsr.GaussianRasterizer(rs)(means3D=xyz, means2D=means2D, opacities=opacity, colors_precomp=color, scales=scl[:, :2].contiguous(),
                                                       rotations=rot)
        loss = l1_plus_linear(img, gt)
        loss.backward()
        decode.training_stats_(m.opacity_accum, m.anchor_demon, m.offset_gradient_accum, m.offset_denom, means2D.grad, nop, rad > 0, mask, vis_idx=vis_idx)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
        if it in (100, 200):
            m.get_scaling = torch.exp(m._scaling).detach()
            gr = torch.nan_to_num(m.offset_gradient_accum / m.offset_denom, nan=0.0).abs().reshape(-1)
            seen = (m.offset_denom > 40.0).reshape(-1)
            thr = float(gr[seen].quantile(0.7)) if bool(seen.any()) else 0.0002      # the scene's own gradient scale: the upper 30 % of the seen slots propose
            Na = anchors.adjust_anchor_(m, grad_threshold=thr)
            counts.append(Na)
            for n in ("_anchor", "_offset", "_anchor_feat", "_opacity", "_scaling", "_rotation", "opacity_accum", "anchor_demon", "max_radii2D"):
                assert getattr(m, n).shape[0] == Na, n
            assert m._offset.shape == (Na, k, 3) and m._scaling.shape == (Na, 6) and m._anchor_feat.shape == (Na, 32)
            assert m.offset_gradient_accum.shape == (Na * k, 1) and m.offset_denom.shape == (Na * k, 1)
            for grp in m.optimizer.param_groups:
                for p in grp["params"]:
                    st = m.optimizer.state.get(p)
                    if st:
                        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, grp["name"]
            assert m.optimizer.param_groups[0]["params"][0] is m._anchor
    assert len(set(counts)) > 1, counts                               # the anchor count changed at least once
    assert all(math.isfinite(x) for x in losses)
    assert sum(losses[-5:]) / 5 <= losses[0], (losses[0], losses[-5:])


# ------------------------------------------------------------------------------------------------------------------------ the selection thresholds
# tests/anchor_edge_cases.py: every slot named by the comparison it sits on (one float32 below, on, one above), in a cell of its own.  The names
# that show are demanded literally and through the restatement; test_anchor_cpu.py shows that reversing any comparison changes them.
import anchor_edge_cases as E                                      # noqa: E402

BAND = [(0.0002, 0.0009, 0.3)]
OPEN = [(0.0002, math.inf, 0.3)]
GROWING = [(0.0002 * 2 ** i, math.inf, 0.5 ** (i + 1)) for i in range(3)]


def _dev(sc):
    return [sc[n].to(DEV) for n in ("anchor", "offset", "scaling", "feat", "grads", "seen")]


@pytest.mark.parametrize("levels", [BAND, OPEN], ids=["band", "open"])
def test_grow_level_on_both_sides_of_every_threshold(levels):
    """thr_lo is `>=`, a finite thr_hi a strict `<`, rand a strict `>`; NaN and -inf are never candidates; +inf is one iff thr_hi is +inf (Scaffold-GS
    and the Octree pass B have no upper threshold: the kernel rejected it while it compared g < +inf)."""
    from gsrast import anchors
    lo, hi, rt = levels[0]
    sc = E.scene(levels, seed=21)
    host = [sc[n] for n in ("anchor", "offset", "scaling", "feat", "grads", "seen")]
    want_a, want_f = R.grow_level(*host, cell=E.CELL, thr_lo=lo, thr_hi=hi, rand=sc["rand"][0], rand_thr=rt)
    got_a, got_f = anchors.grow_level(*_dev(sc), cell=E.CELL, thr_lo=lo, thr_hi=hi, rand=sc["rand"][0].to(DEV), rand_thr=rt)
    names = E.names_of(sc, 0, got_a)
    assert names == E.expected_names(sc, 0), sorted(set(names) ^ set(E.expected_names(sc, 0)))
    assert ((0, "+inf", "grad") in names) == (levels is OPEN) and (0, "lo", "on") in names and (0, "rand", "on") not in names
    assert got_a.shape == want_a.shape and torch.equal(got_a.cpu(), want_a) and torch.equal(got_f.cpu(), want_f)
    if levels is OPEN:                                              # the default thr_hi is the same open end
        again, _ = anchors.grow_level(*_dev(sc), cell=E.CELL, thr_lo=lo, rand=sc["rand"][0].to(DEV), rand_thr=rt)
        assert torch.equal(again, got_a)


def test_anchor_growing_on_both_sides_of_every_level_threshold():
    """Three levels with the thresholds as anchors.anchor_growing computes them: threshold * 2 ** i against the gradient, 0.5 ** (i + 1) against the draw."""
    from gsrast import anchors
    sc = E.scene(GROWING, seed=22)
    host = [sc[n] for n in ("anchor", "offset", "scaling", "feat", "grads", "seen")]
    kw = dict(voxel_size=E.CELL / 16, n_offsets=E.K)
    want, counts = R.anchor_growing(*host, 0.0002, rand=sc["rand"], **kw)
    got = anchors.anchor_growing(*_dev(sc), 0.0002, rand=[x.to(DEV) for x in sc["rand"]], **kw)
    assert all(c > 0 for c in counts) and got["anchor"].shape[0] == sum(counts)
    p = 0
    for l, c in enumerate(counts):
        names = E.names_of(sc, l, got["anchor"][p:p + c])
        assert names == E.expected_names(sc, l), (l, sorted(set(names) ^ set(E.expected_names(sc, l))))
        assert (l, "+inf", "grad") in names and (l, "nan", "grad") not in names
        p += c
    for n in NAMES:
        assert got[n].shape == want[n].shape and torch.equal(got[n].cpu(), want[n]), n
