"""Octree-GS anchor growing + pruning on the device (gsrast.anchors.octree_adjust_anchor_, gsrast.octree.weed_out; gs-sr_amd/csrc/gsr_anchor.hip).
Whole calls are compared by exact equality: against the fixtures the reference's own OctreeGaussian.adjust_anchor produced
(tests/golden/make_golden_anchor_octree.py, whose margins keep that honest) and, on randomised scenes without a knife edge, against the torch
restatement that test_anchor_octree_cpu.py holds to those fixtures.  The weed-out alone is compared with a float64 evaluation.  The knife edges
those scenes avoid have tests of their own at the end: the visible threshold and the gradient band on both sides (tests/anchor_edge_cases.py)."""
import functools
import glob
import math
import os
import warnings

import numpy as np
import pytest
import torch

import ref_anchor_octree_torch as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_anchor_octree_*.npz")))
DEV = "cuda:0"
NAMES = R.NAMES
ACCS = R.ACCS
MODES = ("floor", "round", "ceil")


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
    m.n_offsets, m.levels, m.fork = int(fx["k"]), int(fx["levels"]), int(fx["fork"])
    m.voxel_size, m.init_pos, m.standard_dist = fx["voxel_size"].to(DEV), fx["init_pos"].to(DEV), fx["standard_dist"].to(DEV)      # device tensors, as the reference holds them
    m.cam_infos, m.visible_threshold, m.dist2level = fx["cam_infos"].to(DEV), float(fx["visible_threshold"]), MODES[int(fx["dist2level"])]
    m.progressive, m.coarse_intervals = bool(fx["progressive"]), [float(v) for v in fx["coarse_intervals"]]
    m._level, m._extra_level = fx["in_level"].to(DEV), fx["in_extra_level"].to(DEV)
    m.optimizer = opt_cls([{"params": [getattr(m, "_" + n)], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        m.optimizer.state[getattr(m, "_" + n)] = {"step": torch.tensor(1.0), "exp_avg": fx["m_" + n].to(DEV), "exp_avg_sq": fx["v_" + n].to(DEV)}
    return m


def pass_counts(trace, levels):
    found, kept = torch.zeros(levels, 2, dtype=torch.int64), torch.zeros(levels, 2, dtype=torch.int64)
    for l, which, f, k in trace:
        found[l, "AB".index(which)], kept[l, "AB".index(which)] = f, k
    return found, kept


def check_against(m, Na, trace, fx, want):
    """The model after the call against `want` = a fixture's results or the restatement's, exactly."""
    keep = want["keep"]
    U = want["new_anchor"].shape[0]
    assert Na == int(keep.sum()) + U
    found, kept = pass_counts(trace, int(fx["levels"]))
    assert torch.equal(found, want["pass_found"]) and torch.equal(kept, want["pass_kept"]), (found.tolist(), kept.tolist())
    for n in NAMES:
        p = getattr(m, "_" + n)
        w = torch.cat((fx["in_" + n][keep], want["new_" + n]))
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert p.shape == w.shape and torch.equal(p.detach().cpu(), w), n
        group = [g for g in m.optimizer.param_groups if g["name"] == n][0]
        assert group["params"][0] is p and len(m.optimizer.state) == len(NAMES)
        st = m.optimizer.state[p]
        assert float(st["step"]) == 1.0
        for key, src in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            wm = torch.cat((fx[src + n][keep], torch.zeros_like(want["new_" + n])))
            assert st[key].shape == p.shape and torch.equal(st[key].cpu(), wm), (n, key)
    for n in ACCS:
        assert torch.equal(getattr(m, n).cpu(), want["out_" + n]), n
    assert m._level.dtype == want["out_level"].dtype and torch.equal(m._level.cpu(), want["out_level"])
    assert m._extra_level.dtype == torch.float32 and torch.equal(m._extra_level.cpu(), want["out_extra_level"])


@pytest.mark.parametrize("opt", ["gsrast", "torch"])
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_octree_adjust_anchor_equals_reference_fixture(path, opt):
    from gsrast import anchors
    fx = {k: torch.tensor(v) for k, v in np.load(path).items()}
    m = make_model(fx, _optimizers()[opt])
    trace = []
    Na = anchors.octree_adjust_anchor_(m, int(fx["iteration"]), trace=trace)
    check_against(m, Na, trace, fx, fx)
    for n in NAMES:                                                  # the carried state serves a following step
        getattr(m, "_" + n).grad = torch.ones_like(getattr(m, "_" + n))
    m.optimizer.step()
    torch.cuda.synchronize()
    for n in NAMES:
        st = m.optimizer.state[getattr(m, "_" + n)]
        assert float(st["step"]) == 2.0 and bool(torch.isfinite(st["exp_avg"]).all())


# ------------------------------------------------------------------------------------------------------------------------ the weed-out alone
WEED = dict(levels=6, sd=16.0, fork=2, thr=0.35)


def close_pairs(pos, cams, mode):
    """Per row, the (row, camera) pairs whose float64 pred lies within 1e-5 of a rounding boundary of `mode`; and pred."""
    pred = R.pred_levels(pos, cams, WEED["sd"], WEED["fork"], torch.float64)
    shift = 0.5 if mode == "round" else 0.0
    return ((pred - shift - torch.round(pred - shift)).abs() < 1e-5).sum(dim=1), pred


def weed_inputs(U, C, seed):
    """Positions in a unit box, levels 0..5, cameras at log-spread distances 1.5 .. 40 (pred runs over -2.3 .. 3.4 around standard_dist 16).
    Drawn again, by seed, until at most 1 % of the rows hold a pair within 1e-5 of a boundary (one such row is already too many among 63)."""
    for s in range(seed, seed + 50):
        r = np.random.default_rng(s)
        pos = r.uniform(-0.5, 0.5, (U, 3)).astype(np.float32)
        lv = r.integers(0, 6, U).astype(np.int32)
        v = r.normal(size=(C, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        d = np.exp(r.uniform(np.log(1.5), np.log(40.0), C))
        cams = np.concatenate([v * d[:, None], r.choice([1.0, 2.0], (C, 1))], 1).astype(np.float32)
        pos, lv, cams = torch.tensor(pos), torch.tensor(lv), torch.tensor(cams)
        if all(int((close_pairs(pos, cams, mode)[0] > 0).sum()) <= 0.01 * U for mode in MODES):
            return pos, lv, cams
    raise AssertionError("no seed gives inputs with at most 1 % of rows near a boundary")


@pytest.mark.parametrize("C", ["one", "chunk", "chunk+1"])
@pytest.mark.parametrize("U", [0, 1, 63, 64, 65, 1025, 4099])
def test_weed_out_against_float64(U, C):
    """visible_count equals the float64 evaluation on every row without a (row, camera) pred within 1e-5 of a rounding boundary; a row with such
    pairs may differ by their number at most, and such rows are at most 1 % of all: float32 and float64 differ by 3.7e-7 here, one ulp of log2 at
    |pred| < 16 is 9.5e-7."""
    from gsrast import _rows, octree
    Cn = {"one": 1, "chunk": _rows.WEED_CHUNK, "chunk+1": _rows.WEED_CHUNK + 1}[C]
    levels, sd, fork, thr = WEED["levels"], WEED["sd"], WEED["fork"], WEED["thr"]
    pos, lv, cams = weed_inputs(U, Cn, seed=1000 * Cn + U)
    for mode in MODES:
        count, keep = octree.weed_out(pos.to(DEV), lv.to(DEV), cams.to(DEV), sd, fork, levels, mode, thr)
        assert count.dtype == torch.int32 and keep.dtype == torch.bool and count.shape == (U,) and keep.shape == (U,)
        close, pred = close_pairs(pos, cams, mode)
        want = (lv.reshape(-1, 1) <= R.int_levels(pred, levels, mode)).sum(dim=1).to(torch.int32)
        diff = (count.cpu() - want).abs()
        print(f"U {U} C {Cn} {mode}: rows with a close pair {int((close > 0).sum())}, rows that differ {int((diff > 0).sum())}, kept {int(keep.sum())}")
        assert int((close > 0).sum()) <= 0.01 * U
        assert bool((diff <= close).all())
        assert torch.equal(keep.cpu(), count.cpu().float() / float(Cn) > torch.tensor(thr))
        if U >= 63 and Cn > 1:
            assert 0 < int(keep.sum()) < U


def test_weed_out_at_a_camera_centre_and_far_away():
    """A position that coincides with a camera centre has dist 0 and pred +inf: clamped in floating point, before the integer conversion, it gives
    level levels - 1, so the camera admits every level.  At 1e7 pred is about -20, and beyond the range of float32's d^2 it is -inf: level 0 only."""
    from gsrast import octree
    levels, sd, fork = WEED["levels"], WEED["sd"], WEED["fork"]
    cams = torch.tensor([[1.0, 2.0, 3.0, 1.0]])
    pos = torch.tensor([[1.0, 2.0, 3.0]] * levels + [[0.0, 0.0, 1e7]] * 2 + [[0.0, 3e19, 0.0]] * 2)
    lv = torch.tensor(list(range(levels)) + [0, 1, 0, 1], dtype=torch.int32)
    want = torch.tensor([1] * levels + [1, 0, 1, 0], dtype=torch.int32)
    for mode in MODES:
        assert torch.equal(R.weed_out(pos, lv, cams, sd, fork, levels, mode, 0.5)[0], want), mode          # the restatement, float32 on the host
        count, keep = octree.weed_out(pos.to(DEV), lv.to(DEV), cams.to(DEV), sd, fork, levels, mode, 0.5)
        assert torch.equal(count.cpu(), want) and torch.equal(keep.cpu(), want > 0), (mode, count.tolist())


# ------------------------------------------------------------------------------------------------------------------------ occupancy apart from candidacy
def tiny_model(dist2level="round", voxel_size=1.0):
    """Two anchors, k = 1, two levels about the origin: anchor 0 of level 0 at the cell (2, 2, 2) with a strong gradient and a zero offset, so that its
    one candidate sits in the FINE cell (4, 4, 4) that holds anchor 0 itself; anchor 1 of level 1 far away in the fine cell (40, 40, 40)."""
    t = lambda x, dt=torch.float32: torch.tensor(x, dtype=dt, device=DEV)
    vs = voxel_size
    m = Model()
    m._anchor = torch.nn.Parameter(t([[2 * vs, 2 * vs, 2 * vs], [20 * vs, 20 * vs, 20 * vs]]))
    m._offset = torch.nn.Parameter(torch.zeros(2, 1, 3, device=DEV))
    m._anchor_feat = torch.nn.Parameter(t([[1.0, 2.0], [3.0, 4.0]]))
    m._opacity = torch.nn.Parameter(torch.zeros(2, 1, device=DEV))
    m._scaling = torch.nn.Parameter(torch.zeros(2, 6, device=DEV))
    m._rotation = torch.nn.Parameter(t([[1.0, 0, 0, 0], [1.0, 0, 0, 0]]))
    m.get_scaling = torch.ones(2, 6, device=DEV)
    m.opacity_accum, m.anchor_demon = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    m.offset_gradient_accum, m.offset_denom = t([[1.0], [0.0]]), t([[100.0], [0.0]])          # anchor 0: g = 0.01 >= every threshold; anchor 1: unseen
    m.n_offsets, m.levels, m.fork, m.voxel_size, m.init_pos, m.standard_dist = 1, 2, 2, vs, torch.zeros(3, device=DEV), 8.0 * vs
    m.cam_infos = t([[2 * vs, 2 * vs, 3 * vs, 1.0]])                                         # one camera a cell away: pred = 3, every level is visible
    m.visible_threshold, m.dist2level, m.progressive, m.coarse_intervals = 0.5, dist2level, False, []
    m._level, m._extra_level = t([[0], [1]], torch.int32), torch.zeros(2, device=DEV)
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, "_" + n)], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    return m


def test_pass_b_occupancy_is_level_l_plus_1_only():
    """The candidate's fine cell holds a level-0 anchor (its owner) and no level-1 anchor: pass B adds it.  With one shared mask the owner would
    occupy the fine cell and nothing would be added."""
    from gsrast import anchors
    m = tiny_model()
    trace = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            Na = anchors.octree_adjust_anchor_(m, 3000, trace=trace)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = sum(1 for x in w if "synchroniz" in str(x.message).lower())
    assert trace == [(0, "A", 0, 0), (0, "B", 1, 1), (1, "A", 0, 0)], trace                  # pass A: g lies above its band
    assert syncs <= len(trace) + 2, syncs                                                    # one read per pass, the level histogram, the kept rows
    assert Na == 3 and torch.equal(m._anchor.detach().cpu(), torch.tensor([[2.0, 2, 2], [20.0, 20, 20], [2.0, 2, 2]]))
    assert torch.equal(m._level.cpu(), torch.tensor([[0.0], [1.0], [1.0]])) and m._level.dtype == torch.float32
    assert torch.equal(m._anchor_feat.detach().cpu(), torch.tensor([[1.0, 2.0], [3.0, 4.0], [0.0, 0.0]]))       # pass B: feature zeros
    assert torch.allclose(m._scaling.detach().cpu()[2], torch.full((6,), math.log(0.5)), rtol=1e-6, atol=0.0)
    assert torch.equal(m._extra_level.cpu(), torch.tensor([0.5, 0.0, 0.0]))                  # anchor 0 exceeds the extra threshold at both levels
    # the level itself: occupancy given apart from candidacy adds the cell, the shared mask does not
    a = dict(cell=0.5, thr_lo=0.001, origin=(0.0, 0.0, 0.0))
    m = tiny_model()
    args = (m._anchor.detach(), m._offset.detach(), m.get_scaling, m._anchor_feat.detach(), torch.tensor([0.01, 0.0], device=DEV),
            torch.tensor([True, False], device=DEV))
    is0, is1 = torch.tensor([True, False], device=DEV), torch.tensor([False, True], device=DEV)
    got, _ = anchors.grow_level(*args, mask=is0, occupy=is1, **a)
    assert torch.equal(got.cpu(), torch.tensor([[2.0, 2, 2]]))
    got, _ = anchors.grow_level(*args, mask=is0, **a)
    assert got.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------------ randomised whole calls
CAM_PRED = (5.25, 4.25, 4.25, 3.25, 2.25, 2.25, 1.25, 0.25, -0.75)       # each 0.25 from the boundaries of floor, round and ceil


def random_case(N, k, F, seed, mode="round"):
    """Anchors of 6 levels on the octree lattice of a box (several per cell at times, free cells between them), offsets that reach a few cells.
    Every camera lies at least 40 scene extents away, at the distance that puts pred = CAM_PRED[c] at the scene's centre: over the whole box pred
    moves by less than log2(1 + 1/80) = 0.018, so it stays 0.2 from every boundary and the weed-out is decided per level -- no knife edge."""
    r = np.random.default_rng(seed)
    levels, fork, vs = 6, 2, 0.64
    init_pos = np.array([-3.3, 0.7, 11.0], np.float32)
    lvl = r.integers(0, levels, N).astype(np.int32)
    size = (np.float32(vs) / np.float32(2.0) ** lvl.astype(np.float32)).astype(np.float32)
    side = max(4, int(round((N / levels * 6) ** (1 / 3))))
    anchor = (np.round(r.uniform(0, side, (N, 3))) * size[:, None] + init_pos).astype(np.float32)
    scaling = (r.uniform(0.5, 3.0, (N, 6)) * size[:, None]).astype(np.float32)
    denom = r.integers(0, 100, (N * k, 1)).astype(np.float32)
    demon = r.integers(0, 121, (N, 1)).astype(np.float32)
    lo, hi = anchor.min(0) - 4 * vs, anchor.max(0) + 4 * vs
    centre, extent = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    sd = 40.0 * extent * 2.0 ** max(CAM_PRED)
    v = r.normal(size=(len(CAM_PRED), 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    cams = np.concatenate([centre + v * (sd / 2.0 ** np.array(CAM_PRED))[:, None], np.ones((len(CAM_PRED), 1))], 1).astype(np.float32)
    fx = {"k": k, "levels": levels, "fork": fork, "voxel_size": np.float32(vs), "init_pos": init_pos, "standard_dist": np.float32(sd), "visible_threshold": 0.3,
          "dist2level": MODES.index(mode), "progressive": 0, "iteration": 3000, "coarse_intervals": np.array([0.0]), "cam_infos": cams, "scaling_act": scaling,
          "in_level": lvl.reshape(-1, 1), "in_extra_level": (r.integers(0, 4, N) * 0.25).astype(np.float32),
          "in_anchor": anchor, "in_offset": r.uniform(-1, 1, (N, k, 3)).astype(np.float32), "in_anchor_feat": r.normal(0, 1, (N, F)).astype(np.float32),
          "in_opacity": r.normal(0, 1, (N, 1)).astype(np.float32), "in_scaling": np.log(scaling), "in_rotation": r.normal(0, 1, (N, 4)).astype(np.float32),
          "in_offset_denom": denom, "in_offset_gradient_accum": (denom * np.exp(r.normal(math.log(4e-4), 1.0, (N * k, 1)))).astype(np.float32),
          "in_anchor_demon": demon, "in_opacity_accum": (demon * r.uniform(0.0, 0.02, (N, 1))).astype(np.float32)}
    fx = {n: torch.tensor(x) for n, x in fx.items()}
    for n in NAMES:
        fx["m_" + n] = torch.full_like(fx["in_" + n], 0.25); fx["v_" + n] = torch.full_like(fx["in_" + n], 0.0625)
    pred = R.pred_levels(torch.tensor(np.stack([lo, hi, centre])), fx["cam_infos"], float(sd), fork, torch.float64)
    assert float((pred - torch.tensor(CAM_PRED, dtype=torch.float64)).abs().max()) < 0.05       # the box's corners: no knife edge
    return fx


@functools.lru_cache(maxsize=None)
def random_case_and_restatement(N, k, F):
    fx = random_case(N, k, F, seed=N % 97)
    return fx, R.adjust(fx)


@pytest.mark.parametrize("N,k,F", [(77777, 3, 5), (200000, 10, 32)])
def test_octree_adjust_anchor_equals_restatement(N, k, F):
    from gsrast import anchors
    fx, want = random_case_and_restatement(N, k, F)
    found, kept = want["pass_found"], want["pass_kept"]
    assert int((kept[:, 0] > 0).sum()) >= 3 and int((kept[:, 1] > 0).sum()) >= 3 and not bool(want["keep"].all())
    assert bool(((found > 0) & (kept == 0)).any()) and not bool(((kept > 0) & (kept < found)).any())      # weeded per level: all or nothing
    state = []
    for _ in range(2):
        m = make_model(fx, _optimizers()["gsrast"])
        trace = []
        Na = anchors.octree_adjust_anchor_(m, 3000, trace=trace)
        check_against(m, Na, trace, fx, want)
        state.append([getattr(m, "_" + n).detach() for n in NAMES] + [getattr(m, n) for n in ACCS] + [m._level, m._extra_level])
    for a, b in zip(*state):
        assert torch.equal(a, b)                                     # bitwise deterministic


# ------------------------------------------------------------------------------------------------------------------------ errors
def test_errors():
    from gsrast import anchors, octree
    with pytest.raises(RuntimeError, match="progressive"):
        anchors.octree_adjust_anchor_(tiny_model(dist2level="progressive"), 3000)
    pos, lv, cams = (x.to(DEV) for x in weed_inputs(10, 3, 0))
    with pytest.raises(RuntimeError, match="progressive"):
        octree.weed_out(pos, lv, cams, 16.0, 2, 6, "progressive", 0.3)
    with pytest.raises(RuntimeError, match="packing range"):         # cells of 1e-7: the candidate two units from the origin lies beyond 2^20 cells
        m = tiny_model(voxel_size=1.0)
        m.voxel_size = 1e-7
        anchors.octree_adjust_anchor_(m, 3000)
    m = tiny_model()
    m.cam_infos = m.cam_infos.cpu()
    with pytest.raises(RuntimeError, match="cam_infos must be a CUDA tensor"):
        anchors.octree_adjust_anchor_(m, 3000)
    m = tiny_model()
    m._extra_level = m._extra_level.cpu()
    with pytest.raises(RuntimeError, match="model._extra_level must be a CUDA tensor"):
        anchors.octree_adjust_anchor_(m, 3000)
    m = tiny_model()
    del m.standard_dist
    with pytest.raises(RuntimeError, match="attribute standard_dist is missing"):
        anchors.octree_adjust_anchor_(m, 3000)
    with pytest.raises(RuntimeError, match="positions must be a CUDA tensor"):
        octree.weed_out(pos.cpu(), lv, cams, 16.0, 2, 6, "round", 0.3)


# ------------------------------------------------------------------------------------------------------------------------ the selection thresholds
import anchor_edge_cases as E                                      # noqa: E402


@pytest.mark.parametrize("case", list(E.WEED_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_weed_out_on_both_sides_of_the_visible_threshold(case, mode):
    """Positions that exactly t*C - 1, t*C and t*C + 1 cameras admit (pred 0.25 from every boundary): visible / C > t is strict, so t*C itself is
    dropped -- 2/8 against 0.25, 3/10 against float32(0.3) (the quotient rounds to the same float), 65/260 with the count carried over two LDS chunks."""
    from gsrast import octree
    C, t_count, thr = E.WEED_CASES[case]
    pos, lv, cams, visible, _ = E.weed_case(C, t_count, seed=C, mode=mode)
    want_count, want_keep = R.weed_out(pos, lv, cams, E.WEED["sd"], E.WEED["fork"], E.WEED["levels"], mode, thr)
    count, keep = octree.weed_out(pos.to(DEV), lv.to(DEV), cams.to(DEV), E.WEED["sd"], E.WEED["fork"], E.WEED["levels"], mode, thr)
    assert torch.equal(count.cpu(), visible) and torch.equal(want_count, visible), count.tolist()
    assert torch.equal(keep.cpu(), visible > t_count) and torch.equal(keep.cpu(), want_keep), keep.tolist()


def test_octree_passes_and_an_infinite_gradient():
    """The level with the Octree loop's arguments (per-anchor mask, occupancy apart): pass A's band [thr, ds_thr) rejects a gradient of +inf, pass B
    (no upper threshold) admits it."""
    from gsrast import anchors
    sc = E.scene([(0.0002, 0.0009, 0.3)], seed=31)
    host = [sc[n] for n in ("anchor", "offset", "scaling", "feat", "grads", "seen")]
    dev = [t.to(DEV) for t in host]
    mask = torch.ones(E.N_ANCHORS, dtype=torch.bool)
    for thr_hi, level_names in ((0.0009, [(0.0002, 0.0009, 0.3)]), (math.inf, [(0.0002, math.inf, 0.3)])):
        sc["levels"] = level_names
        want_a, want_f = R.grow_pass(sc["anchor"], mask, sc["offset"], sc["scaling"], sc["feat"], sc["grads"],
                                     (sc["grads"] >= torch.tensor(0.0002)) & ((sc["grads"] < torch.tensor(thr_hi)) if thr_hi != math.inf else mask.repeat_interleave(E.K))
                                     & (sc["rand"][0] > torch.tensor(0.3)), cell=E.CELL, origin=(0.0, 0.0, 0.0))
        got_a, got_f = anchors.grow_level(*dev, cell=E.CELL, thr_lo=0.0002, thr_hi=thr_hi, rand=sc["rand"][0].to(DEV), rand_thr=0.3, mask=mask.to(DEV),
                                          occupy=mask.to(DEV))
        names = E.names_of(sc, 0, got_a)
        assert names == E.expected_names(sc, 0) and ((0, "+inf", "grad") in names) == (thr_hi == math.inf)
        assert torch.equal(got_a.cpu(), want_a) and torch.equal(got_f.cpu(), want_f)
