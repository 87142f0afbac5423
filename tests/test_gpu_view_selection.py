"""GPU: the PGSR neighbour views on the device (gsrast.views; gs-sr_amd/csrc/gsr_views.hip).

Golden scenes: what the reference's own view_selection / calc_score produced (tests/golden/make_golden_view_selection.py).  Edges: the numpy
restatement of the reference (tests/ref_view_selection.py, held to the fixtures exactly by tests/test_view_selection_cpu.py) at the sizes where the
kernels change path: one and two images, C around num_views, tracks around the 64 lanes of the scoring wave and past two of its rounds, observation
counts around the 1024-key sort block, ids that need the sort's high word, an LDS row past 64 KiB.

Tolerance.  Selected indices are compared exactly; scores to a relative 2e-10.  Every term is positive, so the error of a sum is relative.  A few ulps
of the cosine move the angle by at most 57.3 * 4.4e-16 / sin(0.1 deg) = 1.5e-11 degrees for angles in [0.1, 179.9] degrees; a term's relative
sensitivity is |theta - theta0| / s^2 <= 5 per degree for angles below theta0 (s = 1) and <= 1.75 above (s = 10): below 1e-10 together, and summing
n positive terms in another order adds about n * 1e-16.  Every scene is drawn (by seed, on the host) so that its angles lie in that range and any two
different scores among a row's top k + 1 differ by a relative 1e-6 -- four orders above the tolerance -- so the exact comparison of the indices is
never skipped; exactly equal scores (zeros) follow the tie rule on both sides."""
import functools
import glob
import os
import types
import warnings

import numpy as np
import pytest
import torch

import ref_view_selection as rvs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_view_selection_*.npz")))
DEV = "cuda:0"
RTOL = 2e-10
WAVE, SORT_BLOCK = 64, 1024          # csrc/gsr_views.hip VW_WAVE; csrc/gsr_common.h GSR_SORT_BLOCK
PARAMS = (5, 1, 10)


def count_syncs(fn):
    """Host synchronisations of fn() as torch's sync debug mode reports them (tests/test_gpu_create_anchors.py's way)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower()), out


def build(centers, ids_per_image, point_ids, xyz):
    off = np.zeros(len(ids_per_image) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in ids_per_image])
    flat = np.concatenate([np.asarray(a, np.int64).reshape(-1) for a in ids_per_image]) if len(ids_per_image) else np.zeros(0, np.int64)
    order = np.argsort(point_ids, kind="stable")
    return dict(centers=np.asarray(centers, np.float64).reshape(-1, 3), obs_offsets=off, obs_ids=flat.astype(np.int64),
                point_ids=np.asarray(point_ids, np.int64)[order], point_xyz=np.asarray(xyz, np.float64).reshape(-1, 3)[order])


def ring(C, r, z=0.6):
    """C cameras on a loose ring, evenly spread with jitter: no two see a point under less than a fraction of a degree."""
    ang = 2 * np.pi * (np.arange(C) + 0.3 * r.uniform(-1, 1, C)) / max(C, 1)
    rad = r.uniform(3.0, 4.5, C)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), r.uniform(-z, z, C)], axis=1)


def draw(C, n_points, per_image, seed, tracks=(), id_of=None, pad_to=None, empty=True):
    """A random scene: image a observes `per_image` random points, plus repeats, -1 entries and an orphan id (no table row, seen by this image only);
    point t of `tracks` is observed by exactly the first tracks[t] images; one image is left without a valid observation (empty).  id_of maps the
    point's number to its id.  pad_to: single-image orphan ids are added to image 0 until the scene has exactly pad_to observations != -1."""
    r = np.random.default_rng(seed)
    id_of = id_of or (lambda i: 7 * i + 3)
    nt = len(tracks)
    point_ids = np.array([id_of(i) for i in range(n_points)], np.int64)
    xyz = r.normal(0, 0.45, (n_points, 3))
    hole = int(r.integers(1, C - 1)) if empty and C > 2 and not tracks else -1
    ids = []
    for a in range(C):
        if a == hole:
            ids.append(np.full(3, -1, np.int64))
            continue
        seen = [t for t in range(nt) if a < tracks[t]] + (nt + r.choice(n_points - nt, min(per_image, n_points - nt), replace=False)).tolist()
        row = point_ids[seen]
        row = np.concatenate([row, r.choice(row, 2), np.full(2, -1, np.int64), [id_of(n_points + 1 + a)]]) if len(row) else np.full(2, -1, np.int64)
        ids.append(r.permutation(row).astype(np.int64))
    if pad_to is not None:
        have = int(sum((a != -1).sum() for a in ids))
        assert have <= pad_to
        ids[0] = np.concatenate([ids[0], [id_of(n_points + 1 + C + i) for i in range(pad_to - have)]]).astype(np.int64)
    return build(ring(C, r), ids, point_ids, xyz)


def truth(sc, nv):
    score, angles = rvs.scores(sc["centers"], sc["obs_offsets"], sc["obs_ids"], sc["point_ids"], sc["point_xyz"], *PARAMS, with_angles=True)
    return score, (min(angles) if angles else 90.0), (max(angles) if angles else 90.0), rvs.top_gap(score, nv)


@functools.lru_cache(maxsize=None)
def scene(C, n_points, per_image, nv, tracks=(), wide=False, pad_to=None):
    """The first seed whose scene meets the margins, and its truth -- computed once, shared by the tests."""
    id_of = (lambda i: (i % 7) * (1 << 32) + 1000 + 13 * (i // 7)) if wide else None      # seven ids share every low word; the first of them fits 32 bits
    for seed in range(40):
        sc = draw(C, n_points, per_image, seed, tracks, id_of, pad_to)
        if len(np.unique(sc["point_ids"])) != len(sc["point_ids"]):
            continue
        score, lo, hi, gap = truth(sc, nv)
        if lo >= 0.1 and hi <= 179.9 and gap >= 1e-6:
            return sc, score
    raise AssertionError("no seed meets the margins")


def on_device(sc):
    return tuple(torch.from_numpy(sc[n]).to(DEV) for n in ("centers", "obs_offsets", "obs_ids", "point_ids", "point_xyz"))


def select(sc, nv, **kw):
    from gsrast import views
    ids, val, S = views.select_views(*on_device(sc), *PARAMS, num_views=nv, return_scores=True, **kw)
    assert ids.dtype == torch.int32 and val.dtype == torch.float64 and S.dtype == torch.float64
    return ids.cpu().numpy(), val.cpu().numpy(), S.cpu().numpy()


def check(sc, score, nv, **kw):
    """Indices exactly (the scene's margins hold by construction), scores to RTOL, and what must hold bit for bit."""
    ids, val, S = select(sc, nv, **kw)
    C = len(sc["centers"])
    k = min(nv, C)
    want_ids, want_val = rvs.rank(score, nv)
    assert ids.shape == val.shape == (C, k) and S.shape == (C, C)
    err = np.abs(S - score)
    rel = float((err[score > 0] / score[score > 0]).max()) if (score > 0).any() else 0.0
    print(f"C {C} k {k} observations {len(sc['obs_ids'])}: max relative score error {rel:.3g}")
    assert np.array_equal(S == 0, score == 0), "a pair without a shared point scores exactly 0, and only such a pair"
    assert (err <= RTOL * score).all(), rel
    assert np.array_equal(S, S.T), "S[a,b] and S[b,a] are the same bits"
    assert np.array_equal(val, np.take_along_axis(S, ids.astype(np.int64), axis=1)), "near_scores are the matrix's entries"
    assert np.array_equal(ids, want_ids), "the selected images, every row"
    assert (np.abs(val - want_val) <= RTOL * want_val).all()
    return ids, val, S


# ---------------------------------------------------------------------------------------------------------------- golden scenes
@pytest.mark.parametrize("name", SCENES)
def test_golden_scene(name):
    z = np.load(os.path.join(GOLDEN, name))
    nv = int(z["params"][3])
    assert tuple(z["params"][:3]) == PARAMS
    sc = {n: z[n] for n in ("centers", "obs_offsets", "obs_ids", "point_ids", "point_xyz")}
    ids, val, S = select(sc, nv)
    rel = np.abs(S - z["scores"])[z["scores"] > 0] / z["scores"][z["scores"] > 0]
    print(f"{name}: max relative score error {rel.max():.3g}")
    assert np.array_equal(ids, z["sel_ids"]), "near_ids equal the reference's, in every row"
    assert (np.abs(S - z["scores"]) <= RTOL * z["scores"]).all() and (np.abs(val - z["sel_scores"]) <= RTOL * z["sel_scores"]).all()
    assert np.array_equal(S, S.T) and not S.diagonal().any()
    from gsrast import views
    ids32, val32 = (x.cpu().numpy() for x in views.select_views(*on_device(sc), *PARAMS, num_views=nv, wide_ids=False))
    assert np.array_equal(ids32, ids) and np.array_equal(val32, val), "without the high-word passes: the same bits"


def test_view_selection_takes_and_returns_what_the_reference_does(tmp_path):
    from gsrast import views
    z = np.load(os.path.join(GOLDEN, "ref_view_selection_c12.npz"))
    nv = int(z["params"][3])
    points3d = {int(i): types.SimpleNamespace(xyz=x) for i, x in zip(z["point_ids"], z["point_xyz"])}
    view_sel = views.view_selection([c for c in z["centers"]], rvs.images(z["obs_offsets"], z["obs_ids"]), points3d, *PARAMS, num_views=nv, device=DEV)
    assert isinstance(view_sel, list) and len(view_sel) == 12
    assert all(isinstance(row, list) and len(row) == nv and all(isinstance(p, tuple) and isinstance(p[0], int) and isinstance(p[1], float) for p in row)
               for row in view_sel)
    assert [[k for k, _ in row] for row in view_sel] == z["sel_ids"].tolist()
    got = np.array([[s for _, s in row] for row in view_sel])
    assert (np.abs(got - z["sel_scores"]) <= RTOL * z["sel_scores"]).all()
    path = str(tmp_path / "pair.txt")
    views.write_pairs(path, view_sel)
    assert open(path, "rb").read() == z["pair_txt"].tobytes(), "%d truncates: the scores' last bits do not reach the file"
    cams = {1.0: [types.SimpleNamespace() for _ in range(12)]}
    views.assign_near_ids(cams, view_sel)
    assert [c.near_ids for c in cams[1.0]] == z["sel_ids"].tolist()


# ---------------------------------------------------------------------------------------------------------------- edges against the restatement
@pytest.mark.parametrize("C", [1, 2, 5, 6])
def test_few_images(C):
    """One image, two, C = num_views (every row takes its own index last but for exact ties) and C = num_views + 1."""
    nv = 5
    sc, score = scene(C, 24, 9, nv)
    ids, val, S = check(sc, score, nv)
    if C <= nv:
        assert all(a in row for a, row in enumerate(ids.tolist())), "the own index competes with its score 0"
    if C == 1:
        assert ids.tolist() == [[0]] and val.tolist() == [[0.0]]


def test_tracks_of_length_one_and_no_observations_at_all():
    """No point is shared: every score is exactly 0 and every row is an exact tie -- the higher index first, the own index among them."""
    r = np.random.default_rng(3)
    ids = [np.array([10 * a + 1, -1, 10 * a + 2, 10 * a + 1]) for a in range(7)]
    sc = build(ring(7, r), ids, [11, 12, 21], r.normal(0, 0.4, (3, 3)))
    got, val, S = check(sc, np.zeros((7, 7)), 5)
    assert got.tolist() == [[6, 5, 4, 3, 2]] * 7 and not val.any() and not S.any()
    for ids in ([np.zeros(0, np.int64)] * 3, [np.full(4, -1)] * 3):
        sc = build(ring(3, r), ids, np.zeros(0, np.int64), np.zeros((0, 3)))
        got, val, S = check(sc, np.zeros((3, 3)), 10)
        assert got.tolist() == [[2, 1, 0]] * 3


def test_track_lengths_around_the_wave():
    """Tracks of 63, 64, 65 images (one lane short of the scoring wave, the wave, one past it) and of 128, 129, 130 (two rounds, one past them)."""
    tracks = (WAVE - 1, WAVE, WAVE + 1, 2 * WAVE, 2 * WAVE + 1, 2 * WAVE + 2)
    sc, score = scene(2 * WAVE + 2, 40, 4, 5, tracks=tracks)
    counts = np.unique(sc["obs_ids"][sc["obs_ids"] != -1], return_counts=True)[1]
    assert counts.max() >= 2 * WAVE + 2
    check(sc, score, 5)


@pytest.mark.parametrize("n_obs", [SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, 2 * SORT_BLOCK + 1])
def test_observation_counts_around_the_sort_block(n_obs):
    sc, score = scene(6, 60, 30, 5, pad_to=n_obs)
    assert int((sc["obs_ids"] != -1).sum()) == n_obs
    check(sc, score, 5)


@pytest.mark.parametrize("C", [256, 257])
def test_image_counts_around_one_digit_of_the_image_sort(C):
    """The (id, image) entries are sorted by image on img_bits = 8 bits for 256 images -- one pass, the result in the other pair of buffers -- and
    on 9 bits for 257: two balanced passes (5, 4), the result back in the first pair (GsrSort::advance).  More than two sort blocks of entries, their
    count on the device and below the capacity (the observations, -1 included)."""
    import sort_cases
    sc, score = scene(C, 400, 10, 5)
    imgs = rvs.images(sc["obs_offsets"], sc["obs_ids"])
    entries = sum(len(np.unique(a[a != -1])) for a in imgs)
    assert 2 * sort_cases.limits()["block"] < entries < len(sc["obs_ids"]) and sort_cases.path(len(sc["obs_ids"])).blocks > 2
    widths = sort_cases.passes(sort_cases.tile_bits(C))                      # img_bits is the same smallest b >= 1 with 2^b >= C
    assert widths == ([8] if C == 256 else [5, 4]) and sort_cases.result_swapped(sum(widths)) == (C == 256)
    check(sc, score, 5)


def test_ids_beyond_32_bits():
    """Ids up to 2^39, among them ids that differ in the high word only: the sort's high-word passes run, and are needed."""
    sc, score = scene(9, 50, 20, 5, wide=True)
    assert sc["point_ids"].max() >= 1 << 32
    low = sc["point_ids"] & 0xFFFFFFFF
    assert len(np.unique(low)) < len(low), "ids that share their low word"
    check(sc, score, 5)
    from gsrast import views
    with pytest.raises(RuntimeError, match="wide_ids=False but an id has bits above"):
        views.select_views(*on_device(sc), *PARAMS, num_views=5, wide_ids=False)
    # view_selection finds out by itself
    points3d = {int(i): types.SimpleNamespace(xyz=x) for i, x in zip(sc["point_ids"], sc["point_xyz"])}
    view_sel = views.view_selection(list(sc["centers"]), rvs.images(sc["obs_offsets"], sc["obs_ids"]), points3d, *PARAMS, num_views=5, device=DEV)
    assert [[k for k, _ in row] for row in view_sel] == rvs.rank(score, 5)[0].tolist()


def _pair_at(theta_deg, r0=3.0, r1=4.0):
    """Two centres that see the origin under theta_deg."""
    t = np.deg2rad(theta_deg)
    return [r0, 0.0, 0.0], [r1 * np.cos(t), r1 * np.sin(t), 0.0]


def test_angles_at_the_threshold():
    """theta just below and just above theta0 (the term is continuous there, the branch is not), and half a degree to either side, where sigma1 and
    sigma2 give different values."""
    thetas = [5 - 1e-7, 5 + 1e-7, 4.5, 5.5]
    centers, ids = [], []
    for n, th in enumerate(thetas):
        centers += _pair_at(th)
        ids += [[100 + n], [100 + n]]
    sc = build(centers, ids, [100 + n for n in range(4)], np.zeros((4, 3)))
    score, lo, hi, gap = truth(sc, 5)
    assert gap >= 1e-6 and 0.1 <= lo
    got, val, S = check(sc, score, 5)
    assert abs(S[4, 5] - np.exp(-0.125)) < 1e-9 and abs(S[6, 7] - np.exp(-0.00125)) < 1e-9          # sigma1 below theta0, sigma2 above
    assert abs(1 - S[0, 1]) < 1e-13 and abs(1 - S[2, 3]) < 1e-13


def test_multiplicity_counts_in_the_lower_indexed_image_only():
    c0, c1 = _pair_at(12.0)
    c2, c3 = _pair_at(12.0, 3.5, 3.25)
    sc = build([c0, c1, c2, c3], [[7, 7, -1, 7], [7], [9], [9, 9, 9]], [7, 9], np.zeros((2, 3)))
    score, _, _, gap = truth(sc, 5)
    assert gap >= 1e-6
    got, val, S = check(sc, score, 5)
    g = np.exp(-49 / 200)
    assert abs(S[0, 1] - 3 * g) < 1e-9 and abs(S[2, 3] - g) < 1e-9, "three times in image 0 counts three times, three times in image 3 once"


def test_an_lds_row_past_64_kib():
    """C = 8200 images: the row of scores takes more LDS than a workgroup gets by default.  Twenty images observe points (some of them beyond column
    8192), the others nothing; the truth is the restatement of those twenty, scattered."""
    from gsrast import views
    Cn, nv = 8200, 5
    sub, score = scene(20, 40, 12, nv)
    r = np.random.default_rng(0)
    at = np.sort(np.concatenate([[0, 8193, Cn - 1], r.choice(np.arange(1, 8190), 17, replace=False)]))
    imgs = rvs.images(sub["obs_offsets"], sub["obs_ids"])
    ids = [np.zeros(0, np.int64)] * Cn
    centers = ring(Cn, r)
    for n, a in enumerate(at):
        ids[a] = imgs[n]
        centers[a] = sub["centers"][n]
    sc = build(centers, ids, sub["point_ids"], sub["point_xyz"])
    near, val, S = views.select_views(*on_device(sc), *PARAMS, num_views=nv, return_scores=True)
    idx = torch.from_numpy(at).to(DEV)
    block = S[idx][:, idx].cpu().numpy()
    assert (np.abs(block - score) <= RTOL * score).all() and np.array_equal(block == 0, score == 0)
    assert int((S != 0).sum()) == int((score != 0).sum()), "nothing outside the twenty images' block"
    near, val = near.cpu().numpy(), val.cpu().numpy()
    rows = list(at) + [1, 4100, Cn - 2]
    full = np.zeros((len(rows), Cn))
    for n in range(20):
        full[n, at] = score[n]
    want, _ = rvs.rank(full, nv)
    assert np.array_equal(near[rows], want), "the observing images' rows and three empty ones (exact ties: the higher index first)"
    assert np.array_equal(val[rows], np.take_along_axis(S[torch.tensor(rows, device=DEV)].cpu().numpy(), want, axis=1))


# ---------------------------------------------------------------------------------------------------------------- failures, determinism, synchronisation
def test_an_absent_id_is_an_error_only_when_two_images_share_it():
    from gsrast import views
    sc, score = scene(6, 30, 10, 5)
    imgs = rvs.images(sc["obs_offsets"], sc["obs_ids"])
    orphan = int(sc["obs_ids"].max()) + 100
    assert orphan not in sc["point_ids"]
    one = build(sc["centers"], [np.concatenate([a, [orphan, orphan]]) if n == 0 else a for n, a in enumerate(imgs)], sc["point_ids"], sc["point_xyz"])
    check(one, score, 5)                                                                  # seen by one image, twice: never looked up
    two = build(sc["centers"], [np.concatenate([a, [orphan]]) if n in (0, 3) else a for n, a in enumerate(imgs)], sc["point_ids"], sc["point_xyz"])
    with pytest.raises(KeyError):
        rvs.scores(two["centers"], two["obs_offsets"], two["obs_ids"], two["point_ids"], two["point_xyz"], *PARAMS)
    with pytest.raises(RuntimeError, match="absent from the point table"):
        views.select_views(*on_device(two), *PARAMS, num_views=5)


def test_non_finite_values_raise():
    from gsrast import views
    sc, _ = scene(6, 30, 10, 5)
    bad = dict(sc, centers=sc["centers"].copy())
    bad["centers"][2, 1] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        views.select_views(*on_device(bad), *PARAMS, num_views=5)
    # a point on a camera centre: 0 / 0 in the cosine, which the reference leaves in the scores as NaN
    on = build([[1.0, 2.0, 3.0], [3.0, 0.0, 0.0]], [[5], [5]], [5], [[1.0, 2.0, 3.0]])
    with np.errstate(all="ignore"):
        assert np.isnan(rvs.scores(on["centers"], on["obs_offsets"], on["obs_ids"], on["point_ids"], on["point_xyz"], *PARAMS)[0, 1])
    with pytest.raises(RuntimeError, match="non-finite"):
        views.select_views(*on_device(on), *PARAMS, num_views=5)
    # the tables' own order is checked on the device as well
    args = list(on_device(sc))
    with pytest.raises(RuntimeError, match="point_ids does not ascend strictly"):
        views.select_views(args[0], args[1], args[2], args[3].flip(0).contiguous(), args[4], *PARAMS, num_views=5)
    with pytest.raises(RuntimeError, match="obs_offsets does not ascend from 0"):
        views.select_views(args[0], args[1] + 1, args[2], args[3], args[4], *PARAMS, num_views=5)


def test_two_calls_give_identical_bits_and_one_host_synchronisation():
    from gsrast import views
    sc, score = scene(2 * WAVE + 2, 40, 4, 5, tracks=(WAVE - 1, WAVE, WAVE + 1, 2 * WAVE, 2 * WAVE + 1, 2 * WAVE + 2))
    args = on_device(sc)
    views.select_views(*args, *PARAMS, num_views=5)                                       # the library is loaded, the allocator warm
    syncs, first = count_syncs(lambda: views.select_views(*args, *PARAMS, num_views=5, return_scores=True))
    assert syncs == 1, "one host read: the status word"
    second = views.select_views(*args, *PARAMS, num_views=5, return_scores=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(first[2], first[2].T)
    syncs, _ = count_syncs(lambda: views.select_views(*args, *PARAMS, num_views=5, wide_ids=False))
    assert syncs == 1
