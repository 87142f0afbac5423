"""GPU: the VastGaussian scene split on the device (gsrast.partition; gs-sr_amd/csrc/gsr_partition.hip).

Golden scenes: what the reference's own four functions produced (tests/golden/make_golden_partition.py), run end to end through the functions under the
reference's names.  Edges: the numpy restatement (tests/ref_partition.py, held to the fixtures exactly by tests/test_partition_cpu.py) at the sizes where
the kernels change path: the 256-point workgroup of the box pass, the 32-tile mask word, gsr_dist2's 256-point box, observation counts around 256 and 1024.

Tolerance.  Ids, their order, boxes, masks, counts, mz / Mz and rows are compared exactly.  ratio, d and md are float64 sums and quotients whose order
differs between numpy and the kernel, so they are held to the restatement within a bar that is measured, not chosen: the restatement is evaluated in
np.longdouble and in float64 on the very cases a test compares (a golden scene, the edge cameras, the random views), the largest difference is float64's
own floor on them (absolute for ratio, which lives in [0, 1]; relative for d and md), and the bar is 16 x that floor (floors(), printed by every test that uses it).
Measured: MEASURED_FLOORS below."""
import functools
import warnings

import numpy as np
import pytest
import torch

import partition_cases as pc
import ref_partition as rp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 256                                               # csrc/gsr_partition.hip PT_BLOCK
KNN_BOX = 256                                             # csrc/gsr_extra.hip GSR_KNN_BOX
MEASURED_FLOORS = ("floors per case, ratio (absolute) / d / md (relative): grid 4.4e-16 / 2.0e-16 / 1.5e-16, quad 5.3e-16 / 1.8e-16 / 5.3e-17, edge 1.4e-16 / 7.7e-17 / 3.4e-17, "
                   "edge_flat 2.7e-16 / 7.7e-17 / 4.3e-17, random 2.3e-15 / 1.8e-16 / 1.5e-16; bars 16 x those, e.g. ratio 7.1e-15 (grid), 2.3e-15 (edge), 3.7e-14 (random), "
                   "md 5.5e-16 (edge); the kernel on an MI355X: ratio within 3.4e-16 (grid), 1.2e-16 (quad), 5.6e-17 (random), 0 (edges); d and md equal to the "
                   "restatement's bits in every case")


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


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_mask(rows_per_tile, n):
    T = len(rows_per_tile)
    m = np.zeros((n, (T + 31) // 32), np.uint32)
    for k, rows in enumerate(rows_per_tile):
        if len(rows):
            m[np.asarray(rows, np.int64), k >> 5] |= np.uint32(1 << (k & 31))
    return m.view(np.int32)


def bits(mask, T):
    """int32 [n,W] (tensor) -> bool [T,n]."""
    m = mask.cpu().numpy().view(np.uint32)
    return np.array([(m[:, k >> 5] >> np.uint32(k & 31)) & 1 for k in range(T)], bool).reshape(T, -1)


# ---------------------------------------------------------------------------------------------------------------- visibility cases and the bar
W_, H_, F_ = 640.0, 480.0, 500.0
BOX = np.array([[0.0, 2.0, 0.0, 2.0]])


def cam(centre, target, roll=0.0, fx=F_, fy=F_, w=W_, h=H_):
    q, tv = rp.look_at(np.asarray(centre, np.float64), np.asarray(target, np.float64), roll)
    return rp.w2c(q, tv), np.asarray(centre, np.float64), [fx, fy, w, h]


EDGE_CAMS = {
    "member": cam([1, 1, 3], [1, 1, 0]),
    "member_far": cam([1, 1, 30], [1, 1, 0]),                # lifts md, so that the near member itself passes both tests
    "inside": cam([1, 1, 10], [1, 1, 0]),
    "outside": cam([-10, -10, 0.1], [-9, -10, 0.1]),
    "covering": cam([1, 1, 0.5], [1, 1, 0]),
    "one_edge": cam([7, 1, 10], [7, 1, 0]),
    "two_edges": cam([7, 5.5, 10], [7, 5.5, 0]),
    "four_edges": cam([1, 1, 2.0], [1, 1, 0], roll=np.pi / 4),
    "behind": cam([0.7, 1, 0.1], [5, 1.2, 0.1]),
    "behind_oblique": cam([1.2, 0.9, 0.3], [3, 2.5, 0.0]),
    "anisotropic": cam([3, 3, 4], [1, 1, 0], fx=420.0, fy=400.0, w=800.0, h=600.0),
}


def edge_case(zr=(0.0, 0.25)):
    E = np.array([c[0] for c in EDGE_CAMS.values()])
    cen = np.array([c[1] for c in EDGE_CAMS.values()])
    intr = np.array([c[2] for c in EDGE_CAMS.values()], np.float64)
    return dict(boxes=BOX, zr=np.array([zr], np.float64), E=E, cen=cen, intr=intr, members=[[0, 1]], threshold=0.25)


def golden_case(name):
    z, rs = pc.load(name), pc.restated(name)
    return dict(boxes=rs["boxes"], zr=rs["zr"], E=rs["E"], cen=rs["cen"], intr=z["intr"], members=rs["members"], threshold=z["cfg"]["threshold"])


@functools.lru_cache(maxsize=None)
def random_case():
    """Three boxes (wide, tall and thin, flat in z) seen by 96 cameras at random places looking at random targets, many of them with corners behind them;
    a camera with a corner of any box within 1e-3 of the scene's extent of its plane is redrawn."""
    r = np.random.default_rng(11)
    boxes = np.array([[0.0, 3.0, 0.0, 1.0], [4.0, 4.25, -2.0, 3.0], [-3.0, -1.0, 1.0, 2.5]])
    zr = np.array([[-0.1, 0.4], [0.0, 1.5], [0.25, 0.25]], np.float32).astype(np.float64)      # mz, Mz are float32 values, as the z-range gives them
    cams = []
    while len(cams) < 96:
        c = cam(r.uniform([-5, -4, 0.05], [7, 5, 4.0]), r.uniform([-4, -3, -0.5], [6, 4, 1.0]), fx=float(r.uniform(300, 900)), fy=float(r.uniform(300, 900)))
        zc = [rp.project(rp.corners(b, z[0], z[1]), c[0], *c[2])[1] for b, z in zip(boxes, zr)]
        if np.abs(np.array(zc)).min() >= 1e-3 * 12.0:
            cams.append(c)
    return dict(boxes=boxes, zr=zr, E=np.array([c[0] for c in cams]), cen=np.array([c[1] for c in cams]), intr=np.array([c[2] for c in cams], np.float64),
                members=[[0, 1, 2], [3, 4], [5]], threshold=0.25)


def case_of(key):
    return {"edge": edge_case, "edge_flat": lambda: edge_case((0.125, 0.125)), "random": random_case}.get(key, lambda: golden_case(key))()


def restate(case, dtype=np.float64):
    return rp.visibility(case["boxes"], case["zr"], case["E"], case["cen"], case["intr"], case["members"], case["threshold"], dtype)


@functools.lru_cache(maxsize=None)
def floors(key):
    """float64's own floor on the case `key`: the restatement in float64 against itself in np.longdouble.  -> dict(ratio abs, d rel, md rel)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is wider than float64 here"
    a, b = restate(case_of(key)), restate(case_of(key), np.longdouble)
    f = dict(ratio=float(np.abs(a["ratio"] - b["ratio"]).max()), d=float((np.abs(a["d"] - b["d"]) / b["d"]).max()), md=float((np.abs(a["md"] - b["md"]) / b["md"]).max()))
    print(f"{key}: float64 floors {f}; bars 16 x: ratio {16 * f['ratio']:.3g} (absolute), d {16 * f['d']:.3g}, md {16 * f['md']:.3g} (relative)")
    return f


def hold(key, got_ratio, got_d, got_md, want):
    f = floors(key)
    er = float(np.abs(got_ratio - want["ratio"]).max())
    ed = float((np.abs(got_d - want["d"]) / want["d"]).max())
    em = float((np.abs(got_md - want["md"]) / want["md"]).max())
    print(f"{key}: errors: ratio {er:.3g} (bar {16 * f['ratio']:.3g}), d {ed:.3g} (bar {16 * f['d']:.3g}), md {em:.3g} (bar {16 * f['md']:.3g})")
    assert er <= 16 * f["ratio"] and ed <= 16 * f["d"] and em <= 16 * f["md"]


def device_visibility(case):
    from gsrast import partition
    C = len(case["cen"])
    out = partition.visibility(t(case["boxes"]), t(case["zr"].astype(np.float32)), t(case["E"][:, :3]), t(case["cen"]), t(case["intr"]), t(host_mask(case["members"], C)),
                               case["threshold"])
    assert [x.dtype for x in out] == [torch.float64, torch.float64, torch.float64, torch.uint8]
    return [x.cpu().numpy() for x in out]


# ---------------------------------------------------------------------------------------------------------------- golden scenes end to end
@pytest.mark.parametrize("name", pc.SCENES)
def test_golden_scene_end_to_end(name):
    from gsrast import partition
    z, rs = pc.load(name), pc.restated(name)
    c = z["cfg"]
    t1 = partition.camera_position_based_region_division(z["images"], c["num_col"], c["num_row"], c["max_num_images"])
    t2 = partition.position_based_data_selection(t1, z["images"], z["points3D"], ratio=c["ratio"], device=DEV)
    assert [[i.id for i in tl["images"]] for tl in t2] == z["s2"] and [[p.id for p in tl["points3D"]] for tl in t2] == z["s2p"]
    t3, dev = partition.visibility_based_camera_selection(t2, z["images"], z["cameras"], threshod=c["threshold"], device=DEV, return_tensors=True)
    assert [[i.id for i in tl["images"]] for tl in t3] == z["s3"], "the added images in front, in dict order"
    assert np.array_equal(dev["zrange"].cpu().numpy().astype(np.float64), z["zrange"]), "mz, Mz exactly"
    t4 = partition.coverage_based_point_selection(t3, z["points3D"], device=DEV)
    assert [[p.id for p in tl["points3D"]] for tl in t4] == z["s4"] and [[i.id for i in tl["images"]] for tl in t4] == z["s3"]
    for tiles in (t2, t3, t4):
        assert np.array([tl["box"] for tl in tiles]).tobytes() == z["boxes"].tobytes()
    assert all(tl["points3D"][k] is z["points3D"][i] for tl, ids in zip(t4, z["s4"]) for k, i in enumerate(ids)), "the dict's own objects"
    want = rs["vis"]
    non = np.ones_like(want["add"])
    for k in range(len(t1)):
        non[k, rs["members"][k]] = False
    assert np.array_equal(dev["add"].cpu().numpy().astype(bool), want["add"]) and not dev["add"].cpu().numpy().astype(bool)[~non].any()
    hold(name, dev["ratio"].cpu().numpy(), dev["dist"].cpu().numpy(), dev["md"].cpu().numpy(), want)
    stats = dev["stats"].cpu().numpy()
    for k, zs in enumerate(rs["zstats"]):
        d = zs["dist"].astype(np.float64)
        assert abs(stats[k, 0] - d.mean()) <= 1e-12 * d.mean() and abs(stats[k, 1] - d.std()) <= 1e-12 * d.std()
    whole = partition.partition_scene(z["cameras"], z["images"], z["points3D"], c["num_col"], c["num_row"], c["max_num_images"], c["ratio"], c["threshold"], device=DEV)
    assert [[i.id for i in tl["images"]] for tl in whole] == z["s3"] and [[p.id for p in tl["points3D"]] for tl in whole] == z["s4"]


@pytest.mark.parametrize("name", pc.SCENES)
def test_golden_scene_on_tensors(name):
    """Steps 2 to 4 without the reference's structures: the same tiles, from six host reads."""
    from gsrast import partition
    z, rs = pc.load(name), pc.restated(name)
    c = z["cfg"]
    order = np.argsort(z["point_ids"])
    args = (t(z["boxes"]), t(rs["cen"]), t(rs["E"][:, :3]), t(z["intr"]), t(z["xyz"]), t(z["obs_offsets"]), t(z["obs_ids"]), t(z["point_ids"][order]))
    partition.partition_tensors(*args, ratio=c["ratio"], threshold=c["threshold"])
    syncs, out = count_syncs(lambda: partition.partition_tensors(*args, ratio=c["ratio"], threshold=c["threshold"]))
    assert syncs == 6
    T, C = len(z["boxes"]), len(z["image_ids"])
    member, add, inbox = bits(out["member"], T), out["add"].cpu().numpy().astype(bool), bits(out["in_box"], T)
    assert np.array_equal(bits(out["image_mask"], T), member | add)
    assert [z["image_ids"][np.concatenate([np.nonzero(add[k])[0], np.nonzero(member[k])[0]])].tolist() for k in range(T)] == z["s3"]
    assert [z["point_ids"][np.nonzero(inbox[k])[0]].tolist() for k in range(T)] == z["s2p"] and out["in_box_counts"].cpu().tolist() == [len(p) for p in z["s2p"]]
    off, rows = out["tile_offsets"].numpy(), out["rows"].cpu().numpy()
    assert [z["point_ids"][order][rows[off[k]:off[k + 1]]].tolist() for k in range(T)] == z["s4"]
    assert np.array_equal(out["zrange"].cpu().numpy().astype(np.float64), z["zrange"])


# ---------------------------------------------------------------------------------------------------------------- box membership
def boxes_around(T, r):
    """T boxes that all hold (0.5, 0.5) and none of which holds (9, 9)."""
    lo = r.uniform(-1.0, 0.4, (T, 2)); hi = r.uniform(0.6, 2.0, (T, 2))
    return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], axis=1)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65])
def test_box_membership(T):
    from gsrast import partition
    r = np.random.default_rng(T)
    bx = boxes_around(T, r)
    mx, Mx, my, My = bx[0]
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    special = np.array([[mx, 0.5], [Mx, 0.5], [0.5, my], [0.5, My], [mx, my], [Mx, My],                # on each edge and two corners of box 0: inside
                        [dn(mx), 0.5], [up(Mx), 0.5], [0.5, dn(my)], [0.5, up(My)],                      # one ulp outside box 0
                        [0.5, 0.5], [9.0, 9.0], [np.nan, 0.5]])                                           # in all tiles, in none, NaN: in none
    for N in (1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1):
        xy = r.uniform(-1.2, 2.2, (N, 2))
        n = min(N, len(special))
        xy[:n] = special[-n:] if N < len(special) else special
        for cols in (2, 3):
            pts = np.concatenate([xy, r.normal(0, 1, (N, 1))], axis=1) if cols == 3 else xy
            mask, counts = partition.point_tiles(t(pts), t(bx))
            assert mask.dtype == torch.int32 and mask.shape == (N, (T + 31) // 32) and counts.shape == (T,)
            want = rp.inside(xy, bx)
            got = bits(mask, T)
            assert np.array_equal(got, want), (N, T)
            assert np.array_equal(counts.cpu().numpy(), want.sum(axis=1)), (N, T)
            if T % 32:
                assert not (mask.cpu().numpy().view(np.uint32)[:, -1] >> np.uint32(T % 32)).any(), "no bit beyond T"
        if N >= len(special):
            assert got[0, :6].all() and not got[0, 6:10].any() and got[:, 10].all() and not got[:, 11].any() and not got[:, 12].any()
    with pytest.raises(RuntimeError, match="non-finite"):
        bad = bx.copy(); bad[T - 1, 2] = np.nan
        partition.point_tiles(t(xy), t(bad))
    empty, counts = partition.point_tiles(t(np.zeros((0, 3))), t(bx))
    assert empty.shape == (0, (T + 31) // 32) and not counts.any()


def test_box_membership_at_the_tile_limit():
    """T = 1024 is the most the LDS holds (GSR_PART_MAX_TILES); one more raises."""
    from gsrast import partition
    r = np.random.default_rng(9)
    bx = boxes_around(1024, r)
    xy = r.uniform(-1.2, 2.2, (BLOCK + 37, 2))
    mask, counts = partition.point_tiles(t(xy), t(bx))
    want = rp.inside(xy, bx)
    assert mask.shape == (BLOCK + 37, 32) and np.array_equal(bits(mask, 1024), want) and np.array_equal(counts.cpu().numpy(), want.sum(axis=1))
    with pytest.raises(RuntimeError, match="1025 tiles out of range \\[1, 1024\\]"):
        partition.point_tiles(t(xy), t(boxes_around(1025, r)))


# ---------------------------------------------------------------------------------------------------------------- tile z-range
@functools.lru_cache(maxsize=None)
def cloud(n, k=0, outlier=False):
    """n points over a thin ground slab in tile k's box, x in [2k, 2k + 1], whose neighbour distances keep a relative 1e-4 from both 3-sigma thresholds;
    with `outlier`, point 0 sits far above and must be removed.  -> (xyz, its restated z-range), computed once."""
    for seed in range(50):
        r = np.random.default_rng(1000 * k + seed)
        xyz = np.stack([2.0 * k + r.uniform(0, 1, n), r.uniform(0, 1, n), r.normal(0, 0.02, n)], axis=1)
        if outlier:
            xyz[0, 2] = 5.0
        zs = rp.z_range(xyz)
        d = zs["dist"].astype(np.float64)
        if min(np.abs(d - zs["lo"]).min() / abs(float(zs["lo"])), np.abs(d - zs["hi"]).min() / abs(float(zs["hi"]))) >= 1e-4 and zs["mask"].any():
            if not outlier or (not zs["mask"][0] and zs["Mz"] < 5.0):
                return xyz, zs
    raise AssertionError("no seed meets the margins")


def z_range_of(clouds):
    """The clouds (cloud k in tile k's box) as the tiles of one call."""
    from gsrast import partition
    xyz = np.concatenate(clouds)
    bx = np.array([[2.0 * k, 2.0 * k + 1, 0.0, 1.0] for k in range(len(clouds))])
    mask, counts = partition.point_tiles(t(xyz), t(bx))
    assert counts.cpu().tolist() == [len(c) for c in clouds]
    return partition.tile_z_range(t(xyz), mask, counts)


def test_tile_z_range_matches_the_restatement_exactly():
    """Exactly four points, gsr_dist2's 256-point box and its neighbours, several boxes, and an outlier that is the z maximum."""
    sizes = [4, KNN_BOX - 1, KNN_BOX, KNN_BOX + 1, 700]
    got = [cloud(n, k) for k, n in enumerate(sizes)] + [cloud(40, len(sizes), outlier=True)]
    zr, stats = z_range_of([c for c, _ in got])
    assert zr.dtype == torch.float32 and stats.dtype == torch.float64
    zr, stats = zr.cpu().numpy(), stats.cpu().numpy()
    for k, (_, zs) in enumerate(got):
        assert (float(zr[k, 0]), float(zr[k, 1])) == (zs["mz"], zs["Mz"]), k
        d = zs["dist"].astype(np.float64)
        assert abs(stats[k, 0] - d.mean()) <= 1e-12 * d.mean() and abs(stats[k, 1] - d.std()) <= 1e-12 * d.std()
    xyz, out = got[-1]
    assert xyz[:, 2].max() == 5.0 and out["Mz"] < 1.0 and not out["mask"][0], "the outlier is the z maximum, and is excluded"


def test_tile_z_range_errors():
    from gsrast import partition
    with pytest.raises(RuntimeError, match="fewer than four points"):
        z_range_of([cloud(40)[0], cloud(40, 1)[0][:3]])
    with pytest.raises(RuntimeError, match="fewer than four points"):
        z_range_of([cloud(40)[0][:0], cloud(40, 1)[0]])
    for bad in (np.inf, 1e39):
        c = cloud(40)[0].copy()
        c[7, 2] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            z_range_of([c])
    xyz = t(cloud(40)[0])
    mask, counts = partition.point_tiles(xyz, t(np.array([[0.0, 1.0, 0.0, 1.0]])))
    with pytest.raises(RuntimeError, match="counts does not hold the number of bits"):
        partition.tile_z_range(xyz, mask, counts - 1)


# ---------------------------------------------------------------------------------------------------------------- visibility
@pytest.mark.parametrize("zr", [(0.0, 0.25), (0.125, 0.125)])
def test_visibility_edges(zr):
    """Hull inside, outside, covering, cut by one, two and four edges, corners behind the camera, another focal pair; a flat box (mz == Mz) too."""
    case = edge_case(zr)
    want = restate(case)
    assert np.abs(want["zc"]).min() >= 1e-3 * 2.0, "no corner near a camera's plane"
    names = list(EDGE_CAMS)
    r = dict(zip(names, want["ratio"][0]))
    assert 0 < r["inside"] < 0.1 and r["outside"] == 0.0 and abs(r["covering"] - 1) < 1e-12 and 0 < r["one_edge"] < r["inside"] and 0 < r["two_edges"] < r["one_edge"]
    assert 0.5 < r["four_edges"] < 1 and (want["zc"][0, names.index("behind")] < 0).any() and (want["zc"][0, names.index("behind")] > 0).any()
    ratio, d, md, add = device_visibility(case)
    hold("edge" if zr == (0.0, 0.25) else "edge_flat", ratio, d, md, want)
    assert ratio[0, names.index("outside")] == 0.0, "entirely outside: exactly 0"
    assert np.array_equal(add.astype(bool), want["add"])
    assert not add[0, :2].any() and want["ratio"][0, 0] > case["threshold"] and want["d"][0, 0] < want["md"][0], "a member never gets add, whatever its ratio and d"


def test_visibility_random_views():
    """Random views of three boxes: the monotone chain and the clip against scipy's hull and the exact clip, wherever the cameras stand."""
    case = random_case()
    want = restate(case)
    behind = (want["zc"] < 0).any(axis=2) & (want["zc"] > 0).any(axis=2)
    assert behind.sum() >= 20 and (want["ratio"] == 0).any() and ((want["ratio"] > 0) & (want["ratio"] < 1)).sum() >= 100 and want["add"].any()
    assert np.abs(want["ratio"] - 0.25).min() >= 1e-9 and (np.abs(want["d"] - want["md"][:, None]) / want["md"][:, None]).min() >= 1e-9, "no decision at its threshold"
    ratio, d, md, add = device_visibility(case)
    hold("random", ratio, d, md, want)
    assert np.array_equal(add.astype(bool), want["add"]) and np.array_equal(ratio == 0, want["ratio"] == 0)


def test_visibility_errors_and_models():
    from gsrast import partition
    case = edge_case()
    C = len(case["cen"])
    E = case["E"].copy()
    E[4, :3] = [[0, 1, 0, -1.0], [0, 0, 1, -0.5], [1, 0, 0, 0.0]]      # camera z = world x, centre x = 0: the four corners with X = 0 have z exactly 0
    with pytest.raises(RuntimeError, match="camera-space z exactly 0"):
        partition.visibility(t(case["boxes"]), t(case["zr"].astype(np.float32)), t(E[:, :3]), t(case["cen"]), t(case["intr"]), t(host_mask([[0, 1]], C)), 0.25)
    cen = case["cen"].copy(); cen[3, 1] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        partition.visibility(t(case["boxes"]), t(case["zr"].astype(np.float32)), t(case["E"][:, :3]), t(cen), t(case["intr"]), t(host_mask([[0, 1]], C)), 0.25)
    # collinear projections (a degenerate box seen from its own plane): ratio 0, no error -- the documented deviation
    flat = dict(case, boxes=np.array([[0.0, 2.0, 1.0, 1.0]]), zr=np.array([[0.0, 0.0]]))
    ratio, d, md, add = device_visibility(dict(flat, E=case["E"][2:3], cen=case["cen"][2:3], intr=case["intr"][2:3], members=[[]]))
    assert ratio.tolist() == [[0.0]] and not add.any() and np.isnan(md[0]), "no member: md is NaN and nothing is added"
    # the reference-level function reads SIMPLE_PINHOLE and PINHOLE as get_K_matrix does, and keeps the assertion's text for anything else
    z = pc.load("quad")
    t2 = [dict(images=[z["images"][i] for i in ids], box=b, points3D=[z["points3D"][p] for p in pts]) for ids, b, pts in zip(z["s2"], z["boxes"], z["s2p"])]
    other = dict(z["cameras"])
    other[2] = type(other[2])(id=2, model="OPENCV", width=800, height=600, params=np.ones(8))
    with pytest.raises(AssertionError, match="Colmap camera model not handled: only undistorted datasets"):
        partition.visibility_based_camera_selection(t2, z["images"], other, device=DEV)
    assert {c.model for c in z["cameras"].values()} == {"SIMPLE_PINHOLE", "PINHOLE"} and set(z["camera_of"].tolist()) == {1, 2}


# ---------------------------------------------------------------------------------------------------------------- coverage
def cover_scene(M, T, seed, wide=False, C=9):
    """C images, image c in tiles {t : (c + t) % 3 == 0} (image C - 1 in none), M observations in all, ids with gaps, repeats and -1 entries."""
    r = np.random.default_rng(seed)
    n_pts = max(8, M // 3)
    id_of = (lambda i: (i % 7) * (1 << 32) + 1000 + 13 * (i // 7)) if wide else (lambda i: 5 * i + 2)
    pid = np.array(sorted(id_of(i) for i in range(n_pts)), np.int64)
    cuts = np.sort(r.integers(0, M + 1, C - 1))
    off = np.concatenate([[0], cuts, [M]]).astype(np.int64)
    ids = r.choice(pid, M)
    ids[r.random(M) < 0.1] = -1
    tiles = [[c for c in range(C - 1) if (c + k) % 3 == 0] for k in range(T)]
    return off, ids, tiles, pid


def device_coverage(off, ids, tiles, pid, C):
    from gsrast import partition
    offsets, rows = partition.coverage(t(off), t(ids), t(host_mask(tiles, C)), t(pid), len(tiles))
    assert offsets.dtype == torch.int64 and rows.dtype == torch.int64 and not offsets.is_cuda and rows.is_cuda
    offsets, rows = offsets.numpy(), rows.cpu().numpy()
    return [rows[offsets[k]:offsets[k + 1]] for k in range(len(tiles))]


@pytest.mark.parametrize("M", [1, BLOCK - 1, BLOCK, BLOCK + 1, 1023, 1024, 1025, 2049])
def test_coverage_observation_counts(M):
    off, ids, tiles, pid = cover_scene(M, 5, M)
    got = device_coverage(off, ids, tiles, pid, 9)
    want = rp.coverage(tiles, off, ids, pid)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == 5


@pytest.mark.parametrize("T", [31, 32, 33, 65])
def test_coverage_across_a_mask_word(T):
    off, ids, tiles, pid = cover_scene(700, T, T)
    got = device_coverage(off, ids, tiles, pid, 9)
    want = rp.coverage(tiles, off, ids, pid)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and any(len(a) for a in got[32:] or got)


def test_coverage_ids_beyond_32_bits():
    off, ids, tiles, pid = cover_scene(900, 4, 1, wide=True)
    assert pid.max() >= 1 << 32 and len(np.unique(pid & 0xFFFFFFFF)) < len(pid), "ids that share their low word"
    got = device_coverage(off, ids, tiles, pid, 9)
    assert all(np.array_equal(a, b) for a, b in zip(got, rp.coverage(tiles, off, ids, pid)))


def test_coverage_absent_ids_and_empty_tiles():
    off, ids, tiles, pid = cover_scene(600, 4, 2)
    C = 9
    absent = int(pid.max()) + 1
    member_slot = int(off[0])                             # image 0 is in tiles 0 and 3
    lone_slot = int(off[C - 1])                           # image C - 1 is in no tile
    assert off[1] > off[0] and off[C] > off[C - 1]
    bad = ids.copy(); bad[member_slot] = absent
    with pytest.raises(KeyError):
        rp.coverage(tiles, off, bad, pid)
    with pytest.raises(RuntimeError, match="absent from the point table"):
        device_coverage(off, bad, tiles, pid, C)
    ok = ids.copy(); ok[lone_slot] = absent               # the same id in an image of no tile: never looked up
    got = device_coverage(off, ok, tiles, pid, C)
    assert all(np.array_equal(a, b) for a, b in zip(got, rp.coverage(tiles, off, ok, pid)))
    # a tile whose images hold only -1: an empty list; and a tile without images
    only = ids.copy(); only[off[1]:off[2]] = -1
    tiles2 = [[1], [0, 2], []]
    got = device_coverage(off, only, tiles2, pid, C)
    assert len(got[0]) == 0 and len(got[2]) == 0 and np.array_equal(got[1], rp.coverage(tiles2, off, only, pid)[1]) and len(got[1])
    with pytest.raises(RuntimeError, match="point_ids does not ascend strictly"):
        device_coverage(off, ids, tiles, pid[::-1].copy(), C)
    with pytest.raises(RuntimeError, match="obs_offsets does not ascend from 0"):
        device_coverage(off + 1, ids, tiles, pid, C)


# ---------------------------------------------------------------------------------------------------------------- determinism, host reads
def test_two_calls_give_identical_bits_and_the_stated_host_reads():
    from gsrast import partition
    r = np.random.default_rng(5)
    bx = t(np.array([[0.0, 1.0, 0.0, 1.0], [0.5, 1.5, 0.0, 1.0], [2.0, 3.0, 0.0, 1.0]]))
    case = edge_case()
    C = len(case["cen"])
    vis_args = (t(case["boxes"]), t(case["zr"].astype(np.float32)), t(case["E"][:, :3]), t(case["cen"]), t(case["intr"]), t(host_mask(case["members"], C)), 0.25)
    for N in (300, 3000):
        xyz = t(np.stack([r.uniform(0, 3, N), r.uniform(0, 1, N), r.normal(0, 0.02, N)], axis=1))
        off, ids, tiles, pid = cover_scene(N, 3, N)
        cov_args = (t(off), t(ids), t(host_mask(tiles, 9)), t(pid), 3)
        mask, counts = partition.point_tiles(xyz, bx)                                        # the library is loaded, the allocator warm
        partition.tile_z_range(xyz, mask, counts); partition.visibility(*vis_args); partition.coverage(*cov_args)
        syncs, first = count_syncs(lambda: partition.point_tiles(xyz, bx))
        assert syncs == 1, "point_tiles: the status word"
        assert all(torch.equal(a, b) for a, b in zip(first, partition.point_tiles(xyz, bx)))
        syncs, first = count_syncs(lambda: partition.tile_z_range(xyz, mask, counts))
        assert syncs == 2, "tile_z_range: the counts and the status word"
        assert all(torch.equal(a, b) for a, b in zip(first, partition.tile_z_range(xyz, mask, counts)))
        syncs, first = count_syncs(lambda: partition.visibility(*vis_args))
        assert syncs == 1, "visibility: the status word"
        assert all(torch.equal(a, b, ) for a, b in zip(first, partition.visibility(*vis_args)))
        syncs, first = count_syncs(lambda: partition.coverage(*cov_args))
        assert syncs == 1, "coverage: counts and status in one read"
        assert all(torch.equal(a, b) for a, b in zip(first, partition.coverage(*cov_args)))
