"""GPU: the first anchors on the device (gsrast.init, gsrast.anchors.octree_create_from_data_ / create_from_data_; gs-sr_amd/csrc/gsr_init.hip).
Everything is compared by exact equality: whole calls against the fixtures the reference's own create_from_data produced
(tests/golden/make_golden_create_anchors.py, whose margins keep that honest), the pieces against torch / numpy on the CPU from the same float32
inputs -- torch.quantile per camera (its order statistics, then ATen's Lerp.h operation by operation: _quantile_cpu), torch.kthvalue, torch.unique(dim=0), np.unique(axis=0) -- at the sizes where the kernels change path: around the
2048-point chunk of a workgroup, one camera past the batch of 8, more chunks than a camera batch has workgroups, around the 1024-key sort block, one
element and one level."""
import glob
import os
import types
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OCTREE = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_create_anchors_octree_*.npz")))
SCAFFOLD = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_create_anchors_scaffold_*.npz")))
DEV = "cuda:0"
MODES = ("floor", "round", "ceil")
CHUNK, BATCH, SORT_BLOCK = 2048, 8, 1024          # csrc/gsr_init.hip CQ_CHUNK, CQ_CB; csrc/gsr_common.h GSR_SORT_BLOCK
BLOCKS = 4096                                     # csrc/gsr_init.hip CQ_BLOCKS: a camera batch gets max(1, BLOCKS // batches) workgroups for its point chunks


def _inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def _scaling_line(anchor):
    from simple_knn._C import distCUDA2
    dist2 = torch.clamp_min(distCUDA2(anchor).float(), 0.0000001)
    return torch.log(torch.sqrt(dist2))[..., None].repeat(1, 6)


def count_syncs(fn):
    """Host synchronisations of fn() as torch's sync debug mode reports them (tools/bench_densify.py's way)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchroniz" in str(x.message).lower()), out


# ---------------------------------------------------------------------------------------------------------------- whole calls, golden
@pytest.mark.parametrize("name", OCTREE)
def test_octree_create_from_data_matches_the_reference(name):
    from gsrast import anchors
    z = np.load(os.path.join(GOLDEN, name))
    assert len(OCTREE) == 3
    m = types.SimpleNamespace(config=types.SimpleNamespace(sampling_ratio=1), device=DEV, dist_ratio=float(z["dist_ratio"]), levels=int(z["cfg_levels"]),
                              init_level=int(z["cfg_init_level"]), fork=int(z["fork"]), extend=float(z["extend"]), base_layer=int(z["cfg_base_layer"]),
                              visible_threshold=float(z["cfg_visible_threshold"]), dist2level=MODES[int(z["dist2level"])], n_offsets=int(z["n_offsets"]),
                              feat_dim=int(z["feat_dim"]), inverse_opacity_activation=_inverse_sigmoid)
    cameras = {float(s): [types.SimpleNamespace(camera_center=torch.tensor(c, device=DEV)) for c in z[f"centres_{i}"]] for i, s in enumerate(z["scales"])}
    pts = z["points"].copy()
    U = anchors.octree_create_from_data_(m, types.SimpleNamespace(points=pts), cameras, 2.5)
    assert np.array_equal(pts, z["points"]) and m.spatial_lr_scale == 2.5
    eq = lambda t, k: t.dtype == torch.from_numpy(z[k]).dtype and torch.equal(t.detach().cpu(), torch.from_numpy(z[k]))
    assert eq(m.cam_infos, "cam_infos") and eq(m.standard_dist, "standard_dist") and eq(m.voxel_size, "voxel_size") and eq(m.init_pos, "init_pos")
    assert m.voxel_size.dim() == 0 and m.voxel_size.is_cuda and m.standard_dist.dim() == 0
    assert (m.levels, m.init_level, m.base_layer) == (int(z["levels"]), int(z["init_level"]), int(z["base_layer"]))
    # a tenth of the generator's asserted margin between any visible fraction and the threshold: it cannot flip a keep decision
    assert abs(float(m.visible_threshold) - float(z["visible_threshold"])) <= 1e-6
    assert eq(m._anchor, "anchor") and eq(m._level, "level") and U == z["anchor"].shape[0]
    assert all(isinstance(getattr(m, n), torch.nn.Parameter) for n in ("_anchor", "_offset", "_anchor_feat", "_scaling", "_rotation", "_opacity")) and m._anchor.requires_grad
    assert torch.equal(m._scaling.detach(), _scaling_line(m._anchor.detach())) and tuple(m._scaling.shape) == (U, 6)
    assert torch.allclose(m._scaling.detach().cpu(), torch.from_numpy(z["scaling"]), rtol=0, atol=2e-6)          # the device's log against the host's
    assert tuple(m._offset.shape) == (U, m.n_offsets, 3) and not m._offset.any() and tuple(m._anchor_feat.shape) == (U, m.feat_dim) and not m._anchor_feat.any()
    assert torch.equal(m._rotation.detach().cpu(), torch.tensor([1.0, 0, 0, 0]).repeat(U, 1))
    assert torch.equal(m._opacity.detach(), _inverse_sigmoid(0.1 * torch.ones((U, 1), device=DEV)))
    assert m._extra_level.dtype == torch.float32 and tuple(m._extra_level.shape) == (U,) and not m._extra_level.any()
    assert m._anchor_mask.dtype == torch.bool and bool(m._anchor_mask.all()) and m._level.dtype == torch.int32


@pytest.mark.parametrize("name", SCAFFOLD)
def test_scaffold_create_from_data_matches_the_reference(name):
    from gsrast import anchors
    z = np.load(os.path.join(GOLDEN, name))
    assert len(SCAFFOLD) == 4
    m = types.SimpleNamespace(config=types.SimpleNamespace(sampling_ratio=1), device=DEV, voxel_size=float(z["cfg_voxel_size"]), n_offsets=int(z["n_offsets"]),
                              feat_dim=int(z["feat_dim"]), inverse_opacity_activation=_inverse_sigmoid)
    pts = z["points"].copy()
    U = anchors.create_from_data_(m, types.SimpleNamespace(points=pts), {}, 1.0)
    assert np.array_equal(pts, z["points"]), "the caller's array is left as it was (the reference shuffles it)"
    assert m.voxel_size == float(z["voxel_size"])
    assert m._anchor.dtype == torch.float32 and torch.equal(m._anchor.detach().cpu(), torch.from_numpy(z["anchor"])) and U == z["anchor"].shape[0]
    assert torch.equal(m._scaling.detach(), _scaling_line(m._anchor.detach()))
    assert tuple(m.max_radii2D.shape) == (U,) and tuple(m._offset.shape) == (U, m.n_offsets, 3)


# ---------------------------------------------------------------------------------------------------------------- per-camera quantiles
def _quantile_cpu(x, q):
    """torch.quantile(x, q) on the CPU with the interpolation spelt out.  The two order statistics are torch.quantile's own ('lower' / 'higher': its
    float32 rank rule decides which elements they are, and a selection has no rounding); between them ATen's Lerp.h, w < 0.5 ? a + w * (b - a) :
    b - (b - a) * (1 - w), in numpy float32 scalars, every operation rounded on its own.  torch.quantile's 'linear' mode itself is not a fixed
    reference: ATen's AVX2 / AVX512 lerp kernels fuse the product-sum, its DEFAULT level does not, and the two differ in the last bit now and then."""
    f = np.float32
    a, b = f(torch.quantile(x, q, interpolation="lower").item()), f(torch.quantile(x, q, interpolation="higher").item())
    rank = f(f(q) * f(x.numel() - 1))
    w = f(rank - np.floor(rank))
    d = f(b - a)
    plain = f(a + f(w * d)) if w < 0.5 else f(b - f(d * f(f(1) - w)))
    lin = float(torch.quantile(x, q))
    assert abs(lin - float(plain)) <= abs(float(plain)) * 1.2e-7, (lin, float(plain))          # the linear mode: the same up to its fused last bit
    return torch.tensor(plain)


def _quantiles_cpu(points, cams, r):
    """The reference's set_level loop on the CPU: per camera the distance of every point as include/gsrast.h states it, sqrt(((dx*dx + dy*dy) + dz*dz))
    in float32 with every operation rounded on its own, then torch.quantile twice and the camera's scale.  The distance is formed in numpy: torch.sqrt
    on the CPU is not correctly rounded in its vectorised path (592 of 100 000 random values come out one ulp off float32(sqrt(float64(x))), numpy's
    none), which elements it hits depends on the host, and the device's root is the correctly rounded one."""
    out = []
    p = points.numpy()
    for cam in cams.numpy():
        d = p - cam[None, :3]
        dist = torch.from_numpy(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
        assert dist.dtype == torch.float32
        dist_max, dist_min = _quantile_cpu(dist, r), _quantile_cpu(dist, 1 - r)
        out.append(np.array([dist_min.item(), dist_max.item()], np.float32) * cam[3])
    return torch.from_numpy(np.concatenate(out))


def _cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) * 4.0 - 1.5).float()


def _cams(c, seed, scales=(1.0,)):
    g = torch.Generator().manual_seed(1000 + seed)
    cam = torch.randn(c, 4, generator=g).float() * 2.0
    cam[:, 3] = torch.tensor([scales[i % len(scales)] for i in range(c)])
    return cam


def _equidistant(n):
    signs = torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
    return (signs * torch.tensor([0.3, 1.7, 0.9])).repeat((n + 7) // 8, 1)[:n].contiguous()


def _clusters(n):
    p = _cloud(n, 77) * 0.001
    p[n // 2:] += 100.0
    return p


QUANTILE_CASES = {
    "n1": (lambda: _cloud(1, 1), lambda: _cams(1, 1), 0.999),
    "n2_half": (lambda: _cloud(2, 2), lambda: _cams(2, 2), 0.5),
    "n3": (lambda: _cloud(3, 3), lambda: _cams(3, 3), 0.999),
    "n4099": (lambda: _cloud(4099, 4), lambda: _cams(BATCH + 1, 4), 0.999),
    "n100003": (lambda: _cloud(100003, 5), lambda: _cams(3, 5), 0.999),
    "chunk_minus_1": (lambda: _cloud(CHUNK - 1, 6), lambda: _cams(2, 6), 0.999),
    "chunk": (lambda: _cloud(CHUNK, 7), lambda: _cams(2, 7), 0.999),
    "chunk_plus_1": (lambda: _cloud(CHUNK + 1, 8), lambda: _cams(2, 8), 0.999),
    "two_chunks": (lambda: _cloud(2 * CHUNK, 9), lambda: _cams(2, 9), 0.999),
    "two_chunks_plus_1": (lambda: _cloud(2 * CHUNK + 1, 10), lambda: _cams(1, 10), 0.5),
    "one_camera": (lambda: _cloud(777, 11), lambda: _cams(1, 11), 0.999),
    "batch_plus_1_scaled": (lambda: _cloud(3001, 12), lambda: _cams(BATCH + 1, 12, (1.0, 2.0, 0.5, 4.0)), 0.999),
    "equidistant": (lambda: _equidistant(300), lambda: torch.tensor([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 2.0]]), 0.999),
    "two_clusters": (lambda: _clusters(5000), lambda: torch.tensor([[0.0, 0.0, 0.0, 1.0], [100.0, 100.0, 100.0, 3.0], [50.0, 50.0, 50.0, 1.0]]), 0.999),
    "ratio_one": (lambda: _cloud(2500, 13), lambda: _cams(3, 13), 1.0),
    "ratio_half": (lambda: _cloud(2500, 14), lambda: _cams(3, 14, (2.0,)), 0.5),
    # 512 camera batches (the last of 2 cameras) leave 4096 // 512 = 8 workgroups to a batch's 10 point chunks (the last of 5 points): workgroups 0 and 1
    # take a second chunk into the same LDS histograms (test_create_anchors_cpu holds the three inequalities)
    "past_the_block_cap": (lambda: _cloud(PAST_CAP[1], 15), lambda: _cams(PAST_CAP[0], 15, (1.0, 2.0, 0.5, 4.0)), 0.999),
}
PAST_CAP = (4090, 9 * CHUNK + 5)                  # cameras, points


def _quantiles_cpu_in_parallel(points, cams, r, block=50, workers=8):
    """_quantiles_cpu itself over blocks of cameras, on a few threads: a camera's two numbers depend on no other camera."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as ex:
        return torch.cat(list(ex.map(lambda i: _quantiles_cpu(points, cams[i:i + block], r), range(0, cams.shape[0], block))))


@pytest.mark.parametrize("case", sorted(QUANTILE_CASES))
def test_camera_dist_quantiles_equal_torch_quantile(case):
    from gsrast import init
    make_p, make_c, r = QUANTILE_CASES[case]
    p, c = make_p(), make_c()
    want = _quantiles_cpu(p, c, r) if c.shape[0] <= 64 else _quantiles_cpu_in_parallel(p, c, r)
    got = init.camera_dist_quantiles(p.to(DEV), c.to(DEV), r)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * c.shape[0],)
    assert torch.equal(got.cpu(), want), (case, (got.cpu() - want).abs().max())
    if case == "equidistant":
        assert want[0] == want[1] and want[2] == want[0] * 2
    if case == "two_clusters":
        assert want[1] > 1000 * want[0]                                                  # the two targets part in the first pass


def test_camera_dist_quantiles_reports_a_non_finite_point():
    from gsrast import init
    p = _cloud(100, 1)
    p[17, 1] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        init.camera_dist_quantiles(p.to(DEV), _cams(2, 1).to(DEV), 0.999)


# ---------------------------------------------------------------------------------------------------------------- order statistics of an array
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 5000, 300001])
def test_quantile_and_kthvalue_equal_torch(n):
    """300001 elements: more than the 1024 workgroups of 256 threads take in one turn."""
    from gsrast import init
    g = torch.Generator().manual_seed(n)
    x = (torch.randint(-40, 60, (n,), generator=g).float() / 7.0)                       # duplicates, both signs
    if n > 2:
        x[1], x[2] = 0.0, -0.0
    xd = x.to(DEV)
    for q in (0.999, 1 - 0.999, 0.5, 0.0, 1.0, 0.3):
        got = init.quantile(xd, q)
        assert got.dim() == 0 and got.cpu() == _quantile_cpu(x, q), (n, q)
    pair = init.quantile(xd, (0.999, 1 - 0.999))
    assert torch.equal(pair.cpu(), torch.stack([_quantile_cpu(x, 0.999), _quantile_cpu(x, 1 - 0.999)]))
    for k in sorted({1, max(1, int(n * 0.5)), n}):
        assert init.kthvalue(xd, k).cpu() == torch.kthvalue(x, k).values, (n, k)
    assert torch.equal(xd.cpu(), x)
    with pytest.raises(RuntimeError, match="out of range"):
        init.kthvalue(xd, n + 1)


def test_quantile_reports_nan():
    from gsrast import init
    x = torch.arange(600.0)
    x[300] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        init.quantile(x.to(DEV), 0.5)


# ---------------------------------------------------------------------------------------------------------------- unique voxel rows
def _octree_sample_cpu(data, init_pos, voxel_size, fork, levels):
    """The reference's octree_sample on the CPU."""
    pos, lvl = [], []
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    for cur_level in range(levels):
        cur_size = vs / (float(fork) ** cur_level)
        new_positions = torch.unique(torch.round((data - init_pos) / cur_size), dim=0) * cur_size + init_pos
        pos.append(new_positions); lvl.append(torch.ones(new_positions.shape[0], dtype=torch.int) * cur_level)
    return torch.cat(pos), torch.cat(lvl)


def _axis_line(axis, n=50):
    p = torch.zeros(n, 3)
    p[:, axis] = torch.arange(n).float() * 0.37 - 5.0
    return p[torch.randperm(n, generator=torch.Generator().manual_seed(axis))]


def _half_ties():
    k = torch.arange(-6, 7).float()
    g = torch.stack(torch.meshgrid(k, k[:3], k[:2], indexing="ij"), -1).reshape(-1, 3)
    return (g + 0.5) * 0.5                                                                # (p - 0) / 0.5 = k + 0.5 exactly: half to even decides


SAMPLE_CASES = {
    "n1": (lambda: torch.tensor([[0.3, -0.2, 0.9]]), (0.0, 0.0, 0.0), 0.25, 2, 3),
    "one_cell": (lambda: torch.rand(300, 3, generator=torch.Generator().manual_seed(1)) * 0.01 + 0.5, (0.0, 0.0, 0.0), 4.0, 2, 1),
    "all_distinct": (lambda: _cloud(700, 21), (-2.0, -2.0, -2.0), 0.001, 2, 1),
    "half_ties": (_half_ties, (0.0, 0.0, 0.0), 0.5, 2, 1),
    "negative_keys": (lambda: _cloud(900, 22) + 3.0, (6.6, 6.6, 6.6), 0.3, 2, 4),
    "only_z": (lambda: _axis_line(2), (0.0, 0.0, 0.0), 0.5, 2, 2),
    "only_y": (lambda: _axis_line(1), (0.0, 0.0, 0.0), 0.5, 2, 2),
    "only_x": (lambda: _axis_line(0), (0.0, 0.0, 0.0), 0.5, 2, 2),
    "beyond_2_21": (lambda: torch.cat([_cloud(100, 23), torch.tensor([[3000000.0, 1.0, -2.0], [-2500000.0, 0.0, 3.0]])]), (0.0, 0.0, 0.0), 1.0, 2, 2),
    "levels_12": (lambda: _cloud(600, 24), (-1.65, -1.65, -1.65), 1.0, 2, 12),
    "fork_3": (lambda: _cloud(600, 25), (-1.65, -1.65, -1.65), 0.7, 3, 4),
    "sort_block_minus_1": (lambda: _cloud(SORT_BLOCK - 1, 26), (-1.65, -1.65, -1.65), 0.2, 2, 2),
    "sort_block": (lambda: _cloud(SORT_BLOCK, 27), (-1.65, -1.65, -1.65), 0.2, 2, 2),
    "sort_block_plus_1": (lambda: _cloud(SORT_BLOCK + 1, 28), (-1.65, -1.65, -1.65), 0.2, 2, 2),
    "four_sort_blocks_plus_1": (lambda: _cloud(4 * SORT_BLOCK + 1, 29), (-1.65, -1.65, -1.65), 0.05, 2, 3),
}


@pytest.mark.parametrize("case", sorted(SAMPLE_CASES))
def test_octree_sample_equals_torch_unique(case):
    from gsrast import init
    make, init_pos, voxel_size, fork, levels = SAMPLE_CASES[case]
    data = make().float().contiguous()
    want_p, want_l = _octree_sample_cpu(data, torch.tensor(init_pos), voxel_size, fork, levels)
    dev = data.to(DEV)
    syncs, (pos, lvl) = count_syncs(lambda: init.octree_sample(dev, init_pos, voxel_size, fork, levels))
    assert syncs == 1, "one host read, whatever the number of levels"
    assert pos.dtype == torch.float32 and lvl.dtype == torch.int32
    assert torch.equal(lvl.cpu(), want_l) and torch.equal(pos.cpu(), want_p), case
    assert torch.equal(dev.cpu(), data), "the caller's tensor is unchanged"
    zero = pos.cpu()[pos.cpu() == 0]
    assert not torch.signbit(zero).any(), "a zero coordinate is +0.0"
    if case == "half_ties":
        assert want_p.shape[0] < data.shape[0]                                           # k + 0.5 and k + 1.5 meet at the even neighbour


def test_octree_sample_raises_on_overflow_and_nan():
    from gsrast import init
    p = _cloud(300, 5)
    big = p.clone(); big[7, 2] = 3.0e9
    with pytest.raises(RuntimeError, match="int32"):
        init.octree_sample(big.to(DEV), (0.0, 0.0, 0.0), 1.0, 2, 2)
    nan = p.clone(); nan[250, 0] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        init.octree_sample(nan.to(DEV), (0.0, 0.0, 0.0), 1.0, 2, 2)
    with pytest.raises(RuntimeError, match="non-finite"):
        init.voxelize_sample(nan.double().numpy(), 0.1, DEV)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,voxel_size", [(1, 0.1), (SORT_BLOCK + 1, 0.07), (3000, 0.013)])
def test_voxelize_sample_equals_numpy_unique(dtype, n, voxel_size):
    from gsrast import init
    data = (_cloud(n, n).numpy().astype(np.float64) * 1.000001).astype(dtype)
    if n > 8:
        data[-4:] = data[:4]
        data[4] = np.array([0.5, 1.5, -2.5], dtype) * dtype(voxel_size)                   # on or next to half-cell ties in this precision
    keep = data.copy()
    want = (np.unique(np.round(data / voxel_size), axis=0) * voxel_size).astype(np.float32)
    got = init.voxelize_sample(data, voxel_size, DEV)
    assert np.array_equal(data, keep), "the caller's array is unchanged"
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- set_level
@pytest.mark.parametrize("cams_per_scale,fork", [((1,), 2), ((5, 4), 2), ((20, 3), 3)])
def test_set_level_matches_the_reference_and_reads_once(cams_per_scale, fork):
    from gsrast import init
    p = _cloud(3000, 40 + len(cams_per_scale))
    r = 0.999
    centres = {float(2 ** i): (torch.randn(n, 3, generator=torch.Generator().manual_seed(i + n)) * 3.0 + 4.0).float() for i, n in enumerate(cams_per_scale)}
    cam_infos = torch.cat([torch.cat([c, torch.full((c.shape[0], 1), s)], 1) for s, c in centres.items()])
    all_dist = _quantiles_cpu(p, cam_infos, r)
    dist_max, dist_min = _quantile_cpu(all_dist, r), _quantile_cpu(all_dist, 1 - r)
    x = float(torch.log2(dist_max / dist_min) / np.log2(fork))
    assert abs(abs(x - np.floor(x)) - 0.5) > 1e-3                                        # the level count is not rounded from a knife edge
    levels = int(torch.round(torch.log2(dist_max / dist_min) / np.log2(fork)).int().item()) + 1
    dev_p = p.to(DEV)
    cameras = {s: [types.SimpleNamespace(camera_center=row.to(DEV)) for row in c] for s, c in centres.items()}
    syncs, (ci, sd, lv, il) = count_syncs(lambda: init.set_level(dev_p, cameras, r, fork))
    assert syncs == 1, "one host read, whatever the number of cameras"
    assert torch.equal(ci.cpu(), cam_infos) and sd.dim() == 0 and sd.cpu() == dist_max and (lv, il) == (levels, int(levels / 2))
    ci2, sd2, lv2, il2 = init.set_level(dev_p, {s: c.to(DEV) for s, c in centres.items()}, r, fork, levels=7, init_level=2)
    assert torch.equal(ci2, ci) and sd2 == sd and (lv2, il2) == (7, 2)
