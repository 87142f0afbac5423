"""GPU tests (pytest -m gpu) of gsrast.chamfer (gsr_nearest_points, gsr_sample_surface_*, gsr_voxel_downsample_*, gsr_distance_stats of the C ABI,
csrc/gsr_chamfer.hip) against the numpy restatements of tests/chamfer_truth.py on the named inputs of tests/chamfer_cases.py.  Distances, indices,
samples and kept indices are compared with np.array_equal; the statistics at rtol = 1e-12, counts exactly.  The order of the float64 additions
is the only difference from math.fsum, and a value passes through few of them: at most 10 in its thread (20 000 elements over 10 blocks of 256
threads, 8 per thread), 6 + 2 in the block's butterfly and wave sum, and as many again in the finish kernel -- about 40 roundings of 2^-53 on
non-negative terms, 5e-15 relative."""
import functools
import math

import numpy as np
import pytest
import torch

import chamfer_cases as cases
import chamfer_truth as truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nearest(q, t, m):
    from gsrast import chamfer
    d2, i = chamfer.nearest_points(q if isinstance(q, torch.Tensor) else _dev(q), t if isinstance(t, torch.Tensor) else _dev(t), m)
    assert d2.dtype == torch.float32 and i.dtype == torch.int32 and d2.shape == i.shape == (q.shape[0],)
    return d2.cpu().numpy(), i.cpu().numpy()


def _same(got, want, name):
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    print(f"{name}: {len(want[0])} queries, {int((want[1] < 0).sum())} without a target, {len(bad)} differ")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (name, bad[:8], got[0][bad[:8]], want[0][bad[:8]], got[1][bad[:8]], want[1][bad[:8]])


@pytest.mark.parametrize("name", sorted(cases.NEAREST))
def test_nearest_points(name):
    q, t, m = cases.NEAREST[name]
    _same(_nearest(q, t, m), truth.nearest(q, t, m), name)


CAPPED = ([(m, name) for name in ("lattice", "far_query", "two_clusters", "offset_1e4", "size_Q257_T257") for m in (0.05, 0.75, 3.0)] +
          [(m, name) for name in ("ring_400", "ring_1024") for m in (0.5, 0.999, 1.5)])      # the rings: short of the rim, just short of it, beyond it


@pytest.mark.parametrize("m,name", CAPPED)
def test_nearest_points_with_a_cap(name, m):
    """The cases that carry no cap of their own, under three: the cap clamps the cell size from below and ends the shells early."""
    q, t, _ = cases.NEAREST[name]
    _same(_nearest(q, t, m), truth.nearest(q, t, m), f"{name} max_dist={m}")


def _views(a):
    """The three layouts of test_gpu_knn_edges.test_input_layout: packed, a view one float into its storage, the first three columns of [P,4]."""
    P = a.shape[0]
    buf = torch.empty(3 * P + 1, device=DEV)
    view = buf[1:].view(P, 3)
    view.copy_(torch.from_numpy(a))
    wide = torch.full((P, 4), 1e30, device=DEV)
    wide[:, :3] = torch.from_numpy(a).to(DEV)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and not wide[:, :3].is_contiguous()
    return _dev(a), view, wide[:, :3]


@pytest.mark.parametrize("name", cases.LAYOUT)
def test_input_layout(name):
    q, t, m = cases.NEAREST[name]
    want = truth.nearest(q, t, m)
    for i, (qq, tt) in enumerate(zip(_views(q), _views(t))):
        _same(_nearest(qq, tt, m), want, f"{name} layout {i}")
    from gsrast import chamfer
    kept = chamfer.voxel_downsample(_views(t)[2], 0.2)[1].cpu().numpy()
    assert np.array_equal(kept, truth.voxel_downsample(t, 0.2)[1])


@functools.lru_cache(maxsize=None)
def _big_truth(name):
    q, t = cases.big(name)
    return truth.nearest(q, t)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_nearest_points_20000(name):
    """20 000 x 20 000: the all-pairs truth is computed once per cloud; the capped runs are held to it through truth.cap (test_chamfer_cpu holds
    that identity)."""
    q, t = cases.big(name)
    free = _big_truth(name)
    _same(_nearest(q, t, None), free, name)
    _same(_nearest(t, t, None), (np.zeros(len(t), np.float32), _self_index(t)), f"{name} against itself")
    for m in (0.01, 0.03):
        want = truth.cap(*free, m)
        assert (want[1] < 0).any() and (want[1] >= 0).any()
        _same(_nearest(q, t, m), want, f"{name} max_dist={m}")


def _self_index(t):
    """A cloud against itself: d2 = 0 and the lowest index among the rows equal to the query (the row itself unless it has an earlier copy)."""
    _, first, inv = np.unique(t, axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- samples
class _Mesh:
    def __init__(self, v, t):
        self.vertices, self.triangles = _dev(v), _dev(t)


@pytest.mark.parametrize("name", sorted(cases.MESHES))
def test_sample_surface(name):
    from gsrast import chamfer
    v, t, s = cases.MESHES[name]
    got = chamfer.sample_surface(_Mesh(v, t), s)
    want = truth.sample_surface(v, t, s)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    print(f"{name}: {len(want)} samples, {int((got != want).any(axis=1).sum())} differ")
    assert np.array_equal(got, want)


def test_sample_surface_of_a_triangle_mesh_and_empty():
    from gsrast import chamfer
    from gsrast.tsdf import TriangleMesh
    v, t, s = cases.MESHES["T65"]
    mesh = TriangleMesh(_dev(v), _dev(np.zeros_like(v)), _dev(t))
    assert np.array_equal(chamfer.sample_surface(mesh, s).cpu().numpy(), truth.sample_surface(v, t, s))
    empty = chamfer.sample_surface(_Mesh(v, np.zeros((0, 3), np.int32)), s)
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.float32 and empty.is_cuda


def test_sample_surface_errors():
    from gsrast import chamfer
    for (v, t, s), word in ((cases.MESH_BAD_INDEX, "index"), (cases.MESH_NEGATIVE_INDEX, "index"), (cases.MESH_ABOVE_CAP, "1024")):
        with pytest.raises(RuntimeError, match=word):
            chamfer.sample_surface(_Mesh(v, t), s)
    v, t, _ = cases.MESHES["n17"]
    with pytest.raises(RuntimeError, match="2\\^31"):                           # 4096 triangles of n = 1024: 2^32 samples, counted in 64 bits
        chamfer.sample_surface(_Mesh(v, np.tile(t, (4096, 1))), 17.0 / 1023.5)


# ---------------------------------------------------------------------------------------------------------------- thinning
@pytest.mark.parametrize("name", sorted(cases.VOXELS))
def test_voxel_downsample(name):
    from gsrast import chamfer
    pts, cell = cases.VOXELS[name]
    kept, idx = chamfer.voxel_downsample(_dev(pts), cell)
    want_pts, want_idx = truth.voxel_downsample(pts, cell)
    assert idx.dtype == torch.int32 and kept.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kept.cpu().numpy(), want_pts, equal_nan=True)


def test_voxel_downsample_empty_big_and_errors():
    from gsrast import chamfer
    kept, idx = chamfer.voxel_downsample(torch.empty((0, 3), device=DEV), 0.5)
    assert tuple(kept.shape) == (0, 3) and tuple(idx.shape) == (0,)
    pts = cases.big("clustered")[1]
    assert np.array_equal(chamfer.voxel_downsample(_dev(pts), 0.05)[1].cpu().numpy(), truth.voxel_downsample(pts, 0.05)[1])
    for bad in (cases.VOXEL_OUT_OF_RANGE, cases.VOXEL_JUST_OUT_OF_RANGE):
        with pytest.raises(RuntimeError, match="2\\^20"):
            chamfer.voxel_downsample(_dev(bad[0]), bad[1])


# ---------------------------------------------------------------------------------------------------------------- statistics
def _check_stats(got, want):
    assert set(got) == set(want)
    for k in ("n_pred", "n_gt", "thresholds"):
        assert got[k] == want[k], k
    for k in ("accuracy", "completeness", "chamfer"):
        print(f"{k}: {got[k]!r} vs {want[k]!r}")
        assert (math.isnan(got[k]) and math.isnan(want[k])) or got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k
    n = {"precision": got["n_pred"], "recall": got["n_gt"]}
    for k in ("precision", "recall"):                     # the counts behind the shares are integers: held exactly
        for a, b in zip(got[k], want[k]):
            assert (math.isnan(a) and math.isnan(b)) or round(a * n[k]) == round(b * n[k]) and a == b, k
    for a, b in zip(got["fscore"], want["fscore"]):
        assert (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("m", [None, 0.04])
def test_surface_distance_of_clouds(m):
    from gsrast import chamfer
    pred, gt = cases.NEAREST["size_Q257_T257"][:2]
    taus = (0.02, 0.05, 0.1, 0.5)
    _check_stats(chamfer.surface_distance(_dev(pred), _dev(gt), max_dist=m, thresholds=taus), truth.surface_distance(pred, gt, m, taus))
    pred, gt = cases.big("clustered")
    want = _big_stats(m, taus)
    _check_stats(chamfer.surface_distance(_dev(pred), _dev(gt), max_dist=m, thresholds=taus), want)


@functools.lru_cache(maxsize=None)
def _big_back_truth():
    q, t = cases.big("clustered")
    return truth.nearest(t, q)


def _big_stats(m, taus):
    """truth.surface_distance for the clustered 20 000-point clouds from the two shared all-pairs results (the cap applied by truth.cap)."""
    out = []
    for d2, _ in (_big_truth("clustered"), _big_back_truth()):
        if m is not None:
            d2, _ = truth.cap(d2, np.zeros(len(d2), np.int32), m)
        d = np.sqrt(d2.astype(np.float64))
        if m is not None:
            d = np.minimum(d, float(np.float32(m)))
        out.append((math.fsum(d.tolist()) / len(d), [int((d < t).sum()) / len(d) for t in taus]))
    (acc, P), (comp, R) = out
    f = [(2.0 * p * r / (p + r) if p + r > 0 else 0.0) for p, r in zip(P, R)]
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "thresholds": [float(t) for t in taus], "precision": P, "recall": R,
            "fscore": f, "n_pred": 20000, "n_gt": 20000}


def test_surface_distance_of_a_mesh_of_four_sampler_blocks():
    """T3077: the samples of a mesh of more than 1024 triangles (four blocks of the sampler's count, 33 324 samples) go through the whole chain."""
    from gsrast import chamfer
    v, t, s = cases.MESHES["T3077"]
    cloud = cases.NEAREST["size_Q257_T257"][1]
    taus = (0.05, 0.2, 0.5)
    want = truth.surface_distance(truth.sample_surface(v, t, s), cloud, None, taus)
    assert want["n_pred"] == 33324 and 0 < want["precision"][0] < want["precision"][2] < 1
    _check_stats(chamfer.surface_distance(_Mesh(v, t), _dev(cloud), spacing=s, thresholds=taus), want)


def test_mesh_against_its_own_samples():
    from gsrast import chamfer
    v, t, s = cases.MESHES["T65"]
    mesh = _Mesh(v, t)
    r = chamfer.surface_distance(mesh, chamfer.sample_surface(mesh, s), spacing=s, thresholds=(1e-30, 0.5))
    assert r["accuracy"] == 0.0 and r["completeness"] == 0.0 and r["chamfer"] == 0.0
    assert r["precision"] == [1.0, 1.0] and r["recall"] == [1.0, 1.0] and r["fscore"] == [1.0, 1.0]
    assert r["n_pred"] == r["n_gt"] == len(truth.sample_surface(v, t, s))


def test_shifted_square():
    """The unit square against itself moved by h = 1/8 along its normal: x and y of the samples agree bit for bit and z differs by exactly h, so every
    d is exactly h, and the F-score flips from 0 to 1 across tau = h (d < tau is strict)."""
    from gsrast import chamfer
    v, t, s = cases.MESHES["two_triangles"]
    h = 0.125
    up = v.copy(); up[:, 2] += np.float32(h)
    r = chamfer.surface_distance(_Mesh(v, t), _Mesh(up, t), spacing=s, thresholds=(h, float(np.nextafter(h, 1.0)), 0.1, 0.2))
    assert r["accuracy"] == h and r["completeness"] == h and r["chamfer"] == h and r["n_pred"] == r["n_gt"] == 2 * 5 * 5
    assert r["fscore"] == [0.0, 1.0, 0.0, 1.0] and r["precision"] == [0.0, 1.0, 0.0, 1.0] and r["recall"] == [0.0, 1.0, 0.0, 1.0]
    want = truth.surface_distance(truth.sample_surface(v, t, s), truth.sample_surface(up, t, s), None, (h,))
    assert want["accuracy"] == h and want["fscore"] == [0.0]
    thin = chamfer.surface_distance(_Mesh(v, t), _Mesh(up, t), spacing=s, voxel=0.25, max_dist=0.1, thresholds=(0.2,))      # every d is capped at float32(0.1)
    a, b = truth.voxel_downsample(truth.sample_surface(v, t, s), 0.25)[0], truth.voxel_downsample(truth.sample_surface(up, t, s), 0.25)[0]
    _check_stats(thin, truth.surface_distance(a, b, 0.1, (0.2,)))
    assert thin["accuracy"] == pytest.approx(float(np.float32(0.1)), rel=1e-12) and thin["n_pred"] == len(a) < 50


def test_empty_side_and_reproducibility():
    from gsrast import chamfer
    pred, gt = cases.NEAREST["size_Q257_T257"][:2]
    none = torch.empty((0, 3), device=DEV)
    r = chamfer.surface_distance(none, _dev(gt), max_dist=0.5, thresholds=(0.1,))
    _check_stats(r, truth.surface_distance(pred[:0], gt, 0.5, (0.1,)))
    assert math.isnan(r["accuracy"]) and r["completeness"] == 0.5 and math.isnan(r["chamfer"]) and r["n_pred"] == 0
    r = chamfer.surface_distance(_dev(pred), none, thresholds=(0.1,))
    assert r["accuracy"] == math.inf and math.isnan(r["completeness"]) and r["precision"] == [0.0] and r["fscore"][0] != r["fscore"][0]
    r = chamfer.surface_distance(none, none)
    assert math.isnan(r["accuracy"]) and math.isnan(r["completeness"]) and r["fscore"] == []
    q, t = cases.big("uniform")
    runs = [chamfer.surface_distance(_dev(q), _dev(t), max_dist=m, thresholds=(0.01, 0.02)) for m in (None, None, 0.015, 0.015)]
    assert runs[0] == runs[1] and runs[2] == runs[3] and runs[0] != runs[2]      # bit-equal dictionaries
