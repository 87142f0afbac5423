"""CPU: the neighbour-view selection away from the device (gsrast.views; gs-sr_amd/csrc/gsr_views.hip).  The numpy restatement the GPU tests use as
their truth (tests/ref_view_selection.py) is held to the fixtures the reference itself produced (tests/golden/make_golden_view_selection.py), exactly;
write_pairs / read_pairs are held to the reference's pair.txt bytes and to its half list; and every argument error is raised before a device is
touched."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest
import torch

import ref_view_selection as rvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_view_selection_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    theta0, sigma1, sigma2, nv = z["params"].tolist()
    return z, (theta0, sigma1, sigma2, int(nv))


def fixture_view_sel(z):
    return [list(zip(a.tolist(), b.tolist())) for a, b in zip(z["sel_ids"], z["sel_scores"])]


def test_the_three_scenes_are_there():
    assert SCENES == ["ref_view_selection_c12.npz", "ref_view_selection_c4.npz", "ref_view_selection_c70.npz"]
    for name in SCENES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 275183          # no larger than the largest fixture there was


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_the_reference_exactly(name):
    z, (theta0, sigma1, sigma2, nv) = load(name)
    score, angles = rvs.scores(z["centers"], z["obs_offsets"], z["obs_ids"], z["point_ids"], z["point_xyz"], theta0, sigma1, sigma2, with_angles=True)
    assert np.array_equal(score, z["scores"]), "the score matrix, bit for bit"
    ids, val = rvs.rank(score, nv)
    assert np.array_equal(ids, z["sel_ids"]) and np.array_equal(val, z["sel_scores"])
    assert rvs.view_selection(z["centers"], z["obs_offsets"], z["obs_ids"], z["point_ids"], z["point_xyz"], theta0, sigma1, sigma2, nv) == fixture_view_sel(z)
    # the margins the generator asserted still hold for what is in the file
    assert 0.1 <= min(angles) and max(angles) <= 179.9 and rvs.top_gap(score, nv) >= 1e-6


@pytest.mark.parametrize("name", SCENES)
def test_scenes_hold_what_they_are_meant_to(name):
    z, (_, _, _, nv) = load(name)
    Cn = len(z["centers"])
    imgs = rvs.images(z["obs_offsets"], z["obs_ids"])
    assert any((a == -1).all() for a in imgs), "an image without a valid observation"
    assert any((a == -1).any() and (a != -1).any() for a in imgs), "-1 entries"
    assert any(len(np.unique(a[a != -1])) < (a != -1).sum() for a in imgs), "ids repeated within an image"
    assert (np.diff(z["point_ids"]) > 1).any(), "ids with gaps"
    assert z["sel_ids"].shape == (Cn, min(nv, Cn))
    if Cn <= nv:
        assert all(a in row for a, row in enumerate(z["sel_ids"].tolist())), "the own index is selected"
    if Cn == 70:
        valid = np.concatenate([np.unique(a[a != -1]) for a in imgs])
        assert np.unique(valid, return_counts=True)[1].max() > 64, "tracks longer than a wavefront"


@pytest.mark.parametrize("name", SCENES)
def test_write_pairs_and_read_pairs_match_the_reference(name, tmp_path):
    from gsrast import views
    z, _ = load(name)
    path = str(tmp_path / "pair.txt")
    views.write_pairs(path, fixture_view_sel(z))
    assert open(path, "rb").read() == z["pair_txt"].tobytes(), "pair.txt, byte for byte"
    half = views.read_pairs(path)
    k = z["sel_ids"].shape[1]
    assert all(len(row) == (k + 1) // 2 for row in half), "the reference's half list: the first ceil(n / 2) pairs"
    assert [[a for a, _ in row] for row in half] == z["read_ids"].tolist()
    assert [[s for _, s in row] for row in half] == z["read_scores"].tolist()
    assert all(isinstance(a, int) and isinstance(s, float) for row in half for a, s in row)
    assert [[a for a, _ in row] for row in half] == z["sel_ids"][:, :(k + 1) // 2].tolist()


def test_assign_near_ids():
    from gsrast import views
    view_sel = [[(2, 3.5), (1, 0.25)], [(0, 1.0), (2, 0.5)], [(0, 3.5), (1, 0.5)]]
    data = {1.0: [types.SimpleNamespace() for _ in range(3)], 0.5: [types.SimpleNamespace() for _ in range(3)]}
    views.assign_near_ids(data, view_sel)
    for cams in data.values():
        assert [c.near_ids for c in cams] == [[2, 1], [0, 2], [0, 1]]


def test_flatten_and_point_table():
    from gsrast import views
    off, ids = views.flatten_observations([np.array([5, -1, 5]), np.array([], np.int64), [7]])
    assert off.tolist() == [0, 3, 3, 4] and ids.tolist() == [5, -1, 5, 7] and off.dtype == ids.dtype == np.int64
    pid, xyz = views.point_table({9: types.SimpleNamespace(xyz=np.array([1.0, 2.0, 3.0])), 4: types.SimpleNamespace(xyz=[4.0, 5.0, 6.0])})
    assert pid.tolist() == [4, 9] and xyz.tolist() == [[4.0, 5.0, 6.0], [1.0, 2.0, 3.0]] and xyz.dtype == np.float64


def test_select_views_argument_errors_without_a_device():
    from gsrast import views
    cen, off, ids, pid, xyz = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), \
        torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="centers must be a CUDA tensor"):
        views.select_views(cen, off, ids, pid, xyz)
    with pytest.raises(RuntimeError, match="centers must be a tensor"):
        views.select_views(cen.numpy(), off, ids, pid, xyz)
    with pytest.raises(RuntimeError, match="num_views must be a positive integer"):
        views.select_views(cen, off, ids, pid, xyz, num_views=0)
    with pytest.raises(RuntimeError, match="sigma1, sigma2 positive"):
        views.select_views(cen, off, ids, pid, xyz, sigma2=0)
    with pytest.raises(RuntimeError, match="theta0 must be finite"):
        views.select_views(cen, off, ids, pid, xyz, theta0=float("nan"))
    with pytest.raises(RuntimeError, match="2 centres but 1 id arrays"):
        views.view_selection([np.zeros(3), np.ones(3)], [np.zeros(2, np.int64)], {})
    assert views.view_selection([], [], {}) == []
    assert "absent from the point table" in views.status_message(views.ERR_ABSENT) and "non-finite" in views.status_message(views.ERR_NONFINITE)


def test_view_select_entry_point_rejects_bad_arguments_without_a_device():
    """gsr_view_select validates before it launches anything: the messages are checkable without a device."""
    import gsrast
    from gsrast import views
    L = gsrast.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    big = 1 << 24

    def call(Cn=2, M=4, Np=3, theta0=5.0, s1=1.0, s2=10.0, k=2, bits=64, cen=a, scratch=a, nbytes=big, status=a):
        return L.gsr_view_select(cen, Cn, a, a, M, a, a, Np, theta0, s1, s2, k, bits, a, a, None, scratch, nbytes, status, None)
    assert views.MAX_IMAGES == 16384
    assert call(Cn=views.MAX_IMAGES + 1) != 0 and "16384" in gsrast.last_error() and "LDS" in gsrast.last_error()
    assert call(Cn=0) != 0 and "images out of range" in gsrast.last_error()
    assert call(M=1 << 31) != 0 and "observations out of range" in gsrast.last_error()
    assert call(Np=-1) != 0 and "points out of range" in gsrast.last_error()
    assert call(k=3) != 0 and "views out of range" in gsrast.last_error()
    assert call(k=0) != 0 and "views out of range" in gsrast.last_error()
    assert call(bits=48) != 0 and "id_bits" in gsrast.last_error()
    assert call(s1=0.0) != 0 and "sigma1" in gsrast.last_error()
    assert call(theta0=float("inf")) != 0 and "theta0" in gsrast.last_error()
    assert call(cen=None) != 0 and "null pointer" in gsrast.last_error()
    assert call(status=None) != 0 and "null pointer" in gsrast.last_error()
    assert call(nbytes=16) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_view_select_scratch_bytes(4, views.MAX_IMAGES + 1) == 0 and L.gsr_view_select_scratch_bytes(-1, 4) == 0
    n1, n2 = L.gsr_view_select_scratch_bytes(1 << 20, 300), L.gsr_view_select_scratch_bytes(1 << 21, 300)
    assert 0 < n1 < 80 << 20 and 1.8 < n2 / n1 < 2.2, "O(M) scratch, no C x C array"
    assert L.gsr_view_select_scratch_bytes(0, 1) > 0
