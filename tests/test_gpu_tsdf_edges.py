"""GPU tests (pytest -m gpu) of csrc/gsr_tsdf_sparse.hip at its edges, against the float64 truth of tests/tsdf_truth.py (not against the float32
restatement): both branches of the two touch kernels and the wave-uniform switch between them, both texel formats of the voxel pass, sample rows that wrap
inside a wave, fewer samples than a wave, depth pixels and colours the kernels must skip or clamp, voxels behind the camera, refusal / growth / rerun,
probe sequences over the end of the hash table (insert, find, rehash), coordinates at the ends of the key range, and the merge arithmetic.
On ROBUST voxels (tsdf_truth: away from every decision a float32 rounding can flip) weights are EQUAL without a forgiven fraction, |tsdf - truth| <= 1e-4
and colours within 0.05; unit sets are equal; what was never updated reads 0.  test_tsdf_truth_cpu.py holds what these cases rest on.

Worst figures on an MI355X over the robust voxels of each case (weight mismatches: 0 everywhere): see DESIGN.md, "Sparse TSDF volume against a float64 truth"."""
import numpy as np
import pytest
import torch

import ref_mesh_numpy as ref
import tsdf_cases
import tsdf_truth

pytestmark = pytest.mark.gpu

VL = float(np.float32(0.02))
TR = float(np.float32(5 * VL))


def _poison(vol):
    """As test_gpu_tsdf._poison: NaN records and all-ones written-group words, so that a kernel trusting either shows it."""
    for ch in vol.chunks:
        ch.fill_(float("nan"))
    vol.mask.fill_(-1)
    return vol


def _volume(vl=VL, tr=TR, cap=64, **kw):
    from gsrast.tsdf import ScalableTSDFVolume
    return _poison(ScalableTSDFVolume(vl, tr, capacity_units=cap, **kw))


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _integrated(case, cap=4096, defer=False):
    frs, vl, tr, stride, dt, quant, tv = tsdf_cases.small_truth(case)
    vol = _volume(vl, tr, cap, depth_sampling_stride=stride)
    for f in frs:
        vol.integrate(*_dev(f["rgb"], f["depth"]), f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=dt, quantize_rgb8=quant == 2, defer=defer)
    return vol, tv


def _mesh_arrays(mesh):
    m = mesh.cpu()
    return m.vertices.numpy(), m.vertex_colors.numpy(), m.triangles.numpy()


def _mesh_equals(mesh, want, what):
    """The bars of test_gpu_mesh._check: triangles equal, positions within 2 float32 ulps, colours within 4 * 2^-24."""
    v, c, t = _mesh_arrays(mesh)
    rv, rc, rt = want
    assert v.shape == rv.shape and t.shape == rt.shape, (what, v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(t, rt), what
    if len(v):
        assert (np.abs(v.astype(np.float64) - rv.astype(np.float64)) <= 2.0 * np.spacing(np.abs(rv)).astype(np.float64)).all(), what
        assert (np.abs(c.astype(np.float64) - rc.astype(np.float64)) <= 4 * 2.0 ** -24).all(), what


def _check(vol, tv, what):
    """The device volume against the truth, and the mesh module on the pools as these paths left them (unmaterialised) against the numpy restatement of
    the mesh over the device's own voxels and against a volume rebuilt from them through merge_units_."""
    mesh = vol.extract_triangle_mesh()
    got = tuple(x.cpu().numpy() for x in vol.units())
    assert not any(np.isnan(a).any() for a in got[1:])
    nw, et, ec, nrob, share = tsdf_truth.robust_errors(got, tv)
    print(f"{what}: {len(got[0])} units, {nrob} robust updated voxels, fragile share {100 * share:.2f} %, weight mismatches {nw}, "
          f"tsdf error {et:.2e}, colour error {ec:.2e}, mesh {tuple(mesh.vertices.shape)[0]} vertices {tuple(mesh.triangles.shape)[0]} triangles")
    assert nw == 0, (what, nw)
    assert et <= tsdf_truth.TSDF_BAR and ec <= tsdf_truth.COLOUR_BAR, (what, et, ec)
    assert vol.last_touched == len(tv.touched[-1][0])                      # the last frame listed exactly the units its samples name, each once
    assert int(mesh.triangles.shape[0]) > 100
    rebuilt = _volume(vol.voxel_length, vol.sdf_trunc, cap=1024)
    rebuilt.merge_units_(*vol.units(), assume_unique=True)
    again = rebuilt.extract_triangle_mesh()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_mesh_arrays(mesh), _mesh_arrays(again))), what
    co = got[0].astype(np.int64)
    if np.prod(co.max(0) - co.min(0) + 1) <= 600:                          # (the far block of depth_trunc=inf makes the bounding box 8 units deep)
        T, W, Cc, org = ref.dense_from_units(*got)
        _mesh_equals(mesh, ref.extract(T, W, Cc, vol.voxel_length, origin=org), what)


@pytest.mark.parametrize("case", ["t5", "t9", "t12", "t24", "s1", "s3", "s4", "w5x3", "w7x5", "t5_f32", "near", "t5_inf"])
def test_device_equals_the_float64_truth(case):
    """t5: leaders only; t9: a workgroup with both kinds of wave; t12, t24: the plain loops of both touch kernels (fresh units in frame 1, listed again in
    frames 2 and 3); s1 / s3 / s4: 47 x 35 at strides 1, 3, 4; w5x3: 2 samples; w7x5: 35 samples; t5_f32: 16-byte texels (quantize_rgb8=False), tsdf and
    weights held as well; near: the surface closer than one unit, voxels behind the camera and outside the image; t5_inf: depth_trunc=inf."""
    vol, tv = _integrated(case)
    _check(vol, tv, case)


def test_every_frame_through_refusal_growth_and_rerun():
    vol, tv = _integrated("t5", cap=16)
    assert vol.cap > 16 and len(vol.chunks) > 1
    _check(vol, tv, "t5 from 16 units")


def test_deferred_frames_through_the_wide_branch():
    vol, tv = _integrated("t24", defer=True)
    assert vol._pending is not None
    _check(vol, tv, "t24 deferred")
    assert vol._pending is None


# ---------------------------------------------------------------------------------------------------------------- keys and probing
def _random_units(coords, seed):
    rng = np.random.default_rng(seed)
    n = len(coords)
    t = rng.uniform(-1, 1, (n, 16, 16, 16)).astype(np.float32)
    w = rng.integers(1, 5, (n, 16, 16, 16)).astype(np.float32)
    c = rng.uniform(0, 255, (n, 16, 16, 16, 3)).astype(np.float32)
    return np.asarray(coords, np.int32), t, w, c


def _by_coord(vol):
    co, t, w, c = (x.cpu().numpy() for x in vol.units())
    keys = [tuple(k) for k in co.tolist()]
    assert len(set(keys)) == len(keys)
    return {k: (t[i], w[i], c[i]) for i, k in enumerate(keys)}


def _occupied(vol):
    """{table position: key} of the volume's hash table."""
    keys = vol.keys.cpu().numpy()
    return {int(p): int(keys[p]) for p in np.nonzero(keys != -1)[0]}


def _expected_table(coords, log2):
    return {p for _, p in tsdf_truth.probe_positions(coords, log2)}, {tsdf_truth.ts_pack(*(int(v) for v in c)) for c in coords}


def test_probe_sequences_over_the_end_of_the_table():
    """16 units / 32 entries: twelve units whose cluster runs over the end of the table (ts_insert), merged a second time (ts_find across the wrap), then
    eight more: growth to 64 entries, where re-keying (k_ts_rehash) wraps as well."""
    first, more = tsdf_cases.probe_wrap_lists()
    a = _random_units(first, 1)
    vol = _volume(cap=16)
    assert vol.log2 == 5
    vol.merge_units_(*_dev(*a), assume_unique=True)
    pos, keys = _expected_table(first, 5)
    occ = _occupied(vol)
    assert set(occ) == pos and set(occ.values()) == keys and {0, 31} <= set(occ)
    got = _by_coord(vol)
    assert set(got) == {tuple(k) for k in first.tolist()}
    for i, k in enumerate(first.tolist()):
        assert all(np.array_equal(x.view(np.int32), y[i].view(np.int32)) for x, y in zip(got[tuple(k)], a[1:])), k      # into an empty unit: bit for bit
    vol.merge_units_(*_dev(*a), assume_unique=True)
    assert vol.num_units == 12 and _occupied(vol) == occ
    twice = _by_coord(vol)
    for i, k in enumerate(first.tolist()):
        t, w, c = twice[tuple(k)]
        assert np.array_equal(w, 2 * a[2][i]) and np.abs(t.astype(np.float64) - a[1][i]).max() <= 1e-6
        assert np.abs(c.astype(np.float64) - a[3][i]).max() <= 1e-6 * 255 + 1e-4
    b = _random_units(more, 2)
    vol.merge_units_(*_dev(*b), assume_unique=True)
    assert vol.cap == 32 and vol.log2 == 6 and vol.num_units == 20
    both = np.concatenate([first, more])
    pos, keys = _expected_table(both, 6)
    occ = _occupied(vol)
    assert set(occ) == pos and set(occ.values()) == keys and {0, 63} <= set(occ)
    slots = vol.slot.cpu().numpy(); coord = vol.coord.cpu().numpy()
    for p, key in occ.items():                                            # every key names the pool slot that holds its coordinate
        assert tsdf_truth.ts_pack(*(int(v) for v in coord[slots[p]])) == key
    got = _by_coord(vol)
    assert set(got) == {tuple(k) for k in both.tolist()}
    for k in first.tolist():                                              # re-keyed: not a bit of a unit's data moved
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(got[tuple(k)], twice[tuple(k)])), k
    for i, k in enumerate(more.tolist()):
        assert all(np.array_equal(x.view(np.int32), y[i].view(np.int32)) for x, y in zip(got[tuple(k)], b[1:])), k


def test_units_at_the_ends_of_the_key_range():
    lo, hi = tsdf_truth.KEY_LO, tsdf_truth.KEY_HI
    coords = [(lo, hi, -1), (hi, lo, 1), (0, 0, 0)]
    u = _random_units(coords, 3)
    vol = _volume(cap=16)
    vol.merge_units_(*_dev(*u), assume_unique=True)
    got = _by_coord(vol)
    assert set(got) == set(coords)
    for i, k in enumerate(coords):
        assert all(np.array_equal(x.view(np.int32), y[i].view(np.int32)) for x, y in zip(got[k], u[1:])), k
    assert set(_occupied(vol).values()) == {tsdf_truth.ts_pack(*k) for k in coords}
    # the mesh: the three units are far apart, so it is their own meshes one after the other in ascending coordinate order
    order = sorted(range(3), key=lambda i: coords[i])
    vs, cs, ts, base = [], [], [], 0
    for i in order:
        v, c, t = ref.extract(u[1][i], u[2][i], u[3][i], VL, origin=tuple(16 * x for x in coords[i]))
        vs.append(v); cs.append(c); ts.append(t + base); base += len(v)
    want = np.concatenate(vs), np.concatenate(cs), np.concatenate(ts).astype(np.int32)
    assert len(want[2]) > 3000
    _mesh_equals(vol.extract_triangle_mesh(), want, "extreme coordinates")


def test_a_merged_unit_outside_the_key_range_is_refused():
    """k_ts_insert_list packed whatever it was given: a coordinate outside [-2^20 + 1, 2^20 - 2] took another unit's key (tsdf_truth.ts_pack shows which)
    without a word.  Now the error a frame with such a sample gets, and the volume stays usable."""
    vol = _volume(cap=16)
    good = _random_units([(0, 1, tsdf_truth.KEY_LO)], 4)
    vol.merge_units_(*_dev(*good), assume_unique=True)
    for bad in ((0, 0, tsdf_truth.KEY_HI + 2), (tsdf_truth.KEY_LO - 1, 0, 0), (0, tsdf_truth.KEY_HI + 1, 0), (0, -(1 << 21), 0)):
        with pytest.raises(RuntimeError, match="outside the addressable volume"):
            vol.merge_units_(*_dev(*_random_units([(3, 3, 3), bad], 5)), assume_unique=True)
    got = _by_coord(vol)                                                   # (3, 3, 3) may have been given a slot: then it is an explicit empty unit
    assert set(got) <= {(0, 1, tsdf_truth.KEY_LO), (3, 3, 3)} and not np.isnan(got[(0, 1, tsdf_truth.KEY_LO)][0]).any()
    assert all(np.array_equal(x, y[0]) for x, y in zip(got[(0, 1, tsdf_truth.KEY_LO)], good[1:]))
    if (3, 3, 3) in got:
        assert not any(x.any() for x in got[(3, 3, 3)])
    ok = _random_units([(3, 3, 3)], 6)
    vol.merge_units_(*_dev(*ok), assume_unique=True)                       # usable afterwards: the flag does not stick
    got = _by_coord(vol)
    assert set(got) == {(0, 1, tsdf_truth.KEY_LO), (3, 3, 3)} and all(np.array_equal(x, y[0]) for x, y in zip(got[(3, 3, 3)], ok[1:]))


# ---------------------------------------------------------------------------------------------------------------- the merge arithmetic
def _group_of(x, y, z):
    return ((x >> 2) << 8) | ((y >> 2) << 6) | ((z >> 2) << 4) | (((x >> 1) & 1) << 3) | (((y >> 1) & 1) << 2) | ((x & 1) << 1) | (y & 1)


def _merge_units(coords, seed):
    """Hand-made units: weights 0.25 .. 3 and 2^20 (every sum of two is a float32), with single zero voxels, whole zero groups (four consecutive z) and
    whole zero 128-byte lines (2 x 4 x 4 voxels); tsdf and colour are random also where the weight is 0 (they must not arrive)."""
    rng = np.random.default_rng(seed)
    n = len(coords)
    t = rng.uniform(-1, 1, (n, 16, 16, 16)).astype(np.float32)
    c = rng.uniform(0, 255, (n, 16, 16, 16, 3)).astype(np.float32)
    w = rng.choice(np.array([0.25, 0.5, 1.0, 2.75, 3.0, 2.0 ** 20], np.float32), (n, 16, 16, 16))
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    w.reshape(n, 16, 16, 4, 4)[rng.uniform(size=(n, 16, 16, 4)) < 0.3] = 0.0
    lines = rng.uniform(size=(n, 8, 4, 4)) < 0.4
    w[np.repeat(np.repeat(np.repeat(lines, 2, axis=1), 4, axis=2), 4, axis=3)] = 0.0
    return np.asarray(coords, np.int32), t, w, c


def _written_groups(vol):
    """{coordinate: [1024] bool} from the written-group words as they are (nothing materialised)."""
    n = vol.num_units
    bits = ((vol.mask[:n].view(n, 16, 1) >> torch.arange(64, device="cuda").view(1, 1, 64)) & 1).bool().view(n, 1024).cpu().numpy()
    return {tuple(k): bits[i] for i, k in enumerate(vol.coord[:n].cpu().tolist())}


def _lines_with_weight(w):
    """[16,16,16] weights -> [1024] bool per group: its run of eight groups (a 128-byte line) holds a non-zero weight."""
    x, y, z = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    line = np.zeros(128, bool)
    np.logical_or.at(line, (_group_of(x, y, z) >> 3).ravel(), (w > 0).ravel())
    return np.repeat(line, 8)


def test_merge_arithmetic_against_float64():
    A = _merge_units([(0, 0, 0), (1, 0, 0), (5, -3, 2)], 11)
    B = _merge_units([(1, 0, 0), (5, -3, 2), (7, 7, 7)], 12)
    wl = A[2][0]
    assert ((wl.reshape(16, 16, 4, 4) == 0).any(-1) & (wl.reshape(16, 16, 4, 4) > 0).any(-1)).sum() > 50      # zero voxels inside a group with data
    lines0 = _lines_with_weight(wl)
    assert 0.2 < lines0.mean() < 0.9 and (wl == 2.0 ** 20).any() and (wl == 0.25).any()
    vol = _volume(cap=16)
    vol.merge_units_(*_dev(*A), assume_unique=True)
    bits = _written_groups(vol)
    for i, k in enumerate(map(tuple, A[0].tolist())):                      # whole 8-group runs, exactly those that hold an incoming weight
        assert np.array_equal(bits[k], _lines_with_weight(A[2][i])), k
    got = _by_coord(vol)
    for i, k in enumerate(map(tuple, A[0].tolist())):
        has = A[2][i] > 0
        t, w, c = got[k]
        assert np.array_equal(w, A[2][i])
        assert np.array_equal(t[has].view(np.int32), A[1][i][has].view(np.int32)) and np.array_equal(c[has].view(np.int32), A[3][i][has].view(np.int32))
        assert not t[~has].any() and not c[~has].any()                     # neither the poison nor the incoming values of weightless voxels
    vol2 = _volume(cap=16)                                                 # again, without the materialising read in between
    vol2.merge_units_(*_dev(*A), assume_unique=True)
    for v in (vol, vol2):
        v.merge_units_(*_dev(*B), assume_unique=True)
    bits = _written_groups(vol2)
    ia = {tuple(k): i for i, k in enumerate(A[0].tolist())}
    ib = {tuple(k): i for i, k in enumerate(B[0].tolist())}
    for k in set(ia) | set(ib):
        want = np.zeros(1024, bool)
        for units, idx in ((A, ia), (B, ib)):
            if k in idx:
                want |= _lines_with_weight(units[2][idx[k]])
        assert np.array_equal(bits[k], want), k
    g1, g2 = _by_coord(vol), _by_coord(vol2)
    z = np.zeros((16, 16, 16), np.float32); z3 = np.zeros((16, 16, 16, 3), np.float32)
    worst_t = worst_c = 0.0
    for k in set(ia) | set(ib):
        t0, w0, c0 = (A[1][ia[k]], A[2][ia[k]], A[3][ia[k]]) if k in ia else (z, z, z3)
        t1, w1, c1 = (B[1][ib[k]], B[2][ib[k]], B[3][ib[k]]) if k in ib else (z, z, z3)
        t, w, c = g2[k]
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(g1[k], g2[k])), k
        assert not np.isnan(t).any() and not np.isnan(w).any() and not np.isnan(c).any()
        assert np.array_equal(w, w0 + w1), k                               # float32 sums, exact by the choice of weights
        only0, only1, both, none = (w0 > 0) & (w1 == 0), (w0 == 0) & (w1 > 0), (w0 > 0) & (w1 > 0), (w0 == 0) & (w1 == 0)
        assert both.sum() > 100 or k not in ia or k not in ib
        for m, ts, cs in ((only0, t0, c0), (only1, t1, c1)):               # no weight on the other side: bit for bit
            assert np.array_equal(t[m].view(np.int32), ts[m].view(np.int32)) and np.array_equal(c[m].view(np.int32), cs[m].view(np.int32)), k
        assert not t[none].any() and not c[none].any()
        W0, W1 = w0.astype(np.float64)[both], w1.astype(np.float64)[both]
        et = np.abs(t[both] - (t0[both].astype(np.float64) * W0 + t1[both].astype(np.float64) * W1) / (W0 + W1))
        wc = (c0[both].astype(np.float64) * W0[:, None] + c1[both].astype(np.float64) * W1[:, None]) / (W0 + W1)[:, None]
        ec = np.abs(c[both] - wc)
        if both.any():
            worst_t, worst_c = max(worst_t, float(et.max())), max(worst_c, float((ec - 1e-6 * np.abs(wc)).max()))
            assert (et <= 1e-6).all() and (ec <= 1e-6 * np.abs(wc) + 1e-4).all(), k
    print(f"merge: worst tsdf error {worst_t:.2e}, worst colour error beyond 1e-6 relative {worst_c:.2e}")


# ---------------------------------------------------------------------------------------------------------------- a stale error text
def test_growth_is_decided_by_the_frames_own_status_not_by_a_stale_error_text():
    """A deferred frame refused at enqueue ("bad arguments": 65536 pixels wide) is looked at only by finish(); in between another volume fails with
    "capacity exhausted".  The library's error text is one global string: finish() used to find the other volume's text in it, grow this volume and run
    the frame again."""
    from gsrast.tsdf import ScalableTSDFVolume
    vol = _volume(cap=16)
    vol.integrate(torch.zeros(3, 1, 65536, device="cuda"), torch.ones(1, 1, 65536, device="cuda"), 10.0, 10.0, 0.0, 0.0, np.eye(4, dtype=np.float32), defer=True)
    assert len(vol._queue) == 1 and vol._queue[0]["rc"] != 0
    other = ScalableTSDFVolume(VL, TR, capacity_units=16, auto_grow=False)
    f = tsdf_cases.small_scene("t5")[0][0]
    with pytest.raises(RuntimeError, match="capacity exhausted"):
        other.integrate(*_dev(f["rgb"], f["depth"]), f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=6.0)
    with pytest.raises(RuntimeError, match="bad arguments"):
        vol.finish()
    assert vol.cap == 16 and len(vol.chunks) == 1 and not vol._queue
    vol.integrate(*_dev(f["rgb"], f["depth"]), f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=6.0)      # usable, and a real exhaustion still grows
    assert vol.cap > 16 and vol.num_units == len(tsdf_cases.small_truth("t5")[-1].touched[0][0])
