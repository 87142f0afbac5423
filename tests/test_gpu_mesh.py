"""GPU tests (pytest -m gpu) of gsrast.tsdf.ScalableTSDFVolume.extract_triangle_mesh() (gsr_tsdf_sparse_mesh_* of the C ABI) against the numpy
restatement of the mesh's definition (ref_mesh_numpy): triangles EQUAL (the sign decisions are taken on the same stored floats), vertices within
2 float32 ulps of the reference value (one ulp for the device's division), colours within 4 * 2^-24.  Volumes are hand-made through merge_units_."""
import functools

import numpy as np
import pytest
import torch

import ref_mesh_numpy as ref
import tsdf_cases

pytestmark = pytest.mark.gpu

VL = 0.02


def _volume(units, cap=64, perm=None, one_by_one=False):
    """A volume holding the given unit lists (coords, tsdf, weight, color), inserted in the order `perm`."""
    from gsrast.tsdf import ScalableTSDFVolume
    vol = ScalableTSDFVolume(VL, 5 * VL, capacity_units=cap)
    for ch in vol.chunks:                      # whatever the pools held must never show
        ch.fill_(float("nan"))
    vol.mask.fill_(-1)
    co, t, w, c = units
    idx = np.arange(len(co)) if perm is None else np.asarray(perm)
    steps = [idx[i:i + 1] for i in range(len(idx))] if one_by_one else [idx]
    for s in steps:
        vol.merge_units_(*(torch.from_numpy(np.ascontiguousarray(a[s])).cuda() for a in (co, t, w, c)), assume_unique=True)
    return vol


def _check(mesh, want, what=""):
    m = mesh.cpu()
    v, c, t = m.vertices.numpy(), m.vertex_colors.numpy(), m.triangles.numpy()
    rv, rc, rt = want
    assert v.dtype == np.float32 and c.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == rv.shape and t.shape == rt.shape, (what, v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(t, rt), what
    ulps = np.abs(v.astype(np.float64) - rv.astype(np.float64)) / np.spacing(np.abs(rv)).astype(np.float64)
    cerr = np.abs(c.astype(np.float64) - rc.astype(np.float64))
    print(f"{what}: {len(v)} vertices, {len(t)} triangles, position error {ulps.max() if len(v) else 0:.2f} ulp, colour error {cerr.max() if len(v) else 0:.2e}")
    assert (ulps <= 2.0).all(), what
    assert (cerr <= 4 * 2.0 ** -24).all(), what


def _same_bytes(a, b):
    a, b = a.cpu(), b.cpu()
    return all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in ((a.vertices, b.vertices), (a.vertex_colors, b.vertex_colors), (a.triangles, b.triangles)))


def test_all_256_cases():
    """2 x 2 x 2 units at {-1, 0}^3; isolated cubes on a lattice of pitch 3 from voxel 0 of the lower units: an origin coordinate of 15 straddles two
    units, the cube at (15, 15, 15) has a corner in each of the eight."""
    rng = np.random.default_rng(1)
    f = np.zeros((32, 32, 32), np.float32)
    w = np.zeros_like(f)
    want_tris, k = 0, 0
    for ox in range(0, 31, 3):
        for oy in range(0, 31, 3):
            for oz in range(0, 31, 3):
                case = (k * 37 + 1) % 256 if (ox, oy, oz) != (15, 15, 15) else 0b10010110
                k += 1
                for i, (dx, dy, dz) in enumerate(ref.gen_mc_table.CORNERS):
                    f[ox + dx, oy + dy, oz + dz] = rng.uniform(0.1, 0.9) * (-1.0 if (case >> i) & 1 else 1.0)
                    w[ox + dx, oy + dy, oz + dz] = float(rng.integers(1, 4))
                want_tris += int(ref.TABLE[case, 15])
    assert k >= 256 * 5
    col = rng.uniform(0, 255, f.shape + (3,)).astype(np.float32)
    want = ref.extract(f, w, col, VL, origin=(-16, -16, -16))
    assert len(want[2]) == want_tris
    vol = _volume(ref.units_from_dense(f, w, col, (-1, -1, -1)))
    mesh = vol.extract_triangle_mesh()
    assert int(mesh.triangles.shape[0]) == want_tris
    _check(mesh, want, "256 cases")


@functools.lru_cache(maxsize=None)
def _random_content(weights_0123=False, fillers=0):
    """A random field over 2 x 2 x 2 units at (-1, 2, 0) + {0, 1}^3: 10 % of the voxels without weight, unit 5 absent, unit 2 present with all weights 0;
    `fillers` further units in a row along x behind it.  -> (unit lists, dense arrays + origin)"""
    rng = np.random.default_rng(7)
    nx = 32 + 16 * fillers
    f = rng.uniform(-1, 1, (nx, 32, 32)).astype(np.float32)
    f[rng.uniform(size=f.shape) < 0.01] = 0.0                      # ties count as outside
    w = rng.integers(0, 4, f.shape).astype(np.float32) if weights_0123 else (rng.uniform(size=f.shape) > 0.1).astype(np.float32) * rng.integers(1, 9, f.shape)
    w = w.astype(np.float32)
    col = rng.uniform(0, 255, f.shape + (3,)).astype(np.float32)
    if fillers:
        f[32:, 16:, :] = 0.5; w[32:, 16:, :] = 0.0; w[32:, :, 16:] = 0.0      # the row of fillers is one unit thick
    co, T, W, Cc = ref.units_from_dense(f, w, col, (-1, 2, 0))
    W[2] = 0.0
    keep = np.array([i for i in range(len(co)) if i != 5 and not (fillers and (co[i, 0] > 0) and (co[i, 1] > 2 or co[i, 2] > 0))])
    units = tuple(a[keep] for a in (co, T, W, Cc))
    dense = ref.dense_from_units(*units)
    return units, dense


def test_random_field_with_holes():
    units, (T, W, Cc, org) = _random_content()
    vol = _volume(units)
    assert vol.num_units == 7
    _check(vol.extract_triangle_mesh(), ref.extract(T, W, Cc, VL, origin=org), "random field")


def test_random_field_min_weight():
    units, (T, W, Cc, org) = _random_content(weights_0123=True)
    vol = _volume(units)
    want = ref.extract(T, W, Cc, VL, origin=org, min_weight=1.5)
    assert 0 < len(want[2]) < len(ref.extract(T, W, Cc, VL, origin=org)[2])
    _check(vol.extract_triangle_mesh(min_weight=1.5), want, "min_weight 1.5")
    _check(vol.extract_triangle_mesh(), ref.extract(T, W, Cc, VL, origin=org), "min_weight 0")


def test_more_than_1024_units():
    """1030 units in a row along x: the one-workgroup scan of the units' vertex and triangle counts takes a second chunk of 1024 and carries the
    first chunk's totals into it.  A random field in the units at output positions 0, 1, 1023, 1024, 1028 and 1029 -- either side of the chunk
    edge and at both ends; the others hold tsdf 0.5 at weight 1: present, live, without a surface of their own, but with one against a field
    unit beside them.  Inserted in a shuffled order, so that a unit's place in the pool is not its place in the output."""
    rng = np.random.default_rng(13)
    n = 1030
    f = np.full((16 * n, 16, 16), 0.5, np.float32); w = np.ones_like(f); col = np.zeros(f.shape + (3,), np.float32)
    for u in (0, 1, 1023, 1024, 1028, 1029):
        s = slice(16 * u, 16 * u + 16)
        f[s] = rng.uniform(-1, 1, (16, 16, 16)).astype(np.float32)
        f[s][rng.uniform(size=(16, 16, 16)) < 0.01] = 0.0
        w[s] = ((rng.uniform(size=(16, 16, 16)) > 0.1) * rng.integers(1, 9, (16, 16, 16))).astype(np.float32)
        col[s] = rng.uniform(0, 255, (16, 16, 16, 3)).astype(np.float32)
    want = ref.extract(f, w, col, VL)
    units = ref.units_from_dense(f, w, col, (0, 0, 0))
    assert len(units[0]) == n > 1024 and units[0][1024].tolist() == [1024, 0, 0]
    in_late_units = want[0][:, 0] > VL * 16 * 1024                # vertices of the units of the second chunk
    assert in_late_units.sum() > 1000 and (~in_late_units).sum() > 1000
    vol = _volume(units, cap=2048, perm=rng.permutation(n))
    assert vol.num_units == n
    _check(vol.extract_triangle_mesh(), want, "1030 units")


TM_GRID = 4096                                            # csrc/gsr_tsdf_mesh.hip: workgroups of the count and the emit at most (test_mesh_cpu holds it to the source)
ROW_UNITS, ROW_FIELDS = 4100, (0, 1, 4095, 4096, 4099)


def _row_volume(fields, order, step=512):
    """The row of ROW_UNITS units in a pool of 8192, inserted in the given order, `step` units per merge: the fillers are never all on the host."""
    from gsrast.tsdf import ScalableTSDFVolume
    vol = ScalableTSDFVolume(VL, 5 * VL, capacity_units=8192)
    for ch in vol.chunks:
        ch.fill_(float("nan"))
    vol.mask.fill_(-1)
    for i in range(0, len(order), step):
        vol.merge_units_(*(torch.from_numpy(a).cuda() for a in ref.row_units(fields, order[i:i + step])), assume_unique=True)
    return vol


def test_more_than_4096_units():
    """4100 units in a row along x: the count and the emit run TM_GRID = 4096 workgroups, and workgroups 0 .. 3 stage a second unit -- output
    positions 4096 .. 4099 -- into the shared memory that held their first.  A random field in the units at positions 0, 1, 4095, 4096 and 4099 --
    either side of the grid's turn and at both ends; fillers elsewhere, inserted in a shuffled order.  The truth is the mesh of units 0 .. 3
    followed by the mesh of units 4092 .. 4099: every unit between is a filler among fillers (test_mesh_cpu holds the identity on 12 units)."""
    rng = np.random.default_rng(17)
    n = ROW_UNITS
    fields = {u: ref.field_unit(rng) for u in ROW_FIELDS}
    want = ref.concat([ref.extract_row(fields, 0, 4, VL), ref.extract_row(fields, n - 8, n, VL)])
    past_the_turn = want[0][:, 0] > VL * 16 * TM_GRID                                          # vertices of the units a workgroup takes second
    assert past_the_turn.sum() > 1000 and (~past_the_turn).sum() > 1000
    vol = _row_volume(fields, rng.permutation(n))
    assert vol.num_units == n == 4100 > TM_GRID == 4096
    mesh = vol.extract_triangle_mesh()
    _check(mesh, want, "4100 units")
    assert (mesh.vertices[:, 0] > VL * 16 * TM_GRID).sum().item() == past_the_turn.sum()
    assert _same_bytes(mesh, vol.extract_triangle_mesh())
    del vol
    assert _same_bytes(mesh, _row_volume(fields, rng.permutation(n)).extract_triangle_mesh())   # the same content in another order


def test_sphere_on_the_device():
    n, h, centre, r = 32, 0.05, (0.8131, 0.7877, 0.8023), 0.41
    tsdf, w, col = ref.sphere(n, h, centre, r)
    from gsrast.tsdf import ScalableTSDFVolume
    vol = ScalableTSDFVolume(h, 5 * h, capacity_units=16)
    vol.merge_units_(*(torch.from_numpy(a).cuda() for a in ref.units_from_dense(tsdf, w, col, (0, 0, 0))), assume_unique=True)
    mesh = vol.extract_triangle_mesh()
    _check(mesh, ref.extract(tsdf, w, col, h), "sphere")
    m = mesh.cpu()
    v, t = m.vertices.numpy(), m.triangles.numpy()
    top = ref.topology(t, len(v))
    assert top["watertight"] and top["euler"] == 2 and top["unused"] == 0
    assert ref.signed_volume(v, t) > 0
    assert len(np.unique(v, axis=0)) == len(v)
    assert np.abs(np.linalg.norm(v.astype(np.float64) - np.array(centre), axis=1) - r).max() <= h * h / (8 * (r - h))


@pytest.mark.parametrize("defer", [False, True])
def test_integrated_volume_is_left_untouched(defer):
    from gsrast.tsdf import ScalableTSDFVolume
    vol = ScalableTSDFVolume(0.02, 0.1, capacity_units=4096)
    for ch in vol.chunks:
        ch.fill_(float("nan"))
    vol.mask.fill_(-1)
    for f in tsdf_cases.frames(2):
        vol.integrate(torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["depth"]).cuda(), f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=6.0,
                      defer=defer)
    assert bool(vol._queue) == defer                      # deferred frames are still in flight at the call
    if not defer:
        snap = [c.clone() for c in vol.chunks], vol.mask.clone(), vol.stamp.clone()
    mesh = vol.extract_triangle_mesh()
    if defer:
        assert not vol._queue
        snap = [c.clone() for c in vol.chunks], vol.mask.clone(), vol.stamp.clone()
    again = vol.extract_triangle_mesh()
    assert _same_bytes(mesh, again)
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    assert len(snap[0]) == len(vol.chunks) and all(torch.equal(bits(a), bits(b)) for a, b in zip(snap[0], vol.chunks))
    assert torch.equal(snap[1], vol.mask) and torch.equal(snap[2], vol.stamp)
    co, t, w, c = (x.cpu().numpy() for x in vol.units())
    T, W, Cc, org = ref.dense_from_units(co, t, w, c)
    want = ref.extract(T, W, Cc, 0.02, origin=org)
    assert len(want[2]) > 10000
    _check(mesh, want, f"integrated, defer={defer}")
    assert _same_bytes(mesh, vol.extract_triangle_mesh())      # materialised by units(): the same content, the same mesh


def test_order_capacity_and_chunks_do_not_matter():
    units, (T, W, Cc, org) = _random_content(fillers=40)
    n = len(units[0])
    assert n == 47
    a = _volume(units, cap=64)
    perm = np.random.default_rng(3).permutation(n)
    b = _volume(units, cap=64, perm=perm)
    c = _volume(units, cap=16, perm=perm[::-1], one_by_one=True)
    assert len(c.chunks) >= 3 and len(a.chunks) == 1
    ma, mb, mc = a.extract_triangle_mesh(), b.extract_triangle_mesh(), c.extract_triangle_mesh()
    _check(ma, ref.extract(T, W, Cc, VL, origin=org), "47 units")
    assert _same_bytes(ma, mb) and _same_bytes(ma, mc)
    # the content of test_random_field_with_holes itself, permuted, and in a pool that has been grown to three chunks on the way
    units7, _ = _random_content()
    p7 = np.random.default_rng(4).permutation(7)
    d = _volume(units7, cap=16, perm=p7[:3])
    for part in (p7[3:5], p7[5:]):
        d._grow()
        d.merge_units_(*(torch.from_numpy(np.ascontiguousarray(x[part])).cuda() for x in units7), assume_unique=True)
    assert len(d.chunks) == 3 and d.num_units == 7
    m7 = _volume(units7).extract_triangle_mesh()
    assert _same_bytes(m7, _volume(units7, perm=p7).extract_triangle_mesh()) and _same_bytes(m7, d.extract_triangle_mesh())


def test_empty_results():
    from gsrast.tsdf import ScalableTSDFVolume, TriangleMesh
    vol = ScalableTSDFVolume(VL, 5 * VL, capacity_units=16)
    rng = np.random.default_rng(0)
    for k in range(2):
        m = vol.extract_triangle_mesh()
        assert isinstance(m, TriangleMesh) and m.vertices.is_cuda
        assert tuple(m.vertices.shape) == (0, 3) and tuple(m.vertex_colors.shape) == (0, 3) and tuple(m.triangles.shape) == (0, 3)
        assert m.vertices.dtype == torch.float32 and m.vertex_colors.dtype == torch.float32 and m.triangles.dtype == torch.int32
        assert tuple(m.cpu().triangles.shape) == (0, 3)
        f = rng.uniform(0.1, 1, (32, 16, 16)).astype(np.float32)      # second round: two units, all positive
        vol.merge_units_(*(torch.from_numpy(a).cuda() for a in ref.units_from_dense(f, np.ones_like(f), np.zeros(f.shape + (3,), np.float32), (0, 0, 0))),
                         assume_unique=True)
    assert vol.num_units == 2
