"""CPU tests of the mesh rasterizer's restatement (tests/raster_truth.py) and of its named inputs (tests/raster_cases.py), and of what
gsrast.rasterize_mesh / triangle_view_counts / cull_unseen_triangles check before they touch the library.  The restatement is what
tests/test_gpu_mesh_raster.py holds the kernels to bit for bit, so it is itself held here to an independent float64 ray cast, to a second way of
evaluating the depth, and to the facts every named case is there for."""
import numpy as np
import pytest
import torch

import raster_cases as cases
import raster_truth as truth

# E_k == 0 at a candidate centre, summed over the triangles and edges of the case's first view.  The lattice: a triangle with legs of 4 pixels has 5
# centres on each leg and 5 on the diagonal, 15 (centre, edge) pairs, times 98 triangles.  The others are recorded so that a change of a case that
# loses its ties is seen.
TIES = {"ortho_lattice": 1470, "ortho_lattice_flipped": 1470, "sliver": 1, "whole_image": 0, "crossing": 13, "duplicate": 44, "zero_area": 12}


def _first(name):
    return cases.truth_views(name)[0]


def test_the_lattice_is_pixel_exact_and_watertight():
    for name in ("ortho_lattice", "ortho_lattice_flipped"):
        k, r = cases.CASES[name], _first(name)
        px, py, w = r["vert"]
        assert (w == 1.0).all() and np.array_equal(px, k["v"][:, 0].astype(np.float64)) and np.array_equal(py, k["v"][:, 1].astype(np.float64))
        want = np.zeros((32, 32), bool)
        want[:28, :28] = True                             # rows and columns 0 .. 27: the bottom and right boundary belong to nobody
        assert np.array_equal(r["triangle_id"] >= 0, want)
        assert (r["depth"][want] == 1.0).all() and (r["depth"][~want] == 0.0).all()
        assert r["ties"] == TIES[name] and r["dropped"].tolist() == [0, 0, 0]
    a, b = _first("ortho_lattice"), _first("ortho_lattice_flipped")
    assert np.array_equal(a["triangle_id"], b["triangle_id"])                               # the rule does not depend on the winding
    sw = lambda n: truth.setup(cases.CASES[n]["v"], cases.CASES[n]["t"], cases.CASES[n]["mats"][0], 32, 32, 0.01, 0)[5]
    assert sw("ortho_lattice").all() != sw("ortho_lattice_flipped").all()
    # every pixel of the lattice's interior has exactly one owner although up to six triangles have it on an edge: count the coverings directly
    k = cases.CASES["ortho_lattice"]
    cover = np.zeros((32, 32), np.int64)
    for t in range(len(k["t"])):
        one = truth.rasterize(k["v"], k["t"][t:t + 1], k["mats"][0], 32, 32)
        cover += one["triangle_id"] >= 0
    assert np.array_equal(cover, want.astype(np.int64))


def test_the_cases_hit_what_they_claim():
    for name, n in TIES.items():
        assert _first(name)["ties"] == n, name
    r = _first("sliver")
    assert r["box"][0] == 4 and (r["triangle_id"] == -1).all() and r["dropped"].tolist() == [0, 0, 0]
    r = _first("offscreen")
    assert (r["state"] == truth.OK).all() and (r["box"] == 0).all() and (r["triangle_id"] == -1).all()
    r = _first("straddle")
    ids = r["triangle_id"]
    assert set(ids[:, 0]) >= {0} and set(ids[:, -1]) >= {1} and set(ids[0]) >= {2} and set(ids[-1]) >= {3} and (r["box"] > 0).all()
    r = _first("whole_image")
    assert (r["triangle_id"] == 0).all() and r["box"][0] == 32 * 32 and r["depth"].min() > 1.0 and r["depth"].max() < 3.0
    k = cases.CASES["guard_inside"]
    st, X, *_ = truth.setup(k["v"], k["t"], k["mats"][0], 32, 32, 0.01, 0)
    assert st.tolist() == [truth.OK] and X.max() == 1 << 24 and (_first("guard_inside")["triangle_id"] == 0).sum() > 0
    k = cases.CASES["guard_outside"]
    px = truth.project(k["v"], k["mats"][0], 32, 32)[0]
    assert np.rint(px * 256.0).max() == (1 << 24) + 1                                        # one step outside
    assert _first("guard_outside")["dropped"].tolist() == [0, 1, 0] and _first("guard_outside")["state"].tolist() == [truth.GUARDED, truth.OK]
    k = cases.CASES["near_exact"]
    assert truth.project(k["v"], k["mats"][0], 32, 32)[2][0] == k["near"] == cases.NEAR
    assert _first("near_exact")["dropped"].tolist() == [1, 0, 0] and (_first("near_exact")["triangle_id"] != 0).all()
    k = cases.CASES["near_above"]
    assert truth.project(k["v"], k["mats"][0], 32, 32)[2][0] == cases.JUST_ABOVE_NEAR > cases.NEAR
    assert _first("near_above")["dropped"].tolist() == [0, 0, 0] and (_first("near_above")["triangle_id"] == 0).sum() > 100
    assert _first("behind")["dropped"].tolist() == [1, 0, 0] and (_first("behind")["triangle_id"] != 0).all()
    r = _first("duplicate")
    assert (r["triangle_id"] >= 0).sum() > 100 and (r["triangle_id"] <= 0).all()             # of two equal triangles the lower index wins
    r = _first("crossing")
    assert (r["triangle_id"] == 0).sum() > 50 and (r["triangle_id"] == 1).sum() > 50
    r = _first("zero_area")
    assert r["state"].tolist() == [truth.ZERO, truth.ZERO, truth.OK] and r["dropped"].tolist() == [0, 0, 2]
    pos, neg, both = _first("sphere_33x31_cull_pos"), _first("sphere_33x31_cull_neg"), _first("sphere_33x31")
    assert (pos["state"] == truth.CULLED).sum() + (neg["state"] == truth.CULLED).sum() == 400 - (both["state"] == truth.ZERO).sum() * 2
    assert np.array_equal(neg["triangle_id"], both["triangle_id"])                           # the outside of these spheres is area2 < 0
    assert (pos["triangle_id"] >= 0).sum() > 0 and not np.array_equal(pos["triangle_id"], both["triangle_id"])
    assert pos["dropped"].tolist() == neg["dropped"].tolist() == both["dropped"].tolist()    # culled is not dropped
    assert cases.CASES["image_17x15"]["W"] % 16 == 1 and cases.CASES["no_triangles"]["t"].shape == (0, 3) and cases.CASES["no_views"]["mats"].shape == (0, 4, 4)
    for name in cases.NAMES:
        k = cases.CASES[name]
        assert len(k["t"]) <= 6400 and k["W"] <= 128 and k["H"] <= 96 and truth.status(k["v"], k["t"]) == 0
    for name, (k, kind) in cases.errors().items():
        assert truth.status(k["v"], k["t"]) == {"nonfinite": truth.ERR_NONFINITE, "index": truth.ERR_INDEX}[kind], name
        with pytest.raises(ValueError):
            truth.rasterize(k["v"], k["t"], k["mats"][0], k["W"], k["H"])


def test_the_many_views_case_takes_a_second_chunk_of_views():
    """gsr_mesh_rasterize walks the views in chunks of min(max(RS_BUDGET / per-view scratch, 1), RS_CHUNK_MAX, n_views) and its scratch is one
    chunk's: the library's own answer stops growing at RS_CHUNK_MAX views for this size, so view 1024 of box_1030_views starts a second turn."""
    import os
    import re
    import gsrast
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-sr_amd", "csrc", "gsr_mesh_raster.hip")).read()
    assert re.search(r"^#define RS_CHUNK_MAX %d\s" % cases.CHUNK_MAX, src, flags=re.M) and re.search(r"^#define RS_BUDGET \(\(size_t\)256 << 20\)", src, flags=re.M)
    assert "for (int64_t v0 = 0; v0 < n_views; v0 += m.chunk)" in src
    k = cases.CASES["box_1030_views"]
    n, T, V, W, H = len(k["mats"]), len(k["t"]), len(k["v"]), k["W"], k["H"]
    assert (n, T, W, H) == (cases.MANY_VIEWS, 12, 16, 12) and n > cases.CHUNK_MAX
    q = lambda views: gsrast.lib().gsr_mesh_raster_scratch_bytes(T, V, views, W, H)
    assert q(cases.CHUNK_MAX - 1) < q(cases.CHUNK_MAX) == q(n) == q(100000)                   # the views, not the budget, cap the chunk
    align = lambda x: -(-x // 256) * 256
    per_view = align(W * H * 8) + align(4 * T) + align(T)                                    # rs_carve: keys, list and owner bytes of one view
    assert (256 << 20) // per_view > 100 * cases.CHUNK_MAX and "RS_BUDGET / per_view" in src  # the budget alone would allow a hundred times as many
    assert q(cases.CHUNK_MAX) - q(cases.CHUNK_MAX // 2) >= (cases.CHUNK_MAX // 2) * (W * H * 8 + 5 * T)
    # the truth: every view sees the box, and the counts differ from triangle to triangle
    hits = [int((r["triangle_id"] >= 0).sum()) for r in cases.truth_views("box_1030_views")]
    assert min(hits) > 20 and all(r["dropped"].tolist() == [0, 0, 0] for r in cases.truth_views("box_1030_views"))
    plain, tol = cases.truth_counts("box_1030_views"), cases.truth_counts("box_1030_views", cases.TOLERANCE)
    assert plain.sum() > 2 * n and (tol >= plain).all() and tol.max() <= n and len(set(tol.tolist())) > 1 and tol.min() < 1000 <= tol.max()
    both = lambda a, b: truth.view_counts(k["v"], k["t"], k["mats"][a:b], W, H, k["near"], k["cull_sign"], cases.TOLERANCE, views=cases.truth_views("box_1030_views")[a:b])
    assert np.array_equal(both(0, cases.CHUNK_MAX) + both(cases.CHUNK_MAX, n), tol) and both(cases.CHUNK_MAX, n).max() > 0


def test_the_scratch_query_refuses_what_the_input_check_cannot_cover():
    """k_rs_check runs one thread per vertex component and index, 3 max(V, T) of them in 32-bit arithmetic: V is held to 3 V < 2^31 like T, so that
    the rounded-up grid never wraps and leaves vertices unchecked.  The scratch query answers 0 for a refused size, as for every other one."""
    import gsrast
    q = lambda T, V: gsrast.lib().gsr_mesh_raster_scratch_bytes(T, V, 3, 16, 12)
    last = (1 << 31) // 3                                  # 3 * 715 827 882 = 2^31 - 2
    assert 3 * last < 1 << 31 <= 3 * (last + 1)
    assert q(10, last) > 0 and q(last, last) > 0 and q(last, 10) > 0
    assert q(10, last + 1) == 0 and q(10, (1 << 31) - 1) == 0 and q(10, 1431655681) == 0 and q(last + 1, 10) == 0 and q(10, -1) == 0
    assert q(10, last) == q(10, 10)                        # the vertices take no scratch


def _ray_cast(k, M):
    """An independent float64 ray cast on the UNSNAPPED coordinates: strict inequalities, no tie rule, no integers.  -> ids [H,W] (-1: no hit),
    and the mask of the pixels that are more than 4/256 px from the (infinite) edge lines of every triangle in front of the near plane (snapping
    moves a vertex by at most 1/512 px per axis: beyond that band the two coverages agree) and whose two nearest depths differ by more than 1e-6
    relative."""
    W, H = k["W"], k["H"]
    px, py, w = truth.project(k["v"], M, W, H)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    best, second, ids, clear = np.full((H, W), np.inf), np.full((H, W), np.inf), np.full((H, W), -1), np.ones((H, W), bool)
    for t, (a, b, c) in enumerate(k["t"]):
        if not (w[[a, b, c]] > k["near"]).all():
            continue
        x, y, iw = px[[a, b, c]], py[[a, b, c]], 1.0 / w[[a, b, c]]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0:
            continue
        lam = []
        for i, j in ((1, 2), (2, 0), (0, 1)):
            e = (x[j] - x[i]) * (row - y[i]) - (y[j] - y[i]) * (col - x[i])
            clear &= np.abs(e) / np.hypot(x[j] - x[i], y[j] - y[i]) > 4.0 / 256.0
            lam.append(e / area)
        inside = (lam[0] > 0) & (lam[1] > 0) & (lam[2] > 0)
        z = np.where(inside, 1.0 / (lam[0] * iw[0] + lam[1] * iw[1] + lam[2] * iw[2]), np.inf)
        closer = z < best
        second = np.where(closer, best, np.minimum(second, z))
        ids = np.where(closer, t, ids)
        best = np.where(closer, z, best)
    with np.errstate(invalid="ignore"):
        apart = ~np.isfinite(second) | ((second - best) > 1e-6 * best)
    return ids, clear & apart


@pytest.mark.parametrize("name", ["sphere_33x31", "sphere_64x48"])
def test_the_truth_agrees_with_an_independent_ray_cast(name):
    k = cases.CASES[name]
    compared = mismatches = total = 0
    for M, r in zip(k["mats"][:2], cases.truth_views(name)[:2]):
        ids, mask = _ray_cast(k, M)
        compared += int(mask.sum()); total += mask.size
        mismatches += int((ids[mask] != r["triangle_id"][mask]).sum())
        print(f"{name}: {mask.mean():.2f} of the pixels compared, {int((ids[mask] != r['triangle_id'][mask]).sum())} mismatches among them, "
              f"{int((ids != r['triangle_id']).sum())} over all pixels")
    assert compared >= 0.4 * total, compared / total
    assert mismatches == 0


@pytest.mark.parametrize("name", ["sphere_33x31", "sphere_64x48", "crossing", "whole_image"])
def test_the_truths_depth_is_the_float64_depth_at_the_snapped_coordinates(name):
    """A second evaluation: 1 / w is affine in the image, so it is the plane through the three snapped vertices, solved for with a 3 x 3 system."""
    k = cases.CASES[name]
    r = _first(name)
    st, X, Y, rw, A, sw, _ = truth.setup(k["v"], k["t"], k["mats"][0], k["W"], k["H"], k["near"], k["cull_sign"])
    rows, cols = np.nonzero(r["triangle_id"] >= 0)
    assert len(rows) > 100
    worst = 0.0
    for row, col in zip(rows, cols):
        t = r["triangle_id"][row, col]
        plane = np.linalg.solve(np.stack([X[t] / 256.0, Y[t] / 256.0, np.ones(3)], axis=1), rw[t])
        z = 1.0 / (plane[0] * col + plane[1] * row + plane[2])
        worst = max(worst, abs(float(r["depth"][row, col]) - z) / z)
    print(f"{name}: worst relative difference {worst:.3e}")
    assert worst <= 2.0 ** -23                            # one float32 rounding (2^-24) and the float64 noise of the solve


def test_barycentrics_are_weights_of_the_index_buffers_vertices():
    """Interpolating w itself with the weights gives the depth back, for both windings: the weights follow the index buffer, not the exchanged order."""
    for name in ("sphere_33x31", "crossing", "whole_image"):
        k, r = cases.CASES[name], _first(name)
        w = r["vert"][2]
        hit = r["triangle_id"] >= 0
        tri = k["t"][r["triangle_id"][hit]]
        b1, b2 = r["barycentric"][hit][:, 0].astype(np.float64), r["barycentric"][hit][:, 1].astype(np.float64)
        z = (1 - b1 - b2) * w[tri[:, 0]] + b1 * w[tri[:, 1]] + b2 * w[tri[:, 2]]
        assert np.abs(z - r["depth"][hit]).max() <= 1e-5 * r["depth"][hit].max(), name
        assert (r["barycentric"][~hit] == 0).all() and b1.min() >= 0 and b2.min() >= 0 and (b1 + b2).max() <= 1 + 1e-6


def test_counts_on_a_closed_box():
    k, normals, eyes = cases.closed_box()
    import ref_mesh_numpy
    assert ref_mesh_numpy.signed_volume(k["v"], k["t"]) > 0
    v = k["v"].astype(np.float64)[k["t"]]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert np.allclose(n / np.linalg.norm(n, axis=1, keepdims=True), normals)                # counter-clockwise seen from outside
    for tol in (None, 0.01):
        for sign in (0, -1):
            counts = truth.view_counts(k["v"], k["t"], k["mats"], k["W"], k["H"], cull_sign=sign, depth_tolerance=tol)
            # a camera on an axis sees the one face whose normal points at it
            want = np.array([sum(1 for e in eyes if float(np.dot(nn, e - c.mean(0))) > 0) for nn, c in zip(normals, v)])
            if tol is None:
                assert np.array_equal(counts, want), (tol, sign, counts, want)
            else:                                         # the vertex test of an unculled back face passes only at the silhouette, where its vertices are the front face's
                assert (counts >= want).all() and (sign == 0 or np.array_equal(counts, want))
    turned = dict(k)
    turned["mats"] = k["mats"][:1]                        # one camera: the five faces that look away from it are never seen
    c = truth.view_counts(turned["v"], turned["t"], turned["mats"], k["W"], k["H"])
    assert c.tolist() == [0, 0, 1, 1] + [0] * 8


def test_the_fine_sphere_has_triangles_only_the_vertex_test_sees():
    plain, tol = cases.truth_counts("sphere_128x96"), cases.truth_counts("sphere_128x96", cases.TOLERANCE)
    only = (plain == 0) & (tol > 0)
    assert only.sum() > 1000 and (tol >= plain).all() and (tol == 0).sum() > 0
    r = _first("sphere_128x96")
    assert (r["box"] <= 2).sum() > 3200 and (r["box"] == 0).sum() > 500       # mostly at most two candidate centres, hundreds with none at all


def test_the_outside_of_a_marching_cubes_mesh_is_cull_sign_minus_one():
    import ref_mesh_numpy as rm
    v, _, t = rm.extract(*rm.sphere(), 0.05)
    v, t = v.astype(np.float32), t.astype(np.int32)
    assert rm.signed_volume(v, t) > 0
    M = cases.camera((3.0, 0.5, 1.0), target=(0.8131, 0.7877, 0.8023))
    r = truth.rasterize(v, t, M, 64, 48)
    owners = np.unique(r["triangle_id"][r["triangle_id"] >= 0])
    swapped = truth.setup(v, t, M, 64, 48, 0.01, 0)[5]
    assert len(owners) > 300 and swapped[owners].all()                                       # area2 < 0
    assert np.array_equal(truth.rasterize(v, t, M, 64, 48, cull_sign=-1)["triangle_id"], r["triangle_id"])
    import gsrast.mesh
    assert "-1 is the OUTSIDE" in gsrast.mesh.rasterize_mesh.__doc__


def test_the_truths_cull_keeps_order_and_drops_unreferenced_vertices():
    k = cases.CASES["sphere_33x31"]
    counts = cases.truth_counts("sphere_33x31")
    for m in (1, 2):
        v, c, t = truth.cull(k["v"], k["c"], k["t"], counts, m)
        assert len(t) == (counts >= m).sum() and len(np.unique(t)) == len(v) and np.array_equal(v[t], k["v"][k["t"][counts >= m]])


class _HostMesh:
    def __init__(self, v, c, t):
        self.vertices, self.vertex_colors, self.triangles = v, c, t


def test_the_new_functions_are_exported():
    import gsrast
    from gsrast.tsdf import TriangleMesh
    for name in ("rasterize_mesh", "triangle_view_counts", "cull_unseen_triangles", "MeshRaster"):
        assert getattr(gsrast, name) is getattr(gsrast.mesh, name)
    assert callable(TriangleMesh.rasterize) and callable(TriangleMesh.cull_unseen_triangles)
    assert "gsr_mesh_rasterize" in gsrast.EXPORTS and "gsr_mesh_raster_scratch_bytes" in gsrast.EXPORTS and gsrast.ABI_VERSION == 8


def test_argument_checks_run_before_the_library_is_touched(monkeypatch):
    import gsrast
    monkeypatch.setattr(gsrast.mesh, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    k = cases.CASES["whole_image"]
    host = _HostMesh(torch.from_numpy(k["v"]), torch.from_numpy(k["c"]), torch.from_numpy(k["t"]))
    M = torch.from_numpy(k["mats"])
    fs = (gsrast.rasterize_mesh, gsrast.triangle_view_counts, gsrast.cull_unseen_triangles)
    for f in fs:
        for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(height=2.5), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(cull_sign=2),
                   dict(cull_sign=-2), dict(cull_sign=0.5)):
            args = dict(width=32, height=32)
            args.update(kw)
            with pytest.raises(ValueError, match=next(iter(kw))):
                f(host, M, **args)
        with pytest.raises(RuntimeError, match="CUDA tensor"):                               # the values are fine: the host mesh is what is wrong
            f(host, M, 32, 32)
    for f in fs[1:]:
        for tol in (-1e-3, float("nan")):
            with pytest.raises(ValueError, match="depth_tolerance"):
                f(host, M, 32, 32, depth_tolerance=tol)
    for m in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_views"):
            gsrast.cull_unseen_triangles(host, M, 32, 32, min_views=m)
    from gsrast.tsdf import TriangleMesh
    mesh = TriangleMesh(host.vertices, host.vertex_colors, host.triangles)
    with pytest.raises(ValueError, match="width"):
        mesh.rasterize(M, 0, 32)
    with pytest.raises(ValueError, match="min_views"):
        mesh.cull_unseen_triangles(M, 32, 32, min_views=0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh.rasterize(M, 32, 32)


def test_the_matrix_checks(monkeypatch):
    """The mesh is checked first and a host mesh raises, so the matrix checks are reached through the checker itself with the mesh check stubbed."""
    import gsrast
    monkeypatch.setattr(gsrast.mesh, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    k = cases.CASES["whole_image"]
    t = torch.from_numpy(k["t"])
    monkeypatch.setattr(gsrast.mesh, "_arrays", lambda mesh: (torch.from_numpy(k["v"]), torch.from_numpy(k["c"]), t))
    for bad, words in ((k["mats"], "must be a tensor"), (torch.from_numpy(k["mats"]), "CUDA tensor")):
        with pytest.raises(RuntimeError, match=words):
            gsrast.rasterize_mesh(None, bad, 32, 32)
