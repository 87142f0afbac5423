"""Named inputs for the tests of the mesh rasterizer: CASES[name] = dict(v float32 [V,3], c float32 [V,3], t int32 [T,3], mats float32 [n,4,4],
W, H, near, cull_sign).  Every case is small -- 6400 triangles and 128 x 96 at most, the one with 1030 views 12 triangles at 16 x 12 -- and the truths (tests/raster_truth.py) are computed once per
case and shared (truth()), their arrays read-only.

Two kinds of matrices:
  camera()    a look-at camera in the reference's convention (+z forward, y down in the image, row vectors: clip = [x y z 1] @ M, w = camera z)
  PIX         c_0 = x, c_1 = y, w = z: a vertex (ndc_x w, ndc_y w, w) lands at a chosen pixel position and depth; pix() makes such vertices
  ortho(W, H) w = 1 and px = x, py = y for dyadic x, y: pixel-exact"""
import functools

import numpy as np

import raster_truth as truth

F = np.float32


def _colors(n, seed):
    return np.random.default_rng(3000 + seed).uniform(0.0, 1.0, (n, 3)).astype(F)


def camera(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov_x=0.9, aspect=4.0 / 3.0, znear=0.01, zfar=100.0):
    """full_proj_transform [4,4] float32 of a pinhole camera at `eye` looking at `target`: x right, y down, z forward."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                               # world -> camera
    view = np.eye(4)
    view[:3, :3], view[3, :3] = R.T, -R @ eye
    tx = np.tan(fov_x / 2)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1], proj[2, 2], proj[2, 3], proj[3, 2] = 1 / tx, aspect / tx, zfar / (zfar - znear), 1.0, -zfar * znear / (zfar - znear)
    return (view @ proj).astype(F)


PIX = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], F)


def ortho(W, H):
    M = np.zeros((4, 4), F)
    M[0, 0], M[3, 0], M[1, 1], M[3, 1], M[3, 3] = 2.0 / W, 1.0 / W - 1.0, 2.0 / H, 1.0 / H - 1.0, 1.0
    return M


def pix(px, py, w, W, H):
    """The PIX vertex that lands at (px, py) with depth w (exactly where the products are exact in float32)."""
    nx, ny = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0
    return [F(nx * w), F(ny * w), F(w)]


def uv_sphere(rings, segs, radius=1.0, centre=(0.0, 0.0, 0.0), inward=False):
    """2 * rings * segs triangles, counter-clockwise seen from outside (the normals (v1 - v0) x (v2 - v0) point outwards) unless `inward`."""
    th, ph = np.meshgrid(np.pi * (np.arange(rings) + 1) / (rings + 1), 2 * np.pi * np.arange(segs) / segs, indexing="ij")
    body = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1).reshape(-1, 3)
    v = np.concatenate([body, [(0, 0, 1), (0, 0, -1)]]) * radius + np.asarray(centre)
    north, south, t = len(body), len(body) + 1, []
    for i in range(rings - 1):
        for j in range(segs):
            a, b, c, d = i * segs + j, i * segs + (j + 1) % segs, (i + 1) * segs + j, (i + 1) * segs + (j + 1) % segs
            t += [(a, c, b), (b, c, d)]
    t += [(north, j, (j + 1) % segs) for j in range(segs)] + [(south, (rings - 1) * segs + (j + 1) % segs, (rings - 1) * segs + j) for j in range(segs)]
    t = np.array(t, np.int32)
    return v.astype(F), (t[:, [0, 2, 1]] if inward else t)


def ring(n, radius=3.0, height=0.8, **kw):
    """n cameras around the origin."""
    return np.stack([camera((radius * np.cos(2 * np.pi * k / n + 0.3), radius * np.sin(2 * np.pi * k / n + 0.3), height * (1 if k % 2 else -1)), **kw)
                     for k in range(n)])


def all_around(radius=3.0, **kw):
    """Fourteen cameras: the six axes and the eight corners."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0.02, 0.01, 1), (0.01, 0.02, -1)] + [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    return np.stack([camera(radius * np.asarray(d, np.float64) / np.linalg.norm(d), **kw) for d in dirs])


def _case(v, t, mats, W, H, near=0.01, cull_sign=0, seed=0):
    v = np.ascontiguousarray(v, dtype=F).reshape(-1, 3)
    mats = np.ascontiguousarray(mats, dtype=F).reshape(-1, 4, 4)
    return dict(v=v, c=_colors(len(v), seed), t=np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3), mats=mats, W=W, H=H, near=near, cull_sign=cull_sign)


def lattice(flip):
    """8 x 8 vertices at the pixel centres (4 i, 4 j): 98 triangles whose edges and diagonals run through centres."""
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    v = np.stack([4.0 * i.ravel(), 4.0 * j.ravel(), np.zeros(64)], axis=1)
    t = []
    for a in range(7):
        for b in range(7):
            p, q, r, s = a * 8 + b, (a + 1) * 8 + b, a * 8 + b + 1, (a + 1) * 8 + b + 1
            t += [(p, q, s), (p, s, r)]
    t = np.array(t, np.int32)
    return _case(v, t[:, [0, 2, 1]] if flip else t, ortho(32, 32), 32, 32, seed=1)


def _pix_case(tris, W=32, H=32, near=0.01, cull_sign=0, seed=0):
    """tris: per triangle three (px, py, w)."""
    v = [pix(px, py, w, W, H) for tri in tris for px, py, w in tri]
    return _case(v, np.arange(3 * len(tris)).reshape(-1, 3), PIX, W, H, near, cull_sign, seed)


NEAR = 0.5
JUST_ABOVE_NEAR = float(np.nextafter(F(NEAR), F(1)))
GUARD_PX, GUARD_PX_OUT = 65536.0, 65536.0 + 1.0 / 256.0       # X = 2^24 and 2^24 + 1, both exact in float32 at W = 32, w = 1


def _all():
    sph = {400: uv_sphere(10, 20), 1024: uv_sphere(16, 32), 6400: uv_sphere(40, 80)}
    c = {}
    c["ortho_lattice"], c["ortho_lattice_flipped"] = lattice(False), lattice(True)
    c["sphere_33x31"] = _case(*sph[400], ring(8), 33, 31, seed=2)
    c["sphere_33x31_cull_pos"] = _case(*sph[400], ring(8)[:2], 33, 31, cull_sign=1, seed=2)
    c["sphere_33x31_cull_neg"] = _case(*sph[400], ring(8)[:2], 33, 31, cull_sign=-1, seed=2)
    c["sphere_64x48"] = _case(*sph[1024], ring(3), 64, 48, seed=3)
    c["sphere_128x96"] = _case(*sph[6400], ring(3, radius=4.5), 128, 96, seed=4)
    c["image_17x15"] = _case(*sph[400], ring(2, radius=2.6), 17, 15, seed=5)
    c["sliver"] = _pix_case([[(2.25, 2.25, 1), (6.75, 3.75, 1), (6.8, 3.8, 1)]])
    c["offscreen"] = _pix_case([[(-9, 3, 1), (-2, 5, 1), (-5, 20, 1)], [(33, 3, 1), (40, 5, 1), (35, 20, 1)],
                                [(3, -9, 1), (5, -2, 1), (20, -5, 1)], [(3, 33, 1), (5, 40, 1), (20, 35, 1)]])
    c["straddle"] = _pix_case([[(-4, 3.5, 1), (5, 6, 2), (-3, 12, 1)], [(36, 14, 1), (27.5, 16, 2), (35, 25, 1)],
                               [(10, -4, 1), (19, -3, 2), (14, 5.5, 1)], [(10, 36, 1), (14, 27.25, 2), (20, 35, 1)]])
    c["whole_image"] = _pix_case([[(-10, -10, 1), (100, -10, 2), (-10, 100, 3)]])
    c["guard_inside"] = _pix_case([[(3, 3, 1), (GUARD_PX, 9, 1), (3, 20, 1)]])
    c["guard_outside"] = _pix_case([[(3, 3, 1), (GUARD_PX_OUT, 9, 1), (3, 20, 1)], [(3, 3, 2), (20, 9, 2), (3, 20, 2)]])
    c["near_exact"] = _pix_case([[(3, 3, NEAR), (20, 9, 1), (3, 20, 1)], [(3, 3, 2), (20, 9, 2), (3, 20, 2)]], near=NEAR)
    c["near_above"] = _pix_case([[(3, 3, JUST_ABOVE_NEAR), (20, 9, 1), (3, 20, 1)], [(3, 3, 2), (20, 9, 2), (3, 20, 2)]], near=NEAR)
    c["behind"] = _pix_case([[(3, 3, -1), (20, 9, -1), (3, 20, -2)], [(3, 3, 2), (20, 9, 2), (3, 20, 2)]])
    c["duplicate"] = _pix_case([[(3, 3, 1), (20, 9, 2), (3, 20, 1.5)]] * 2)
    c["crossing"] = _pix_case([[(2, 2, 1), (29, 4, 3), (3, 28, 1)], [(2, 3, 3), (29, 2, 1), (27, 29, 1)]])
    zero = _pix_case([[(3, 3, 1), (20, 9, 1), (3, 20, 1)], [(4, 4, 1), (8, 8, 1), (16, 16, 1)], [(1, 1, 1), (2, 9, 1), (9, 2, 1)]])
    zero["t"][0] = (0, 0, 1)                              # equal indices; triangle 1 is collinear; triangle 2 is an ordinary one
    c["zero_area"] = zero
    c["no_triangles"] = _case(sph[400][0][:3], np.zeros((0, 3), np.int32), ring(2), 16, 12)
    c["no_views"] = _case(*sph[400], np.zeros((0, 4, 4), F), 16, 12)
    return c


CASES = _all()                                            # box_1030_views joins below, NAMES follows it
SPHERES = ("sphere_33x31", "sphere_64x48", "sphere_128x96")
TOLERANCE = 0.05                                          # depth_tolerance of the visibility tests, in the units of the spheres (radius 1)


def errors():
    """name -> (case, kind): the two status errors."""
    bad_v = dict(CASES["sphere_33x31"]); bad_v["v"] = bad_v["v"].copy(); bad_v["v"][7, 1] = np.nan
    inf_v = dict(CASES["sphere_33x31"]); inf_v["v"] = inf_v["v"].copy(); inf_v["v"][0, 2] = np.inf
    hi = dict(CASES["sphere_33x31"]); hi["t"] = hi["t"].copy(); hi["t"][5, 2] = len(hi["v"])
    neg = dict(CASES["sphere_33x31"]); neg["t"] = neg["t"].copy(); neg["t"][0, 0] = -1
    return {"nan": (bad_v, "nonfinite"), "inf": (inf_v, "nonfinite"), "index_V": (hi, "index"), "index_negative": (neg, "index")}


def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for a in x.values():
            _frozen(a)
    elif isinstance(x, (list, tuple)):
        for a in x:
            _frozen(a)
    return x


@functools.lru_cache(maxsize=None)
def truth_views(name):
    """The truth's rasterize() of every view of the case."""
    k = CASES[name]
    return _frozen([truth.rasterize(k["v"], k["t"], M, k["W"], k["H"], k["near"], k["cull_sign"]) for M in k["mats"]])


def truth_maps(name):
    """-> depth [n,H,W], triangle_id [n,H,W], barycentric [n,H,W,2], dropped [n,3]"""
    k, r = CASES[name], truth_views(name)
    n, H, W = len(r), k["H"], k["W"]
    st = lambda key, shape, dt: np.stack([x[key] for x in r]) if n else np.zeros((0,) + shape, dt)
    return st("depth", (H, W), F), st("triangle_id", (H, W), np.int32), st("barycentric", (H, W, 2), F), st("dropped", (3,), np.int32)


@functools.lru_cache(maxsize=None)
def truth_counts(name, depth_tolerance=None):
    k = CASES[name]
    return _frozen(truth.view_counts(k["v"], k["t"], k["mats"], k["W"], k["H"], k["near"], k["cull_sign"], depth_tolerance, views=truth_views(name)))


def named_triangle(name):
    """(view, triangle, b): the triangle with the largest candidate box of the case's first view and the exact pixel count b of that box."""
    box = truth_views(name)[0]["box"]
    t = int(np.argmax(box))
    return 0, t, int(box[t])


@functools.lru_cache(maxsize=None)
def nested_spheres():
    """An outer sphere (radius 1, 1024 triangles) with an inner one (radius 0.5, the next 1024) no camera outside can see, fourteen views all around."""
    v0, t0 = uv_sphere(16, 32)
    v1, t1 = uv_sphere(16, 32, radius=0.5)
    return _frozen(_case(np.concatenate([v0, v1]), np.concatenate([t0, t1 + len(v0)]), all_around(), 64, 48, seed=9))


def closed_box():
    """A unit cube centred at the origin, 12 triangles counter-clockwise from outside, and six cameras on the axes, outside."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]       # -x +x -y +y -z +z
    t = np.array([q for a, b, c, d in quads for q in ((a, b, c), (a, c, d))], np.int32)
    normals = np.repeat(np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float64), 2, axis=0)
    eyes = np.array([(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0.01, 0.02, 3), (0.02, 0.01, -3)], np.float64)
    return _case(v, t, np.stack([camera(e) for e in eyes]), 48, 36), normals, eyes


# The box from 1030 cameras around it at 16 x 12: more views than one chunk of the rasterizer takes (MANY_VIEWS > CHUNK_MAX, csrc/gsr_mesh_raster.hip
# RS_CHUNK_MAX; test_raster_cpu holds the chunk rule), so the views from 1024 on go through a second turn of its loop.
CHUNK_MAX, MANY_VIEWS = 1024, 1030
CASES["box_1030_views"] = _case(closed_box()[0]["v"], closed_box()[0]["t"], ring(MANY_VIEWS), 16, 12, seed=6)
NAMES = sorted(CASES)
