"""Named inputs for the tests of the mesh smoothing filters, the normals and the vertex adjacency: CASES[name] = (vertices float32 [V,3], colors
float32 [V,3], triangles int32 [T,3]).  Every case is small: the largest, strip_z_65536, carries 52 000 vertices, and the fans stay at two
iterations (iterations()) because one thread walks the hub's list.  Degrees stay at 64 or below outside the fans, which is what the bars of
tests/test_gpu_smooth.py are derived for.  The truths are computed once and shared (truth_*), their arrays are read-only."""
import functools

import numpy as np

import simplify_cases
from simplify_cases import grid_triangles

FILTERS = ("simple", "laplacian", "taubin")
SCOPES = ("all", "vertex")
LAMBDA, MU = 0.5, -0.53


def _colors(n, seed):
    return np.random.default_rng(2000 + seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def _pack(v, t, seed=0):
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    return v, _colors(len(v), seed), np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)


def torus_points(nu=32, nv=16, R=1.0, r=0.4):
    u, w = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    n = np.stack([np.cos(w) * np.cos(u), np.cos(w) * np.sin(u), np.sin(w)], axis=-1).reshape(-1, 3)       # the analytic outward normal
    return v, n


def torus(noise=0.0):
    """32 x 16 quads, R = 1, r = 0.4, welded both ways: every degree is 6.  grid_triangles winds them so that the normals point outwards."""
    v, _ = torus_points()
    if noise:
        v = v + np.random.default_rng(7).normal(0.0, noise, v.shape)
    return _pack(v, grid_triangles(32, 16, wrap_u=True, wrap_v=True), 1)


def sphere():
    """A UV sphere with poles, 12 rings x 24 segments: the poles have degree 24."""
    th, ph = np.meshgrid(np.pi * (np.arange(12) + 1) / 13, 2 * np.pi * np.arange(24) / 24, indexing="ij")
    body = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1).reshape(-1, 3)
    v = np.concatenate([body, [(0, 0, 1), (0, 0, -1)]])
    north, south = len(body), len(body) + 1
    caps = [(north, j, (j + 1) % 24) for j in range(24)] + [(south, 11 * 24 + (j + 1) % 24, 11 * 24 + j) for j in range(24)]
    return _pack(v, np.concatenate([grid_triangles(12, 24, wrap_v=True), np.array(caps, dtype=np.int32)]), 2)


def sheet(n=17, shift=0.0, detail=0.0, seed=3):
    """A planar regular n x n grid with a boundary, spacing 1/8 (dyadic); `detail`: noise of that size on every coordinate."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i.ravel() * 0.125, j.ravel() * 0.125, np.zeros(n * n)], axis=1) + shift
    if detail:
        v = v + np.random.default_rng(seed).uniform(-detail, detail, v.shape)
    return _pack(v, grid_triangles(n, n), seed)


def soup(V, seed):
    """V random vertices in a cube and 2 V random index triples: degenerate triangles, equal triples and unreferenced vertices all occur; the mean
    degree is about 12."""
    r = np.random.default_rng(seed)
    return _pack(r.uniform(-2.0, 2.0, (V, 3)), r.integers(0, V, (2 * V, 3)), seed)


def fan(spokes, closed, hub=7):
    """One hub (vertex `hub`) and `spokes` rim vertices on a wavy circle.  closed: triangle k = (hub, rim k, rim k + 1), around: every rim edge is
    shared with the hub only once, the rim is a cycle.  Open: spokes // 2 separate triangles (hub, rim 2k, rim 2k + 1) that share no rim edge, and
    for an odd count one more on the last and the first rim vertex."""
    a = 2 * np.pi * np.arange(spokes) / spokes
    rim = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(5 * a)], axis=1)
    v = np.insert(rim, hub, (0.0, 0.0, 0.3), axis=0)
    ids = np.array([k if k < hub else k + 1 for k in range(spokes)])
    if closed:
        t = [(hub, ids[k], ids[(k + 1) % spokes]) for k in range(spokes)]
    else:
        t = [(hub, ids[2 * k], ids[2 * k + 1]) for k in range(spokes // 2)] + ([(hub, ids[spokes - 1], ids[0])] if spokes % 2 else [])
    return _pack(v, t, spokes + closed)


def duplicates():
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5), (2, 0.5, 0.25)]
    return _pack(v, [(0, 1, 2)] * 8 + [(0, 2, 1)] + [(1, 3, 2), (1, 4, 3)], 4)


def degenerate():
    """(a, a, b), (a, a, a), a zero-area triangle with three distinct indices (collinear points), and two ordinary triangles."""
    v = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 1), (3, 3, 3), (0.5, 0.5, 2)]
    return _pack(v, [(0, 0, 3), (5, 5, 5), (0, 1, 2), (0, 1, 3), (1, 4, 3), (6, 6, 4)], 5)


def cancelling():
    """Two mirrored triangles on one vertex set: every vertex normal sums to zero and falls back to (0, 0, 1)."""
    return _pack([(0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], [(0, 1, 2), (0, 2, 1)], 6)


def isolated():
    """A 6 x 6 sheet with unreferenced vertices in front of it, inside it and behind it."""
    i, j = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    body = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, 0.2 * np.cos(i.ravel() * 1.0 + j.ravel())], axis=1)
    v = np.concatenate([[(9, 9, 9)], body[:20], [(7, 7, 7), (-3, 2, 1)], body[20:], [(5, 5, 5)]])
    t = grid_triangles(6, 6).astype(np.int64)
    t = np.where(t < 20, t + 1, t + 3)
    return _pack(v, t, 7)


@functools.lru_cache(maxsize=None)
def _all():
    cube_v, _, cube_t, _ = simplify_cases.cube()
    strip_v, _, strip_t, _ = simplify_cases.CASES["strip_z_65536"]
    c = {"alone": _pack([(0, 0, 0), (1, 0, 0), (0, 1, 0.5)], [(0, 1, 2)], 10),
         "no_triangles": _pack(np.random.default_rng(30).uniform(0, 3, (5, 3)), np.zeros((0, 3)), 11),
         "empty": _pack(np.zeros((0, 3)), np.zeros((0, 3)), 12),
         "cube": _pack(cube_v, cube_t, 13), "sphere": sphere(), "torus": torus(), "torus_noisy": torus(0.01),
         "sheet_17x17": sheet(), "strip_z_65536": _pack(strip_v, strip_t, 14),
         "fan_1025": fan(1025, False), "fan_1025_closed": fan(1025, True), "fan_5000": fan(5000, False), "fan_5000_closed": fan(5000, True),
         "duplicates": duplicates(), "degenerate": degenerate(), "cancelling": cancelling(), "isolated": isolated(),
         "far_from_origin": sheet(9, shift=1.0e4, detail=1.0e-3, seed=15)}
    for n in (255, 256, 257, 1025):
        c[f"size_V{n}"] = soup(n, 100 + n)
    return c


CASES = _all()
NAMES = sorted(CASES)
SMALL = [n for n in NAMES if len(CASES[n][0]) <= 600 and not n.startswith("fan")]      # the dense-matrix formulation is run on these


def iterations(name):
    """The iteration counts a case is smoothed with: 1 and 10, the fans 1 and 2."""
    return (1, 2) if name.startswith("fan") else (1, 10)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def truth_adjacency(name):
    import smooth_truth
    v, _, t = CASES[name]
    return _frozen(*smooth_truth.adjacency(t, len(v)))


@functools.lru_cache(maxsize=None)
def truth_normals(name, which, normalized):
    import smooth_truth
    v, _, t = CASES[name]
    return _frozen((smooth_truth.triangle_normals if which == "triangle" else smooth_truth.vertex_normals)(v, t, normalized))


@functools.lru_cache(maxsize=None)
def truth_smooth(name, kind, n, scope):
    import smooth_truth
    v, c, t = CASES[name]
    return _frozen(*smooth_truth.smooth(v, c, t, kind, n, LAMBDA, MU, scope))


def errors():
    """name -> (vertices, colors, triangles, the status bit: "index" or "nonfinite")."""
    v, c, t = CASES["sheet_17x17"]
    nan, inf, neg, past = v.copy(), v.copy(), t.copy(), t.copy()
    nan[17, 1] = np.nan
    inf[40, 2] = -np.inf
    neg[0, 0] = -1
    past[7, 2] = len(v)
    return {"nan": (nan, c, t, "nonfinite"), "inf": (inf, c, t, "nonfinite"), "index_negative": (v, c, neg, "index"), "index_V": (v, c, past, "index")}
