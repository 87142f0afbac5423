"""numpy restatement of the mesh gsrast.tsdf.ScalableTSDFVolume.extract_triangle_mesh() defines (include/gsrast.h, gsr_tsdf_sparse_mesh_count) over
dense [nx,ny,nz] arrays: the same table (tools/gen_mc_table.py), the same float32 formulas, the same order -- units of 16^3 voxels in ascending
coordinate order, voxels x-major inside a unit, vertices by axis and triangles in table order inside a voxel.  Plus the mesh checks the tests share."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table  # noqa: E402

TABLE = np.array(gen_mc_table.table(), dtype=np.int64)                  # [256, 16]
EDGE_CORNER = np.array([a for a, _ in gen_mc_table.EDGES], dtype=np.int64)
EDGE_AXIS = np.array(gen_mc_table.EDGE_AXIS, dtype=np.int64)
CORNER_OFF = np.array(gen_mc_table.CORNERS, dtype=np.int64)             # [8, 3]


def _sh(a, d):
    """a[p + d] on the domain of voxels that have an upper neighbour (every axis one shorter than a), d in {0,1}^3."""
    n = a.shape
    return a[d[0]:n[0] - 1 + d[0], d[1]:n[1] - 1 + d[1], d[2]:n[2] - 1 + d[2]]


def _ordered(p, origin):
    """Rows of p (padded voxel indices [m,3]) in output order: by unit coordinate, then by the voxel's place in its unit."""
    G = p + np.asarray(origin, dtype=np.int64) - 1
    u, l = G >> 4, G & 15
    return p[np.lexsort((l[:, 2], l[:, 1], l[:, 0], u[:, 2], u[:, 1], u[:, 0]))]


def extract(tsdf, weight, color, voxel_length, origin=(0, 0, 0), min_weight=0.0):
    """tsdf, weight [nx,ny,nz], color [nx,ny,nz,3] (0..255); `origin`: global voxel index of element [0,0,0]; outside the arrays the weight is 0.
    -> (vertices [V,3] float32, colors [V,3] float32, triangles [T,3] int32)"""
    f32 = np.float32
    ok = np.pad(np.asarray(weight, f32) > f32(min_weight), 1)
    f = np.where(ok, np.pad(np.asarray(tsdf, f32), 1), f32(0))
    col = np.pad(np.asarray(color, f32), ((1, 1), (1, 1), (1, 1), (0, 0)))
    inside = f < 0
    cv = np.ones(tuple(n - 1 for n in f.shape), bool)
    case = np.zeros(cv.shape, np.int64)
    for i, d in enumerate(CORNER_OFF):
        cv &= _sh(ok, d)
        case |= _sh(inside, d).astype(np.int64) << i
    cvp = np.pad(cv, ((1, 0), (1, 0), (1, 0)))             # cvp[p + 1] = cv[p]; cubes with a negative origin do not exist
    edge = np.zeros(cv.shape + (3,), bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ea = np.eye(3, dtype=np.int64)
        around = np.zeros(cv.shape, bool)
        for sb in (0, 1):
            for sc in (0, 1):
                d = 1 - sb * ea[b] - sc * ea[c]
                around |= cvp[d[0]:d[0] + cv.shape[0], d[1]:d[1] + cv.shape[1], d[2]:d[2] + cv.shape[2]]
        edge[..., a] = (_sh(inside, (0, 0, 0)) != _sh(inside, ea[a])) & around
    # vertices
    pv = _ordered(np.argwhere(edge.any(axis=-1)), origin)
    ev = edge[pv[:, 0], pv[:, 1], pv[:, 2]]                 # [m, 3]
    vox, axis = np.nonzero(ev)                              # row-major: voxel order, then axis
    p0 = pv[vox]
    p1 = p0 + np.eye(3, dtype=np.int64)[axis]
    vid = np.full(cv.shape + (3,), -1, np.int64)
    vid[p0[:, 0], p0[:, 1], p0[:, 2], axis] = np.arange(len(vox))
    f0, f1 = f[p0[:, 0], p0[:, 1], p0[:, 2]], f[p1[:, 0], p1[:, 1], p1[:, 2]]
    with np.errstate(all="ignore"):
        t = (f0 / (f0 - f1)).astype(f32)
    G = (p0 + np.asarray(origin, dtype=np.int64) - 1).astype(f32)
    verts = f32(voxel_length) * (G + f32(0.5))
    along = f32(voxel_length) * ((G[np.arange(len(vox)), axis] + f32(0.5)) + t)
    verts[np.arange(len(vox)), axis] = along
    c0, c1 = col[p0[:, 0], p0[:, 1], p0[:, 2]], col[p1[:, 0], p1[:, 1], p1[:, 2]]
    colors = ((c0 + t[:, None] * (c1 - c0)) / f32(255.0)).astype(f32)
    # triangles
    ntri = np.where(cv, TABLE[case, 15], 0)
    pc = _ordered(np.argwhere(ntri > 0), origin)
    rows = TABLE[case[pc[:, 0], pc[:, 1], pc[:, 2]]]        # [m, 16]
    e = rows[:, :15].reshape(-1, 5, 3)
    keep = np.arange(5)[None, :] < rows[:, 15:16]
    e = np.where(keep[..., None], e, 0)
    q = pc[:, None, None, :] + CORNER_OFF[EDGE_CORNER[e]]   # [m, 5, 3, 3]
    tris = vid[q[..., 0], q[..., 1], q[..., 2], EDGE_AXIS[e]][keep]
    assert (tris >= 0).all(), "a triangle names an edge without a vertex"
    return verts.astype(f32), colors, tris.astype(np.int32).reshape(-1, 3)


def dense_from_units(coords, tsdf, weight, color):
    """Unit lists shaped like ScalableTSDFVolume.units() -> (tsdf, weight, color, origin) dense over the units' bounding box."""
    coords = np.asarray(coords, np.int64)
    lo, hi = coords.min(axis=0), coords.max(axis=0) + 1
    n = (hi - lo) * 16
    T, W, Cc = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(tuple(n) + (3,), np.float32)
    for k, c in enumerate(coords):
        s = tuple(slice(int(16 * (c[a] - lo[a])), int(16 * (c[a] - lo[a]) + 16)) for a in range(3))
        T[s], W[s], Cc[s] = tsdf[k], weight[k], color[k]
    return T, W, Cc, tuple(int(v) * 16 for v in lo)


def units_from_dense(tsdf, weight, color, origin_unit):
    """Dense arrays whose edges are multiples of 16 -> unit lists (coords [n,3] int32, tsdf / weight [n,16,16,16], color [n,16,16,16,3]), x-major."""
    nu = [s // 16 for s in tsdf.shape]
    co, T, W, Cc = [], [], [], []
    for ux in range(nu[0]):
        for uy in range(nu[1]):
            for uz in range(nu[2]):
                s = (slice(16 * ux, 16 * ux + 16), slice(16 * uy, 16 * uy + 16), slice(16 * uz, 16 * uz + 16))
                co.append([origin_unit[0] + ux, origin_unit[1] + uy, origin_unit[2] + uz]); T.append(tsdf[s]); W.append(weight[s]); Cc.append(color[s])
    return np.array(co, np.int32), np.stack(T), np.stack(W), np.stack(Cc)


def field_unit(rng):
    """One unit of a random field: tsdf in (-1, 1) with 1 % exact zeros, 10 % of the voxels without weight, random colours.  -> (tsdf, weight, color)"""
    f = rng.uniform(-1, 1, (16, 16, 16)).astype(np.float32)
    f[rng.uniform(size=(16, 16, 16)) < 0.01] = 0.0
    w = ((rng.uniform(size=(16, 16, 16)) > 0.1) * rng.integers(1, 9, (16, 16, 16))).astype(np.float32)
    return f, w, rng.uniform(0, 255, (16, 16, 16, 3)).astype(np.float32)


def row_units(fields, units):
    """Unit lists (coords, tsdf, weight, color) of the given units of a row along x: `fields` {unit: field_unit()}, every other unit the filler
    tsdf 0.5 at weight 1 -- present, live, without a surface of its own, but with one against a field unit beside it."""
    units = np.asarray(units, np.int64)
    n = len(units)
    T, W, Cc = np.full((n, 16, 16, 16), 0.5, np.float32), np.ones((n, 16, 16, 16), np.float32), np.zeros((n, 16, 16, 16, 3), np.float32)
    for k, u in enumerate(units.tolist()):
        if u in fields:
            T[k], W[k], Cc[k] = fields[u]
    co = np.zeros((n, 3), np.int32)
    co[:, 0] = units
    return co, T, W, Cc


def extract_row(fields, lo, hi, voxel_length):
    """extract() of units lo .. hi - 1 of the row alone, at their place."""
    T, W, Cc, org = dense_from_units(*row_units(fields, np.arange(lo, hi)))
    return extract(T, W, Cc, voxel_length, origin=org)


def concat(meshes):
    """Meshes that share no vertex, one after the other: the triangles of each offset by the vertices in front of it."""
    base = np.cumsum([0] + [len(m[0]) for m in meshes[:-1]])
    return (np.concatenate([m[0] for m in meshes]), np.concatenate([m[1] for m in meshes]),
            np.concatenate([m[2] + np.int32(b) for m, b in zip(meshes, base)]).astype(np.int32))


def topology(triangles, n_vertices):
    """-> dict(watertight, euler, unused): every directed edge has its opposite exactly once; V - E + F; vertices no triangle names."""
    t = np.asarray(triangles, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = d[:, 0] * (n_vertices + 1) + d[:, 1]
    rev = d[:, 1] * (n_vertices + 1) + d[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    watertight = bool((cnt == 1).all()) and np.array_equal(uk, np.unique(rev))
    und = np.unique(np.minimum(d[:, 0], d[:, 1]) * (n_vertices + 1) + np.maximum(d[:, 0], d[:, 1]))
    return dict(watertight=watertight, euler=int(n_vertices - len(und) + len(t)), unused=int(n_vertices - len(np.unique(t))))


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def sphere(n=32, h=0.05, centre=(0.8131, 0.7877, 0.8023), r=0.41):
    """The analytic sphere of the tests: tsdf = min(1, sdf / (5 h)) in float32 at the voxel centres h (i + 0.5), weights 1, a colour ramp."""
    g = (np.arange(n, dtype=np.float64) + 0.5) * h
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    sdf = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    tsdf = np.minimum(1.0, sdf / (5 * h)).astype(np.float32)
    color = np.stack([X, Y, Z], axis=-1) / (n * h) * 255.0
    return tsdf, np.ones_like(tsdf), color.astype(np.float32)
