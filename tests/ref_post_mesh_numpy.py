"""The mesh filter's definition restated on the CPU (include/gsrast.h, gsr_mesh_*): the four Open3D calls of the reference's post_process_mesh
(gssr/utils/mesh_utils.py:28-48) with numpy and scipy.  Open3D is not part of the reference tree, so this is a restatement of its published
semantics (0.18), not a recording of its results."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

FLOOR = 50


def edge_keys(triangles):
    """[T,3] -> int64 [T,3]: the undirected edges (i0,i1), (i1,i2), (i2,i0) as min << 32 | max."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b = t, np.roll(t, -1, axis=1)
    return (np.minimum(a, b) << 32) | np.maximum(a, b)


def cluster_connected_triangles(triangles, vertices=None):
    """-> (triangle_clusters int32 [T], cluster_n_triangles int32 [C], cluster_area float64 [C] or None).  Adjacent = sharing an edge key;
    clusters numbered by their first triangle."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(t)
    if T == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), (np.zeros(0, np.float64) if vertices is not None else None)
    keys = edge_keys(t).reshape(-1)
    tri = np.repeat(np.arange(T, dtype=np.int64), 3)
    order = np.argsort(keys, kind="stable")
    ks, ts = keys[order], tri[order]
    first = np.r_[True, ks[1:] != ks[:-1]]                       # the first half-edge of every run of equal keys
    head = ts[np.flatnonzero(first)[np.cumsum(first) - 1]]       # ... and its triangle, for every half-edge of the run
    g = coo_matrix((np.ones(len(ts), np.int8), (ts, head)), shape=(T, T))
    n, lab = connected_components(g, directed=False)
    lowest = np.full(n, T, np.int64)
    np.minimum.at(lowest, lab, np.arange(T))
    new = np.empty(n, np.int64)
    new[np.argsort(lowest)] = np.arange(n)
    clusters = new[lab]
    counts = np.bincount(clusters, minlength=n)
    area = None
    if vertices is not None:
        area = np.zeros(n, np.float64)
        np.add.at(area, clusters, triangle_areas(vertices, t))
    return clusters.astype(np.int32), counts.astype(np.int32), area


def triangle_areas(vertices, triangles):
    v = np.asarray(vertices, np.float32).astype(np.float64)[np.asarray(triangles, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def remove_triangles_by_mask(triangles, mask):
    return np.asarray(triangles)[~np.asarray(mask, bool)]


def remove_unreferenced_vertices(vertices, colors, triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    used = np.zeros(len(vertices), bool)
    used[t.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return vertices[used], colors[used], new[t].astype(np.int32).reshape(-1, 3)


def remove_degenerate_triangles(triangles):
    t = np.asarray(triangles).reshape(-1, 3)
    return t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]


def threshold(cluster_n_triangles, cluster_to_keep):
    if cluster_to_keep < 1:
        raise ValueError(f"cluster_to_keep must be a positive integer but found {cluster_to_keep}")
    n_cluster = np.sort(np.asarray(cluster_n_triangles).copy())[-cluster_to_keep]        # IndexError beyond the number of clusters
    return max(int(n_cluster), FLOOR)


def post_process_mesh(vertices, colors, triangles, cluster_to_keep=1000):
    """-> (vertices, colors, triangles, after_step_3): the four steps in the reference's order; after_step_3 = the arrays before the
    degenerate triangles go (what the hand-written cases look at)."""
    vertices, colors = np.asarray(vertices, np.float32), np.asarray(colors, np.float32)
    triangles = np.asarray(triangles, np.int32).reshape(-1, 3)
    clusters, counts, _ = cluster_connected_triangles(triangles)
    thr = threshold(counts, cluster_to_keep)
    t = remove_triangles_by_mask(triangles, counts[clusters] < thr)
    v, c, t = remove_unreferenced_vertices(vertices, colors, t)
    step3 = (v, c, t)
    return v, c, remove_degenerate_triangles(t), step3
