"""Named inputs of the registration tests (numpy only): the sheet two clouds are sampled from, rigid and similarity motions, the ICP cases with
their thresholds and stated outcomes, the point pairs of the solve cases, the polygons and probe points of the crop.  tests/test_register_cpu.py
asserts the structure each case is named for; tests/test_gpu_register.py runs them on the device."""
import functools

import numpy as np

F = np.float32
SIZES = (0, 1, 63, 64, 65, 257)                           # transform_points
SUM_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2049)
SUM_BLOCKS, SUM_PER_BLOCK = 1024, 1024                    # RG_BLOCKS, RG_PER_BLOCK of csrc/gsr_register.hip: the grid of blocks stops growing at their product
SUM_PAST_GRID = SUM_BLOCKS * SUM_PER_BLOCK + 257


def height(x, y):
    return 0.25 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * x * y + 0.1 * x * x


def sheet(n, seed):
    """n float32 points of a height field over [-1,1]^2, neither flat nor symmetric: a registration has one answer."""
    xy = np.random.default_rng(seed).uniform(-1, 1, (n, 2))
    return np.stack([xy[:, 0], xy[:, 1], height(xy[:, 0], xy[:, 1])], 1).astype(F)


def rigid(axis, degrees, t, scale=1.0):
    """float64 [4,4], column-vector convention: a turn of `degrees` about `axis` (Rodrigues), times scale, then the move t."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = scale * (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    M[:3, 3] = t
    return M


def move(points, M):
    """points through M in float64, rounded to float32: for building inputs."""
    p = points.astype(np.float64)
    return np.stack([((M[a, 0] * p[:, 0] + M[a, 1] * p[:, 1]) + M[a, 2] * p[:, 2]) + M[a, 3] for a in range(3)], 1).astype(F)


MOTION = rigid((1, 2, 3), 4.0, (0.03, -0.02, 0.01))
MOTION_SCALED = rigid((1, 2, 3), 4.0, (0.03, -0.02, 0.01), 1.1)


def _partial_overlap(seed=22):
    """3000 targets; sources: 1200 of their pre-images with x < 0.3, 60 floaters 0.5 off the sheet, 40 points 0.08 to 0.2 off it (they cross the cap
    as the fit moves).  The seed is one under which every convergence delta stays clear of its threshold (test_register_cpu)."""
    inv = np.linalg.inv(MOTION)
    target = sheet(3000, seed)
    pre = move(target, inv)[np.flatnonzero(target[:, 0] < 0.3)[:1200]]
    floaters = sheet(60, seed + 200); floaters[:, 2] += F(0.5)
    near = sheet(40, seed + 300); near[:, 2] += np.random.default_rng(seed + 100).uniform(0.08, 0.2, 40).astype(F)
    return np.concatenate([pre, move(floaters, inv), move(near, inv)]).astype(F), target


def _icp_cases():
    src = sheet(1500, 1)
    po_s, po_t = _partial_overlap()
    c = {}
    # name: source, target, cap, keyword arguments, and what the truth's trace has to show: iterations, converged, status
    c["exact_copy"] = dict(source=src, target=move(src, MOTION), cap=0.15, kw=dict(relative_rmse=1e-5), iterations=10, converged=True, status=0)
    c["partial_overlap"] = dict(source=po_s, target=po_t, cap=0.15, kw=dict(relative_fitness=1e-4, relative_rmse=1e-5, max_iteration=40), iterations=16,
                                converged=True, status=0)
    c["different_sampling"] = dict(source=sheet(1500, 6), target=move(sheet(2500, 7), MOTION), cap=0.15, kw=dict(max_iteration=12), iterations=12,
                                   converged=False, status=0)
    c["max_iteration_0"] = dict(source=src, target=move(src, MOTION), cap=0.15, kw=dict(max_iteration=0), iterations=0, converged=False, status=0)
    c["with_scaling"] = dict(source=src, target=move(src, MOTION_SCALED), cap=0.3, kw=dict(with_scaling=True, max_iteration=50), iterations=37, converged=True,
                             status=0)
    c["no_inliers"] = dict(source=src, target=move(src, MOTION) + F(100), cap=0.01, kw=dict(init=rigid((0, 0, 1), 10.0, (0.5, 0, 0))), iterations=0,
                           converged=False, status=2)
    for n in (1, 2, 3):
        for t in (1, 2, 3):
            both = n == 3 and t == 3                      # three pairs are a fit; fewer are degenerate
            c[f"N{n}_T{t}"] = dict(source=src[:n], target=move(src, MOTION)[:t], cap=0.5, kw=dict(relative_rmse=1e-5), iterations=2 if both else 0,
                                   converged=both, status=0 if both else 2)
    return c


ICP = _icp_cases()
# The bar of the device's ICP transformation against the truth's (tests/test_gpu_register.py): 8 x the largest element difference
# between truth.icp as it is and truth.icp with every sum of every iteration moved by a relative 1e-12, the bar the device's sums are held to.
# Measured over the four main cases: 7.4e-13, the partial-overlap case (test_the_transformation_bar_is_eight_times_what_the_sums_bar_moves prints it).
TRANSFORM_BAR = 6.0e-12


def _solve_cases():
    """name: (source, target, with_scaling).  Rows correspond."""
    r = np.random.default_rng(11)
    p = r.uniform(-1, 1, (40, 3)).astype(F)
    flat = p.copy(); flat[:, 2] = 0
    line = np.outer(np.linspace(-1, 1, 9), [1.0, 2.0, -0.5]).astype(F)
    half_turn = p * np.array([-1, -1, 1], F)              # 180 degrees about z, exactly: the quaternion has w = 0
    c = {
        "identity": (p, p.copy(), False),
        "general_rotation": (p, move(p, rigid((3, -1, 2), 67.0, (0.4, -1.2, 2.5))), False),
        "half_turn": (p, half_turn, False),
        "coplanar": (flat, move(flat, rigid((1, 1, 0), 30.0, (0, 0.2, 0))), False),
        "reflection": (p, p * np.array([-1, 1, 1], F), False),              # a mirror image: the SVD's least-squares orthogonal matrix has det -1
        "scale_half": (p, move(p, rigid((0, 1, 1), 20.0, (1, 2, 3), 0.5)), True),
        "scale_three": (p, move(p, rigid((0, 1, 1), 20.0, (1, 2, 3), 3.0)), True),
        "n_2": (p[:2], p[:2] + F(1), False),
        "sources_equal": (np.tile(p[:1], (5, 1)), p[:5], False),
        "targets_equal": (p[:5], np.tile(p[:1], (5, 1)), False),
        "collinear": (line, move(line, rigid((0, 0, 1), 25.0, (0.1, 0, 0))), False),
    }
    return c


SOLVE = _solve_cases()
SOLVE_DEGENERATE = ("n_2", "sources_equal", "targets_equal")
_P = np.random.default_rng(11).uniform(-1, 1, (40, 3)).astype(F)
OFFSET_1E4 = (_P + F(1e4), move(_P, rigid((1, 0, 2), 12.0, (0, 0, 0))) + F(1e4))        # an extent of 2 at 1e4: the raw moments are 1e8 a term, the centred ones 1


def a3(rows):
    return np.asarray(rows, F).reshape(-1, 3)


NONFINITE_ROWS = a3([[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf], [np.inf, -np.inf, 0], [3e38, 3e38, 3e38], [1, 2, 3]])
TRANSFORMS = {"motion": MOTION, "scale_half": rigid((2, 0, 1), 33.0, (1, -2, 0.5), 0.5), "scale_three": rigid((2, 0, 1), 33.0, (1, -2, 0.5), 3.0)}


# ---------------------------------------------------------------------------------------------------------------- crop
def star(K, r_out=1.0, r_in=0.45, centre=(0.1, -0.2)):
    """K vertices alternating between two radii: concave for K >= 6, a triangle or a kite below."""
    ang = 2 * np.pi * np.arange(K) / K + 0.1
    rad = np.where(np.arange(K) % 2 == 0, r_out, r_in) if K >= 6 else np.full(K, r_out)
    return np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], 1)


SQUARE = np.array([[-0.5, -0.5], [0.75, -0.5], [0.75, 0.5], [-0.5, 0.5]])      # convex, its coordinates are float32 numbers
ELL = np.array([[-1, -1], [1, -1], [1, 0], [0, 0], [0, 1], [-1, 1]], np.float64)      # concave
POLYGONS = {"square": SQUARE, "ell": ELL, "K3": star(3), "K4": star(4), "K64": star(64), "K65": star(65), "K1024": star(1024)}


def crop_points(polygon, axis, lo, hi, n=257, seed=5):
    """n float32 points: random ones about the polygon and the slab, then points exactly on a vertex's v (left and right of it), on a vertex, in the
    middle of an edge, on axis_min and axis_max and one ulp outside them, and non-finite ones.  Columns are (u, v, w) moved to their axes."""
    r = np.random.default_rng(seed)
    P = np.asarray(polygon, np.float64)
    pts = np.stack([r.uniform(-1.3, 1.3, n), r.uniform(-1.3, 1.3, n), r.uniform(lo - 0.2, hi + 0.2, n)], 1).astype(F)
    mid = 0.5 * (lo + hi)
    special = []
    for k in range(min(len(P), 6)):
        u, v = P[k]
        special += [[u - 0.25, v, mid], [u + 0.25, v, mid], [u, v, mid], [0.5 * (u + P[k - 1][0]), 0.5 * (v + P[k - 1][1]), mid]]
    special += [[0.1, -0.2, lo], [0.1, -0.2, hi], [0.1, -0.2, np.nextafter(F(lo), F(-np.inf))], [0.1, -0.2, np.nextafter(F(hi), F(np.inf))]]
    special += [[np.nan, 0, mid], [0, np.inf, mid], [0.1, -0.2, np.nan], [-np.inf, 0, mid]]
    k = min(len(special), n)
    if n:
        pts[n - k:] = np.asarray(special, F)[:k]
    ax = "XYZ".index(axis)
    iu, iv = [a for a in range(3) if a != ax]
    out = np.empty_like(pts)
    out[:, iu], out[:, iv], out[:, ax] = pts[:, 0], pts[:, 1], pts[:, 2]
    return out


@functools.lru_cache(maxsize=None)
def icp_truth(name, perturb=0.0):
    """register_truth.icp of a named case, computed once per process and shared by the tests that need it; callers leave it unchanged."""
    import register_truth
    c = ICP[name]
    return register_truth.icp(c["source"], c["target"], c["cap"], perturb=perturb, **c["kw"])
