"""A numpy float64 restatement of the reference's neighbour-view selection (view_selection / calc_score, gssr/utils/mvsnet_utils.py:306-343) in the
reference's own operation order, on the flat arrays gsrast.views.select_views takes.  tests/test_view_selection_cpu.py holds it to the fixtures the
reference itself produced, exactly; the GPU tests then use it as the truth at the sizes no fixture covers.

The reference's list search `[it for it in id_i if it in id_j]` is a set lookup here; what is summed, and in which order, is unchanged: the entries
of image i (the lower index) in their order and multiplicity, -1 skipped, every term through the same scalar numpy calls (np.dot, np.linalg.norm,
np.arccos, np.exp), so the sums agree to the last bit.

Ranking: the reference's np.argsort(score[i])[::-1] leaves the order of equal scores to an unstable sort.  `rank` applies the project's rule instead:
a stable ascending sort, reversed -- descending score, the higher index first among equal scores.  `margins` says how far a scene is from the cases in
which rounding could change a selection."""
import numpy as np


def images(obs_offsets, obs_ids):
    return [np.asarray(obs_ids[int(obs_offsets[a]):int(obs_offsets[a + 1])]) for a in range(len(obs_offsets) - 1)]


def term(ci, cj, p, theta0, sigma1, sigma2):
    """-> (g, theta): one term of calc_score, its operations one by one."""
    to_i, to_j = ci - p, cj - p                          # the two rays from the point
    cosine = np.dot(to_i, to_j) / np.linalg.norm(to_i)   # divided by one length, then by the other: the order decides the last bit
    cosine = cosine / np.linalg.norm(to_j)
    theta = (180 / np.pi) * np.arccos(cosine)            # degrees
    off = theta - theta0
    numerator = -off * off                               # the negation comes before the product, as in the reference; the value is the same either way
    sigma = sigma1 if theta <= theta0 else sigma2        # the narrow bell below theta0, the wide one above
    return np.exp(numerator / (2 * sigma ** 2)), theta


def scores(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0=5, sigma1=1, sigma2=10, with_angles=False):
    """-> score [C,C] float64 (and the list of every angle met).  A shared id without a row in point_ids raises KeyError, as the reference's dict does."""
    centers = np.asarray(centers, np.float64)
    table = {int(i): np.asarray(x, np.float64) for i, x in zip(point_ids, point_xyz)}
    ids = images(obs_offsets, obs_ids)
    sets = [set(a.tolist()) for a in ids]
    C = len(ids)
    score = np.zeros((C, C))
    angles = []
    for i in range(C):
        for j in range(i + 1, C):
            s = 0
            for pid in ids[i].tolist():
                if pid == -1 or pid not in sets[j]:
                    continue
                g, theta = term(centers[i], centers[j], table[pid], theta0, sigma1, sigma2)
                angles.append(theta)
                s += g
            score[i, j] = score[j, i] = s
    return (score, angles) if with_angles else score


def rank(score, num_views):
    """-> (ids [C,k] int64, scores [C,k]), k = min(num_views, C): descending score, the higher index first among equal scores."""
    sel = np.stack([np.argsort(row, kind="stable")[::-1][:num_views] for row in score])
    return sel.astype(np.int64), np.take_along_axis(score, sel, axis=1)


def view_selection(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0=5, sigma1=1, sigma2=10, num_views=10):
    """-> the reference's list of lists of (index, score)."""
    sel, val = rank(scores(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0, sigma1, sigma2), num_views)
    return [list(zip(a.tolist(), b.tolist())) for a, b in zip(sel, val)]


def top_gap(score, num_views):
    """The smallest relative difference between two DIFFERENT values among the top k + 1 of any row (own zero included); inf where there is none.
    Exactly equal values do not count: their order is the tie rule's, which no rounding moves as long as they stay exactly equal (zeros do)."""
    gap = np.inf
    for row in score:
        top = np.sort(row)[::-1][:num_views + 1]
        for x in range(len(top)):
            for y in range(x + 1, len(top)):
                if top[x] != top[y]:
                    gap = min(gap, abs(top[x] - top[y]) / max(abs(top[x]), abs(top[y])))
    return gap


def margins(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0=5, sigma1=1, sigma2=10, num_views=10):
    """-> (min angle, max angle, top gap) in degrees, degrees, relative."""
    score, angles = scores(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0, sigma1, sigma2, with_angles=True)
    return (min(angles) if angles else np.inf), (max(angles) if angles else -np.inf), top_gap(score, num_views)
