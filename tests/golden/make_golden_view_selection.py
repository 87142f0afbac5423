"""Golden vectors of the PGSR neighbour-view selection, produced by RUNNING the reference's own view_selection, calc_score, write_pairs and read_pairs
(numpy, CPU; gssr/utils/mvsnet_utils.py:306-362).

    python tests/golden/make_golden_view_selection.py <reference checkout>     # writes tests/golden/ref_view_selection_*.npz

Three scenes: C = 4 images with num_views = 5 (every row selects the image's own index), C = 12, and C = 70 with points that every image observes
(tracks longer than a wavefront).  Each has -1 entries, ids repeated within an image, ids with gaps, ids of points that only one image observes and
that the point table does not hold (the reference never looks those up), and one image without a valid observation.

The files hold arrays only: the centres, the flattened ids with their offsets, the point table, the full score matrix (calc_score for every pair),
what view_selection selected, the bytes of the pair.txt that write_pairs wrote and what read_pairs made of it.

Margins that keep the exact comparison of the selected indices honest (asserted; a scene is redrawn by seed until they hold):
  * every angle lies in [0.1, 179.9] degrees, where a few ulps of the cosine move a term by less than 1e-10 relative;
  * in every row, any two DIFFERENT values among the top k + 1 scores (own zero included) differ by a relative 1e-6 or more;
  * values that are exactly EQUAL there are zeros (the row of the image without observations, its column in the others, the own index), which no
    rounding moves; the order the reference leaves them in is its sort's, so the generator also asserts that what the reference selected IS the
    project's tie rule (descending score, the higher index first; tests/ref_view_selection.rank) in every row.  Whether numpy's sort leaves exact ties that way depends on
    its version and SIMD dispatch: it is checked on the numpy the generator runs with (2.2.6 for the committed files, printed below), never assumed, and
    a scene in which it did not hold is redrawn."""
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : ref_view_selection
import ref_view_selection as rvs  # noqa: E402
from gssr.utils import mvsnet_utils as ref  # noqa: E402

THETA0, SIGMA1, SIGMA2 = 5, 1, 10
SCENES = {"c4": dict(C=4, num_views=5, n_points=30, per_image=14, everywhere=0),
          "c12": dict(C=12, num_views=5, n_points=80, per_image=24, everywhere=0),
          "c70": dict(C=70, num_views=5, n_points=160, per_image=20, everywhere=6)}


def draw(C, n_points, per_image, everywhere, seed, **_):
    """Cameras on a loose ring around a cloud; every image observes the `everywhere` first points and a random choice of the others."""
    r = np.random.default_rng(seed)
    ang = np.sort(r.uniform(0, 2 * np.pi, C))
    rad = r.uniform(3.0, 4.5, C)
    centers = np.stack([rad * np.cos(ang), rad * np.sin(ang), r.uniform(-0.6, 0.6, C)], axis=1)
    point_ids = np.sort(r.choice(np.arange(3, 40 * n_points), n_points, replace=False)).astype(np.int64)      # gaps
    xyz = r.normal(0, 0.45, (n_points, 3))
    orphan = int(point_ids.max()) + 5                    # ids no table row exists for, each seen by one image only
    empty = int(r.integers(1, C - 1))                    # the image without a valid observation
    ids = []
    for a in range(C):
        if a == empty:
            ids.append(np.full(5, -1, np.int64))
            continue
        seen = np.concatenate([np.arange(everywhere), everywhere + r.choice(n_points - everywhere, per_image, replace=False)])
        row = point_ids[seen]
        row = np.concatenate([row, r.choice(row, 3), np.full(4, -1, np.int64), [orphan + a]])      # repeats, no-point entries, an orphan
        ids.append(r.permutation(row).astype(np.int64))
    return centers, ids, point_ids, xyz


def run(name, cfg):
    for seed in range(1000):
        centers, ids, point_ids, xyz = draw(seed=seed, **cfg)
        offsets = np.zeros(len(ids) + 1, np.int64)
        offsets[1:] = np.cumsum([len(a) for a in ids])
        flat = np.concatenate(ids)
        lo, hi, gap = rvs.margins(centers, offsets, flat, point_ids, xyz, THETA0, SIGMA1, SIGMA2, cfg["num_views"])
        if not (lo >= 0.1 and hi <= 179.9 and gap >= 1e-6):
            continue
        C, nv = cfg["C"], cfg["num_views"]
        points3d = {int(i): types.SimpleNamespace(xyz=x) for i, x in zip(point_ids, xyz)}
        cams = [c for c in centers]
        view_sel = ref.view_selection(cams, ids, points3d, THETA0, SIGMA1, SIGMA2, nv)
        restated = rvs.scores(centers, offsets, flat, point_ids, xyz, THETA0, SIGMA1, SIGMA2)
        if np.array_equal(np.array([[k for k, _ in row] for row in view_sel], np.int64), rvs.rank(restated, nv)[0]):
            break                                        # the reference's sort left the exact ties in the tie rule's order
    else:
        raise SystemExit(f"{name}: no seed meets the margins")
    score = np.zeros((C, C))
    for i in range(C):
        for j in range(i + 1, C):
            _, _, s = ref.calc_score(ids, cams, points3d, THETA0, SIGMA1, SIGMA2, (i, j))
            score[i, j] = score[j, i] = s
    sel_ids = np.array([[k for k, _ in row] for row in view_sel], np.int64)
    sel_scores = np.array([[s for _, s in row] for row in view_sel], np.float64)
    assert np.array_equal(sel_scores, np.take_along_axis(score, sel_ids, axis=1))
    want_ids, _ = rvs.rank(score, nv)
    assert np.array_equal(sel_ids, want_ids), f"{name}: the reference's sort left equal scores in another order than the tie rule"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pair.txt")
        ref.write_pairs(path, view_sel)
        pair_txt = np.frombuffer(open(path, "rb").read(), np.uint8)
        half = ref.read_pairs(path)
    out = os.path.join(HERE, f"ref_view_selection_{name}.npz")
    np.savez_compressed(out, centers=centers, obs_offsets=offsets, obs_ids=flat, point_ids=point_ids, point_xyz=xyz,
                        params=np.array([THETA0, SIGMA1, SIGMA2, nv], np.float64), scores=score, sel_ids=sel_ids, sel_scores=sel_scores, pair_txt=pair_txt,
                        read_ids=np.array([[k for k, _ in row] for row in half], np.int64), read_scores=np.array([[s for _, s in row] for row in half], np.float64))
    print(f"{name}: seed {seed}, C {C}, k {sel_ids.shape[1]}, observations {len(flat)}, angles [{lo:.3g}, {hi:.5g}] deg, top gap {gap:.2g}, "
          f"restatement - reference {np.abs(restated - score).max()}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    print(f"numpy {np.__version__}")
    for name, cfg in SCENES.items():
        run(name, cfg)
