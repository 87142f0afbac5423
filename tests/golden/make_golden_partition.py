"""Golden vectors of the VastGaussian scene split, produced by RUNNING the reference's own four functions (gssr/utils/vastgaussian_utils.py:89-286) on the CPU.

    python tests/golden/make_golden_partition.py <reference checkout>     # writes tests/golden/ref_partition_*.npz

Three stand-ins let the reference's module import and run without a GPU and without shapely; nothing else of it is replaced:
  * shapely.geometry: a stub whose Polygon(hull).intersection(box(0, 0, w, h)).area is the exact convex clip of tests/ref_partition.py
    (clip_convex, area) -- the hull itself is the reference's own scipy.spatial.ConvexHull call;
  * simple_knn._C.distCUDA2 = tests/glue_truth.dist2_bruteforce, which the project's distCUDA2 matches bit for bit;
  * torch.Tensor.cuda = the identity.
The reference's projection() is wrapped (not replaced) to record the corner array it is given: that is where the tiles' mz / Mz are read from.

Scenes: `quad` (quadtree mode) and `grid` (num_col x num_row with leftover images that no tile gets): low oblique cameras, at heights comparable with the
tile size, over a ground cloud; SIMPLE_PINHOLE and PINHOLE cameras; a point far above the cloud that the 3-sigma mask removes; -1 ids, repeated ids, ids
with gaps, a points3D dict that does not ascend.  Asserted, a scene being redrawn by seed until all hold:
  * step 3 adds at least one image, rejects at least one by ratio alone (d < md) and at least one by d alone (ratio > threshold);
  * some image is in two tiles; the far point is inside a tile's box, is that tile's z maximum, and Mz is not its z;
  * no neighbour distance within a relative 1e-4 of either 3-sigma threshold (float32 pairwise summation moves them by about 1e-6);
  * no ratio within 1e-6 of the threshold, no d within a relative 1e-6 of md;
  * every corner's camera-space |z| is at least 1e-3 of the scene's extent.
The files hold arrays only: the model, the parameters, and per step the tiles' image ids, point ids (flattened, with offsets) and boxes."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit(__doc__)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ : ref_partition, glue_truth
import glue_truth  # noqa: E402
import ref_partition as rp  # noqa: E402
import torch  # noqa: E402


class _Polygon:
    def __init__(self, coords):
        self.coords = np.asarray(coords, np.float64).reshape(-1, 2)

    def intersection(self, rect):
        x0, y0, w, h = rect
        assert x0 == 0 and y0 == 0
        return types.SimpleNamespace(area=float(rp.area(rp.clip_convex(self.coords, w, h))))


geometry = types.ModuleType("shapely.geometry")
geometry.Polygon = _Polygon
geometry.box = lambda x0, y0, x1, y1: (x0, y0, x1, y1)
shapely = types.ModuleType("shapely")
shapely.geometry = geometry
knn = types.ModuleType("simple_knn")
knn._C = types.ModuleType("simple_knn._C")
knn._C.distCUDA2 = lambda pts: torch.from_numpy(glue_truth.dist2_bruteforce(pts.numpy()))
sys.modules.update({"shapely": shapely, "shapely.geometry": geometry, "simple_knn": knn, "simple_knn._C": knn._C})
torch.Tensor.cuda = lambda self, *a, **k: self
sys.path.insert(0, sys.argv[1])
from gssr.utils import vastgaussian_utils as ref  # noqa: E402

_seen = []
_projection = ref.projection


def _recording(points, extr, intr):
    if not _seen or not np.array_equal(_seen[-1], points):
        _seen.append(points.copy())
    return _projection(points, extr, intr)


ref.projection = _recording

EXTENT = 4.0
SCENES = {"quad": dict(C=32, n_points=640, num_col=None, num_row=None, max_num_images=10, ratio=0.2, threshold=0.25),
          "grid": dict(C=35, n_points=600, num_col=2, num_row=2, max_num_images=150, ratio=0.1, threshold=0.5)}
MODELS = ["SIMPLE_PINHOLE", "PINHOLE"]


def draw(C, n_points, seed, **_):
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(C)))
    cells = r.permutation(side * side)[:C]
    cx = (cells % side + r.uniform(0.1, 0.9, C)) * EXTENT / side
    cy = (cells // side + r.uniform(0.1, 0.9, C)) * EXTENT / side
    cen = np.stack([cx, cy, r.uniform(0.35, 0.9, C)], axis=1)
    ang, rad = r.uniform(0, 2 * np.pi, C), r.uniform(0.6, 1.6, C)
    target = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang), np.zeros(C)], axis=1)
    qt = [rp.look_at(c, t) for c, t in zip(cen, target)]
    qvecs, tvecs = np.array([q for q, _ in qt]), np.array([t for _, t in qt])
    xyz = np.stack([r.uniform(-0.3, EXTENT + 0.3, n_points), r.uniform(-0.3, EXTENT + 0.3, n_points), r.normal(0, 0.04, n_points)], axis=1)
    xyz[0] = [cen[3, 0], cen[3, 1], 3.0]                 # far above the cloud, over a camera: inside that camera's tile
    point_ids = r.permutation(r.choice(np.arange(5, 20 * n_points), n_points, replace=False)).astype(np.int64)      # gaps, and no ascending order
    ids = []
    for a in range(C):
        near = np.nonzero(np.hypot(xyz[:, 0] - target[a, 0], xyz[:, 1] - target[a, 1]) < 1.2)[0]
        seen = r.choice(near, min(40, len(near)), replace=False)
        row = point_ids[seen]
        row = np.concatenate([row, r.choice(row, 3) if len(row) else row, np.full(4, -1, np.int64)])
        ids.append(r.permutation(row).astype(np.int64))
    image_ids = (7 + 3 * r.permutation(C)).astype(np.int64)
    camera_of = r.integers(1, 3, C).astype(np.int64)
    cam_wh = np.array([[640, 480], [800, 600]], np.float64)
    cam_params = np.array([[330.0, 320.0, 240.0, 0.0], [420.0, 400.0, 400.0, 300.0]], np.float64)
    return dict(qvecs=qvecs, tvecs=tvecs, image_ids=image_ids, camera_of=camera_of, cam_wh=cam_wh, cam_params=cam_params, ids=ids, point_ids=point_ids, xyz=xyz)


def structures(sc):
    cameras = {k + 1: types.SimpleNamespace(id=k + 1, model=MODELS[k], width=int(sc["cam_wh"][k, 0]), height=int(sc["cam_wh"][k, 1]),
                                            params=sc["cam_params"][k, :3 + k]) for k in range(2)}
    images = {int(i): types.SimpleNamespace(id=int(i), qvec=q, tvec=t, camera_id=int(c), name=f"{int(i):05d}.jpg", point3D_ids=p)
              for i, q, t, c, p in zip(sc["image_ids"], sc["qvecs"], sc["tvecs"], sc["camera_of"], sc["ids"])}
    points3D = {int(i): types.SimpleNamespace(id=int(i), xyz=x) for i, x in zip(sc["point_ids"], sc["xyz"])}
    return cameras, images, points3D


def flat(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in lists])
    return off, (np.concatenate([np.asarray(a, np.int64) for a in lists]) if len(lists) else np.zeros(0, np.int64))


def margins(sc, cfg):
    """-> the restated partition when the scene meets every condition of the module docstring, else the name of the one it misses."""
    intr = np.array([[sc["cam_params"][c - 1, 0], sc["cam_params"][c - 1, 0 if c == 1 else 1], *sc["cam_wh"][c - 1]] for c in sc["camera_of"]])
    rs = rp.partition(sc["qvecs"], sc["tvecs"], intr, *flat(sc["ids"]), sc["point_ids"], sc["xyz"], cfg["num_col"], cfg["num_row"], cfg["max_num_images"],
                      cfg["ratio"], cfg["threshold"])
    vis, T = rs["vis"], len(rs["boxes"])
    non = np.ones_like(vis["add"])
    for t in range(T):
        non[t, rs["members"][t]] = False
    ok_r, ok_d = vis["ratio"] > cfg["threshold"], vis["d"] < vis["md"][:, None]
    if not (non & ok_r & ok_d).any(): return "no image added"
    if not (non & ~ok_r & ok_d).any(): return "none rejected by ratio alone"
    if not (non & ok_r & ~ok_d).any(): return "none rejected by d alone"
    if np.abs(vis["ratio"][non] - cfg["threshold"]).min() < 1e-6: return "a ratio at the threshold"
    if (np.abs(vis["d"] - vis["md"][:, None]) / vis["md"][:, None])[non].min() < 1e-6: return "a d at md"
    if np.abs(vis["zc"]).min() < 1e-3 * EXTENT: return "a corner in a camera's plane"
    for z in rs["zstats"]:
        d = z["dist"].astype(np.float64)
        if min(np.abs(d - z["lo"]).min() / abs(float(z["lo"])), np.abs(d - z["hi"]).min() / abs(float(z["hi"]))) < 1e-4: return "a distance at a 3-sigma threshold"
    far = [t for t in range(T) if 0 in rs["in_box"][t]]
    if not far or any(rs["zr"][t, 1] >= 3.0 or sc["xyz"][rs["in_box"][t], 2].max() != 3.0 for t in far): return "the far point is not removed"
    if np.bincount(np.concatenate(rs["images"]), minlength=cfg["C"]).max() < 2: return "no image in two tiles"
    return rs


def run(name, cfg):
    for seed in range(400):
        sc = draw(seed=seed, **cfg)
        rs = margins(sc, cfg)
        if not isinstance(rs, str):
            break
        print(f"{name}: seed {seed}: {rs}")
    else:
        raise SystemExit(f"{name}: no seed meets the margins")
    cameras, images, points3D = structures(sc)
    del _seen[:]
    t1 = ref.camera_position_based_region_division(images, cfg["num_col"], cfg["num_row"], cfg["max_num_images"])
    t2 = ref.position_based_data_selection(t1, images, points3D, ratio=cfg["ratio"])
    t3 = ref.visibility_based_camera_selection(t2, images, cameras, threshod=cfg["threshold"])
    t4 = ref.coverage_based_point_selection(t3, points3D)
    T = len(t1)
    assert len(_seen) == T
    zr = np.array([[b[0, 2], b[1, 2]] for b in _seen], np.float64)
    out = dict(qvecs=sc["qvecs"], tvecs=sc["tvecs"], image_ids=sc["image_ids"], camera_of=sc["camera_of"], cam_wh=sc["cam_wh"], cam_params=sc["cam_params"],
               point_ids=sc["point_ids"], xyz=sc["xyz"],
               params=np.array([-1 if cfg["num_col"] is None else cfg["num_col"], -1 if cfg["num_row"] is None else cfg["num_row"], cfg["max_num_images"],
                                cfg["ratio"], cfg["threshold"]], np.float64),
               boxes=np.array([t["box"] for t in t1], np.float64), zrange=zr,
               centers=np.array([ref.get_cam_center(i) for i in images.values()], np.float64))
    out["obs_offsets"], out["obs_ids"] = flat(sc["ids"])
    out["s1_off"], out["s1_images"] = flat([[it["image"].id for it in t["images"]] for t in t1])
    out["s2_off"], out["s2_images"] = flat([[i.id for i in t["images"]] for t in t2])
    out["s2p_off"], out["s2_points"] = flat([[p.id for p in t["points3D"]] for t in t2])
    out["s3_off"], out["s3_images"] = flat([[i.id for i in t["images"]] for t in t3])
    out["s4_off"], out["s4_points"] = flat([[p.id for p in t["points3D"]] for t in t4])
    for tiles in (t2, t3, t4):
        assert all(np.array_equal(a["box"], b["box"]) for a, b in zip(tiles, t1))
    # the restatement agrees with the reference's run exactly
    assert np.array_equal(rs["boxes"], out["boxes"]) and np.array_equal(rs["zr"], zr) and np.array_equal(rs["cen"], out["centers"])
    assert [list(sc["image_ids"][i]) for i in rs["images"]] == [[i.id for i in t["images"]] for t in t3]
    assert [list(p) for p in rs["points"]] == [[p.id for p in t["points3D"]] for t in t4]
    box_txt = f"mx Mx my My\n{t1[0]['box'][0]} {t1[0]['box'][1]} {t1[0]['box'][2]} {t1[0]['box'][3]}"
    out["box_txt"] = np.frombuffer(box_txt.encode(), np.uint8)
    path = os.path.join(HERE, f"ref_partition_{name}.npz")
    np.savez_compressed(path, **out)
    added = [len(t3[k]["images"]) - len(t2[k]["images"]) for k in range(T)]
    print(f"{name}: seed {seed}, tiles {T}, images per tile {[len(t['images']) for t in t1]} -> {[len(t['images']) for t in t3]} (added {added}), "
          f"points in box {[len(t['points3D']) for t in t2]} -> covered {[len(t['points3D']) for t in t4]}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    print(f"numpy {np.__version__}")
    for name, cfg in SCENES.items():
        run(name, cfg)
