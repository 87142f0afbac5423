"""What the scene-partition tests share: the golden scenes as the reference's structures and as arrays.  TEST INFRASTRUCTURE ONLY."""
import functools
import glob
import os
import types

import numpy as np

import ref_partition as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = sorted(os.path.basename(p)[len("ref_partition_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ref_partition_*.npz")))
MODELS = ["SIMPLE_PINHOLE", "PINHOLE"]


def split(off, flat):
    return [flat[off[t]:off[t + 1]].tolist() for t in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def load(name):
    """-> dict: the fixture's arrays, its parameters, the reference's three dicts, intr [C,4], and per step the lists of ids."""
    z = dict(np.load(os.path.join(GOLDEN, f"ref_partition_{name}.npz")))
    nc, nr, mx, ratio, thr = z["params"].tolist()
    z["cfg"] = dict(num_col=None if nc < 0 else int(nc), num_row=None if nr < 0 else int(nr), max_num_images=int(mx), ratio=ratio, threshold=thr)
    ids = split(z["obs_offsets"], z["obs_ids"])
    z["cameras"] = {k + 1: types.SimpleNamespace(id=k + 1, model=MODELS[k], width=int(z["cam_wh"][k, 0]), height=int(z["cam_wh"][k, 1]),
                                                 params=z["cam_params"][k, :3 + k]) for k in range(2)}
    z["images"] = {int(i): types.SimpleNamespace(id=int(i), qvec=q, tvec=t, camera_id=int(c), name=f"{int(i):05d}.jpg", point3D_ids=np.array(p, np.int64))
                   for i, q, t, c, p in zip(z["image_ids"], z["qvecs"], z["tvecs"], z["camera_of"], ids)}
    z["points3D"] = {int(i): types.SimpleNamespace(id=int(i), xyz=x) for i, x in zip(z["point_ids"], z["xyz"])}
    z["intr"] = np.array([[z["cam_params"][c - 1, 0], z["cam_params"][c - 1, 0 if c == 1 else 1], *z["cam_wh"][c - 1]] for c in z["camera_of"]], np.float64)
    for key, off, flat in (("s1", "s1_off", "s1_images"), ("s2", "s2_off", "s2_images"), ("s2p", "s2p_off", "s2_points"), ("s3", "s3_off", "s3_images"),
                           ("s4", "s4_off", "s4_points")):
        z[key] = split(z[off], z[flat])
    return z


@functools.lru_cache(maxsize=None)
def restated(name):
    """ref_partition.partition of the scene: computed once, shared, never modified."""
    z = load(name)
    c = z["cfg"]
    return rp.partition(z["qvecs"], z["tvecs"], z["intr"], z["obs_offsets"], z["obs_ids"], z["point_ids"], z["xyz"], c["num_col"], c["num_row"], c["max_num_images"],
                        c["ratio"], c["threshold"])


def image_at(cen, k):
    """An image whose centre is cen (identity rotation) with id k."""
    return types.SimpleNamespace(id=k, qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=-np.asarray(cen, np.float64), camera_id=1, name=f"{k}.jpg",
                                 point3D_ids=np.zeros(0, np.int64))
