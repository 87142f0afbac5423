"""Synthetic RGB-D frames for the TSDF tests (numpy only): a wavy surface seen from a few nearby poses."""
import functools

import numpy as np


def frames(n=4, W=160, H=120, seed=0, holes=True):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 140.0, 135.0, W / 2 - 0.5, H / 2 - 0.5
    out = []
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    for k in range(n):
        a = 0.06 * k
        E = np.array([[np.cos(a), 0, np.sin(a), 0.05 * k], [0, 1, 0, -0.03 * k], [-np.sin(a), 0, np.cos(a), 0.08 * k], [0, 0, 0, 1]], np.float64)
        depth = (4.0 + 0.4 * np.sin(u / 17.0 + k) + 0.3 * np.cos(v / 13.0)).astype(np.float32)[None]
        if holes:
            depth[0, : 6 + k] = 0.0                       # masked rows (mesh_utils.py:165-166 zeroes depth where the alpha mask is low)
            depth[0, 40:50, 60:90] = 9.0                  # beyond depth_trunc
        rgb = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
        out.append(dict(rgb=rgb, depth=depth, fx=fx, fy=fy, cx=cx, cy=cy, E=E.astype(np.float32)))
    return out


def rgb8(rgb):
    return (np.clip(rgb, 0, 1) * 255).astype(np.uint8).astype(np.float32)


def small_frames(W=48, H=36, n=3, fx=40.0, dist=1.0, seed=0, defects=True, top_hole=None):
    """Small scenes for the float64-truth tests (tsdf_truth): the poses of `frames`, a wavy surface at distance `dist`, the camera shifted by a seeded
    fraction of a unit (so that the seed decides which unit faces the samples come close to), and -- `defects` -- every kind of depth pixel the kernels
    must skip: zero rows, a block beyond depth_trunc (9.0; a sample again with depth_trunc=inf), a NaN block, a negative block; colours in [-0.1, 1.1].
    top_hole=(rows, first column): the top `rows` pixel rows are valid only left of that column -- a wave of samples with a few valid ones.
    No colour lies within 1e-3 of a byte boundary without being on it: the float32 product c * 255 then truncates like the exact one."""
    rng = np.random.default_rng(seed)
    fy, cx, cy = fx * 135.0 / 140.0, W / 2 - 0.5, H / 2 - 0.5
    ph = rng.uniform(0, 2 * np.pi, 2)
    shift = rng.uniform(-0.16, 0.16, 3)
    out = []
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    for k in range(n):
        a = 0.06 * k
        E = np.array([[np.cos(a), 0, np.sin(a), 0.05 * k + shift[0]], [0, 1, 0, -0.03 * k + shift[1]], [-np.sin(a), 0, np.cos(a), 0.08 * k + shift[2]],
                      [0, 0, 0, 1]], np.float64)
        depth = (dist * (1.0 + 0.12 * np.sin(u / 7.0 + k + ph[0]) + 0.09 * np.cos(v / 5.0 + ph[1]))).astype(np.float32)[None]
        if defects:
            depth[0, : 2 + k] = 0.0
            depth[0, H // 3: H // 3 + 5, W // 3: W // 3 + 9] = 9.0
            depth[0, H // 2: H // 2 + 3, 2:8] = np.nan
            depth[0, H // 2 + 4: H // 2 + 7, W - 10: W - 3] = -1.0
        if top_hole:
            depth[0, : top_hole[0], top_hole[1]:] = 0.0
        rgb = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
        q = np.clip(rgb.astype(np.float64), 0, 1) * 255
        near = (np.abs(q - np.round(q)) < 1e-3) & (q != np.round(q))
        rgb[near] += np.float32(1e-4)
        out.append(dict(rgb=rgb, depth=depth, fx=fx, fy=fy, cx=cx, cy=cy, E=E.astype(np.float32)))
    return out


SMALL_VL, SMALL_DT = 0.02, 6.0
# name -> (small_frames arguments, sdf_trunc in voxels, depth sampling stride).  The seeds are the first for which no sample of any frame is fragile
# (tsdf_truth: allocation is then exact) and, for "t9", for which one workgroup holds both kinds of wave; test_tsdf_truth_cpu.py asserts both.
SMALL_SCENES = {
    "t5": (dict(seed=0), 5, 4),
    "t9": (dict(W=96, H=72, fx=80.0, top_hole=(12, 16), seed=2822), 9, 4),
    "t12": (dict(seed=5), 12, 4),
    "t24": (dict(seed=0), 24, 4),
    "s1": (dict(W=47, H=35, seed=382), 5, 1),
    "s3": (dict(W=47, H=35, seed=0), 5, 3),
    "s4": (dict(W=47, H=35, seed=0), 5, 4),
    "w5x3": (dict(W=5, H=3, fx=4.0, defects=False, seed=0), 5, 4),
    "w7x5": (dict(W=7, H=5, fx=6.0, defects=False, seed=0), 5, 1),
    "near": (dict(W=64, H=48, dist=0.28, seed=0), 5, 4),
}


def small_scene(name):
    """-> (frames, voxel_length, sdf_trunc, stride).  voxel_length is a float32 value and sdf_trunc a whole number of voxels."""
    kw, tv, stride = SMALL_SCENES[name]
    vl = float(np.float32(SMALL_VL))
    return small_frames(**kw), vl, float(np.float32(tv * vl)), stride


def probe_wrap_lists():
    """Unit coordinates for the probing tests of a 16-unit volume (32 table entries, 64 after one growth) -> (first [12,3], more [8,3]) int32.
    `first`: first probe positions 29, 30, 31, 31, 31, 0, 0, 1, 2, 2, 5, 9 of 32 -- the cluster runs over the end of the table -- and the three at 31 all at
    63 of 64, so that re-keying the grown table wraps as well.  `more`: 62, 63, 0, 0, 1, 20, 33, 47 of 64.  The first coordinates of [-6, 6]^3 in x-major order that fit."""
    from tsdf_truth import ts_hash, ts_pack
    cube = [(x, y, z) for x in range(-6, 7) for y in range(-6, 7) for z in range(-6, 7)]
    used = set()

    def pick(ok):
        c = next(c for c in cube if c not in used and ok(ts_pack(*c)))
        used.add(c)
        return c
    first = [pick(lambda k, p=p: ts_hash(k, 5) == p and (p != 31 or ts_hash(k, 6) == 63)) for p in (29, 30, 31, 31, 31, 0, 0, 1, 2, 2, 5, 9)]
    more = [pick(lambda k, p=p: ts_hash(k, 6) == p) for p in (62, 63, 0, 0, 1, 20, 33, 47)]
    return np.array(first, np.int32), np.array(more, np.int32)


# the truth cases the CPU and GPU tests share: name -> (scene, depth_trunc, quant)
TRUTH_CASES = {n: (n, SMALL_DT, 2) for n in SMALL_SCENES}
TRUTH_CASES.update({"t5_inf": ("t5", float("inf"), 2), "t5_f32": ("t5", SMALL_DT, 1)})


@functools.lru_cache(maxsize=None)
def small_truth(case):
    """-> (frames, voxel_length, sdf_trunc, stride, depth_trunc, quant, tsdf_truth.SparseTruth after every frame).  Computed once; nobody changes it."""
    import tsdf_truth
    scene, dt, quant = TRUTH_CASES[case]
    frs, vl, tr, stride = small_scene(scene)
    tv = tsdf_truth.SparseTruth(vl, tr, stride)
    for f in frs:
        tv.integrate(f["rgb"], f["depth"], f["fx"], f["fy"], f["cx"], f["cy"], f["E"], depth_trunc=dt, quant=quant)
    return frs, vl, tr, stride, dt, quant, tv
