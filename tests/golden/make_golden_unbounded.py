"""Golden lattice of the unbounded mesh path, produced by RUNNING the reference's own extract_mesh_unbounded (torch, CPU).

    python tests/golden/make_golden_unbounded.py          # needs /root/reference; about half a minute and 6 GB; writes ref_unbounded_lattice.npz

Pinned (reference file:line -> fixture):
  ref_unbounded_lattice.npz
        gssr/utils/mesh_utils.py:181-277 GaussianExtractor.extract_mesh_unbounded(resolution=512) -- the smallest size it accepts, one 512^3 block --
        through its real gssr/utils/mcube_utils.py:17-95 marching_cubes_with_contraction: the lattice it builds (np.linspace / torch.linspace), the
        un-contraction, the adaptive truncation and the running average over the frames.  skimage is absent: `measure.marching_cubes` is a recorder
        that keeps the `volume` it is handed and raises; a wrapper around marching_cubes_with_contraction records `bounding_box_max`, the quantile
        bound R.  Frames and cameras are those of ref_tsdf_unbounded.npz.  Saved: the inputs, R, and the volume on the sub-lattice of every
        STRIDE-th plane per axis (57^3 of the 512^3 samples) and, by index, the samples around the zero crossing (all negative ones, a share of
        the small positive ones) -- the full volume is never committed.
"""
import os
import types

import numpy as np
import torch

from make_golden_ref import HERE, _bare, ref_import, save

STRIDE = 9
BAND, BAND_STRIDE = 0.25, 16


class _Recorded(Exception):
    pass


def unbounded_lattice_fixture():
    mu = ref_import("gssr.utils.mesh_utils")
    mc = ref_import("gssr.utils.mcube_utils")
    fr = np.load(os.path.join(HERE, "ref_tsdf_unbounded.npz"))
    nf = fr["full_proj"].shape[0]
    stack = [types.SimpleNamespace(full_proj_transform=torch.tensor(fr["full_proj"][i])) for i in range(nf)]
    center = np.array([0.1, -0.05, 2.6], np.float32); radius = 1.7
    r = np.random.default_rng(131)
    xyz = (center + r.normal(0, 1.1, (500, 3))).astype(np.float32)
    ex = _bare(mu.GaussianExtractor, viewpoint_stack=stack, depthmaps=[torch.tensor(d) for d in fr["depth"]], rgbmaps=[torch.tensor(c) for c in fr["rgb"]],
               radius=radius, center=torch.tensor(center), gaussians=types.SimpleNamespace(get_xyz=torch.tensor(xyz)))
    got = {}

    def recorder(volume, level, spacing):
        got["volume"] = np.array(volume, np.float32)
        raise _Recorded()
    mc.measure.marching_cubes = recorder
    real = mc.marching_cubes_with_contraction

    def wrapped(**kw):
        got["R"] = float(kw["bounding_box_max"][0])
        assert kw["bounding_box_min"] == (-kw["bounding_box_max"][0],) * 3 and kw["resolution"] == 512
        return real(**kw)
    mu.marching_cubes_with_contraction = wrapped
    mu.tqdm = lambda it, **kw: it
    try:
        ex.extract_mesh_unbounded(resolution=512)
    except _Recorded:
        pass
    vol = got["volume"]
    assert vol.shape == (512, 512, 512)
    sub = np.ascontiguousarray(vol[::STRIDE, ::STRIDE, ::STRIDE])
    # the strided planes hold next to no negative sample (the reference starts every sample at tsdf 1 with weight 1, so few averages cross 0): every
    # negative sample of the full volume and every BAND_STRIDE-th of the positive ones below BAND are kept by index, so that signs are pinned too
    neg = np.argwhere(vol < 0)
    pos = np.argwhere((vol >= 0) & (vol < BAND))[::BAND_STRIDE]
    band = np.concatenate([neg, pos]).astype(np.int16)
    band_val = vol[band[:, 0], band[:, 1], band[:, 2]]
    print("band", len(neg), "negative +", len(pos), "positive below", BAND)
    print("R", got["R"], "touched", float((vol != 1).mean()), "negative", float((vol < 0).mean()), "sub", sub.shape)
    save("ref_unbounded_lattice.npz", xyz=xyz, center=center, radius=np.float64(radius), R=np.float64(got["R"]), resolution=512, crop=512,
         stride=STRIDE, volume=sub, band_index=band, band_value=band_val)


if __name__ == "__main__":
    unbounded_lattice_fixture()
