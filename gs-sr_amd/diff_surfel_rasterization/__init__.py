"""Drop-in replacement for `diff_surfel_rasterization` (submodules/diff-surfel-rasterization/
diff_surfel_rasterization/__init__.py): 2DGS surfel rasterizer with the fork's 11-channel auxiliary map.

    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                        rotations=None, cov3D_precomp=None) -> (color[3,H,W], radii[P], allmap[11,H,W])

allmap channels: 0 depth*alpha, 1 alpha, 2-4 view-space normal, 5 median depth, 6 distortion, 7 median splat index,
8-10 median normal.  `scales` is (P,2); the `cov3D_precomp` slot carries a precomputed transMat (P,9).
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from gsrast import SURFEL
from gsrast import rasterize as _rz


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _rz.rasterize_gaussians(SURFEL, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        from diff_gaussian_rasterization import GaussianRasterizer as _G
        return _G(self.raster_settings).markVisible(positions)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp = _rz.exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp, device=means3D.device)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   raster_settings)
