"""Drop-in replacement for `diff_plane_rasterization` (submodules/diff-plane-rasterization/
diff_plane_rasterization/__init__.py): PGSR plane rasterizer.

    GaussianRasterizationSettings(..., prefiltered, render_geo, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, means2D_abs, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None, all_map=None)
        -> (color[3,H,W], radii[P], out_observe[P] int32, out_all_map[5,H,W], plane_depth[1,H,W])
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from gsrast import PLANE
from gsrast import rasterize as _rz


def rasterize_gaussians(means3D, means2D, means2D_abs, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, all_map, raster_settings):
    return _rz.rasterize_gaussians(PLANE, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                                   means2D_abs=means2D_abs, all_map=all_map)


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
    render_geo: bool
    debug: bool


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        from diff_gaussian_rasterization import GaussianRasterizer as _G
        return _G(self.raster_settings).markVisible(positions)

    def forward(self, means3D, means2D, means2D_abs, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None, all_map=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp, all_map = _rz.exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp, all_map)
        return rasterize_gaussians(means3D, means2D, means2D_abs, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, all_map, raster_settings)
