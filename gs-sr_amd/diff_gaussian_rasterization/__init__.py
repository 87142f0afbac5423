"""Drop-in replacement for the reference's CUDA extension `diff_gaussian_rasterization`
(submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py), backed by the hand-written HIP
library libgsrast_hip.so for MI355X (gfx950).  Same names, argument meaning, return tuples and error messages:

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix,
                                  projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                        rotations=None, cov3D_precomp=None) -> (color[3,H,W], radii[P] int32)
    GaussianRasterizer.markVisible(positions) -> bool[P]
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from gsrast import EWA, call, dev_f32
from gsrast import rasterize as _rz


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _rz.rasterize_gaussians(EWA, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


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
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            rs = self.raster_settings
            pos = dev_f32(positions, "positions", allow_empty=True)
            P = int(positions.size(0))
            visible = torch.zeros((P,), dtype=torch.bool, device=positions.device)
            if P:
                vm, pm = dev_f32(rs.viewmatrix, "viewmatrix"), dev_f32(rs.projmatrix, "projmatrix")
                call("gsr_mark_visible", positions.device, P, pos, vm, pm, visible)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp = _rz.exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   raster_settings)
