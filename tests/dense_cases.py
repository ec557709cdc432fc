"""The named scenes of the dense-reference GPU tests, the camera arguments of a dense call and the mask of
the Gaussians whose fp32 radius differs (test infrastructure).

    sparse      2000 Gaussians of SH degree 3 (seed 41) at 200x120
    sparse-low  sparse with a third of the opacities (mask of seed 7) lowered to 0.003
    deep        6000 of degree 1 (seed 47), scales 0.01 .. 0.08
    opaque      8000 of degree 1 (seed 49), scales 0.02 .. 0.12, opacity 0.5 + 0.49 o
    empty-tile  the first three Gaussians of sparse at 72x40: whole tiles that nothing touches
"""
import math

import numpy as np
import torch

import dense_ref
import gs_scenes

LEAVES = ("means3D", "opacities", "shs", "scales", "rotations")
_SCENES = {}


def lowered():
    """the Gaussians of sparse-low whose opacity is lowered"""
    return torch.rand(2000, generator=torch.Generator().manual_seed(7)) < 1.0 / 3.0


def scene(name, device):
    """(cam, leaves, sh degree) of a named scene; leaves: LEAVES and a zero means2D; built once per device."""
    key = (name, str(device))
    if key not in _SCENES:
        cam = gs_scenes.identity_camera(200, 120)
        if name in ("sparse", "empty-tile", "sparse-low"):
            sc, deg = gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41), 3
        elif name == "deep":
            sc, deg = gs_scenes.random_gaussians(6000, 1, cam=cam, seed=47, scale_range=(0.01, 0.08)), 1
        elif name == "opaque":
            sc, deg = gs_scenes.random_gaussians(8000, 1, cam=cam, seed=49, scale_range=(0.02, 0.12)), 1
            sc.opacities = 0.5 + 0.49 * sc.opacities
        else:
            raise KeyError(name)
        if name == "sparse-low":
            sc.opacities = sc.opacities.clone()
            sc.opacities[lowered()] = 0.003
        leaves = {k: getattr(sc, k) for k in LEAVES}
        if name == "empty-tile":
            leaves = {k: v[:3].contiguous() for k, v in leaves.items()}
            cam = gs_scenes.identity_camera(72, 40)
        leaves = {k: v.to(device) for k, v in leaves.items()}
        leaves["means2D"] = torch.zeros_like(leaves["means3D"])
        _SCENES[key] = (cam, leaves, deg)
    return _SCENES[key]


def dense_args(cam, device, dtype):
    """(view, proj, campos, tanfovx, tanfovy, W, H): the arguments of every dense call after the opacities."""
    return (cam.world_view_transform.to(device, dtype), cam.full_proj_transform.to(device, dtype),
            cam.camera_center.to(device, dtype), math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), cam.image_width,
            cam.image_height)


def rect_and_radii(cam, leaves, deg, device):
    """(tile rectangles [P, 4] int64 numpy, radii [P] int32 cpu) of the fp64 dense reference."""
    f = torch.float64
    with torch.no_grad():
        q = dense_ref._prep(leaves["means3D"].to(f), torch.zeros_like(leaves["means3D"], dtype=f),
                            leaves["opacities"].to(f), *dense_args(cam, device, f), shs=leaves["shs"].to(f), deg=deg,
                            scales=leaves["scales"].to(f), rots=leaves["rotations"].to(f))
    return q["rect"].numpy(), q["radii"].cpu()


def wide_mask(rect, rdiff, W, H, into=None):
    """bool [H, W]: a Gaussian whose radius differs (rdiff [P] bool) composites into a rectangle up to one
    tile wider in fp32; those pixels are set in `into` (or in a new map of zeros)."""
    wide = np.zeros((H, W), bool) if into is None else into
    for i in np.nonzero(rdiff)[0]:
        x0, y0, x1, y1 = rect[i]
        wide[max(16 * y0 - 16, 0):16 * y1 + 16, max(16 * x0 - 16, 0):16 * x1 + 16] = True
    return wide
