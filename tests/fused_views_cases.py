"""Constructed scenes and cameras for the K-view per-Gaussian backward (k_backward_gaussians; test
infrastructure, pure torch / numpy).

The random balls in front of circle cameras that the other multi-view tests use make nearly every
Gaussian visible in every view.  Here the views differ per Gaussian:

  visibility_scene()   three cameras of different image sizes and fields of view, side by side and
                       turned to different yaws; clusters of Gaussians placed in each of the 8
                       seen / not-seen patterns over the three views, for each of the three reasons
                       a view may not see a Gaussian (depth <= 0.2, empty tile rectangle, opacity
                       below 1/255), and a cluster whose colour clamps in one view and not in another
  ring_cameras(K)      K cameras on a circle, cycling the three image sizes; optionally the last one
                       turned to a target that no other camera sees
  layout_scene(...)    a small ball of Gaussians with SH rows of M coefficients (every one non-zero,
                       also those past the active degree), precomputed colours or precomputed 3D
                       covariances

Every scene is a dict of CPU float32 tensors named as the rasterizer's inputs (`leaves`): means3D,
opacities, and shs | colors, and scales + rotations | cov3D.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

import gs_scenes

SIZES = ((64, 48), (80, 32), (48, 64))  # (W, H)
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
GROUP = 32  # Gaussians per cluster

# The three cameras of visibility_scene(): (x of the position, yaw in degrees, vertical field of view).
# Together with the image shapes the horizontal / vertical half angles are about 35 / 28 (view 0),
# 42 / 20 (view 1: wide and low) and 28 / 35 degrees (view 2: narrow and tall).  They stand 0.1 apart
# (not at one point): the colour clamp depends on the direction from the camera centre alone, so views
# from one point could never clamp one Gaussian differently.
VIS_CAMS = ((0.0, 30.0, 56.0), (0.1, 0.0, 40.0), (-0.1, -5.0, 70.0))

# (name, pattern over the three views, azimuth, elevation in degrees, distance range, opacity range)
# azimuth from +z towards +x, elevation towards -y (up in the image)
VIS_GROUPS = (
    ("all", (1, 1, 1), 8.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("v1v2", (0, 1, 1), -18.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("v0v1", (1, 1, 0), 33.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("v0v2", (1, 0, 1), 18.0, 25.0, (3.0, 4.0), (0.3, 0.9)),
    ("v1", (0, 1, 0), -38.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("v0", (1, 0, 0), 55.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("v2", (0, 0, 1), -18.0, 28.0, (3.0, 4.0), (0.3, 0.9)),
    # not seen by anyone: behind the cameras (depth), and in front of all three but too faint
    ("behind", (0, 0, 0), 180.0, 0.0, (3.0, 4.0), (0.3, 0.9)),
    ("faint", (0, 0, 0), 8.0, 4.0, (3.0, 4.0), (0.0005, 0.003)),
    # close to the cameras: inside view 1's frustum by direction, but nearer than 0.2 along its axis
    ("near_v0", (1, 0, 0), 40.0, 0.0, (0.245, 0.255), (0.3, 0.9)),
    # close, seen by all three from clearly different directions: the colour-clamp cluster
    ("clamp", (1, 1, 1), 3.0, 0.0, (0.48, 0.52), (0.3, 0.9)),
)


@dataclass
class VisibilityScene:
    leaves: dict          # means3D, opacities, shs [P, 16, 3], scales, rotations
    cams: list            # the three MiniCameras
    group: np.ndarray     # [P] index into VIS_GROUPS
    pattern: np.ndarray   # [P, 3] bool: the pattern each Gaussian was placed for


def _yaw_camera(x, yaw_deg, fovy_deg, W, H):
    a = math.radians(yaw_deg)
    return gs_scenes.look_at_camera((x, 0.0, 0.0), (x + math.sin(a), 0.0, math.cos(a)), W, H, fovy_deg)


def visibility_cameras():
    return [_yaw_camera(x, yaw, fovy, W, H) for (x, yaw, fovy), (W, H) in zip(VIS_CAMS, SIZES)]


def visibility_scene(seed=11) -> VisibilityScene:
    g = torch.Generator().manual_seed(seed)
    cams = visibility_cameras()

    def rand(n, lo, hi):
        return lo + (hi - lo) * torch.rand((n,), generator=g, dtype=torch.float64)

    means, opac, group, pattern, scales = [], [], [], [], []
    for k, (_, pat, az, el, (r0, r1), (o0, o1)) in enumerate(VIS_GROUPS):
        a = torch.deg2rad(az + rand(GROUP, -0.7, 0.7))
        e = torch.deg2rad(el + rand(GROUP, -0.3, 0.3))
        r = rand(GROUP, r0, r1)
        means.append(torch.stack([r * torch.cos(e) * torch.sin(a), -r * torch.sin(e), r * torch.cos(e) * torch.cos(a)], 1))
        opac.append(rand(GROUP, o0, o1))
        # about a third of a pixel wide at its distance: the radius stays at 2 to 3 pixels
        scales.append(r[:, None] * torch.exp(rand(3 * GROUP, math.log(0.002), math.log(0.006))).reshape(GROUP, 3))
        group += [k] * GROUP
        pattern += [pat] * GROUP
    means3D = torch.cat(means).float()
    P = means3D.shape[0]
    q = torch.randn((P, 4), generator=g)
    shs = torch.cat([(torch.rand((P, 1, 3), generator=g) - 0.5) / SH_C0, 0.05 * torch.randn((P, 15, 3), generator=g)], 1)
    group = np.asarray(group)
    # the clamp cluster: channel 0 is +0.3 seen from view 1 and -0.3 (clamped to 0) seen from view 2, by a
    # degree-1 term linear in the unit direction d: rgb = 0.5 + C0 s0 + C1 (-y s1 + z s2 - x s3)
    idx = np.nonzero(group == [n for n, *_ in VIS_GROUPS].index("clamp"))[0]
    m = means3D[idx].double()
    d1 = torch.nn.functional.normalize(m - cams[1].camera_center.double()[None], dim=1)
    d2 = torch.nn.functional.normalize(m - cams[2].camera_center.double()[None], dim=1)
    dd = d1 - d2
    w = (0.6 / SH_C1) * dd / (dd * dd).sum(1, keepdim=True)      # w . d1 - w . d2 = 0.6 / C1
    s0 = -(0.5 + SH_C1 * (w * (d1 + d2)).sum(1) / 2) / SH_C0     # the two colours are +0.3 and -0.3
    shs[idx, 0, 0] = s0.float()
    shs[idx, 1, 0], shs[idx, 2, 0], shs[idx, 3, 0] = (-w[:, 1]).float(), w[:, 2].float(), (-w[:, 0]).float()
    leaves = dict(means3D=means3D.contiguous(), opacities=torch.cat(opac).float()[:, None].contiguous(),
                  shs=shs.contiguous(), scales=torch.cat(scales).float().contiguous(),
                  rotations=torch.nn.functional.normalize(q).contiguous())
    return VisibilityScene(leaves, cams, group, np.asarray(pattern, bool))


def ring_cameras(K, radius=6.0, last_target=None):
    """K <= 17 cameras on a circle around the origin looking at it (gs_scenes.circle_cameras), the
    image sizes cycling through SIZES.  last_target: the last camera looks at that point instead."""
    assert 1 <= K <= 17
    cams = [gs_scenes.circle_cameras(K, radius, *SIZES[v % 3])[v] for v in range(K)]
    if last_target is not None:
        a = 2.0 * math.pi * (K - 1) / K
        cams[-1] = gs_scenes.look_at_camera((radius * math.cos(a), 0.0, radius * math.sin(a)), last_target,
                                            *SIZES[(K - 1) % 3])
    return cams


LAYOUTS = ((0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16))  # (active degree D, stored coefficients M)
MARK_TARGET = (0.0, -10.0, 0.0)  # where layout_scene(marked=) puts its marked Gaussians: above every ring camera's view


def layout_scene(P, D, M, kind="sh", seed=3, marked=0):
    """P Gaussians in a ball of radius 2 around the origin (in view of every ring camera).
    kind "sh": SH rows [P, M, 3] of active degree D, all M coefficients non-zero; "colors": precomputed
    colours [P, 3] (D, M unused); "cov3d": SH rows and precomputed covariances [P, 6] instead of scales
    and rotations.  marked: the last `marked` Gaussians sit around MARK_TARGET instead."""
    assert kind in ("sh", "colors", "cov3d") and (kind == "colors" or (D, M) in LAYOUTS)
    d = gs_scenes.random_gaussians(P, 3, seed=seed, ball_radius=2.0, scale_range=(0.02, 0.08))
    g = torch.Generator().manual_seed(seed + 1000)
    if marked:
        d.means3D[P - marked:] = torch.tensor(MARK_TARGET) + 0.3 * (torch.rand((marked, 3), generator=g) - 0.5)
    leaves = dict(means3D=d.means3D.contiguous(), opacities=d.opacities.contiguous())
    if kind == "colors":
        leaves["colors"] = torch.rand((P, 3), generator=g)
    else:
        shs = d.shs[:, :M].clone()
        shs[:, 1:] = 0.2 * torch.randn((P, M - 1, 3), generator=g)
        leaves["shs"] = shs.contiguous()
    if kind == "cov3d":
        R = _quat_R(d.rotations.double())
        L = R * d.scales.double()[:, None, :]
        S = L @ L.transpose(1, 2)
        leaves["cov3D"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]],
                                      1).float().contiguous()
    else:
        leaves["scales"], leaves["rotations"] = d.scales.contiguous(), d.rotations.contiguous()
    return leaves


def _quat_R(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
        torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
        torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1),
    ], -2)


# ---- what the fp64 reference (tests/dense_ref.py) says about a scene: shared by the CPU checks of the
# ---- constructions and the GPU tests, which compare the kernels' view of the scene with it ----
def dense_prep(leaves, cam, D, mod=1.0, dtype=torch.float64):
    import dense_ref

    t = {k: v.to(dtype) for k, v in leaves.items()}
    return dense_ref._prep(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"],
                           cam.world_view_transform.to(dtype), cam.full_proj_transform.to(dtype),
                           cam.camera_center.to(dtype), math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                           cam.image_width, cam.image_height, shs=t.get("shs"), deg=D, colors=t.get("colors"),
                           scales=t.get("scales"), rots=t.get("rotations"), cov3D=t.get("cov3D"), mod=mod)


def contributes(radii, opacities):
    """[P] bool: the Gaussians of a view that can reach a pixel -- a non-empty tile rectangle in front
    of the near plane (radius > 0) and an opacity of at least 1/255 (below it alpha never reaches the
    1/255 a pixel needs: the rasterizer gives such a Gaussian no tile instances)."""
    return (np.asarray(radii) > 0) & (np.asarray(opacities).reshape(-1) >= np.float32(1.0 / 255.0))


def clamp_bits(leaves, cam, D):
    """[P, 3] bool: the colour channels that the SH evaluation clamps at 0 in this view (fp64)."""
    import dense_ref

    m, c = leaves["means3D"].double(), cam.camera_center.double()
    d = torch.nn.functional.normalize(m - c[None], dim=1)
    return (dense_ref.sh_rgb(D, leaves["shs"].double(), d) + 0.5 < 0).numpy()
