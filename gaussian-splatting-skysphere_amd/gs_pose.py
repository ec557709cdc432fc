"""Pose refinement: a camera's tensors chained to a learnable twist, for `camera_grads=True`.

`GaussianRasterizer(..., camera_grads=True)` and `gs_sky.compose(..., camera_grads=True)` hand
gradients to `settings.viewmatrix`, `.projmatrix` and `.campos` as independent tensors.  This module
is the chain from a pose to the three of them, in plain torch (16 numbers: nothing for a kernel):

    twist = CameraTwist(cam).to(device)                      # delta = 0: the camera's own pose
    opt = torch.optim.Adam(twist.parameters(), lr=1e-3)
    s = twist.settings(base_settings)                        # non-leaf camera tensors
    image, *_ = gs_sky.render_with_sky(GaussianRasterizer(s), sky, camera_grads=True, means3D=..., ...)
    loss(image, gt).backward()                               # delta.grad: splats + sky
    opt.step()

Row-vector convention (include/gsrast.h; the reference's Camera keeps world_view_transform that
way): a point is a row p, p_cam = p @ view, the rotation block sits upper left and the translation in
the last row.  delta = (w, v): view = view0 @ exp(delta^) with

    delta^ = [[   0,  w_z, -w_y, 0],
              [-w_z,    0,  w_x, 0],
              [ w_y, -w_x,    0, 0],
              [ v_x,  v_y,  v_z, 0]]

so w turns the camera about its own axes (radians) and v moves it along them; projmatrix =
view @ projection and campos = view.inverse()[3, :3], as the reference's Camera builds them.
"""
from __future__ import annotations

import torch

__all__ = ["twist_matrix", "CameraTwist"]


def twist_matrix(delta: torch.Tensor) -> torch.Tensor:
    """exp(delta^) [4, 4] of a twist delta [6] = (w, v), row-vector convention, differentiable."""
    w, v = delta[:3], delta[3:]
    z = torch.zeros((), dtype=delta.dtype, device=delta.device)
    hat = torch.stack([torch.stack([z, w[2], -w[1], z]), torch.stack([-w[2], z, w[0], z]),
                       torch.stack([w[1], -w[0], z, z]), torch.stack([v[0], v[1], v[2], z])])
    return torch.matrix_exp(hat)


class CameraTwist(torch.nn.Module):
    """A camera with a learnable correction of its pose: one parameter `delta` [6], zeros at the start.

    cam: anything with `world_view_transform` and `projection_matrix` [4, 4] (the reference's Camera,
    gs_scenes.MiniCamera); both are copied into buffers, `delta` takes their dtype and device."""

    def __init__(self, cam):
        super().__init__()
        view0 = cam.world_view_transform.detach().clone()
        if tuple(view0.shape) != (4, 4) or tuple(cam.projection_matrix.shape) != (4, 4):
            raise ValueError("CameraTwist: world_view_transform and projection_matrix must be [4, 4]")
        self.register_buffer("view0", view0)
        self.register_buffer("projection", cam.projection_matrix.detach().clone().to(view0))
        self.delta = torch.nn.Parameter(torch.zeros(6, dtype=view0.dtype, device=view0.device))

    def camera_tensors(self):
        """(viewmatrix, projmatrix, campos) at the current delta, chained to it."""
        view = self.view0 @ twist_matrix(self.delta)
        return view, view @ self.projection, view.inverse()[3, :3]

    def settings(self, base_settings):
        """base_settings (a GaussianRasterizationSettings) with the three camera tensors replaced."""
        view, proj, campos = self.camera_tensors()
        return base_settings._replace(viewmatrix=view, projmatrix=proj, campos=campos)

    forward = settings
