"""Skysphere background on MI355X: a learnable equirectangular sky behind the splats.

The rasterizer's `aux_outputs=True` call returns `alpha = 1 - final_T` so that a per-pixel
background can be composited as `color + (1 - alpha) * sky`.  This module is that sky: a texture
[3, Hs, Ws] sampled along every pixel's camera ray, one fused HIP forward and one fused backward
(csrc/gs_sky.hip, C ABI gs_sky_compose_forward / gs_sky_compose_backward) in place of the ray
arithmetic, the bilinear gather and its scatter gradient written in torch.

Conventions (include/gsrast.h, the same in every layer): pixel (x, y) has the camera-space ray
`(((2x + 1) / W - 1) tanfovx, ((2y + 1) / H - 1) tanfovy, 1)` -- integer coordinates are pixel
centres, the inverse of the rasterizer's projection -- turned into the world by
`d_i = sum_j V[i][j] d_cam_j` with `V = settings.viewmatrix` (row-vector convention);
`u = atan2(d.x, d.z) / 2pi + 0.5` picks the column (wrapping), `v = acos(-d.y / |d|) / pi` the row
(row 0 is world -y, "up" for y-down cameras; rows clamp), texel centres at half-integers, bilinear.

    sky = SkySphere(512, 1024).cuda()
    image, radii, invdepth, alpha = render_with_sky(GaussianRasterizer(settings), sky, means3D=..., ...)

Gradients flow to the texture, to alpha (and through the rasterizer's aux backward to the
opacities and geometry) and to the colour.  dL/dtexture is bitwise reproducible (64-bit fixed-point
sums).  `gs_train.FusedAdam` steps `sky.texture` like any other parameter.

Pose refinement: with `camera_grads=True` a `settings.viewmatrix` that requires grad also receives
the sky's dL/dviewmatrix [4, 4] (the rotation block; a sky at infinity does not see the translation),
summed on the same backward pass in fp64 in a fixed order (gs_sky_compose_backward_camera, bitwise
reproducible).  `render_with_sky(..., camera_grads=True)` hands the flag to the rasterizer too, and
autograd adds the two shares; `gs_pose.CameraTwist` chains the camera tensors to a pose.
"""
from __future__ import annotations

import ctypes

import torch

from diff_gaussian_rasterization import _native

_lib = _native.load()

__all__ = ["pixel_directions", "compose", "SkySphere", "render_with_sky"]


def pixel_directions(settings) -> torch.Tensor:
    """World-space rays [H, W, 3] of the pixel centres (not normalised), on the device and in the
    dtype of settings.viewmatrix: the rays the sky kernels sample along."""
    V = settings.viewmatrix
    H, W = int(settings.image_height), int(settings.image_width)
    x = torch.arange(W, device=V.device, dtype=V.dtype)
    y = torch.arange(H, device=V.device, dtype=V.dtype)
    cx = ((2 * x + 1) / W - 1) * settings.tanfovx
    cy = ((2 * y + 1) / H - 1) * settings.tanfovy
    cx, cy = cx[None, :].expand(H, W), cy[:, None].expand(H, W)
    return torch.stack([V[i, 0] * cx + V[i, 1] * cy + V[i, 2] for i in range(3)], dim=-1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _f32(t, name):
    if t.dtype != torch.float32:
        raise ValueError(f"gs_sky.compose: {name} must be float32 (got {t.dtype})")


class _Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, alpha, texture, settings, viewmatrix):
        # (viewmatrix: settings.viewmatrix itself, an input for the graph's sake -- camera_grads)
        if not texture.is_cuda or (color is not None and not color.is_cuda) or (alpha is not None and not alpha.is_cuda):
            raise RuntimeError("gs_sky.compose (MI355X/HIP) needs device tensors; there is no CPU path")
        H, W = int(settings.image_height), int(settings.image_width)
        if texture.dim() != 3 or texture.shape[0] != 3 or texture.shape[1] < 1 or texture.shape[2] < 1:
            raise ValueError(f"gs_sky.compose: texture must be [3, Hs, Ws] (got {tuple(texture.shape)})")
        _f32(texture, "texture")
        if color is not None:
            if tuple(color.shape) != (3, H, W):
                raise ValueError(f"gs_sky.compose: color must be [3, {H}, {W}] (got {tuple(color.shape)})")
            _f32(color, "color")
        if alpha is not None:
            if tuple(alpha.shape) not in ((H, W), (1, H, W)):
                raise ValueError(f"gs_sky.compose: alpha must be [{H}, {W}] or [1, {H}, {W}] (got {tuple(alpha.shape)})")
            _f32(alpha, "alpha")
        dev = texture.device
        tex = texture.detach().contiguous()
        col = None if color is None else color.detach().to(dev).contiguous()
        alp = None if alpha is None else alpha.detach().to(dev).contiguous()
        view = settings.viewmatrix.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(view.shape) != (4, 4):
            raise ValueError(f"gs_sky.compose: settings.viewmatrix must be [4, 4] (got {tuple(view.shape)})")
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        Hs, Ws = int(tex.shape[1]), int(tex.shape[2])
        tfx, tfy = float(settings.tanfovx), float(settings.tanfovy)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            _native.check(_lib.gs_sky_compose_forward(W, H, _p(view), tfx, tfy, Hs, Ws, _p(tex), _p(col), _p(alp),
                                                      _p(out), st), "sky forward")
        ctx.save_for_backward(tex, alp, view)
        ctx.geom = (W, H, Hs, Ws, tfx, tfy, None if alpha is None else tuple(alpha.shape))
        return out

    @staticmethod
    def backward(ctx, grad):
        tex, alp, view = ctx.saved_tensors
        W, H, Hs, Ws, tfx, tfy, alpha_shape = ctx.geom
        need_color, need_alpha, need_tex = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_view = ctx.needs_input_grad[4]
        if grad is None:
            return None, None, None, None, None
        dev = tex.device
        g = grad.to(torch.float32).contiguous()
        dalpha = torch.empty((H, W), dtype=torch.float32, device=dev) if need_alpha else None
        dtex = torch.empty_like(tex) if need_tex else None
        dview = None
        if need_view:
            dview = torch.empty((4, 4), dtype=torch.float32, device=dev)
            scratch = (torch.empty((_lib.gs_sky_scratch_bytes(Hs, Ws),), dtype=torch.uint8, device=dev)
                       if need_tex else None)
            cam_scratch = torch.empty((_lib.gs_sky_camera_scratch_bytes(W, H),), dtype=torch.uint8, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            with torch.cuda.device(dev):
                _native.check(_lib.gs_sky_compose_backward_camera(
                    W, H, _p(view), tfx, tfy, Hs, Ws, _p(tex), _p(alp), _p(g), _p(dalpha), _p(dtex), 0, _p(scratch),
                    _p(dview), 0, _p(cam_scratch), st), "sky backward")
        elif need_alpha or need_tex:
            scratch = (torch.empty((_lib.gs_sky_scratch_bytes(Hs, Ws),), dtype=torch.uint8, device=dev)
                       if need_tex else None)
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            with torch.cuda.device(dev):
                _native.check(_lib.gs_sky_compose_backward(W, H, _p(view), tfx, tfy, Hs, Ws, _p(tex), _p(alp), _p(g),
                                                           _p(dalpha), _p(dtex), 0, _p(scratch), st), "sky backward")
        if dalpha is not None:
            dalpha = dalpha.view(alpha_shape)
        return (g if need_color else None), dalpha, dtex, None, dview


def compose(color, alpha, texture, settings, camera_grads=False):
    """image [3, H, W] = color + (1 - alpha) * sky(texture) for the camera of `settings`
    (a GaussianRasterizationSettings: image size, tanfovx / tanfovy, viewmatrix).

    color [3, H, W] or None (0), alpha [H, W] / [1, H, W] or None (0), texture [3, Hs, Ws]; fp32
    device tensors.  Differentiable w.r.t. all three (dL/dcolor is the incoming gradient itself).

    camera_grads: a settings.viewmatrix that requires grad (a leaf or not; float32 [4, 4] on the
    texture's device) receives the sky's dL/dviewmatrix as well, row 3 and column 3 zero.  Without it,
    or with a matrix that does not require grad, the matrix is a constant: the call as it always was.
    tanfovx, tanfovy, projmatrix and campos get nothing from the sky."""
    V = settings.viewmatrix
    if camera_grads and isinstance(V, torch.Tensor) and V.requires_grad:
        if V.dtype != torch.float32 or tuple(V.shape) != (4, 4) or V.device != texture.device:
            raise ValueError("gs_sky.compose: camera_grads needs settings.viewmatrix as a float32 [4, 4] tensor on "
                             f"the texture's device (got {V.dtype} {tuple(V.shape)} on {V.device})")
        return _Compose.apply(color, alpha, texture, settings, V)
    return _Compose.apply(color, alpha, texture, settings, None)


class SkySphere(torch.nn.Module):
    """A learnable equirectangular sky: `texture` is an nn.Parameter [3, Hs, Ws] (row 0 at world -y,
    columns around the world y axis starting at -z)."""

    def __init__(self, Hs=512, Ws=1024, init=0.5):
        super().__init__()
        if Hs < 1 or Ws < 1:
            raise ValueError(f"SkySphere: texture size must be positive (got {Hs} x {Ws})")
        self.texture = torch.nn.Parameter(torch.full((3, int(Hs), int(Ws)), float(init), dtype=torch.float32))

    def forward(self, color, alpha, settings, camera_grads=False):
        return compose(color, alpha, self.texture, settings, camera_grads)

    def render(self, settings, camera_grads=False):
        """The bare sky of the camera, [3, H, W] (no splats: colour 0, alpha 0)."""
        return compose(None, None, self.texture, settings, camera_grads)


def render_with_sky(rasterizer, sky, camera_grads=False, **inputs):
    """One render with the sky behind the splats: calls `rasterizer(**inputs, aux_outputs=True)` and
    composes its colour and alpha with `sky` (a SkySphere).  Returns (image, radii, invdepth, alpha).
    The rasterizer's own background must be zero: it is already part of `color`, and a non-zero one
    would be added on top of the sky.

    camera_grads=True goes to both calls: the camera tensors of the settings that require grad get the
    rasterizer's gradients, and the view matrix the sky's share on top (autograd adds the two).  The
    rasterizer's refusals (prepared views, split SH rows, deferring gradient owners) are its own."""
    s = rasterizer.raster_settings
    if bool((s.bg != 0).any()):
        raise ValueError("render_with_sky: settings.bg must be all zeros (the sky is the background)")
    if not camera_grads:
        color, radii, invdepth, alpha = rasterizer(**inputs, aux_outputs=True)
        return sky(color, alpha, s), radii, invdepth, alpha
    color, radii, invdepth, alpha = rasterizer(**inputs, aux_outputs=True, camera_grads=True)
    return sky(color, alpha, s, camera_grads=True), radii, invdepth, alpha
