"""The skysphere's view-matrix gradient in plain torch: sky_ref's taps and sample along rays built
from a leaf V, so that autograd gives dL/dV in any float dtype (sky_ref.directions detaches V).
floor gives the taps no gradient (they are integer tensors and the fractions tx - floor(tx)).

    d_cam = (cx, cy, 1),  d_i = sum_j V[i][j] d_cam_j  (i, j < 3: row 3 and column 3 of dL/dV are zeros)
    L = sum g (color + (1 - alpha) sample(texture, d))

Flagged pixels: the sample's slope jumps where tx or ty crosses a texel boundary, and 1 / rho
amplifies every rounding next to a pole, so an fp32 evaluation may differ there by more than
rounding.  `flagged` marks, from the fp64 rays, the pixels with tx or ty within
eps = max(1e-3, 32 2^-24 Ws) texels of an integer or with rho / |d| < 0.05; every comparison zeroes
dL/dimage there (a zero adds nothing to any sum: all other pixels are still checked)."""
import math

import torch

import sky_ref

FLAG_CAP = 0.02  # at most this share of a case's pixels may be flagged
POLE = 0.05


def directions(V, tanfovx, tanfovy, W, H):
    """World rays [H, W, 3] of the pixel centres in V's dtype and on its device, differentiable w.r.t. V."""
    x = torch.arange(W, dtype=V.dtype, device=V.device)
    y = torch.arange(H, dtype=V.dtype, device=V.device)
    cx = (((2 * x + 1) / W - 1) * tanfovx)[None, :].expand(H, W)
    cy = (((2 * y + 1) / H - 1) * tanfovy)[:, None].expand(H, W)
    return torch.stack([V[i, 0] * cx + V[i, 1] * cy + V[i, 2] for i in range(3)], dim=-1)


def sky(texture, V, tanfovx, tanfovy, W, H):
    """The sky's colour [3, H, W], differentiable w.r.t. the texture and V."""
    return sky_ref.sample(texture, directions(V, tanfovx, tanfovy, W, H))


def flagged(viewmatrix, tanfovx, tanfovy, W, H, Hs, Ws):
    """bool [H, W] (CPU): the pixels left out of every comparison (module docstring)."""
    d = directions(viewmatrix.detach().to("cpu", torch.float64), tanfovx, tanfovy, W, H)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    norm = d.norm(dim=-1)
    tx = (torch.atan2(dx, dz) / (2 * math.pi) + 0.5) * Ws - 0.5
    ty = torch.acos(torch.clamp(-dy / norm, -1.0, 1.0)) / math.pi * Hs - 0.5
    eps = max(1e-3, 32 * 2.0 ** -24 * Ws)
    near = ((tx - torch.round(tx)).abs() < eps) | ((ty - torch.round(ty)).abs() < eps)
    pole = torch.sqrt(dx * dx + dz * dz) / norm < POLE
    return near | pole | ~torch.isfinite(tx) | ~torch.isfinite(ty)


def loss(alpha, texture, g, V, tanfovx, tanfovy):
    """sum g (1 - alpha) sky in V's dtype (the colour's term does not depend on V); alpha may be None."""
    H, W = g.shape[1], g.shape[2]
    om = 1 if alpha is None else 1 - alpha.reshape(H, W)
    return (g * (om * sky(texture, V, tanfovx, tanfovy, W, H))).sum()


def view_grad(alpha, texture, g, viewmatrix, tanfovx, tanfovy, dtype, device="cpu"):
    """dL/dviewmatrix [4, 4] in `dtype` by autograd with V as a leaf."""
    cast = lambda t: None if t is None else t.detach().to(device, dtype)  # noqa: E731
    V = cast(viewmatrix).clone().requires_grad_(True)
    loss(cast(alpha), cast(texture), cast(g), V, tanfovx, tanfovy).backward()
    return V.grad
