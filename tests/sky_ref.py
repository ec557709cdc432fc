"""The skysphere definition (include/gsrast.h, gs_sky.py) in plain torch with autograd, in any
float dtype: the reference of tests/test_sky_cpu.py and tests/test_gpu_sky.py.

    d_cam = (((2x + 1) / W - 1) tanfovx, ((2y + 1) / H - 1) tanfovy, 1)
    d_i   = sum_j V[i][j] d_cam_j
    u = atan2(d.x, d.z) / 2pi + 0.5,  v = acos(clamp(-d.y / |d|, -1, 1)) / pi
    tx = u Ws - 0.5, ty = v Hs - 0.5; columns floor(tx), floor(tx) + 1 wrap, rows floor(ty),
    floor(ty) + 1 clamp; bilinear weights from the fractions
    image = color + (1 - alpha) sky

Run in float64 it is the exact reference, in float32 the measure of what fp32 arithmetic can give
(the conditioning term of the GPU tests' bound)."""
import math

import torch


def directions(viewmatrix, tanfovx, tanfovy, W, H, dtype=torch.float64, device="cpu"):
    """World rays [H, W, 3] of the pixel centres."""
    V = viewmatrix.detach().to(device, dtype)
    x = torch.arange(W, dtype=dtype, device=device)
    y = torch.arange(H, dtype=dtype, device=device)
    cx = (((2 * x + 1) / W - 1) * tanfovx)[None, :].expand(H, W)
    cy = (((2 * y + 1) / H - 1) * tanfovy)[:, None].expand(H, W)
    return torch.stack([V[i, 0] * cx + V[i, 1] * cy + V[i, 2] for i in range(3)], dim=-1)


def taps(dirs, Hs, Ws):
    """(xa, xb, ya, yb, fx, fy) of every ray: wrapped columns, clamped rows, fractions."""
    dx, dy, dz = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    u = torch.atan2(dx, dz) / (2 * math.pi) + 0.5
    v = torch.acos(torch.clamp(-dy / dirs.norm(dim=-1), -1.0, 1.0)) / math.pi
    tx, ty = u * Ws - 0.5, v * Hs - 0.5
    x0f, y0f = torch.floor(tx), torch.floor(ty)
    x0, y0 = x0f.long(), y0f.long()
    return (torch.remainder(x0, Ws), torch.remainder(x0 + 1, Ws), y0.clamp(0, Hs - 1), (y0 + 1).clamp(0, Hs - 1),
            tx - x0f, ty - y0f)


def sample(texture, dirs):
    """Bilinear sky colour [3, H, W] of the rays, differentiable w.r.t. the texture."""
    Hs, Ws = texture.shape[1], texture.shape[2]
    xa, xb, ya, yb, fx, fy = taps(dirs, Hs, Ws)
    t00, t01, t10, t11 = texture[:, ya, xa], texture[:, ya, xb], texture[:, yb, xa], texture[:, yb, xb]
    top = t00 + fx * (t01 - t00)
    bot = t10 + fx * (t11 - t10)
    return top + fy * (bot - top)


def compose(color, alpha, texture, viewmatrix, tanfovx, tanfovy, dtype=torch.float64):
    """image [3, H, W] = color + (1 - alpha) sky in `dtype`, on the device of `color`; color [3, H, W],
    alpha [H, W] and texture [3, Hs, Ws] are used as given (cast them to `dtype` and set requires_grad
    first)."""
    H, W = color.shape[1], color.shape[2]
    dirs = directions(viewmatrix, tanfovx, tanfovy, W, H, dtype, color.device)
    return color + (1 - alpha) * sample(texture, dirs)


def reference(color, alpha, texture, g, viewmatrix, tanfovx, tanfovy, dtype):
    """(image, dL/dalpha, dL/dtexture) for L = sum g image, as CPU tensors of `dtype`."""
    c = color.detach().to("cpu", dtype)
    a = alpha.detach().to("cpu", dtype).reshape(c.shape[1], c.shape[2]).requires_grad_(True)
    t = texture.detach().to("cpu", dtype).requires_grad_(True)
    img = compose(c, a, t, viewmatrix, tanfovx, tanfovy, dtype)
    (img * g.detach().to("cpu", dtype)).sum().backward()
    return img.detach(), a.grad, t.grad
