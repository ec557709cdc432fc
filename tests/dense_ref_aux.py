"""dense_ref.render_local with the two aux outputs (test infrastructure).

render_local_aux restates render_local's loop (same per-Gaussian half, dense_ref._prep, same
decisions and flags) with two more accumulators:

    invdepth(p) = sum_i (1 / tz_i) alpha_i T_i     (a colour channel of colour 1 / tz_i, no background)
    alpha(p)    = 1 - T_final(p)

tz_i is the view depth _prep returns, differentiable with respect to means3D, so autograd carries
the depth chain.  dense_ref.py itself is not modified."""
from __future__ import annotations

import torch

import dense_ref


def render_local_aux(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, bg, shs=None, deg=0,
                     colors=None, scales=None, rots=None, cov3D=None, mod=1.0, flag_rel=1e-5, flag_T_rel=None):
    """Returns (img [3, H, W], radii [P], flag [H, W], invdepth [1, H, W], alpha [1, H, W])."""
    flag_T_rel = flag_rel if flag_T_rel is None else flag_T_rel
    dt, dev = means3D.dtype, means3D.device
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    pix, conic, rgb, tz, x0, y0, x1, y1, radii, order = (q[k] for k in ("pix", "conic", "rgb", "tz", "x0", "y0", "x1",
                                                                         "y1", "radii", "order"))
    npx = W * H
    Tr = torch.ones(npx, dtype=dt, device=dev)
    C = torch.zeros((3, npx), dtype=dt, device=dev)
    D = torch.zeros(npx, dtype=dt, device=dev)
    done = torch.zeros(npx, dtype=torch.bool, device=dev)
    flag = torch.zeros(npx, dtype=torch.bool, device=dev)
    rect = torch.stack([x0, y0, x1, y1], 1).to(torch.int64).cpu()
    for i in order:
        rx0, ry0, rx1, ry1 = (int(v) for v in rect[i])
        xs = torch.arange(16 * rx0, min(16 * rx1, W), device=dev)
        ys = torch.arange(16 * ry0, min(16 * ry1, H), device=dev)
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        idx = (yy * W + xx).reshape(-1)
        dx, dy = pix[i, 0] - xx.reshape(-1).to(dt), pix[i, 1] - yy.reshape(-1).to(dt)
        power = -0.5 * (conic[i, 0] * dx * dx + conic[i, 2] * dy * dy) - conic[i, 1] * dx * dy
        a_raw = opac[i] * torch.exp(power)
        alpha = a_raw - torch.clamp(a_raw.detach() - 0.99, min=0.0)   # min(0.99, .), straight-through grad
        Ti = Tr[idx]
        with torch.no_grad():
            live = ~done[idx]
            ok = live & (power <= 0) & (alpha >= 1.0 / 255.0)
            test_T = Ti * (1 - alpha)
            stop = ok & (test_T < 1e-4)
            near = live & (((alpha - 1.0 / 255.0).abs() <= flag_rel / 255.0) | (power.abs() <= 1e-6)
                           | (ok & ((test_T - 1e-4).abs() <= flag_T_rel * 1e-4)))
            flag[idx] |= near
            ok = ok & ~stop
            done[idx] |= stop
        w = alpha * Ti * ok.to(dt)
        C = C.index_add(1, idx, rgb[i][:, None] * w[None])
        D = D.index_add(0, idx, (1.0 / tz[i]) * w)
        Tr = Tr.index_put((idx,), torch.where(ok, Ti * (1 - alpha), Ti))
    img = C + Tr[None] * bg[:, None]
    return img.reshape(3, H, W), radii, flag.reshape(H, W), D.reshape(1, H, W), (1.0 - Tr).reshape(1, H, W)
