"""Dense reference of feature rendering and its gradient in the features (test infrastructure).

features_local restates dense_ref_contrib.contributions_local's loop -- the same _prep, the same
decisions, the same `flag` map with flag_rel / flag_T_rel -- with C channels in the input dtype.
With w_i(p) = alpha_i(p) T_i(p) over the pixels where Gaussian i is composited (`ok` of the colour
loop, the entry that stops a pixel excluded),

    out[c, p]   = sum_i f_i[c] w_i(p)               front to back, no background term
    dfeat[i, c] = sum_p w_i(p) g_c(p)               for a given image gradient g [C, H, W]

zero_flagged: g is zeroed at the pixels of the returned flag map (and of `also_flag`) before dfeat is
formed -- the flags are only complete after the loop, so each Gaussian's (pixels, alpha T) is kept and
applied afterwards; the gradient used is returned as `g`.  No graph is kept.
"""
from __future__ import annotations

import torch

import dense_ref


@torch.no_grad()
def features_local(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, features, g=None, shs=None,
                   deg=0, colors=None, scales=None, rots=None, cov3D=None, mod=1.0, flag_rel=1e-5, flag_T_rel=None,
                   zero_flagged=False, also_flag=None):
    """-> dict(out [C, H, W], dfeat [P, C] (input dtype; None without g), flag [H, W] bool,
    radii [P] int32, g [C, H, W] as used).  features: [P, C]; also_flag: bool [H, W] or None."""
    flag_T_rel = flag_rel if flag_T_rel is None else flag_T_rel
    dt, dev = means3D.dtype, means3D.device
    P = means3D.shape[0]
    f = features.to(dev, dt)
    C = f.shape[1]
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    pix, conic, x0, y0, x1, y1, radii, order = (q[k] for k in ("pix", "conic", "x0", "y0", "x1", "y1", "radii",
                                                                "order"))
    npx = W * H
    Tr = torch.ones(npx, dtype=dt, device=dev)
    done = torch.zeros(npx, dtype=torch.bool, device=dev)
    flag = torch.zeros(npx, dtype=torch.bool, device=dev)
    out = torch.zeros((C, npx), dtype=dt, device=dev)
    rect = torch.stack([x0, y0, x1, y1], 1).to(torch.int64).cpu()
    kept = []
    for i in order:
        rx0, ry0, rx1, ry1 = (int(v) for v in rect[i])
        xs = torch.arange(16 * rx0, min(16 * rx1, W), device=dev)
        ys = torch.arange(16 * ry0, min(16 * ry1, H), device=dev)
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        idx = (yy * W + xx).reshape(-1)
        dx, dy = pix[i, 0] - xx.reshape(-1).to(dt), pix[i, 1] - yy.reshape(-1).to(dt)
        power = -0.5 * (conic[i, 0] * dx * dx + conic[i, 2] * dy * dy) - conic[i, 1] * dx * dy
        alpha = torch.clamp(opac[i] * torch.exp(power), max=0.99)
        Ti = Tr[idx]
        live = ~done[idx]
        ok = live & (power <= 0) & (alpha >= 1.0 / 255.0)
        test_T = Ti * (1 - alpha)
        stop = ok & (test_T < 1e-4)
        near = live & (((alpha - 1.0 / 255.0).abs() <= flag_rel / 255.0) | (power.abs() <= 1e-6)
                       | (ok & ((test_T - 1e-4).abs() <= flag_T_rel * 1e-4)))
        flag[idx] |= near
        ok = ok & ~stop
        done[idx] |= stop
        w = (alpha * Ti) * ok.to(dt)
        out[:, idx] += f[i][:, None] * w[None, :]
        kept.append((i, idx, w))
        Tr[idx] = torch.where(ok, test_T, Ti)
    dfeat, gg = None, None
    if g is not None:
        gg = g.to(dev, dt).reshape(C, npx)
        if zero_flagged:
            bad = flag if also_flag is None else flag | also_flag.to(dev).reshape(-1)
            gg = gg * (~bad).to(dt)[None, :]
        dfeat = torch.zeros((P, C), dtype=dt, device=dev)
        for i, idx, w in kept:
            dfeat[i] = gg[:, idx] @ w
        gg = gg.reshape(C, H, W)
    return dict(out=out.reshape(C, H, W), dfeat=dfeat, flag=flag.reshape(H, W), radii=radii, g=gg)
