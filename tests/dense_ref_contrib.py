"""Dense reference of the per-Gaussian contribution statistics (test infrastructure).

contributions_local restates dense_ref.render_local's loop -- the same _prep, the same decisions, the
same `flag` map with flag_rel / flag_T_rel -- and keeps, per Gaussian i and for a weight map m,

    wsum[i]  = sum_p m_p alpha_i(p) T_i(p)
    wmax[i]  = max_p m_p alpha_i(p) T_i(p)     (0 if i is never composited)
    count[i] = #{p : i composited at p and m_p != 0}

over the pixels where i is composited (`ok` of the colour loop: inside the tile rectangle, the pixel
still live, power <= 0, alpha >= 1/255, and not the entry that stops the pixel).  It also returns the
alpha map 1 - T_final, so that sum_i wsum[i] = sum_p m_p alpha_p telescopes.  No graph is kept.

zero_flagged: the weight map is zeroed at the pixels of the returned flag map (and of `also_flag`)
before the statistics are formed -- the flags are only complete after the loop, so each Gaussian's
(pixels, alpha T, composited) is kept and weighted afterwards; the map used is returned as `weights`.
"""
from __future__ import annotations

import torch

import dense_ref


@torch.no_grad()
def contributions_local(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, weights=None, shs=None,
                        deg=0, colors=None, scales=None, rots=None, cov3D=None, mod=1.0, flag_rel=1e-5,
                        flag_T_rel=None, zero_flagged=False, also_flag=None):
    """-> dict(wsum [P], wmax [P] (input dtype), count [P] int64, radii [P] int32, flag [H, W] bool,
    alpha [H, W], weights [H, W]).  weights: [H, W] (None: ones); also_flag: bool [H, W] or None."""
    flag_T_rel = flag_rel if flag_T_rel is None else flag_T_rel
    dt, dev = means3D.dtype, means3D.device
    P = means3D.shape[0]
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    pix, conic, x0, y0, x1, y1, radii, order = (q[k] for k in ("pix", "conic", "x0", "y0", "x1", "y1", "radii",
                                                                "order"))
    npx = W * H
    m = torch.ones(npx, dtype=dt, device=dev) if weights is None else weights.to(dev, dt).reshape(-1)
    Tr = torch.ones(npx, dtype=dt, device=dev)
    done = torch.zeros(npx, dtype=torch.bool, device=dev)
    flag = torch.zeros(npx, dtype=torch.bool, device=dev)
    wsum = torch.zeros(P, dtype=dt, device=dev)
    wmax = torch.zeros(P, dtype=dt, device=dev)
    count = torch.zeros(P, dtype=torch.int64, device=dev)
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
        kept.append((i, idx, (alpha * Ti) * ok.to(dt), ok))
        Tr[idx] = torch.where(ok, test_T, Ti)
    if zero_flagged:
        bad = flag if also_flag is None else flag | also_flag.to(dev).reshape(-1)
        m = m * (~bad).to(dt)
    for i, idx, w, ok in kept:
        mw = m[idx] * w
        wsum[i] = mw.sum()
        wmax[i] = mw.max() if mw.numel() else 0.0
        count[i] = (ok & (m[idx] != 0)).sum()
    return dict(wsum=wsum, wmax=wmax, count=count, radii=radii, flag=flag.reshape(H, W),
                alpha=(1.0 - Tr).reshape(H, W), weights=m.reshape(H, W))
