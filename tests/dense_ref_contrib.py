"""Dense reference of the per-Gaussian contribution statistics (test infrastructure).

contributions_local consumes dense_ref.walk_local -- the same _prep, the same decisions, the same `flag`
map with flag_rel / flag_T_rel as dense_ref.render_local -- and keeps, per Gaussian i and for a weight map m,

    wsum[i]  = sum_p m_p alpha_i(p) T_i(p)
    wmax[i]  = max_p m_p alpha_i(p) T_i(p)     (0 if i is never composited)
    count[i] = #{p : i composited at p and m_p != 0}

over the pixels where i is composited (`ok` of the walk: inside the tile rectangle, the pixel
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
    dt, dev = means3D.dtype, means3D.device
    P = means3D.shape[0]
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    walk = dense_ref.walk_local(q, False, flag_rel, flag_T_rel)
    m = torch.ones(W * H, dtype=dt, device=dev) if weights is None else weights.to(dev, dt).reshape(-1)
    wsum = torch.zeros(P, dtype=dt, device=dev)
    wmax = torch.zeros(P, dtype=dt, device=dev)
    count = torch.zeros(P, dtype=torch.int64, device=dev)
    kept = [(i, idx, (alpha * Ti) * ok.to(dt), ok) for i, idx, _, _, _, alpha, Ti, ok in walk]
    flag = walk.flag
    if zero_flagged:
        bad = flag if also_flag is None else flag | also_flag.to(dev).reshape(-1)
        m = m * (~bad).to(dt)
    for i, idx, w, ok in kept:
        mw = m[idx] * w
        wsum[i] = mw.sum()
        wmax[i] = mw.max() if mw.numel() else 0.0
        count[i] = (ok & (m[idx] != 0)).sum()
    return dict(wsum=wsum, wmax=wmax, count=count, radii=q["radii"], flag=flag.reshape(H, W),
                alpha=(1.0 - walk.T).reshape(H, W), weights=m.reshape(H, W))
