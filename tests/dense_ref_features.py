"""Dense reference of feature rendering and its gradient in the features (test infrastructure).

features_local consumes dense_ref.walk_local -- the same _prep, the same decisions, the same `flag` map
with flag_rel / flag_T_rel as dense_ref_contrib.contributions_local -- with C channels in the input dtype.
With w_i(p) = alpha_i(p) T_i(p) over the pixels where Gaussian i is composited (`ok` of the walk,
the entry that stops a pixel excluded),

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
    dt, dev = means3D.dtype, means3D.device
    P = means3D.shape[0]
    f = features.to(dev, dt)
    C = f.shape[1]
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    walk = dense_ref.walk_local(q, False, flag_rel, flag_T_rel)
    npx = W * H
    out = torch.zeros((C, npx), dtype=dt, device=dev)
    kept = []
    for i, idx, _, _, _, alpha, Ti, ok in walk:
        w = (alpha * Ti) * ok.to(dt)
        out[:, idx] += f[i][:, None] * w[None, :]
        kept.append((i, idx, w))
    flag = walk.flag
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
    return dict(out=out.reshape(C, H, W), dfeat=dfeat, flag=flag.reshape(H, W), radii=q["radii"], g=gg)
