"""dense_ref.render_local with the two aux outputs (test infrastructure).

render_local_aux consumes the same walk as render_local (dense_ref.walk_local: same per-Gaussian half,
same decisions and flags) with two more accumulators:

    invdepth(p) = sum_i (1 / tz_i) alpha_i T_i     (a colour channel of colour 1 / tz_i, no background)
    alpha(p)    = 1 - T_final(p)

tz_i is the view depth _prep returns, differentiable with respect to means3D, so autograd carries
the depth chain."""
from __future__ import annotations

import torch

import dense_ref


def render_local_aux(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, bg, shs=None, deg=0,
                     colors=None, scales=None, rots=None, cov3D=None, mod=1.0, flag_rel=1e-5, flag_T_rel=None):
    """Returns (img [3, H, W], radii [P], flag [H, W], invdepth [1, H, W], alpha [1, H, W])."""
    dt, dev = means3D.dtype, means3D.device
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    walk = dense_ref.walk_local(q, True, flag_rel, flag_T_rel)
    C = torch.zeros((3, W * H), dtype=dt, device=dev)
    D = torch.zeros(W * H, dtype=dt, device=dev)
    for i, idx, _, _, _, alpha, Ti, ok in walk:
        w = alpha * Ti * ok.to(dt)
        C = C.index_add(1, idx, q["rgb"][i][:, None] * w[None])
        D = D.index_add(0, idx, (1.0 / q["tz"][i]) * w)
    img = C + walk.T[None] * bg[:, None]
    return (img.reshape(3, H, W), q["radii"], walk.flag.reshape(H, W), D.reshape(1, H, W),
            (1.0 - walk.T).reshape(1, H, W))
