"""The antialiasing opacity scale for the dense reference (test infrastructure).

aa_scale restates the raw EWA covariance exactly as dense_ref._prep forms it (the 1.3x FoV clamp, a
clamped tx / ty detached, `view` a tensor so that it can be a leaf) and returns

    s = sqrt(max(0.000025, det S / det(S + 0.3 I)))

in the caller's dtype.  The antialiased reference render is then dense_ref.render_local (or
dense_ref_aux.render_local_aux) fed `opac * s[:, None]`: autograd carries the chain to the
covariance, the mean and the view matrix.  aa_closed_form is the backward the kernels implement
(DESIGN.md §2), for the CPU check against autograd.  dense_ref.py itself is not modified."""
from __future__ import annotations

import torch

import dense_ref

AA_FLOOR = 0.000025


def raw_cov2d(means3D, view, tanfovx, tanfovy, W, H, scales=None, rots=None, cov3D=None, mod=1.0):
    """(c00, c01, c11) before the 0.3 dilation, as dense_ref._prep."""
    dt = means3D.dtype
    P = means3D.shape[0]
    ones = torch.ones((P, 1), dtype=dt, device=means3D.device)
    p_view = torch.cat([means3D, ones], 1) @ view
    if cov3D is None:
        R = dense_ref.quat_R(rots)
        L = R * (mod * scales)[:, None, :]
        Sig = L @ L.transpose(1, 2)
    else:
        c = cov3D
        Sig = torch.stack([torch.stack([c[:, 0], c[:, 1], c[:, 2]], -1), torch.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                           torch.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], -2)
    fx, fy = W / (2 * tanfovx), H / (2 * tanfovy)
    tz = p_view[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = p_view[:, 0] / tz, p_view[:, 1] / tz
    tx = torch.clamp(txtz, -limx, limx) * tz
    ty = torch.clamp(tytz, -limy, limy) * tz
    tx = torch.where(txtz.abs() > limx, tx.detach(), tx)
    ty = torch.where(tytz.abs() > limy, ty.detach(), ty)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / tz ** 2], -1),
                     torch.stack([zero, fy / tz, -fy * ty / tz ** 2], -1)], -2)
    T = J @ view[:3, :3].T
    cov2 = T @ Sig @ T.transpose(1, 2)
    return cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]


def scale_of(c00, c01, c11):
    """(s, r) of a raw covariance."""
    D0 = c00 * c11 - c01 * c01
    D = (c00 + 0.3) * (c11 + 0.3) - c01 * c01
    r = D0 / D
    return torch.sqrt(torch.clamp(r, min=AA_FLOOR)), r


def aa_scale(means3D, view, tanfovx, tanfovy, W, H, scales=None, rots=None, cov3D=None, mod=1.0, with_ratio=False):
    """s [P] (and r [P] with with_ratio) in means3D's dtype."""
    s, r = scale_of(*raw_cov2d(means3D, view, tanfovx, tanfovy, W, H, scales, rots, cov3D, mod))
    return (s, r) if with_ratio else s


def aa_closed_form(op, g, c00, c01, c11):
    """The kernels' backward of op' = op s for g = dL/dop': (dL/dop, dL/dc00, dL/dc01, dL/dc11)."""
    a, c = c00 + 0.3, c11 + 0.3
    D0 = c00 * c11 - c01 * c01
    D = a * c - c01 * c01
    r = D0 / D
    s = torch.sqrt(torch.clamp(r, min=AA_FLOOR))
    gr = torch.where(r > AA_FLOOR, (op * g) / (2 * s), torch.zeros_like(r))
    return (s * g, gr * (c11 * D - D0 * c) / D ** 2, gr * (-2 * c01 * (D - D0)) / D ** 2,
            gr * (c00 * D - D0 * a) / D ** 2)
