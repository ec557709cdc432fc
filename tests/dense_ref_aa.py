"""The antialiasing opacity scale for the dense reference (test infrastructure).

aa_scale takes the raw EWA covariance from dense_ref.raw_cov2, which dense_ref._prep also calls (the 1.3x FoV
clamp, a clamped tx / ty detached, `view` a tensor so that it can be a leaf), and returns

    s = sqrt(max(0.000025, det S / det(S + 0.3 I)))

in the caller's dtype.  The antialiased reference render is then dense_ref.render_local (or
dense_ref_aux.render_local_aux) fed `opac * s[:, None]`: autograd carries the chain to the
covariance, the mean and the view matrix.  aa_closed_form is the backward the kernels implement
(DESIGN.md §2), for the CPU check against autograd."""
from __future__ import annotations

import torch

import dense_ref

AA_FLOOR = 0.000025


def raw_cov2d(means3D, view, tanfovx, tanfovy, W, H, scales=None, rots=None, cov3D=None, mod=1.0):
    """(c00, c01, c11) before the 0.3 dilation, as dense_ref._prep."""
    cov2 = dense_ref.raw_cov2(means3D, view, tanfovx, tanfovy, W, H, scales, rots, cov3D, mod)[-1]
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
