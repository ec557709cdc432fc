"""Dense reference of the absolute screen-space gradient (test infrastructure).

absgrad_local consumes dense_ref.walk_local -- the same _prep, the same decisions, the same `flag` map with
flag_rel / flag_T_rel as dense_ref.render_local -- in two passes and without autograd:

  front to back  each Gaussian i keeps its pixels, d = mean2D_i - p, o G, alpha = min(0.99, o G), the
                 transmittance T_i in front of it and `ok` (composited: inside the tile rectangle, the pixel
                 live, power <= 0, alpha >= 1/255, not the entry that stops the pixel);
  back to front  per pixel S_i = sum_{j behind i} (g . c_j) alpha_j T_j + T_final (g . bg), so that
                     dL/dalpha_i(p) = T_i (g . c_i) - S_i / (1 - alpha_i)
                 where g . c runs over the colour channels, alpha (a channel of colour 1 and background 0:
                 sum_j alpha_j T_j = 1 - T_final) and the inverse depth (one of colour 1 / z_i and background 0).

With q = o G dL/dalpha (the clamp does not gate the gradient) and the conic (cxx, cxy, cyy),

    a_x(i, p) = |q (cxx dx + cxy dy)|                 a_y(i, p) = |q (cxy dx + cyy dy)|
    abs[i]    = (0.5 W sum_p a_x, 0.5 H sum_p a_y, 0)
    signed[i] = (-0.5 W sum_p q (cxx dx + cxy dy), -0.5 H sum_p q (cxy dx + cyy dy), 0)

signed is dL/dmeans2D (power's derivative in dx is -(cxx dx + cxy dy)); tests/test_absgrad_cpu.py checks it
against fp64 autograd of dense_ref.render_local, which proves the closed form.

zero_flagged: dL/dimage (and the aux gradients) are zeroed at the pixels of the returned flag map (and of
`also_flag`) before the second pass; the pixel mask used is returned as `keep`.
"""
from __future__ import annotations

import torch

import dense_ref


@torch.no_grad()
def absgrad_local(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, bg, dL_dimage, shs=None, deg=0,
                  colors=None, scales=None, rots=None, cov3D=None, mod=1.0, dL_dalpha=None, dL_dinvdepth=None,
                  flag_rel=1e-5, flag_T_rel=None, zero_flagged=False, also_flag=None):
    """-> dict(abs [P, 3], signed [P, 3] (input dtype), radii [P] int32, flag [H, W] bool, keep [H, W] bool,
    rect [P, 4] int64 (x0, y0, x1, y1 in tiles)).  dL_dimage [3, H, W]; dL_dalpha /
    dL_dinvdepth [H, W] or [1, H, W] or None."""
    dt, dev = means3D.dtype, means3D.device
    P = means3D.shape[0]
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    conic, rgb, tz = q["conic"], q["rgb"], q["tz"]
    walk = dense_ref.walk_local(q, False, flag_rel, flag_T_rel)
    kept = list(walk)
    npx, flag, Tr = W * H, walk.flag, walk.T

    keep = torch.ones(npx, dtype=torch.bool, device=dev)
    if zero_flagged:
        keep = ~(flag if also_flag is None else flag | also_flag.to(dev).reshape(-1))
    kf = keep.to(dt)
    g = dL_dimage.to(dev, dt).reshape(3, npx) * kf[None]
    gA = None if dL_dalpha is None else dL_dalpha.to(dev, dt).reshape(npx) * kf
    gD = None if dL_dinvdepth is None else dL_dinvdepth.to(dev, dt).reshape(npx) * kf
    S = Tr * (g * bg.to(dev, dt)[:, None]).sum(0)  # the background's term: T_final (g . bg)
    out_abs = torch.zeros((P, 3), dtype=dt, device=dev)
    out_sgn = torch.zeros((P, 3), dtype=dt, device=dev)
    for i, idx, dx, dy, a_raw, alpha, Ti, ok in reversed(kept):
        okf = ok.to(dt)
        gc = (g[:, idx] * rgb[i][:, None]).sum(0)
        if gA is not None:
            gc = gc + gA[idx]
        if gD is not None:
            gc = gc + gD[idx] / tz[i]
        dLda = Ti * gc - S[idx] / (1 - alpha)
        qq = a_raw * dLda * okf
        bx = conic[i, 0] * dx + conic[i, 1] * dy
        by = conic[i, 1] * dx + conic[i, 2] * dy
        out_abs[i, 0] = 0.5 * W * (qq * bx).abs().sum()
        out_abs[i, 1] = 0.5 * H * (qq * by).abs().sum()
        out_sgn[i, 0] = -0.5 * W * (qq * bx).sum()
        out_sgn[i, 1] = -0.5 * H * (qq * by).sum()
        S[idx] += gc * (alpha * Ti) * okf
    return dict(abs=out_abs, signed=out_sgn, radii=q["radii"], flag=flag.reshape(H, W), keep=keep.reshape(H, W),
                rect=q["rect"])


@torch.no_grad()
def half_planes(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs=None, deg=0, colors=None,
                scales=None, rots=None, cov3D=None, mod=1.0):
    """For scenes of splats whose tile rectangles do not overlap: bool maps [H, W] of the pixels where the
    splat that owns the pixel's tile has cxx dx + cxy dy > 0 (`x`) resp. cxy dx + cyy dy > 0 (`y`), False
    outside every rectangle; and `overlap`, whether two rectangles share a tile."""
    dt, dev = means3D.dtype, means3D.device
    q = dense_ref._prep(means3D, means2D, opac, view, proj, campos, tanfovx, tanfovy, W, H, shs, deg, colors, scales,
                        rots, cov3D, mod)
    pix, conic = q["pix"], q["conic"]
    owner = torch.zeros((H, W), dtype=torch.int64, device=dev)
    hx = torch.zeros((H, W), dtype=torch.bool, device=dev)
    hy = torch.zeros((H, W), dtype=torch.bool, device=dev)
    for i in q["order"]:
        yy, xx = dense_ref.rect_pixels(q["rect"][i], W, H, dev)
        owner[yy, xx] += 1
        dx, dy = pix[i, 0] - xx.to(dt), pix[i, 1] - yy.to(dt)
        hx[yy, xx] = conic[i, 0] * dx + conic[i, 1] * dy > 0
        hy[yy, xx] = conic[i, 1] * dx + conic[i, 2] * dy > 0
    return dict(x=hx, y=hy, overlap=bool((owner > 1).any()), radii=q["radii"])
