"""Per-Gaussian contribution statistics and importance pruning on MI355X.

How much each Gaussian takes part in a rendered view, from one cheap walk over the forward's tile
lists (csrc/gs_contrib.hip, C ABI gs_contrib_stats) instead of a full backward.  With
w_i(p) = alpha_i(p) T_i(p) over the pixels where the colour forward composited Gaussian i (the entry
that stops a pixel is not composited, as upstream) and an optional per-pixel weight map m >= 0:

    wsum[i]  = sum_p m_p w_i(p)     the blending weight the view gives i (error-weighted with m = |error|)
    wmax[i]  = max_p m_p w_i(p)     the RadSplat / LightGaussian pruning score
    count[i] = #{p : i composited at p, m_p != 0}     the hit count

all exact per view and bitwise reproducible; a pixel of weight 0 adds nothing (a foreground mask).

    stats = accumulate_views([GaussianRasterizer(s) for s in settings], means3D=..., opacities=..., ...)
    keep = keep_mask(stats, min_count=1, min_wmax=0.02)
    prune(gaussians, keep)

The statistics come from the two-call forward (plain, or antialiased with antialiasing=True); they
are not defined for bounded (binning_capacity=), prepared (prepare_views) or graph-captured forwards.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from diff_gaussian_rasterization import _C, _contiguous_matrix

__all__ = ["Contributions", "view_contributions", "accumulate_views", "keep_mask", "prune"]


class Contributions(NamedTuple):
    wsum: torch.Tensor   # [P] fp32
    wmax: torch.Tensor   # [P] fp32
    count: torch.Tensor  # [P] int32
    radii: torch.Tensor  # [P] int32, of the (last) view


def _weights(pixel_weights, H, W, device):
    if pixel_weights is None:
        return None
    m = pixel_weights
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float32:
        raise ValueError("pixel_weights must be a float32 tensor")
    if tuple(m.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"pixel_weights must have shape ({H}, {W}) or (1, {H}, {W}) (got {tuple(m.shape)})")
    if m.device != device:
        raise ValueError(f"pixel_weights is on {m.device}, expected {device}")
    return m.contiguous()


def view_contributions(rasterizer, *, pixel_weights=None, out: Optional[Contributions] = None, antialiasing=False,
                       means3D, opacities, means2D=None, shs=None, colors_precomp=None, scales=None, rotations=None,
                       cov3D_precomp=None) -> Contributions:
    """The statistics of one view: the two-call forward of `rasterizer`'s settings on these inputs
    (the keywords of GaussianRasterizer.forward, same checks and exception texts; means2D is not
    read), then gs_contrib_stats.  No graph is recorded.  out: a Contributions to combine with in
    place (wsum += , wmax = max, count +=; radii replaced by this view's), which is returned."""
    s = rasterizer.raster_settings
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    _C.check_image_size(s.image_width, s.image_height)
    H, W = int(s.image_height), int(s.image_width)
    _C._dev_check(means3D, "means3D")
    m = _weights(pixel_weights, H, W, means3D.device)
    if out is not None:
        P = means3D.shape[0]
        for t, dt, n in zip(out[:3], (torch.float32, torch.float32, torch.int32), Contributions._fields):
            if t.dtype != dt or t.device != means3D.device or tuple(t.shape) != (P,) or not t.is_contiguous():
                raise ValueError(f"out.{n} must be a contiguous {dt} tensor of shape ({P},) on {means3D.device}")
    empty = torch.Tensor([])
    e = lambda t: empty if t is None else t.detach()  # noqa: E731
    with torch.no_grad():
        view, proj = _contiguous_matrix(s.viewmatrix), _contiguous_matrix(s.projmatrix)
        R, _color, radii, geom, binning, img = _C.rasterize_gaussians_two_call(
            s.bg, means3D.detach(), e(colors_precomp), opacities.detach(), e(scales), e(rotations), s.scale_modifier,
            e(cov3D_precomp), view, proj, s.tanfovx, s.tanfovy, H, W, e(shs), s.sh_degree, s.campos, s.prefiltered,
            s.debug, antialiasing=bool(antialiasing))
        stats = _C.contribution_stats(R, radii, geom, binning, img, view, proj, s.campos, s.tanfovx, s.tanfovy, H, W,
                                      debug=s.debug, pixel_weights=m, out=None if out is None else tuple(out[:3]))
    return Contributions(*stats, radii)


def accumulate_views(rasterizers, *, pixel_weights=None, **inputs) -> Contributions:
    """The statistics of several views of one set of Gaussians combined: wsum and count summed, wmax
    the maximum over the views.  pixel_weights: None, or one map (or None) per view."""
    rasterizers = list(rasterizers)
    if not rasterizers:
        raise ValueError("accumulate_views: no view")
    maps = [None] * len(rasterizers) if pixel_weights is None else list(pixel_weights)
    if len(maps) != len(rasterizers):
        raise ValueError("accumulate_views: one pixel_weights entry per view")
    stats = None
    for r, m in zip(rasterizers, maps):
        stats = view_contributions(r, pixel_weights=m, out=stats, **inputs)
    return stats


def keep_mask(stats, *, min_count=None, min_wmax=None, keep_fraction=None, score="wsum") -> torch.Tensor:
    """bool [P]: the Gaussians that pass every given test.  min_count: count >= min_count;
    min_wmax: wmax >= min_wmax; keep_fraction f: among the ceil(f P) largest by `score` ("wsum",
    "wmax" or "count"), ties broken by the lower index."""
    P = stats.wsum.shape[0]
    keep = torch.ones((P,), dtype=torch.bool, device=stats.wsum.device)
    if min_count is not None:
        keep &= stats.count >= min_count
    if min_wmax is not None:
        keep &= stats.wmax >= min_wmax
    if keep_fraction is not None:
        if not 0.0 <= keep_fraction <= 1.0:
            raise ValueError("keep_fraction must lie in [0, 1]")
        if score not in ("wsum", "wmax", "count"):
            raise ValueError(f"unknown score {score!r}")
        n = min(P, int(math.ceil(keep_fraction * P)))
        top = torch.argsort(getattr(stats, score), descending=True, stable=True)[:n]
        frac = torch.zeros_like(keep)
        frac[top] = True
        keep &= frac
    return keep


_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def prune(gaussians, keep: torch.Tensor) -> None:
    """Keep the rows of `gaussians` where `keep` (bool [P]) is set: the effect of the reference's
    GaussianModel.prune_points(~keep) on any object with the attributes and named optimizer groups
    that gs_train.densify_and_prune uses.  The six parameters become new nn.Parameters of the kept
    rows in order, the Adam moments follow ('step' kept), xyz_gradient_accum, denom and max_radii2D
    are sliced.  Sharded moments (gs_view_parallel.ShardedAdam) are refused until gathered, and a
    gradient bucket that owns the replaced parameters is rebound, as in densify_and_prune."""
    sharded = getattr(gaussians.optimizer, "_gs_sharded_moments", None)
    if sharded is not None and sharded.moments_sharded():
        raise RuntimeError("prune: the Adam moments are sharded over the ranks (gs_view_parallel.ShardedAdam); "
                           "call its gather_state() first")
    if sharded is not None:
        sharded.sync()  # an overlapped step's all-gathers, before the parameters are read here
    params = [getattr(gaussians, a) for a in _ATTRS]
    P = params[0].shape[0]
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
        raise ValueError("prune: keep must be a bool tensor")
    if tuple(keep.shape) != (P,):
        raise ValueError(f"prune: keep must have shape ({P},) (got {tuple(keep.shape)})")
    keep = keep.to(params[0].device)
    groups = {g["name"]: g for g in gaussians.optimizer.param_groups}
    for n, p in zip(_NAMES, params):
        if len(groups[n]["params"]) != 1 or groups[n]["params"][0] is not p:
            raise ValueError(f"prune: optimizer group '{n}' must hold exactly the model's tensor")
        if p.shape[0] != P:
            raise ValueError(f"prune: {n} has {p.shape[0]} rows, xyz has {P}")
    from diff_gaussian_rasterization import _sink_owner

    owners = []
    for p in params:
        o = _sink_owner(p)
        if o is not None and hasattr(o, "rebind") and all(o is not x for x in owners):
            owners.append(o)
    replaced = {}
    for n, a, old in zip(_NAMES, _ATTRS, params):
        newp = torch.nn.Parameter(old.detach()[keep].requires_grad_(True))
        state = gaussians.optimizer.state.get(old, None)
        if state is not None:
            state["exp_avg"] = state["exp_avg"][keep]
            state["exp_avg_sq"] = state["exp_avg_sq"][keep]
            del gaussians.optimizer.state[old]
            gaussians.optimizer.state[newp] = state
        groups[n]["params"][0] = newp
        setattr(gaussians, a, newp)
        replaced[id(old)] = newp
    for o in owners:
        o.rebind([replaced.get(id(p), p) for p in o.params])
    gaussians.xyz_gradient_accum = gaussians.xyz_gradient_accum[keep]
    gaussians.denom = gaussians.denom[keep]
    gaussians.max_radii2D = gaussians.max_radii2D[keep]
