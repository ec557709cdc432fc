"""Per-Gaussian feature channels rendered as images on MI355X.

Any per-Gaussian quantity -- a semantic or language feature vector, a normal, an id colour, a sky
logit, a gs_importance score -- composited through the finished tile lists of one rendered view
(csrc/gs_features.hip, C ABI gs_feature_forward / gs_feature_backward) instead of three channels at
a time through the whole rasterizer:

    out[c, p]   = sum_i f_i[c] alpha_i(p) T_i(p)            the colour forward's own alpha and T
    dL/df_i[c]  = sum_p alpha_i(p) T_i(p) dL/dout[c, p]

    view = FeatureView.from_inputs(GaussianRasterizer(settings), means3D=..., opacities=..., shs=...,
                                   scales=..., rotations=...)
    sem = render_features(view, features)          # [C, H, W]; differentiable in `features`
    loss(sem).backward()                           # features.grad [P, C]

The geometry is constant: render_features is differentiable in `features` ONLY.  Nothing flows to
means3D, scales, rotations, opacities or the camera (joint geometry gradients would need the tile
backward to carry C more channels).  There is no background term: compose out + (1 - alpha) * bg
with the aux alpha of the same view.  Both directions are bitwise reproducible.

The view comes from the two-call forward (plain, or antialiased with antialiasing=True); feature
rendering is not defined for bounded (binning_capacity=), prepared (prepare_views) or
graph-captured forwards.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from diff_gaussian_rasterization import _C, _contiguous_matrix

__all__ = ["FeatureView", "render_features", "render_features_for", "MAX_CHANNELS"]

# GS_MAX_FEATURE_CHANNELS of include/gsrast.h: a larger C is refused (render it in slices of columns)
MAX_CHANNELS = 1024


class FeatureView(NamedTuple):
    """One rendered view's buffers: what render_features composites through, any number of times."""
    num_rendered: int
    radii: torch.Tensor       # [P] int32
    geom: torch.Tensor
    binning: torch.Tensor
    img: torch.Tensor
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    campos: torch.Tensor
    tanfovx: float
    tanfovy: float
    image_height: int
    image_width: int
    color: torch.Tensor       # [3, H, W], the view's rendered image
    debug: bool = False

    @classmethod
    def from_inputs(cls, rasterizer, *, antialiasing=False, means3D, opacities, means2D=None, shs=None,
                    colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None) -> "FeatureView":
        """The two-call forward of `rasterizer`'s settings on these inputs (the keywords of
        GaussianRasterizer.forward, same checks and exception texts; means2D is not read).  No graph
        is recorded: the geometry is constant for every render over the view."""
        s = rasterizer.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        _C.check_image_size(s.image_width, s.image_height)
        H, W = int(s.image_height), int(s.image_width)
        _C._dev_check(means3D, "means3D")
        empty = torch.Tensor([])
        e = lambda t: empty if t is None else t.detach()  # noqa: E731
        with torch.no_grad():
            view, proj = _contiguous_matrix(s.viewmatrix), _contiguous_matrix(s.projmatrix)
            R, color, radii, geom, binning, img = _C.rasterize_gaussians_two_call(
                s.bg, means3D.detach(), e(colors_precomp), opacities.detach(), e(scales), e(rotations),
                s.scale_modifier, e(cov3D_precomp), view, proj, s.tanfovx, s.tanfovy, H, W, e(shs), s.sh_degree,
                s.campos, s.prefiltered, s.debug, antialiasing=bool(antialiasing))
        return cls(int(R), radii, geom, binning, img, view, proj, s.campos, float(s.tanfovx), float(s.tanfovy), H, W,
                   color, bool(s.debug))

    def _args(self):
        return (self.num_rendered, self.radii, self.geom, self.binning, self.img, self.viewmatrix, self.projmatrix,
                self.campos, self.tanfovx, self.tanfovy, self.image_height, self.image_width)


def _check_features(view: FeatureView, features) -> None:
    P, dev = int(view.radii.numel()), view.radii.device
    want = f"features must be a float32 tensor of shape ({P}, C), 1 <= C <= {MAX_CHANNELS}, on {dev}"
    if not isinstance(features, torch.Tensor):
        raise ValueError(f"{want} (got {type(features).__name__})")
    if features.dtype != torch.float32:
        raise ValueError(f"{want} (got dtype {features.dtype})")
    if features.ndimension() != 2 or features.shape[0] != P or not 1 <= features.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"{want} (got shape {tuple(features.shape)})")
    if features.device != dev:
        raise ValueError(f"{want} (got device {features.device})")


class _RenderFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, view):
        ctx.view = view
        return _C.feature_forward(*view._args(), features.detach(), debug=view.debug)

    @staticmethod
    def backward(ctx, dL_dout):
        view = ctx.view
        return _C.feature_backward(*view._args(), dL_dout.contiguous(), debug=view.debug), None


def render_features(view: FeatureView, features: torch.Tensor) -> torch.Tensor:
    """[C, H, W]: `features` ([P, C] fp32 on the view's device) composited through the view's lists
    with the colour forward's own alpha and T, no background term.  Differentiable in `features`
    only -- the geometry of the view is constant.  One view may be rendered any number of times,
    with different C.  Any other input raises ValueError naming the expected shape."""
    _check_features(view, features)
    return _RenderFeatures.apply(features, view)


def render_features_for(rasterizer, features, *, antialiasing=False, **inputs) -> torch.Tensor:
    """One shot: FeatureView.from_inputs(rasterizer, **inputs), then render_features."""
    return render_features(FeatureView.from_inputs(rasterizer, antialiasing=antialiasing, **inputs), features)
