"""diff_gaussian_rasterization -- MI355X-native drop-in for the 3DGS differentiable rasterizer.

Public surface used by the reference's render adapter
(/root/reference/gaussian_renderer/__init__.py:14 import, :36-49 settings, :51 rasterizer,
:85-93 call):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                  viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None)
        -> (color [3, H, W] fp32, radii [P] int32)
    GaussianRasterizer(raster_settings)(..., aux_outputs=True)      (extension)
        -> (color, radii, invdepth [1, H, W] fp32, alpha [1, H, W] fp32)
    GaussianRasterizer(raster_settings)(..., camera_grads=True)     (extension)
        -> the same outputs; settings.viewmatrix / .projmatrix / .campos receive gradients
    GaussianRasterizer(raster_settings)(..., antialiasing=True)     (extension; later upstream's switch)
        -> the same outputs, every splat's opacity compensated for the 0.3 px^2 dilation
    GaussianRasterizer(raster_settings)(..., absgrad=True)          (extension; AbsGS, gsplat's `absgrad`)
        -> the same outputs; after backward() means2D.absgrad holds sum_p |dL_p/dmean2D| [P, 3]
    GaussianRasterizer.markVisible(positions) -> bool [P]
    rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings)

This is the 2023 two-output API of graphdeco-inria/diff-gaussian-rasterization (the reference's
un-vendored submodule, /root/reference/.gitmodules:4-6), implemented over libgsrast.so (hand-written
HIP for gfx950, C ABI in include/gsrast.h).  Gradients flow to every tensor input that requires
them, including `means2D`, whose .grad holds the NDC-space screen gradient read by densification
(/root/reference/scene/gaussian_model.py:405-407).

aux_outputs=True adds two differentiable by-products of the same tile walk (rasterize_gaussians_aux):
alpha = 1 - final_T, the accumulated opacity (per-pixel backgrounds: color + (1 - alpha) * sky), and
invdepth = sum_i alpha_i T_i / z_i, the expected inverse depth (depth regularisation).  The default
call runs the same kernels and gives the same bits as before.
"""
from __future__ import annotations

import weakref
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_gaussians_aux",
           "cpu_deep_copy_tuple",
           "register_gradient_sink", "unregister_gradient_sink", "prepare_views", "last_num_rendered",
           "bounded_status"]

# ------------------------------------------------------------------------------------------
# Gradient sinks (an extension beyond the upstream API, used by gs_view_parallel.GradBucket).
# A leaf tensor registered here gets its rasterizer gradient written -- or, once the step already
# holds one, ADDED (gs_backward_accumulate) -- straight into the buffer its owner hands out
# (normally the tensor's own .grad, a view into a flat all-reduce bucket), and the autograd
# Function returns None for it.  The result equals autograd's `grad += g` with no extra pass over
# the gradients and no pack/unpack copy.
#
# The owner protocol (duck-typed, no base class; gs_view_parallel.GradBucket and
# gs_train_step._AdamBackward are the owners in the tree).  Required:
#   owner.claim(tensor) -> (buffer, accumulate) or None     None: the normal autograd path.  Asked in
#       the backward, in input order, for each registered input that needs a gradient.
# Optional hooks, each looked up in one place (_forward_step, _backward_step, _deferring_owner):
#   owner.forwarded(geomBuffer, P)     after the forward, once per distinct owner of the call's sinks:
#       the view's geometry buffer, whose error-flags word can be copied out behind the forward.
#   owner.write_order(stream) -> torch.cuda.Event or None   the stream waits for it before the
#       gradient-writing kernel; owner.written(stream) is called once the backward is enqueued.  An
#       owner shared by views on several streams orders its writes with the two; only owners whose
#       claim handed out a buffer are asked.
#   owner.defers (a true attribute) and owner.defer_view(ctx, inputs, view)   the owner of the call's
#       first sink takes the whole per-Gaussian half of a plain backward when every input gradient
#       the backward must produce (means2D aside) is registered with it: only the per-tile half runs
#       (_C.backward_render, dL/dmeans2D returned to autograd), nothing is claimed, and defer_view
#       gets inputs = dict(means3D, sh, colors, scales, rotations, cov3D, scale_modifier, degree,
#       debug, sh_rest) and view = (viewmatrix, projmatrix, campos, tanfovx, tanfovy, W, H,
#       geomBuffer) for _C.backward_gaussians.  Camera gradients refuse such an owner, and so do aux
#       gradients unless it opts in (accepts_aux).
#   owner.accepts_sh_split (a true attribute)   a deferring owner that handles split SH rows
#       (inputs["sh_rest"]); without it a deferred sh_split view is refused.
#   owner.accepts_aux (a true attribute)   a deferring owner that takes a backward with an alpha /
#       inverse-depth gradient (gs_train_step._AdamBackward; GradBucket does not): the aux per-tile half
#       runs (_C.backward_render(aux_grads=...)) and such an owner's defer_view inputs carry one more key,
#       inputs["invdepth_sums"]: the [P] fp32 per-Gaussian dL/d(1 / z) sums whose depth-chain term the
#       owner's per-Gaussian half must add to dL/dmeans3D (gs_backward_gaussians_adam_stats_aux), or
#       None for a plain backward.  The alpha gradient needs nothing per Gaussian.
# What an owner may read from the `ctx` it is handed: ctx.sinks, the call's registered inputs that
# require grad as [(input index, gradient name, tensor, owner)] in _SINK_INPUTS order, and
# ctx.needs_input_grad[0:8], the same eight inputs in every Function.  Nothing else of ctx is stable.
# ------------------------------------------------------------------------------------------
_SINKS: dict = {}  # id(tensor) -> (weakref to the tensor, owner)


def register_gradient_sink(tensor: torch.Tensor, owner) -> None:
    if not tensor.is_leaf:
        raise ValueError("register_gradient_sink: only leaf tensors can own a gradient sink")
    _SINKS[id(tensor)] = (weakref.ref(tensor), owner)


def unregister_gradient_sink(tensor: torch.Tensor) -> None:
    e = _SINKS.get(id(tensor))
    if e is not None and e[0]() is tensor:
        del _SINKS[id(tensor)]


def _sink_owner(t):
    if t is None or not isinstance(t, torch.Tensor) or not t.requires_grad:
        return None
    e = _SINKS.get(id(t))
    return e[1] if e is not None and e[0]() is t else None


# autograd input index -> gradient name (_C.GRAD_NAMES)
_SINK_INPUTS = ((0, "means3D"), (1, "means2D"), (2, "sh"), (3, "colors"), (4, "opacity"), (5, "scales"),
                (6, "rotations"), (7, "cov3D"))


def cpu_deep_copy_tuple(input_tuple):
    """CPU copies of every tensor in the tuple (used for the debug snapshot on failure)."""
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, prepared=None, sh_split=None, binning_capacity=None, antialiasing=False,
                        absgrad=None):
    """absgrad: None, or the call's _AbsgradHolder (GaussianRasterizer(...)(..., absgrad=True))."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, prepared, sh_split, binning_capacity,
                                     bool(antialiasing), absgrad)


# ------------------------------------------------------------------------------------------
# Bounded forwards (an extension beyond the upstream API, ABI v10).  Upstream reads num_rendered
# back to size its binning buffer, one host wait per forward.  With `binning_capacity=N` the
# buffer is sized for N instances ahead of time and the forward is enqueued without any host
# wait, event or allocation inside the library, so a training step can be captured into a
# HIP graph (torch.cuda.CUDAGraph).  Outputs are bit-identical while the view's instance count
# fits; a view that exceeds N leaves a sticky flag (its outputs invalid, all accesses in bounds)
# that the next bounded forward raises, or bounded_status() reports.  last_num_rendered() is the
# count of the last forward that read it back, a base for N.
# ------------------------------------------------------------------------------------------
def last_num_rendered() -> int:
    return _C._LAST_NUM_RENDERED[0]


def bounded_status():
    """(flags, instances) left by bounded forwards on the current device since the last call
    (cleared); raises RuntimeError if one exceeded its capacity, culled a prefiltered point or
    timed out.  Covers the forwards whose kernels ran: call it after a synchronisation."""
    return _C.bounded_status()


class PreparedView:
    """The first half of one view's forward, computed by prepare_views for several views at once
    (an extension beyond the upstream API).  Hand it to that view's GaussianRasterizer call as
    `prepared=`; it is checked against the call's settings and inputs and used once."""

    def __init__(self, triple, settings, inputs):
        self.triple, self.settings, self.inputs = triple, settings, inputs
        # autograd version counters: an in-place update between prepare_views and the call (an
        # optimizer step) would leave the prepared geometry stale
        self.versions = tuple(None if t is None else t._version for t in inputs)

    def take(self, settings, inputs):
        if self.triple is None:
            raise RuntimeError("prepare_views: a prepared view is used once")
        if settings is not self.settings or any(
                (a is None) != (b is None) or (a is not None and (a.data_ptr(), a.shape) != (b.data_ptr(), b.shape))
                for a, b in zip(inputs, self.inputs)):
            raise RuntimeError("prepare_views: the rasterizer call does not match the prepared view")
        if any(v is not None and b._version != v for b, v in zip(self.inputs, self.versions)):
            raise RuntimeError("prepare_views: an input was modified in place after prepare_views (stale prepared "
                               "view); prepare the views again")
        t, self.triple = self.triple, None
        return t


def prepare_views(rasterizers, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                  cov3D_precomp=None, streams=None, binning_capacity=None):
    """Run the first half of the forward (preprocess, depth order, instance offsets) of several
    views of the same Gaussians at once: one preprocess launch reads every Gaussian's inputs once
    for all cameras (gs_forward_preprocess_views) and one host wait returns every view's instance
    count.  Returns one PreparedView per rasterizer, to pass as `prepared=` to that rasterizer's
    call with the same tensors; view k's ordering runs on streams[k] (its call must run there).
    The rasterizers must share sh_degree, scale_modifier, prefiltered and debug.
    binning_capacity (one int, or one per view): bounded views -- no instance count is read back,
    each view's binning buffer is sized for its capacity (see bounded_status())."""
    ss = [r.raster_settings for r in rasterizers]
    s0 = ss[0]
    for s in ss[1:]:
        if (s.sh_degree, s.scale_modifier, s.prefiltered, s.debug) != (s0.sh_degree, s0.scale_modifier,
                                                                          s0.prefiltered, s0.debug):
            raise ValueError("prepare_views: the views must share sh_degree, scale_modifier, prefiltered, debug")
    empty = torch.Tensor([])
    e = lambda t: empty if t is None else t  # noqa: E731
    caps = None
    if binning_capacity is not None:
        caps = ([int(binning_capacity)] * len(ss) if isinstance(binning_capacity, int)
                else [int(c) for c in binning_capacity])
    # view k's matrices are read on the current stream (the preprocess) and on streams[k]
    own = [None] * len(ss) if not streams else [[streams[k]] for k in range(len(ss))]
    views = [_contiguous_matrix(s.viewmatrix, o) for s, o in zip(ss, own)]
    projs = [_contiguous_matrix(s.projmatrix, o) for s, o in zip(ss, own)]
    with torch.no_grad():
        tri = _C.preprocess_views([s.bg for s in ss], means3D.detach(), e(colors_precomp).detach(), opacities.detach(),
                                  e(scales).detach(), e(rotations).detach(), s0.scale_modifier,
                                  e(cov3D_precomp).detach(), views, projs, [s.tanfovx for s in ss],
                                  [s.tanfovy for s in ss], [s.image_height for s in ss], [s.image_width for s in ss],
                                  e(shs).detach(), s0.sh_degree, [s.campos for s in ss], s0.prefiltered, s0.debug,
                                  streams, caps)
    inputs = (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
    return [PreparedView(t, s, inputs) for t, s in zip(tri, ss)]


_CONTIG: dict = {}  # id(camera tensor) -> (weakref, _version, contiguous copy)


def _contiguous_matrix(t: torch.Tensor, streams=None) -> torch.Tensor:
    """t.contiguous() for the camera matrices, memoised per source tensor and version.  The
    reference's Camera keeps world_view_transform / full_proj_transform as transposed views
    (scene/cameras.py:54-56), so every render() would otherwise copy both (one copy launch each).
    The copy is made on the current stream; `streams` (views rendered on other streams) are
    recorded on it, so that the allocator does not reuse it while their kernels may still read
    it after the memo drops it."""
    if t.is_contiguous():
        c = t
    else:
        e = _CONTIG.get(id(t))
        if e is not None and e[0]() is t and e[1] == t._version:
            c = e[2]
        else:
            c = t.contiguous()
            if len(_CONTIG) > 256:
                _CONTIG.clear()
            _CONTIG[id(t)] = (weakref.ref(t), t._version, c)
    if streams and c.is_cuda:
        for st in streams:
            if st is not None:
                c.record_stream(st)
    return c


def _run_with_snapshot(fn, args, debug, dump_name, phase):
    """settings.debug: keep CPU copies of the arguments and dump them if the native call fails."""
    if not debug:
        return fn(*args)
    cpu_args = cpu_deep_copy_tuple(args)
    try:
        return fn(*args)
    except Exception:
        torch.save(cpu_args, dump_name)
        print(f"\nAn error occured in {phase}. Please forward {dump_name} for debugging.")
        raise


def _antialiasing_refusal(prepared=None, binning_capacity=None, sh_split=None):
    """The paths an antialiased call cannot take: their kernels (k_preprocess_views, the bounded
    forwards, the split-row loaders) do not scale the opacity."""
    for name, v in (("prepared", prepared), ("binning_capacity", binning_capacity), ("sh_split", sh_split)):
        if v is not None:
            raise RuntimeError(f"antialiasing: not supported with {name}=")


# ------------------------------------------------------------------------------------------
# Absolute screen-space gradients (an extension beyond the upstream API; AbsGS, gsplat's `absgrad`).
# absgrad=True: the backward's tile walk also sums |dL_p/dmean2D| over each splat's pixels (the signed sum
# in means2D.grad cancels for a large splat over fine detail, which then never crosses the densification
# threshold), and the caller's means2D tensor gets `.absgrad`, [P, 3] fp32 in the units of means2D.grad,
# written (not accumulated) by that backward.  The other outputs and gradients are bit-identical to the
# call without it.  The backward goes over ctypes (gs_backward_accumulate_absgrad).  Prepared views,
# bounded forwards and deferring gradient owners are refused: the K-view / bounded forwards are those of
# the multi-view and graph-captured steps, which do not densify per view through this call, and a
# deferring owner's per-tile half (gs_backward_render) has no absolute sums.
# ------------------------------------------------------------------------------------------
class _AbsgradHolder:
    """Carries the caller's means2D tensor to the backward (autograd hands the Function's inputs back
    as other tensor objects; a non-tensor argument passes through as it is)."""

    def __init__(self, means2D):
        self.tensor = means2D


def _absgrad_refusal(prepared=None, binning_capacity=None):
    for name, v in (("prepared", prepared), ("binning_capacity", binning_capacity)):
        if v is not None:
            raise RuntimeError(f"absgrad: not supported with {name}=")


_T_ABS_DEFER = ("absgrad: not supported with a deferring gradient owner (GradBucket(defer=True), the fused "
                "backward + Adam of gs_train_step)")

_T_AA_DEFER = ("antialiasing: not supported with a deferring gradient owner (GradBucket(defer=True), the fused "
               "backward + Adam of gs_train_step)")


def _forward_step(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s,
                  prepared=None, sh_split=None, binning_capacity=None, aux=False, antialiasing=False, absgrad=None):
    """The forward of the three autograd Functions: the native call (plain, with split SH rows or a
    binning capacity, over a prepared view, with the aux outputs, or antialiased), everything the
    backward needs on `ctx`, and the call's gradient sinks.  -> (color, radii), or with aux (color,
    radii, invdepth, alpha)."""
    if antialiasing:
        _antialiasing_refusal(prepared, binning_capacity, sh_split)
    if absgrad is not None:
        _absgrad_refusal(prepared, binning_capacity)
    # the camera matrices arrive transposed (cameras.py:54-56 world_view_transform is a
    # .transpose(0, 1) view); make them contiguous once and reuse them in backward
    view, proj = _contiguous_matrix(s.viewmatrix), _contiguous_matrix(s.projmatrix)
    sh_rest = None
    sh_input = sh  # the autograd input (with sh_split: the gradient carrier; its sink owner receives dL/dshs)
    if sh_split is not None:
        # split SH rows: the kernels read features_dc / features_rest in place; `sh` is only the
        # [P, M, 3] carrier of the concatenation's gradient (its values are never read)
        dc, sh_rest = (t.detach() for t in sh_split)
        if prepared is not None:
            raise RuntimeError("sh_split: not supported with prepared views")
        if tuple(sh.shape) != (dc.shape[0], 1 + sh_rest.shape[1], 3):
            raise RuntimeError("sh_split: shs must be the [P, M, 3] gradient carrier of cat(features_dc, "
                               "features_rest)")
        sh = dc
    args = (s.bg, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            view, proj, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree,
            s.campos, s.prefiltered, s.debug)
    if prepared is not None and binning_capacity is not None:
        raise RuntimeError("binning_capacity: not supported with prepared views")
    if prepared is not None:
        nz = lambda t: None if t is None or t.numel() == 0 else t  # noqa: E731
        tri = prepared.take(s, (means3D, nz(sh), nz(colors_precomp), opacities, nz(scales), nz(rotations),
                                nz(cov3Ds_precomp)))
        out = _C.rasterize_gaussians(*args, prepared=tri)
    elif antialiasing:
        # (the snapshot's arguments end with the flag)
        out = _run_with_snapshot(lambda *a: _C.rasterize_gaussians_aa(*a[:-1], aux=aux), args + (True,), s.debug,
                                 "snapshot_fw.dump", "forward")
    else:
        if aux:
            fn = lambda *a: _C.rasterize_gaussians_aux(*a, sh_rest=sh_rest)  # noqa: E731
        elif sh_rest is not None or binning_capacity is not None:
            fn = lambda *a: _C.rasterize_gaussians(*a, sh_rest=sh_rest, capacity=binning_capacity)  # noqa: E731
        else:
            fn = _C.rasterize_gaussians
        out = _run_with_snapshot(fn, args, s.debug, "snapshot_fw.dump", "forward")
    num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = out[:6]
    ctx.raster_settings = s
    ctx.num_rendered = num_rendered
    ctx.matrices = (view, proj)
    ctx.antialiasing = bool(antialiasing)
    ctx.absgrad = absgrad  # None, or the holder of the caller's means2D
    ctx.sh_rest = sh_rest
    # the split rows are kept outside save_for_backward (they are not inputs of the Function):
    # their version counters stand in for autograd's in-place check
    ctx.sh_split_versions = None if sh_rest is None else (sh._version, sh_rest._version)
    ctx.set_materialize_grads(False)  # no zero-filled gradient for the (int) radii output, or an unused one
    # (an antialiased backward chains through the opacity scale: it reads the opacities too)
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                          binningBuffer, imgBuffer, *((opacities,) if antialiasing else ()))
    ctx.mark_non_differentiable(radii)
    sinks = []
    if _SINKS:
        inputs = (means3D, means2D, sh_input, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        for k, name in _SINK_INPUTS:
            owner = _sink_owner(inputs[k])
            if owner is not None:
                sinks.append((k, name, inputs[k], owner))
        # an owner that follows its views' forward status (gs_train_step._AdamBackward) gets the
        # view's geometry buffer now, while its error-flags word can still be copied out
        # stream-ordered behind this forward
        for owner in {id(o): o for _k, _n, _t, o in sinks}.values():
            if hasattr(owner, "forwarded"):
                owner.forwarded(geomBuffer, means3D.shape[0])
    ctx.sinks = sinks
    return (color, radii) + tuple(out[6:])


def _backward_step(ctx, grad_out_color, aux_grads=None, camera=None):
    """The backward of the three autograd Functions.  aux_grads: None or (dL/dinvdepth, dL/dalpha),
    either may be None; camera: None, or whether dL/dcampos is wanted.  -> (the eight Gaussian
    gradients in input order, None where an owner's buffer or a deferred pass received it; the
    camera gradients (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos or None), or None without `camera`
    or when no output reached the loss).  A deferring owner takes the view here (with aux gradients
    only one that has `accepts_aux`); the callers that cannot be deferred (aux gradients to another
    owner, camera gradients) refuse it first."""
    if aux_grads is not None and aux_grads[0] is None and aux_grads[1] is None:
        aux_grads = None  # only the colour reached the loss (or nothing did): the plain backward
    absgrad = getattr(ctx, "absgrad", None)
    if grad_out_color is None and aux_grads is None:  # no output reached the loss
        if absgrad is not None:
            t = absgrad.tensor
            t.absgrad = torch.zeros((t.shape[0], 3), dtype=torch.float32, device=ctx.saved_tensors[1].device)
        return (None,) * 8, None
    s = ctx.raster_settings
    colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer = (
        ctx.saved_tensors[:10])
    antialiasing = getattr(ctx, "antialiasing", False)
    if ctx.sh_rest is not None and (sh._version, ctx.sh_rest._version) != ctx.sh_split_versions:
        raise RuntimeError("sh_split: features_dc or features_rest was modified by an inplace operation between "
                           "the forward and the backward")
    view, proj = ctx.matrices
    if grad_out_color is None:  # the loss reads the aux outputs only
        grad_out_color = torch.zeros((3, s.image_height, s.image_width), dtype=torch.float32, device=means3D.device)
    args = (s.bg, means3D, radii, colors_precomp, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            view, proj, s.tanfovx, s.tanfovy, grad_out_color.contiguous(), sh, s.sh_degree,
            s.campos, geomBuffer, ctx.num_rendered, binningBuffer, imgBuffer, s.debug)

    # a sink owner that defers the per-Gaussian half (GradBucket(defer=True)) takes this view
    # when every parameter gradient the call needs goes to it: only the per-tile half and
    # dL_dmeans2D run now, the per-Gaussian half later for all of its views in one pass
    deferrer = _deferring_owner(ctx)
    if deferrer is not None and absgrad is not None:
        raise RuntimeError(_T_ABS_DEFER)  # its per-tile half (gs_backward_render) has no absolute sums
    if deferrer is not None and antialiasing:
        # its per-Gaussian half (k_backward_gaussians, the fused backward + Adam) has no opacity-scale chain
        raise RuntimeError(_T_AA_DEFER)
    if deferrer is not None and ctx.sh_rest is not None and not getattr(deferrer, "accepts_sh_split", False):
        raise RuntimeError("sh_split: not supported with a deferring gradient bucket")
    if deferrer is not None:
        M = (1 + ctx.sh_rest.size(1)) if ctx.sh_rest is not None else (sh.size(1) if sh.ndimension() == 3 else 0)
        dm2 = _C.backward_render(s.bg, view, proj, s.campos, s.tanfovx, s.tanfovy, grad_out_color.contiguous(),
                                 means3D.size(0), s.sh_degree, M,
                                 geomBuffer, ctx.num_rendered, binningBuffer, imgBuffer, ctx.needs_input_grad[1],
                                 s.debug, **({} if aux_grads is None else {"aux_grads": aux_grads}))
        more = {}
        if getattr(deferrer, "accepts_aux", False):  # (the other owners' inputs are what they were)
            more["invdepth_sums"] = None
            if aux_grads is not None:
                dm2, more["invdepth_sums"] = dm2
        deferrer.defer_view(ctx, dict(means3D=means3D, sh=sh, colors=colors_precomp, scales=scales,
                                      rotations=rotations, cov3D=cov3Ds_precomp, scale_modifier=s.scale_modifier,
                                      degree=s.sh_degree, debug=s.debug, sh_rest=ctx.sh_rest, **more),
                            (view, proj, s.campos, s.tanfovx, s.tanfovy, s.image_width, s.image_height,
                             geomBuffer))
        return (None, dm2) + (None,) * 6, None

    sinks, sunk, owners = {}, set(), []
    for k, name, t, owner in ctx.sinks:
        if ctx.needs_input_grad[k]:
            claim = owner.claim(t)
            if claim is not None:
                sinks[name] = claim
                sunk.add(k)
                if all(o is not owner for o in owners):
                    owners.append(owner)
    # sink owners may order their buffer's writes across streams (views rendered on several
    # streams, GradBucket): the last kernel waits for the owner's previous write
    wait = None
    if owners:
        st = torch.cuda.current_stream(grad_out_color.device)
        evs = [e for e in (o.write_order(st) for o in owners if hasattr(o, "write_order")) if e is not None]
        for e in evs[1:]:
            st.wait_event(e)
        wait = evs[0] if evs else None

    more = {} if absgrad is None else {"absgrad": True}  # (the default call's arguments are what they were)

    def _bwd(*a):
        return _C.backward_impl(*a, want_all=False, sinks=sinks, wait_event=wait, sh_rest=ctx.sh_rest,
                                aux_grads=aux_grads, camera=camera, **more)

    def _bwd_aa(*a):  # (the snapshot's arguments end with the flag and the opacities)
        return _C.backward_impl(*a[:-2], want_all=False, sinks=sinks, wait_event=wait, sh_rest=ctx.sh_rest,
                                aux_grads=aux_grads, camera=camera, aa_opacity=a[-1], **more)

    if antialiasing:
        res = _run_with_snapshot(_bwd_aa, args + (True, ctx.saved_tensors[10]), s.debug, "snapshot_bw.dump",
                                 "backward")
    else:
        res = _run_with_snapshot(_bwd, args, s.debug, "snapshot_bw.dump", "backward")
    (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
     grad_rotations) = res[:8]
    if absgrad is not None:
        absgrad.tensor.absgrad = res[-1]  # written by this backward (a second one writes the same bits)
    for o in owners:
        if hasattr(o, "written"):
            o.written(st)
    grads = [grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
             grad_rotations, grad_cov3Ds_precomp]
    for k in sunk:  # already in the sink's buffer (the tensor's .grad)
        grads[k] = None
    return tuple(grads), (res[8] if camera is not None else None)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, prepared=None, sh_split=None, binning_capacity=None, antialiasing=False,
                absgrad=None):
        return _forward_step(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                             raster_settings, prepared, sh_split, binning_capacity, antialiasing=antialiasing,
                             absgrad=absgrad)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        return _backward_step(ctx, grad_out_color)[0] + (None,) * 6


# ------------------------------------------------------------------------------------------
# Aux outputs (an extension beyond the 2023 upstream API; later upstream revisions return the
# inverse depth as a third output).  aux_outputs=True: the render's AUX walk also writes
#   alpha    = 1 - final_T           the accumulated opacity, 0 where no splat reaches the pixel
#   invdepth = sum_i alpha_i T_i / z_i   the expected inverse depth (no background term)
# both [1, H, W] and differentiable: alpha is a colour channel of colour 0 and background -1, the
# inverse depth one of colour 1 / z_i (its gradient also reaches means3D through z_i).  Colour and
# radii are bit-identical to the plain call's, and a backward that receives no aux gradient runs
# the plain backward.  Aux calls take the two-call path over ctypes (not _gs_ext); prepared views,
# bounded forwards and deferring gradient owners that do not opt in (owner.accepts_aux) are refused.
# ------------------------------------------------------------------------------------------
def rasterize_gaussians_aux(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings, sh_split=None, antialiasing=False, absgrad=None):
    """-> (color, radii, invdepth, alpha)"""
    return _RasterizeGaussiansAux.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                        cov3Ds_precomp, raster_settings, sh_split, bool(antialiasing), absgrad)


class _RasterizeGaussiansAux(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, sh_split=None, antialiasing=False, absgrad=None):
        return _forward_step(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                             raster_settings, sh_split=sh_split, aux=True, antialiasing=antialiasing, absgrad=absgrad)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_invdepth, grad_alpha):
        # without an aux gradient the backward is the plain one, which a deferring owner may take
        # (so may one with an aux gradient, by an owner that opted in: accepts_aux)
        deferrer = _deferring_owner(ctx)
        if ((grad_invdepth is not None or grad_alpha is not None) and deferrer is not None
                and not getattr(deferrer, "accepts_aux", False)):
            raise RuntimeError("aux_outputs: an alpha / inverse-depth gradient is not supported with a deferring "
                               "gradient owner (GradBucket(defer=True), the fused backward + Adam of gs_train_step)")
        return _backward_step(ctx, grad_out_color, (grad_invdepth, grad_alpha))[0] + (None,) * 4


# ------------------------------------------------------------------------------------------
# Camera gradients (an extension beyond the upstream API).  camera_grads=True: those of
# settings.viewmatrix, .projmatrix and .campos that require grad enter the autograd Function as
# tensor inputs and receive dL/dviewmatrix, dL/dprojmatrix [4, 4] and dL/dcampos [3], treated as
# independent inputs (the caller's graph chains them to a pose: full_proj = view @ P, campos =
# view.inverse()[3, :3]).  The forward, the Gaussian gradients and their kernels are those of the
# plain / aux call, bit for bit; the backward goes over ctypes and gs_backward_camera follows it on
# the stream (two small kernels: fp64 sums in a fixed order, bitwise reproducible).  Prepared views,
# bounded forwards, split SH rows and deferring gradient owners are refused.
# ------------------------------------------------------------------------------------------
class _RasterizeGaussiansCamera(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                viewmatrix, projmatrix, campos, raster_settings, aux, antialiasing=False, absgrad=None):
        # (viewmatrix, projmatrix, campos are raster_settings' own tensors: inputs for the graph's sake)
        ctx.camera_aux = aux
        ctx.camera_meta = tuple((t.shape, t.device) for t in (viewmatrix, projmatrix, campos))
        return _forward_step(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                             raster_settings, aux=aux, antialiasing=antialiasing, absgrad=absgrad)

    @staticmethod
    def backward(ctx, *grad_outs):
        if _deferring_owner(ctx) is not None:
            raise RuntimeError("camera_grads: not supported with a deferring gradient owner "
                               "(GradBucket(defer=True), the fused backward + Adam of gs_train_step)")
        grads, camera_grads = _backward_step(ctx, grad_outs[0], grad_outs[2:4] if ctx.camera_aux else None,
                                             bool(ctx.needs_input_grad[10]))
        cam = [None, None, None]
        if camera_grads is not None:
            for k, g in enumerate(camera_grads):
                shape, device = ctx.camera_meta[k]
                if g is not None and ctx.needs_input_grad[8 + k]:
                    cam[k] = g.reshape(shape).to(device)
        return grads + tuple(cam) + (None,) * 4


def _deferring_owner(ctx):
    """The one sink owner with `defer_view` that receives every input gradient this backward must
    produce (means2D aside), or None."""
    if not ctx.sinks:
        return None
    owner = ctx.sinks[0][3]
    if not getattr(owner, "defers", False):
        return None
    sunk = {k for k, _name, _t, o in ctx.sinks if o is owner}
    for k in range(8):
        if k != 1 and ctx.needs_input_grad[k] and k not in sunk:
            return None
    return owner


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            s = self.raster_settings
            return _C.mark_visible(positions, s.viewmatrix, s.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, prepared=None, sh_split=None, binning_capacity=None, aux_outputs=False,
                camera_grads=False, absgrad=False, antialiasing=False):
        """prepared: this call's PreparedView from prepare_views (extension; default: none).
        binning_capacity: size the binning buffer for that many instances and run the forward
        without a host wait (extension, ABI v10; see bounded_status()).
        sh_split: (features_dc [P,1,3], features_rest [P,M-1,3]) read in place instead of the
        concatenated shs (extension, ABI v8: no per-iteration cat); `shs` is then a [P,M,3] tensor
        whose values are never read and whose .grad receives dL/d cat(features_dc, features_rest)
        (what FusedAdam.step_activated consumes).  Bit-identical to passing the concatenation.
        aux_outputs: also return the expected inverse depth and the accumulated opacity of the same
        walk, (color, radii, invdepth [1,H,W], alpha [1,H,W]), both differentiable (extension; not
        with prepared= or binning_capacity=).
        camera_grads: settings.viewmatrix / .projmatrix / .campos that require grad receive their
        gradients (extension; with or without aux_outputs; not with prepared=, binning_capacity=,
        sh_split= or a deferring gradient owner).  None of them requiring grad: the call without it.
        antialiasing: compensate every splat's opacity for the 0.3 px^2 low-pass dilation of its
        footprint, op' = op sqrt(det S / det(S + 0.3 I)) (floor 0.005; later upstream revisions'
        `antialiasing` switch, the Mip-Splatting 2D filter normalisation), so a splat smaller than a
        pixel keeps its energy at any resolution; gradients chain through the scale (extension; with
        or without aux_outputs / camera_grads; not with prepared=, binning_capacity=, sh_split= or a
        deferring gradient owner).  False: today's kernels and bits.
        absgrad: after backward(), the caller's means2D tensor carries `.absgrad` [P, 3] fp32: the sum
        over each splat's pixels of the absolute per-pixel screen-space gradient, in the units of
        means2D.grad[:, :2] (column 2 is 0), written by that backward -- what AbsGS densifies on, since
        the signed sum cancels for a large splat over detail (extension; with or without sh_split=,
        aux_outputs, camera_grads, antialiasing; means2D must require grad; not with prepared=,
        binning_capacity= or a deferring gradient owner).  False: today's calls and bits."""
        s = self.raster_settings
        antialiasing = bool(antialiasing)
        if antialiasing:
            _antialiasing_refusal(prepared, binning_capacity, sh_split)
        holder = None
        if absgrad:
            _absgrad_refusal(prepared, binning_capacity)
            if not (isinstance(means2D, torch.Tensor) and means2D.requires_grad):
                raise RuntimeError("absgrad: means2D does not require grad")
            holder = _AbsgradHolder(means2D)
        if camera_grads:
            for name, v in (("prepared", prepared), ("binning_capacity", binning_capacity), ("sh_split", sh_split)):
                if v is not None:
                    raise RuntimeError(f"camera_grads: not supported with {name}=")
            camera_grads = any(isinstance(t, torch.Tensor) and t.requires_grad
                               for t in (s.viewmatrix, s.projmatrix, s.campos))
        if aux_outputs and prepared is not None:
            raise RuntimeError("aux_outputs: not supported with prepared views (prepared=)")
        if aux_outputs and binning_capacity is not None:
            raise RuntimeError("aux_outputs: not supported with a bounded forward (binning_capacity=)")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        _C.check_image_size(s.image_width, s.image_height)
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        if camera_grads:
            return _RasterizeGaussiansCamera.apply(means3D, means2D, shs, colors_precomp, opacities, scales,
                                                   rotations, cov3D_precomp, s.viewmatrix, s.projmatrix, s.campos, s,
                                                   bool(aux_outputs), antialiasing, holder)
        if aux_outputs:
            return rasterize_gaussians_aux(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                           cov3D_precomp, s, sh_split, antialiasing, holder)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   s, prepared, sh_split, binning_capacity, antialiasing, holder)
