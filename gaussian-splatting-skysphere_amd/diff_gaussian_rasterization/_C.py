"""Native entry points of `diff_gaussian_rasterization`, bound to libgsrast.so (C ABI, gfx950).

Same names, argument order, return tuples and error behaviour as the upstream torch extension
`diff_gaussian_rasterization._C` that the reference binds (un-vendored submodule,
/root/reference/.gitmodules:4-6; signatures restated in SURVEY.md §8b):

    rasterize_gaussians(...)           -> (num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer)
    rasterize_gaussians_backward(...)  -> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D,
                                           dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    mark_visible(means3D, viewmatrix, projmatrix) -> bool[P]

Tensors must live on a HIP device; all work is enqueued on the current torch stream of that
device.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _native

_lib = _native.load()


def _load_ext():
    """The torch C++ host fast path (_gs_ext, csrc/gs_torch_ext.cpp) of the plain forward / backward
    calls, if built (setup_ext.py); GSRAST_NO_EXT=1 keeps every call on the ctypes path."""
    if os.environ.get("GSRAST_NO_EXT", "0") not in ("", "0"):
        return None
    try:
        from . import _gs_ext
    except ImportError:
        return None
    _gs_ext.init()
    return _gs_ext


_EXT = _load_ext()


def check_image_size(W, H):
    """Raises for an image beyond the library's size limits (include/gsrast.h: GS_MAX_GRID_DIM,
    GS_MAX_TILES), with the library's message: its sizing query returns 0 bytes for such a size."""
    if (W, H) in _SIZES_OK:  # (a training loop asks about a handful of sizes, every iteration)
        return
    if W > 0 and H > 0 and _lib.gs_image_buffer_bytes(int(W), int(H)) == 0:
        raise RuntimeError(f"rasterize_gaussians: {_native.last_error()}")
    if len(_SIZES_OK) < 4096:
        _SIZES_OK.add((W, H))


_SIZES_OK = set()


def _dev_check(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"diff_gaussian_rasterization (MI355X/HIP) needs device tensors; {name} is on {t.device}. "
            "There is no CPU rasterizer in the product path."
        )


def _f32(t, name, device, allow_empty=True, host_ok=False):
    """Contiguous fp32 device tensor, or None for an absent / empty input.  host_ok: a camera-side
    input (bg, viewmatrix, projmatrix, campos) may come from the host and is copied over; every
    per-Gaussian tensor must already live on means3D's device."""
    if t is None:
        return None
    if t.numel() == 0:
        if allow_empty:
            return None
        raise RuntimeError(f"{name} must not be empty")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if t.device != device:
        if host_ok and t.numel() <= 16:
            t = t.to(device)
        else:
            _dev_check(t, name)
            raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    return t.contiguous()


def _camera_side(device, background, viewmatrix, projmatrix, campos):
    """(bg, view, proj, campos) of a call that takes them outside _Inputs: the camera-side tensors
    may come from the host (_f32(..., host_ok=True)); an absent one stays None."""
    return (_f32(background, "background", device, host_ok=True), _f32(viewmatrix, "viewmatrix", device, host_ok=True),
            _f32(projmatrix, "projmatrix", device, host_ok=True), _f32(campos, "campos", device, host_ok=True))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# Every C call below names its arguments as include/gsrast.h does (_native.ordered puts them in order),
# and calls the widest entry of its family: the narrower ones are that entry with NULL / 0 in the
# extra slots (csrc/gs_api.hip forwards them so).
_call = _native.call


def _camera(view, proj, campos, tan_fovx, tan_fovy):
    """The camera arguments of the C entries, by name."""
    return dict(viewmatrix=_ptr(view), projmatrix=_ptr(proj), campos=_ptr(campos), tan_fovx=float(tan_fovx),
                tan_fovy=float(tan_fovy))


def _aux_grads(aux_grads, H, W, dev):
    """(dL_dout_invdepth, dL_dout_alpha) of a backward as contiguous [H, W] tensors, either may be None."""
    if aux_grads is None:
        return None, None
    d_inv, d_alpha = (_f32(t, n, dev) for t, n in zip(aux_grads, ("dL_dout_invdepth", "dL_dout_alpha")))
    for t in (d_inv, d_alpha):
        if t is not None and t.numel() != H * W:
            raise RuntimeError("aux gradients must have shape (1, H, W)")
    return d_inv, d_alpha


class _Inputs:
    """Validated, contiguous views of one rasterizer call's tensors."""

    def __init__(self, background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix,
                 projmatrix, sh, campos, need_opacity=True, sh_rest=None):
        if means3D.ndimension() != 2 or means3D.size(1) != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        _dev_check(means3D, "means3D")
        self.device = means3D.device
        d = self.device
        self.P = means3D.size(0)
        self.means3D = _f32(means3D, "means3D", d)
        self.bg = _f32(background, "background", d, host_ok=True)
        self.colors = _f32(colors, "colors_precomp", d)
        self.opacity = _f32(opacity, "opacities", d)
        self.scales = _f32(scales, "scales", d)
        self.rotations = _f32(rotations, "rotations", d)
        self.cov3D = _f32(cov3D_precomp, "cov3D_precomp", d)
        self.view = _f32(viewmatrix, "viewmatrix", d, host_ok=True)
        self.proj = _f32(projmatrix, "projmatrix", d, host_ok=True)
        self.sh = _f32(sh, "sh", d)
        self.campos = _f32(campos, "campos", d, host_ok=True)
        self.M = 0 if self.sh is None else (self.sh.size(1) if self.sh.ndimension() == 3 else self.sh.numel() // max(1, 3 * self.P))
        # split SH rows (ABI v8): sh is features_dc [P, 1, 3], sh_rest features_rest [P, M - 1, 3]
        self.sh_rest = _f32(sh_rest, "features_rest", d)
        if self.sh_rest is not None:
            if self.sh is None or self.colors is not None:
                raise RuntimeError("split SH: features_dc and features_rest replace shs (no colors_precomp)")
            if tuple(self.sh.shape) != (self.P, 1, 3) or self.sh_rest.ndimension() != 3 or tuple(
                    self.sh_rest.shape[::2]) != (self.P, 3):
                raise RuntimeError("split SH: expected features_dc [P, 1, 3] and features_rest [P, M - 1, 3]")
            self.M = 1 + self.sh_rest.size(1)
        if self.P > 0:
            if self.colors is not None and self.colors.numel() != 3 * self.P:
                raise RuntimeError("colors_precomp must have shape (P, 3)")
            if need_opacity and (self.opacity is None or self.opacity.numel() != self.P):
                raise RuntimeError("opacities must have shape (P, 1)")

    def head(self, W, H, degree=None):
        """The leading arguments of the C entries, by name; degree=None: an entry of the render half,
        which takes no D / M."""
        d = dict(P=self.P, background=_ptr(self.bg), image_width=W, image_height=H)
        if degree is not None:
            d.update(D=int(degree), M=self.M)
        return d

    def scene(self, scale_modifier, rest=True):
        """The per-Gaussian arguments of the C entries, by name; rest=False: an entry without shs_rest."""
        d = dict(means3D=_ptr(self.means3D), shs=_ptr(self.sh), colors_precomp=_ptr(self.colors),
                 opacities=_ptr(self.opacity), scales=_ptr(self.scales), scale_modifier=float(scale_modifier),
                 rotations=_ptr(self.rotations), cov3D_precomp=_ptr(self.cov3D))
        if rest:
            d["shs_rest"] = _ptr(self.sh_rest)
        return d

    def camera(self, tan_fovx, tan_fovy):
        return _camera(self.view, self.proj, self.campos, tan_fovx, tan_fovy)

    def preprocess(self, W, H, degree, scale_modifier, tan_fovx, tan_fovy, prefiltered, debug, st,
                   antialiasing=False):
        """The two-call forward's first half (gs_forward_preprocess_aa; gs_forward_preprocess_split for
        split SH rows): (num_rendered, radii, geomBuffer), every radius written by the kernels."""
        radii = torch.empty((self.P,), dtype=torch.int32, device=self.device)
        geom = torch.empty((_lib.gs_geom_buffer_bytes(self.P),), dtype=torch.uint8, device=self.device)
        nr = ctypes.c_longlong(0)
        split = self.sh_rest is not None
        if antialiasing and split:
            raise RuntimeError("antialiasing: not supported with sh_split=")
        args = dict(self.head(W, H, degree), **self.scene(scale_modifier, rest=split),
                    **self.camera(tan_fovx, tan_fovy), prefiltered=int(bool(prefiltered)), radii_out=_ptr(radii),
                    geom_buffer=_ptr(geom), debug=int(bool(debug)), stream=st)
        if split:  # features_dc / features_rest in place of shs / colors_precomp
            args["shs_dc"] = args.pop("shs")
            del args["colors_precomp"]
            _call("gs_forward_preprocess_split", "rasterize_gaussians (preprocess)", num_rendered=ctypes.byref(nr),
                  **args)
        else:
            _call("gs_forward_preprocess_aa", "rasterize_gaussians (preprocess)", num_rendered_host=ctypes.byref(nr),
                  antialiasing=int(bool(antialiasing)), **args)
        _LAST_NUM_RENDERED[0] = int(nr.value)
        return int(nr.value), radii, geom


def preprocess_views(backgrounds, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                     viewmatrices, projmatrices, tan_fovx, tan_fovy, image_heights, image_widths, sh, degree, campos,
                     prefiltered, debug, streams=None, capacities=None):
    """First half of K views' forwards in one preprocess launch (gs_forward_preprocess_views):
    returns [(num_rendered, radii, geomBuffer, bounded)] per view, each what rasterize_gaussians
    computes for that camera before its binning; view k's depth ordering is enqueued on streams[k]
    (default: the current stream).  Pass each view's tuple to rasterize_gaussians(..., prepared=).
    capacities: K binning capacities -- nothing is read back (gs_forward_preprocess_views_bounded),
    num_rendered is the capacity and the view's render is bounded (gs_forward_render_bounded)."""
    K = len(viewmatrices)
    if not 1 <= K <= 8:
        raise RuntimeError("preprocess_views: 1 to 8 views per call")
    if _EXT is not None and means3D.is_cuda:
        return list(_EXT.preprocess_views(
            list(backgrounds), means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp,
            list(viewmatrices), list(projmatrices), [float(t) for t in tan_fovx], [float(t) for t in tan_fovy],
            [int(h) for h in image_heights], [int(w) for w in image_widths], sh, int(degree), list(campos),
            bool(prefiltered), bool(debug), [s.cuda_stream for s in streams] if streams is not None else [],
            None if capacities is None else [int(c) for c in capacities]))
    xs = [_Inputs(backgrounds[k], means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrices[k],
                  projmatrices[k], sh, campos[k]) for k in range(K)]
    x, dev = xs[0], xs[0].device
    u8 = dict(dtype=torch.uint8, device=dev)
    radii = [torch.empty((x.P,), dtype=torch.int32, device=dev) for _ in range(K)]
    # the views' geometry buffers are slices of one allocation (one stride apart): the library then
    # runs the K depth sorts as one set of launches
    gb = _lib.gs_geom_buffer_bytes(x.P) if x.P else 0
    geom_all = torch.empty((K * gb,), **u8)
    geoms = [geom_all[k * gb:(k + 1) * gb] for k in range(K)]
    if x.P == 0:
        return [(0, r, g, False) for r, g in zip(radii, geoms)]
    if capacities is not None and len(capacities) != K:
        raise RuntimeError("preprocess_views: one capacity per view")
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    nr = (ctypes.c_longlong * K)()
    vst = None
    if streams is not None:
        vst = (ctypes.c_void_p * K)(*[s.cuda_stream for s in streams])
    if capacities is not None:
        for k, c in enumerate(capacities):
            nr[k] = int(c)
    bounded = capacities is not None
    # (two entries, not one family: the bounded one reads nr as the capacities and waits for nothing)
    entry, counts = (("gs_forward_preprocess_views_bounded", "capacity") if bounded
                     else ("gs_forward_preprocess_views", "num_rendered_host"))
    with torch.cuda.device(dev):
        _call(entry, "preprocess_views", K=K, P=x.P, D=int(degree), M=x.M, background=arr([y.bg for y in xs]),
              image_width=(ctypes.c_int * K)(*[int(w) for w in image_widths]),
              image_height=(ctypes.c_int * K)(*[int(h) for h in image_heights]),
              **x.scene(scale_modifier, rest=False), viewmatrix=arr([y.view for y in xs]),
              projmatrix=arr([y.proj for y in xs]), campos=arr([y.campos for y in xs]),
              tan_fovx=(ctypes.c_float * K)(*[float(t) for t in tan_fovx]),
              tan_fovy=(ctypes.c_float * K)(*[float(t) for t in tan_fovy]), prefiltered=int(bool(prefiltered)),
              radii_out=arr(radii), geom_buffer=arr(geoms), debug=int(bool(debug)), stream=_stream(dev),
              view_streams=vst, **{counts: nr})
    out = [(int(nr[k]), radii[k], geoms[k], bounded) for k in range(K)]
    W0, H0 = int(image_widths[0]), int(image_heights[0])
    if os.environ.get("GSRAST_BATCH_VIEWS", "1") != "0" and all(
            int(w) == W0 and int(h) == H0 for w, h in zip(image_widths, image_heights)):
        # the K views' binning (duplicate, tile sort, ranges) as one set of launches: every binning
        # buffer is a slice of one allocation, sized for the largest count, which then stands for
        # every view's num_rendered (buffer layout, backward scratch)
        I = max(int(nr[k]) for k in range(K))
        bb, ib = _lib.gs_binning_buffer_bytes(I, W0, H0), _lib.gs_image_buffer_bytes(W0, H0)
        bin_all, img_all = torch.empty((K * bb,), **u8), torch.empty((K * ib,), **u8)
        bins = [bin_all[k * bb:(k + 1) * bb] for k in range(K)]
        imgs = [img_all[k * ib:(k + 1) * ib] for k in range(K)]
        with torch.cuda.device(dev):
            _call("gs_forward_bin_views", "preprocess_views (binning)", K=K, P=x.P, image_width=W0, image_height=H0,
                  geom_buffer=arr(geoms), num_rendered=nr, binning_buffer=arr(bins), image_buffer=arr(imgs),
                  debug=int(bool(debug)), stream=_stream(dev), view_streams=vst)
        out = [(I, radii[k], geoms[k], bounded, bins[k], imgs[k]) for k in range(K)]
    if streams is not None:  # the buffers are used on the views' streams
        for k, s in enumerate(streams):
            for t in out[k][1:]:
                if isinstance(t, torch.Tensor):
                    t.record_stream(s)
    return out


# instance count of the last forward that read it back (bounded forwards do not): a base for a
# binning capacity (last_num_rendered())
_LAST_NUM_RENDERED = [0]


def bounded_status():
    """(flags, instances) that bounded forwards left on the current device since the last call
    (gs_bounded_status; clears them).  Raises RuntimeError when a flag is set."""
    flags, inst = ctypes.c_uint(0), ctypes.c_longlong(0)
    rc = _lib.gs_bounded_status(ctypes.byref(flags), ctypes.byref(inst))
    if rc != 0:
        raise RuntimeError(f"bounded forward: {_native.last_error()}")
    return int(flags.value), int(inst.value)


# forward error flags (include/gsrast.h; gs_internal.h ERR_*): a view with ERR_INVALID set is skipped
# by the backward's record sums and by the fused backward + Adam
ERR_PREFILTERED, ERR_LOOKBACK, ERR_INSTANCES, ERR_CAPACITY = 1, 4, 8, 16
ERR_INVALID = ERR_LOOKBACK | ERR_CAPACITY


def view_flags_word(geom_buffer: torch.Tensor, P: int) -> torch.Tensor:
    """The int32 word of a view's geometry buffer that holds its forward error flags
    (gs_geom_flags_offset, ABI v17), as a one-element device tensor view: copy it out behind the
    forward (non_blocking into pinned memory) to read the view's status at a later sync."""
    off = int(_lib.gs_geom_flags_offset(int(P)))
    if geom_buffer.dtype != torch.uint8 or geom_buffer.numel() < off + 4:
        raise ValueError("view_flags_word: not a geometry buffer of this P")
    return geom_buffer[off:off + 4].view(torch.int32)


class row_waits:
    """Context manager (extension, ABI v17 gs_set_row_waits): the next forward preprocess on this
    thread inside the block launches in Gaussian-row chunks, each behind a stream wait on its
    chunk's event.  waits: [(lo, hi, torch.cuda.Event or None)] covering [0, P) in order.  The
    waits are cleared on exit whether or not a preprocess consumed them."""

    def __init__(self, waits):
        self.waits = list(waits or [])

    def __enter__(self):
        w = self.waits
        if not w:
            return self
        if w[0][0] != 0 or any(w[k][1] != w[k + 1][0] for k in range(len(w) - 1)):
            raise ValueError("row_waits: chunks must be contiguous from row 0")
        bounds = (ctypes.c_int * (len(w) + 1))(*([w[0][0]] + [hi for _, hi, _ in w]))
        evs = (ctypes.c_void_p * len(w))(*[e.cuda_event if e is not None else None for _, _, e in w])
        self._keep = (bounds, evs)
        _native.check(_lib.gs_set_row_waits(len(w), ctypes.cast(bounds, ctypes.c_void_p),
                                            ctypes.cast(evs, ctypes.c_void_p)), "row waits")
        return self

    def __exit__(self, *exc):
        if self.waits:
            _lib.gs_set_row_waits(0, None, None)
        return False


def forward_order_status() -> None:
    """Take the ordering flags of every queued read-back forward on the current device (waits for
    their renders; gs_forward_order_status, ABI v17).  Raises RuntimeError when a look-back wait of
    one of them timed out -- that report is then consumed, not repeated by the next call."""
    if _lib.gs_forward_order_status() != 0:
        raise RuntimeError(_native.last_error())


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, prepared=None, sh_rest=None, capacity=None):
    """prepared: (num_rendered, radii, geomBuffer) of this call from preprocess_views (the first
    half already ran); otherwise both halves run here.  sh_rest: split SH rows (sh is then
    features_dc [P,1,3], sh_rest features_rest [P,M-1,3]; gs_forward_preprocess_split).
    capacity: the binning buffer is sized for that many instances and the whole forward is
    enqueued without a host wait (gs_forward_bounded); the returned num_rendered is the capacity."""
    if _EXT is not None and prepared is not None and capacity is None and sh_rest is None and means3D.is_cuda:
        return _EXT.forward_prepared(background, means3D, viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy),
                                     int(image_height), int(image_width), campos, bool(debug), tuple(prepared))
    if _EXT is not None and prepared is None and capacity is not None and means3D.is_cuda:
        return _EXT.forward_bounded(background, means3D, colors, opacity, scales, rotations, float(scale_modifier),
                                    cov3D_precomp, viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy),
                                    int(image_height), int(image_width), sh, int(degree), campos, bool(prefiltered),
                                    bool(debug), sh_rest, int(capacity))
    if _EXT is not None and prepared is None and capacity is None and means3D.is_cuda:
        out = _EXT.forward(background, means3D, colors, opacity, scales, rotations, float(scale_modifier),
                           cov3D_precomp, viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), int(image_height),
                           int(image_width), sh, int(degree), campos, bool(prefiltered), bool(debug), sh_rest)
        _LAST_NUM_RENDERED[0] = out[0]
        return out
    x = _Inputs(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
                campos, sh_rest=sh_rest)
    if prepared is not None and x.sh_rest is not None:
        raise RuntimeError("split SH rows are not supported with prepared views")
    if prepared is not None and capacity is not None:
        raise RuntimeError("a binning capacity is not supported with prepared views")
    return _forward_ctypes(x, int(image_height), int(image_width), degree, scale_modifier, tan_fovx, tan_fovy,
                           prefiltered, debug, prepared=prepared, capacity=capacity)


def _forward_ctypes(x, H, W, degree, scale_modifier, tan_fovx, tan_fovy, prefiltered, debug, prepared=None,
                    capacity=None, aux=False, antialiasing=False):
    """The forward of validated inputs over ctypes: rasterize_gaussians' six values, and with aux
    (the two-call path only) the render's (invdepth [1, H, W], alpha [1, H, W]) behind them.
    antialiasing (the two-call path only): the preprocess scales the opacities (gs_forward_preprocess_aa)."""
    if antialiasing and (prepared is not None or capacity is not None):
        raise RuntimeError("antialiasing: not supported with " + ("prepared=" if prepared is not None
                                                                  else "binning_capacity="))
    dev = x.device
    u8 = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    if x.P == 0:
        # upstream: nothing is launched for an empty scene; the images stay all-zero (no background)
        return (0, torch.zeros((3, H, W), **f32), torch.zeros((0,), dtype=torch.int32, device=dev),
                torch.empty((0,), **u8), torch.empty((0,), **u8), torch.empty((0,), **u8)) + tuple(
                    torch.zeros((1, H, W), **f32) for _ in range(2 if aux else 0))
    # every pixel of the images and every radius is written by the kernels
    out_color = torch.empty((3, H, W), **f32)
    planes = tuple(torch.empty((1, H, W), **f32) for _ in range(2 if aux else 0))  # invdepth, alpha
    if capacity is not None:
        capacity = int(capacity)
        radii = torch.empty((x.P,), dtype=torch.int32, device=dev)
        geom = torch.empty((_lib.gs_geom_buffer_bytes(x.P),), **u8)
        binning = torch.empty((_lib.gs_binning_buffer_bytes(capacity, W, H),), **u8)
        img = torch.empty((_lib.gs_image_buffer_bytes(W, H),), **u8)
        with torch.cuda.device(dev):
            _call("gs_forward_bounded", "rasterize_gaussians (bounded)", **x.head(W, H, degree),
                  **x.scene(scale_modifier), **x.camera(tan_fovx, tan_fovy), prefiltered=int(bool(prefiltered)),
                  radii_out=_ptr(radii), geom_buffer=_ptr(geom), capacity=capacity, binning_buffer=_ptr(binning),
                  image_buffer=_ptr(img), out_color=_ptr(out_color), debug=int(bool(debug)), stream=_stream(dev))
        return capacity, out_color, radii, geom, binning, img
    with torch.cuda.device(dev):
        st = _stream(dev)
        bounded = False
        if prepared is not None:
            num_rendered, radii, geom = prepared[:3]
            bounded = len(prepared) > 3 and prepared[3]
            if radii.numel() != x.P or geom.numel() != _lib.gs_geom_buffer_bytes(x.P):
                raise RuntimeError("rasterize_gaussians: the prepared view does not match these inputs")
            if len(prepared) > 4:  # binned with the other prepared views: the compositing only
                binning, img = prepared[4], prepared[5]
                if img.numel() != _lib.gs_image_buffer_bytes(W, H):
                    raise RuntimeError("rasterize_gaussians: the prepared view was binned for another image size")
                _call("gs_forward_render_binned", "rasterize_gaussians (render)", **x.head(W, H),
                      **x.camera(tan_fovx, tan_fovy), geom_buffer=_ptr(geom), num_rendered=num_rendered,
                      binning_buffer=_ptr(binning), image_buffer=_ptr(img), out_color=_ptr(out_color),
                      bounded=int(bool(bounded)), debug=int(bool(debug)), stream=st)
                return num_rendered, out_color, radii, geom, binning, img
        else:
            num_rendered, radii, geom = x.preprocess(W, H, degree, scale_modifier, tan_fovx, tan_fovy, prefiltered,
                                                     debug, st, antialiasing=antialiasing)
        binning = torch.empty((_lib.gs_binning_buffer_bytes(num_rendered, W, H),), **u8)
        img = torch.empty((_lib.gs_image_buffer_bytes(W, H),), **u8)
        args = dict(x.head(W, H), **x.camera(tan_fovx, tan_fovy), radii=_ptr(radii), geom_buffer=_ptr(geom),
                    binning_buffer=_ptr(binning), image_buffer=_ptr(img), out_color=_ptr(out_color),
                    debug=int(bool(debug)), stream=st)
        if bounded and not aux:  # its own mode (the sticky status), not gs_forward_render_aux's family
            _call("gs_forward_render_bounded", "rasterize_gaussians (render)", capacity=num_rendered, **args)
        else:
            invdepth, alpha = planes or (None, None)
            _call("gs_forward_render_aux", "rasterize_gaussians (render%s)" % (", aux outputs" if aux else ""),
                  num_rendered=num_rendered, out_invdepth=_ptr(invdepth), out_alpha=_ptr(alpha), **args)
    return (num_rendered, out_color, radii, geom, binning, img) + planes


def rasterize_gaussians_aux(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                            viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                            prefiltered, debug, sh_rest=None):
    """rasterize_gaussians plus the render's aux outputs (gs_forward_render_aux): returns its six
    values and (invdepth [1, H, W], alpha [1, H, W]).  Always the two-call path over ctypes."""
    x = _Inputs(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
                campos, sh_rest=sh_rest)
    return _forward_ctypes(x, int(image_height), int(image_width), degree, scale_modifier, tan_fovx, tan_fovy,
                           prefiltered, debug, aux=True)


def rasterize_gaussians_aa(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                           viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                           prefiltered, debug, aux=False):
    """rasterize_gaussians with antialiasing (gs_forward_preprocess_aa): every splat's opacity is scaled
    by sqrt(det cov2D / det(cov2D + 0.3 I)) (floor 0.005) where it enters the splat record and the
    culling limit; with aux also rasterize_gaussians_aux's two planes.  Always the two-call path over
    ctypes; the backward of such a forward is backward_impl(..., aa_opacity=opacity)."""
    x = _Inputs(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
                campos)
    return _forward_ctypes(x, int(image_height), int(image_width), degree, scale_modifier, tan_fovx, tan_fovy,
                           prefiltered, debug, aux=bool(aux), antialiasing=True)


def rasterize_gaussians_two_call(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width,
                                 sh, degree, campos, prefiltered, debug, sh_rest=None, antialiasing=False):
    """rasterize_gaussians, always as the two-call forward over ctypes (gs_forward_preprocess, _split or
    _aa, then gs_forward_render): the forward contribution_stats is defined for.  Same six values and
    the same bits as rasterize_gaussians / rasterize_gaussians_aa."""
    x = _Inputs(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
                campos, sh_rest=sh_rest)
    return _forward_ctypes(x, int(image_height), int(image_width), degree, scale_modifier, tan_fovx, tan_fovy,
                           prefiltered, debug, antialiasing=bool(antialiasing))


def contribution_stats(R, radii, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, campos, tan_fovx,
                       tan_fovy, image_height, image_width, debug=False, pixel_weights=None, out=None):
    """Per-Gaussian contribution statistics of one rendered view (gs_contrib_stats, include/gsrast.h):
    (wsum [P] fp32, wmax [P] fp32, count [P] int32) from the buffers of a two-call forward
    (rasterize_gaussians_two_call / _aux / _aa), before or after that view's backward.
    pixel_weights: an [H, W] fp32 device map m >= 0 (None: 1); a pixel of weight 0 adds nothing.
    out: (wsum, wmax, count) to combine with in place (sum, max, sum); they are returned."""
    _dev_check(radii, "radii")
    dev = radii.device
    P, H, W = int(radii.numel()), int(image_height), int(image_width)
    if out is None:
        # every row is written by the kernels (P == 0 or no instance: zero-filled by the library)
        stats = (torch.empty((P,), dtype=torch.float32, device=dev), torch.empty((P,), dtype=torch.float32, device=dev),
                 torch.empty((P,), dtype=torch.int32, device=dev))
    else:
        stats = tuple(out)
        for t, dt, n in zip(stats, (torch.float32, torch.float32, torch.int32), ("wsum", "wmax", "count")):
            if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != P:
                raise RuntimeError(f"contribution_stats: out {n} must be a contiguous {dt} tensor of {P} elements "
                                   f"on {dev}")
    if P == 0:
        return stats
    m = None
    if pixel_weights is not None:
        m = _f32(pixel_weights, "pixel_weights", dev, allow_empty=False)
        if m.numel() != H * W:
            raise RuntimeError("pixel_weights must have shape (H, W)")
    _, view, proj, cam = _camera_side(dev, None, viewmatrix, projmatrix, campos)
    R = binning_layout_count(R, binningBuffer, W, H)
    with torch.cuda.device(dev):
        scratch = torch.empty((_lib.gs_contrib_scratch_bytes(R),), dtype=torch.uint8, device=dev)
        _call("gs_contrib_stats", "contribution_stats", P=P, image_width=W, image_height=H,
              **_camera(view, proj, cam, tan_fovx, tan_fovy), radii=_ptr(radii), geom_buffer=_ptr(geomBuffer),
              num_rendered=int(R), binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer),
              pixel_weights=_ptr(m), scratch=_ptr(scratch), wsum=_ptr(stats[0]), wmax=_ptr(stats[1]),
              count=_ptr(stats[2]), accumulate=int(out is not None), debug=int(bool(debug)), stream=_stream(dev))
    return stats


def feature_group_channels():
    """Channels one walk of the lists carries (gs_feature_group_channels)."""
    return int(_lib.gs_feature_group_channels())


def _feature_matrix(t, name, P, dev):
    """[P, C] (features) as a contiguous fp32 device tensor; C >= 1 (the library refuses a C beyond its limit)"""
    if t.ndimension() != 2 or t.size(0) != P or t.size(1) < 1:
        raise RuntimeError(f"{name} must have shape ({P}, C) with C >= 1 (got {tuple(t.shape)})")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if t.device != dev:
        _dev_check(t, name)
        raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
    return t.contiguous()


def feature_forward(R, radii, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, campos, tan_fovx,
                    tan_fovy, image_height, image_width, features, debug=False, out=None):
    """features [P, C] fp32 composited through one rendered view's tile lists (gs_feature_forward,
    include/gsrast.h): out [C, H, W] = sum_i f_i[c] alpha_i T_i, each channel in the form and order of
    a colour channel, no background term.  The buffers are those of a two-call forward
    (rasterize_gaussians_two_call / _aux / _aa), before or after that view's backward.
    out: a contiguous fp32 [C, H, W] device tensor to write into (every element is written)."""
    _dev_check(radii, "radii")
    dev = radii.device
    P, H, W = int(radii.numel()), int(image_height), int(image_width)
    f = _feature_matrix(features, "features", P, dev)
    C = int(f.size(1))
    if out is None:
        out = torch.empty((C, H, W), dtype=torch.float32, device=dev)  # every pixel is written by the library
    elif out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or tuple(out.shape) != (C, H, W):
        raise RuntimeError(f"feature_forward: out must be a contiguous float32 tensor of shape ({C}, {H}, {W}) on {dev}")
    _, view, proj, cam = _camera_side(dev, None, viewmatrix, projmatrix, campos)
    R = binning_layout_count(R, binningBuffer, W, H) if P > 0 else 0
    with torch.cuda.device(dev):
        _call("gs_feature_forward", "feature_forward", P=P, C=C, image_width=W, image_height=H,
              **_camera(view, proj, cam, tan_fovx, tan_fovy), radii=_ptr(radii), geom_buffer=_ptr(geomBuffer),
              num_rendered=int(R), binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer),
              features=_ptr(f), out=_ptr(out), debug=int(bool(debug)), stream=_stream(dev))
    return out


def feature_backward(R, radii, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, campos, tan_fovx,
                     tan_fovy, image_height, image_width, dL_dout, debug=False, out=None):
    """The gradient of feature_forward in the features (gs_feature_backward): dL_dout [C, H, W] fp32 ->
    dL_dfeatures [P, C] = sum_p alpha_i T_i dL_dout[c, p], contribution_stats' wsum per channel.
    out: a contiguous fp32 [P, C] device tensor to ADD to in place (one fp32 add per element); it is returned."""
    _dev_check(radii, "radii")
    dev = radii.device
    P, H, W = int(radii.numel()), int(image_height), int(image_width)
    if dL_dout.ndimension() != 3 or dL_dout.size(0) < 1 or tuple(dL_dout.shape[1:]) != (H, W):
        raise RuntimeError(f"dL_dout must have shape (C, {H}, {W}) with C >= 1 (got {tuple(dL_dout.shape)})")
    g = _f32(dL_dout, "dL_dout", dev, allow_empty=False)
    C = int(g.size(0))
    if out is None:
        grad = torch.empty((P, C), dtype=torch.float32, device=dev)  # every row is written by the library
    else:
        grad = out
        if grad.dtype != torch.float32 or grad.device != dev or not grad.is_contiguous() or tuple(grad.shape) != (P, C):
            raise RuntimeError(f"feature_backward: out must be a contiguous float32 tensor of shape ({P}, {C}) on {dev}")
    _, view, proj, cam = _camera_side(dev, None, viewmatrix, projmatrix, campos)
    R = binning_layout_count(R, binningBuffer, W, H) if P > 0 else 0
    with torch.cuda.device(dev):
        scratch = torch.empty((_lib.gs_feature_scratch_bytes(R),), dtype=torch.uint8, device=dev)
        _call("gs_feature_backward", "feature_backward", P=P, C=C, image_width=W, image_height=H,
              **_camera(view, proj, cam, tan_fovx, tan_fovy), radii=_ptr(radii), geom_buffer=_ptr(geomBuffer),
              num_rendered=int(R), binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer),
              dL_dout=_ptr(g), scratch=_ptr(scratch), dL_dfeatures=_ptr(grad), accumulate=int(out is not None),
              debug=int(bool(debug)), stream=_stream(dev))
    return grad


def binning_layout_count(R, binningBuffer, W, H):
    """The instance count binningBuffer is laid out for, which the C-ABI calls take as num_rendered:
    R for a buffer of gs_binning_buffer_bytes(R) bytes (the two-call, bounded and prepared
    forwards); for a buffer the eager forward sized ahead of its count (gs_forward_counted: the
    returned num_rendered is the exact count, the buffer holds the capacity) that capacity."""
    R = int(R)
    n = binningBuffer.numel()
    if n == _lib.gs_binning_buffer_bytes(R, W, H):
        return R
    L = int(_lib.gs_binning_layout_count(n, W, H))
    if L < R:
        raise RuntimeError(f"binningBuffer ({n} bytes) is too small for num_rendered = {R}")
    return L


# gradient outputs of the backward, in the upstream return order, with their GS_ACC_* bit
GRAD_NAMES = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
GS_ACC = {n: 1 << k for k, n in enumerate(GRAD_NAMES)}


def backward_impl(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                  projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                  imageBuffer, debug, want_all=True, sinks=None, wait_event=None, sh_rest=None, aux_grads=None,
                  camera=None, aa_opacity=None, absgrad=False):
    """Shared backward.  With want_all=False the gradients that no autograd input can receive
    (colours when SHs drive the colour, cov3D when scale/rotation drive it, ...) are None and
    not computed.  sinks: {name: (buffer, accumulate)} -- that gradient is written into (or, with
    accumulate, added to) the caller's buffer, which is returned in its place
    (the GS_ACC bits; multi-view gradient buckets, gs_view_parallel.GradBucket).
    wait_event: torch.cuda.Event the stream waits for before the kernel that writes the gradients
    (a sink shared with views on other streams).  sh_rest: split SH rows as rasterize_gaussians;
    the `sh` gradient is then that of the concatenation, [P, M, 3].
    aux_grads: (dL_dout_invdepth, dL_dout_alpha) of a rasterize_gaussians_aux forward, either may be
    None (over ctypes).
    camera: None, or whether dL/dcampos is wanted -- the return then ends with one more item, the
    view's camera gradients (dL_dviewmatrix [4, 4], dL_dprojmatrix [4, 4], dL_dcampos [3] or None) of
    gs_backward_camera_aa, run right behind the backward on its stream (over ctypes).
    aa_opacity: the opacities [P, 1] of a rasterize_gaussians_aa forward -- the backward of an antialiased
    view (over ctypes), which chains through the opacity scale and so reads them; None: a plain
    forward's backward.
    absgrad: the return ends with one more item (after the camera gradients), the view's absolute
    screen-space gradient [P, 3] (over ctypes; with sh_rest, aux_grads, camera and aa_opacity as above).
    Every combination is one call of gs_backward_accumulate_absgrad, the widest entry of its family."""
    if aux_grads is not None and aux_grads[0] is None and aux_grads[1] is None:
        aux_grads = None
    antialiasing = aa_opacity is not None
    if antialiasing and sh_rest is not None:
        raise RuntimeError("antialiasing: not supported with sh_split=")
    if camera is not None and sh_rest is not None:
        raise RuntimeError("camera_grads: not supported with split SH rows (sh_split=)")
    if (_EXT is not None and not want_all and means3D.is_cuda and aux_grads is None and camera is None
            and not antialiasing and not absgrad):
        return _EXT.backward(background, means3D, radii, colors, scales, rotations, float(scale_modifier),
                             cov3D_precomp, viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color,
                             sh, int(degree), campos, geomBuffer, int(R), binningBuffer, imageBuffer, bool(debug),
                             sh_rest, sinks or {}, wait_event.cuda_event if wait_event is not None else 0)
    x = _Inputs(background, means3D, colors, aa_opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
                campos, need_opacity=antialiasing, sh_rest=sh_rest)
    P, dev = x.P, x.device
    f32 = dict(dtype=torch.float32, device=dev)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = x.M
    sinks = sinks or {}
    need_col = want_all or x.colors is not None
    need_cov = want_all or x.cov3D is not None
    need_sh = want_all or x.sh is not None
    need_sr = want_all or (x.scales is not None and x.rotations is not None)
    has_sr = x.scales is not None and x.rotations is not None and x.cov3D is None
    shapes = dict(means2D=(P, 3), colors=(P, 3), opacity=(P, 1), means3D=(P, 3), cov3D=(P, 6), sh=(P, M, 3),
                  scales=(P, 3), rotations=(P, 4))
    # is the gradient computed by the kernels (else zero-filled or absent)?  Split SH rows are SH colours
    # (no colors_precomp: _Inputs): dL/dcolors is not asked of the library, and with want_all it is zeros
    computed = dict(means2D=True, colors=x.sh_rest is None, opacity=True, means3D=True,
                    cov3D=x.cov3D is not None or (want_all and has_sr), sh=x.sh is not None, scales=has_sr,
                    rotations=has_sr)
    needed = dict(means2D=True, colors=need_col, opacity=True, means3D=True, cov3D=need_cov, sh=need_sh,
                  scales=need_sr, rotations=need_sr)
    acc = 0
    outs = {}
    for n in GRAD_NAMES:
        if n in sinks and computed[n]:
            buf, accumulate = sinks[n]
            if (buf.dtype != torch.float32 or buf.device != dev or not buf.is_contiguous()
                    or buf.numel() != math.prod(shapes[n])):
                raise RuntimeError(f"gradient sink for {n}: expected a contiguous float32 buffer of "
                                   f"{math.prod(shapes[n])} elements on {dev}")
            outs[n] = buf
            acc |= GS_ACC[n] if accumulate else 0
        elif needed[n]:
            outs[n] = (torch.empty if computed[n] else torch.zeros)(shapes[n], **f32)
        else:
            outs[n] = None
    ret = tuple(outs[n] for n in GRAD_NAMES)
    if camera is not None:  # written by the finishing kernel, structural zeros included (P == 0: no launch)
        cam_out = (torch.zeros if P == 0 else torch.empty)((35,), **f32)
        ret += ((cam_out[:16].view(4, 4), cam_out[16:32].view(4, 4), cam_out[32:] if camera else None),)
    abs_out = None
    if absgrad:  # written by its kernel, zero rows included (P == 0: no launch)
        abs_out = torch.empty((P, 3), **f32)
        ret += (abs_out,)
    if P == 0:
        return ret
    dpix = _f32(dL_dout_color, "dL_dout_color", dev)
    grads = {"dL_d" + n: _ptr(outs[n] if computed[n] else None) for n in GRAD_NAMES}
    R = binning_layout_count(R, binningBuffer, W, H)
    with torch.cuda.device(dev):
        st = _stream(dev)
        d_inv, d_alpha = _aux_grads(aux_grads, H, W, dev)
        what = "rasterize_gaussians_backward" + (" (aux outputs)" if aux_grads is not None else "")
        if absgrad:
            n_scratch = _lib.gs_grad_buffer_bytes_absgrad(R, P)
            what += " (antialiasing, absgrad)" if antialiasing else " (absgrad)"
        else:
            n_scratch = _lib.gs_grad_buffer_bytes(R) if aux_grads is None else _lib.gs_grad_buffer_bytes_aux(R, P)
            what += " (antialiasing)" if antialiasing else ""
        grad_scratch = torch.empty((n_scratch,), dtype=torch.uint8, device=dev)
        _call("gs_backward_accumulate_absgrad", what, **x.head(W, H, degree), **x.scene(scale_modifier),
              **x.camera(tan_fovx, tan_fovy), radii=_ptr(radii), geom_buffer=_ptr(geomBuffer), num_rendered=int(R),
              binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer), dL_dout_color=_ptr(dpix),
              dL_dout_invdepth=_ptr(d_inv), dL_dout_alpha=_ptr(d_alpha), grad_buffer=_ptr(grad_scratch),
              **grads, accumulate=acc,
              wait_event=ctypes.c_void_p(wait_event.cuda_event) if wait_event is not None else None,
              debug=int(bool(debug)), stream=st, antialiasing=int(antialiasing), dL_dmeans2D_abs=_ptr(abs_out))
        if camera is not None:
            cam_scratch = torch.empty((_lib.gs_camera_grad_scratch_bytes(P),), dtype=torch.uint8, device=dev)
            _call("gs_backward_camera_aa", "rasterize_gaussians_backward (camera gradients)", **x.head(W, H, degree),
                  **x.scene(scale_modifier, rest=False), **x.camera(tan_fovx, tan_fovy), geom_buffer=_ptr(geomBuffer),
                  num_rendered=int(R), aux_grad_buffer=_ptr(grad_scratch) if aux_grads is not None else None,
                  aux_valid=int(aux_grads is not None), scratch=_ptr(cam_scratch), dL_dviewmatrix=_ptr(cam_out),
                  dL_dprojmatrix=ctypes.c_void_p(cam_out.data_ptr() + 64),
                  dL_dcampos=ctypes.c_void_p(cam_out.data_ptr() + 128) if camera else None, debug=int(bool(debug)),
                  stream=st, antialiasing=int(antialiasing))
    return ret


def backward_render(background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, dL_dout_color, P, degree, M,
                    geomBuffer, R, binningBuffer, imageBuffer, want_means2D, debug, aux_grads=None):
    """Per-tile half of the backward (gs_backward_render_aux): the view's per-Gaussian record sums,
    kept in geomBuffer for backward_gaussians, and its dL_dmeans2D [P, 3] (or None).
    aux_grads: (dL_dout_invdepth, dL_dout_alpha) of a rasterize_gaussians_aux forward, either may be
    None (over ctypes); the return is then (dL_dmeans2D, invdepth_sums): the
    [P] per-Gaussian dL/d(1 / z) sums of the depth chain (written for Gaussians with instances only),
    the input of FusedAdam.prepare_fused_backward."""
    if aux_grads is not None and aux_grads[0] is None and aux_grads[1] is None:
        aux_grads = None
    aux = aux_grads is not None
    if not aux and _EXT is not None and geomBuffer.is_cuda:
        return _EXT.backward_render(background, viewmatrix, projmatrix, campos, float(tan_fovx), float(tan_fovy),
                                    dL_dout_color, int(P), int(degree), int(M), geomBuffer, int(R), binningBuffer,
                                    imageBuffer, bool(want_means2D), bool(debug))
    dev = geomBuffer.device
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    dm2 = torch.empty((P, 3), dtype=torch.float32, device=dev) if want_means2D else None
    sums = torch.empty((P,), dtype=torch.float32, device=dev) if aux else None
    ret = (dm2, sums) if aux else dm2
    if P == 0:
        return ret
    bg, view, proj, cam = _camera_side(dev, background, viewmatrix, projmatrix, campos)
    dpix = _f32(dL_dout_color, "dL_dout_color", dev)
    d_inv, d_alpha = _aux_grads(aux_grads, H, W, dev)
    R = binning_layout_count(R, binningBuffer, W, H)
    with torch.cuda.device(dev):
        n_scratch = _lib.gs_grad_buffer_bytes_aux(R, P) if aux else _lib.gs_grad_buffer_bytes(R)
        grad_scratch = torch.empty((n_scratch,), dtype=torch.uint8, device=dev)
        what = "rasterize_gaussians_backward (render half%s)" % (", aux outputs" if aux else "")
        _call("gs_backward_render_aux", what, P=P, D=int(degree), M=int(M), background=_ptr(bg), image_width=W,
              image_height=H, **_camera(view, proj, cam, tan_fovx, tan_fovy), geom_buffer=_ptr(geomBuffer),
              num_rendered=int(R), binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer),
              dL_dout_color=_ptr(dpix), dL_dout_invdepth=_ptr(d_inv), dL_dout_alpha=_ptr(d_alpha),
              grad_buffer=_ptr(grad_scratch), dL_dmeans2D=_ptr(dm2), invdepth_sums=_ptr(sums), accumulate=0,
              debug=int(bool(debug)), stream=_stream(dev))
    return ret


def backward_gaussians(means3D, sh, colors, scales, rotations, cov3D_precomp, scale_modifier, degree, views, outs,
                       accumulate, wait_event=None, debug=False, first=0, count=None):
    """Per-Gaussian half of the backward for several views at once (gs_backward_gaussians).
    views: [(viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, W, H, geomBuffer)] in order (each
    after its backward_render); outs: {name: buffer} for colors / opacity / means3D / cov3D / sh /
    scales / rotations (absent: not produced); accumulate: GS_ACC bits of the first view.
    first / count: only the Gaussians [first, first + count) (gs_backward_gaussians_range)."""
    if _EXT is not None and means3D.is_cuda:
        return _EXT.backward_gaussians(means3D, sh, colors, scales, rotations, cov3D_precomp, float(scale_modifier),
                                       int(degree), views, outs, int(accumulate),
                                       wait_event.cuda_event if wait_event is not None else 0, bool(debug),
                                       int(first), -1 if count is None else int(count))
    x = _Inputs(None, means3D, colors, None, scales, rotations, cov3D_precomp, views[0][0],
                views[0][1], sh, views[0][2], need_opacity=False)
    P, dev = x.P, x.device
    if P == 0 or not views:
        return
    arr = (_native.ViewGrad * len(views))()
    keep = []
    for k, (vm, pm, cp, tx, ty, W, H, geom) in enumerate(views):
        _, vm, pm, cp = _camera_side(dev, None, vm, pm, cp)
        keep += [vm, pm, cp]
        arr[k] = _native.ViewGrad(vm.data_ptr(), pm.data_ptr(), cp.data_ptr() if cp is not None else None,
                                  float(tx), float(ty), int(W), int(H), geom.data_ptr())
    o = {n: outs.get(n) for n in ("colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")}
    for n, t in o.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
            raise RuntimeError(f"backward_gaussians: {n} output must be a contiguous float32 tensor on {dev}")
    count = P - int(first) if count is None else int(count)
    with torch.cuda.device(dev):
        _call("gs_backward_gaussians_range", "rasterize_gaussians_backward (per-Gaussian half)", P=P, first=int(first),
              count=count, D=int(degree), M=x.M, means3D=_ptr(x.means3D), shs=_ptr(x.sh),
              colors_precomp=_ptr(x.colors), scales=_ptr(x.scales), scale_modifier=float(scale_modifier),
              rotations=_ptr(x.rotations), cov3D_precomp=_ptr(x.cov3D), num_views=len(views), views=arr,
              dL_dcolors=_ptr(o["colors"]), dL_dopacity=_ptr(o["opacity"]), dL_dmeans3D=_ptr(o["means3D"]),
              dL_dcov3D=_ptr(o["cov3D"]), dL_dsh=_ptr(o["sh"]), dL_dscales=_ptr(o["scales"]),
              dL_drotations=_ptr(o["rotations"]), accumulate=int(accumulate),
              wait_event=ctypes.c_void_p(wait_event.cuda_event) if wait_event is not None else None,
              debug=int(bool(debug)), stream=_stream(dev))


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                 degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug):
    return backward_impl(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                         viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer,
                         R, binningBuffer, imageBuffer, debug, want_all=True)


def mark_visible(means3D, viewmatrix, projmatrix):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _dev_check(means3D, "means3D")
    dev = means3D.device
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P == 0:
        return present
    m = _f32(means3D, "means3D", dev)
    _, v, p, _ = _camera_side(dev, None, viewmatrix, projmatrix, None)
    with torch.cuda.device(dev):
        _native.check(_lib.gs_mark_visible(P, _ptr(m), _ptr(v), _ptr(p), _ptr(present), _stream(dev)), "mark_visible")
    return present


def debug_export(P, W, H, num_rendered, geomBuffer, binningBuffer, imageBuffer, device):
    """Forward intermediates for tests: dict of device tensors."""
    u32 = dict(dtype=torch.int32, device=device)
    f32 = dict(dtype=torch.float32, device=device)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    L = binning_layout_count(num_rendered, binningBuffer, W, H) if P > 0 else int(num_rendered)
    out = dict(
        point_list=torch.zeros((max(L, 1),), **u32),
        ranges=torch.zeros((gx * gy, 2), **u32),
        xy=torch.zeros((P, 2), **f32),
        conic_opacity=torch.zeros((P, 4), **f32),
        rgb=torch.zeros((P, 3), **f32),
        depth=torch.zeros((P,), **f32),
        tiles_touched=torch.zeros((P,), **u32),
        final_T=torch.zeros((H, W), **f32),
        n_contrib=torch.zeros((H, W), **u32),
    )
    if P > 0:
        with torch.cuda.device(device):
            # (the outputs carry the entry's parameter names)
            _call("gs_debug_export", "debug_export", P=P, image_width=W, image_height=H, num_rendered=L,
                  geom_buffer=_ptr(geomBuffer), binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer),
                  stream=_stream(device), **{k: _ptr(t) for k, t in out.items()})
    out["point_list"] = out["point_list"][:num_rendered]
    return out


def debug_export_slots(W, H, num_rendered, binningBuffer, imageBuffer, device):
    """(slots[num_rendered], tile_cut[tiles]) as int32 device tensors: the depth-ordered instance slot of
    each entry of the tile-sorted list and each tile's backward record cut (valid after a backward)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    L = binning_layout_count(num_rendered, binningBuffer, W, H)
    slots = torch.zeros((max(L, 1),), dtype=torch.int32, device=device)
    cuts = torch.zeros((gx * gy,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _call("gs_debug_export_slots", "debug_export_slots", image_width=W, image_height=H, num_rendered=L,
              binning_buffer=_ptr(binningBuffer), image_buffer=_ptr(imageBuffer), slots=_ptr(slots),
              tile_cut=_ptr(cuts), stream=_stream(device))
    return slots[:int(num_rendered)], cuts
