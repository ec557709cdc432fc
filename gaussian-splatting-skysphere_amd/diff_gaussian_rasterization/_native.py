"""Loader for libgsrast.so, the MI355X (gfx950) HIP rasterizer behind include/gsrast.h.

There is no fallback: if the shared library is missing or does not load, importing
`diff_gaussian_rasterization._C` raises.  Build it with `make -C gaussian-splatting-skysphere_amd`
(or `python __graft_entry__.py build`).
"""
from __future__ import annotations

import ctypes
import operator
import os

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("GSRAST_LIB", os.path.join(_PKG_ROOT, "build", "libgsrast.so"))

_i = ctypes.c_int
_ll = ctypes.c_longlong
_sz = ctypes.c_size_t
_u = ctypes.c_uint
_s = ctypes.c_char_p


class ViewGrad(ctypes.Structure):
    """gs_view_grad (include/gsrast.h): one view of a multi-view per-Gaussian backward."""
    _fields_ = [("viewmatrix", ctypes.c_void_p), ("projmatrix", ctypes.c_void_p), ("campos", ctypes.c_void_p),
                ("tan_fovx", ctypes.c_float), ("tan_fovy", ctypes.c_float), ("image_width", ctypes.c_int),
                ("image_height", ctypes.c_int), ("geom_buffer", ctypes.c_void_p)]


_CODES = {"": ctypes.c_void_p, "i": _i, "ll": _ll, "sz": _sz, "u": _u, "s": _s, "f": ctypes.c_float,
          "d": ctypes.c_double, "pll": ctypes.POINTER(_ll), "pu": ctypes.POINTER(_u),
          "pd": ctypes.POINTER(ctypes.c_double), "pv": ctypes.POINTER(ViewGrad)}


def _a(spec):
    """[(name, ctype)] of a run of parameters: a word is `name` (a pointer passed as c_void_p) or
    `name:code` with a code of _CODES."""
    return [(n, _CODES[c]) for n, _, c in (w.partition(":") for w in spec.split())]


# parameter groups the entries share, named as include/gsrast.h names them
HEAD = _a("P:i D:i M:i background image_width:i image_height:i")
VIEW_HEAD = _a("P:i background image_width:i image_height:i")  # the render half: no SH degree
GEOM = _a("opacities scales scale_modifier:f rotations cov3D_precomp")
SCENE = _a("means3D shs colors_precomp") + GEOM
SCENE_SPLIT = _a("means3D shs_dc shs_rest") + GEOM  # split SH rows in place of shs / colors_precomp
SCENE3 = _a("means3D shs shs_rest colors_precomp") + GEOM  # whole or split rows, or colours
GAUSS_IN = _a("means3D shs colors_precomp scales scale_modifier:f rotations cov3D_precomp")
CAMERA = _a("viewmatrix projmatrix campos tan_fovx:f tan_fovy:f")
FWD_OUT = _a("prefiltered:i radii_out geom_buffer")
TILE_BUFS = _a("geom_buffer num_rendered:ll binning_buffer image_buffer")
VIEW_BUFS = _a("radii") + TILE_BUFS
BWD_BUFS = VIEW_BUFS + _a("dL_dout_color")
AUX_GRADS = _a("dL_dout_invdepth dL_dout_alpha")
GAUSS_GRADS = _a("dL_dcolors dL_dopacity dL_dmeans3D dL_dcov3D dL_dsh dL_dscales dL_drotations")
GRADS = _a("dL_dmeans2D") + GAUSS_GRADS
TAIL = _a("debug:i stream")
ACC_TAIL = _a("accumulate:u wait_event") + TAIL
CAMERA_GRAD = (HEAD + SCENE + CAMERA + _a("geom_buffer num_rendered:ll aux_grad_buffer aux_valid:i scratch "
                                          "dL_dviewmatrix dL_dprojmatrix dL_dcampos") + TAIL)
VIEWS_FRONT = (_a("K:i P:i D:i M:i background image_width image_height") + SCENE
               + _a("viewmatrix projmatrix campos tan_fovx tan_fovy") + FWD_OUT)  # per-view host arrays of K
VIEWS_TAIL = TAIL + _a("view_streams")
ADAM_HYPER = _a("lr_host step_host weight_decay_host beta1:d beta2:d eps:d maximize:i")
ADAM = (_a("P:i D:i M:i means3D shs_dc shs_rest scales scale_modifier:f rotations view:pv params_host exp_avg_host "
           "exp_avg_sq_host") + ADAM_HYPER)  # the fused per-Gaussian backward + Adam of one view
STATS = _a("radii grad2d grad_stride:i max_radii2D grad_accum denom")
FEATURE = _a("P:i C:i image_width:i image_height:i") + CAMERA + VIEW_BUFS
SKY = _a("W:i H:i viewmatrix tanfovx:f tanfovy:f Hs:i Ws:i texture")
SKY_BWD = SKY + _a("alpha dL_dimage dL_dalpha dL_dtexture accumulate_texture:i scratch")
LOSS = _a("planes:i H:i W:i window11_host")

# name -> (restype, [(parameter, ctype)]): the prototypes of include/gsrast.h, in its names and order
# (tests/test_native_table_cpu.py compares the two)
ENTRIES = {
    "gs_abi_version": (_i, []),
    "gs_last_error": (_s, []),
    "gs_geom_buffer_bytes": (_sz, _a("P:i")),
    "gs_binning_buffer_bytes": (_sz, _a("num_rendered:ll image_width:i image_height:i")),
    "gs_image_buffer_bytes": (_sz, _a("image_width:i image_height:i")),
    "gs_grad_buffer_bytes": (_sz, _a("num_rendered:ll")),
    "gs_binning_layout_count": (_ll, _a("bytes:sz image_width:i image_height:i")),
    "gs_forward_preprocess": (_i, HEAD + SCENE + CAMERA + FWD_OUT + _a("num_rendered_host:pll") + TAIL),
    "gs_forward_preprocess_views": (_i, VIEWS_FRONT + _a("num_rendered_host:pll") + VIEWS_TAIL),
    "gs_forward_render": (_i, VIEW_HEAD + CAMERA + VIEW_BUFS + _a("out_color") + TAIL),
    "gs_rasterize_forward": (_ll, HEAD + SCENE + CAMERA + _a("prefiltered:i out_color radii_out alloc alloc_ctx "
                                                            "geom_out binning_out image_out") + TAIL),
    "gs_backward": (_i, HEAD + SCENE + CAMERA + BWD_BUFS + _a("grad_buffer") + GRADS + TAIL),
    "gs_backward_accumulate": (_i, HEAD + SCENE + CAMERA + BWD_BUFS + _a("grad_buffer") + GRADS + ACC_TAIL),
    # ABI v8: features_dc / features_rest in place of shs (and of colors_precomp / dL_dcolors)
    "gs_forward_preprocess_split": (_i, HEAD + SCENE_SPLIT + CAMERA + FWD_OUT + _a("num_rendered:pll") + TAIL),
    "gs_backward_accumulate_split": (_i, HEAD + SCENE_SPLIT + CAMERA + BWD_BUFS + _a("grad_buffer dL_dmeans2D")
                                     + GAUSS_GRADS[1:] + ACC_TAIL),
    "gs_backward_render": (_i, HEAD + CAMERA + TILE_BUFS + _a("dL_dout_color grad_buffer dL_dmeans2D accumulate:u")
                           + TAIL),
    "gs_backward_gaussians": (_i, _a("P:i D:i M:i") + GAUSS_IN + _a("num_views:i views:pv") + GAUSS_GRADS + ACC_TAIL),
    # ABI v9: the per-Gaussian half for the Gaussians [first, first + count)
    "gs_backward_gaussians_range": (_i, _a("P:i first:i count:i D:i M:i") + GAUSS_IN + _a("num_views:i views:pv")
                                    + GAUSS_GRADS + ACC_TAIL),
    # ABI v10: the whole forward without a host wait (binning buffer sized ahead) and its sticky status
    "gs_forward_bounded": (_i, HEAD + SCENE3 + CAMERA + FWD_OUT + _a("capacity:ll binning_buffer image_buffer "
                                                                    "out_color") + TAIL),
    "gs_bounded_status": (_i, _a("flags:pu instances:pll")),
    "gs_forward_preprocess_views_bounded": (_i, VIEWS_FRONT + _a("capacity:pll") + VIEWS_TAIL),
    "gs_forward_render_bounded": (_i, VIEW_HEAD + CAMERA + _a("radii geom_buffer capacity:ll binning_buffer "
                                                              "image_buffer out_color") + TAIL),
    # ABI v11: the binning of K prepared views in one set of launches, then each view's compositing
    "gs_forward_bin_views": (_i, _a("K:i P:i image_width:i image_height:i geom_buffer num_rendered:pll binning_buffer "
                                    "image_buffer") + VIEWS_TAIL),
    "gs_forward_render_binned": (_i, VIEW_HEAD + CAMERA + TILE_BUFS + _a("out_color bounded:i") + TAIL),
    # ABI v14: the eager forward with its instance count read back at the end
    "gs_forward_counted": (_i, HEAD + SCENE3 + CAMERA + FWD_OUT + _a("capacity:ll binning_buffer image_buffer "
                                                                    "out_color num_rendered_host:pll") + TAIL),
    # ABI v15: one view's per-Gaussian backward half fused with the six groups' Adam step
    "gs_backward_gaussians_adam": (_i, ADAM + TAIL),
    # ABI v16: the same plus the view's densification statistics in that pass
    "gs_backward_gaussians_adam_stats": (_i, ADAM + STATS + TAIL),
    # ABI v17: a view's forward error-flags word (its offset in the geometry buffer) and the
    # read-back forwards' ordering status, taken in the caller's own call
    "gs_geom_flags_offset": (_sz, _a("P:i")),
    "gs_forward_order_status": (_i, []),
    "gs_set_row_waits": (_i, _a("n:i bounds events")),
    # GSRAST_HAS_AUX: the alpha / inverse-depth outputs of the render and their gradients
    "gs_grad_buffer_bytes_aux": (_sz, _a("num_rendered:ll P:i")),
    "gs_forward_render_aux": (_i, VIEW_HEAD + CAMERA + VIEW_BUFS + _a("out_color out_invdepth out_alpha") + TAIL),
    "gs_backward_accumulate_aux": (_i, HEAD + SCENE3 + CAMERA + BWD_BUFS + AUX_GRADS + _a("grad_buffer") + GRADS
                                   + ACC_TAIL),
    # GSRAST_HAS_AUX_DEFERRED: the per-tile half with the aux gradients, and the fused per-Gaussian
    # half + Adam with the inverse depth's chain
    "gs_backward_render_aux": (_i, HEAD + CAMERA + TILE_BUFS + _a("dL_dout_color") + AUX_GRADS
                               + _a("grad_buffer dL_dmeans2D invdepth_sums accumulate:u") + TAIL),
    "gs_backward_gaussians_adam_stats_aux": (_i, ADAM + STATS + _a("invdepth_sums") + TAIL),
    # GSRAST_HAS_CAMERA_GRAD: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos of one view after its backward
    "gs_camera_grad_scratch_bytes": (_sz, _a("P:i")),
    "gs_backward_camera": (_i, CAMERA_GRAD),
    # GSRAST_HAS_ANTIALIASING: the entries they extend (gs_forward_preprocess, gs_backward_accumulate_aux,
    # gs_backward_camera) plus `int antialiasing`
    "gs_forward_preprocess_aa": (_i, HEAD + SCENE + CAMERA + FWD_OUT + _a("num_rendered_host:pll") + TAIL
                                 + _a("antialiasing:i")),
    "gs_backward_accumulate_aa": (_i, HEAD + SCENE3 + CAMERA + BWD_BUFS + AUX_GRADS + _a("grad_buffer") + GRADS
                                  + ACC_TAIL + _a("antialiasing:i")),
    "gs_backward_camera_aa": (_i, CAMERA_GRAD + _a("antialiasing:i")),
    # GSRAST_HAS_ABSGRAD: gs_backward_accumulate_aa plus the absolute screen-space gradient output
    "gs_grad_buffer_bytes_absgrad": (_sz, _a("num_rendered:ll P:i")),
    "gs_backward_accumulate_absgrad": (_i, HEAD + SCENE3 + CAMERA + BWD_BUFS + AUX_GRADS + _a("grad_buffer") + GRADS
                                       + ACC_TAIL + _a("antialiasing:i dL_dmeans2D_abs")),
    # GSRAST_HAS_CONTRIB: per-Gaussian contribution statistics (wsum, wmax, count) of a rendered view
    "gs_contrib_scratch_bytes": (_sz, _a("num_rendered:ll")),
    "gs_contrib_stats": (_i, _a("P:i image_width:i image_height:i") + CAMERA + VIEW_BUFS
                         + _a("pixel_weights scratch wsum wmax count accumulate:i") + TAIL),
    # GSRAST_HAS_FEATURES: per-Gaussian feature channels through a rendered view's lists, and their gradient
    "gs_feature_group_channels": (_i, []),
    "gs_feature_scratch_bytes": (_sz, _a("num_rendered:ll")),
    "gs_feature_forward": (_i, FEATURE + _a("features out") + TAIL),
    "gs_feature_backward": (_i, FEATURE + _a("dL_dout scratch dL_dfeatures accumulate:i") + TAIL),
    # GSRAST_HAS_SKY: the skysphere background and its gradients
    "gs_sky_scratch_bytes": (_sz, _a("Hs:i Ws:i")),
    "gs_sky_compose_forward": (_i, SKY + _a("color alpha out_image stream")),
    "gs_sky_compose_backward": (_i, SKY_BWD + _a("stream")),
    # GSRAST_HAS_SKY_CAMERA: the sky's dL/dviewmatrix on the same pass
    "gs_sky_camera_scratch_bytes": (_sz, _a("W:i H:i")),
    "gs_sky_compose_backward_camera": (_i, SKY_BWD + _a("dL_dviewmatrix accumulate_view:i camera_scratch stream")),
    "gs_mark_visible": (_i, _a("P:i means3D viewmatrix projmatrix present stream")),
    "gs_knn_scratch_bytes": (_sz, _a("P:i")),
    "gs_knn_mean_dist2": (_i, _a("P:i points out scratch stream")),
    "gs_set_exact_exp": (_i, _a("exact:i")),
    "gs_debug_launch_log": (_i, _a("enable:i")),
    "gs_debug_launched_kernels": (_ll, _a("buf:s cap:ll")),
    "gs_ssim_partial_count": (_sz, _a("planes:i H:i W:i")),
    "gs_ssim_forward": (_i, LOSS + _a("img1 img2 dmaps partial plane_sum stream")),
    "gs_ssim_backward": (_i, _a("planes:i channels:i H:i W:i window11_host img1 img2 dmaps scale dimg1 stream")),
    "gs_photometric_loss_forward": (_i, LOSS + _a("img gt lambda_dssim:f dmaps partial out3 stream")),
    "gs_photometric_loss_backward": (_i, LOSS + _a("img gt dmaps lambda_dssim:f grad dimg stream")),
    "gs_adam_step": (_i, _a("count:i params_host grads_host exp_avg_host exp_avg_sq_host numel_host") + ADAM_HYPER
                     + _a("stream")),
    "gs_adam_step_activated": (_i, _a("count:i params_host grad_src_host grad_mode_host sh_coeffs:i exp_avg_host "
                                      "exp_avg_sq_host numel_host") + ADAM_HYPER + _a("stream")),
    "gs_activate_forward": (_i, _a("P:i sh_rest:i features_dc features_rest opacity_raw scaling_raw rotation_raw shs "
                                   "opacity scales rotations stream")),
    "gs_activate_backward": (_i, _a("P:i sh_rest:i dL_dshs dL_dopacity dL_dscales dL_drotations opacity scales "
                                    "rotation_raw dL_dfeatures_dc dL_dfeatures_rest dL_dopacity_raw dL_dscaling_raw "
                                    "dL_drotation_raw stream")),
    "gs_densify_block_count": (_sz, _a("P:i")),
    "gs_densify_classify": (_i, _a("P:i grad_accum denom opacity_raw scaling_raw grad_threshold:d pd_extent:d "
                                   "min_opacity:d big_extent:d has_screen:i max_screen:d N:i flags block_counts "
                                   "totals stream")),
    "gs_densify_split_stds": (_i, _a("P:i N:i totals_host flags block_counts scaling_raw stds stream")),
    "gs_densify_emit": (_i, _a("P:i N:i totals_host flags block_counts samples params_host exp_avg_host "
                               "exp_avg_sq_host out_params_host out_exp_avg_host out_exp_avg_sq_host widths_host "
                               "stream")),
    "gs_densify_stats": (_i, _a("P:i") + STATS + _a("stream")),
    "gs_debug_export": (_i, _a("P:i image_width:i image_height:i num_rendered:ll geom_buffer binning_buffer "
                               "image_buffer point_list ranges xy conic_opacity rgb depth tiles_touched final_T "
                               "n_contrib stream")),
    "gs_debug_export_slots": (_i, _a("image_width:i image_height:i num_rendered:ll binning_buffer image_buffer slots "
                                     "tile_cut stream")),
    "gs_debug_set_scan_spin_limit": (_u, _a("limit:u")),
    "gs_debug_set_tile_sort_packed": (_i, _a("on:i")),
    "gs_debug_tile_sort_packed_count": (_ll, []),
    "gs_debug_sh_rows_staged": (_i, _a("D:i M:i shs")),
    "gs_profile_enable": (None, _a("on:i")),
    "gs_profile_collect": (_i, []),
    "gs_profile_reset": (None, []),
    "gs_profile_stat": (_i, _a("i:i name:s name_len:i total_ms:pd launches:pll")),
}

# name -> (restype, argtypes), what load() declares
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in ENTRIES.items()}
_NAMES = {name: tuple(n for n, _ in params) for name, (_, params) in ENTRIES.items()}
# name -> (mapping of named values -> their sequence in declaration order), resolved once per entry: an
# itemgetter, which yields a tuple only from two names up.  With a per-call `[named[n] for n in names]` the ctypes
# path's eager forward + backward measured above the parent's host-time spread in one of four figures of a
# noisy A/B (profiles/entry_families_host_ab.txt); with this form every figure lies inside.
_PICK = {name: operator.itemgetter(*names) if len(names) > 1 else (lambda named, names=names: [named[n] for n in names])
         for name, names in _NAMES.items()}


def _in_order(entry, named):
    try:
        args = _PICK[entry](named)
    except KeyError as e:
        raise TypeError(f"{entry}: missing argument {e.args[0]!r}") from None
    if len(named) != len(args):
        raise TypeError(f"{entry}: unknown argument(s) {sorted(set(named) - set(_NAMES[entry]))}")
    return args


def ordered(entry, **named):
    """The arguments of a C entry in its declaration order, from their names in include/gsrast.h.
    Every parameter must be named (an absent pointer is an explicit None) and nothing else."""
    return list(_in_order(entry, named))


_lib = None


def load():
    """Load libgsrast.so once and declare every C-ABI symbol.  Raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libgsrast.so not found at {LIB_PATH}; build it with "
            f"`make -C {_PKG_ROOT}` (hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().gs_last_error()
    return msg.decode() if msg else "unknown error"


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {last_error()}")


def call(entry, what, **named):
    """entry(**named) through ordered(); a non-zero status raises RuntimeError(`what`: the library's message)."""
    check(getattr(_lib or load(), entry)(*_in_order(entry, named)), what)


def profile_stats():
    """Per-kernel (name -> (total_ms, launches)) collected with gs_profile_enable(1)."""
    lib = load()
    lib.gs_profile_collect()
    out = {}
    i = 0
    buf = ctypes.create_string_buffer(128)
    ms = ctypes.c_double()
    n = ctypes.c_longlong()
    while lib.gs_profile_stat(i, buf, 128, ctypes.byref(ms), ctypes.byref(n)):
        out[buf.value.decode()] = (ms.value, n.value)
        i += 1
    return out
