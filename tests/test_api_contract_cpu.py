"""The host contract of the forward / backward C entries (include/gsrast.h), without a GPU.

Every validation failure and every empty-scene return of these entries happens before the first
HIP call, so the order of the checks, the error texts and what is left in `*num_rendered_host`
can be pinned on any machine.  Each row of the tables below is one call through `_native.load()`
with one or two faults in its arguments; rows with two faults pin which check comes first.  The
expected values were recorded from the library before its host layer was rebuilt from shared
steps (the rows passed there unmodified); they are the contract, not a description of the code.

Every pointer argument is NULL or the address of a small host array that the library only tests
for NULL: no row may reach a device call (each row has a fault, or an empty scene, in front of it).
"""
import ctypes

import pytest

from diff_gaussian_rasterization import _native

_BUF = (ctypes.c_float * 64)()  # 16-byte aligned host words; never dereferenced by a row
X = ctypes.cast(_BUF, ctypes.c_void_p)
ODD = ctypes.c_void_p(X.value + 4)  # not 16-byte aligned
OTHER = ctypes.c_void_p(X.value + 64)
BIG = 1 << 31  # GS_MAX_INSTANCES + 1
SENTINEL = 7  # what *num_rendered_host holds before a call


def ptrs(*v):
    return (ctypes.c_void_p * len(v))(*[x.value if isinstance(x, ctypes.c_void_p) else x for x in v])


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def lls(*v):
    return (ctypes.c_longlong * len(v))(*v)


def view(**over):
    f = dict(viewmatrix=X.value, projmatrix=X.value, campos=X.value, tan_fovx=0.5, tan_fovy=0.5, image_width=16,
             image_height=16, geom_buffer=X.value)
    f.update(over)
    return _native.ViewGrad(**f)


def views(*v):
    return (_native.ViewGrad * len(v))(*v)


@ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t)
def _alloc(ctx, kind, nbytes):
    return X.value


# arguments that are not a plain non-NULL pointer by default (every other name defaults to X)
DEFAULTS = dict(P=4, D=3, M=16, W=16, H=16, K=2, first=0, count=4, scale_modifier=1.0, tan_fovx=0.5, tan_fovy=0.5,
                prefiltered=0, debug=0, stream=None, bounded=0, capacity=100, num_rendered=10, accumulate=0,
                wait_event=None, colors=None, cov3D=None, view_streams=None, num_views=1, beta1=0.9, beta2=0.999,
                eps=1e-15, maximize=0, grad_stride=2, alloc_ctx=None, weight_decay=None, geom_out=None,
                binning_out=None, image_out=None,
                # the densify-statistics pointers of the fused Adam entry: all NULL = no statistics
                st_radii=None, grad2d=None, max_radii2D=None, grad_accum=None, denom=None)


def _default(name):
    if name in DEFAULTS:
        return DEFAULTS[name]
    return {
        "bgs": lambda: ptrs(X, X), "views_": lambda: ptrs(X, X), "projs": lambda: ptrs(X, X),
        "camposs": lambda: ptrs(X, X), "radiis": lambda: ptrs(X, X), "geoms": lambda: ptrs(X, X),
        "binnings": lambda: ptrs(X, X), "images": lambda: ptrs(X, X),
        "Ws": lambda: ints(16, 16), "Hs": lambda: ints(16, 16),
        "tfxs": lambda: (ctypes.c_float * 2)(0.5, 0.5), "tfys": lambda: (ctypes.c_float * 2)(0.5, 0.5),
        "nrs": lambda: lls(SENTINEL, SENTINEL), "caps": lambda: lls(100, 100), "nr_list": lambda: lls(10, 10),
        "view_list": lambda: views(view()), "view1": lambda: ctypes.pointer(view()),
        "params": lambda: ptrs(X, X, X, X, X, X), "exp_avg": lambda: ptrs(X, X, X, X, X, X),
        "exp_avg_sq": lambda: ptrs(X, X, X, X, X, X), "lr": lambda: (ctypes.c_double * 6)(*[1e-3] * 6),
        "steps": lambda: lls(1, 1, 1, 1, 1, 1), "alloc": lambda: ctypes.cast(_alloc, ctypes.c_void_p),
    }.get(name, lambda: X)()


SCENE = "means3D shs colors opac scales scale_modifier rots cov3D"
SCENE_SPLIT2 = "means3D shs shs_rest opac scales scale_modifier rots cov3D"  # dc / rest in place of shs / colors
SCENE_SPLIT3 = "means3D shs shs_rest colors opac scales scale_modifier rots cov3D"
CAM = "view proj campos tan_fovx tan_fovy"
GRADS = "dmeans2D dcolors dopacity dmeans3D dcov3D dsh dscales drots"
GRADS_SPLIT = "dmeans2D dopacity dmeans3D dcov3D dsh dscales drots"
BWD_BUFS = "radii geom num_rendered binning image dL_dout_color"
VIEWS_FRONT = (f"K P D M bgs Ws Hs {SCENE} views_ projs camposs tfxs tfys prefiltered radiis geoms")
ADAM = ("P D M means3D shs shs_rest scales scale_modifier rots view1 params exp_avg exp_avg_sq lr steps weight_decay "
        "beta1 beta2 eps maximize")
PARAMS = {
    "gs_forward_preprocess": f"P D M bg W H {SCENE} {CAM} prefiltered radii geom nr debug stream",
    "gs_forward_preprocess_split": f"P D M bg W H {SCENE_SPLIT2} {CAM} prefiltered radii geom nr debug stream",
    "gs_forward_bounded": (f"P D M bg W H {SCENE_SPLIT3} {CAM} prefiltered radii geom capacity binning image "
                           "out_color debug stream"),
    "gs_forward_counted": (f"P D M bg W H {SCENE_SPLIT3} {CAM} prefiltered radii geom capacity binning image "
                           "out_color nr debug stream"),
    "gs_forward_render": f"P bg W H {CAM} radii geom num_rendered binning image out_color debug stream",
    "gs_forward_render_bounded": f"P bg W H {CAM} radii geom num_rendered binning image out_color debug stream",
    "gs_forward_render_aux": (f"P bg W H {CAM} radii geom num_rendered binning image out_color out_invdepth "
                              "out_alpha debug stream"),
    "gs_forward_render_binned": f"P bg W H {CAM} geom num_rendered binning image out_color bounded debug stream",
    "gs_forward_bin_views": "K P W H geoms nr_list binnings images debug stream view_streams",
    "gs_forward_preprocess_views": f"{VIEWS_FRONT} nrs debug stream view_streams",
    "gs_forward_preprocess_views_bounded": f"{VIEWS_FRONT} caps debug stream view_streams",
    "gs_rasterize_forward": (f"P D M bg W H {SCENE} {CAM} prefiltered out_color radii alloc alloc_ctx geom_out "
                             "binning_out image_out debug stream"),
    "gs_backward": f"P D M bg W H {SCENE} {CAM} {BWD_BUFS} grad_buffer {GRADS} debug stream",
    "gs_backward_accumulate": (f"P D M bg W H {SCENE} {CAM} {BWD_BUFS} grad_buffer {GRADS} accumulate wait_event "
                               "debug stream"),
    "gs_backward_accumulate_aux": (f"P D M bg W H {SCENE_SPLIT3} {CAM} {BWD_BUFS} dL_dout_invdepth dL_dout_alpha "
                                   f"grad_buffer {GRADS} accumulate wait_event debug stream"),
    "gs_backward_accumulate_split": (f"P D M bg W H {SCENE_SPLIT2} {CAM} {BWD_BUFS} grad_buffer {GRADS_SPLIT} "
                                     "accumulate wait_event debug stream"),
    "gs_backward_render": (f"P D M bg W H {CAM} geom num_rendered binning image dL_dout_color grad_buffer dmeans2D "
                           "accumulate debug stream"),
    "gs_backward_gaussians": ("P D M means3D shs colors scales scale_modifier rots cov3D num_views view_list dcolors "
                              "dopacity dmeans3D dcov3D dsh dscales drots accumulate wait_event debug stream"),
    "gs_backward_gaussians_range": ("P first count D M means3D shs colors scales scale_modifier rots cov3D num_views "
                                    "view_list dcolors dopacity dmeans3D dcov3D dsh dscales drots accumulate "
                                    "wait_event debug stream"),
    "gs_backward_gaussians_adam": f"{ADAM} debug stream",
    "gs_backward_gaussians_adam_stats": (f"{ADAM} st_radii grad2d grad_stride max_radii2D grad_accum denom debug "
                                         "stream"),
}
# entries without a split / colour source of their own default to SH colours; the three-source
# entries (shs, shs_rest, colors) default to plain SHs
NO_REST = {"gs_forward_bounded", "gs_forward_counted", "gs_backward_accumulate_aux"}

# message texts
E_P = "P must be >= 0"
E_SIZE = "image size must be positive (got %d x %d)"
E_SIZE_SHORT = "image size must be positive"
E_IN = "missing required input pointer"
E_COL = "Please provide excatly one of either SHs or precomputed colors!"
E_COV = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
E_DEG = "SH degree must be in [0, 3] (got %d)"
E_CAMPOS = "campos is required with SHs"
E_OUT = "missing output pointer"
E_BUF = "missing buffer pointer"
E_GRAD = "missing gradient output pointer"
E_DSH = "dL_dsh is required with SHs"
E_NR = "num_rendered out of range"
E_CAP = "capacity out of range"
E_REST = "split SH: features_rest is NULL"
E_SPLIT = "split SH: features_dc and features_rest replace shs (no colours)"
E_SPLIT_M = "split SH: M must be >= 2 (got 1)"
E_ACC = "accumulate: unknown GS_ACC bits 0x100"
E_VIEWS = "views: 1 to 8 per call"
E_VARR = "missing per-view argument array"
E_STRIDE = ("bin_views: each kind of buffer must be K slices of one allocation, one stride apart, each sized for the "
            "largest num_rendered")

COLOURS = dict(shs=None, colors=X, campos=None, D=9, M=0)  # precomputed colours: D, M and campos are not looked at


def front_rows(e, nr, buf_msg):
    """The validation shared by the single-view forward fronts (nr: what the entry leaves in
    *num_rendered_host, or None for an entry without one)."""
    return [
        (e, dict(P=-1, W=0), 1, E_P, nr),
        (e, dict(W=0, means3D=None), 1, E_SIZE % (0, 16), nr),
        (e, dict(H=-2, radii=None), 1, E_SIZE % (16, -2), nr),
        (e, dict(P=0, W=0), 1, E_SIZE % (0, 16), nr),
        (e, dict(P=0, means3D=None, radii=None), 0, "", nr),
        (e, dict(means3D=None, D=7), 1, E_IN, nr),
        (e, dict(opac=None), 1, E_IN, nr),
        (e, dict(view=None), 1, E_IN, nr),
        (e, dict(proj=None), 1, E_IN, nr),
        (e, dict(bg=None, cov3D=X), 1, E_IN, nr),
        (e, dict(cov3D=X, D=4), 1, E_COV, nr),
        (e, dict(scales=None), 1, E_COV, nr),
        (e, dict(rots=None, radii=None), 1, E_COV, nr),
        (e, dict(D=4, M=9), 1, E_DEG % 4, nr),
        (e, dict(D=-1), 1, E_DEG % -1, nr),
        (e, dict(M=9, campos=None), 1, "shs has 9 coefficients, degree 3 needs 16", nr),
        (e, dict(campos=None, radii=None), 1, E_CAMPOS, nr),
        (e, dict(radii=None), 1, buf_msg, nr),
        (e, dict(geom=None), 1, buf_msg, nr),
    ]


def colour_rows(e, nr, buf_msg):
    """Entries that take precomputed colours."""
    return [
        (e, dict(colors=X, D=7), 1, E_COL, nr),
        (e, dict(shs=None), 1, E_COL, nr),
        (e, dict(COLOURS, geom=None), 1, buf_msg, nr),
    ]


def split3_rows(e, nr):
    """Entries with shs, shs_rest and colours side by side."""
    return [
        (e, dict(COLOURS, shs_rest=X, geom=None), 1, E_SPLIT, nr),
        (e, dict(shs_rest=X, colors=X), 1, E_COL, nr),
        (e, dict(shs_rest=X, D=0, M=1, geom=None), 1, E_SPLIT_M, nr),
        (e, dict(shs_rest=X, P=0, D=0, M=1), 1, E_SPLIT_M, nr),
    ]


def split2_rows(e, nr):
    """Entries whose colour inputs are features_dc / features_rest."""
    return [
        (e, dict(shs_rest=None, W=0), 1, E_REST, nr),
        (e, dict(shs_rest=None, P=-1), 1, E_REST, nr),
        (e, dict(shs=None), 1, E_COL, nr),
        (e, dict(D=0, M=1, geom=None), 1, E_SPLIT_M, nr),
        (e, dict(D=0, M=1, W=0), 1, E_SIZE % (0, 16), nr),
    ]


def capacity_rows(e, nr):
    return [
        (e, dict(P=0, capacity=-1), 0, "", nr),
        (e, dict(capacity=-1, geom=None), 1, E_CAP, nr),
        (e, dict(capacity=BIG, out_color=None), 1, E_CAP, nr),
        (e, dict(capacity=-1, W=0), 1, E_SIZE % (0, 16), nr),
        (e, dict(binning=None), 1, E_BUF, nr),
        (e, dict(image=None), 1, E_BUF, nr),
        (e, dict(out_color=None), 1, E_BUF, nr),
    ]


def render_rows(e, radii=True):
    rows = [
        (e, dict(P=0, W=0, geom=None), 0, "", None),
        (e, dict(P=-3, num_rendered=-1), 0, "", None),
        (e, dict(W=0, geom=None), 1, E_SIZE_SHORT, None),
        (e, dict(H=0, num_rendered=-1), 1, E_SIZE_SHORT, None),
        (e, dict(num_rendered=-1, geom=None), 1, E_NR, None),
        (e, dict(num_rendered=BIG), 1, E_NR, None),
        (e, dict(geom=None), 1, E_BUF, None),
        (e, dict(binning=None), 1, E_BUF, None),
        (e, dict(image=None), 1, E_BUF, None),
        (e, dict(out_color=None, bg=None), 1, E_BUF, None),
    ]
    if radii:
        rows.append((e, dict(radii=None), 1, E_BUF, None))
    return rows


def backward_rows(e, accumulate=True):
    rows = [
        (e, dict(P=-1, W=0), 1, E_P, None),
        (e, dict(W=0, geom=None), 1, E_SIZE % (0, 16), None),
        (e, dict(P=0, W=0), 1, E_SIZE % (0, 16), None),
        (e, dict(P=0, geom=None, means3D=None), 0, "", None),
        (e, dict(opac=None, geom=None), 1, E_BUF, None),  # the backward does not need the opacities
        (e, dict(means3D=None, geom=None), 1, E_IN, None),
        (e, dict(bg=None), 1, E_IN, None),
        (e, dict(cov3D=X, geom=None), 1, E_COV, None),
        (e, dict(D=4, geom=None), 1, E_DEG % 4, None),
        (e, dict(campos=None, geom=None), 1, E_CAMPOS, None),
        (e, dict(geom=None, dmeans2D=None), 1, E_BUF, None),
        (e, dict(binning=None), 1, E_BUF, None),
        (e, dict(image=None), 1, E_BUF, None),
        (e, dict(dL_dout_color=None), 1, E_BUF, None),
        (e, dict(grad_buffer=None, num_rendered=-1), 1, E_BUF, None),
        (e, dict(dmeans2D=None, num_rendered=-1), 1, E_GRAD, None),
        (e, dict(dopacity=None), 1, E_GRAD, None),
        (e, dict(dmeans3D=None), 1, E_GRAD, None),
        (e, dict(num_rendered=-1, radii=None), 1, E_NR, None),
        (e, dict(num_rendered=BIG), 1, E_NR, None),
    ]
    if accumulate:
        rows += [
            (e, dict(accumulate=0x100, num_rendered=-1), 1, E_NR, None),
            (e, dict(accumulate=0x100), 1, E_ACC, None),
            (e, dict(accumulate=0x100, dmeans3D=None), 1, E_GRAD, None),
            (e, dict(accumulate=0x100, P=0), 0, "", None),
        ]
    return rows


def gaussians_rows(e):
    empty = dict(count=0) if e.endswith("_range") else {}  # (the range entry checks its range before P == 0)
    return [
        (e, dict(P=-1, num_views=-1), 1, E_P, None),
        (e, dict(num_views=-1, means3D=None), 1, "bad view list", None),
        (e, dict(view_list=None), 1, "bad view list", None),
        (e, dict(empty, P=0, means3D=None), 0, "", None),
        (e, dict(num_views=0, view_list=None, means3D=None), 0, "", None),
        (e, dict(means3D=None, colors=X), 1, E_IN, None),
        (e, dict(colors=X, D=9), 1, E_COL, None),
        (e, dict(shs=None, cov3D=X), 1, E_COL, None),
        (e, dict(cov3D=X, D=9), 1, E_COV, None),
        (e, dict(rots=None, dopacity=None), 1, E_COV, None),
        (e, dict(D=4, dopacity=None), 1, "bad SH degree / coefficient count", None),
        (e, dict(M=9), 1, "bad SH degree / coefficient count", None),
        (e, dict(dopacity=None, accumulate=0x100), 1, E_GRAD, None),
        (e, dict(dmeans3D=None), 1, E_GRAD, None),
        (e, dict(accumulate=0x100, view_list=views(view(viewmatrix=None))), 1, E_ACC, None),
        (e, dict(view_list=views(view(viewmatrix=None, image_width=0))), 1, "view 0: missing pointer", None),
        (e, dict(view_list=views(view(projmatrix=None))), 1, "view 0: missing pointer", None),
        (e, dict(view_list=views(view(geom_buffer=None))), 1, "view 0: missing pointer", None),
        (e, dict(view_list=views(view(campos=None))), 1, "view 0: missing pointer", None),
        (e, dict(view_list=views(view(image_width=0))), 1, "view 0: bad image size", None),
        (e, dict(num_views=2, view_list=views(view(), view(image_height=0))), 1, "view 1: bad image size", None),
        (e, dict(num_views=2, view_list=views(view(image_height=0), view(campos=None))), 1, "view 0: bad image size",
         None),
        # precomputed colours: campos is not needed, so the second view's image size is the fault
        (e, dict(shs=None, colors=X, D=9, M=0, num_views=2,
                 view_list=views(view(campos=None), view(campos=None, image_width=-1))), 1,
         "view 1: bad image size", None),
    ]


E_ADAM_ALIGN = "fused Adam backward: %s parameter, exp_avg and exp_avg_sq must be 16-byte aligned"


def six(k, v):
    """Six valid-looking group pointers (xyz, f_dc, f_rest, opacity, scaling, rotation) with group k's set to v."""
    a = [X] * 6
    a[k] = v
    return ptrs(*a)


def adam_rows(e):
    return [
        (e, dict(P=-1, M=15), 1, E_P, None),
        (e, dict(P=0, M=15, means3D=None), 0, "", None),
        (e, dict(M=15, means3D=None), 1, "fused Adam backward: 16 SH coefficients, degree 0..3 only", None),
        (e, dict(D=4), 1, "fused Adam backward: 16 SH coefficients, degree 0..3 only", None),
        (e, dict(shs_rest=None), 1, E_IN, None),
        (e, dict(view1=None, params=six(3, None)), 1, E_IN, None),
        (e, dict(steps=None), 1, E_IN, None),
        (e, dict(view1=ctypes.pointer(view(projmatrix=None, image_width=0))), 1, "view: missing pointer", None),
        (e, dict(view1=ctypes.pointer(view(campos=None))), 1, "view: missing pointer", None),
        (e, dict(view1=ctypes.pointer(view(image_width=0)), params=six(3, None)), 1, "view: bad image size", None),
        (e, dict(params=six(3, None)), 1, "missing tensor pointer", None),
        (e, dict(exp_avg_sq=six(5, None), means3D=OTHER), 1, "missing tensor pointer", None),
        (e, dict(steps=lls(1, 1, 0, 1, 1, 1)), 1, "adam: step must be >= 1", None),
        (e, dict(steps=lls(0, 1, 1, 1, 1, 1), params=six(3, None)), 1, "adam: step must be >= 1", None),
        (e, dict(steps=lls(1, 1, 1, 1, 0, 1), params=six(3, None)), 1, "missing tensor pointer", None),
        (e, dict(means3D=OTHER, params=six(5, ODD)), 1, "means3D must be the xyz parameter (params_host[0])", None),
        (e, dict(params=six(5, ODD), shs=ODD), 1, "rotation parameter must be 16-byte aligned", None),
        (e, dict(shs=ODD), 1, "split SH rows must be 16-byte aligned", None),
        (e, dict(shs_rest=ODD), 1, "split SH rows must be 16-byte aligned", None),
    ]


def build_rows():
    rows = []
    # ---- single-view forward fronts ----
    e = "gs_forward_preprocess"
    rows += front_rows(e, 0, E_OUT) + colour_rows(e, 0, E_OUT)
    rows += [(e, dict(nr=None), 1, E_OUT, None), (e, dict(nr=None, W=0), 1, E_SIZE % (0, 16), None)]
    e = "gs_forward_preprocess_split"
    rows += front_rows(e, 0, E_OUT) + split2_rows(e, 0)
    rows += [(e, dict(nr=None), 1, E_OUT, None), (e, dict(nr=None, shs_rest=None), 1, E_REST, None)]
    e = "gs_forward_bounded"
    rows += front_rows(e, None, E_BUF) + colour_rows(e, None, E_BUF) + split3_rows(e, None) + capacity_rows(e, None)
    e = "gs_forward_counted"
    rows += front_rows(e, 0, E_BUF) + colour_rows(e, 0, E_BUF) + split3_rows(e, 0) + capacity_rows(e, 0)
    rows += [(e, dict(nr=None), 1, E_BUF, None), (e, dict(nr=None, capacity=-1), 1, E_CAP, None),
             (e, dict(nr=None, P=0), 0, "", None)]
    # ---- render tails ----
    rows += render_rows("gs_forward_render") + render_rows("gs_forward_render_bounded")
    e = "gs_forward_render_aux"
    rows += render_rows(e) + [(e, dict(out_invdepth=None, out_alpha=None, radii=None), 1, E_BUF, None)]
    e = "gs_forward_render_binned"
    rows += render_rows(e, radii=False) + [(e, dict(bounded=1, binning=None), 1, E_BUF, None),
                                           (e, dict(bounded=1, P=0), 0, "", None)]
    # ---- multi-view fronts ----
    e = "gs_forward_bin_views"
    rows += [
        (e, dict(K=0, P=-1), 1, E_VIEWS, None),
        (e, dict(K=9, geoms=None), 1, E_VIEWS, None),
        (e, dict(P=-1, W=0), 1, E_P, None),
        (e, dict(W=0, geoms=None), 1, E_SIZE_SHORT, None),
        (e, dict(H=0, P=0), 1, E_SIZE_SHORT, None),
        (e, dict(geoms=None, P=0), 1, "missing per-view array", None),
        (e, dict(nr_list=None), 1, "missing per-view array", None),
        (e, dict(binnings=None), 1, "missing per-view array", None),
        (e, dict(images=None), 1, "missing per-view array", None),
        (e, dict(P=0, geoms=ptrs(None, None), nr_list=lls(-1, -1)), 0, "", None),
        (e, dict(geoms=ptrs(X, None)), 1, "view 1: missing buffer", None),
        (e, dict(images=ptrs(None, X), nr_list=lls(-1, 5)), 1, "view 0: missing buffer", None),
        (e, dict(nr_list=lls(5, -1)), 1, E_NR, None),
        (e, dict(nr_list=lls(BIG, 5), binnings=ptrs(X, None)), 1, E_NR, None),
        (e, dict(nr_list=lls(5, BIG), binnings=ptrs(None, X)), 1, "view 0: missing buffer", None),
        (e, dict(), 1, E_STRIDE, None),  # K = 2 views at the same address: not one stride apart
        (e, dict(geoms=ptrs(X, OTHER)), 1, E_STRIDE, None),  # 64 bytes apart: less than a geometry buffer
    ]
    e = "gs_forward_preprocess_views"
    S = SENTINEL
    rows += [
        (e, dict(nrs=None, K=0), 1, E_VARR, None),
        (e, dict(K=0, bgs=None), 1, E_VIEWS, [S, S]),
        (e, dict(K=9), 1, E_VIEWS, [S, S]),
        (e, dict(bgs=None, P=-1), 1, E_VARR, [S, S]),
        (e, dict(view_streams=None, radiis=None), 1, E_VARR, [S, S]),
        (e, dict(tfys=None), 1, E_VARR, [S, S]),
        (e, dict(P=-1), 1, E_P, [0, S]),
        (e, dict(Ws=ints(16, 0)), 1, E_SIZE % (0, 16), [0, 0]),
        (e, dict(Ws=ints(0, 16), P=0), 1, E_SIZE % (0, 16), [0, S]),
        (e, dict(means3D=None), 1, E_IN, [0, S]),
        (e, dict(views_=ptrs(X, None)), 1, E_IN, [0, 0]),
        (e, dict(colors=X), 1, E_COL, [0, S]),
        (e, dict(camposs=ptrs(X, None), radiis=ptrs(X, None)), 1, E_CAMPOS, [0, 0]),
        (e, dict(radiis=ptrs(X, None)), 1, E_OUT, [0, 0]),
        (e, dict(geoms=ptrs(None, X), Ws=ints(16, 0)), 1, E_OUT, [0, S]),
        (e, dict(P=0, radiis=ptrs(None, None), means3D=None), 0, "", [0, 0]),
        (e, dict(K=1, P=0), 0, "", [0, S]),
    ]
    e = "gs_forward_preprocess_views_bounded"
    rows += [
        (e, dict(caps=None, K=9), 1, "missing capacity array", None),
        (e, dict(K=0, bgs=None), 1, E_VIEWS, None),
        (e, dict(projs=None, caps=lls(-1, -1)), 1, E_VARR, None),
        (e, dict(caps=lls(100, -1), means3D=None), 1, E_IN, None),
        (e, dict(caps=lls(-1, 100), means3D=None), 1, E_CAP, None),
        (e, dict(caps=lls(100, BIG), P=0), 1, E_CAP, None),
        (e, dict(caps=lls(100, -1), radiis=ptrs(None, X)), 1, E_OUT, None),
        (e, dict(Hs=ints(16, -1)), 1, E_SIZE % (16, -1), None),
        (e, dict(geoms=ptrs(X, None)), 1, E_OUT, None),
        (e, dict(P=0, geoms=ptrs(None, None)), 0, "", None),
    ]
    # ---- the two-call forward behind an allocator callback ----
    e = "gs_rasterize_forward"
    rows += [
        (e, dict(alloc=None, W=0), -1, "alloc callback is NULL", None),
        (e, dict(W=0), -1, E_SIZE % (0, 16), None),
        (e, dict(means3D=None), -1, E_IN, None),
        (e, dict(radii=None), -1, E_OUT, None),
        (e, dict(P=0), 0, "", None),
    ]
    # ---- backwards ----
    e = "gs_backward"
    rows += backward_rows(e, accumulate=False) + colour_rows(e, None, E_BUF)
    e = "gs_backward_accumulate"
    rows += backward_rows(e) + colour_rows(e, None, E_BUF)
    e = "gs_backward_accumulate_aux"
    rows += backward_rows(e) + colour_rows(e, None, E_BUF) + split3_rows(e, None)
    rows += [(e, dict(dL_dout_invdepth=None, dL_dout_alpha=None, geom=None), 1, E_BUF, None)]
    e = "gs_backward_accumulate_split"
    rows += backward_rows(e) + split2_rows(e, None)
    e = "gs_backward_render"
    rows += [
        (e, dict(P=-1, W=0), 1, E_P, None),
        (e, dict(W=0, view=None), 1, E_SIZE % (0, 16), None),
        (e, dict(P=0, H=0), 1, E_SIZE % (16, 0), None),
        (e, dict(P=0, view=None, geom=None), 0, "", None),
        (e, dict(view=None, geom=None), 1, E_IN, None),
        (e, dict(proj=None), 1, E_IN, None),
        (e, dict(bg=None, num_rendered=-1), 1, E_IN, None),
        (e, dict(campos=None, dmeans2D=None, geom=None), 1, E_BUF, None),  # neither is looked at
        (e, dict(binning=None), 1, E_BUF, None),
        (e, dict(image=None), 1, E_BUF, None),
        (e, dict(dL_dout_color=None), 1, E_BUF, None),
        (e, dict(grad_buffer=None, num_rendered=-1), 1, E_BUF, None),
        (e, dict(num_rendered=-1, accumulate=2), 1, E_NR, None),
        (e, dict(num_rendered=BIG), 1, E_NR, None),
        (e, dict(accumulate=2), 1, "accumulate: only GS_ACC_MEANS2D applies here", None),
        (e, dict(accumulate=3, D=9, M=0), 1, "accumulate: only GS_ACC_MEANS2D applies here", None),
    ]
    rows += gaussians_rows("gs_backward_gaussians")
    e = "gs_backward_gaussians_range"
    rows += gaussians_rows(e) + [
        (e, dict(P=-1, first=-1), 1, E_P, None),
        (e, dict(first=-1, num_views=-1), 1, "Gaussian range out of bounds", None),
        (e, dict(count=-1), 1, "Gaussian range out of bounds", None),
        (e, dict(first=3, count=2, means3D=None), 1, "Gaussian range out of bounds", None),
        (e, dict(first=0x7FFFFFFF, count=0x7FFFFFFF), 1, "Gaussian range out of bounds", None),
        (e, dict(first=4, count=0, means3D=None), 0, "", None),
        (e, dict(first=2, count=2, means3D=None), 1, E_IN, None),
    ]
    rows += adam_rows("gs_backward_gaussians_adam")
    e = "gs_backward_gaussians_adam_stats"
    rows += adam_rows(e) + [
        (e, dict(st_radii=X), 1, "densify stats: all five pointers or none", None),
        (e, dict(st_radii=X, grad2d=X, max_radii2D=X, grad_accum=X, grad_stride=1), 1,
         "densify stats: all five pointers or none", None),
        (e, dict(st_radii=X, grad2d=X, max_radii2D=X, grad_accum=X, denom=X, grad_stride=1), 1,
         "densify stats: grad_stride must be >= 2", None),
        (e, dict(denom=X, shs=ODD), 1, "split SH rows must be 16-byte aligned", None),
    ]
    # ---- SH colours need their dL_dsh output (the view-direction term of dL_dmeans3D is formed with it):
    # ---- checked behind the required gradient pointers, in front of num_rendered / the accumulate bits / the
    # ---- views; precomputed colours do without.  (Appended here: the ids of the rows above carry their index.)
    for e in ("gs_backward", "gs_backward_accumulate", "gs_backward_accumulate_aux", "gs_backward_accumulate_split"):
        rows += [
            (e, dict(dsh=None), 1, E_DSH, None),
            (e, dict(dsh=None, num_rendered=-1), 1, E_DSH, None),
            (e, dict(dsh=None, dmeans3D=None), 1, E_GRAD, None),
            (e, dict(dsh=None, image=None), 1, E_BUF, None),
            (e, dict(dsh=None, P=0), 0, "", None),
        ]
        if e != "gs_backward_accumulate_split":
            rows += [(e, dict(COLOURS, dsh=None, dcolors=None, dcov3D=None, num_rendered=-1), 1, E_NR, None)]
        if e != "gs_backward":
            rows += [(e, dict(dsh=None, accumulate=0x100), 1, E_DSH, None)]
    for e in ("gs_backward_gaussians", "gs_backward_gaussians_range"):
        rows += [
            (e, dict(dsh=None), 1, E_DSH, None),
            (e, dict(dsh=None, accumulate=0x100), 1, E_DSH, None),
            (e, dict(dsh=None, view_list=views(view(image_width=0))), 1, E_DSH, None),
            (e, dict(dsh=None, dopacity=None), 1, E_GRAD, None),
            (e, dict(dsh=None, M=9), 1, "bad SH degree / coefficient count", None),
            (e, dict(dsh=None, num_views=0), 0, "", None),
            # precomputed colours: no dL_dsh, and neither dL_dcolors, dL_dcov3D, dL_dscales nor dL_drotations is required
            (e, dict(shs=None, colors=X, D=9, M=0, dsh=None, dcolors=None, dcov3D=None, dscales=None, drots=None,
                     view_list=views(view(image_width=0))), 1, "view 0: bad image size", None),
        ]
    # ---- the fused Adam kernel's 16-byte accesses: the parameter and both moments of features_dc, features_rest
    # ---- and rotation, checked behind the SH rows' alignment (gs_backward_gaussians_adam forwards to
    # ---- gs_backward_gaussians_adam_stats_aux, whose own rows are in tests/test_sky_train_cpu.py).  Appended here.
    e = "gs_backward_gaussians_adam"
    for k, name in ((1, "features_dc"), (2, "features_rest"), (5, "rotation")):
        for arg in ("params", "exp_avg", "exp_avg_sq"):
            if (k, arg) != (5, "params"):  # (its own, older message: adam_rows)
                rows.append((e, {arg: six(k, ODD)}, 1, E_ADAM_ALIGN % name, None))
    rows += [
        (e, dict(exp_avg=six(2, ODD), shs_rest=ODD), 1, "split SH rows must be 16-byte aligned", None),
        (e, dict(exp_avg_sq=six(1, ODD), means3D=OTHER), 1, "means3D must be the xyz parameter (params_host[0])", None),
        # (several: the first in group order is named)
        (e, dict(exp_avg=ptrs(X, ODD, ODD, X, X, ODD)), 1, E_ADAM_ALIGN % "features_dc", None),
        (e, dict(exp_avg=six(5, ODD), P=0), 0, "", None),
    ]
    return rows


# The image-size limits (include/gsrast.h): gx = ceil(W / 16) and gy = ceil(H / 16) at most
# GS_MAX_GRID_DIM = 65535 each, gx * gy at most GS_MAX_TILES = 2^22.  The last accepted and the first
# refused value of each.
W_LAST, W_FIRST = 65535 * 16, 65535 * 16 + 1          # gx = 65535 | 65536 (with H = 16: one tile row)
SQ_LAST, SQ_FIRST = 2048 * 16, 2048 * 16 + 1          # 2048 x 2048 = 2^22 tiles | 2049 x 2048
LIMIT_SIZES = [  # (W, H, accepted)
    (W_LAST, 16, True), (W_FIRST, 16, False), (16, W_LAST, True), (16, W_FIRST, False),
    (SQ_LAST, SQ_LAST, True), (SQ_FIRST, SQ_LAST, False), (SQ_LAST, SQ_FIRST, False),
    (64 * 16, 65535 * 16, True), (64 * 16 + 1, 65535 * 16, False),   # 64 x 65535 < 2^22 < 65 x 65535
    (0x7FFFFFFF, 16, False), (16, 0x7FFFFFFF, False), (0x7FFFFFFF, 0x7FFFFFFF, False),
]


def E_LIMIT(W, H, prefix=""):
    return (f"{prefix}image size {W} x {H} is too large: at most 65535 tiles of 16 pixels per row and per column "
            "and 4194304 tiles in all")


def size_limit_rows():
    """A table of its own (the ids of ROWS carry their index, and other tables are derived from
    ROWS).  The limit check follows the positive-size check directly: a row with an accepted size
    reaches the entry's next check, a refused one reports the limit in front of it."""
    rows = []
    fronts = [("gs_forward_preprocess", 0, 1), ("gs_forward_preprocess_split", 0, 1), ("gs_forward_bounded", None, 1),
              ("gs_forward_counted", 0, 1), ("gs_rasterize_forward", None, -1), ("gs_backward", None, 1),
              ("gs_backward_accumulate", None, 1), ("gs_backward_accumulate_aux", None, 1),
              ("gs_backward_accumulate_split", None, 1)]
    for e, nr, rc in fronts:  # validate(): P, positive size, the limits, pointers
        for W, H, ok in LIMIT_SIZES:
            rows.append((e, dict(W=W, H=H, means3D=None), rc, E_IN if ok else E_LIMIT(W, H), nr))
        rows += [
            (e, dict(P=-1, W=W_FIRST), rc, E_P, nr),
            (e, dict(W=W_FIRST, H=0), rc, E_SIZE % (W_FIRST, 0), nr),
            (e, dict(P=0, W=W_FIRST), rc, E_LIMIT(W_FIRST, 16), nr),      # also for an empty scene, as W = 0 is
            (e, dict(P=0, W=W_LAST, means3D=None), 0, "", nr),
        ]
    for e in ("gs_forward_render", "gs_forward_render_bounded", "gs_forward_render_aux", "gs_forward_render_binned"):
        for W, H, ok in LIMIT_SIZES:
            rows.append((e, dict(W=W, H=H, num_rendered=-1), 1, E_NR if ok else E_LIMIT(W, H), None))
        rows += [(e, dict(P=0, W=W_FIRST), 0, "", None), (e, dict(W=W_FIRST, H=0), 1, E_SIZE_SHORT, None)]
    e = "gs_forward_bin_views"
    for W, H, ok in LIMIT_SIZES:
        rows.append((e, dict(W=W, H=H, geoms=None), 1, "missing per-view array" if ok else E_LIMIT(W, H), None))
    rows += [(e, dict(P=-1, W=W_FIRST), 1, E_P, None), (e, dict(P=0, W=W_FIRST), 1, E_LIMIT(W_FIRST, 16), None)]
    S = SENTINEL
    e = "gs_forward_preprocess_views"
    rows += [
        (e, dict(Ws=ints(16, W_FIRST)), 1, E_LIMIT(W_FIRST, 16), [0, 0]),
        (e, dict(Ws=ints(W_FIRST, 0)), 1, E_LIMIT(W_FIRST, 16), [0, S]),          # view 0 is checked first
        (e, dict(Ws=ints(16, W_LAST), views_=ptrs(X, None)), 1, E_IN, [0, 0]),
        (e, dict(Ws=ints(SQ_LAST, 16), Hs=ints(SQ_LAST, 16), means3D=None), 1, E_IN, [0, S]),
        # view 0's pointers are checked before view 1's size
        (e, dict(Ws=ints(16, SQ_LAST), Hs=ints(16, SQ_FIRST), means3D=None), 1, E_IN, [0, S]),
        (e, dict(Ws=ints(16, SQ_LAST), Hs=ints(16, SQ_FIRST)), 1, E_LIMIT(SQ_LAST, SQ_FIRST), [0, 0]),
    ]
    e = "gs_forward_preprocess_views_bounded"
    rows += [
        (e, dict(Hs=ints(16, W_FIRST)), 1, E_LIMIT(16, W_FIRST), None),
        (e, dict(Hs=ints(16, W_LAST), geoms=ptrs(X, None)), 1, E_OUT, None),
    ]
    e = "gs_backward_render"
    for W, H, ok in LIMIT_SIZES:
        rows.append((e, dict(W=W, H=H, view=None), 1, E_IN if ok else E_LIMIT(W, H), None))
    rows += [(e, dict(P=-1, W=W_FIRST), 1, E_P, None), (e, dict(P=0, W=W_FIRST), 1, E_LIMIT(W_FIRST, 16), None)]
    for e in ("gs_backward_gaussians", "gs_backward_gaussians_range"):
        for W, H, ok in LIMIT_SIZES:
            # an accepted size leaves the next fault (the unknown accumulate bits are checked before the
            # views; so a NULL gradient pointer cannot follow them: use the second view's size)
            vl = views(view(image_width=W, image_height=H), view(image_width=0))
            rows.append((e, dict(num_views=2, view_list=vl), 1,
                         "view 1: bad image size" if ok else E_LIMIT(W, H, "view 0: "), None))
        rows += [
            (e, dict(num_views=2, view_list=views(view(), view(image_width=SQ_FIRST, image_height=SQ_LAST))), 1,
             E_LIMIT(SQ_FIRST, SQ_LAST, "view 1: "), None),
            (e, dict(view_list=views(view(image_width=W_FIRST, campos=None))), 1, "view 0: missing pointer", None),
        ]
    for e in ("gs_backward_gaussians_adam", "gs_backward_gaussians_adam_stats"):
        for W, H, ok in LIMIT_SIZES:
            v1 = ctypes.pointer(view(image_width=W, image_height=H))
            rows.append((e, dict(view1=v1, steps=lls(1, 1, 0, 1, 1, 1)), 1,
                         "adam: step must be >= 1" if ok else E_LIMIT(W, H, "view: "), None))
    return rows


ROWS = build_rows()
LIMIT_ROWS = size_limit_rows()


def _id(i, row):
    e, over = row[0], row[1]
    return f"{i:03d}-{e[3:]}[" + ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else '*'}"
                                         for k, v in over.items()) + "]"


def call(entry, over):
    """One call of `entry` with the default (valid-looking) arguments and `over` on top; returns
    (rc, error text, what *num_rendered_host holds afterwards)."""
    names = PARAMS[entry].split()
    unknown = set(over) - set(names)
    assert not unknown, f"{entry} has no argument {unknown}"
    nr = ctypes.c_longlong(SENTINEL)
    args, left = [], None
    for n in names:
        if n == "nr":
            v = over.get("nr", nr)
            args.append(None if v is None else ctypes.byref(nr))
            left = None if v is None else nr
        elif n == "shs_rest" and n not in over:
            args.append(None if entry in NO_REST else X)
        else:
            v = over[n] if n in over else _default(n)
            if n == "nrs":
                left = v
            args.append(v)
    lib = _native.load()
    rc = getattr(lib, entry)(*args)
    err = lib.gs_last_error().decode()
    if left is None:
        return rc, err, None
    return rc, err, left.value if isinstance(left, ctypes.c_longlong) else list(left)


def test_table_covers_every_entry_and_matches_the_declared_signatures():
    assert {r[0] for r in ROWS} == set(PARAMS)
    for entry, names in PARAMS.items():
        assert len(names.split()) == len(_native.SIGNATURES[entry][1]), entry
    assert X.value % 16 == 0


@pytest.mark.parametrize("row", ROWS, ids=[_id(i, r) for i, r in enumerate(ROWS)])
def test_early_return(row):
    entry, over, rc, text, left = row
    got = call(entry, over)
    assert got == (rc, text, left), (entry, over)


@pytest.mark.parametrize("row", LIMIT_ROWS, ids=[_id(i, r) for i, r in enumerate(LIMIT_ROWS)])
def test_image_size_limits(row):
    entry, over, rc, text, left = row
    got = call(entry, over)
    assert got == (rc, text, left), (entry, over)


def test_image_size_limit_rows_cover_every_entry_with_a_size():
    with_size = {e for e, names in PARAMS.items() if {"W", "Ws", "view_list", "view1"} & set(names.split())}
    assert {r[0] for r in LIMIT_ROWS} == with_size == set(PARAMS)
    for W, H, ok in LIMIT_SIZES:  # the table's own arithmetic, from the limits as documented
        gx, gy = -(-W // 16), -(-H // 16)
        assert ok == (gx <= 65535 and gy <= 65535 and gx * gy <= 1 << 22), (W, H)


def test_sizing_queries_return_zero_past_the_limits():
    """gs_image_buffer_bytes, gs_binning_buffer_bytes and gs_binning_layout_count agree with the
    entries: a size the entries refuse has no buffer size (0, the message in gs_last_error), the
    last accepted size has one, and a refused query does not fail the thread's next call."""
    lib = _native.load()
    for W, H, ok in LIMIT_SIZES:
        img, binb = lib.gs_image_buffer_bytes(W, H), lib.gs_binning_buffer_bytes(1000, W, H)
        if ok:
            assert img >= 8 * W * H and binb >= 20 * 1000, (W, H)
            assert lib.gs_binning_layout_count(binb, W, H) >= 1000
        else:
            assert img == 0 and binb == 0 and lib.gs_binning_layout_count(1 << 40, W, H) == 0, (W, H)
            assert lib.gs_last_error().decode() == E_LIMIT(W, H)
            assert call("gs_forward_render", dict(P=0)) == (0, "", None)  # the next call starts clean
    # 17 tile bits and a non-positive size: as before
    assert lib.gs_image_buffer_bytes(4107, 4085) >= 8 * 4107 * 4085
    assert lib.gs_image_buffer_bytes(0, 16) > 0


def test_rasterizer_refuses_an_oversized_image_before_the_device():
    """Through GaussianRasterizer: the library's message, raised before any tensor is looked at
    (host tensors here, which an accepted size rejects as such)."""
    import torch

    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

    def rast(W, H):
        eye = torch.eye(4)
        return GaussianRasterizer(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
            viewmatrix=eye, projmatrix=eye, sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False))

    m = torch.zeros((2, 3))
    kw = dict(means3D=m, means2D=m, opacities=torch.ones(2, 1), colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    import re

    with pytest.raises(RuntimeError, match=re.escape(E_LIMIT(SQ_FIRST, SQ_LAST))):
        rast(SQ_FIRST, SQ_LAST)(**kw)
    with pytest.raises(RuntimeError, match=re.escape(E_LIMIT(16, W_FIRST))):
        rast(16, W_FIRST)(**kw)
    with pytest.raises(RuntimeError, match="no CPU rasterizer"):
        rast(SQ_LAST, SQ_LAST)(**kw)
