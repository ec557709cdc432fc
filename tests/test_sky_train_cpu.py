"""The deferred aux backward's C entries (GSRAST_HAS_AUX_DEFERRED), without a GPU.

gs_backward_render_aux and gs_backward_gaussians_adam_stats_aux are gs_backward_render and
gs_backward_gaussians_adam_stats with the aux arguments added, and the old entries forward to them:
the host contract of the new entries is the old entries' contract, row for row (the tables of
test_api_contract_cpu.py, run here against the new names), plus the rule of the new argument --
invdepth_sums is a required buffer exactly when an aux gradient is given.  As there, every row has a
fault or an empty scene in front of the first device call.
"""
import ctypes
import os
import re

import pytest

import test_api_contract_cpu as tc
from diff_gaussian_rasterization import _native

X, ODD = tc.X, tc.ODD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = {
    "gs_backward_render_aux": (f"P D M bg W H {tc.CAM} geom num_rendered binning image dL_dout_color "
                               "dL_dout_invdepth dL_dout_alpha grad_buffer dmeans2D invdepth_sums accumulate debug "
                               "stream"),
    "gs_backward_gaussians_adam_stats_aux": (f"{tc.ADAM} st_radii grad2d grad_stride max_radii2D grad_accum denom "
                                             "invdepth_sums debug stream"),
}


def call(entry, over):
    names = PARAMS[entry].split()
    assert not set(over) - set(names), f"{entry} has no argument {set(over) - set(names)}"
    args = [over[n] if n in over else tc._default(n) for n in names]
    lib = _native.load()
    rc = getattr(lib, entry)(*args)
    return rc, lib.gs_last_error().decode()


def test_header_declares_the_deferred_aux_entries():
    with open(os.path.join(ROOT, "include", "gsrast.h")) as f:
        text = f.read()
    assert re.search(r"^#define GSRAST_HAS_AUX_DEFERRED 1$", text, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", text).group(1)) == 17
    assert _native.load().gs_abi_version() == 17
    for name in PARAMS:
        assert re.search(rf"^int {name}\(", text, re.M), name


def test_signatures_resolve_and_match_the_argument_lists():
    lib = _native.load()
    for name, names in PARAMS.items():
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(names.split()), name
        assert getattr(lib, name).argtypes == args
    # the old entries with the new arguments in place: same types otherwise
    r, ra = _native.SIGNATURES["gs_backward_render"][1], _native.SIGNATURES["gs_backward_render_aux"][1]
    assert ra == r[:16] + [ctypes.c_void_p] * 2 + r[16:18] + [ctypes.c_void_p] + r[18:]
    a = _native.SIGNATURES["gs_backward_gaussians_adam_stats"][1]
    aa = _native.SIGNATURES["gs_backward_gaussians_adam_stats_aux"][1]
    assert aa == a[:-2] + [ctypes.c_void_p] + a[-2:]


def _render_rows():
    e, rows = "gs_backward_render_aux", []
    # gs_backward_render's rows: with both aux gradients (invdepth_sums given), with one, and with
    # none and no invdepth_sums (the plain call) -- the same check answers in each
    base = [r for r in tc.ROWS if r[0] == "gs_backward_render"]
    assert len(base) == 16
    for more in (dict(), dict(dL_dout_alpha=None), dict(dL_dout_invdepth=None, dL_dout_alpha=None, invdepth_sums=None)):
        rows += [(e, dict(over, **more), rc, text) for _e, over, rc, text, _l in base]
    rows += [
        # an aux gradient without invdepth_sums: a missing buffer, in the buffers' place in the order
        (e, dict(invdepth_sums=None), 1, tc.E_BUF),
        (e, dict(invdepth_sums=None, dL_dout_invdepth=None), 1, tc.E_BUF),
        (e, dict(invdepth_sums=None, dL_dout_alpha=None), 1, tc.E_BUF),
        (e, dict(invdepth_sums=None, bg=None), 1, tc.E_IN),
        (e, dict(invdepth_sums=None, num_rendered=-1), 1, tc.E_BUF),
        (e, dict(invdepth_sums=None, accumulate=2), 1, tc.E_BUF),
        (e, dict(invdepth_sums=None, W=0), 1, tc.E_SIZE % (0, 16)),
        (e, dict(invdepth_sums=None, P=-1), 1, tc.E_P),
        (e, dict(invdepth_sums=None, P=0), 0, ""),
        # no aux gradient: invdepth_sums is not looked at
        (e, dict(invdepth_sums=None, dL_dout_invdepth=None, dL_dout_alpha=None, num_rendered=-1), 1, tc.E_NR),
        (e, dict(dL_dout_invdepth=None, dL_dout_alpha=None, num_rendered=tc.BIG), 1, tc.E_NR),
    ]
    return rows


def _adam_rows():
    e = "gs_backward_gaussians_adam_stats_aux"
    base = [r for r in tc.ROWS if r[0] == "gs_backward_gaussians_adam_stats"]
    assert len(base) == 23
    rows = []
    for more in (dict(), dict(invdepth_sums=None)):
        rows += [(e, dict(over, **more), rc, text) for _e, over, rc, text, _l in base]
    return rows


def _size_limit_rows():
    """The image-size limits (tests/test_api_contract_cpu.py) in the two aux entries, after every
    earlier row: the last accepted and the first refused size."""
    r, a = "gs_backward_render_aux", "gs_backward_gaussians_adam_stats_aux"
    v = lambda W, H: ctypes.pointer(tc.view(image_width=W, image_height=H))  # noqa: E731
    rows = []
    for W, H, ok in tc.LIMIT_SIZES:
        rows.append((r, dict(W=W, H=H, view=None), 1, tc.E_IN if ok else tc.E_LIMIT(W, H)))
        rows.append((a, dict(view1=v(W, H), steps=tc.lls(1, 1, 0, 1, 1, 1)), 1,
                     "adam: step must be >= 1" if ok else tc.E_LIMIT(W, H, "view: ")))
    return rows


def _alignment_rows():
    """The fused kernel's 16-byte accesses (tests/test_api_contract_cpu.py, behind every earlier row): the
    parameter and both moments of features_dc, features_rest and rotation, with and without the aux sums,
    in front of the statistics' checks; the scalar groups' moments may sit anywhere."""
    a = "gs_backward_gaussians_adam_stats_aux"
    rows = []
    for k, name in ((1, "features_dc"), (2, "features_rest"), (5, "rotation")):
        for arg in ("params", "exp_avg", "exp_avg_sq"):
            if (k, arg) != (5, "params"):
                rows.append((a, {arg: tc.six(k, ODD)}, 1, tc.E_ADAM_ALIGN % name))
    rows += [
        (a, dict(exp_avg=tc.six(2, ODD), invdepth_sums=None), 1, tc.E_ADAM_ALIGN % "features_rest"),
        (a, dict(exp_avg_sq=tc.six(5, ODD), st_radii=X), 1, tc.E_ADAM_ALIGN % "rotation"),
        (a, dict(exp_avg=tc.six(1, ODD), shs=ODD), 1, "split SH rows must be 16-byte aligned"),
        (a, dict(exp_avg=tc.ptrs(ODD, X, X, ODD, ODD, X), exp_avg_sq=tc.ptrs(ODD, X, X, ODD, ODD, X), st_radii=X), 1,
         "densify stats: all five pointers or none"),
    ]
    return rows


ROWS = _render_rows() + _adam_rows() + _size_limit_rows() + _alignment_rows()


def _id(i, row):
    return f"{i:03d}-{row[0][3:]}[" + ",".join(
        f"{k}={'NULL' if v is None else v if isinstance(v, int) else '*'}" for k, v in row[1].items()) + "]"


@pytest.mark.parametrize("row", ROWS, ids=[_id(i, r) for i, r in enumerate(ROWS)])
def test_early_return(row):
    entry, over, rc, text = row
    assert call(entry, over) == (rc, text)


def test_the_issue_s_cases_are_in_the_table():
    """P < 0, a bad image size, a missing buffer, an aux gradient with invdepth_sums NULL (render
    entry); P < 0, a bad image size, a missing pointer, M != 16 (Adam entry)."""
    got = {(e, text) for e, _o, rc, text in ROWS if rc}
    r, a = "gs_backward_render_aux", "gs_backward_gaussians_adam_stats_aux"
    for want in ((r, tc.E_P), (r, tc.E_SIZE % (0, 16)), (r, tc.E_BUF), (a, tc.E_P), (a, "view: bad image size"),
                 (a, tc.E_IN), (a, "fused Adam backward: 16 SH coefficients, degree 0..3 only")):
        assert want in got, want
    assert (r, dict(invdepth_sums=None), 1, tc.E_BUF) in ROWS
