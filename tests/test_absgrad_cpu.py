"""The absolute screen-space gradient without a GPU: the dense reference's closed form, and the host
contract of gs_backward_accumulate_absgrad / gs_grad_buffer_bytes_absgrad.

1. dense_ref_absgrad.absgrad_local forms dL/dalpha per (pixel, Gaussian) in closed form (no autograd).  Its
   signed sums must equal fp64 autograd's dL/dmeans2D of dense_ref.render_local (and, with the aux channels,
   of dense_ref_aux.render_local_aux) to 1e-10 of the largest entry: that proves the closed form, of which
   the absolute sums are the same terms without their signs.  abs >= |signed| elementwise.
2. The new entry's validation comes before any device work (the shared host steps): the messages and their
   order, in the style of tests/test_api_contract_cpu.py.  Every pointer is NULL or a host address the
   library only tests for NULL.
3. gs_grad_buffer_bytes_absgrad >= gs_grad_buffer_bytes_aux, by at least the side arrays.
4. The autograd layer's refusals that need no device: means2D without requires_grad, prepared=,
   binning_capacity=; add_densification_stats(absgrad=True) without the attribute.
"""
import ctypes
import math

import pytest
import torch

import dense_ref
import dense_ref_absgrad
import dense_ref_aux
import gs_scenes
from diff_gaussian_rasterization import _native

f64 = torch.float64


def _case(W, H, P, seed):
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, 1, cam=cam, seed=seed)
    t = {k: getattr(sc, k).to(f64) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    args = (cam.world_view_transform.to(f64), cam.full_proj_transform.to(f64), cam.camera_center.to(f64),
            math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H)
    g = torch.Generator().manual_seed(seed + 1)
    bg = torch.tensor([0.2, 0.5, 0.9], dtype=f64)
    dpix = torch.randn((3, H, W), generator=g, dtype=f64)
    d_alpha = torch.randn((1, H, W), generator=g, dtype=f64)
    d_inv = torch.randn((1, H, W), generator=g, dtype=f64)
    return t, args, bg, dpix, d_alpha, d_inv


@pytest.mark.parametrize("W,H,P,seed", [(40, 24, 30, 3), (72, 40, 3, 41)])
def test_signed_sums_equal_autograd(W, H, P, seed):
    t, args, bg, dpix, d_alpha, d_inv = _case(W, H, P, seed)
    kw = dict(shs=t["shs"], deg=1, scales=t["scales"], rots=t["rotations"])
    for aux in (False, True):
        m2 = torch.zeros_like(t["means3D"], requires_grad=True)
        if aux:
            img, radii, _, inv, alpha = dense_ref_aux.render_local_aux(t["means3D"], m2, t["opacities"], *args, bg, **kw)
            ((img * dpix).sum() + (alpha * d_alpha).sum() + (inv * d_inv).sum()).backward()
        else:
            img, radii, _ = dense_ref.render_local(t["means3D"], m2, t["opacities"], *args, bg, **kw)
            (img * dpix).sum().backward()
        ref = dense_ref_absgrad.absgrad_local(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], *args, bg,
                                              dpix, dL_dalpha=d_alpha if aux else None,
                                              dL_dinvdepth=d_inv if aux else None, **kw)
        assert torch.equal(ref["radii"], radii) and int((radii > 0).sum()) >= min(P, 3)
        want = m2.grad
        scale = float(want.abs().max())
        err = float((ref["signed"] - want).abs().max())
        print(f"\n[{W}x{H} P={P} aux={aux}] max|signed - autograd| {err:.3e}  max|autograd| {scale:.3e}")
        assert scale > 0 and err <= 1e-10 * scale
        assert not ref["signed"][:, 2].any() and not ref["abs"][:, 2].any()
        assert bool((ref["abs"] >= ref["signed"].abs()).all())
        assert bool((ref["abs"][:, :2] > ref["signed"][:, :2].abs()).any())  # a random dL/dimage cancels somewhere
        assert not ref["abs"][radii == 0].any()


def test_zero_flagged_masks_the_gradient():
    t, args, bg, dpix, _, _ = _case(40, 24, 30, 3)
    kw = dict(shs=t["shs"], deg=1, scales=t["scales"], rots=t["rotations"])
    z = torch.zeros_like(t["means3D"])
    also = torch.ones((24, 40), dtype=torch.bool)
    ref = dense_ref_absgrad.absgrad_local(t["means3D"], z, t["opacities"], *args, bg, dpix, zero_flagged=True,
                                          also_flag=also, **kw)
    assert not ref["keep"].any() and not ref["abs"].any() and not ref["signed"].any()


# ---- the host contract of the new entries ----
_BUF = (ctypes.c_float * 64)()
X = ctypes.cast(_BUF, ctypes.c_void_p)

NAMES = ("P D M bg W H means3D shs shs_rest colors opac scales scale_modifier rots cov3D view proj campos tan_fovx "
         "tan_fovy radii geom num_rendered binning image dL_dout_color dL_dout_invdepth dL_dout_alpha grad_buffer "
         "dmeans2D dcolors dopacity dmeans3D dcov3D dsh dscales drots accumulate wait_event debug stream antialiasing "
         "dmeans2D_abs").split()
DEFAULTS = dict(P=4, D=3, M=16, W=16, H=16, scale_modifier=1.0, tan_fovx=0.5, tan_fovy=0.5, num_rendered=10,
                accumulate=0, wait_event=None, debug=0, stream=None, colors=None, cov3D=None, shs_rest=None,
                antialiasing=0)


def call(entry, **over):
    assert not set(over) - set(NAMES)
    names = NAMES if entry == "gs_backward_accumulate_absgrad" else NAMES[:-1]
    args = [over[n] if n in over else DEFAULTS.get(n, X) for n in names]
    lib = _native.load()
    rc = getattr(lib, entry)(*args)
    return rc, lib.gs_last_error().decode()


E_IN = "missing required input pointer"
E_BUF = "missing buffer pointer"
ROWS = [
    (dict(P=-1, W=0), 1, "P must be >= 0"),
    (dict(W=0, means3D=None), 1, "image size must be positive (got 0 x 16)"),
    (dict(P=0, means3D=None, dmeans2D_abs=None), 0, ""),
    (dict(P=0), 0, ""),
    (dict(means3D=None, D=7), 1, E_IN),
    (dict(view=None), 1, E_IN),
    (dict(colors=X, D=7), 1, "Please provide excatly one of either SHs or precomputed colors!"),
    (dict(scales=None), 1, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    (dict(D=4, M=9), 1, "SH degree must be in [0, 3] (got 4)"),
    (dict(campos=None, geom=None), 1, "campos is required with SHs"),
    (dict(geom=None), 1, E_BUF),
    (dict(grad_buffer=None), 1, E_BUF),
    (dict(dL_dout_color=None, dmeans2D=None), 1, E_BUF),
    (dict(dmeans2D=None), 1, "missing gradient output pointer"),
    (dict(num_rendered=1 << 31), 1, "num_rendered out of range"),
    (dict(accumulate=0x100), 1, "accumulate: unknown GS_ACC bits 0x100"),
    # antialiasing: the opacities are required, and split rows are refused first, as gs_backward_accumulate_aa does
    (dict(antialiasing=1, opac=None), 1, E_IN),
    (dict(antialiasing=0, opac=None, geom=None), 1, E_BUF),
    (dict(antialiasing=1, shs_rest=X, means3D=None), 1, "antialiasing: not supported with split SH rows (shs_rest)"),
    (dict(shs_rest=X, D=0, M=1, geom=None), 1, "split SH: M must be >= 2 (got 1)"),
]


@pytest.mark.parametrize("over,rc,text", ROWS, ids=[str(i) for i in range(len(ROWS))])
def test_absgrad_entry_early_return(over, rc, text):
    assert call("gs_backward_accumulate_absgrad", **over) == (rc, text), over
    # the call it extends answers the same (the shared host steps): with the output NULL it IS that call
    over_aa = {k: v for k, v in over.items() if k != "dmeans2D_abs"}
    assert call("gs_backward_accumulate_aa", **over_aa) == (rc, text), over
    assert call("gs_backward_accumulate_absgrad", **dict(over, dmeans2D_abs=None)) == (rc, text), over


def test_signature_is_the_aa_entry_plus_the_output():
    sig = _native.SIGNATURES
    assert sig["gs_backward_accumulate_absgrad"][1] == sig["gs_backward_accumulate_aa"][1] + [ctypes.c_void_p]
    assert len(sig["gs_backward_accumulate_absgrad"][1]) == len(NAMES)


def test_grad_buffer_bytes_absgrad():
    lib = _native.load()
    for R, P in ((0, 0), (1, 1), (10, 4), (1000, 300), (1 << 20, 100000), ((1 << 31) - 1, 1 << 24), (-5, -5)):
        aux, ab = lib.gs_grad_buffer_bytes_aux(R, P), lib.gs_grad_buffer_bytes_absgrad(R, P)
        Re, Pe = max(R, 1), max(P, 1)
        assert ab >= aux + 8 * Re + 8 * Pe, (R, P)
        assert ab <= aux + 8 * Re + 8 * Pe + 512 and ab % 256 == 0, (R, P)
    # 64-bit offsets: the largest instance count's side arrays start past 2^32 bytes
    assert lib.gs_grad_buffer_bytes_absgrad((1 << 31) - 1, 1) > 44 * ((1 << 31) - 1)


# ---- the autograd layer's host-side refusals (no device is reached) ----
def test_rasterizer_keyword_and_refusals():
    import inspect

    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert p["absgrad"].default is False
    eye = torch.eye(4)
    r = GaussianRasterizer(GaussianRasterizationSettings(
        image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=eye, projmatrix=eye, sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False))
    m = torch.zeros((2, 3))
    kw = dict(means3D=m, opacities=torch.ones(2, 1), colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    m2 = torch.zeros((2, 3), requires_grad=True)
    with pytest.raises(RuntimeError, match="^absgrad: means2D does not require grad$"):
        r(means2D=m, absgrad=True, **kw)
    with pytest.raises(RuntimeError, match="^absgrad: not supported with prepared=$"):
        r(means2D=m2, absgrad=True, prepared=object(), **kw)
    with pytest.raises(RuntimeError, match="^absgrad: not supported with binning_capacity=$"):
        r(means2D=m2, absgrad=True, binning_capacity=100, **kw)
    with pytest.raises(RuntimeError, match="no CPU rasterizer"):  # accepted: the call goes on to the device check
        r(means2D=m2, absgrad=True, **kw)
    assert not hasattr(m2, "absgrad")


def test_add_densification_stats_needs_the_attribute():
    import gs_train

    v = torch.zeros((2, 3), requires_grad=True)
    v.grad = torch.zeros((2, 3))
    with pytest.raises(RuntimeError, match="has no .absgrad"):
        gs_train.add_densification_stats(object(), v, torch.zeros(2, dtype=torch.int32), absgrad=True)
