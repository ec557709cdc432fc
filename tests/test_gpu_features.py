"""Feature rendering (gs_features.render_features, gs_feature_forward / gs_feature_backward) on the GPU.

The scenes are tests/test_gpu_contrib.py's, built by its _scene (sparse, deep, opaque at 200 x 120;
empty-tile, 3 Gaussians at 72 x 40).  Every check runs in both numerics modes (gs_set_exact_exp),
with the channel counts C in {1, 3, G, G + 1, 2 G + 3}, G = gs_feature_group_channels(): one group, a
full group, a one-channel tail group, three groups with a tail -- so both instantiations of the two
walks and the reduce are launched in this process (tests/test_zz_kernel_coverage.py).

1. Bit identities (torch.equal): run to run, forward and backward; features = colors_precomp gives
   the plain call's image over a zero background; a channel of 1 / depth gives the aux inverse depth;
   under a non-negative map m per channel, dL/dfeatures[:, c] is contribution_stats' wsum under m;
   channel c of a C-channel render is the one-channel render of column c, and likewise the backward;
   two views accumulated with out= equal the two results added in torch; radii == 0 rows are zero;
   forward -> features -> colour backward leaves the colour backward's gradients as forward ->
   backward gives them; P == 0 and a zero gradient give zeros; on empty-tile the tiles without entries
   are zero and every pixel of a NaN-prefilled output is written.
2. dL/dfeatures (C = 3, a signed random gradient) against dL/dcolors_precomp of the plain call with
   dL/dimage = g and bg = 0, within twice test_gpu_dense._check's bound (test_gpu_contrib._check2).
3. A channel of ones against the aux alpha, per pixel within 2 n_contrib[p] 2^-24 (two roundings per
   composited entry of the telescoping product; tests/test_gpu_aux.py section 2).
4. Against the fp64 dense reference (dense_ref_features.features_local, flag_rel=1e-3, flag_T_rel=1e-2),
   C = G + 1: flagged pixels and the widened rectangles of Gaussians whose radius differs are left out
   of `out` and g is zeroed there; max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|ref| for out and
   for dL/dfeatures; at most 2 % of the pixels flagged and a mean of differing radii <= 1e-3 (asserted).
   The map is linear in the features, so this is the gradient check (no gradcheck: fp32 kernels).
5. Autograd: render_features(view, f).backward() gives the raw call's gradient; the same view again
   with another C.
6. Refusals: a wrong shape, dtype or device, C = 0 and C above the limit raise with their messages.
"""
import math

import numpy as np
import pytest
import torch

import dense_cases
import dense_ref_features
import gs_scenes
import test_gpu_contrib as tc
from gpu_checks import check_4x, check_tol, mode  # noqa: F401

pytestmark = pytest.mark.gpu


def _G():
    from diff_gaussian_rasterization import _C

    return _C.feature_group_channels()


def _channel_counts():
    G = _G()
    return [1, 3, G, G + 1, 2 * G + 3]


def _view(cam, leaves, deg, device, **over):
    import gs_features

    v = gs_features.FeatureView.from_inputs(tc._rasterizer(cam, deg, device), **tc._inputs(leaves, **over))
    torch.cuda.synchronize()
    return v


def _fwd(view, f, out=None):
    from diff_gaussian_rasterization import _C

    r = _C.feature_forward(*view._args(), f, out=out)
    torch.cuda.synchronize()
    return r


def _bwd(view, g, out=None):
    from diff_gaussian_rasterization import _C

    r = _C.feature_backward(*view._args(), g, out=out)
    torch.cuda.synchronize()
    return r


def _randn(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


# ------------------------------------------------------------------------------------------
# 1. bit identities
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_run_to_run_and_group_independence(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    view = _view(cam, leaves, deg, device)
    Cs = _channel_counts()
    Cmax = max(Cs)
    F, g = _randn((P, Cmax), 101, device), _randn((Cmax, H, W), 102, device)
    # the one-channel renders of every column, once
    one_out = [_fwd(view, F[:, c:c + 1].contiguous()) for c in range(Cmax)]
    one_d = [_bwd(view, g[c:c + 1].contiguous()) for c in range(Cmax)]
    assert float(one_out[0].abs().max()) > 0 and float(one_d[0].abs().max()) > 0
    for C in Cs:
        f, gc = F[:, :C].contiguous(), g[:C].contiguous()
        out, out2 = _fwd(view, f), _fwd(view, f)
        d, d2 = _bwd(view, gc), _bwd(view, gc)
        assert out.shape == (C, H, W) and d.shape == (P, C) and out.dtype == d.dtype == torch.float32
        assert torch.equal(out, out2), f"C={C}: the forward differs run to run"
        assert torch.equal(d, d2), f"C={C}: the backward differs run to run"
        for c in range(C):
            assert torch.equal(out[c], one_out[c][0]), f"C={C}: channel {c} differs from its one-channel render"
            assert torch.equal(d[:, c], one_d[c][:, 0]), f"C={C}: column {c} differs from its one-channel backward"
        assert not d[view.radii == 0].any()  # radii == 0 rows are exactly zero
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all())
    # a zero gradient gives zeros
    assert not _bwd(view, torch.zeros((Cs[-1], H, W), device=device)).any()


@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_colour_and_inverse_depth_identities(device, mode, name):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    G = _G()
    cols = torch.rand((P, 3), generator=torch.Generator().manual_seed(3)).to(device)
    # (a) features = colors_precomp: the plain call's image over a zero background
    img, radii = tc._render(cam, leaves, deg, device, shs=None, colors_precomp=cols)
    view = _view(cam, leaves, deg, device)
    assert torch.equal(view.radii, radii)
    out = _fwd(view, cols)
    assert float(img.abs().max()) > 0
    assert torch.equal(out, img), f"{int((out != img).sum())} of {img.numel()} values differ from the colour path"
    # the view keeps its own rendered colour (SH here)
    img_sh, _ = tc._render(cam, leaves, deg, device)
    assert torch.equal(view.color, img_sh)
    # (b) a channel of 1 / depth (a correctly rounded division, on the host) is the aux inverse depth; it
    # rides in a tail group behind G channels of noise
    ex = _C.debug_export(P, W, H, view.num_rendered, view.geom, view.binning, view.img, device)
    depth = ex["depth"].cpu()
    inv = torch.where(radii.cpu() > 0, 1.0 / depth, torch.zeros_like(depth)).to(device)
    f = torch.cat([_randn((P, G), 7, device), inv[:, None]], 1).contiguous()
    _, _, invdepth, alpha = tc._render(cam, leaves, deg, device, aux=True)
    assert float(invdepth.max()) > 0
    assert torch.equal(_fwd(view, f)[G], invdepth[0])
    assert torch.equal(_fwd(view, inv[:, None].contiguous())[0], invdepth[0])


@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_backward_is_wsum_per_channel_and_accumulates(device, mode, name):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    G = _G()
    C = G + 1
    view = _view(cam, leaves, deg, device)
    maps = torch.stack([tc._map(cam, device, seed=30 + c) - 0.25 for c in range(C)])  # in [0, 1)
    assert float(maps.min()) >= 0.0
    d = _bwd(view, maps)
    for c in range(C):
        wsum = _C.contribution_stats(*view._args(), pixel_weights=maps[c])[0]
        assert torch.equal(d[:, c], wsum), f"column {c} differs from wsum under its map"
    assert float(d.max()) > 0
    # two views accumulated in place
    cam2 = gs_scenes.jittered_cameras(2, W, H)[1]
    view2 = _view(cam2, leaves, deg, device)
    g = _randn((C, H, W), 55, device)
    d1, d2 = _bwd(view, g), _bwd(view2, g)
    acc = d1.clone()
    ret = _bwd(view2, g, out=acc)
    assert ret.data_ptr() == acc.data_ptr()
    assert torch.equal(ret, d1 + d2) and not torch.equal(d1, d2)


@pytest.mark.parametrize("name", ["sparse", "opaque"])
def test_features_leave_the_colour_backward_alone(device, mode, name):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    C = 2 * _G() + 3
    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    e = torch.Tensor([])
    dpix = gs_scenes.dl_dimage(H, W, seed=5, scale=1.0).to(device)
    F, g = _randn((P, C), 61, device), _randn((C, H, W), 62, device)

    def run(features):
        with torch.no_grad():
            R, color, radii, geom, binning, img = _C.rasterize_gaussians_two_call(
                s.bg, leaves["means3D"], e, leaves["opacities"], leaves["scales"], leaves["rotations"],
                s.scale_modifier, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, H, W, leaves["shs"],
                s.sh_degree, s.campos, s.prefiltered, s.debug)
            args = (R, radii, geom, binning, img, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, H, W)
            before = (_C.feature_forward(*args, F), _C.feature_backward(*args, g)) if features else None
            grads = _C.rasterize_gaussians_backward(
                s.bg, leaves["means3D"], radii, e, leaves["scales"], leaves["rotations"], s.scale_modifier, e,
                s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, leaves["shs"], s.sh_degree, s.campos, geom, R,
                binning, img, s.debug)
            after = (_C.feature_forward(*args, F), _C.feature_backward(*args, g)) if features else None
            ex = _C.debug_export(P, W, H, R, geom, binning, img, device)
        torch.cuda.synchronize()
        return color, radii, grads, ex, before, after

    c0, r0, g0, ex0, _, _ = run(False)
    c1, r1, g1, ex1, before, after = run(True)
    assert torch.equal(c0, c1) and torch.equal(r0, r1)
    for k in ("final_T", "n_contrib", "point_list", "ranges"):
        assert torch.equal(ex0[k], ex1[k]), k
    assert len(g0) == len(g1) == 8
    for k, (u, v) in enumerate(zip(g0, g1)):
        assert torch.equal(u, v), f"gradient {k} differs after the feature calls"
    for u, v in zip(before, after):
        assert torch.equal(u, v), "after the colour backward differs from before it"


def test_no_gaussians_give_zeros(device, mode):
    import gs_features

    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    none = {k: v[:0].contiguous() for k, v in leaves.items()}
    view = _view(cam, none, deg, device)
    for C in (1, _G() + 1):
        out = _fwd(view, torch.zeros((0, C), device=device), out=torch.full((C, H, W), math.nan, device=device))
        assert out.shape == (C, H, W) and not out.any()
        assert _bwd(view, torch.ones((C, H, W), device=device)).shape == (0, C)
        f = torch.zeros((0, C), device=device, requires_grad=True)
        gs_features.render_features(view, f).sum().backward()
        assert f.grad.shape == (0, C)


def test_empty_tiles_are_written_as_zeros(device, mode):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene("empty-tile", device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    view = _view(cam, leaves, deg, device)
    ex = _C.debug_export(P, W, H, view.num_rendered, view.geom, view.binning, view.img, device)
    ranges = ex["ranges"].cpu().numpy()
    empty = np.nonzero(ranges[:, 1] == ranges[:, 0])[0]
    gx = (W + 15) // 16
    assert 1 <= empty.size < ranges.shape[0]
    for C in _channel_counts():
        out = torch.full((C, H, W), math.nan, device=device)
        ret = _fwd(view, torch.ones((P, C), device=device) + _randn((P, C), 70 + C, device).abs(), out=out)
        assert ret.data_ptr() == out.data_ptr()
        assert bool(torch.isfinite(out).all()), "a pixel was not written"
        assert float(out.max()) > 0
        for t in empty:
            ty, tx = divmod(int(t), gx)
            assert not out[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].any()


# ------------------------------------------------------------------------------------------
# 2. against the existing backward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "deep", "opaque"])
def test_backward_against_the_colour_gradient(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    g = gs_scenes.dl_dimage(H, W, seed=5, scale=1.0).to(device)
    cols = torch.rand((P, 3), generator=torch.Generator().manual_seed(3)).to(device).requires_grad_(True)
    kw = tc._inputs(leaves, shs=None, colors_precomp=cols)
    img, radii = tc._rasterizer(cam, deg, device)(means2D=torch.zeros_like(leaves["means3D"]), **kw)
    (img * g).sum().backward()
    torch.cuda.synchronize()
    view = _view(cam, leaves, deg, device)
    assert torch.equal(radii, view.radii)
    d = _bwd(view, g)
    print()
    check_tol(d, cols.grad, f"[{name}] dL/dfeatures vs dL/dcolors_precomp", times=2)


# ------------------------------------------------------------------------------------------
# 3. alpha
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "deep", "opaque", "empty-tile"])
def test_channel_of_ones_against_the_aux_alpha(device, mode, name):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    view = _view(cam, leaves, deg, device)
    ones = _fwd(view, torch.ones((P, 1), device=device))[0].double()
    _, _, _, alpha = tc._render(cam, leaves, deg, device, aux=True)
    ex = _C.debug_export(P, W, H, view.num_rendered, view.geom, view.binning, view.img, device)
    bound = 2.0 * ex["n_contrib"].double() * 2.0 ** -24
    d = (ones - alpha[0].double()).abs()
    worst = float((d / bound.clamp_min(2.0 ** -60)).max())
    print(f"\n[{name}] ones channel vs aux alpha: max|d| {float(d.max()):.3e}, largest bound "
          f"{float(bound.max()):.3e}, worst pixel at {worst:.3f} of its bound")
    assert float(alpha.max()) > 0
    assert bool((d <= bound).all()), f"{int((d > bound).sum())} pixels beyond 2 n_contrib 2^-24"


# ------------------------------------------------------------------------------------------
# 4. against the fp64 dense reference
# ------------------------------------------------------------------------------------------
_DENSE = {}


def _dense(cam, leaves, deg, device, dtype, features, g, **flags):
    t = {k: v.detach().to(dtype) for k, v in leaves.items()}
    return dense_ref_features.features_local(
        t["means3D"], t["means2D"], t["opacities"], *dense_cases.dense_args(cam, device, dtype), features.to(dtype),
        g=g.to(dtype), shs=t["shs"], deg=deg, scales=t["scales"],
        rots=t["rotations"], **flags)


def _dense_case(name, cam, leaves, deg, device, hip_radii, C):
    """(features, g zeroed at the left-out pixels, left-out pixels, differing radii, fp64, fp32): the
    dense side does not depend on the kernels' numerics mode, so it is computed once per scene and set
    of differing radii (test_gpu_contrib._dense_case's scheme)."""
    c = _DENSE.setdefault(name, {})
    P = leaves["means3D"].shape[0]
    if "rect" not in c:
        c["rect"], c["radii"] = dense_cases.rect_and_radii(cam, leaves, deg, device)
        c["F"] = _randn((P, C), 201, device)
        c["g0"] = _randn((C, cam.image_height, cam.image_width), 202, device)
    rdiff = (hip_radii.cpu() != c["radii"]).numpy()
    wide = dense_cases.wide_mask(c["rect"], rdiff, cam.image_width, cam.image_height)
    if "wide" not in c or not np.array_equal(c["wide"], wide):
        c["wide"] = wide
        c["f64"] = _dense(cam, leaves, deg, device, torch.float64, c["F"], c["g0"], flag_rel=1e-3, flag_T_rel=1e-2,
                          zero_flagged=True, also_flag=torch.from_numpy(wide))
        c["g"] = c["f64"]["g"].float().contiguous()
        c["f32"] = _dense(cam, leaves, deg, device, torch.float32, c["F"], c["g"])
    out = c["f64"]["flag"].cpu().numpy() | wide
    assert torch.equal((c["g"] == 0).all(0), torch.from_numpy(out).to(device))
    return c["F"], c["g"], out, rdiff, c["f64"], c["f32"]


@pytest.mark.parametrize("name", ["sparse", "deep", "opaque"])
def test_against_dense_fp64(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    P = leaves["means3D"].shape[0]
    C = _G() + 1
    view = _view(cam, leaves, deg, device)
    F, g, left_out, rdiff, r64, r32 = _dense_case(name, cam, leaves, deg, device, view.radii, C)
    print(f"\n[{name}] pixels left out {int(left_out.sum())}/{left_out.size} ({left_out.mean():.4f}), radii differing "
          f"{int(rdiff.sum())}/{P}")
    assert left_out.mean() <= 0.02
    assert rdiff.mean() <= 1e-3, f"{int(rdiff.sum())} radii differ"
    out, d = _fwd(view, F), _bwd(view, g)
    keep_px = np.broadcast_to(~left_out, (C,) + left_out.shape)
    check_4x(out, r64["out"], r32["out"], f"[{name}] out", keep_px)
    check_4x(d, r64["dfeat"], r32["dfeat"], f"[{name}] dL/dfeatures", ~rdiff)


# ------------------------------------------------------------------------------------------
# 5. autograd
# ------------------------------------------------------------------------------------------
def test_autograd_matches_the_raw_call(device, mode):
    import gs_features

    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    G = _G()
    view = _view(cam, leaves, deg, device)
    for C in (G + 1, 3):  # one view, rendered again with another C
        f = _randn((P, C), 300 + C, device).requires_grad_(True)
        g = _randn((C, H, W), 310 + C, device)
        out = gs_features.render_features(view, f)
        assert out.requires_grad and torch.equal(out.detach(), _fwd(view, f.detach()))
        (out * g).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(f.grad, _bwd(view, g))
    # nothing flows to the geometry: the view was made without a graph
    m = leaves["means3D"].clone().requires_grad_(True)
    f = _randn((P, 3), 320, device).requires_grad_(True)
    out = gs_features.render_features_for(tc._rasterizer(cam, deg, device), f, **tc._inputs(leaves, means3D=m))
    out.sum().backward()
    torch.cuda.synchronize()
    assert m.grad is None and f.grad is not None
    assert torch.equal(out.detach(), _fwd(view, f.detach()))


# ------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------
def test_refused_inputs(device):
    import gs_features
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    view = _view(cam, leaves, deg, device)
    lim = gs_features.MAX_CHANNELS
    bad = [torch.zeros((P,), device=device), torch.zeros((P - 1, 4), device=device),
           torch.zeros((P, 4, 1), device=device), torch.zeros((P, 0), device=device),
           torch.zeros((P, lim + 1), device=device), torch.zeros((P, 4), device=device, dtype=torch.float64),
           torch.zeros((P, 4))]
    for f in bad:
        with pytest.raises(ValueError, match=r"features must be a float32 tensor of shape \(%d, C\), 1 <= C <= %d"
                           % (P, lim)):
            gs_features.render_features(view, f)
    # the library's own refusals through the raw calls
    with pytest.raises(RuntimeError, match=r"feature channels must lie in \[1, %d\] \(got %d\)" % (lim, lim + 1)):
        _C.feature_forward(*view._args(), torch.zeros((P, lim + 1), device=device))
    with pytest.raises(RuntimeError, match=r"features must have shape \(%d, C\) with C >= 1" % P):
        _C.feature_forward(*view._args(), torch.zeros((P, 0), device=device))
    with pytest.raises(RuntimeError, match="dL_dout must have shape"):
        _C.feature_backward(*view._args(), torch.zeros((3, H, W + 1), device=device))
    with pytest.raises(RuntimeError, match="out must be a contiguous float32 tensor of shape"):
        _C.feature_backward(*view._args(), torch.zeros((3, H, W), device=device),
                            out=torch.zeros((P, 4), device=device))
    # the limit itself renders
    out = _fwd(view, torch.zeros((P, lim), device=device))
    assert out.shape == (lim, H, W) and not out.any()
    torch.cuda.synchronize()
