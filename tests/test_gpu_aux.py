"""The aux outputs of the rasterizer (GaussianRasterizer(..., aux_outputs=True)): alpha = 1 - final_T
and the expected inverse depth sum_i alpha_i T_i / z_i, with their gradients.

Four seeded scenes, all through gs_scenes.identity_camera (200 x 120, not a multiple of the 16-px
tile in either direction, so edge tiles have lanes outside the image):

    sparse      random_gaussians(2000, 3, seed=41): a third of the pixels see no splat (alpha 0), one
                staged batch per tile
    deep        random_gaussians(6000, 1, seed=47, scale_range=(0.01, 0.08)): two to three batches
    opaque      random_gaussians(8000, 1, seed=49, scale_range=(0.02, 0.12)), opacities 0.5 + 0.49 o:
                T-stopped pixels, up to five batches
    empty-tile  the first 3 Gaussians of `sparse` at 72 x 40: most tiles hold no instance (the
                backward's n_eff == 0 return) and the outputs are 0 there

Every check runs in both numerics modes (gs_set_exact_exp), so the four AUX render instantiations
and the two small aux kernels are launched in this process (tests/test_zz_kernel_coverage.py).

1. Bit identities: colour and radii of an aux call equal the plain call's; alpha is 1 - final_T of
   the image buffer, bit for bit; a backward that receives a colour gradient only gives the plain
   path's gradients bit for bit and launches no AUX kernel (the profiler's per-name launch log of
   that backward); two identical aux runs give identical outputs and gradients.
2. Against the existing colour path: the same geometry rendered with colors_precomp = (1/z, 1, 0).
   invdepth vs channel 0 within 1e-6 |ref| (same accumulation by contract, inputs at most 1 ulp
   apart per term, all terms positive: the sum moves by about 2 * 2^-23 relative; 4x that; bit
   equality is expected and printed); alpha vs channel 1 (the sum of the weights) within
   2 n_max 2^-24 (two roundings per composited entry of a telescoping sum, n_max the largest
   n_contrib).  Gradients of L = sum gC color + sum gD invdepth + sum gA alpha against the sum of two
   plain renders' autograd gradients (SH colour with gC; the (1/z, 1, 0) render with gD, gA and z
   built in torch, so autograd carries the depth chain), within twice test_gpu_dense._check's bounds
   (each side is a valid fp32 order that the suite already holds to those bounds against fp64).
3. Against the fp64 dense reference (dense_ref_aux.render_local_aux), test_gpu_dense's harness for
   five outputs: flagged pixels and differing-radius Gaussians left out (caps 0.02 / 1e-3), dL/d.
   zeroed at flagged pixels, three losses (aux only, colour only, all three).  invdepth and alpha:
   max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|ref| (the conditioning rule of
   test_gpu_dense; the dense fp32 run alone reaches 0.97 of 1e-5 |ref| + 1e-5 max on `sparse`'s
   alpha, so that bound has no room for a second fp32 order).  Gradients: _check's bounds, and the
   4x rule for the covariance chain, as there.  The loss weights are the harness's draw,
   dl_dimage(seed = the scene's seed + 1, scale=1.0), for the colour and the next two seeds for
   gD and gA.  Measured on MI355X: every tensor within 0.65 of its bound (the image and dL/dSH of
   sparse / all three; dL/dopacity 0.56).  That bound is tight for fp32: an earlier draw of the weights (seed 11) put one Gaussian of sparse / aux only at
   1.05 of it (HIP -5.2e-5, dense fp32 +0.8e-5 on a gradient of 3.9e-2 whose per-pixel terms
   cancel; the backward recovers T by repeated division, as the plain kernels do, and that
   relative drift does not cancel with the terms), with the dense fp32 run at 0.80 elsewhere.
4. Interface: the refused combinations, an accumulating gradient sink, P == 0, single aux gradients.
"""
import pytest
import torch

import dense_cases
import dense_ref_aux
import gs_scenes
import parity_report
import gpu_checks
from gpu_checks import RTOL, check_4x, check_tol, mode  # noqa: F401

pytestmark = pytest.mark.gpu

CHAIN = ("means2D", "means3D", "scales", "rotations")
LEAVES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
AUX_KERNELS = ("render_fwd_aux", "render_bwd_aux", "sum_records_aux", "depth_chain_aux")


def _weights(cam, device, seed=5):
    H, W = cam.image_height, cam.image_width
    gC = gs_scenes.dl_dimage(H, W, seed=seed, scale=1.0).to(device)
    gD = gs_scenes.dl_dimage(H, W, seed=seed + 1, scale=1.0)[:1].contiguous().to(device)
    gA = gs_scenes.dl_dimage(H, W, seed=seed + 2, scale=1.0)[1:2].contiguous().to(device)
    return gC, gD, gA


def _hip(cam, leaves, deg, device, aux=True, gC=None, gD=None, gA=None, colors=None, into=None):
    """One forward (+ backward of sum gC color + sum gD invdepth + sum gA alpha) through the public
    call.  colors: a [P, 3] tensor (possibly a function of the leaves) instead of the SH rows.
    into: leaf tensors to reuse (their .grad accumulates).  Returns (outputs, leaf tensors)."""
    from diff_gaussian_rasterization import GaussianRasterizer

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    t = into or {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    kw = dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], scales=t["scales"],
              rotations=t["rotations"])
    if colors is None:
        kw["shs"] = t["shs"]
    else:
        kw["colors_precomp"] = colors(t) if callable(colors) else colors
    out = GaussianRasterizer(s)(**kw, aux_outputs=True) if aux else GaussianRasterizer(s)(**kw)
    terms = [(w * o).sum() for w, o in zip((gC, None, gD, gA), out) if w is not None]
    if terms:
        sum(terms).backward()
    torch.cuda.synchronize()
    return out, t


def _grads(t):
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in t.items()}


def _raw_aux(cam, leaves, deg, device):
    """The aux forward through _C, with its buffers (for _C.debug_export)."""
    from diff_gaussian_rasterization import _C

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    e = torch.Tensor([])
    with torch.no_grad():
        R, color, radii, geom, binning, img, invdepth, alpha = _C.rasterize_gaussians_aux(
            s.bg, leaves["means3D"], e, leaves["opacities"], leaves["scales"], leaves["rotations"], s.scale_modifier,
            e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, leaves["shs"],
            s.sh_degree, s.campos, s.prefiltered, s.debug)
        ex = _C.debug_export(leaves["means3D"].shape[0], s.image_width, s.image_height, R, geom, binning, img, device)
    torch.cuda.synchronize()
    return color, radii, invdepth, alpha, ex


# ------------------------------------------------------------------------------------------
# 1. bit identities
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "deep", "opaque", "empty-tile"])
def test_bit_identities(device, mode, name):
    from diff_gaussian_rasterization import _native

    cam, leaves, deg = dense_cases.scene(name, device)
    gC, gD, gA = _weights(cam, device)
    (img0, radii0), t0 = _hip(cam, leaves, deg, device, aux=False, gC=gC)
    lib = gpu_checks.lib()
    # the per-name launch log of one aux forward's colour-only backward
    from diff_gaussian_rasterization import GaussianRasterizer

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    t1 = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    img1, radii1, inv1, alpha1 = GaussianRasterizer(s)(
        means3D=t1["means3D"], means2D=t1["means2D"], opacities=t1["opacities"], shs=t1["shs"], scales=t1["scales"],
        rotations=t1["rotations"], aux_outputs=True)
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        (gC * img1).sum().backward()
        torch.cuda.synchronize()
        launched = _native.profile_stats()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    assert "render_bwd" in launched, launched
    assert not [k for k in AUX_KERNELS if k in launched], launched
    assert torch.equal(img1, img0) and torch.equal(radii1, radii0)
    assert inv1.shape == alpha1.shape == (1, cam.image_height, cam.image_width)
    for k in LEAVES:
        assert torch.equal(t1[k].grad, t0[k].grad), f"colour-only backward of an aux forward: d{k} differs"

    # alpha is 1 - final_T of the image buffer, as stored
    color, radii, inv, alpha, ex = _raw_aux(cam, leaves, deg, device)
    assert torch.equal(color, img0) and torch.equal(radii, radii0)
    assert torch.equal(alpha[0], 1.0 - ex["final_T"])
    assert torch.equal(alpha, alpha1.detach()) and torch.equal(inv, inv1.detach())
    none = ex["n_contrib"] == 0
    assert torch.equal(alpha[0][none], torch.zeros_like(alpha[0][none]))
    assert torch.equal(inv[0][none], torch.zeros_like(inv[0][none]))
    if name in ("sparse", "empty-tile"):
        assert none.float().mean() > 0.2
    if name == "empty-tile":  # a whole tile that nothing touches
        assert int((ex["ranges"][:, 1] == ex["ranges"][:, 0]).sum()) >= 1

    # two identical aux runs: identical outputs and gradients
    (oa, ta), (ob, tb) = (_hip(cam, leaves, deg, device, gC=gC, gD=gD, gA=gA) for _ in range(2))
    for a, b in zip(oa, ob):
        assert torch.equal(a, b)
    for k in LEAVES:
        assert torch.equal(ta[k].grad, tb[k].grad), f"d{k} differs run to run"
    assert torch.equal(oa[2].detach(), inv) and torch.equal(oa[3].detach(), alpha)


# ------------------------------------------------------------------------------------------
# 2. against the existing colour path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep", "opaque"])
def test_against_colour_path(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    gC, gD, gA = _weights(cam, device)
    _, _, inv, alpha, ex = _raw_aux(cam, leaves, deg, device)
    depth = ex["depth"]
    cols = torch.stack([1.0 / depth, torch.ones_like(depth), torch.zeros_like(depth)], 1).contiguous()
    (ref_img, _), _ = _hip(cam, leaves, deg, device, aux=False, colors=cols)
    ref_img = ref_img.detach()
    ref_inv, ref_alpha = ref_img[0].double(), ref_img[1].double()
    d_inv = (inv[0].double() - ref_inv).abs()
    print(f"\n[{name}] invdepth bit-equal to channel 0 at {int((inv[0] == ref_img[0]).sum())}/{inv[0].numel()} pixels, "
          f"max rel {float((d_inv / ref_inv.clamp_min(1e-300)).max()):.3e}")
    parity_report.record("invdepth vs colour path", inv[0].double().cpu().numpy(), ref_inv.cpu().numpy(), 1e-6, 0.0)
    assert bool((d_inv <= 1e-6 * ref_inv.abs()).all())
    n_max = int(ex["n_contrib"].max())
    d_alpha = float((alpha[0].double() - ref_alpha).abs().max())
    print(f"[{name}] alpha vs sum of weights: max|d| {d_alpha:.3e}, bound {2 * n_max * 2.0 ** -24:.3e} (n_max {n_max})")
    assert d_alpha <= 2 * n_max * 2.0 ** -24

    # gradients: the aux call against the sum of two plain renders
    _, t = _hip(cam, leaves, deg, device, gC=gC, gD=gD, gA=gA)
    view = cam.world_view_transform.to(device)

    def zcols(tt):
        z = tt["means3D"] @ view[:3, 2] + view[3, 2]
        return torch.stack([1.0 / z, torch.ones_like(z), torch.zeros_like(z)], 1)

    _, r = _hip(cam, leaves, deg, device, aux=False, gC=gC)
    gAD = torch.cat([gD, gA, torch.zeros_like(gD)], 0)
    _hip(cam, leaves, deg, device, aux=False, gC=gAD, colors=zcols, into=r)
    got, ref = _grads(t), _grads(r)
    for k in LEAVES:
        check_tol(got[k], ref[k], f"d{k} vs colour path", frac=5e-5 if k in CHAIN else RTOL, times=2)


# ------------------------------------------------------------------------------------------
# 3. against the fp64 dense reference
# ------------------------------------------------------------------------------------------
_DENSE = {}


def _dense(name, cam, leaves, deg, device, dtype):
    """render_local_aux on copies of the leaves in dtype (graph kept: one forward, several losses)."""
    key = (name, dtype)
    if key not in _DENSE:
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
        res = dense_ref_aux.render_local_aux(
            t["means3D"], t["means2D"], t["opacities"], *dense_cases.dense_args(cam, device, dtype),
            torch.zeros(3, dtype=dtype, device=device), shs=t["shs"], deg=deg, scales=t["scales"], rots=t["rotations"])
        _DENSE[key] = (t, res)
    return _DENSE[key]


_DENSE_GRADS = {}


def _dense_grads(key, t, outs, ws):
    """Autograd gradients of the loss's terms of sum w . out (ws: all three weights) through the kept
    dense graph; computed once per key (the
    dense side does not depend on the kernels' numerics mode).  The gradient is linear in the
    weights, so the loss on all three outputs is the sum of the colour-only and the aux-only ones
    (one backward pass through the 8000-step graph less)."""
    name, loss, dtype, mask = key
    if loss == "all":
        parts = [_dense_grads((name, l, dtype, mask), t, outs, ws) for l in ("colour", "aux")]
        return {k: parts[0][k] + parts[1][k] for k in LEAVES}
    if key not in _DENSE_GRADS:
        total = sum((w.to(o.dtype) * o).sum() for w, o, u in zip(ws, outs, LOSSES[loss]) if u)
        g = torch.autograd.grad(total, [t[k] for k in LEAVES], retain_graph=True, allow_unused=True)
        _DENSE_GRADS[key] = {k: (torch.zeros_like(t[k]) if v is None else v) for k, v in zip(LEAVES, g)}
    return _DENSE_GRADS[key]


SCENE_SEED = {"sparse": 41, "opaque": 49, "empty-tile": 41}
LOSSES = {"aux": (False, True, True), "colour": (True, False, False), "all": (True, True, True)}


@pytest.mark.parametrize("loss", ["aux", "colour", "all"])
@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_against_dense_fp64(device, mode, name, loss):
    from diff_gaussian_rasterization import GaussianRasterizer

    cam, leaves, deg = dense_cases.scene(name, device)
    W, H, P = cam.image_width, cam.image_height, leaves["means3D"].shape[0]
    ref, (rimg, rradii, flag, rinv, ralpha) = _dense(name, cam, leaves, deg, device, torch.float64)
    r32, (img32, _, _, inv32, alpha32) = _dense(name, cam, leaves, deg, device, torch.float32)

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    hip = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    img, radii, inv, alpha = GaussianRasterizer(s)(
        means3D=hip["means3D"], means2D=hip["means2D"], opacities=hip["opacities"], shs=hip["shs"],
        scales=hip["scales"], rotations=hip["rotations"], aux_outputs=True)

    rdiff = (radii.cpu() != rradii.cpu()).numpy()
    assert rdiff.mean() <= 1e-3, f"{int(rdiff.sum())} radii differ"
    fl = flag.cpu().numpy().copy()
    dense_cases.wide_mask(dense_cases.rect_and_radii(cam, leaves, deg, device)[0], rdiff, W, H, into=fl)
    print(f"\n[dense aux {name}/{loss}] flagged pixels {int(fl.sum())}/{fl.size}, radii differing {int(rdiff.sum())}/{P}")
    assert fl.mean() <= 0.02
    keep_px = torch.from_numpy(~fl).to(device)
    # the harness's draw, dl_dimage(seed = the scene's seed + 1), for the colour; the next two seeds for gD, gA
    full = [w * keep_px[None] for w in _weights(cam, device, seed=SCENE_SEED[name] + 1)]
    ws = [w if u else None for w, u in zip(full, LOSSES[loss])]
    sum((w * o).sum() for w, o in zip(ws, (img, inv, alpha)) if w is not None).backward()
    torch.cuda.synchronize()
    mask = fl.tobytes()
    g_ref = _dense_grads((name, loss, torch.float64, mask), ref, (rimg, rinv, ralpha), full)
    g_32 = _dense_grads((name, loss, torch.float32, mask), r32, (img32, inv32, alpha32), full)
    got = _grads(hip)
    keep_g = ~rdiff

    tag = f"{name}/{loss}"
    check_tol(img.permute(1, 2, 0), rimg.permute(1, 2, 0), f"image [{tag}]", ~fl)
    check_4x(inv[0], rinv[0], inv32[0], f"invdepth [{tag}]", ~fl)
    check_4x(alpha[0], ralpha[0], alpha32[0], f"alpha [{tag}]", ~fl)
    for k in LEAVES:
        check_4x(got[k], g_ref[k], g_32[k], f"d{k} [{tag}]", keep_g, enforce=k in CHAIN)
        check_tol(got[k], g_ref[k], f"d{k} [{tag}]", keep_g, frac=5e-5 if k in CHAIN else RTOL)


# ------------------------------------------------------------------------------------------
# 4. interface
# ------------------------------------------------------------------------------------------
def _tiny_call(device, t, **kw):
    from diff_gaussian_rasterization import GaussianRasterizer

    cam, _, deg = dense_cases.scene("empty-tile", device)
    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    return GaussianRasterizer(s)(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"],
                                 scales=t["scales"], rotations=t["rotations"], **kw)


def _tiny_leaves(device):
    _, leaves, _ = dense_cases.scene("empty-tile", device)
    return {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}


def test_refused_combinations(device, mode):
    from diff_gaussian_rasterization import register_gradient_sink, unregister_gradient_sink

    t = _tiny_leaves(device)
    with pytest.raises(RuntimeError, match="aux_outputs.*prepared"):
        _tiny_call(device, t, aux_outputs=True, prepared=object())
    with pytest.raises(RuntimeError, match="aux_outputs.*binning_capacity"):
        _tiny_call(device, t, aux_outputs=True, binning_capacity=4096)

    class Deferrer:  # what GradBucket(defer=True) and gs_train_step's fused backward + Adam owner look like
        defers = True

        def claim(self, p):
            raise AssertionError("no gradient may be claimed")

        def defer_view(self, *a):
            raise AssertionError("the view must not be deferred")

    owner = Deferrer()
    params = [t[k] for k in ("means3D", "opacities", "shs", "scales", "rotations")]
    for p in params:
        register_gradient_sink(p, owner)
    try:
        _, _, inv, alpha = _tiny_call(device, t, aux_outputs=True)
        with pytest.raises(RuntimeError, match="aux_outputs.*deferring"):
            (inv.sum() + alpha.sum()).backward()
    finally:
        for p in params:
            unregister_gradient_sink(p)


def test_accumulating_sink(device, mode):
    """An owner that hands out (buffer, True): the buffer ends as before + grad, the depth chain's
    term included.  opacity: one fp32 old + new, exact.  means3D: (before + g) + g_depth against
    before + (g + g_depth): three roundings at the operands' magnitude, 4 * 2^-24 (max|before| +
    max|grad|) (the depth term of this scene is smaller than the total)."""
    from diff_gaussian_rasterization import register_gradient_sink, unregister_gradient_sink

    cam, _, _ = dense_cases.scene("empty-tile", device)
    gC, gD, gA = _weights(cam, device)
    t0 = _tiny_leaves(device)
    out = _tiny_call(device, t0, aux_outputs=True)
    (gC * out[0]).sum().add((gD * out[2]).sum()).add((gA * out[3]).sum()).backward()
    torch.cuda.synchronize()
    assert float(t0["means3D"].grad.abs().max()) > 0

    g = torch.Generator(device="cpu").manual_seed(3)
    t = _tiny_leaves(device)
    before = {k: torch.randn(t[k].shape, generator=g).to(device) for k in ("means3D", "opacities")}
    bufs = {k: v.clone() for k, v in before.items()}

    class Owner:
        def claim(self, p):
            for k in bufs:
                if p is t[k]:
                    return bufs[k], True
            return None

    owner = Owner()
    for k in bufs:
        register_gradient_sink(t[k], owner)
    try:
        out = _tiny_call(device, t, aux_outputs=True)
        (gC * out[0]).sum().add((gD * out[2]).sum()).add((gA * out[3]).sum()).backward()
        torch.cuda.synchronize()
    finally:
        for k in bufs:
            unregister_gradient_sink(t[k])
    assert t["means3D"].grad is None and t["opacities"].grad is None  # sunk
    assert torch.equal(bufs["opacities"], before["opacities"] + t0["opacities"].grad)
    want = before["means3D"] + t0["means3D"].grad
    tol = 4 * 2.0 ** -24 * float(before["means3D"].abs().max() + t0["means3D"].grad.abs().max())
    assert float((bufs["means3D"] - want).abs().max()) <= tol
    for k in ("shs", "scales", "rotations", "means2D"):
        assert torch.equal(t[k].grad, t0[k].grad)


def test_empty_scene_returns_zeros(device, mode):
    from diff_gaussian_rasterization import GaussianRasterizer

    cam, leaves, deg = dense_cases.scene("empty-tile", device)
    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    e = {k: v[:0].contiguous() for k, v in leaves.items()}
    img, radii, inv, alpha = GaussianRasterizer(s)(
        means3D=e["means3D"], means2D=e["means2D"], opacities=e["opacities"], shs=e["shs"], scales=e["scales"],
        rotations=e["rotations"], aux_outputs=True)
    H, W = cam.image_height, cam.image_width
    assert img.shape == (3, H, W) and radii.numel() == 0 and inv.shape == alpha.shape == (1, H, W)
    assert not img.any() and not inv.any() and not alpha.any()


def test_single_aux_gradients(device, mode):
    """dL/dalpha only and dL/dinvdepth only both run, and (linearity) add up to the run with both,
    within twice _check's bounds (two fp32 orders)."""
    cam, leaves, deg = dense_cases.scene("sparse", device)
    _, gD, gA = _weights(cam, device)
    _, ta = _hip(cam, leaves, deg, device, gA=gA)
    _, td = _hip(cam, leaves, deg, device, gD=gD)
    _, tb = _hip(cam, leaves, deg, device, gD=gD, gA=gA)
    ga, gd, gb = _grads(ta), _grads(td), _grads(tb)
    assert float(ga["opacities"].abs().max()) > 0 and float(gd["means3D"].abs().max()) > 0
    assert not ga["shs"].any() and not gd["shs"].any()
    for k in LEAVES:
        check_tol(ga[k] + gd[k], gb[k], f"d{k} alpha-only + invdepth-only", frac=5e-5 if k in CHAIN else RTOL, times=2)
