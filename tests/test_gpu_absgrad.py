"""Absolute screen-space gradients (GaussianRasterizer(...)(..., absgrad=True),
gs_backward_accumulate_absgrad) on the GPU.

The scenes are tests/test_gpu_contrib.py's, built the same way through gs_scenes.identity_camera(200, 120)
(not a multiple of the 16-px tile either way, so edge tiles have lanes outside the image):

    sparse      random_gaussians(2000, 3, seed=41): one staged batch per tile
    deep        random_gaussians(6000, 1, seed=47, scale_range=(0.01, 0.08)): two or three batches (the
                deferred record store across batches)
    opaque      random_gaussians(8000, 1, seed=49, scale_range=(0.02, 0.12)), opacities 0.5 + 0.49 o:
                T-stopped pixels, up to five batches
    empty-tile  the first 3 Gaussians of `sparse` at 72 x 40: tiles with n_eff == 0

Every check runs in both numerics modes (gs_set_exact_exp), with and without aux gradients, so the four
walk instantiations, both record sums and the output kernel are launched in this process
(tests/test_zz_kernel_coverage.py).

1. Bit identities: .absgrad run to run; every other output with and without absgrad (plain, aux,
   camera calls); the autograd path against a raw gs_backward_accumulate_absgrad call whose scratch was
   prefilled with 0xFF bytes; a NULL output against gs_backward_accumulate(_aux), outputs and launch
   names; the exact zeros.
2. Triangle inequality against the existing path: absgrad[:, k] >= |grad[:, k]| - (2e-5 |grad| + 2e-5 max|grad|),
   twice test_gpu_dense._check's bound (two summation orders of the same terms, the rule of
   test_gpu_contrib.test_wsum_against_the_colour_gradient).
3. One-signed terms: 12 isolated splats over bg = 0 with a non-negative dL/dimage zeroed on one side of
   each splat's gradient half-plane: every term has one sign and absgrad equals |grad| under the rule of 2.
4. Symmetric cancellation: one isotropic splat on the optical axis under a uniform dL/dimage:
   |grad| <= count 2^-23 absgrad (count fp32 roundings of non-negative terms), x and y agree, absgrad > 0.
5. Against the fp64 dense reference (dense_ref_absgrad.absgrad_local, flag_rel=1e-3, flag_T_rel=1e-2;
   dL/dimage zeroed at flagged pixels and in the widened rectangles of Gaussians whose radius differs):
   max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|f64| per column.
6. Antialiasing: absgrad of antialiasing=True equals that of the plain call fed op s, rule of 2; in exact
   mode image, radii and lists bit-equal.
7. Training: add_densification_stats(absgrad=True) and train_step(absgrad=True); the refusals.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import dense_cases
import dense_ref_aa
import dense_ref_absgrad
import gpu_checks
import gs_scenes
from gpu_checks import RTOL, check_4x, check_tol, mode  # noqa: F401

pytestmark = pytest.mark.gpu

def _dpix(cam, device, seed=5):
    """a random signed dL/dimage of unit scale"""
    return gs_scenes.dl_dimage(cam.image_height, cam.image_width, seed=seed, scale=1.0).to(device)


def _aux_grads(cam, device, seed=6):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((1, cam.image_height, cam.image_width), generator=g).to(device) for _ in range(2))


GRADS = ("means3D", "means2D", "colour", "opacities", "scales", "rotations")


def _run(cam, leaves, deg, device, dpix, absgrad, aux_grads=None, aux=False, camera=False, antialiasing=False,
         colors=None, bg=None):
    """One forward + backward through GaussianRasterizer.  -> dict(img, radii, grads (GRADS order), absgrad or
    None, invdepth / alpha, cam (gV, gP, gC))."""
    from diff_gaussian_rasterization import GaussianRasterizer

    s = gs_scenes.raster_settings_for(cam, deg, device=device, bg=bg)
    if camera:
        s = s._replace(viewmatrix=s.viewmatrix.clone().requires_grad_(True),
                       projmatrix=s.projmatrix.clone().requires_grad_(True),
                       campos=s.campos.clone().requires_grad_(True))
    t = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items() if k != "shs"}
    col = (leaves["shs"] if colors is None else colors).detach().clone().requires_grad_(True)
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], scales=t["scales"],
              rotations=t["rotations"], **({"shs": col} if colors is None else {"colors_precomp": col}))
    more = {}
    if absgrad:
        more["absgrad"] = True
    if aux or aux_grads is not None:
        more["aux_outputs"] = True
    if camera:
        more["camera_grads"] = True
    if antialiasing:
        more["antialiasing"] = True
    out = GaussianRasterizer(s)(**kw, **more)
    loss = (out[0] * dpix).sum()
    if aux_grads is not None:
        loss = loss + (out[2] * aux_grads[0]).sum() + (out[3] * aux_grads[1]).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = dict(img=out[0].detach(), radii=out[1], m2=m2,
               grads=[t["means3D"].grad, m2.grad, col.grad, t["opacities"].grad, t["scales"].grad, t["rotations"].grad],
               absgrad=getattr(m2, "absgrad", None))
    if len(out) > 2:
        res["invdepth"], res["alpha"] = out[2].detach(), out[3].detach()
    if camera:
        res["cam"] = (s.viewmatrix.grad, s.projmatrix.grad, s.campos.grad)
    return res


def _same(a, b, what):
    for k in ("img", "radii", "invdepth", "alpha"):
        if k in a or k in b:
            assert torch.equal(a[k], b[k]), f"{what}: {k}"
    for n, u, v in zip(GRADS, a["grads"], b["grads"]):
        assert u is not None and torch.equal(u, v), f"{what}: dL/d{n}"
    if "cam" in a or "cam" in b:
        for n, u, v in zip(("view", "proj", "campos"), a["cam"], b["cam"]):
            assert u is not None and torch.equal(u, v), f"{what}: dL/d{n}"


# ---- the raw entries, with the caller's own scratch ----
def _forward_raw(cam, leaves, deg, device, aux=False):
    from diff_gaussian_rasterization import _C

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    e = torch.Tensor([])
    fn = _C.rasterize_gaussians_aux if aux else _C.rasterize_gaussians_two_call
    with torch.no_grad():
        out = fn(s.bg, leaves["means3D"], e, leaves["opacities"], leaves["scales"], leaves["rotations"],
                 s.scale_modifier, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width,
                 leaves["shs"], s.sh_degree, s.campos, s.prefiltered, s.debug)
    return s, out


def _names():
    from diff_gaussian_rasterization import _native

    return set(_native.profile_stats())


def _backward_raw(entry, s, leaves, fwd, dpix, aux_grads, device, want_abs=True, fill=None):
    """gs_backward_accumulate / _aux / _absgrad over ctypes with this function's own scratch (`fill`: its bytes
    before the call).  -> (the eight gradients, absgrad or None, the launch names)."""
    from diff_gaussian_rasterization import _C

    lib = gpu_checks.lib()
    R, _, radii, geom, binning, img = fwd[:6]
    P, M = leaves["means3D"].shape[0], leaves["shs"].shape[1]
    H, W = s.image_height, s.image_width
    Rl = _C.binning_layout_count(R, binning, W, H)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    f32 = dict(dtype=torch.float32, device=device)
    shapes = [(P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4)]
    # (dL/dcolors: SH colours; dL/dcov3D is written whenever it is passed)
    outs = [torch.full(sh, float("nan"), **f32) for sh in shapes]
    outs[1] = None
    n = {"gs_backward_accumulate": lib.gs_grad_buffer_bytes(Rl), "gs_backward_accumulate_aux":
         lib.gs_grad_buffer_bytes_aux(Rl, P), "gs_backward_accumulate_absgrad":
         lib.gs_grad_buffer_bytes_absgrad(Rl, P) if want_abs else (
             lib.gs_grad_buffer_bytes_aux(Rl, P) if aux_grads is not None else lib.gs_grad_buffer_bytes(Rl))}[entry]
    scratch = torch.full((n,), 0 if fill is None else fill, dtype=torch.uint8, device=device)
    ab = torch.full((P, 3), float("nan"), **f32) if want_abs and entry.endswith("absgrad") else None
    head = (P, s.sh_degree, M, p(s.bg), W, H, p(leaves["means3D"]), p(leaves["shs"]))
    mid = (p(leaves["opacities"]), p(leaves["scales"]), float(s.scale_modifier), p(leaves["rotations"]), None,
           p(s.viewmatrix), p(s.projmatrix), p(s.campos), float(s.tanfovx), float(s.tanfovy), p(radii), p(geom), int(Rl),
           p(binning), p(img), p(dpix))
    d_inv, d_alpha = (None, None) if aux_grads is None else aux_grads
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    tail = (*[p(o) for o in outs], 0, None, 0, st)
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        if entry == "gs_backward_accumulate":
            rc = lib.gs_backward_accumulate(*head, None, *mid, p(scratch), *tail)
        elif entry == "gs_backward_accumulate_aux":
            rc = lib.gs_backward_accumulate_aux(*head, None, None, *mid, p(d_inv), p(d_alpha), p(scratch), *tail)
        else:
            rc = lib.gs_backward_accumulate_absgrad(*head, None, None, *mid, p(d_inv), p(d_alpha), p(scratch), *tail, 0,
                                                    p(ab))
        assert rc == 0, lib.gs_last_error().decode()
        torch.cuda.synchronize()
        names = _names()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    return outs, ab, names


# ------------------------------------------------------------------------------------------
# 1. bit identities
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_bit_identities(device, mode, name):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    dpix, ag = _dpix(cam, device), _aux_grads(cam, device)

    # run to run, and a second backward of one graph
    a, b = _run(cam, leaves, deg, device, dpix, True), _run(cam, leaves, deg, device, dpix, True)
    assert a["absgrad"].shape == (P, 3) and a["absgrad"].dtype == torch.float32 and a["absgrad"].device == device
    assert torch.equal(a["absgrad"], b["absgrad"])
    plain = _run(cam, leaves, deg, device, dpix, False)
    assert plain["absgrad"] is None
    _same(a, plain, "absgrad vs plain")
    # aux outputs, with both aux gradients and with the colour's only
    for g in (ag, None):
        x = _run(cam, leaves, deg, device, dpix, True, aux_grads=g, aux=True)
        y = _run(cam, leaves, deg, device, dpix, False, aux_grads=g, aux=True)
        _same(x, y, f"aux (aux gradients: {g is not None})")
        assert torch.equal(x["absgrad"], _run(cam, leaves, deg, device, dpix, True, aux_grads=g, aux=True)["absgrad"])
        if g is None:
            assert torch.equal(x["absgrad"], a["absgrad"])  # no aux gradient: the plain walk's sums
        else:
            assert not torch.equal(x["absgrad"], a["absgrad"])
            a_aux = x
    # camera gradients, with and without aux gradients
    for g in (None, ag):
        x = _run(cam, leaves, deg, device, dpix, True, aux_grads=g, camera=True)
        y = _run(cam, leaves, deg, device, dpix, False, aux_grads=g, camera=True)
        _same(x, y, f"camera (aux gradients: {g is not None})")
        assert torch.equal(x["absgrad"], (a if g is None else a_aux)["absgrad"])

    # the raw entry with a scratch of 0xFF bytes; a NULL output against the entries it extends
    for g, ref, plain_entry, walk in ((None, a, "gs_backward_accumulate", "render_bwd"),
                                      (ag, a_aux, "gs_backward_accumulate_aux", "render_bwd_aux")):
        s, fwd = _forward_raw(cam, leaves, deg, device, aux=g is not None)
        gf = None if g is None else tuple(t.contiguous() for t in g)
        outs, ab, names = _backward_raw("gs_backward_accumulate_absgrad", s, leaves, fwd, dpix, gf, device, fill=0xFF)
        assert torch.equal(ab, ref["absgrad"]), "raw call over a 0xFF scratch vs autograd"
        sfx = "_aux" if g is not None else ""
        if fwd[0] > 0:
            assert {f"render_bwd{sfx}_abs", f"sum_records{sfx}_abs", "mean2d_absgrad"} <= names
            assert not {"render_bwd", "render_bwd_aux", "sum_records", "sum_records_aux"} & names
        outs0, ab0, names0 = _backward_raw("gs_backward_accumulate_absgrad", s, leaves, fwd, dpix, gf, device,
                                           want_abs=False, fill=0xFF)
        outs1, _, names1 = _backward_raw(plain_entry, s, leaves, fwd, dpix, gf, device, fill=0xFF)
        assert ab0 is None and names0 == names1 and not any(n.endswith("absgrad") or n.endswith("_abs") for n in names0)
        for k, (u, v, w) in enumerate(zip(outs0, outs1, outs)):
            if u is not None:
                assert not torch.isnan(u).any() and torch.equal(u, v) and torch.equal(u, w), f"gradient {k}"
        # the lists, final_T and n_contrib are the forward's: untouched by either backward
        ex = _C.debug_export(P, W, H, fwd[0], fwd[3], fwd[4], fwd[5], device)
        _backward_raw("gs_backward_accumulate_absgrad", s, leaves, fwd, dpix, gf, device)
        ex2 = _C.debug_export(P, W, H, fwd[0], fwd[3], fwd[4], fwd[5], device)
        for k in ("final_T", "n_contrib", "point_list", "ranges"):
            assert torch.equal(ex[k], ex2[k]), k
    if name == "empty-tile":
        assert int((ex["ranges"][:, 1] == ex["ranges"][:, 0]).sum()) >= 1

    # the exact zeros
    for r in (a, a_aux):
        ab = r["absgrad"]
        assert not ab[r["radii"] == 0].any() and not ab[:, 2].any()
        assert bool((ab >= 0).all()) and float(ab.max()) > 0 and bool(torch.isfinite(ab).all())
    z = _run(cam, leaves, deg, device, torch.zeros_like(dpix), True)
    assert not z["absgrad"].any()
    z = _run(cam, leaves, deg, device, torch.zeros_like(dpix), True, aux_grads=tuple(torch.zeros_like(t) for t in ag))
    assert not z["absgrad"].any()
    none = _run(cam, {k: v[:0].contiguous() for k, v in leaves.items()}, deg, device, dpix, True)
    assert none["absgrad"].shape == (0, 3)


# ------------------------------------------------------------------------------------------
# 2. the triangle inequality against the existing path
# ------------------------------------------------------------------------------------------
def _tol2(ref):
    """twice test_gpu_dense._check's bound: 2 (1e-5 |ref| + 1e-5 max|ref|)"""
    ref = np.abs(ref)
    return 2 * (RTOL * ref + RTOL * float(ref.max(initial=0.0)))


def _check_ge(ab, grad, name):
    ab, g = ab.detach().double().cpu().numpy()[:, :2], np.abs(grad.detach().double().cpu().numpy()[:, :2])
    for k in range(2):
        tol = _tol2(g[:, k])
        short = g[:, k] - ab[:, k]
        print(f"{name}[{k}]: max(|grad| - absgrad) {short.max(initial=0.0):.3e}  max|grad| {g[:, k].max():.3e}  "
              f"sum absgrad / sum |grad| {ab[:, k].sum() / g[:, k].sum():.3f}  "
              f"({float((short / np.maximum(tol, 1e-300)).max(initial=0.0)):.3f} of the bound)")
        assert np.all(short <= tol), f"{name}[{k}]: {int((short > tol).sum())} below |grad| - tol"


@pytest.mark.parametrize("name", ["sparse", "deep", "opaque"])
def test_triangle_inequality(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    print()
    r = _run(cam, leaves, deg, device, _dpix(cam, device), True)
    _check_ge(r["absgrad"], r["grads"][1], f"[{name}]")
    vis = r["radii"] > 0
    assert float((r["absgrad"][vis][:, :2].sum(0) / r["grads"][1][vis][:, :2].abs().sum(0)).min()) > 1.05
    r = _run(cam, leaves, deg, device, _dpix(cam, device), True, aux_grads=_aux_grads(cam, device))
    _check_ge(r["absgrad"], r["grads"][1], f"[{name}, aux gradients]")


# ------------------------------------------------------------------------------------------
# 3. one-signed terms equal the signed gradient
# ------------------------------------------------------------------------------------------
def _grid_scene(device):
    """12 splats on a 4 x 3 grid at depth 5, about 2.5 px wide, random orientations"""
    cam = gs_scenes.identity_camera(200, 120)
    W, H = 200, 120
    fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
    g = torch.Generator().manual_seed(31)
    z = 5.0
    px = torch.tensor([25.0, 75.0, 125.0, 175.0]).repeat(3) + (torch.rand(12, generator=g) - 0.5)
    py = torch.tensor([20.0, 60.0, 100.0]).repeat_interleave(4) + (torch.rand(12, generator=g) - 0.5)
    means = torch.stack([(px + 0.5 - W / 2) * z / fx, (py + 0.5 - H / 2) * z / fy, torch.full((12,), z)], 1)
    scales = (1.4 + 1.0 * torch.rand((12, 3), generator=g)) * z / fx
    rots = torch.nn.functional.normalize(torch.randn((12, 4), generator=g), dim=1)
    leaves = dict(means3D=means, opacities=0.3 + 0.6 * torch.rand((12, 1), generator=g), scales=scales, rotations=rots,
                  shs=torch.zeros((12, 1, 3)))
    cols = 0.2 + 0.8 * torch.rand((12, 3), generator=g)
    return cam, {k: v.float().contiguous().to(device) for k, v in leaves.items()}, cols.to(device)


def test_one_signed_terms_equal_the_signed_gradient(device, mode):
    cam, leaves, cols = _grid_scene(device)
    H, W = cam.image_height, cam.image_width
    hp = dense_ref_absgrad.half_planes(leaves["means3D"], torch.zeros_like(leaves["means3D"]), leaves["opacities"],
                                       *dense_cases.dense_args(cam, device, torch.float32), colors=cols,
                                       scales=leaves["scales"],
                                       rots=leaves["rotations"])
    assert not hp["overlap"], "the splats' tile rectangles must not overlap"
    assert int((hp["radii"] > 0).sum()) == 12
    m = (0.25 + torch.rand((H, W), generator=torch.Generator().manual_seed(33))).to(device)
    print()
    for k, side in enumerate(("x", "y")):
        assert 0.1 < float(hp[side].float().mean()) < 0.9
        dpix = (m * hp[side]).expand(3, H, W).contiguous()
        r = _run(cam, leaves, 0, device, dpix, True, colors=cols, bg=torch.zeros(3, device=device))
        assert torch.equal(r["radii"].cpu(), hp["radii"].cpu())
        ab, gr = r["absgrad"][:, k], r["grads"][1][:, k]
        assert float(gr.abs().min()) > 0
        check_tol(ab, gr.abs(), f"one-signed {side}: absgrad vs |grad|", times=2)
        # (the other column's terms change sign inside the half-plane: it stays a strict bound somewhere)
        _check_ge(r["absgrad"], r["grads"][1], f"one-signed {side}")


# ------------------------------------------------------------------------------------------
# 4. symmetric cancellation
# ------------------------------------------------------------------------------------------
def test_symmetric_cancellation(device, mode):
    import gs_importance
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = gs_scenes.identity_camera(200, 120)
    H, W = cam.image_height, cam.image_width
    fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
    assert abs(fx - fy) <= 1e-9 * fx  # square pixels: an isotropic splat on the axis is isotropic on screen
    z = 5.0
    leaves = dict(means3D=torch.tensor([[0.0, 0.0, z]]), opacities=torch.tensor([[0.3]]),
                  scales=torch.full((1, 3), 6.0 * z / fx), rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]),
                  shs=torch.zeros((1, 1, 3)))
    leaves = {k: v.to(device) for k, v in leaves.items()}
    cols = torch.tensor([[0.7, 0.4, 0.9]], device=device)
    dpix = torch.ones((3, H, W), device=device)
    r = _run(cam, leaves, 0, device, dpix, True, colors=cols, bg=torch.zeros(3, device=device))
    st = gs_importance.view_contributions(
        GaussianRasterizer(gs_scenes.raster_settings_for(cam, 0, device=device, bg=torch.zeros(3, device=device))),
        means3D=leaves["means3D"], opacities=leaves["opacities"], colors_precomp=cols, scales=leaves["scales"],
        rotations=leaves["rotations"])
    count = int(st.count[0])
    ab, gr = r["absgrad"][0, :2].double(), r["grads"][1][0, :2].double()
    bound = count * 2.0 ** -23 * ab
    ux, uy = float(ab[0]) / (0.5 * W), float(ab[1]) / (0.5 * H)
    print(f"\ncount {count}  absgrad {ab.tolist()}  grad {gr.tolist()}  bound {bound.tolist()}  "
          f"|ux - uy| {abs(ux - uy):.3e} (bound {count * 2.0 ** -23 * max(ux, uy):.3e})")
    assert count > 300 and int(r["radii"][0]) > 10
    assert bool((ab > 0).all())
    assert bool((gr.abs() <= bound).all())
    assert abs(ux - uy) <= count * 2.0 ** -23 * max(ux, uy)


# ------------------------------------------------------------------------------------------
# 5. against the fp64 dense reference
# ------------------------------------------------------------------------------------------
_DENSE = {}


def _dense(cam, leaves, deg, device, dt, dpix, ag, **flags):
    t = {k: v.detach().to(dt) for k, v in leaves.items()}
    bg = torch.zeros(3, dtype=dt, device=device)
    return dense_ref_absgrad.absgrad_local(
        t["means3D"], t["means2D"], t["opacities"], *dense_cases.dense_args(cam, device, dt), bg, dpix.to(dt),
        shs=t["shs"], deg=deg, scales=t["scales"], rots=t["rotations"],
        dL_dalpha=None if ag is None else ag[1].to(dt), dL_dinvdepth=None if ag is None else ag[0].to(dt), **flags)


def _dense_case(key, cam, leaves, deg, device, hip_radii, dpix, ag):
    """dL/dimage zeroed at the flagged pixels and the fp64 / fp32 dense sums under it; independent of the
    kernels' numerics mode: computed once per scene and set of differing radii."""
    c = _DENSE.setdefault(key, {})
    if "probe" not in c:
        # (radii and rectangles do not depend on the gradient)
        c["rect"], c["radii"] = dense_cases.rect_and_radii(cam, leaves, deg, device)
        c["probe"] = True
    rdiff = (hip_radii.cpu() != c["radii"]).numpy()
    wide = dense_cases.wide_mask(c["rect"], rdiff, cam.image_width, cam.image_height)
    if "wide" not in c or not np.array_equal(c["wide"], wide):
        c["wide"] = wide
        c["f64"] = _dense(cam, leaves, deg, device, torch.float64, dpix, ag, flag_rel=1e-3, flag_T_rel=1e-2,
                          zero_flagged=True, also_flag=torch.from_numpy(wide))
        keep = c["f64"]["keep"]
        c["dpix"] = (dpix * keep).contiguous()
        c["ag"] = None if ag is None else tuple((t * keep).contiguous() for t in ag)
        c["f32"] = _dense(cam, leaves, deg, device, torch.float32, c["dpix"], c["ag"])
    fl = ~c["f64"]["keep"].cpu().numpy()
    return c["dpix"], c["ag"], fl, rdiff, c["f64"], c["f32"]


@pytest.mark.parametrize("name,aux", [("sparse", False), ("deep", False), ("opaque", False), ("sparse", True)])
def test_against_dense_fp64(device, mode, name, aux):
    cam, leaves, deg = dense_cases.scene(name, device)
    P = leaves["means3D"].shape[0]
    dpix0, ag0 = _dpix(cam, device, seed=17), (_aux_grads(cam, device, seed=18) if aux else None)
    radii = _run(cam, leaves, deg, device, dpix0, False)["radii"]
    dpix, ag, fl, rdiff, r64, r32 = _dense_case((name, aux), cam, leaves, deg, device, radii, dpix0, ag0)
    print(f"\n[{name}{', aux gradients' if aux else ''}] flagged pixels {int(fl.sum())}/{fl.size} ({fl.mean():.4f}), "
          f"radii differing {int(rdiff.sum())}/{P}")
    assert fl.mean() <= 0.02
    assert not rdiff.any(), f"{int(rdiff.sum())} radii differ"
    r = _run(cam, leaves, deg, device, dpix, True, aux_grads=ag)
    keep = ~rdiff
    for k in range(2):
        assert float(r64["abs"][:, k][torch.from_numpy(keep)].abs().max()) > 0
        check_4x(r["absgrad"][:, k], r64["abs"][:, k], r32["abs"][:, k], f"[{name}{'+aux' if aux else ''}] absgrad[{k}]",
                 keep)
    assert not r["absgrad"][:, 2].any()


# ------------------------------------------------------------------------------------------
# 6. antialiasing
# ------------------------------------------------------------------------------------------
def test_antialiasing_equals_the_plain_call_with_the_compensated_opacities(device, mode):
    from diff_gaussian_rasterization import _C

    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    dpix = _dpix(cam, device)
    s = dense_ref_aa.aa_scale(leaves["means3D"], cam.world_view_transform.to(device), math.tan(cam.FoVx / 2),
                              math.tan(cam.FoVy / 2), W, H, scales=leaves["scales"], rots=leaves["rotations"])
    assert float(s.min()) < 0.9 and float(s.max()) < 1.0
    aa = _run(cam, leaves, deg, device, dpix, True, antialiasing=True)
    _same(aa, _run(cam, leaves, deg, device, dpix, False, antialiasing=True), "antialiased: absgrad vs without")
    off = _run(cam, leaves, deg, device, dpix, True)
    assert not torch.equal(aa["absgrad"], off["absgrad"])
    eff = (leaves["opacities"] * s[:, None]).contiguous()
    if mode == 1:
        # the kernels' own op s (the splat record's opacity; a culled Gaussian keeps its input): bit-equal
        # image, radii and lists, as tests/test_gpu_aa.py has it
        st = gs_scenes.raster_settings_for(cam, deg, device=device)
        e = torch.Tensor([])
        args = lambda op: (st.bg, leaves["means3D"], e, op, leaves["scales"], leaves["rotations"],  # noqa: E731
                           st.scale_modifier, e, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, H, W, leaves["shs"],
                           st.sh_degree, st.campos, st.prefiltered, st.debug)
        with torch.no_grad():
            oa = _C.rasterize_gaussians_aa(*args(leaves["opacities"]))
            ex_a = _C.debug_export(P, W, H, oa[0], oa[3], oa[4], oa[5], device)
            eff = torch.where(oa[2][:, None] > 0, ex_a["conic_opacity"][:, 3:4], leaves["opacities"]).contiguous()
            op = _C.rasterize_gaussians(*args(eff))
            ex_p = _C.debug_export(P, W, H, op[0], op[3], op[4], op[5], device)
        assert torch.equal(oa[1], op[1]) and torch.equal(oa[2], op[2])
        for k in ("tiles_touched", "point_list", "final_T", "n_contrib"):
            assert torch.equal(ex_a[k], ex_p[k]), k
    plain = _run(cam, dict(leaves, opacities=eff), deg, device, dpix, True)
    assert torch.equal(aa["radii"], plain["radii"])
    print()
    for k in range(2):
        check_tol(aa["absgrad"][:, k], plain["absgrad"][:, k], f"antialiased absgrad[{k}] vs compensated opacities", times=2)


# ------------------------------------------------------------------------------------------
# 7. training, and the refusals
# ------------------------------------------------------------------------------------------
def _train_setup(device):
    cam = gs_scenes.identity_camera(200, 120)
    sc = gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41)
    settings = gs_scenes.raster_settings_for(cam, 3, device=device)
    gt = torch.rand((3, 120, 200), generator=torch.Generator().manual_seed(9)).to(device)
    return sc, settings, gt


def _snapshot(m):
    out = []
    for grp in m.optimizer.param_groups:
        p = grp["params"][0]
        st = m.optimizer.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out


def test_add_densification_stats(device, mode):
    import gs_train

    cam, leaves, deg = dense_cases.scene("sparse", device)
    P = leaves["means3D"].shape[0]
    r = _run(cam, leaves, deg, device, _dpix(cam, device), True)

    class Stats:
        def __init__(self):
            g = torch.Generator().manual_seed(3)
            self.max_radii2D = torch.rand((P,), generator=g).to(device)
            self.xyz_gradient_accum = torch.rand((P, 1), generator=g).to(device)
            self.denom = torch.rand((P, 1), generator=g).to(device)

    a, b, c = Stats(), Stats(), Stats()
    gs_train.add_densification_stats(a, r["m2"], r["radii"], absgrad=True)
    gs_train.densify_stats(b.max_radii2D, b.xyz_gradient_accum, b.denom, r["radii"], r["absgrad"])
    gs_train.add_densification_stats(c, r["m2"], r["radii"])
    torch.cuda.synchronize()
    for n in ("max_radii2D", "xyz_gradient_accum", "denom"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert torch.equal(a.max_radii2D, c.max_radii2D) and torch.equal(a.denom, c.denom)
    assert not torch.equal(a.xyz_gradient_accum, c.xyz_gradient_accum)
    with pytest.raises(RuntimeError, match="has no .absgrad"):
        gs_train.add_densification_stats(a, torch.zeros((P, 3), device=device, requires_grad=True), r["radii"],
                                         absgrad=True)


@pytest.mark.parametrize("sky", [False, True], ids=["plain", "sky"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "glue"])
def test_train_step(device, mode, sky, fused):
    import gs_sky
    import gs_train_step as ts

    sc, settings, gt = _train_setup(device)
    kw = dict(sky=True) if sky else {}
    models, losses = [], []
    for absgrad in (False, True):
        m = ts.TrainModel(sc, device, fused=fused)
        if sky:
            sp = gs_sky.SkySphere(16, 32).to(device)
            with torch.no_grad():
                sp.texture.copy_(torch.rand((3, 16, 32), generator=torch.Generator().manual_seed(21)).to(device))
            m.attach_sky(sp)
        losses.append([ts.train_step(m, settings, gt, fused=fused, loss_item=True, **kw,
                                     **({"absgrad": True} if absgrad else {})) for _ in range(2)])
        models.append(m)
    torch.cuda.synchronize()
    a, b = models
    assert losses[0] == losses[1]
    for k, (u, v) in enumerate(zip(_snapshot(a), _snapshot(b))):
        assert torch.equal(u, v), f"parameter / moment {k}"
    if sky:
        assert torch.equal(a.sky.texture, b.sky.texture)
    assert torch.equal(a.denom, b.denom) and torch.equal(a.max_radii2D, b.max_radii2D)
    assert float(a.denom.max()) == 2.0
    # the rule of 2. on the accumulated norms
    sa, sb = (x.xyz_gradient_accum.double().cpu().numpy()[:, 0] for x in (a, b))
    tol = _tol2(sa)
    print(f"\nsum accum: signed {sa.sum():.6e}  absgrad {sb.sum():.6e}  max(signed - abs) {(sa - sb).max():.3e}")
    assert np.all(sb >= sa - tol) and sb.sum() > 1.05 * sa.sum()


def test_train_step_refusals(device):
    import gs_train_step as ts

    sc, settings, gt = _train_setup(device)
    m = ts.TrainModel(sc, device, fused=True)
    params = lambda: [grp["params"][0].detach().clone() for grp in m.optimizer.param_groups]  # noqa: E731
    before = params()
    with pytest.raises(ValueError, match="absgrad= is not supported with fuse_adam=True"):
        ts.train_step(m, settings, gt, absgrad=True, fuse_adam=True)
    with pytest.raises(ValueError, match=r"absgrad= is not supported with a bounded forward \(binning_capacity=\)"):
        ts.train_step(m, settings, gt, absgrad=True, binning_capacity=1 << 16)
    for u, v in zip(before, params()):
        assert torch.equal(u, v)


def test_autograd_refusals(device):
    import gs_view_parallel
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    cam, leaves, deg = dense_cases.scene("sparse", device)
    r = GaussianRasterizer(gs_scenes.raster_settings_for(cam, deg, device=device))
    kw = dict(means3D=leaves["means3D"], opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
              rotations=leaves["rotations"])
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    with pytest.raises(RuntimeError, match="absgrad: means2D does not require grad"):
        r(means2D=torch.zeros_like(leaves["means3D"]), absgrad=True, **kw)
    with pytest.raises(RuntimeError, match="absgrad: not supported with binning_capacity="):
        r(means2D=m2, absgrad=True, binning_capacity=1 << 16, **kw)
    (pv,) = prepare_views([r], leaves["means3D"], leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                          rotations=leaves["rotations"])
    with pytest.raises(RuntimeError, match="absgrad: not supported with prepared="):
        r(means2D=m2, absgrad=True, prepared=pv, **kw)
    # a deferring gradient owner
    t = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    bucket = gs_view_parallel.GradBucket([t["means3D"], t["shs"], t["opacities"], t["scales"], t["rotations"]],
                                         defer=True)
    try:
        img, _ = r(means2D=m2, absgrad=True, **{k: t[k] for k in kw})
        with pytest.raises(RuntimeError, match=r"absgrad: not supported with a deferring gradient owner"):
            img.sum().backward()
    finally:
        bucket.close()
    torch.cuda.synchronize()
    # sh_split= composes: bit-equal to the concatenated rows
    dpix = _dpix(cam, device)
    whole = _run(cam, leaves, deg, device, dpix, True)
    dc, rest = leaves["shs"][:, :1].contiguous(), leaves["shs"][:, 1:].contiguous()
    carrier = torch.empty_like(leaves["shs"]).requires_grad_(True)
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    img, _ = r(means2D=m2, absgrad=True, sh_split=(dc, rest), **dict(kw, shs=carrier))
    (img * dpix).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(m2.absgrad, whole["absgrad"]) and torch.equal(carrier.grad, whole["grads"][2])
