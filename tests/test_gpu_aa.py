"""GPU tests of antialiasing (GaussianRasterizer(...)(..., antialiasing=True)): the opacity of every
splat scaled by s = sqrt(max(0.000025, det S / det(S + 0.3 I))) where it enters the splat record and
the culling limit, and the backward's chain through s.

  1. off is off: antialiasing=False is the call without the keyword, bits and launches;
  2. the render path is untouched: the antialiased call equals the plain call fed the effective
     opacities, bit for bit, and its opacity gradient is s times that call's;
  3. against the fp64 dense reference (tests/dense_ref.py fed opac * dense_ref_aa.aa_scale, autograd
     carrying the chain) by the method of tests/test_gpu_dense.py, every degree and both covariance
     sources; 4. the same with the aux outputs; 5. the camera gradients, view / proj / campos leaves of
     aa_scale too;
  6. what it is for: a sub-pixel splat keeps its energy;  7. the refusals, and a splat scaled below 1/255.

Bound of 3-5 (the project's conditioning rule, measured against the reference only):
max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|f64| for the image and every gradient.  Pixels
where a decision sits at its threshold are flagged by the reference and left out (dL/dimage zeroed
there), Gaussians whose fp32 radius differs are left out of the gradient checks, and so are Gaussians
whose fp64 ratio r lies within 1e-3 (relative) of the floor 2.5e-5, where fp32 may take the other
branch of the chain gradient.  The counts are bounded: 2 %, 0.1 %, 1 %."""
import math

import pytest
import torch

import dense_cases
import dense_ref
import dense_ref_aa
import dense_ref_aux
import gpu_checks
import gs_scenes
from gpu_checks import check_4x, exact_mode  # noqa: F401

pytestmark = pytest.mark.gpu

EYE, TARGET = (0.7, -0.4, -1.1), (0.1, 0.2, 4.0)


def _cov6(d):
    R = dense_ref.quat_R(d.rotations)
    L = R * d.scales[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


_SCENES = {}


def _scene(name, device):
    """dict(cam, leaves, deg, bg, mod, seed)"""
    if name in _SCENES:
        return _SCENES[name]
    mod, bg = 1.0, torch.zeros(3)
    sh = lambda d: {k: getattr(d, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}  # noqa: E731
    if name == "a":
        cam, deg, seed = gs_scenes.identity_camera(192, 128), 3, 41
        leaves = sh(gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41))
    elif name == "b":
        cam, deg, seed = gs_scenes.identity_camera(160, 96), 1, 47
        leaves = sh(gs_scenes.random_gaussians(3000, 1, cam=cam, seed=47, scale_range=(0.001, 0.012)))
    elif name == "c":  # the floor: most splats sit at s = 0.005, some of them still render
        cam, deg, seed = gs_scenes.identity_camera(96, 64), 0, 48
        leaves = sh(gs_scenes.random_gaussians(1500, 0, cam=cam, seed=48, scale_range=(0.0003, 0.003)))
    elif name == "d":  # precomputed colours and covariances, a coloured background
        cam, deg, seed, P = gs_scenes.identity_camera(128, 80), 0, 44, 1000
        d = gs_scenes.random_gaussians(P, 0, cam=cam, seed=44, scale_range=(0.002, 0.03))
        leaves = dict(means3D=d.means3D, opacities=d.opacities,
                      colors=torch.rand((P, 3), generator=torch.Generator().manual_seed(45)), cov3D=_cov6(d))
        bg = torch.tensor([0.1, 0.2, 0.3])
    elif name == "e":
        cam, deg, seed, mod = gs_scenes.identity_camera(128, 80), 2, 46, 0.7
        leaves = sh(gs_scenes.random_gaussians(1000, 2, cam=cam, seed=46, scale_range=(0.002, 0.03)))
    elif name.startswith("cam"):  # cam0 .. cam3: SH degree; camc: precomputed colours
        cam, seed = gs_scenes.look_at_camera(EYE, TARGET, 96, 64), 61
        deg = 0 if name == "camc" else int(name[3])
        d = gs_scenes.random_gaussians(300, deg, cam=cam, seed=61, scale_range=(0.002, 0.03))
        leaves = sh(d)
        if name == "camc":
            del leaves["shs"]
            leaves["colors"] = torch.rand((300, 3), generator=torch.Generator().manual_seed(62))
    elif name == "off":
        cam, deg, seed = gs_scenes.identity_camera(96, 64), 1, 49
        leaves = sh(gs_scenes.random_gaussians(500, 1, cam=cam, seed=49))
    else:
        raise KeyError(name)
    leaves = {k: v.to(device) for k, v in leaves.items()}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"])
    _SCENES[name] = dict(cam=cam, leaves=leaves, deg=deg, bg=bg.to(device), mod=mod, seed=seed)
    return _SCENES[name]


def _fresh(leaves):
    return {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}


def _settings(sc, device, cam_leaves=False):
    s = gs_scenes.raster_settings_for(sc["cam"], sc["deg"], bg=sc["bg"], scale_modifier=sc["mod"], device=device)
    cams = None
    if cam_leaves:
        cams = [t.detach().clone().contiguous().requires_grad_(True) for t in (s.viewmatrix, s.projmatrix, s.campos)]
        s = s._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
    return s, cams


def _call(s, t, **kw):
    from diff_gaussian_rasterization import GaussianRasterizer

    args = {"shs": t.get("shs"), "colors_precomp": t.get("colors"), "scales": t.get("scales"),
            "rotations": t.get("rotations"), "cov3D_precomp": t.get("cov3D")}
    return GaussianRasterizer(s)(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"],
                                 **{k: v for k, v in args.items() if v is not None}, **kw)


def _raw_args(s, t):
    """The nineteen arguments of _C.rasterize_gaussians for leaves `t`."""
    e = torch.Tensor([])
    g = lambda k: t[k].detach() if k in t else e  # noqa: E731
    return (s.bg, g("means3D"), g("colors"), g("opacities"), g("scales"), g("rotations"), s.scale_modifier, g("cov3D"),
            s.viewmatrix.contiguous(), s.projmatrix.contiguous(), s.tanfovx, s.tanfovy, s.image_height, s.image_width,
            g("shs"), s.sh_degree, s.campos, s.prefiltered, s.debug)


def _weights(sc, device, aux=False):
    H, W, seed = sc["cam"].image_height, sc["cam"].image_width, sc["seed"]
    ws = [gs_scenes.dl_dimage(H, W, seed=seed + 1, scale=1.0).to(device)]
    if aux:
        ws += [gs_scenes.dl_dimage(H, W, seed=seed + 2, scale=1.0)[:1].contiguous().to(device),
               gs_scenes.dl_dimage(H, W, seed=seed + 3, scale=1.0)[1:2].contiguous().to(device)]
    return ws


# ---- the dense side: one forward per (scene, dtype, aux) ----
_DENSE = {}


def _dense(name, sc, dtype, device, aux=False):
    """(leaves, camera leaves, outputs, radii, flag map, r): the dense reference fed opac * s."""
    key = (name, dtype, aux)
    if key not in _DENSE:
        cam = sc["cam"]
        W, H = cam.image_width, cam.image_height
        tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sc["leaves"].items()}
        cams = [x.to(device, dtype).contiguous().clone().requires_grad_(True)
                for x in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
        s, r = dense_ref_aa.aa_scale(t["means3D"], cams[0], tx, ty, W, H, scales=t.get("scales"),
                                     rots=t.get("rotations"), cov3D=t.get("cov3D"), mod=sc["mod"], with_ratio=True)
        assert s.dtype == dtype
        fn = dense_ref_aux.render_local_aux if aux else dense_ref.render_local
        res = fn(t["means3D"], t["means2D"], t["opacities"] * s[:, None], cams[0], cams[1], cams[2], tx, ty, W, H,
                 sc["bg"].to(dtype), shs=t.get("shs"), deg=sc["deg"], colors=t.get("colors"), scales=t.get("scales"),
                 rots=t.get("rotations"), cov3D=t.get("cov3D"), mod=sc["mod"])
        outs = (res[0], res[3], res[4]) if aux else (res[0],)
        _DENSE[key] = (t, cams, outs, res[1], res[2], r.detach())
    return _DENSE[key]


def _masks(name, sc, device, radii, aux=False):
    """test_gpu_dense's harness plus the floor: -> (flag map, Gaussians kept in the gradient checks)."""
    cam = sc["cam"]
    W, H = cam.image_width, cam.image_height
    ref, rcams, _, rradii, flag, r = _dense(name, sc, torch.float64, device, aux)
    P = radii.numel()
    rdiff = (radii.cpu() != rradii.cpu()).numpy()
    near_floor = ((r - dense_ref_aa.AA_FLOOR).abs() <= 1e-3 * dense_ref_aa.AA_FLOOR).cpu().numpy()
    fl = flag.cpu().numpy().copy()
    if rdiff.any():
        with torch.no_grad():
            q = dense_ref._prep(ref["means3D"], ref["means2D"], ref["opacities"], rcams[0], rcams[1], rcams[2],
                                math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H, shs=ref.get("shs"),
                                deg=sc["deg"], colors=ref.get("colors"), scales=ref.get("scales"),
                                rots=ref.get("rotations"), cov3D=ref.get("cov3D"), mod=sc["mod"])
        dense_cases.wide_mask(q["rect"].numpy(), rdiff, W, H, into=fl)
    at_floor = int((r <= dense_ref_aa.AA_FLOOR).sum())
    print(f"\n[aa {name}] flagged pixels {int(fl.sum())}/{fl.size}, radii differing {int(rdiff.sum())}/{P}, "
          f"near the floor {int(near_floor.sum())}/{P}, at s = 0.005 {at_floor}/{P}, visible {int((radii > 0).sum())}")
    assert fl.mean() <= 0.02 and rdiff.mean() <= 1e-3 and near_floor.mean() <= 0.01
    return fl, ~rdiff & ~near_floor


def _against_dense(name, device, aux=False, cam_leaves=False):
    sc = _scene(name, device)
    s, cams = _settings(sc, device, cam_leaves)
    t = _fresh(sc["leaves"])
    out = _call(s, t, antialiasing=True, aux_outputs=aux, camera_grads=cam_leaves)
    outs, radii = ((out[0], out[2], out[3]) if aux else (out[0],)), out[1]
    assert int((radii > 0).sum()) > 0
    fl, keep_g = _masks(name, sc, device, radii, aux)
    keep_px = torch.from_numpy(~fl).to(device)
    ws = [w * keep_px[None] for w in _weights(sc, device, aux)]
    sum((w * o).sum() for w, o in zip(ws, outs)).backward()
    torch.cuda.synchronize()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        rt, rcams, routs, _, _, _ = _dense(name, sc, dtype, device, aux)
        for x in list(rt.values()) + rcams:
            x.grad = None
        sum((w.to(dtype) * o).sum() for w, o in zip(ws, routs)).backward(retain_graph=True)
        runs[dtype] = (rt, rcams, routs)
    (r64, c64, o64), (r32, c32, o32) = runs[torch.float64], runs[torch.float32]
    for k, nm in enumerate(("image", "invdepth", "alpha")[:len(outs)]):
        check_4x(outs[k].permute(1, 2, 0), o64[k].permute(1, 2, 0), o32[k].permute(1, 2, 0), f"{nm} [aa {name}]", ~fl)
    zero = lambda x: torch.zeros_like(x) if x.grad is None else x.grad  # noqa: E731
    for k in t:
        check_4x(zero(t[k]), zero(r64[k]), zero(r32[k]), f"d{k} [aa {name}]", keep_g)
    assert float(zero(r64["opacities"]).abs().max()) > 0
    return sc, t, cams, (c64, c32), zero


# ------------------------------------------------------------------------------------------
# 1. off is off
# ------------------------------------------------------------------------------------------
def test_off_is_off(device):
    from diff_gaussian_rasterization import _native

    sc = _scene("off", device)
    s, _ = _settings(sc, device)
    w = _weights(sc, device)[0]
    lib = gpu_checks.lib()

    def run(**kw):
        t = _fresh(sc["leaves"])
        torch.cuda.synchronize()
        lib.gs_profile_collect()
        lib.gs_profile_reset()
        lib.gs_profile_enable(1)
        try:
            img, radii = _call(s, t, **kw)
            (img * w).sum().backward()
            torch.cuda.synchronize()
            launched = _native.profile_stats()
        finally:
            lib.gs_profile_enable(0)
            lib.gs_profile_reset()
        return img, radii, t, {k: v[1] for k, v in launched.items()}

    i0, r0, t0, l0 = run()
    i1, r1, t1, l1 = run(antialiasing=False)
    assert torch.equal(i0, i1) and torch.equal(r0, r1)
    for k in t0:
        assert torch.equal(t0[k].grad, t1[k].grad), k
    assert l0 == l1 and "preprocess" in l0 and "preprocess_bwd" in l0, (l0, l1)
    # and on is on: another image, the same radii
    i2, r2, _, l2 = run(antialiasing=True)
    assert "preprocess" in l2 and "preprocess_bwd" in l2 and torch.equal(r2, r0) and not torch.equal(i2, i0)


# ------------------------------------------------------------------------------------------
# 2. the render path is untouched
# ------------------------------------------------------------------------------------------
def test_equals_the_plain_call_with_the_effective_opacities(device, exact_mode):
    from diff_gaussian_rasterization import _C

    cam = gs_scenes.identity_camera(192, 128)
    d = gs_scenes.random_gaussians(2000, 3, cam, seed=41).to(device)
    leaves = {k: getattr(d, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    leaves["means2D"] = torch.zeros_like(d.means3D)
    sc = dict(cam=cam, leaves=leaves, deg=3, bg=torch.zeros(3, device=device), mod=1.0, seed=41)
    s, _ = _settings(sc, device)
    P, W, H = 2000, 192, 128
    w = _weights(sc, device)[0]

    def export(out):
        n, img, radii, geom, binning, imgb = out[:6]
        return img, radii, _C.debug_export(P, W, H, n, geom, binning, imgb, device)

    img_a, radii_a, ex_a = export(_C.rasterize_gaussians_aa(*_raw_args(s, leaves)))
    eff = torch.where(radii_a[:, None] > 0, ex_a["conic_opacity"][:, 3:4], leaves["opacities"]).contiguous()
    scale = (eff / leaves["opacities"])[:, 0]
    vis = radii_a > 0
    assert int(vis.sum()) > 100
    assert bool((scale[vis] < 1).all()) and bool((scale[vis] >= 0.005 * (1 - 1e-6)).all())
    assert float(scale[vis].min()) < 0.9  # some splats of this scene are really compensated
    img_p, radii_p, ex_p = export(_C.rasterize_gaussians(*_raw_args(s, dict(leaves, opacities=eff))))
    assert torch.equal(img_a, img_p) and torch.equal(radii_a, radii_p)
    for k in ("tiles_touched", "point_list", "final_T", "n_contrib"):
        assert torch.equal(ex_a[k], ex_p[k]), k
    for k in ("conic_opacity", "xy", "rgb", "depth"):  # (a culled Gaussian's record is not written)
        assert torch.equal(ex_a[k][vis], ex_p[k][vis]), k
    # radii do not depend on the opacity: the plain call with the original opacities has the same
    _, radii_o, _ = export(_C.rasterize_gaussians(*_raw_args(s, leaves)))
    assert torch.equal(radii_a, radii_o)
    # gradients, through the public call
    ta, tp = _fresh(leaves), _fresh(dict(leaves, opacities=eff))
    ia, ra = _call(s, ta, antialiasing=True)
    ip, rp = _call(s, tp)
    assert torch.equal(ia, img_a) and torch.equal(ip, img_a)
    (ia * w).sum().backward()
    (ip * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ta["means2D"].grad, tp["means2D"].grad) and torch.equal(ta["shs"].grad, tp["shs"].grad)
    ga, gp = ta["opacities"].grad[:, 0], tp["opacities"].grad[:, 0]
    assert float(gp.abs().max()) > 0
    # dL/dop = s dL/dop': one multiply here and one division in `scale`, 4 ulp
    assert torch.all((ga - scale * gp).abs() <= 1e-6 * (scale * gp).abs()), float((ga - scale * gp).abs().max())
    # the chain through s moves the geometry gradients
    assert not torch.equal(ta["scales"].grad, tp["scales"].grad)


# ------------------------------------------------------------------------------------------
# 3. against the fp64 reference, 4. with the aux outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"],
                         ids=["a_sh3", "b_sh1_small", "c_sh0_floor", "d_colors_cov3d", "e_sh2_mod0.7"])
def test_against_dense_fp64(device, name):
    sc, t, _, _, _ = _against_dense(name, device)
    if name == "c":
        r = _dense(name, sc, torch.float64, device)[5]
        assert int((r <= dense_ref_aa.AA_FLOOR).sum()) > 1000  # the floor is what this scene is about


def test_aux_outputs_against_dense_fp64(device):
    _against_dense("b", device, aux=True)


def test_aux_alpha_is_one_minus_final_T(device):
    from diff_gaussian_rasterization import _C

    sc = _scene("b", device)
    s, _ = _settings(sc, device)
    cam = sc["cam"]
    out = _C.rasterize_gaussians_aa(*_raw_args(s, sc["leaves"]), aux=True)
    ex = _C.debug_export(sc["leaves"]["means3D"].shape[0], cam.image_width, cam.image_height, out[0], out[3], out[4],
                         out[5], device)
    assert torch.equal(out[7][0], 1.0 - ex["final_T"]) and float(out[7].max()) > 0


# ------------------------------------------------------------------------------------------
# 5. camera gradients
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cam2", "cam0", "cam1", "cam3", "camc"])
def test_camera_gradients(device, name):
    sc, t, cams, (c64, c32), zero = _against_dense(name, device, cam_leaves=True)
    for k, nm in enumerate(("viewmatrix", "projmatrix", "campos")):
        check_4x(zero(cams[k]), zero(c64[k]), zero(c32[k]), f"d{nm} [aa {name}]")
    assert float(zero(c64[0]).abs().max()) > 0
    if name != "cam2":
        return
    # reproducible bit for bit, and the chain through s is really in dL/dviewmatrix
    ws = _weights(sc, device)

    def gV(**kw):
        s, cm = _settings(sc, device, True)
        img, _ = _call(s, _fresh(sc["leaves"]), camera_grads=True, **kw)
        (img * ws[0]).sum().backward()
        torch.cuda.synchronize()
        return cm[0].grad.clone()

    g1, g2, g0 = gV(antialiasing=True), gV(antialiasing=True), gV(antialiasing=False)
    assert torch.equal(g1, g2) and not torch.equal(g1, g0)


# ------------------------------------------------------------------------------------------
# 6. what it is for
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.013, -0.021)], ids=["centred", "shifted"])
@pytest.mark.parametrize("v", [0.1, 0.5, 4.0])
def test_a_small_splat_keeps_its_energy(device, v, shift):
    W = H = 64
    cam = gs_scenes.identity_camera(W, H)
    f = W / (2 * math.tan(cam.FoVx / 2))
    z, op = 4.0, 0.9
    var_w = v * (z / f) ** 2  # raw screen variance v px^2
    t = dict(means3D=torch.tensor([[shift[0], shift[1], z]], device=device),
             opacities=torch.tensor([[op]], device=device), colors=torch.ones((1, 3), device=device),
             cov3D=torch.tensor([[var_w, 0, 0, var_w, 0, var_w]], device=device))
    t["means2D"] = torch.zeros_like(t["means3D"])
    s = gs_scenes.raster_settings_for(cam, 0, bg=torch.zeros(3, device=device), device=device)
    with torch.no_grad():
        on = float(_call(s, t, antialiasing=True)[0][0].double().sum()) / (2 * math.pi * op * v)
        off = float(_call(s, t)[0][0].double().sum()) / (2 * math.pi * op * v)
    sc = v / (v + 0.3)
    print(f"\n[aa energy] v = {v}: sum / (2 pi op v) = {on:.4f} with antialiasing, {off:.4f} without")
    # the mass below the alpha threshold, the 3-sigma rectangle (1.1 %) and the sampling error
    assert abs(on - 1) <= (1 / 255) / (op * sc) + 0.03
    assert off > on and (v > 1 or off > 1.5)


# ------------------------------------------------------------------------------------------
# 7. refusals; a splat scaled below 1/255
# ------------------------------------------------------------------------------------------
class _Deferrer:
    defers = True

    def __init__(self):
        self.deferred = []

    def claim(self, t):
        return None

    def defer_view(self, ctx, inputs, view):
        self.deferred.append(view)


def test_refusals_on_the_gpu_path(device):
    from diff_gaussian_rasterization import prepare_views, register_gradient_sink, unregister_gradient_sink, GaussianRasterizer

    sc = _scene("off", device)
    s, _ = _settings(sc, device)
    t = _fresh(sc["leaves"])
    prepared = prepare_views([GaussianRasterizer(s)], t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"],
                             rotations=t["rotations"])[0]
    split = (t["shs"][:, :1].detach().contiguous(), t["shs"][:, 1:].detach().contiguous())
    for name, value in (("prepared", prepared), ("binning_capacity", 100000), ("sh_split", split)):
        with pytest.raises(RuntimeError) as e:
            _call(s, t, antialiasing=True, **{name: value})
        assert str(e.value) == f"antialiasing: not supported with {name}="
    _call(s, t, prepared=prepared)  # untouched by the refusal: still usable, once
    owner = _Deferrer()
    params = [v for k, v in t.items() if k != "means2D"]
    for p in params:
        register_gradient_sink(p, owner)
    try:
        img, _ = _call(s, t, antialiasing=True)
        with pytest.raises(RuntimeError) as e:
            img.sum().backward()
        assert str(e.value) == ("antialiasing: not supported with a deferring gradient owner (GradBucket(defer=True), "
                                "the fused backward + Adam of gs_train_step)")
        assert not owner.deferred
    finally:
        for p in params:
            unregister_gradient_sink(p)
    torch.cuda.synchronize()


def test_a_splat_scaled_below_the_alpha_threshold(device):
    """op' = 0.5 * 0.005 < 1/255: visible to upstream's rule (radii > 0), no instances, zero gradients."""
    W = H = 64
    cam = gs_scenes.identity_camera(W, H)
    f = W / (2 * math.tan(cam.FoVx / 2))
    var = [4.0 * (4.0 / f) ** 2, 1e-4 * (4.0 / f) ** 2]  # 4 px^2, and far below a pixel: s = 0.005
    t = dict(means3D=torch.tensor([[-0.5, 0.1, 4.0], [0.4, -0.2, 4.0]], device=device),
             opacities=torch.tensor([[0.9], [0.5]], device=device),
             colors=torch.tensor([[1.0, 0.5, 0.2], [0.3, 0.6, 0.9]], device=device),
             cov3D=torch.tensor([[u, 0, 0, u, 0, u] for u in var], device=device))
    t["means2D"] = torch.zeros_like(t["means3D"])
    t = _fresh(t)
    s = gs_scenes.raster_settings_for(cam, 0, bg=torch.zeros(3, device=device), device=device)
    img, radii = _call(s, t, antialiasing=True)
    img0, radii0 = _call(s, _fresh(t))
    assert bool((radii > 0).all()) and torch.equal(radii, radii0)
    (img * gs_scenes.dl_dimage(H, W, seed=3, scale=1.0).to(device)).sum().backward()
    torch.cuda.synchronize()
    for k, v in t.items():
        assert not v.grad[1].any(), k
        if k != "means2D":
            assert v.grad[0].any(), k
    # the plain call draws the second splat (0.5 at its centre), the antialiased one does not
    px, py = int(round((0.4 / 4.0) * f + 31.5)), int(round((-0.2 / 4.0) * f + 31.5))
    assert float(img0.detach()[:, py, px].max()) > 0.1 and not img.detach()[:, py - 2:py + 3, px - 2:px + 3].any()
