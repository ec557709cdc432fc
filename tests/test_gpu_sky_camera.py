"""The skysphere's view-matrix gradient (gs_sky.compose(..., camera_grads=True), k_sky_bwd<true> +
k_sky_cam_finish, C ABI gs_sky_compose_backward_camera) on the GPU against tests/sky_pose_ref.py.

Shapes: cases A-D of tests/test_gpu_sky.py with its seeded inputs (edge blocks with lanes outside the
image, the pole and the clamped rows, the seam and both scatter paths, a texture far finer than the
image), a 1 x 1 image with a 1 x 1 texture and a 17 x 1 image with a 4 x 8 texture.

Every comparison with the reference zeroes dL/dimage at the reference's flagged pixels
(sky_pose_ref.flagged: a texel boundary within eps, or next to a pole); at most 2 % of a case's pixels
may be flagged.

1. dL/dviewmatrix against fp64 autograd, with alpha given and None, with the texture gradient on and
   off: max|hip - f64| <= 4 max|ref f32 - f64| + 1e-5 max|f64| over the 3 x 3 block (the project's
   conditioning rule; ref f32 is the same reference in fp32 on the CPU).
2. Bit identities: camera_grads changes nothing else, run to run, autograd = ABI, accumulate_view,
   the view gradient alone.
3. Exact zeros.  4. Non-finite dL/dimage.  5. Interface.
6. Additivity of the rasterizer's and the sky's shares through render_with_sky(camera_grads=True).
7. dL/ddelta of a gs_pose.CameraTwist through splats + sky against the dense reference chain.
8. A rotation recovered from a bare sky by Adam on CameraTwist.delta.
"""
import ctypes
import math

import pytest
import torch

import gs_scenes
from gpu_checks import check_4x
import sky_pose_ref
from test_gpu_sky import CASES, _Recorder, _bits, _inputs

pytestmark = pytest.mark.gpu

TINY = {
    "one": (lambda: gs_scenes.identity_camera(1, 1), 1, 1),
    "row17": (lambda: gs_scenes.identity_camera(17, 1), 4, 8),
}


def _tiny_inputs(name, device):
    """(settings, alpha [H, W], texture, g) of a TINY shape, seeded"""
    make_cam, Hs, Ws = TINY[name]
    cam = make_cam()
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(99)
    alpha, tex, g = torch.rand((H, W), generator=gen), torch.rand((3, Hs, Ws), generator=gen), torch.randn((3, H, W), generator=gen)
    return (gs_scenes.raster_settings_for(cam, 0, device=device),) + tuple(t.to(device) for t in (alpha, tex, g))


def _hip(s, alpha, tex, g, camera_grads=True, alpha_grad=True, tex_grad=True, view=None, color=None):
    """One compose + backward of sum g image with the view matrix as a leaf that requires grad.
    -> (image, alpha.grad, texture.grad, viewmatrix.grad)"""
    import gs_sky

    V = (s.viewmatrix if view is None else view).detach().clone().requires_grad_(True)
    a = None if alpha is None else alpha.detach().clone().requires_grad_(alpha_grad)
    t = tex.detach().clone().requires_grad_(tex_grad)
    img = gs_sky.compose(color, a, t, s._replace(viewmatrix=V), camera_grads=camera_grads)
    if img.requires_grad:
        (img * g).sum().backward()
    torch.cuda.synchronize()
    return img.detach(), None if a is None else a.grad, t.grad, V.grad


def _abi(s, alpha, tex, g, want_alpha=True, want_tex=True, want_view=True, accumulate_view=0, into=None):
    """gs_sky_compose_backward_camera called directly, outputs and scratches pre-filled with garbage.
    -> (dL/dalpha, dL/dtexture, dL/dviewmatrix)"""
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    H, W = int(s.image_height), int(s.image_width)
    Hs, Ws = tex.shape[1], tex.shape[2]
    dev = tex.device
    dalpha = torch.full((H, W), float("nan"), device=dev) if want_alpha else None
    dtex = torch.full_like(tex, float("nan")) if want_tex else None
    dview = (into if into is not None else torch.full((4, 4), float("nan"), device=dev)) if want_view else None
    scratch = (torch.empty((lib.gs_sky_scratch_bytes(Hs, Ws),), dtype=torch.uint8, device=dev).fill_(0xA5)
               if want_tex else None)
    cam_scratch = torch.empty((lib.gs_sky_camera_scratch_bytes(W, H),), dtype=torch.uint8, device=dev).fill_(0xA5)
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
    view = s.viewmatrix.detach().contiguous()
    _native.check(lib.gs_sky_compose_backward_camera(
        W, H, p(view), s.tanfovx, s.tanfovy, Hs, Ws, p(tex), p(alpha), p(g), p(dalpha), p(dtex), 0, p(scratch),
        p(dview), accumulate_view, p(cam_scratch), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
        "sky backward camera")
    torch.cuda.synchronize()
    return dalpha, dtex, dview


_MASKED = {}


def _masked(name, device):
    """(settings, alpha, texture, g zeroed at the flagged pixels) of a case; asserts the 2 % cap."""
    if name not in _MASKED:
        if name in CASES:
            s, _, alpha, tex, g = _inputs(name, device)
        else:
            s, alpha, tex, g = _tiny_inputs(name, device)
        fl = sky_pose_ref.flagged(s.viewmatrix, s.tanfovx, s.tanfovy, int(s.image_width), int(s.image_height),
                                  tex.shape[1], tex.shape[2])
        share = float(fl.double().mean())
        print(f"\n[sky camera {name}] flagged pixels {int(fl.sum())}/{fl.numel()} = {100 * share:.2f} %")
        assert share <= sky_pose_ref.FLAG_CAP
        _MASKED[name] = (s, alpha, tex, g * (~fl).to(device)[None])
    return _MASKED[name]


_REFS = {}


def _ref(name, with_alpha, device):
    """{dtype: dL/dviewmatrix} of the masked case from the torch reference on the CPU; built once."""
    key = (name, with_alpha)
    if key not in _REFS:
        s, alpha, tex, g = _masked(name, device)
        _REFS[key] = {dt: sky_pose_ref.view_grad(alpha if with_alpha else None, tex, g, s.viewmatrix, s.tanfovx,
                                                 s.tanfovy, dt) for dt in (torch.float64, torch.float32)}
    return _REFS[key]


def _zero_border(gv):
    z = torch.zeros(4, device=gv.device)
    return torch.equal(_bits(gv[3]), _bits(z)) and torch.equal(_bits(gv[:, 3]), _bits(z))


def _all_zero_bits(gv):
    return gv.shape == (4, 4) and not _bits(gv).any()


# ---- 1. against the fp64 reference ----
@pytest.mark.parametrize("tex_grad", [True, False], ids=["tex", "notex"])
@pytest.mark.parametrize("with_alpha", [True, False], ids=["alpha", "noalpha"])
@pytest.mark.parametrize("name", list(CASES) + ["row17"])
def test_matches_fp64_reference(name, with_alpha, tex_grad, device):
    s, alpha, tex, g = _masked(name, device)
    ref = _ref(name, with_alpha, device)
    _, _, dtex, gv = _hip(s, alpha if with_alpha else None, tex, g, tex_grad=tex_grad)
    assert gv is not None and gv.shape == (4, 4) and gv.dtype == torch.float32 and gv.device == tex.device
    assert (dtex is not None) == tex_grad
    assert _zero_border(gv)
    assert float(ref[torch.float64].abs().max()) > 0
    check_4x(gv[:3, :3], ref[torch.float64][:3, :3], ref[torch.float32][:3, :3],
             f"sky {name} dL_dviewmatrix [{'alpha' if with_alpha else 'no alpha'}, {'tex' if tex_grad else 'no tex'}]")


# ---- 2. bit identities ----
@pytest.mark.parametrize("name", list(CASES))
def test_bit_identities(name, device):
    s, color, alpha, tex, g = _inputs(name, device)
    img0, da0, dt0, gv0 = _hip(s, alpha, tex, g, camera_grads=False, color=color)
    img1, da1, dt1, gv1 = _hip(s, alpha, tex, g, color=color)
    assert gv0 is None, "the default call must leave the view matrix without a gradient"
    # camera_grads changes nothing else
    assert torch.equal(_bits(img0), _bits(img1)) and torch.equal(_bits(da0), _bits(da1))
    assert torch.equal(_bits(dt0), _bits(dt1))
    assert torch.isfinite(gv1).all() and float(gv1.abs().max()) > 0 and _zero_border(gv1)
    # run to run, and the autograd path against the direct call
    _, _, _, gv2 = _hip(s, alpha, tex, g, color=color)
    assert torch.equal(_bits(gv1), _bits(gv2))
    da3, dt3, gv3 = _abi(s, alpha, tex, g)
    assert torch.equal(_bits(gv1), _bits(gv3))
    assert torch.equal(_bits(da1), _bits(da3)) and torch.equal(_bits(dt1), _bits(dt3))
    # accumulate_view = 1: fp32 old + new
    pre = torch.randn((4, 4), generator=torch.Generator().manual_seed(5)).to(device)
    _, _, acc = _abi(s, alpha, tex, g, want_alpha=False, want_tex=False, accumulate_view=1, into=pre.clone())
    assert torch.equal(_bits(acc), _bits(pre + gv1))
    # the view gradient alone, through both paths, and with one of the other two
    assert torch.equal(_bits(_abi(s, alpha, tex, g, want_alpha=False, want_tex=False)[2]), _bits(gv1))
    assert torch.equal(_bits(_hip(s, alpha, tex, g, alpha_grad=False, tex_grad=False)[3]), _bits(gv1))
    assert torch.equal(_bits(_hip(s, alpha, tex, g, alpha_grad=False)[3]), _bits(gv1))
    assert torch.equal(_bits(_hip(s, alpha, tex, g, tex_grad=False)[3]), _bits(gv1))
    # NULL dL_dviewmatrix: gs_sky_compose_backward's bits
    da4, dt4, none = _abi(s, alpha, tex, g, want_view=False)
    assert none is None and torch.equal(_bits(da4), _bits(da0)) and torch.equal(_bits(dt4), _bits(dt0))


# ---- 3. exact zeros ----
def test_exact_zeros(device):
    s, color, alpha, tex, g = _inputs("C", device)
    assert _all_zero_bits(_hip(s, torch.ones_like(alpha), tex, g)[3]), "alpha == 1"
    assert _all_zero_bits(_hip(s, alpha, tex, torch.zeros_like(g))[3]), "g == 0"
    sb, _, alpha_b, tex_b, g_b = _inputs("B", device)
    for a in (alpha_b, None):
        assert _all_zero_bits(_hip(sb, a, torch.full_like(tex_b, 0.7310585975646973), g_b)[3]), "constant texture"
    # a degenerate matrix: every ray is 0; the call completes, finite
    img, da, dt, gv = _hip(s, alpha, tex, g, view=torch.zeros((4, 4), device=device))
    assert _all_zero_bits(gv), "zero view matrix"
    assert torch.isfinite(img).all() and torch.isfinite(da).all() and torch.isfinite(dt).all()
    # one texel: all four taps are the same
    s1, alpha1, tex1, g1 = _tiny_inputs("one", device)
    for a in (alpha1, None):
        assert _all_zero_bits(_hip(s1, a, tex1, g1)[3]), "1 x 1"
    assert _all_zero_bits(_abi(s1, alpha1, tex1, g1)[2])


# ---- 4. non-finite gradients ----
def test_non_finite_gradients_complete_and_repeat(device):
    """inf / NaN in dL/dimage: the values are meaningless, the run completes and repeats itself"""
    s, color, alpha, tex, g = _inputs("C", device)
    bad = g.clone()
    bad[0, 5, 7] = float("inf")
    bad[1, 60, 100] = float("nan")
    bad[2, 119, 199] = -float("inf")
    _, dt1, gv1 = _abi(s, alpha, tex, bad, want_alpha=False)
    _, dt2, gv2 = _abi(s, alpha, tex, bad, want_alpha=False)
    assert torch.equal(_bits(gv1), _bits(gv2)) and torch.equal(_bits(dt1), _bits(dt2))


# ---- 5. interface ----
def _launches(fn):
    """{launch name: count} of fn() by the library's profiler"""
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        stats = _native.profile_stats()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    return {k: v[1] for k, v in stats.items()}


def test_launches(device):
    import gs_sky

    s, color, alpha, tex, g = _inputs("A", device)

    def run(camera_grads, view_grad, alpha_grad=True, tex_grad=True):
        V = s.viewmatrix.detach().clone().requires_grad_(view_grad)
        a, t = alpha.clone().requires_grad_(alpha_grad), tex.clone().requires_grad_(tex_grad)
        (gs_sky.compose(color, a, t, s._replace(viewmatrix=V), camera_grads=camera_grads) * g).sum().backward()
        return V

    plain = _launches(lambda: run(False, False))
    assert plain == {"sky_fwd": 1, "sky_clear": 1, "sky_absmax": 1, "sky_bwd": 1, "sky_finish": 1}, plain
    # the flag without a matrix that requires grad: the plain call
    assert _launches(lambda: run(True, False)) == plain
    # a matrix that requires grad without the flag: the plain call, and no gradient
    out = {}
    assert _launches(lambda: out.setdefault("V", run(False, True))) == plain
    assert out["V"].grad is None
    both = _launches(lambda: out.setdefault("W", run(True, True)))
    assert both == {"sky_fwd": 1, "sky_clear": 1, "sky_absmax": 1, "sky_bwd_cam": 1, "sky_cam_finish": 1,
                    "sky_finish": 1}, both
    assert out["W"].grad is not None
    # the view gradient alone: nothing of the texture's scatter runs
    alone = _launches(lambda: run(True, True, alpha_grad=False, tex_grad=False))
    assert alone == {"sky_fwd": 1, "sky_bwd_cam": 1, "sky_cam_finish": 1}, alone


def test_view_matrix_errors_and_layouts(device):
    import gs_sky

    s, color, alpha, tex, g = _inputs("B", device)
    V = s.viewmatrix.detach()
    for bad in (V.double(), V[:3].clone(), V.cpu().clone()):
        bad = bad.requires_grad_(True)
        with pytest.raises(ValueError, match="gs_sky.compose: camera_grads needs"):
            gs_sky.compose(color, alpha, tex, s._replace(viewmatrix=bad), camera_grads=True)
    # a leaf stored transposed and a non-leaf: the gradient comes back in the tensor's logical layout
    want = _hip(s, alpha, tex, g)[3]
    vt = V.t().contiguous().t().detach().requires_grad_(True)
    assert vt.is_leaf and not vt.is_contiguous()
    (gs_sky.compose(color, alpha, tex, s._replace(viewmatrix=vt), camera_grads=True) * g).sum().backward()
    assert vt.grad.shape == (4, 4) and torch.equal(_bits(vt.grad), _bits(want))
    leaf = V.clone().requires_grad_(True)
    (gs_sky.compose(color, alpha, tex, s._replace(viewmatrix=leaf * 1.0), camera_grads=True) * g).sum().backward()
    assert torch.equal(_bits(leaf.grad), _bits(want))
    # SkySphere.render / forward hand the flag on
    sky = gs_sky.SkySphere(tex.shape[1], tex.shape[2]).to(device)
    with torch.no_grad():
        sky.texture.copy_(tex)
    for call in (lambda st: sky.render(st, camera_grads=True), lambda st: sky(None, None, st, camera_grads=True)):
        leaf = V.clone().requires_grad_(True)
        (call(s._replace(viewmatrix=leaf)) * g).sum().backward()
        assert torch.equal(_bits(leaf.grad), _bits(_hip(s, None, tex, g)[3]))
    leaf = V.clone().requires_grad_(True)
    (sky.render(s._replace(viewmatrix=leaf)) * g).sum().backward()
    assert leaf.grad is None


# ---- 6. additivity through render_with_sky ----
def _splats(device):
    """the sh2 scene of tests/test_gpu_camera.py (500 Gaussians, SH 2, a look-at camera at 192 x 128)"""
    import test_gpu_camera as cam_t

    return cam_t, cam_t._scene("sh2", device)


def _raster_inputs(t):
    return dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"],
                scales=t["scales"], rotations=t["rotations"])


def test_render_with_sky_adds_the_two_shares(device):
    import gs_sky
    from diff_gaussian_rasterization import GaussianRasterizer

    cam_t, sc = _splats(device)
    H, W = sc["cam"].image_height, sc["cam"].image_width
    g = gs_scenes.dl_dimage(H, W, seed=77, scale=1.0).to(device)
    sky = gs_sky.SkySphere(32, 64).to(device)
    with torch.no_grad():
        sky.texture.copy_(_inputs("A", device)[3])
    s, cams = cam_t._settings(sc, device)
    rec = _Recorder(GaussianRasterizer(s))
    image, radii, invdepth, alpha = gs_sky.render_with_sky(rec, sky, camera_grads=True,
                                                           **_raster_inputs(cam_t._fresh(sc["leaves"])))
    assert bool((alpha == 0).any()) and bool((alpha > 0.5).any()), "the scene must show bare sky and splats"
    (image * g).sum().backward()
    torch.cuda.synchronize()
    # the rasterizer's share: the aux call fed the dL/dcolor and dL/dalpha the sky's backward produced
    s_r, cams_r = cam_t._settings(sc, device)
    out = GaussianRasterizer(s_r)(**_raster_inputs(cam_t._fresh(sc["leaves"])), aux_outputs=True, camera_grads=True)
    torch.autograd.backward([out[0], out[3]], [rec.color.grad, rec.alpha.grad])
    # the sky's share: compose on the detached colour and alpha
    s_s, cams_s = cam_t._settings(sc, device, req=(True, False, False))
    tex_grad_before = sky.texture.grad.clone()
    (gs_sky.compose(rec.color.detach(), rec.alpha.detach(), sky.texture, s_s, camera_grads=True) * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(sky.texture.grad), _bits(tex_grad_before + tex_grad_before))
    for c in cams_r + cams_s[:1]:
        assert c.grad is not None and float(c.grad.abs().max()) > 0
    assert torch.equal(_bits(cams[0].grad), _bits(cams_r[0].grad + cams_s[0].grad))
    assert not torch.equal(cams[0].grad, cams_r[0].grad)
    assert torch.equal(_bits(cams[1].grad), _bits(cams_r[1].grad))
    assert torch.equal(_bits(cams[2].grad), _bits(cams_r[2].grad))
    # without the flag nothing reaches the camera tensors
    s_n, cams_n = cam_t._settings(sc, device)
    img_n = gs_sky.render_with_sky(GaussianRasterizer(s_n), sky, **_raster_inputs(cam_t._fresh(sc["leaves"])))[0]
    assert torch.equal(_bits(img_n), _bits(image))
    (img_n * g).sum().backward()
    assert all(c.grad is None for c in cams_n)
    # the rasterizer's refusals surface unchanged
    with pytest.raises(RuntimeError, match="camera_grads:.*prepared"):
        gs_sky.render_with_sky(GaussianRasterizer(s), sky, camera_grads=True, prepared=object(),
                               **_raster_inputs(cam_t._fresh(sc["leaves"])))


# ---- 7. end to end: a twist of the pose through splats and sky ----
def test_end_to_end_twist_with_sky(device):
    """dL/ddelta at delta = 0 through CameraTwist + render_with_sky(camera_grads=True) against the same
    chain in fp64 behind dense_ref_aux.render_local_aux and sky_pose_ref (one view matrix feeds both);
    the fp32 side of the rule is the chain in fp32.  dL/dimage is zeroed at the rasterizer's flagged
    pixels and at the sky's.  A sky at infinity does not see the translation: its three components
    are those of a run whose sky takes no camera gradient, bit for bit."""
    import gs_pose
    import gs_sky
    from diff_gaussian_rasterization import GaussianRasterizer

    cam_t, sc0 = _splats(device)
    sc = dict(sc0, aux=True)
    name = "sh2 aux+sky"  # this file's entries in test_gpu_camera's caches of the dense runs
    cam = sc["cam"]
    H, W = cam.image_height, cam.image_width
    tfx, tfy = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    tex = _inputs("A", device)[3]
    sky = gs_sky.SkySphere(tex.shape[1], tex.shape[2]).to(device)
    with torch.no_grad():
        sky.texture.copy_(tex)
    base = gs_scenes.raster_settings_for(cam, sc["deg"], bg=sc["bg"], device=device)

    def hip(sky_flag):
        twist = gs_pose.CameraTwist(cam).to(device)
        s = twist.settings(base)
        assert all(not c.is_leaf and c.requires_grad for c in (s.viewmatrix, s.projmatrix, s.campos))
        inputs = _raster_inputs(cam_t._fresh(sc["leaves"]))
        if sky_flag:
            image, radii, _, _ = gs_sky.render_with_sky(GaussianRasterizer(s), sky, camera_grads=True, **inputs)
        else:
            color, radii, _, alpha = GaussianRasterizer(s)(**inputs, aux_outputs=True, camera_grads=True)
            image = sky(color, alpha, s)
        return twist, image, radii

    twist, image, radii = hip(True)
    _, fl_r, _ = cam_t._masked_weights(name, sc, device, radii)
    fl_s = sky_pose_ref.flagged(cam.world_view_transform, tfx, tfy, W, H, tex.shape[1], tex.shape[2]).numpy()
    print(f"[twist + sky] flagged pixels: rasterizer {int(fl_r.sum())}, sky {int(fl_s.sum())} of {fl_r.size}")
    assert fl_s.mean() <= sky_pose_ref.FLAG_CAP
    keep = torch.from_numpy(~(fl_r | fl_s)).to(device)
    g = gs_scenes.dl_dimage(H, W, seed=78, scale=1.0).to(device) * keep[None]
    (image * g).sum().backward()
    torch.cuda.synchronize()
    got = twist.delta.grad
    assert got is not None and float(got.abs().min()) > 0

    want = []
    for dtype in (torch.float64, torch.float32):
        _, cams, outs, _, _ = cam_t._dense(name, sc, dtype, device)
        skyc = sky_pose_ref.sky(tex.to(dtype), cams[0], tfx, tfy, W, H)
        total = (g.to(dtype) * (outs[0] + (1 - outs[2]) * skyc)).sum()
        gr = torch.autograd.grad(total, cams, retain_graph=True)
        delta = torch.zeros(6, dtype=dtype, device=device, requires_grad=True)
        chain = cam_t._pose_chain(delta, cam.world_view_transform.to(device, dtype),
                                  cam.projection_matrix.to(device, dtype))
        torch.autograd.backward(list(chain), list(gr))
        want.append(delta.grad)
    check_4x(got, want[0], want[1], "ddelta [twist, sh2 + sky]")

    twist_r, image_r, _ = hip(False)
    assert torch.equal(_bits(image_r), _bits(image))
    (image_r * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(twist_r.delta.grad[3:]), _bits(got[3:]))
    assert not torch.equal(twist_r.delta.grad[:3], got[:3])


# ---- 8. a rotation recovered from a bare sky ----
def test_rotation_recovery_from_a_bare_sky(device):
    """Adam (lr 2e-3, 100 steps, mean squared error) on CameraTwist.delta from zero against the image
    at delta* = (0.02, -0.03, 0.015, 0, 0, 0): the rotation error ends at or below 0.1 |delta*| and the
    loss at or below 1 % of its first value (the torch reference in fp32 on the CPU reaches 0.0064
    |delta*| and 2e-5).  The sky is the only term: without its view gradient delta.grad stays None."""
    import gs_pose
    import gs_sky

    cam = gs_scenes.look_at_camera((0, 0, 0), (0.3, -0.4, -3.0), 96, 64)
    base = gs_scenes.raster_settings_for(cam, 0, device=device)
    Hs, Ws = 64, 128
    v = (torch.arange(Hs, dtype=torch.float64) + 0.5) / Hs * math.pi
    u = (torch.arange(Ws, dtype=torch.float64) + 0.5) / Ws * 2 * math.pi
    tex = torch.stack([0.5 + 0.25 * torch.sin(2 * u + 0.3)[None, :] * torch.sin(v)[:, None]
                       + 0.15 * torch.cos(3 * v + 0.5 * c)[:, None] + 0.1 * torch.sin((3 + c) * u + c)[None, :]
                       * torch.sin(2 * v)[:, None] for c in range(3)]).float()
    sky = gs_sky.SkySphere(Hs, Ws).to(device)
    with torch.no_grad():
        sky.texture.copy_(tex)
    sky.texture.requires_grad_(False)
    star = torch.tensor([0.02, -0.03, 0.015, 0.0, 0.0, 0.0], device=device)
    target_twist = gs_pose.CameraTwist(cam).to(device)
    with torch.no_grad():
        target_twist.delta.copy_(star)
        target = sky.render(target_twist.settings(base))
    twist = gs_pose.CameraTwist(cam).to(device)
    opt = torch.optim.Adam(twist.parameters(), lr=2e-3)
    losses = []
    for _ in range(100):
        opt.zero_grad(set_to_none=True)
        loss = ((sky.render(twist.settings(base), camera_grads=True) - target) ** 2).mean()
        loss.backward()
        assert twist.delta.grad is not None
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        last = float(((sky.render(twist.settings(base)) - target) ** 2).mean())
    first = float(losses[0])
    err = float((twist.delta.detach()[:3] - star[:3]).norm()) / float(star.norm())
    print(f"[rotation recovery] rotation error {err:.4f} |delta*|, loss {first:.3e} -> {last:.3e} ({last / first:.2e})")
    assert err <= 0.1
    assert last <= 0.01 * first
