"""Camera gradients of the rasterizer (GaussianRasterizer(..., camera_grads=True)): dL/dviewmatrix,
dL/dprojmatrix and dL/dcampos of settings' tensors, against fp64 autograd of the dense reference.

Every scene is seen through gs_scenes.look_at_camera((0.7, -0.4, -1.1), (0.1, 0.2, 4.0), W, H), never
the identity camera (an identity view hides transposed indices), and every test runs in both
numerics modes (gs_set_exact_exp).

Reference: dense_ref.render_local (dense_ref_aux.render_local_aux for the aux case) with view, proj
and campos as fp64 leaves, in the harness of test_gpu_dense._run_and_compare: flagged pixels are left
out of the image check and dL/dpix is zeroed there for all three backwards; caps: flagged share
<= 0.02, differing radii <= 1e-3.  For each of gV, gP and gC
    max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|f64|
(the project's conditioning rule: the dense reference in fp32, camera leaves included, is one other
valid fp32 order).  The dense side does not depend on the kernels' numerics mode and is computed
once per scene and mask.

Scenes:
    A       random_gaussians(2000, 3, seed=41) at 192 x 128: 7 full workgroups + 208 rows
    B       random_gaussians(6000, 1, seed=47, scale_range=(0.01, 0.08)) at 200 x 120, aux_outputs=True,
            loss over colour, inverse depth and alpha
    C       P = 256 * 257 + 1 = 65,793 rows at 72 x 40 of which 268 (rows [::251] and 0, 255, 256, 65535,
            65536, P - 1) stay and every other is mirrored through the camera centre (behind the
            camera): 258 partial rows, so the finish kernel loops, and a last workgroup of one row.
            The reference runs on the 268 rows.
    D       4,000 Gaussians with colors_precomp + cov3D_precomp on a coloured background
    E       the clamp branch: 600 small Gaussians + 48 large ones whose camera-space x/z (first 24) or
            y/z (last 24) is +-(1.32 .. 1.45) tan; all 48 must have a non-zero reference dL/dmeans3D
    small3  the first 3 Gaussians of A at 72 x 40;  one: the first alone
    sh0, sh2  SH degrees 0 and 2 on a 500-Gaussian cut of A (with A, B and D / the view-only call every
            k_camera_grad instantiation is launched in this process: tests/test_zz_kernel_coverage.py)
"""
import ctypes
import math

import pytest
import torch

import dense_cases
import dense_ref
import dense_ref_aux
import gpu_checks
import gs_scenes
from gpu_checks import check_4x, check_tol, mode  # noqa: F401

pytestmark = pytest.mark.gpu

EYE, TARGET = (0.7, -0.4, -1.1), (0.1, 0.2, 4.0)
CAM_KERNELS = ("camera_grad", "camera_grad_finish")
NAMES = ("viewmatrix", "projmatrix", "campos")


def _cam(W, H):
    return gs_scenes.look_at_camera(EYE, TARGET, W, H)


_SCENES = {}


def _scene_leaves(sc):
    return {k: getattr(sc, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}


def _scene(name, device):
    """dict(cam, leaves, deg, bg, aux, seed, rows): rows = the rows the reference runs on (None: all)."""
    if name in _SCENES:
        return _SCENES[name]
    bg, aux, rows = torch.zeros(3), False, None
    if name in ("A", "small3", "one", "sh0", "sh2"):
        cam, deg, seed = _cam(192, 128), 3, 41
        leaves = _scene_leaves(gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41))
        if name in ("small3", "one"):
            leaves = {k: v[:3 if name == "small3" else 1].contiguous() for k, v in leaves.items()}
            cam = _cam(72, 40)
        elif name != "A":
            deg = int(name[2])
            leaves = {k: v[:500].contiguous() for k, v in leaves.items()}
            leaves["shs"] = leaves["shs"][:, :(deg + 1) ** 2].contiguous()
    elif name == "B":
        cam, deg, seed, aux = _cam(200, 120), 1, 47, True
        leaves = _scene_leaves(gs_scenes.random_gaussians(6000, 1, cam=cam, seed=47, scale_range=(0.01, 0.08)))
    elif name == "C":
        cam, deg, seed, P = _cam(72, 40), 1, 53, 256 * 257 + 1
        leaves = _scene_leaves(gs_scenes.random_gaussians(P, 1, cam=cam, seed=53, scale_range=(0.02, 0.1)))
        stay = torch.zeros(P, dtype=torch.bool)
        stay[::251] = True
        stay[[0, 255, 256, 65535, 65536, P - 1]] = True
        assert int(stay.sum()) == 268
        m = leaves["means3D"]
        leaves["means3D"] = torch.where(stay[:, None], m, 2.0 * cam.camera_center[None] - m).contiguous()
        rows = stay
    elif name == "D":
        cam, deg, seed, P = _cam(256, 160), 0, 44, 4000
        d = gs_scenes.random_gaussians(P, 0, cam=cam, seed=44)
        R = dense_ref.quat_R(d.rotations)
        L = R * d.scales[:, None, :]
        S = L @ L.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
        leaves = dict(means3D=d.means3D, opacities=d.opacities,
                      colors=torch.rand((P, 3), generator=torch.Generator().manual_seed(45)), cov3D=cov)
        bg = torch.tensor([0.1, 0.2, 0.3])
    elif name == "E":
        cam, deg, seed = _cam(136, 88), 2, 61
        small = gs_scenes.random_gaussians(600, 2, cam=cam, seed=61)
        big = gs_scenes.random_gaussians(48, 2, cam=cam, seed=62, scale_range=(0.5, 1.0), z_range=(3.0, 5.0))
        g = torch.Generator().manual_seed(63)
        ratio = (1.32 + 0.13 * torch.rand(48, generator=g, dtype=torch.float64)) * torch.where(
            torch.rand(48, generator=g) < 0.5, -1.0, 1.0).double()
        wvt = cam.world_view_transform.double()
        pc = torch.cat([big.means3D.double(), torch.ones((48, 1), dtype=torch.float64)], 1) @ wvt
        pc[:24, 0] = ratio[:24] * math.tan(cam.FoVx / 2) * pc[:24, 2]
        pc[24:, 1] = ratio[24:] * math.tan(cam.FoVy / 2) * pc[24:, 2]
        big.means3D = (pc @ wvt.inverse())[:, :3].float().contiguous()
        leaves = _scene_leaves(gs_scenes.concat_scenes(small, big))
    else:
        raise KeyError(name)
    leaves = {k: v.to(device) for k, v in leaves.items()}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"])
    _SCENES[name] = dict(cam=cam, leaves=leaves, deg=deg, bg=bg.to(device), aux=aux, seed=seed, rows=rows)
    return _SCENES[name]


def _weights(sc, device):
    """the harness's draw for the colour, dl_dimage(seed = the scene's seed + 1, scale=1.0); the next two
    seeds for the inverse depth and alpha of an aux scene"""
    H, W, seed = sc["cam"].image_height, sc["cam"].image_width, sc["seed"]
    ws = [gs_scenes.dl_dimage(H, W, seed=seed + 1, scale=1.0).to(device)]
    if sc["aux"]:
        ws += [gs_scenes.dl_dimage(H, W, seed=seed + 2, scale=1.0)[:1].contiguous().to(device),
               gs_scenes.dl_dimage(H, W, seed=seed + 3, scale=1.0)[1:2].contiguous().to(device)]
    return ws


def _settings(sc, device, req=(True, True, True), cams=None):
    """The scene's settings with fresh camera leaves (requires_grad per `req`), or with `cams`."""
    s = gs_scenes.raster_settings_for(sc["cam"], sc["deg"], bg=sc["bg"], device=device)
    if cams is None:
        cams = [t.detach().clone().contiguous().requires_grad_(r)
                for t, r in zip((s.viewmatrix, s.projmatrix, s.campos), req)]
    return s._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2]), cams


def _call(s, t, aux, **kw):
    from diff_gaussian_rasterization import GaussianRasterizer

    args = {"shs": t.get("shs"), "colors_precomp": t.get("colors"), "scales": t.get("scales"),
            "rotations": t.get("rotations"), "cov3D_precomp": t.get("cov3D")}
    out = GaussianRasterizer(s)(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"],
                                **{k: v for k, v in args.items() if v is not None}, aux_outputs=aux, **kw)
    return (out[0], out[2], out[3]) if aux else (out[0],), out[1]


def _fresh(leaves):
    return {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}


def _hip(sc, device, ws=None, camera_grads=True, req=(True, True, True), cams=None, **kw):
    """One forward (+ backward of sum_k sum w_k out_k) through the public call.
    -> (outputs, radii, leaf tensors, camera tensors)"""
    s, cams = _settings(sc, device, req, cams)
    t = _fresh(sc["leaves"])
    outs, radii = _call(s, t, sc["aux"], camera_grads=camera_grads, **kw)
    if ws is not None:
        sum((w * o).sum() for w, o in zip(ws, outs)).backward()
    torch.cuda.synchronize()
    return outs, radii, t, cams


# ---- the dense side: forward once per (scene, dtype), camera gradients once per (scene, dtype, mask) ----
_DENSE, _DENSE_GRADS = {}, {}


def _dense(name, sc, dtype, device):
    key = (name, dtype)
    if key not in _DENSE:
        cam, rows = sc["cam"], sc["rows"]
        lv = sc["leaves"] if rows is None else {k: v[rows.to(device)] for k, v in sc["leaves"].items()}
        t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in lv.items()}
        cams = [x.to(device, dtype).contiguous().requires_grad_(True)
                for x in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
        fn = dense_ref_aux.render_local_aux if sc["aux"] else dense_ref.render_local
        res = fn(t["means3D"], t["means2D"], t["opacities"], cams[0], cams[1], cams[2], math.tan(cam.FoVx / 2),
                 math.tan(cam.FoVy / 2), cam.image_width, cam.image_height, sc["bg"].to(dtype), shs=t.get("shs"),
                 deg=sc["deg"], colors=t.get("colors"), scales=t.get("scales"), rots=t.get("rotations"),
                 cov3D=t.get("cov3D"))
        outs = (res[0], res[3], res[4]) if sc["aux"] else (res[0],)
        _DENSE[key] = (t, cams, outs, res[1], res[2])
    return _DENSE[key]


def _dense_grads(name, sc, dtype, device, ws, mask):
    """(gV, gP, gC, dL/dmeans3D) of the dense run under the masked weights."""
    key = (name, dtype, mask)
    if key not in _DENSE_GRADS:
        t, cams, outs, _, _ = _dense(name, sc, dtype, device)
        total = sum((w.to(dtype) * o).sum() for w, o in zip(ws, outs))
        g = torch.autograd.grad(total, cams + [t["means3D"]], retain_graph=True, allow_unused=True)
        _DENSE_GRADS[key] = [torch.zeros_like(x) if v is None else v for x, v in zip(cams + [t["means3D"]], g)]
    return _DENSE_GRADS[key]


def _masked_weights(name, sc, device, radii):
    """test_gpu_dense's harness: the flagged pixels (and the rectangles of Gaussians whose fp32 radius
    differs) -> (weights zeroed there, the flag map, the mask's key)."""
    cam, rows = sc["cam"], sc["rows"]
    W, H = cam.image_width, cam.image_height
    ref, rcams, _, rradii, flag = _dense(name, sc, torch.float64, device)
    hr = radii.cpu()
    if rows is not None:
        assert not hr[~rows].any(), "a hidden row is visible"
        hr = hr[rows]
    rdiff = (hr != rradii.cpu()).numpy()
    assert rdiff.mean() <= 1e-3, f"{int(rdiff.sum())} radii differ"
    fl = flag.cpu().numpy().copy()
    if rdiff.any():
        with torch.no_grad():
            q = dense_ref._prep(ref["means3D"], ref["means2D"], ref["opacities"], rcams[0], rcams[1], rcams[2],
                                math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H, shs=ref.get("shs"),
                                deg=sc["deg"], colors=ref.get("colors"), scales=ref.get("scales"),
                                rots=ref.get("rotations"), cov3D=ref.get("cov3D"))
        dense_cases.wide_mask(q["rect"].numpy(), rdiff, W, H, into=fl)
    print(f"\n[camera {name}] flagged pixels {int(fl.sum())}/{fl.size}, radii differing {int(rdiff.sum())}/{rdiff.size}, "
          f"visible {int((hr > 0).sum())}")
    assert fl.mean() <= 0.02
    keep_px = torch.from_numpy(~fl).to(device)
    return [w * keep_px[None] for w in _weights(sc, device)], fl, fl.tobytes()


def _cam_grads(cams):
    return [torch.zeros_like(c) if c.grad is None else c.grad for c in cams]


# ------------------------------------------------------------------------------------------
# 1. against the fp64 dense reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "small3", "one", "sh0", "sh2"])
def test_against_dense_fp64(device, mode, name):
    sc = _scene(name, device)
    s, cams = _settings(sc, device)
    t = _fresh(sc["leaves"])
    outs, radii = _call(s, t, sc["aux"], camera_grads=True)
    ws, fl, mask = _masked_weights(name, sc, device, radii)
    if name != "C":
        assert int((radii > 0).sum()) > 0
    sum((w * o).sum() for w, o in zip(ws, outs)).backward()
    torch.cuda.synchronize()
    g64 = _dense_grads(name, sc, torch.float64, device, ws, mask)
    g32 = _dense_grads(name, sc, torch.float32, device, ws, mask)
    rimg = _dense(name, sc, torch.float64, device)[2][0]
    check_tol(outs[0].permute(1, 2, 0), rimg.permute(1, 2, 0), f"image [{name}]", ~fl)
    got = _cam_grads(cams)
    assert got[0].shape == (4, 4) and got[1].shape == (4, 4) and got[2].shape == (3,)
    # structural zeros, written as such
    assert torch.equal(got[0][:, 3], torch.zeros(4, device=device))
    assert torch.equal(got[1][:, 2], torch.zeros(4, device=device))
    for k, nm in enumerate(NAMES):
        check_4x(got[k], g64[k], g32[k], f"d{nm} [{name}]")
    assert float(g64[0].abs().max()) > 0 and float(g64[1].abs().max()) > 0
    if name in ("D", "sh0"):  # precomputed colours, or a constant SH colour: the camera position enters nothing
        assert cams[2].grad is None or not cams[2].grad.any()
        assert not g64[2].any()
    else:
        assert float(g64[2].abs().max()) > 0
    if name == "E":  # every clamped Gaussian takes part (its means3D gradient is non-zero in the reference)
        with torch.no_grad():
            ref, rcams = _dense(name, sc, torch.float64, device)[:2]
            tv = torch.cat([ref["means3D"][600:], torch.ones((48, 1), dtype=torch.float64, device=device)], 1) @ rcams[0]
            cam = sc["cam"]
            assert (tv[:24, 0].abs() > 1.3 * math.tan(cam.FoVx / 2) * tv[:24, 2]).all()
            assert (tv[24:, 1].abs() > 1.3 * math.tan(cam.FoVy / 2) * tv[24:, 2]).all()
        n_live = int((g64[3][600:].abs().amax(1) > 0).sum())
        print(f"  clamped Gaussians with a non-zero reference dL/dmeans3D: {n_live} of 48")
        assert n_live == 48


def test_empty_scene_gives_zero_gradients_and_no_launch(device, mode):
    from diff_gaussian_rasterization import _native

    sc = dict(_scene("small3", device))
    sc["leaves"] = {k: v[:0].contiguous() for k, v in sc["leaves"].items()}
    lib = gpu_checks.lib()
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        outs, radii, t, cams = _hip(sc, device, ws=_weights(sc, device))
        launched = _native.profile_stats()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    assert radii.numel() == 0
    assert not [k for k in CAM_KERNELS if k in launched], launched
    for c in cams:
        assert c.grad is not None and c.grad.shape == c.shape and not c.grad.any()


# ------------------------------------------------------------------------------------------
# 2. bit identities
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_bit_identities(device, mode, name):
    """camera_grads=True changes nothing else (plain and aux), and is reproducible bit for bit."""
    sc = _scene(name, device)
    ws = _weights(sc, device)
    o0, r0, t0, c0 = _hip(sc, device, ws, camera_grads=False)
    o1, r1, t1, c1 = _hip(sc, device, ws)
    o2, r2, t2, c2 = _hip(sc, device, ws)
    assert torch.equal(r0, r1) and all(torch.equal(a, b) for a, b in zip(o0, o1))
    for k in t0:
        assert t0[k].grad is not None and torch.equal(t0[k].grad, t1[k].grad), f"d{k} differs with camera_grads"
    # the default: requires_grad matrices keep getting no gradient
    assert all(c.grad is None for c in c0)
    for a, b, nm in zip(c1, c2, NAMES):
        assert a.grad is not None and a.grad.abs().max() > 0, nm
        assert torch.equal(a.grad, b.grad), f"d{nm}: two identical runs differ"


def test_no_camera_tensor_requires_grad_launches_nothing(device, mode):
    from diff_gaussian_rasterization import _native

    sc = _scene("sh2", device)
    ws = _weights(sc, device)
    o0, r0, t0, _ = _hip(sc, device, ws, camera_grads=False, req=(False, False, False))
    lib = gpu_checks.lib()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        o1, r1, t1, c1 = _hip(sc, device, ws, req=(False, False, False))
        launched = _native.profile_stats()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    assert "render_bwd" in launched and "preprocess_bwd" in launched, launched
    assert not [k for k in CAM_KERNELS if k in launched], launched
    assert all(c.grad is None for c in c1)
    assert torch.equal(o0[0], o1[0]) and all(torch.equal(t0[k].grad, t1[k].grad) for k in t0)


def test_only_viewmatrix_skips_the_sh_rows(device, mode):
    """Only viewmatrix requires grad: gV as in the full call, nothing for the other two, and the
    instantiation without the SH read (DEG -1) is the one launched."""
    from diff_gaussian_rasterization import _native

    sc = _scene("sh2", device)
    ws = _weights(sc, device)
    _, _, _, full = _hip(sc, device, ws)
    lib = gpu_checks.lib()
    assert lib.gs_debug_launch_log(1) in (0, 1)
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        _, _, _, cams = _hip(sc, device, ws, req=(True, False, False))
        launched = _native.profile_stats()
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()
    assert launched["camera_grad"][1] == 1 and launched["camera_grad_finish"][1] == 1, launched
    assert torch.equal(cams[0].grad, full[0].grad)
    assert cams[1].grad is None and cams[2].grad is None
    n = lib.gs_debug_launched_kernels(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.gs_debug_launched_kernels(buf, n + 1)
    assert any("k_camera_gradILin1E" in k for k in buf.value.decode().split()), "DEG -1 instantiation not launched"
    # a leaf stored transposed (the reference's Camera keeps world_view_transform as a .transpose(0, 1)
    # view): the gradient comes back in the tensor's logical layout
    vt = cams[0].detach().t().contiguous().t().detach().requires_grad_(True)
    assert vt.is_leaf and not vt.is_contiguous() and torch.equal(vt, cams[0])
    _hip(sc, device, ws, cams=[vt, cams[1].detach(), cams[2].detach()])
    assert vt.grad.shape == (4, 4) and torch.equal(vt.grad, full[0].grad)


def test_invalid_instance_list_gives_zero_camera_gradients(device, mode):
    """The record sums' rule: a bounded forward whose instances exceed its capacity leaves no valid
    instance list (every access stays in bounds, tests/test_gpu_bounded.py), its record sums are
    zero, and so are the three camera gradients (the finishing kernel reads the view's flags).  The
    public call refuses binning_capacity= with camera_grads, so this goes through _C."""
    from diff_gaussian_rasterization import _C, bounded_status, last_num_rendered

    sc = _scene("sh2", device)
    s, _ = _settings(sc, device, req=(False, False, False))
    lv, e = sc["leaves"], torch.Tensor([])
    dpix = _weights(sc, device)[0]

    def run(cap):
        with torch.no_grad():
            R, _, radii, geom, binning, img = _C.rasterize_gaussians(
                s.bg, lv["means3D"], e, lv["opacities"], lv["scales"], lv["rotations"], s.scale_modifier, e,
                s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, lv["shs"],
                s.sh_degree, s.campos, s.prefiltered, s.debug, capacity=cap)
            res = _C.backward_impl(s.bg, lv["means3D"], radii, e, lv["scales"], lv["rotations"], s.scale_modifier, e,
                                   s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, lv["shs"], s.sh_degree,
                                   s.campos, geom, R, binning, img, s.debug, want_all=False, camera=True)
        torch.cuda.synchronize()
        return res[8]

    assert bounded_status() == (0, 0)
    run(None)
    n = last_num_rendered()
    assert n > 3
    for g in run(n):  # the capacity fits: the gradients of the read-back forward
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    for g in run(n // 3):
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="binning capacity"):
        bounded_status()
    assert bounded_status() == (0, 0)  # cleared


# ------------------------------------------------------------------------------------------
# 3. end to end: a twist of the pose
# ------------------------------------------------------------------------------------------
def _pose_chain(delta, view0, projection):
    """view = view0 exp(delta^) (row vectors: rotation block upper left, translation in the last row),
    full_proj = view @ projection and campos = view.inverse()[3, :3], as the reference's Camera builds
    them (scene/cameras.py)."""
    w, v = delta[:3], delta[3:]
    z = torch.zeros((), dtype=delta.dtype, device=delta.device)
    hat = torch.stack([torch.stack([z, w[2], -w[1], z]), torch.stack([-w[2], z, w[0], z]),
                       torch.stack([w[1], -w[0], z, z]), torch.stack([v[0], v[1], v[2], z])])
    view = view0 @ torch.matrix_exp(hat)
    return view, view @ projection, view.inverse()[3, :3]


def test_end_to_end_twist(device, mode):
    """dL/ddelta at delta = 0 through the HIP path (non-leaf camera tensors built in torch on the
    device) against the same chain in fp64 behind the dense reference's camera gradients; the fp32
    side of the rule is the chain in fp32 behind the dense fp32 run's."""
    name = "sh2"
    sc = _scene(name, device)
    cam = sc["cam"]

    def chain(dtype):
        delta = torch.zeros(6, dtype=dtype, device=device, requires_grad=True)
        return delta, _pose_chain(delta, cam.world_view_transform.to(device, dtype),
                                  cam.projection_matrix.to(device, dtype))

    delta, cams = chain(torch.float32)
    assert all(not c.is_leaf and c.requires_grad for c in cams)
    s, _ = _settings(sc, device, cams=list(cams))
    t = _fresh(sc["leaves"])
    outs, radii = _call(s, t, False, camera_grads=True)
    ws, _, mask = _masked_weights(name, sc, device, radii)
    (ws[0] * outs[0]).sum().backward()
    torch.cuda.synchronize()
    assert delta.grad is not None and float(delta.grad.abs().max()) > 0
    want = []
    for dtype in (torch.float64, torch.float32):
        g = _dense_grads(name, sc, dtype, device, ws, mask)
        d, c = chain(dtype)
        torch.autograd.backward(list(c), [g[0], g[1], g[2]])
        want.append(d.grad)
    check_4x(delta.grad, want[0], want[1], "ddelta [twist, sh2]")


# ------------------------------------------------------------------------------------------
# 4. interface
# ------------------------------------------------------------------------------------------
def test_refused_combinations(device, mode):
    from diff_gaussian_rasterization import register_gradient_sink, unregister_gradient_sink

    sc = _scene("small3", device)
    s, cams = _settings(sc, device)
    t = _fresh(sc["leaves"])
    with pytest.raises(RuntimeError, match="camera_grads:.*prepared"):
        _call(s, t, False, camera_grads=True, prepared=object())
    with pytest.raises(RuntimeError, match="camera_grads:.*binning_capacity"):
        _call(s, t, False, camera_grads=True, binning_capacity=4096)
    with pytest.raises(RuntimeError, match="camera_grads:.*sh_split"):
        _call(s, t, False, camera_grads=True,
              sh_split=(t["shs"][:, :1].detach().contiguous(), t["shs"][:, 1:].detach().contiguous()))

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
        for aux in (False, True):
            outs, _ = _call(s, t, aux, camera_grads=True)
            with pytest.raises(RuntimeError, match="camera_grads:.*deferring"):
                sum(o.sum() for o in outs).backward()
    finally:
        for p in params:
            unregister_gradient_sink(p)


# ------------------------------------------------------------------------------------------
# 5. camera gradients behind an owner that claims gradient buffers
# ------------------------------------------------------------------------------------------
def _run_with_claiming_owner(sc, device, ws, bufs, accumulate):
    """_hip with an owner registered on the inputs named in `bufs` that hands out (bufs[k], accumulate)."""
    from diff_gaussian_rasterization import register_gradient_sink, unregister_gradient_sink

    s, cams = _settings(sc, device)
    t = _fresh(sc["leaves"])

    class Owner:
        def claim(self, p):
            for k in bufs:
                if p is t[k]:
                    return bufs[k], accumulate
            return None

    owner = Owner()
    for k in bufs:
        register_gradient_sink(t[k], owner)
    try:
        outs, _ = _call(s, t, sc["aux"], camera_grads=True)
        sum((w * o).sum() for w, o in zip(ws, outs)).backward()
        torch.cuda.synchronize()
    finally:
        for k in bufs:
            unregister_gradient_sink(t[k])
    return t, cams


def _garbage(sc, device):
    g = torch.Generator(device="cpu").manual_seed(3)
    return {k: torch.randn(sc["leaves"][k].shape, generator=g).to(device) for k in ("means3D", "opacities")}


def test_overwriting_sink_with_camera_grads(device, mode):
    """An owner that hands out (buffer, False) for means3D and opacities: the buffers hold the un-sunk
    run's gradients bit for bit, the sunk inputs get no .grad, and every other Gaussian gradient and
    the three camera gradients (fixed-order fp64 sums) are those of the un-sunk run."""
    sc = _scene("small3", device)
    ws = _weights(sc, device)
    _, _, t0, c0 = _hip(sc, device, ws)
    assert float(t0["means3D"].grad.abs().max()) > 0 and float(t0["opacities"].grad.abs().max()) > 0
    bufs = _garbage(sc, device)
    t, cams = _run_with_claiming_owner(sc, device, ws, bufs, False)
    assert t["means3D"].grad is None and t["opacities"].grad is None  # sunk
    for k in bufs:
        assert torch.equal(bufs[k], t0[k].grad), k
    for k in ("shs", "scales", "rotations", "means2D"):
        assert torch.equal(t[k].grad, t0[k].grad), k
    for a, b, nm in zip(cams, c0, NAMES):
        assert a.grad is not None and float(a.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad), nm


def test_accumulating_sink_with_camera_grads(device, mode):
    """An owner that hands out (buffer, True): the buffer ends as before + grad.  opacity: one fp32
    old + new, exact (tests/test_gpu_aux.py::test_accumulating_sink).  means3D: that test's bound,
    4 * 2^-24 (max|before| + max|grad|); without the aux outputs there is no depth-chain term, the sum
    is one fp32 addition as well, and the exact comparison holds too."""
    sc = _scene("small3", device)
    ws = _weights(sc, device)
    _, _, t0, c0 = _hip(sc, device, ws)
    assert float(t0["means3D"].grad.abs().max()) > 0
    before = _garbage(sc, device)
    bufs = {k: v.clone() for k, v in before.items()}
    t, cams = _run_with_claiming_owner(sc, device, ws, bufs, True)
    assert t["means3D"].grad is None and t["opacities"].grad is None  # sunk
    assert torch.equal(bufs["opacities"], before["opacities"] + t0["opacities"].grad)
    want = before["means3D"] + t0["means3D"].grad
    tol = 4 * 2.0 ** -24 * float(before["means3D"].abs().max() + t0["means3D"].grad.abs().max())
    err = float((bufs["means3D"] - want).abs().max())
    print(f"\n  means3D: max|buffer - (before + grad)| {err:.3e}  (bound {tol:.3e})")
    assert err <= tol
    assert torch.equal(bufs["means3D"], want)
    for k in ("shs", "scales", "rotations", "means2D"):
        assert torch.equal(t[k].grad, t0[k].grad), k
    for a, b, nm in zip(cams, c0, NAMES):
        assert torch.equal(a.grad, b.grad), nm
