"""GPU parity: the HIP path (through the C ABI, via the drop-in package) against the CPU oracle on
identical seeded inputs.

Two numerics modes (gs_set_exact_exp):
  - EXACT mode (the tests below unless marked "fast"): every integer and every float of the
    forward is BIT-EXACT.  The kernels and the oracle follow one explicit operation order with no
    FMA contraction and the same exp2 polynomial, so radii, num_rendered, the tile-sorted instance
    list, ranges, splat attributes, n_contrib, final_T and the image must be identical.
  - FAST mode (the library default, hardware v_exp_f32 in the render loops, <= 1 ulp): everything
    up to the render loop is still bit-exact (radii, num_rendered, list, ranges, splat attributes);
    n_contrib must be identical except at the pixels the oracle flags as near a threshold (alpha
    within 1e-6 of 1/255 or a tested T within 2e-5 of 1e-4, relative), final_T and the image
    within 1e-5 * |ref| + 1e-5 * max|ref| away from those pixels, and the gradients at the
    backward tolerance below for every Gaussian not listed in a tile holding a flagged pixel.
    The flagged count is reported and bounded (<= 0.1 % of the pixels).
  - Backward: the GPU sums per-pixel terms in fp32 (in-lane over the lane's pixels, then the wave's
    DPP tree -> per-instance records -> per-Gaussian fp64 sum); the oracle sums the identical fp32
    terms in fp64.
    Per tensor: |gpu - oracle| <= 1e-5 * |oracle| + 1e-5 * max|oracle|  (north-star 1e-5 rel fp32).
"""
import math

import numpy as np
import pytest
import torch

import gs_scenes
from gpu_checks import RTOL, check_tol, exact_mode, fast_mode  # noqa: F401

# every test here runs in the bit-exact numerics mode unless it switches to fast (and restores)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("exact_mode")]

def _oracle_scene(oracle, cam, sc, bg, colors=None, cov3D=None, deg=None, mod=1.0):
    deg = sc.sh_degree if deg is None else deg
    return oracle.Scene(bg=bg, means3D=sc.means3D.numpy(), opacities=sc.opacities.numpy(), W=cam.image_width,
                        H=cam.image_height, viewmatrix=cam.world_view_transform.numpy(),
                        projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(),
                        tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2),
                        shs=None if colors is not None else sc.shs.numpy(), sh_degree=deg, colors_precomp=colors,
                        scales=None if cov3D is not None else sc.scales.numpy(),
                        rotations=None if cov3D is not None else sc.rotations.numpy(), cov3D_precomp=cov3D,
                        scale_modifier=mod)


def _gpu_run(cam, sc, device, bg, dpix, colors=None, cov3D=None, deg=None, mod=1.0, debug=False):
    """Forward + backward through GaussianRasterizer exactly as the reference adapter calls it."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C

    deg = sc.sh_degree if deg is None else deg
    s = gs_scenes.raster_settings_for(cam, deg, bg=torch.tensor(bg, device=device), scale_modifier=mod,
                                      debug=debug, device=device)
    d = sc.to(device)
    means3D = d.means3D.clone().requires_grad_(True)
    means2D = torch.zeros_like(means3D, requires_grad=True)
    opac = d.opacities.clone().requires_grad_(True)
    kw = {}
    leaves = dict(means3D=means3D, means2D=means2D, opacities=opac)
    if colors is None:
        kw["shs"] = leaves["shs"] = d.shs.clone().requires_grad_(True)
    else:
        kw["colors_precomp"] = leaves["colors"] = torch.tensor(colors, device=device).requires_grad_(True)
    if cov3D is None:
        kw["scales"] = leaves["scales"] = d.scales.clone().requires_grad_(True)
        kw["rotations"] = leaves["rotations"] = d.rotations.clone().requires_grad_(True)
    else:
        kw["cov3D_precomp"] = leaves["cov3D"] = torch.tensor(cov3D, device=device).requires_grad_(True)
    img, radii = GaussianRasterizer(s)(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    (img * torch.tensor(dpix, device=device)).sum().backward()
    torch.cuda.synchronize()
    return img, radii, leaves


def _check_forward_exact(oracle_fw, cam, sc, device, colors=None, cov3D=None, deg=None):
    """Bit-exact comparison of every forward intermediate (through _C + debug export)."""
    from diff_gaussian_rasterization import _C

    deg = sc.sh_degree if deg is None else deg
    s = gs_scenes.raster_settings_for(cam, deg, bg=torch.tensor(oracle_fw["bg"], device=device), device=device)
    d = sc.to(device)
    e = torch.Tensor([])
    num, color, radii, geom, binb, imgb = _C.rasterize_gaussians(
        s.bg, d.means3D, e if colors is None else torch.tensor(colors, device=device), d.opacities,
        d.scales if cov3D is None else e, d.rotations if cov3D is None else e, s.scale_modifier,
        e if cov3D is None else torch.tensor(cov3D, device=device), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy,
        s.image_height, s.image_width, d.shs if colors is None else e, deg, s.campos, False, False)
    ex = _C.debug_export(sc.P, cam.image_width, cam.image_height, num, geom, binb, imgb, device)
    torch.cuda.synchronize()
    assert num == oracle_fw["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), oracle_fw["radii"])
    vis = oracle_fw["radii"] > 0
    np.testing.assert_array_equal(ex["tiles_touched"].cpu().numpy().astype(np.uint32), oracle_fw["tiles_touched"])
    np.testing.assert_array_equal(ex["point_list"].cpu().numpy().astype(np.uint32), oracle_fw["point_list"])
    np.testing.assert_array_equal(ex["ranges"].cpu().numpy().astype(np.uint32), oracle_fw["ranges"])
    np.testing.assert_array_equal(ex["xy"].cpu().numpy()[vis], oracle_fw["xy"][vis])
    np.testing.assert_array_equal(ex["conic_opacity"].cpu().numpy()[vis], oracle_fw["conic_opacity"][vis])
    np.testing.assert_array_equal(ex["rgb"].cpu().numpy()[vis], oracle_fw["rgb"][vis])
    np.testing.assert_array_equal(ex["n_contrib"].cpu().numpy().astype(np.uint32), oracle_fw["n_contrib"])
    np.testing.assert_array_equal(ex["final_T"].cpu().numpy(), oracle_fw["final_T"])
    np.testing.assert_array_equal(color.cpu().numpy(), oracle_fw["color"])


def _check_backward(gr, leaves, colors=None, cov3D=None, rtol=RTOL, chain_frac=None):
    """chain_frac: bound (fraction of the max) for the gradients reached through the conic ->
    covariance chain (dmeans3D, dscales, drotations, dcov3D); default rtol."""
    g = lambda k: leaves[k].grad.detach().cpu().numpy()  # noqa: E731
    cf = rtol if chain_frac is None else chain_frac
    check_tol(g("means2D"), gr["dmeans2D"], "dmeans2D", rtol=rtol, frac=rtol)
    check_tol(g("opacities"), gr["dopacity"], "dopacity", rtol=rtol, frac=rtol)
    check_tol(g("means3D"), gr["dmeans3D"], "dmeans3D", rtol=rtol, frac=cf)
    if colors is None:
        check_tol(g("shs"), gr["dsh"], "dsh", rtol=rtol, frac=rtol)
    else:
        check_tol(g("colors"), gr["dcolors"], "dcolors", rtol=rtol, frac=rtol)
    if cov3D is None:
        check_tol(g("scales"), gr["dscales"], "dscales", rtol=rtol, frac=cf)
        check_tol(g("rotations"), gr["drotations"], "drotations", rtol=rtol, frac=cf)
    else:
        check_tol(g("cov3D"), gr["dcov3D"], "dcov3D", rtol=rtol, frac=cf)


CHAIN_KEYS = (("means3D", "dmeans3D"), ("scales", "dscales"), ("rotations", "drotations"), ("cov3D", "dcov3D"))
NOISE_FACTOR = 4.0


def _check_chain_noise(leaves, gr64, gr32, factor=NOISE_FACTOR, rtol=RTOL):
    """Conditioning-aware bound for the conic -> covariance chain gradients.  gr64: the oracle with
    fp64 sums; gr32: the same oracle summing in fp32 (oracle.backward_f32_acc), i.e. one other valid
    fp32 order.  |gr32 - gr64| is what fp32 summation alone does to these gradients on this scene;
    the device (fp32 wave trees per tile, fp64 across tiles) must stay within `factor` times that,
    plus rtol of the max for well-conditioned scenes where both are ~0.  The fixed fraction-of-max
    bounds (chain_frac) stay as a second check."""
    out = {}
    for k, rk in CHAIN_KEYS:
        if k not in leaves:
            continue
        gpu = leaves[k].grad.detach().cpu().numpy().astype(np.float64)
        r64 = np.asarray(gr64[rk], np.float64)
        r32 = np.asarray(gr32[rk], np.float64)
        d_gpu = float(np.abs(gpu - r64).max(initial=0.0))
        d_32 = float(np.abs(r32 - r64).max(initial=0.0))
        scale = float(np.abs(r64).max(initial=0.0))
        out[rk] = (d_gpu, d_32, scale)
        print(f"chain noise {rk}: max|gpu - f64| {d_gpu:.3e}  max|f32 order - f64| {d_32:.3e}  max|f64| {scale:.3e}")
        assert d_gpu <= factor * d_32 + rtol * scale, (rk, d_gpu, d_32, scale)
    return out


CASES = [
    # name, P, sh_degree, W, H, bg
    ("tiny", 64, 3, 64, 48, 0.0),
    ("C1_10k_sh0_256", 10_000, 0, 256, 256, 0.0),
    ("ragged_sh1_bg", 3_000, 1, 203, 117, 0.5),
    ("C2_100k_sh3_800", 100_000, 3, 800, 800, 0.0),
    # degenerate frames: one pixel, one row, one column, smaller than a tile; a single Gaussian
    ("one_pixel", 16, 0, 1, 1, 0.2),
    ("one_row", 300, 1, 37, 1, 0.0),
    ("one_col", 300, 2, 1, 45, 0.3),
    ("single_gaussian", 1, 3, 33, 17, 0.1),
]


@pytest.mark.parametrize("name,P,deg,W,H,bgv", CASES, ids=[c[0] for c in CASES])
def test_forward_bitexact_and_backward_vs_oracle(oracle, device, name, P, deg, W, H, bgv):
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=0)
    bg = np.full(3, bgv, np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=1).numpy()
    img, radii, leaves = _gpu_run(cam, sc, device, bg, dpix)
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    gr = oracle.backward(osc, dpix)
    _check_backward(gr, leaves)


def _check_forward_fast(ofw, cam, sc, device, bg):
    """Fast-mode forward: bit-exact up to the render loop, tolerance in it (module docstring).
    Pixels the oracle flags as near an alpha / T decision get the decision-flip bound instead:
    one flipped entry moves a pixel's colour by at most 0.01 (T stop: alpha T c with T (1 - alpha)
    ~ 1e-4, alpha <= 0.99) or alpha T c ~ c / 255 (alpha test), plus the background term.
    Returns (colour, Gaussians listed in a flagged pixel's tile, near mask)."""
    from diff_gaussian_rasterization import _C

    s = gs_scenes.raster_settings_for(cam, sc.sh_degree, bg=torch.tensor(bg, device=device), device=device)
    d = sc.to(device)
    e = torch.Tensor([])
    num, color, radii, geom, binb, imgb = _C.rasterize_gaussians(
        s.bg, d.means3D, e, d.opacities, d.scales, d.rotations, s.scale_modifier, e, s.viewmatrix, s.projmatrix,
        s.tanfovx, s.tanfovy, s.image_height, s.image_width, d.shs, sc.sh_degree, s.campos, False, False)
    ex = _C.debug_export(sc.P, cam.image_width, cam.image_height, num, geom, binb, imgb, device)
    torch.cuda.synchronize()
    assert num == ofw["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
    vis = ofw["radii"] > 0
    for k in ("point_list", "ranges", "tiles_touched"):
        np.testing.assert_array_equal(ex[k].cpu().numpy().astype(np.uint32), ofw[k].astype(np.uint32), err_msg=k)
    for k in ("xy", "conic_opacity", "rgb"):
        np.testing.assert_array_equal(ex[k].cpu().numpy()[vis], ofw[k][vis], err_msg=k)
    near = ofw["near"].astype(bool)
    H, W = near.shape
    assert near.sum() <= max(1, near.size // 1000), f"{int(near.sum())} near-threshold pixels"
    keep = ~near
    np.testing.assert_array_equal(ex["n_contrib"].cpu().numpy().astype(np.uint32)[keep], ofw["n_contrib"][keep])
    check_tol(ex["final_T"].cpu().numpy()[keep], ofw["final_T"][keep], "final_T")
    col = color.cpu().numpy()
    check_tol(col[:, keep], ofw["color"][:, keep], "color")
    if near.any():  # decision-flip bound at the flagged pixels
        cmax = float(np.abs(ofw["rgb"][vis]).max(initial=0.0)) + float(np.abs(bg).max())
        dT = np.abs(ex["final_T"].cpu().numpy()[near] - ofw["final_T"][near])
        dC = np.abs(col[:, near] - ofw["color"][:, near])
        assert dT.max() <= 0.01 + 1e-6, f"final_T at flagged pixels: max |d| = {dT.max():.3e}"
        assert dC.max() <= 0.02 * cmax + 1e-6, f"colour at flagged pixels: max |d| = {dC.max():.3e} (cmax {cmax})"
    # Gaussians listed in a tile that holds a flagged pixel
    excl = np.zeros(sc.P, bool)
    gx = (W + 15) // 16
    for y, x in zip(*np.nonzero(near)):
        t = (y // 16) * gx + x // 16
        a, b = ofw["ranges"][t]
        excl[ofw["point_list"][a:b]] = True
    return color, excl, near


_GRADS = (("means2D", "dmeans2D"), ("opacities", "dopacity"), ("means3D", "dmeans3D"), ("shs", "dsh"),
          ("scales", "dscales"), ("rotations", "drotations"))


def _check_backward_masked(gr, leaves, excl, rtol=RTOL):
    keep = ~excl
    g = lambda k: leaves[k].grad.detach().cpu().numpy()[keep]  # noqa: E731
    for k, o in _GRADS:
        check_tol(g(k), gr[o][keep], o, rtol=rtol, frac=rtol)


def _fast_mode_parity(oracle, device, cam, sc, bg, dpix_seed=1):
    """Fast mode vs the oracle with no Gaussian left unchecked:
      (1) dL/dimage zeroed at the flagged pixels, on both sides: every gradient of EVERY Gaussian
          at the strict tolerance (the backward is per pixel, so this is exactly the gradient over
          all unflagged pixels);
      (2) the full dL/dimage: the Gaussians listed in no flagged pixel's tile at the strict
          tolerance; the others within the strict tolerance plus twice the flagged pixels' own
          contribution to them, measured on each side as full - masked (a decision flip changes
          a flagged pixel's terms, never an unflagged one's).
    Prints the flagged-pixel and bounded-Gaussian fractions."""
    W, H = cam.image_width, cam.image_height
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True, near=True)
    color, excl, near = _check_forward_fast(ofw, cam, sc, device, bg)
    dpix = gs_scenes.dl_dimage(H, W, seed=dpix_seed).numpy()
    dpix_m = dpix * (~near)[None].astype(np.float32)
    img, _, lm = _gpu_run(cam, sc, device, bg, dpix_m)
    assert torch.equal(img, color)  # the autograd path renders the same image
    gm = oracle.backward(osc, dpix_m)
    gpu_m = {o: lm[k].grad.detach().cpu().numpy() for k, o in _GRADS}
    for k, o in _GRADS:
        check_tol(gpu_m[o], gm[o], o + " (all Gaussians, unflagged pixels)")
    del lm
    _, _, lf = _gpu_run(cam, sc, device, bg, dpix)
    gf = oracle.backward(osc, dpix)
    _check_backward_masked(gf, lf, excl)
    worst = 0.0
    for k, o in _GRADS:
        gpu_f = lf[k].grad.detach().cpu().numpy()
        ref = gf[o].astype(np.float64)
        scale = max(np.abs(ref).max(), 1e-30)
        flag = np.abs(gf[o].astype(np.float64) - gm[o]) + np.abs(gpu_f.astype(np.float64) - gpu_m[o])
        d = np.abs(gpu_f - ref)[excl]
        tol = (RTOL * np.abs(ref) + RTOL * scale + 2.0 * flag)[excl]
        assert (d <= tol).all(), f"{o}: flagged-tile Gaussians beyond the flip bound, max|d| {d.max():.3e}"
        if d.size:
            worst = max(worst, float(d.max() / scale))
    print(f"\n[fast parity {W}x{H} P={sc.P}] flagged pixels {near.mean():.2e}, Gaussians in flagged tiles "
          f"{excl.mean():.2e} (bounded), worst bounded |d|/max {worst:.2e}")


FAST_CASES = [c for c in CASES if c[0] != "tiny"] + [("C3_crop_sh3_1080", 60_000, 3, 480, 1080, 0.0)]


@pytest.mark.parametrize("name,P,deg,W,H,bgv", FAST_CASES, ids=[c[0] for c in FAST_CASES])
def test_fast_mode_forward_and_backward_vs_oracle(oracle, device, fast_mode, name, P, deg, W, H, bgv):
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=0)
    _fast_mode_parity(oracle, device, cam, sc, np.full(3, bgv, np.float32))


def test_fast_mode_full_c3_vs_oracle(oracle, device, fast_mode):
    """The benchmarked configuration itself: C3 = 1M Gaussians SH3 at 1920x1080 in the default
    (fast) numerics mode, against the oracle at full size (no crop)."""
    cam = gs_scenes.identity_camera(1920, 1080)
    sc = gs_scenes.random_gaussians(1_000_000, 3, cam=cam, seed=0)
    _fast_mode_parity(oracle, device, cam, sc, np.zeros(3, np.float32))


@pytest.mark.timeout(600)
def test_fast_mode_full_c5_vs_oracle(oracle, device, fast_mode):
    """C5 (bench --workload c5) at full size: 5M Gaussians SH3 at 1920x1080, 21.6M instances, most
    of them behind saturated pixels (the record cuts and the longest-first order at their extreme),
    in the default numerics mode against the oracle; same checks as full C3."""
    cam = gs_scenes.identity_camera(1920, 1080)
    sc = gs_scenes.random_gaussians(5_000_000, 3, cam=cam, seed=0)
    _fast_mode_parity(oracle, device, cam, sc, np.zeros(3, np.float32))


def test_fast_mode_is_deterministic(device, fast_mode):
    cam = gs_scenes.identity_camera(256, 256)
    sc = gs_scenes.random_gaussians(20000, 3, cam=cam, seed=13)
    dpix = gs_scenes.dl_dimage(256, 256).numpy()
    bg = np.zeros(3, np.float32)
    a, _, la = _gpu_run(cam, sc, device, bg, dpix)
    b, _, lb = _gpu_run(cam, sc, device, bg, dpix)
    assert torch.equal(a, b)
    for k in la:
        assert torch.equal(la[k].grad, lb[k].grad), k


def _large_splat_scene(anisotropy):
    W, H = 640, 360
    cam = gs_scenes.identity_camera(W, H)
    small = gs_scenes.random_gaussians(3000, 2, cam=cam, seed=21)
    big = gs_scenes.random_gaussians(60, 2, cam=cam, seed=22, scale_range=(0.3, 1.5), z_range=(2.0, 4.0))
    big.scales[::3, 0] /= anisotropy
    return cam, gs_scenes.concat_scenes(small, big)


def test_large_and_elongated_splats(oracle, device):
    """Skysphere-like mix: many small splats plus large ones spanning dozens of tiles and several
    duplicate workgroups (row spans over many tile rows, segments crossing workgroups, long
    per-Gaussian record runs).  Every gradient, the covariance chain included, at the 1e-5
    contract (round 6: measured max 4.9e-6 of the max, drotations, tests/parity_report.py; the
    bound was 1e-4 through round 5): large splats' per-pixel dL/dconic terms cancel across hundreds
    of tiles, the GPU sums them in fp32 wave trees (the oracle in fp64), and the conic ->
    covariance chain amplifies the ~1e-7 relative difference (test_needle_splats_conditioning is
    the extreme case)."""
    cam, sc = _large_splat_scene(anisotropy=3.0)
    W, H = cam.image_width, cam.image_height
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    assert ofw["tiles_touched"].max() > 300
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=23).numpy()
    img, _, leaves = _gpu_run(cam, sc, device, bg, dpix)
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    gr = oracle.backward(osc, dpix)
    _check_backward(gr, leaves)
    _check_chain_noise(leaves, gr, oracle.backward_f32_acc(osc, dpix))


def test_needle_splats_conditioning(oracle, device):
    """Needles (60:1 and more) make conic -> covariance -> scale/rotation/mean an ill-conditioned
    chain: the fp32 per-pixel sums of dL/dconic (GPU: fp32 wave trees; oracle: fp64) agree to
    ~1e-6 relative, and the chain amplifies that in the covariance-derived gradients (upstream's
    fp32 atomics have the same property).  Forward stays bit-exact; dmeans2D / dopacity / dsh keep
    the 1e-5 bound; dmeans3D / dscales / drotations are held to 5e-5 of their max (round 6: measured
    2.3e-5, drotations; the bound was 2e-3 through round 5).  Against the independent fp64 dense
    reference, which also rounds no per-pixel term to fp32, the same needles sit at up to 8.9e-4 of
    the max (test_gpu_dense.py::test_hip_vs_dense_large_and_needle_splats, bound 1e-3): that
    distance is the fp32 per-pixel terms through the ill-conditioned chain, not the summation."""
    cam, sc = _large_splat_scene(anisotropy=60.0)
    W, H = cam.image_width, cam.image_height
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=23).numpy()
    img, _, leaves = _gpu_run(cam, sc, device, bg, dpix)
    gr = oracle.backward(osc, dpix)
    g = lambda k: leaves[k].grad.detach().cpu().numpy()  # noqa: E731
    check_tol(g("means2D"), gr["dmeans2D"], "dmeans2D")
    check_tol(g("opacities"), gr["dopacity"], "dopacity")
    check_tol(g("shs"), gr["dsh"], "dsh")
    for k, rk in (("means3D", "dmeans3D"), ("scales", "dscales"), ("rotations", "drotations")):
        check_tol(g(k), gr[rk], rk, rtol=1e-5, frac=5e-5)
    # the 5e-5 above is the conditioning, not the device: an fp32 order of the oracle's own sums
    # moves these gradients as far (and the device stays within NOISE_FACTOR of that)
    noise = _check_chain_noise(leaves, gr, oracle.backward_f32_acc(osc, dpix))
    assert max(d32 / s for _, d32, s in noise.values()) > 1e-5  # the chain really is ill-conditioned here


def test_few_huge_splats_use_per_splat_duplicate(oracle, device):
    """More than 2048 instances per Gaussian on average: the binning falls back to the per-splat
    duplicate kernel (DUP_SLOTS * P < num_rendered); results stay bit-exact."""
    W, H = 1920, 1080
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(4, 0, cam=cam, seed=31, scale_range=(3.0, 6.0), z_range=(3.0, 5.0))
    sc.means3D[:, :2] = 0.0
    sc.opacities[:] = 0.9
    bg = np.zeros(3, np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    assert ofw["num_rendered"] > 2048 * 4
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=32).numpy()
    img, _, leaves = _gpu_run(cam, sc, device, bg, dpix)
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    _check_backward(oracle.backward(osc, dpix), leaves)


def test_precomputed_colors_and_cov3d(oracle, device):
    W, H = 160, 96
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(2000, 0, cam=cam, seed=3)
    colors = np.random.default_rng(0).random((2000, 3), dtype=np.float32)
    cov = oracle.cov3d(sc.scales.numpy(), 1.0, sc.rotations.numpy())
    bg = np.array([0.2, 0.1, 0.0], np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg, colors=colors, cov3D=cov)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    _check_forward_exact(ofw, cam, sc, device, colors=colors, cov3D=cov)
    dpix = gs_scenes.dl_dimage(H, W, seed=2).numpy()
    img, _, leaves = _gpu_run(cam, sc, device, bg, dpix, colors=colors, cov3D=cov)
    gr = oracle.backward(osc, dpix)
    _check_backward(gr, leaves, colors=colors, cov3D=cov)


def test_active_degree_below_max_uses_stride_M(oracle, device):
    """train.py raises the active SH degree every 1000 its (gaussian_model.py:120-122): shs keeps
    M = 16 coefficients while D < 3; coefficients past (D+1)^2 get zero gradient."""
    W, H = 128, 128
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(4000, 3, cam=cam, seed=4)
    bg = np.zeros(3, np.float32)
    for D in (0, 1, 2):
        osc = _oracle_scene(oracle, cam, sc, bg, deg=D)
        ofw = oracle.forward(osc, intermediates=True)
        ofw["bg"] = bg
        _check_forward_exact(ofw, cam, sc, device, deg=D)
        dpix = gs_scenes.dl_dimage(H, W, seed=5).numpy()
        img, _, leaves = _gpu_run(cam, sc, device, bg, dpix, deg=D)
        gr = oracle.backward(osc, dpix)
        _check_backward(gr, leaves)
        assert torch.all(leaves["shs"].grad[:, (D + 1) ** 2:] == 0)


def test_scale_modifier(oracle, device):
    W, H = 96, 96
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(1500, 1, cam=cam, seed=6)
    bg = np.zeros(3, np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg, mod=0.6)
    ofw = oracle.forward(osc)
    dpix = gs_scenes.dl_dimage(H, W, seed=7).numpy()
    img, radii, leaves = _gpu_run(cam, sc, device, bg, dpix, mod=0.6)
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
    _check_backward(oracle.backward(osc, dpix), leaves)


def test_empty_scene_returns_zero_image(device):
    """Upstream skips all work for P == 0: all-zero image (background NOT composited), empty radii."""
    cam = gs_scenes.identity_camera(64, 32)
    sc = gs_scenes.random_gaussians(0, 0, cam=cam)
    img, radii, leaves = _gpu_run(cam, sc, device, np.ones(3, np.float32), np.ones((3, 32, 64), np.float32))
    assert img.shape == (3, 32, 64) and torch.all(img == 0) and radii.numel() == 0


def test_all_culled_scene_is_background(oracle, device):
    cam = gs_scenes.identity_camera(64, 48)
    sc = gs_scenes.random_gaussians(500, 0, cam=cam, seed=9)
    sc.means3D[:, 2] = -sc.means3D[:, 2]  # behind the camera
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    dpix = gs_scenes.dl_dimage(48, 64).numpy()
    img, radii, leaves = _gpu_run(cam, sc, device, bg, dpix)
    assert torch.all(radii == 0)
    ref = np.broadcast_to(bg[:, None, None], (3, 48, 64))
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ref)
    for k, v in leaves.items():
        assert torch.all(v.grad == 0), k


def test_interleaved_culled_gaussians(oracle, device):
    """Culled Gaussians scattered through the index order (behind the camera, every third one):
    the first depth-sort pass drops them inside every sort tile (the visibility compaction)."""
    W, H = 160, 120
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(9000, 2, cam=cam, seed=12)
    sc.means3D[::3, 2] = -sc.means3D[::3, 2]
    bg = np.zeros(3, np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=13).numpy()
    _, radii, leaves = _gpu_run(cam, sc, device, bg, dpix)
    assert torch.all(radii[::3] == 0) and int((radii > 0).sum()) > 3000
    _check_backward(oracle.backward(osc, dpix), leaves)


def test_multi_view_circle_cameras(oracle, device):
    """C4-style cameras (look-at, non-identity view) exercise the full view / projection path."""
    cams = gs_scenes.circle_cameras(3, 6.0, 200, 150)
    sc = gs_scenes.random_gaussians(5000, 3, seed=10, ball_radius=2.0)
    bg = np.zeros(3, np.float32)
    for cam in cams:
        osc = _oracle_scene(oracle, cam, sc, bg)
        ofw = oracle.forward(osc, intermediates=True)
        ofw["bg"] = bg
        _check_forward_exact(ofw, cam, sc, device)
        dpix = gs_scenes.dl_dimage(150, 200, seed=11).numpy()
        _, _, leaves = _gpu_run(cam, sc, device, bg, dpix)
        _check_backward(oracle.backward(osc, dpix), leaves)


def test_prefiltered_near_point_raises(device):
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = gs_scenes.identity_camera(32, 32)
    sc = gs_scenes.random_gaussians(10, 0, cam=cam, seed=1).to(device)
    sc.means3D[0, 2] = 0.1
    s = gs_scenes.raster_settings_for(cam, 0, device=device)._replace(prefiltered=True)
    with pytest.raises(RuntimeError, match="prefiltered"):
        GaussianRasterizer(s)(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities,
                              shs=sc.shs, scales=sc.scales, rotations=sc.rotations)


def test_debug_mode_matches_normal_mode(device):
    cam = gs_scenes.identity_camera(80, 64)
    sc = gs_scenes.random_gaussians(800, 2, cam=cam, seed=12)
    dpix = gs_scenes.dl_dimage(64, 80).numpy()
    bg = np.zeros(3, np.float32)
    a, _, la = _gpu_run(cam, sc, device, bg, dpix, debug=False)
    b, _, lb = _gpu_run(cam, sc, device, bg, dpix, debug=True)
    assert torch.equal(a, b)
    for k in la:
        assert torch.equal(la[k].grad, lb[k].grad), k


def test_backward_is_deterministic(device):
    """No float atomics anywhere: two backward passes are bit-identical."""
    cam = gs_scenes.identity_camera(256, 256)
    sc = gs_scenes.random_gaussians(20000, 3, cam=cam, seed=13)
    dpix = gs_scenes.dl_dimage(256, 256).numpy()
    bg = np.zeros(3, np.float32)
    _, _, la = _gpu_run(cam, sc, device, bg, dpix)
    _, _, lb = _gpu_run(cam, sc, device, bg, dpix)
    for k in la:
        assert torch.equal(la[k].grad, lb[k].grad), k


def test_mark_visible(oracle, device):
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = gs_scenes.identity_camera(64, 64)
    sc = gs_scenes.random_gaussians(3000, 0, cam=cam, seed=14)
    sc.means3D[::3, 2] *= -1
    s = gs_scenes.raster_settings_for(cam, 0, device=device)
    vis = GaussianRasterizer(s).markVisible(sc.means3D.to(device)).cpu().numpy()
    ref = oracle.mark_visible(sc.means3D.numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy())
    np.testing.assert_array_equal(vis, ref)


@pytest.mark.parametrize("P", [4, 100, 5000])
def test_knn_matches_oracle(oracle, device, P):
    from simple_knn._C import distCUDA2

    g = torch.Generator().manual_seed(P)
    pts = torch.randn((P, 3), generator=g) * torch.tensor([3.0, 1.0, 0.5])
    got = distCUDA2(pts.to(device)).cpu().numpy()
    ref = oracle.knn_mean_dist2(pts.numpy())
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("P,ball", [(1_000_000, False), (1_000_000, True), (5_000_000, False)],
                         ids=["C3_1M_frustum", "C4_1M_ball", "C5_5M_frustum"])
def test_knn_init_scale_vs_kdtree(device, P, ball):
    """distCUDA2 at the size GaussianModel.create_from_pcd calls it (scene/gaussian_model.py:134: the
    whole initial point cloud): exact 3-NN mean squared distance of 20k sampled points against a
    scipy k-d tree over all P points (fp64 distances of the same fp32 coordinates; rtol 1e-6), and
    the call's time."""
    from scipy.spatial import cKDTree

    from simple_knn._C import distCUDA2

    cam = gs_scenes.identity_camera(1920, 1080)
    sc = gs_scenes.random_gaussians(P, 0, cam=None if ball else cam, seed=11, ball_radius=2.0 if ball else None)
    pts = sc.means3D
    dp = pts.to(device)
    distCUDA2(dp)  # warm-up (first-call allocations)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    got = distCUDA2(dp)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    got = got.cpu().numpy()
    x = pts.numpy().astype(np.float64)
    tree = cKDTree(x)
    q = np.random.default_rng(P).choice(P, 20_000, replace=False)
    d, _ = tree.query(x[q], k=4)  # the point itself first (distance 0)
    ref = (d[:, 1:] ** 2).mean(axis=1)
    np.testing.assert_allclose(got[q], ref, rtol=1e-6, atol=0)
    assert np.isfinite(got).all() and (got > 0).all()
    print(f"\n[distCUDA2 P={P} {'ball' if ball else 'frustum'}] {ms:.2f} ms")


@pytest.mark.parametrize("P", [1_000_000, 5_000_000], ids=["C3_1M", "C5_5M"])
def test_large_c3_properties(device, P):
    """C3 / C5 sizes (1M / 5M Gaussians SH3, 1920x1080) -- size-independent properties instead of
    the oracle: the tile-sorted list is ordered by (tile, depth, index), ranges tile the list
    exactly, n_contrib <= list length, image finite, bit-identical reruns.  C5 (I = 21.6M) also
    covers the sort chunks of several 2048-key tiles per workgroup (I > 8.4M: no first-pass
    counts from the duplicate) and the large-scene ordering path."""
    from diff_gaussian_rasterization import _C

    cam = gs_scenes.identity_camera(1920, 1080)
    sc = gs_scenes.random_gaussians(P, 3, cam=cam, seed=0).to(device)
    s = gs_scenes.raster_settings_for(cam, 3, device=device)
    e = torch.Tensor([])
    args = (s.bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, s.viewmatrix, s.projmatrix,
            s.tanfovx, s.tanfovy, 1080, 1920, sc.shs, 3, s.campos, False, False)
    num, color, radii, geom, binb, imgb = _C.rasterize_gaussians(*args)
    num2, color2, radii2, *_ = _C.rasterize_gaussians(*args)
    assert num == num2 and torch.equal(color, color2) and torch.equal(radii, radii2)
    ex = _C.debug_export(sc.P, 1920, 1080, num, geom, binb, imgb, device)
    if P > 1_000_000:
        assert num > 8_400_000  # the multi-tile sort chunks are exercised
    lst = ex["point_list"].long()
    rng = ex["ranges"].long()
    assert num == int(ex["tiles_touched"].sum())
    # ranges partition [0, num) in tile order
    nonempty = rng[:, 1] > rng[:, 0]
    starts, ends = rng[nonempty, 0], rng[nonempty, 1]
    assert starts[0] == 0 and ends[-1] == num and torch.all(starts[1:] == ends[:-1])
    # inside each tile: (depth bits, gid) non-decreasing
    depth_bits = ex["depth"].view(torch.int32).long()
    tile_of = torch.repeat_interleave(torch.arange(rng.shape[0], device=device)[nonempty], ends - starts)
    same = tile_of[1:] == tile_of[:-1]
    d0, d1 = depth_bits[lst[:-1]], depth_bits[lst[1:]]
    ordered = (d1 > d0) | ((d1 == d0) & (lst[1:] > lst[:-1]))
    assert torch.all(ordered[same])
    ncon = ex["n_contrib"].long()
    assert torch.isfinite(color).all() and (color >= 0).all()
    assert int(ncon.max()) <= int((ends - starts).max())


def test_large_scene_sort_path_vs_oracle(oracle, device):
    """More than 1,048,576 Gaussians take the large-scene ordering path (tile counts carried
    through the depth sort, 3-launch offsets scan; gs_forward.hip fwd_order).  A small image keeps
    the oracle quick; a third of the Gaussians sit behind the camera (dropped by the first pass)."""
    W, H = 320, 240
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(1_100_000, 1, cam=cam, seed=21)
    sc.means3D[::3, 2] = -sc.means3D[::3, 2]
    bg = np.zeros(3, np.float32)
    osc = _oracle_scene(oracle, cam, sc, bg)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=22).numpy()
    _, _, leaves = _gpu_run(cam, sc, device, bg, dpix)
    _check_backward(oracle.backward(osc, dpix), leaves)


def _random_case(seed, oracle):
    """One randomized configuration: camera pose, ragged image size, P, SH degree (active <= max),
    background, scale modifier, precomputed colours / covariances, scale range."""
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.integers(17, 300)), int(rng.integers(13, 220))
    fovy = float(rng.uniform(35.0, 80.0))
    pos = rng.normal(size=3) * rng.uniform(0.0, 2.0)
    tgt = pos + np.array([0.0, 0.0, 4.0]) + rng.normal(size=3) * 0.8
    cam = gs_scenes.look_at_camera(tuple(pos), tuple(tgt), W, H, fovy)
    P = int(rng.integers(1, 6000))
    deg_max = int(rng.integers(0, 4))
    deg = int(rng.integers(0, deg_max + 1))
    lo = float(rng.uniform(0.002, 0.02))
    sc = gs_scenes.random_gaussians(P, deg_max, cam=cam, seed=2000 + seed, scale_range=(lo, lo * rng.uniform(2, 12)),
                                    z_range=(float(rng.uniform(0.5, 3.0)), float(rng.uniform(4.0, 20.0))))
    bg = rng.random(3).astype(np.float32) * (rng.random() < 0.5)
    mod = float(rng.uniform(0.5, 1.5)) if rng.random() < 0.5 else 1.0
    colors = rng.random((P, 3), dtype=np.float32) if rng.random() < 0.25 else None
    cov = None
    if rng.random() < 0.25:
        cov = np.ascontiguousarray(oracle.cov3d(sc.scales.numpy(), mod, sc.rotations.numpy()))
    return cam, sc, bg, mod, deg, colors, cov


@pytest.mark.parametrize("seed", range(24))
def test_randomized_configurations_vs_oracle(oracle, device, seed):
    """Randomized cameras (off-axis poses, FoV 35-80 deg, ragged image sizes), scene sizes, active /
    max SH degree, background, scale modifier and precomputed colour / covariance inputs, in the
    exact numerics mode: image and radii bit-exact against the oracle (plus every forward
    intermediate when scale_modifier is 1), every gradient at the 1e-5 contract, the covariance
    chain included (round 6: measured max 4.4e-7 of the max over the 24 cases; the chain bound was
    1e-4 through round 5)."""
    cam, sc, bg, mod, deg, colors, cov = _random_case(seed, oracle)
    W, H = cam.image_width, cam.image_height
    cov_mod = 1.0 if cov is not None else mod  # a precomputed covariance already carries the modifier
    osc = _oracle_scene(oracle, cam, sc, bg, colors=colors, cov3D=cov, deg=deg, mod=cov_mod)
    ofw = oracle.forward(osc, intermediates=True)
    ofw["bg"] = bg
    if cov_mod == 1.0:
        _check_forward_exact(ofw, cam, sc, device, colors=colors, cov3D=cov, deg=deg)
    dpix = gs_scenes.dl_dimage(H, W, seed=seed, scale=1.0).numpy()
    img, radii, leaves = _gpu_run(cam, sc, device, bg, dpix, colors=colors, cov3D=cov, deg=deg, mod=cov_mod)
    np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    gr = oracle.backward(osc, dpix)
    _check_backward(gr, leaves, colors=colors, cov3D=cov)
    _check_chain_noise(leaves, gr, oracle.backward_f32_acc(osc, dpix))


@pytest.mark.parametrize("deg,M", [(3, 16), (1, 16), (2, 9)])
def test_sh_split_matches_concatenated_rows(device, fast_mode, deg, M):
    """GaussianRasterizer(..., sh_split=(features_dc, features_rest)) reads the two tensors in place
    (gs_forward_preprocess_split / gs_backward_accumulate_split): image, radii and every gradient are
    bit-identical to the call on cat(features_dc, features_rest), in the default numerics mode; the
    carrier's .grad is dL/d cat(...), [P, M, 3]."""
    from diff_gaussian_rasterization import GaussianRasterizer

    W, H = 320, 240
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(20_000, 3, cam=cam, seed=31)
    d = sc.to(device)
    g = torch.Generator().manual_seed(32)
    shs_full = torch.randn((sc.P, M, 3), generator=g).mul_(0.3).to(device)
    dc, rest = shs_full[:, :1].contiguous(), shs_full[:, 1:].contiguous()
    s = gs_scenes.raster_settings_for(cam, deg, bg=torch.tensor([0.1, 0.2, 0.3], device=device), device=device)
    dpix = gs_scenes.dl_dimage(H, W, seed=33).to(device)

    def run(split):
        leaves = [t.clone().requires_grad_(True) for t in (d.means3D, d.opacities, d.scales, d.rotations)]
        m2 = torch.zeros_like(d.means3D, requires_grad=True)
        shs = (torch.empty((sc.P, M, 3), device=device) if split else shs_full.clone()).requires_grad_(True)
        img, radii = GaussianRasterizer(s)(means3D=leaves[0], means2D=m2, opacities=leaves[1], shs=shs,
                                           scales=leaves[2], rotations=leaves[3],
                                           sh_split=(dc, rest) if split else None)
        img.backward(dpix)
        torch.cuda.synchronize()
        return img.detach(), radii, [t.grad for t in leaves + [m2, shs]]

    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert x.shape == y.shape and torch.equal(x, y), k


def test_sh_split_rejects_bad_carriers(device):
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    cam = gs_scenes.identity_camera(64, 48)
    sc = gs_scenes.random_gaussians(100, 3, cam=cam, seed=1).to(device)
    s = gs_scenes.raster_settings_for(cam, 3, device=device)
    dc, rest = sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous()
    r = GaussianRasterizer(s)
    kw = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, scales=sc.scales,
              rotations=sc.rotations)
    with pytest.raises(RuntimeError, match="carrier"):
        r(shs=torch.empty((100, 9, 3), device=device), sh_split=(dc, rest), **kw)
    pv = prepare_views([r], sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    with pytest.raises(RuntimeError, match="prepared"):
        r(shs=sc.shs, sh_split=(dc, rest), prepared=pv[0], **kw)
