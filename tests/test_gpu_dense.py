"""GPU parity against an independent reference: the HIP path (fp32, the library's default numerics)
against tests/dense_ref.py -- a dense PyTorch restatement of the spec in
fp64, differentiated by autograd, composited Gaussian by Gaussian over each tile rectangle on the
same GPU (dense_ref.render_local) -- at thousands of Gaussians.  Neither the C oracle nor the
kernels' hand-derived backward enter this comparison.

Where a decision of the per-pixel loop sits at its threshold (alpha vs 1/255, the tested T vs 1e-4,
power vs 0) fp32 and fp64 may decide differently; the reference flags those pixels (relative 1e-5
of the threshold) and they are left out of the image check; the backward runs with dL/dpix zeroed
there (a pixel with dL/dpix = 0 adds nothing to any gradient, whatever it decided), and a Gaussian
whose fp32 radius differs from the fp64 one (which moves its rectangle) is left out of the gradient
checks.  The counts are bounded and printed.  Bounds: the image and the
opacity and colour (SH or precomputed) gradients 1e-5 * |ref| + 1e-5 * max|ref|.  The
screen-position gradient and the covariance chain behind it (means2D, means3D, scales, rotations,
cov3D) sum terms with cancellation over hundreds of pixels, each term carrying the T recovered by
repeated division, so fp32 itself moves them by about 1e-5 of their max: they get 1e-5 * |ref| +
5e-5 * max|ref| (round 4, tile-wave backward: the largest measured is 2.5e-5, dmeans3D of the
scale_modifier case, where the dense fp32 run deviates as much) and, as the conditioning check, a
max deviation within 4x that of the same dense reference evaluated in fp32 (one other valid fp32
order), plus 1e-5 of the max."""
import pytest
import torch

import dense_cases
import dense_ref
import gs_scenes
from gpu_checks import check_4x, check_tol

pytestmark = pytest.mark.gpu

CHAIN = ("means2D", "means3D", "scales", "rotations", "cov3D")


def _dense(cam, leaves, W, H, bg, deg, mod, dtype, device, flag_rel=1e-5, flag_T_rel=None):
    """dense_ref.render_local on copies of `leaves` in `dtype` (their grads by autograd)."""
    t = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
    res = dense_ref.render_local(
        t["means3D"], t["means2D"], t["opacities"], *dense_cases.dense_args(cam, device, dtype), bg.to(dtype), shs=t.get("shs"), deg=deg, colors=t.get("colors"),
        scales=t.get("scales"), rots=t.get("rotations"), cov3D=t.get("cov3D"), mod=mod, flag_rel=flag_rel,
        flag_T_rel=flag_T_rel)
    return t, res


def _run_and_compare(cam, leaves, W, H, bg, deg=0, mod=1.0, seed=0, device=None, chain_frac=5e-5, flag_rel=1e-5,
                     flag_T_rel=None, noise_check=True):
    from diff_gaussian_rasterization import GaussianRasterizer

    P = leaves["means3D"].shape[0]
    dpix = gs_scenes.dl_dimage(H, W, seed=seed + 1, scale=1.0).to(device)
    # the HIP path, fp32, as the reference adapter calls it
    s = gs_scenes.raster_settings_for(cam, deg, bg=bg, scale_modifier=mod, device=device)
    hip = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    kw = {"shs": hip.get("shs"), "colors_precomp": hip.get("colors"), "scales": hip.get("scales"),
          "rotations": hip.get("rotations"), "cov3D_precomp": hip.get("cov3D")}
    img, radii = GaussianRasterizer(s)(means3D=hip["means3D"], means2D=hip["means2D"], opacities=hip["opacities"],
                                       **{k: v for k, v in kw.items() if v is not None})
    # the dense reference on the same GPU, fp64 (the reference) and fp32 (what fp32 alone does)
    ref, (rimg, rradii, flag) = _dense(cam, leaves, W, H, bg, deg, mod, torch.float64, device, flag_rel,
                                       flag_T_rel)
    r32, (img32, _, _) = _dense(cam, leaves, W, H, bg, deg, mod, torch.float32, device)

    # Gaussians whose radius (and so tile rectangle) differs between fp32 and fp64
    rdiff = (radii.cpu() != rradii.cpu()).numpy()
    assert rdiff.mean() <= 1e-3, f"{int(rdiff.sum())} radii differ"
    fl = flag.cpu().numpy()
    with torch.no_grad():
        q = dense_ref._prep(ref["means3D"], ref["means2D"], ref["opacities"],
                            *dense_cases.dense_args(cam, device, torch.float64), shs=ref.get("shs"), deg=deg,
                            colors=ref.get("colors"), scales=ref.get("scales"), rots=ref.get("rotations"),
                            cov3D=ref.get("cov3D"), mod=mod)
    dense_cases.wide_mask(q["rect"].numpy(), rdiff, W, H, into=fl)
    print(f"\n[dense] flagged pixels {int(fl.sum())}/{fl.size}, radii differing {int(rdiff.sum())}/{P}")
    assert fl.mean() <= 0.02
    # the backward runs with dL/dpix zeroed at the flagged pixels: a pixel with dL/dpix = 0 adds
    # nothing to any gradient, so a decision that fp32 and fp64 take differently there changes none
    keep_px = torch.from_numpy(~fl).to(device)
    dpm = dpix * keep_px[None]
    (img * dpm).sum().backward()
    (rimg * dpm.double()).sum().backward()
    (img32 * dpm).sum().backward()
    torch.cuda.synchronize()
    keep_g = ~rdiff

    check_tol(img.permute(1, 2, 0), rimg.permute(1, 2, 0), "image", ~fl)
    for k in hip:
        if k not in CHAIN:
            check_tol(hip[k].grad, ref[k].grad, f"d{k}", keep_g)
            continue
        check_tol(hip[k].grad, ref[k].grad, f"d{k}", keep_g, frac=chain_frac)
        check_4x(hip[k].grad, ref[k].grad, r32[k].grad, f"d{k}", keep_g, enforce=noise_check)


CASES = [(2000, 3, 192, 128, 0.0, 41, None), (6000, 2, 320, 200, 0.3, 42, None),
         # deeper overlap (scales up to 0.08): long walks, T-stop decisions
         (12000, 3, 400, 256, 0.0, 43, (0.01, 0.08))]


@pytest.mark.parametrize("P,deg,W,H,bgv,seed,scale_range", CASES,
                         ids=["2k_sh3_192x128", "6k_sh2_320x200_bg", "12k_sh3_400x256_deep"])
def test_hip_vs_dense_autograd_reference(device, P, deg, W, H, bgv, seed, scale_range):
    cam = gs_scenes.identity_camera(W, H)
    kw = {} if scale_range is None else {"scale_range": scale_range}
    d = gs_scenes.random_gaussians(P, deg, cam=cam, seed=seed, **kw).to(device)
    leaves = {k: getattr(d, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    leaves["means2D"] = torch.zeros_like(d.means3D)
    _run_and_compare(cam, leaves, W, H, torch.full((3,), bgv, device=device), deg=deg, seed=seed, device=device)


def test_hip_vs_dense_precomputed_colors_and_cov3d(device):
    """colors_precomp and cov3D_precomp (upper-triangular xx, xy, xz, yy, yz, zz) instead of SH and
    scale / rotation, a coloured background."""
    W, H, P = 256, 160, 4000
    cam = gs_scenes.identity_camera(W, H)
    d = gs_scenes.random_gaussians(P, 0, cam=cam, seed=44).to(device)
    g = torch.Generator(device=device).manual_seed(45)
    with torch.no_grad():
        R = dense_ref.quat_R(d.rotations)
        L = R * d.scales[:, None, :]
        S = L @ L.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
    leaves = dict(means3D=d.means3D, means2D=torch.zeros_like(d.means3D), opacities=d.opacities,
                  colors=torch.rand((P, 3), device=device, generator=g), cov3D=cov)
    _run_and_compare(cam, leaves, W, H, torch.tensor([0.1, 0.2, 0.3], device=device), seed=44, device=device)


def test_hip_vs_dense_scale_modifier(device):
    """scale_modifier 0.7 on SH1 rows."""
    W, H, P = 256, 160, 4000
    cam = gs_scenes.identity_camera(W, H)
    d = gs_scenes.random_gaussians(P, 1, cam=cam, seed=46).to(device)
    leaves = {k: getattr(d, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    leaves["means2D"] = torch.zeros_like(d.means3D)
    _run_and_compare(cam, leaves, W, H, torch.zeros(3, device=device), deg=1, mod=0.7, seed=46, device=device)


def test_hip_vs_dense_large_and_needle_splats(device):
    """tests/test_gpu_parity.py's large-splat scene with needles (one axis / 60): 60 splats spanning
    dozens of tiles among 3000 small ones.
    The forward decisions are less well conditioned here too: a needle's falloff is a quadratic form
    with large, nearly cancelling conic terms (power carries ~1e-4 relative fp32 error), and the
    large splats are opaque (alpha up to the 0.99 clamp, where one ulp of alpha is 1e-5 of 1 - alpha,
    so T drifts ~1e-4 relative along a walk): alpha decisions within 2e-4 and T-stop decisions
    within 1e-3 (relative) of their thresholds are flagged.  Every Gaussian, needles included, is
    held to the fixed bounds -- for the covariance chain 1e-3 of max (measured, round 4: means3D /
    scales 4.9e-5 / 8.1e-5, rotations 5.4e-4 of max); the 4x-of-dense-fp32
    check is left out here: the kernels follow
    upstream's covariance-backward formulas, whose fp32 conditioning on needles differs from that of
    the autograd graph the dense fp32 run differentiates (against the oracle's own fp32 order they
    stay within 4x, tests/test_gpu_parity.py::test_needle_splats_conditioning)."""
    W, H = 640, 360
    cam = gs_scenes.identity_camera(W, H)
    small = gs_scenes.random_gaussians(3000, 2, cam=cam, seed=21)
    big = gs_scenes.random_gaussians(60, 2, cam=cam, seed=22, scale_range=(0.3, 1.5), z_range=(2.0, 4.0))
    big.scales[::3, 0] /= 60.0
    d = gs_scenes.concat_scenes(small, big).to(device)
    leaves = {k: getattr(d, k) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    leaves["means2D"] = torch.zeros_like(d.means3D)
    _run_and_compare(cam, leaves, W, H, torch.tensor([0.1, 0.2, 0.3], device=device), deg=2, seed=23, device=device,
                     flag_rel=2e-4, flag_T_rel=1e-3, chain_frac=1e-3, noise_check=False)
