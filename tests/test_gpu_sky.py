"""The skysphere background (gs_sky, csrc/gs_sky.hip) on the GPU against tests/sky_ref.py.

Seeded inputs: color and texture uniform in [0, 1], alpha uniform in [0, 1] with 10 % of the pixels
exactly 0 and 10 % exactly 1, g = dL/dimage standard normal.  Shapes (image W x H, texture Hs x Ws):

    A  identity_camera(200, 120), 32 x 64: edge blocks with lanes outside the image; every block sums
       through its LDS box
    B  look_at_camera((0.3, 0.2, -1), (0.1, -5, 0.2), 72, 40), 16 x 32: the row-0 pole is in view, rows
       clamp, boxes that span the whole circle (box columns wider than the texture wrap onto one texel)
    C  look_at_camera((0, 0, 0), (0.02, 0.1, -3), 200, 120, fovy 100), 33 x 67 (odd): the atan2 seam
       crosses the image, columns wrap; the six seam blocks exceed the box and add straight to memory
    D  identity_camera(41, 23), 256 x 512: a texture much finer than the image, no block's box fits
       (all direct atomics); 3 H W is not a multiple of 4 (the max-reduction's scalar tail)

(tests/test_sky_cpu.py checks on the CPU which blocks of A-D take which path.)

1. image, dL/dalpha and dL/dtexture against the fp64 reference, every pixel and texel:
   max|hip - f64| <= 4 max|ref f32 - f64| + 1e-5 max|f64| per tensor (the conditioning rule of
   tests/test_gpu_dense.py), ref f32 the same torch code in fp32 on the CPU.  Measured on MI355X:
   every tensor within 0.19 of its bound (D's dL/dtexture; the HIP error is about that of ref f32).
2. Two backward runs give bit-identical gradients; accumulate_texture = 1 on a pre-filled buffer
   equals pre + (write-mode result) in fp32, bit for bit.
3. Exact cases: alpha == 1, None inputs, a constant texture, single gradients.
4. The ray convention against the rasterizer's projection (one small Gaussian on a pixel's ray).
5. End to end through render_with_sky, gradients into the rasterizer, FusedAdam on the texture.
6. A timing record at 1920 x 1080 with a 1024 x 2048 texture (no assertion on time).
"""
import ctypes
import os

import pytest
import torch

import gs_scenes
from gpu_checks import check_4x
import sky_ref

pytestmark = pytest.mark.gpu

CASES = {
    "A": (lambda: gs_scenes.identity_camera(200, 120), 32, 64),
    "B": (lambda: gs_scenes.look_at_camera((0.3, 0.2, -1.0), (0.1, -5.0, 0.2), 72, 40), 16, 32),
    "C": (lambda: gs_scenes.look_at_camera((0, 0, 0), (0.02, 0.1, -3.0), 200, 120, fovy_deg=100.), 33, 67),
    "D": (lambda: gs_scenes.identity_camera(41, 23), 256, 512),
}

_INPUTS = {}
_REFS = {}


def _inputs(name, device):
    """(settings, color, alpha [H, W], texture, g) of a case, on the device; built once."""
    if name not in _INPUTS:
        make_cam, Hs, Ws = CASES[name]
        cam = make_cam()
        H, W = cam.image_height, cam.image_width
        gen = torch.Generator().manual_seed(1234 + ord(name))
        color = torch.rand((3, H, W), generator=gen)
        alpha = torch.rand((H, W), generator=gen)
        pick = torch.rand((H, W), generator=gen)
        alpha = torch.where(pick < 0.1, torch.zeros(()), torch.where(pick > 0.9, torch.ones(()), alpha))
        tex = torch.rand((3, Hs, Ws), generator=gen)
        g = torch.randn((3, H, W), generator=gen)
        s = gs_scenes.raster_settings_for(cam, 0, device=device)
        _INPUTS[name] = (s,) + tuple(t.to(device) for t in (color, alpha, tex, g))
    return _INPUTS[name]


def _refs(name, device):
    """{dtype: (image, dL/dalpha, dL/dtexture)} of a case from the torch reference on the CPU; built once."""
    if name not in _REFS:
        s, color, alpha, tex, g = _inputs(name, device)
        _REFS[name] = {dt: sky_ref.reference(color, alpha, tex, g, s.viewmatrix, s.tanfovx, s.tanfovy, dt)
                       for dt in (torch.float64, torch.float32)}
    return _REFS[name]


def _hip(s, color, alpha, tex, g, color_grad=True, alpha_grad=True, tex_grad=True):
    """One compose + backward of sum g image; (image, color.grad, alpha.grad, tex.grad)."""
    import gs_sky

    c = None if color is None else color.detach().clone().requires_grad_(color_grad)
    a = None if alpha is None else alpha.detach().clone().requires_grad_(alpha_grad)
    t = tex.detach().clone().requires_grad_(tex_grad)
    img = gs_sky.compose(c, a, t, s)
    if img.requires_grad:
        (img * g).sum().backward()
    torch.cuda.synchronize()
    return img.detach(), None if c is None else c.grad, None if a is None else a.grad, t.grad


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _abi_backward(s, alpha, tex, g, want_alpha=True, want_tex=True, accumulate=0, into=None):
    """gs_sky_compose_backward called directly: (dL/dalpha, dL/dtexture)."""
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    H, W = int(s.image_height), int(s.image_width)
    Hs, Ws = tex.shape[1], tex.shape[2]
    dev = tex.device
    dalpha = torch.full((H, W), float("nan"), device=dev) if want_alpha else None
    dtex = (into if into is not None else torch.full_like(tex, float("nan"))) if want_tex else None
    scratch = torch.empty((lib.gs_sky_scratch_bytes(Hs, Ws),), dtype=torch.uint8, device=dev).fill_(0xA5)
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
    view = s.viewmatrix.contiguous()
    _native.check(lib.gs_sky_compose_backward(W, H, p(view), s.tanfovx, s.tanfovy, Hs, Ws, p(tex), p(alpha), p(g),
                                              p(dalpha), p(dtex), accumulate, p(scratch),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "sky backward")
    torch.cuda.synchronize()
    return dalpha, dtex


# ---- 1. against the fp64 reference ----
@pytest.mark.parametrize("name", list(CASES))
def test_matches_fp64_reference(name, device):
    s, color, alpha, tex, g = _inputs(name, device)
    ref = _refs(name, device)
    img, dcolor, dalpha, dtex = _hip(s, color, alpha, tex, g)
    for tensor, got, k in (("image", img, 0), ("dL_dalpha", dalpha, 1), ("dL_dtexture", dtex, 2)):
        check_4x(got, ref[torch.float64][k], ref[torch.float32][k], f"sky {name} {tensor}")
    assert torch.equal(dcolor, g)
    # alpha as the rasterizer returns it, [1, H, W]: same bits, gradient in that shape
    img1, _, dalpha1, dtex1 = _hip(s, color, alpha[None], tex, g)
    assert dalpha1.shape == (1,) + tuple(alpha.shape)
    assert torch.equal(_bits(img1), _bits(img)) and torch.equal(_bits(dalpha1[0]), _bits(dalpha))
    assert torch.equal(_bits(dtex1), _bits(dtex))


# ---- 2. determinism ----
@pytest.mark.parametrize("name", list(CASES))
def test_backward_is_bitwise_reproducible(name, device):
    s, color, alpha, tex, g = _inputs(name, device)
    da1, dt1 = _abi_backward(s, alpha, tex, g)
    da2, dt2 = _abi_backward(s, alpha, tex, g)
    assert torch.isfinite(da1).all() and torch.isfinite(dt1).all()
    assert torch.equal(_bits(da1), _bits(da2)) and torch.equal(_bits(dt1), _bits(dt2))
    # the autograd path runs the same call
    _, _, da3, dt3 = _hip(s, color, alpha, tex, g)
    assert torch.equal(_bits(da1), _bits(da3)) and torch.equal(_bits(dt1), _bits(dt3))
    # accumulate_texture = 1: fp32 old + new
    pre = torch.randn(tex.shape, generator=torch.Generator().manual_seed(5)).to(device)
    _, acc = _abi_backward(s, alpha, tex, g, want_alpha=False, accumulate=1, into=pre.clone())
    assert torch.equal(_bits(acc), _bits(pre + dt1))


def test_non_finite_gradients_stay_in_bounds_and_reproducible(device):
    """inf / NaN in dL/dimage: the values are meaningless, the run completes and repeats itself"""
    s, color, alpha, tex, g = _inputs("C", device)
    bad = g.clone()
    bad[0, 5, 7] = float("inf")
    bad[1, 60, 100] = float("nan")
    bad[2, 119, 199] = -float("inf")
    _, dt1 = _abi_backward(s, alpha, tex, bad, want_alpha=False)
    _, dt2 = _abi_backward(s, alpha, tex, bad, want_alpha=False)
    assert torch.equal(_bits(dt1), _bits(dt2))


# ---- 3. NULL variants and exact cases ----
def test_opaque_pixels_keep_the_colour_bits(device):
    s, color, alpha, tex, g = _inputs("C", device)
    img, _, dalpha, dtex = _hip(s, color, torch.ones_like(alpha), tex, g)
    assert torch.equal(_bits(img), _bits(color))
    assert torch.count_nonzero(dtex) == 0
    assert torch.count_nonzero(dalpha) > 0


@pytest.mark.parametrize("name", ["B", "C"])
def test_render_is_compose_with_zeros(name, device):
    import gs_sky

    s, color, alpha, tex, g = _inputs(name, device)
    sky = gs_sky.SkySphere(tex.shape[1], tex.shape[2]).to(device)
    with torch.no_grad():
        sky.texture.copy_(tex)
    bare = sky.render(s)
    (bare * g).sum().backward()
    img, _, _, dtex = _hip(s, torch.zeros_like(color), torch.zeros_like(alpha), tex, g)
    assert torch.equal(_bits(bare), _bits(img))
    assert torch.equal(_bits(sky.texture.grad), _bits(dtex))
    # one of the two given
    only_c = gs_sky.compose(color, None, tex, s)
    assert torch.equal(_bits(only_c), _bits(_hip(s, color, torch.zeros_like(alpha), tex, g)[0]))
    only_a = gs_sky.compose(None, alpha, tex, s)
    assert torch.equal(_bits(only_a), _bits(_hip(s, torch.zeros_like(color), alpha, tex, g)[0]))


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_constant_texture(name, device):
    s, color, alpha, tex, g = _inputs(name, device)
    c = 0.7310585975646973
    img, _, _, _ = _hip(s, color, alpha, torch.full_like(tex, c), g)
    want = color + (1 - alpha) * c
    assert (img - want).abs().max().item() <= 4 * 2.0 ** -24 * abs(c)


@pytest.mark.parametrize("name", ["A", "C"])
def test_single_gradients(name, device):
    s, color, alpha, tex, g = _inputs(name, device)
    _, _, dalpha, dtex = _hip(s, color, alpha, tex, g)
    _, dc, da, dt = _hip(s, color, alpha, tex, g, tex_grad=False)
    assert dt is None and torch.equal(_bits(da), _bits(dalpha)) and torch.equal(dc, g)
    _, dc, da, dt = _hip(s, color, alpha, tex, g, alpha_grad=False)
    assert da is None and torch.equal(_bits(dt), _bits(dtex))
    _, dc, da, dt = _hip(s, color, alpha, tex, g, color_grad=False, alpha_grad=False)
    assert dc is None and da is None and torch.equal(_bits(dt), _bits(dtex))
    _, dc, da, dt = _hip(s, color, alpha, tex, g, alpha_grad=False, tex_grad=False)
    assert da is None and dt is None and torch.equal(dc, g)


def test_shape_and_dtype_errors(device):
    import gs_sky

    s, color, alpha, tex, g = _inputs("B", device)
    for bad in ((color[:, :-1], alpha, tex), (color, alpha[:, :-1], tex), (color, alpha, tex[:2]),
                (color.double(), alpha, tex), (color, alpha.half(), tex), (color, alpha, tex.double())):
        with pytest.raises(ValueError):
            gs_sky.compose(*bad, s)


# ---- 4. the ray convention against the rasterizer's projection ----
@pytest.mark.parametrize("name,x,y", [("B", 50, 11), ("C", 150, 30), ("C", 21, 97)])
def test_ray_of_a_pixel_meets_the_projection(name, x, y, device):
    import gs_sky
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = CASES[name][0]()
    s = gs_scenes.raster_settings_for(cam, 0, device=device)
    d = gs_sky.pixel_directions(s)[y, x]
    mean = (s.campos + 3.0 * d / d.norm())[None].contiguous()
    one = lambda *v: torch.tensor([v], dtype=torch.float32, device=device)  # noqa: E731
    _, radii, _, alpha = GaussianRasterizer(s)(means3D=mean, means2D=torch.zeros_like(mean), opacities=one(0.99),
                                               colors_precomp=one(1.0, 1.0, 1.0), scales=one(0.01, 0.01, 0.01),
                                               rotations=one(1.0, 0.0, 0.0, 0.0), aux_outputs=True)
    assert int(radii[0]) > 0
    k = int(alpha[0].argmax())
    assert (k // cam.image_width, k % cam.image_width) == (y, x)


# ---- 5. end to end ----
class _Recorder(torch.nn.Module):
    """a rasterizer that keeps its colour and alpha outputs, with their gradients"""

    def __init__(self, rasterizer):
        super().__init__()
        self.rasterizer = rasterizer
        self.raster_settings = rasterizer.raster_settings

    def forward(self, **kw):
        out = self.rasterizer(**kw)
        self.color, self.alpha = out[0], out[3]
        self.color.retain_grad()
        self.alpha.retain_grad()
        return out


def test_render_with_sky_end_to_end(device):
    import gs_sky
    import gs_train
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = CASES["A"][0]()
    sc = gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41).to(device)
    s = gs_scenes.raster_settings_for(cam, 3, device=device)
    leaves = {k: getattr(sc, k).clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    sky = gs_sky.SkySphere(32, 64).to(device)
    with torch.no_grad():
        sky.texture.copy_(_inputs("A", device)[3])
    g = _inputs("A", device)[4]
    rec = _Recorder(GaussianRasterizer(s))
    image, radii, invdepth, alpha = gs_sky.render_with_sky(
        rec, sky, means3D=leaves["means3D"], means2D=torch.zeros_like(leaves["means3D"]), opacities=leaves["opacities"],
        shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
    assert image.shape == (3, cam.image_height, cam.image_width) and alpha is rec.alpha
    assert bool((alpha == 0).any()) and bool((alpha > 0.5).any()), "the scene must show bare sky and splats"
    (image * g).sum().backward()
    torch.cuda.synchronize()
    args = (rec.color, rec.alpha, sky.texture, g, s.viewmatrix, s.tanfovx, s.tanfovy)
    f64, f32 = sky_ref.reference(*args, torch.float64), sky_ref.reference(*args, torch.float32)
    check_4x(image, f64[0], f32[0], "sky e2e image")
    check_4x(rec.alpha.grad[0], f64[1], f32[1], "sky e2e dL_dalpha")
    check_4x(sky.texture.grad, f64[2], f32[2], "sky e2e dL_dtexture")
    assert torch.equal(rec.color.grad, g)
    og = leaves["opacities"].grad
    assert torch.isfinite(og).all() and torch.count_nonzero(og) > 0
    # one optimizer step on the texture: FusedAdam's generic path against torch.optim.Adam
    twin = torch.nn.Parameter(sky.texture.detach().clone())
    twin.grad = sky.texture.grad.clone()
    before = sky.texture.detach().clone()
    gs_train.FusedAdam([{"params": [sky.texture], "lr": 1e-2}]).step()
    torch.optim.Adam([{"params": [twin], "lr": 1e-2}]).step()
    torch.cuda.synchronize()
    assert not torch.equal(sky.texture.detach(), before)
    assert (sky.texture - twin).abs().max().item() <= 1e-6 * twin.abs().max().item()


# ---- 6. timing record ----
def test_timing_record_1080p(device):
    """forward + backward at 1920 x 1080 with a 1024 x 2048 texture: the fused path and the torch fp32
    reference on the GPU (what a user writes without gs_sky).  Recorded, not asserted."""
    import gs_sky

    cam = gs_scenes.identity_camera(1920, 1080)
    s = gs_scenes.raster_settings_for(cam, 0, device=device)
    gen = torch.Generator().manual_seed(7)
    color = torch.rand((3, 1080, 1920), generator=gen).to(device).requires_grad_(True)
    alpha = torch.rand((1080, 1920), generator=gen).to(device).requires_grad_(True)
    tex = torch.rand((3, 1024, 2048), generator=gen).to(device).requires_grad_(True)
    g = torch.randn((3, 1080, 1920), generator=gen).to(device)

    def fused():
        return gs_sky.compose(color, alpha, tex, s)

    def glue():
        return sky_ref.compose(color, alpha, tex, s.viewmatrix, s.tanfovx, s.tanfovy, torch.float32)

    def time_ms(fn, warm=5, iters=50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(warm + iters):
            if k == warm:
                a.record()
            color.grad = alpha.grad = tex.grad = None
            out = fn()
            out.backward(g)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters, out.detach()

    t_fused, out_fused = time_ms(fused)
    grads_fused = [t.grad.clone() for t in (color, alpha, tex)]
    t_glue, out_glue = time_ms(glue)
    text = (f"sky compose forward + backward, 1920x1080, texture 1024x2048, mean of 50:\n"
            f"fused HIP  {t_fused:.3f} ms\ntorch fp32 {t_glue:.3f} ms\n")
    print(text)
    if os.environ.get("GS_SKY_TIMING"):  # a file to keep the record in (as GS_PARITY_REPORT for the parity figures)
        with open(os.environ["GS_SKY_TIMING"], "w") as f:
            f.write(text)
    assert torch.isfinite(out_fused).all() and torch.isfinite(out_glue).all()
    assert all(torch.isfinite(t).all() for t in grads_fused)
