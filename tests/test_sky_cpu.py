"""The skysphere's surface that needs no GPU: the header, the three C-ABI symbols and their
argument checks (they fail on the host, before any GPU call), the public module's errors, the
ray convention of gs_sky.pixel_directions, and the fp64 reference's own gradients."""
import ctypes
import math
import os
import re

import pytest
import torch

import gs_scenes
import sky_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_sky_scratch_bytes", "gs_sky_compose_forward", "gs_sky_compose_backward")


def test_header_defines_has_sky_and_keeps_abi_17():
    h = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"^#define GSRAST_HAS_SKY 1\b", h, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", h).group(1)) == 17
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, h), name


def test_sky_symbols_load():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_abi_version() == 17
    for name in SYMBOLS:
        assert name in _native.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize("Hs,Ws", [(1, 1), (4, 8), (33, 67), (1024, 2048)])
def test_scratch_holds_a_64_bit_sum_per_texel_value(Hs, Ws):
    from diff_gaussian_rasterization import _native

    n = _native.load().gs_sky_scratch_bytes(Hs, Ws)
    assert n >= 8 * 3 * Hs * Ws + 4 and n % 16 == 0


def test_bad_arguments_fail_on_the_host():
    """Non-zero return and a message, with fake non-NULL pointers that a GPU call would fault on."""
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every case below is refused by the host checks
    fwd_ok = dict(W=8, H=6, view=p, Hs=4, Ws=8, tex=p, color=None, alpha=None, out=p)
    for change, text in (({"W": 0}, "image size"), ({"H": -1}, "image size"), ({"Hs": 0}, "texture size"),
                         ({"Ws": 0}, "texture size"), ({"view": None}, "missing pointer"),
                         ({"tex": None}, "missing pointer"), ({"out": None}, "missing pointer")):
        a = dict(fwd_ok, **change)
        rc = lib.gs_sky_compose_forward(a["W"], a["H"], a["view"], 0.5, 0.5, a["Hs"], a["Ws"], a["tex"], a["color"],
                                        a["alpha"], a["out"], None)
        assert rc != 0 and text in _native.last_error(), (change, _native.last_error())
    bwd_ok = dict(W=8, H=6, view=p, Hs=4, Ws=8, tex=p, g=p, dalpha=p, dtex=p, scratch=p)
    for change, text in (({"W": 0}, "image size"), ({"H": 0}, "image size"), ({"Hs": -3}, "texture size"),
                         ({"Ws": 0}, "texture size"), ({"view": None}, "missing pointer"),
                         ({"tex": None}, "missing pointer"), ({"g": None}, "missing pointer"),
                         ({"scratch": None}, "scratch"), ({"scratch": ctypes.c_void_p(72)}, "16-byte")):
        a = dict(bwd_ok, **change)
        rc = lib.gs_sky_compose_backward(a["W"], a["H"], a["view"], 0.5, 0.5, a["Hs"], a["Ws"], a["tex"], None, a["g"],
                                         a["dalpha"], a["dtex"], 0, a["scratch"], None)
        assert rc != 0 and text in _native.last_error(), (change, _native.last_error())
    # nothing requested: nothing to do, and no scratch needed
    assert lib.gs_sky_compose_backward(8, 6, p, 0.5, 0.5, 4, 8, p, None, p, None, None, 0, None, None) == 0


def test_compose_on_cpu_tensors_raises():
    import gs_sky

    cam = gs_scenes.identity_camera(8, 6)
    s = gs_scenes.raster_settings_for(cam, 0, device="cpu")
    tex = torch.rand(3, 4, 8)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        gs_sky.compose(torch.rand(3, 6, 8), torch.rand(6, 8), tex, s)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        gs_sky.SkySphere(4, 8).render(s)


def test_render_with_sky_refuses_a_background_colour():
    import gs_sky

    cam = gs_scenes.identity_camera(8, 6)
    s = gs_scenes.raster_settings_for(cam, 0, bg=torch.tensor([0.0, 0.5, 0.0]), device="cpu")

    class Rasterizer:
        raster_settings = s

        def __call__(self, **kw):
            raise AssertionError("the rasterizer must not run")

    with pytest.raises(ValueError, match="bg must be all zeros"):
        gs_sky.render_with_sky(Rasterizer(), gs_sky.SkySphere(4, 8))


@pytest.mark.parametrize("cam", [gs_scenes.identity_camera(8, 6),
                                 gs_scenes.look_at_camera((0.3, 0.2, -1.0), (0.1, -5.0, 0.2), 72, 40)],
                         ids=["identity", "look_at"])
def test_pixel_directions_match_the_reference(cam):
    import gs_sky

    s = gs_scenes.raster_settings_for(cam, 0, device="cpu")
    d = gs_sky.pixel_directions(s)
    H, W = cam.image_height, cam.image_width
    assert d.shape == (H, W, 3) and d.dtype == torch.float32
    ref = sky_ref.directions(s.viewmatrix, s.tanfovx, s.tanfovy, W, H, torch.float64)
    assert (d.double() - ref).abs().max() <= 8 * 2.0 ** -24 * ref.abs().max()
    # the ray of pixel (x, y) projects back onto (x, y): p = campos + 3 d through full_proj_transform
    p = cam.camera_center.double() + 3.0 * ref
    ph = torch.cat([p, torch.ones(H, W, 1, dtype=torch.float64)], -1) @ cam.full_proj_transform.double()
    ndc = ph[..., :2] / ph[..., 3:]
    pix_x = ((ndc[..., 0] + 1) * W - 1) / 2
    pix_y = ((ndc[..., 1] + 1) * H - 1) / 2
    assert (pix_x - torch.arange(W, dtype=torch.float64)[None, :]).abs().max() < 1e-4
    assert (pix_y - torch.arange(H, dtype=torch.float64)[:, None]).abs().max() < 1e-4


def test_identity_camera_looks_down_plus_z_with_row_zero_up():
    """The centre of an identity camera's image samples the middle of the texture (u = 0.5 at +z,
    v = 0.5 at the horizon), and rays above the centre (smaller y: world -y) land in smaller rows."""
    cam = gs_scenes.identity_camera(9, 7)
    d = sky_ref.directions(cam.world_view_transform, 0.5, 0.5, 9, 7)
    xa, xb, ya, yb, fx, fy = sky_ref.taps(d, 16, 32)
    assert xa[3, 4] == 15 and xb[3, 4] == 16 and abs(float(fx[3, 4]) - 0.5) < 1e-9
    assert ya[3, 4] == 7 and yb[3, 4] == 8 and abs(float(fy[3, 4]) - 0.5) < 1e-9
    assert ya[0, 4] < ya[6, 4] and xa[3, 0] < xa[3, 8]


def test_gpu_shapes_cover_both_scatter_paths():
    """The backward sums a 16 x 16 block through an LDS copy of its texel box when the box holds at
    most 256 texels and adds straight to memory otherwise (csrc/gs_sky.hip).  The shapes of
    tests/test_gpu_sky.py: A all boxed, D none, C both; B and C see the seam, B the row-0 pole."""
    from test_gpu_sky import CASES

    seen = {}
    for name, (make_cam, Hs, Ws) in CASES.items():
        cam = make_cam()
        H, W = cam.image_height, cam.image_width
        d = sky_ref.directions(cam.world_view_transform, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H)
        xa, xb, ya, yb, fx, fy = sky_ref.taps(d, Hs, Ws)
        x0 = torch.where((xa == Ws - 1) & (xb == 0), torch.full_like(xa, -1), xa)  # unwrapped left column
        boxed = []
        for by in range(0, H, 16):
            for bx in range(0, W, 16):
                X, A, B = (t[by:by + 16, bx:bx + 16] for t in (x0, ya, yb))
                boxed.append(int((X.max() + 1 - X.min() + 1) * (B.max() - A.min() + 1)) <= 256)
        seen[name] = (sum(boxed), len(boxed), bool((xa == Ws - 1).any() and (xa == 0).any()), int(ya.min()))
    assert seen["A"][0] == seen["A"][1]
    assert seen["D"][0] == 0
    assert 0 < seen["C"][0] < seen["C"][1]
    assert seen["B"][2] and seen["C"][2] and not seen["A"][2]
    assert seen["B"][3] == 0


def test_fp64_reference_passes_gradcheck():
    cam = gs_scenes.look_at_camera((0.3, 0.2, -1.0), (0.1, -5.0, 0.2), 8, 6)
    g = torch.Generator().manual_seed(3)
    color = torch.rand(3, 6, 8, generator=g, dtype=torch.float64, requires_grad=True)
    alpha = torch.rand(6, 8, generator=g, dtype=torch.float64, requires_grad=True)
    tex = torch.rand(3, 4, 8, generator=g, dtype=torch.float64, requires_grad=True)
    tfx, tfy = 0.5 * 8 / 6, 0.5

    def f(c, a, t):
        return sky_ref.compose(c, a, t, cam.world_view_transform, tfx, tfy, torch.float64)

    assert torch.autograd.gradcheck(f, (color, alpha, tex), eps=1e-6, atol=1e-7)
