"""The skysphere's view-matrix gradient, the part that needs no GPU: the header and the two C-ABI
symbols (GSRAST_HAS_SKY_CAMERA), the scratch size, the host checks of
gs_sky_compose_backward_camera in their documented order, and the torch reference
(tests/sky_pose_ref.py) against finite differences."""
import ctypes
import math
import os
import re

import pytest
import torch

import sky_pose_ref
from test_gpu_sky import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_sky_camera_scratch_bytes", "gs_sky_compose_backward_camera")


def test_header_defines_has_sky_camera_and_keeps_abi_17():
    h = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"^#define GSRAST_HAS_SKY_CAMERA 1\b", h, re.M)
    assert re.search(r"^#define GSRAST_HAS_SKY 1\b", h, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", h).group(1)) == 17
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, code), name


def test_symbols_load():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_abi_version() == 17
    for name in SYMBOLS:
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert len(_native.SIGNATURES["gs_sky_compose_backward_camera"][1]) == 18


@pytest.mark.parametrize("W,H", [(1, 1), (16, 16), (17, 1), (41, 23), (200, 120), (1920, 1080), (16385, 3)])
def test_scratch_holds_nine_doubles_per_block(W, H):
    from diff_gaussian_rasterization import _native

    n = _native.load().gs_sky_camera_scratch_bytes(W, H)
    blocks = ((W + 15) // 16) * ((H + 15) // 16)
    assert n % 16 == 0 and n >= 9 * 8 * blocks


def test_scratch_of_a_non_positive_size_is_zero():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    for W, H in ((0, 8), (8, 0), (-1, 8), (8, -3), (0, 0)):
        assert lib.gs_sky_camera_scratch_bytes(W, H) == 0


def test_bad_arguments_fail_on_the_host_in_order():
    """Non-zero return and a message, with fake non-NULL pointers that a GPU call would fault on.
    A call that breaks several checks reports the first of the documented order."""
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(72)  # never dereferenced: every call below ends on the host
    ok = dict(W=8, H=6, view=p, Hs=4, Ws=8, tex=p, g=p, dalpha=p, dtex=p, scratch=p, dview=p, cam=p)

    def call(**change):
        a = dict(ok, **change)
        return lib.gs_sky_compose_backward_camera(a["W"], a["H"], a["view"], 0.5, 0.5, a["Hs"], a["Ws"], a["tex"], None,
                                                  a["g"], a["dalpha"], a["dtex"], 0, a["scratch"], a["dview"], 0,
                                                  a["cam"], None)

    cases = (
        # 1. the checks of gs_sky_compose_backward, each also with the camera scratch missing
        ({"W": 0}, "image size"), ({"H": 0, "cam": None}, "image size"), ({"Hs": -3, "cam": odd}, "texture size"),
        ({"Ws": 0, "scratch": None}, "texture size"), ({"view": None, "cam": None}, "missing pointer"),
        ({"tex": None, "scratch": None}, "missing pointer"), ({"g": None, "cam": odd}, "missing pointer"),
        ({"scratch": None, "cam": None}, "gs_sky_scratch_bytes"), ({"scratch": odd, "cam": None}, "16-byte"),
        ({"scratch": odd, "cam": odd}, "sky: scratch must be"),
        # 2. dL_dviewmatrix without its scratch
        ({"cam": None}, "gs_sky_camera_scratch_bytes"),
        ({"cam": None, "dalpha": None, "dtex": None, "scratch": None}, "gs_sky_camera_scratch_bytes"),
        # 3. its alignment
        ({"cam": odd}, "camera_scratch must be 16-byte aligned"),
        ({"cam": odd, "dtex": None, "scratch": None}, "camera_scratch must be 16-byte aligned"),
    )
    for change, text in cases:
        rc = call(**change)
        assert rc != 0 and text in _native.last_error(), (change, _native.last_error())
    # 4. nothing requested: nothing to do, no scratch needed, whatever the camera scratch is
    for cam in (None, p, odd):
        assert call(dalpha=None, dtex=None, scratch=None, dview=None, cam=cam) == 0
    # without dL_dviewmatrix the camera scratch is not looked at: gs_sky_compose_backward's checks
    assert call(dview=None, cam=odd, scratch=None) != 0 and "gs_sky_scratch_bytes" in _native.last_error()


# ---- the reference ----
def _case(name):
    """(V, tanfovx, tanfovy, W, H, alpha, texture, g, flags) of a case of tests/test_gpu_sky.py in
    fp64 on the CPU, with that file's seeded draws."""
    make_cam, Hs, Ws = CASES[name]
    cam = make_cam()
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(1234 + ord(name))
    torch.rand((3, H, W), generator=gen)  # the colour's draw
    alpha = torch.rand((H, W), generator=gen)
    pick = torch.rand((H, W), generator=gen)
    alpha = torch.where(pick < 0.1, torch.zeros(()), torch.where(pick > 0.9, torch.ones(()), alpha))
    tex = torch.rand((3, Hs, Ws), generator=gen)
    g = torch.randn((3, H, W), generator=gen)
    tfx, tfy = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    fl = sky_pose_ref.flagged(cam.world_view_transform, tfx, tfy, W, H, Hs, Ws)
    return cam.world_view_transform.double(), tfx, tfy, W, H, alpha.double(), tex.double(), g.double(), fl


@pytest.mark.parametrize("name", list(CASES))
def test_flagged_share_stays_under_the_cap(name):
    fl = _case(name)[-1]
    share = float(fl.double().mean())
    print(f"\n[sky pose {name}] flagged {int(fl.sum())}/{fl.numel()} = {100 * share:.2f} %")
    assert share <= sky_pose_ref.FLAG_CAP


@pytest.mark.parametrize("name", list(CASES))
def test_reference_matches_central_differences(name):
    """fp64 autograd of sky_pose_ref against central differences over the nine entries of V, step
    1e-6, with dL/dimage zeroed at the flagged pixels (the flag margin is a thousand steps wide: no
    other pixel changes its cell); row 3 and column 3 are zeros."""
    V, tfx, tfy, W, H, alpha, tex, g, fl = _case(name)
    g = g * (~fl)[None]
    grad = sky_pose_ref.view_grad(alpha, tex, g, V, tfx, tfy, torch.float64)
    assert grad.shape == (4, 4) and not grad[3].any() and not grad[:, 3].any()
    h, fd = 1e-6, torch.zeros(3, 3, dtype=torch.float64)
    with torch.no_grad():
        for i in range(3):
            for j in range(3):
                Vp, Vm = V.clone(), V.clone()
                Vp[i, j] += h
                Vm[i, j] -= h
                fd[i, j] = (sky_pose_ref.loss(alpha, tex, g, Vp, tfx, tfy)
                            - sky_pose_ref.loss(alpha, tex, g, Vm, tfx, tfy)) / (2 * h)
    scale = float(grad.abs().max())
    err = float((fd - grad[:3, :3]).abs().max())
    print(f"\n[sky pose {name}] max|fd - autograd| {err:.3e}  max|autograd| {scale:.3e}")
    assert scale > 0 and err <= 1e-6 * scale
