"""The camera gradients' surface that needs no GPU: the header, the two C-ABI symbols, the scratch
sizing, the order of gs_backward_camera's checks, the public argument, and a self-check of the fp64
reference the GPU tests compare against.

Scratch layout: one row of 28 doubles per workgroup of 256 Gaussians (the 27 sums, 12 view + 12 proj
+ 3 campos, and a zero so that a row is 14 whole 16-byte pairs), at least one row:
    gs_camera_grad_scratch_bytes(P) = 28 * 8 * max(1, ceil(P / 256)).
"""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_camera_grad_scratch_bytes", "gs_backward_camera")


def test_header_defines_has_camera_grad_and_keeps_abi_17():
    h = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"^#define GSRAST_HAS_CAMERA_GRAD 1\b", h, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", h).group(1)) == 17
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, h), name


def test_camera_symbols_load():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_abi_version() == 17
    for name in SYMBOLS:
        assert name in _native.SIGNATURES and hasattr(lib, name), name


def test_scratch_bytes_formula_and_monotonic():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    prev = 0
    for P in (0, 1, 255, 256, 257, 65_536, 65_793, 1_000_000, 5_000_000):
        n = lib.gs_camera_grad_scratch_bytes(P)
        rows = max(1, (P + 255) // 256)
        assert n == 28 * 8 * rows, (P, n)
        assert n >= 27 * 8 * ((P + 255) // 256) and n >= prev, (P, n, prev)
        prev = n
    assert lib.gs_camera_grad_scratch_bytes(-5) == lib.gs_camera_grad_scratch_bytes(0)


def test_forward_has_camera_grads_argument():
    from diff_gaussian_rasterization import GaussianRasterizer

    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert "camera_grads" in p and p["camera_grads"].default is False


# ---- the order of gs_backward_camera's checks (the table idiom of tests/test_api_contract_cpu.py) ----
_BUF = (ctypes.c_float * 64)()  # 16-byte aligned host words; never dereferenced by a row
X = ctypes.cast(_BUF, ctypes.c_void_p)
ODD = ctypes.c_void_p(X.value + 4)
PARAMS = ("P D M bg W H means3D shs colors opac scales scale_modifier rots cov3D view proj campos tan_fovx tan_fovy "
          "geom num_rendered aux_grad_buffer aux_valid scratch dview dproj dcampos debug stream").split()
DEFAULTS = dict(P=4, D=3, M=16, W=16, H=16, scale_modifier=1.0, tan_fovx=0.5, tan_fovy=0.5, num_rendered=10,
                aux_grad_buffer=None, aux_valid=0, colors=None, cov3D=None, debug=0, stream=None)
E_P = "P must be >= 0"
E_SIZE = "image size must be positive (got %d x %d)"
E_IN = "missing required input pointer"
E_COL = "Please provide excatly one of either SHs or precomputed colors!"
E_COV = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
E_DEG = "SH degree must be in [0, 3] (got %d)"
E_CAMPOS = "campos is required with SHs"
E_GRAD = "missing gradient output pointer"
E_BUF = "missing buffer pointer"
E_ALIGN = "camera grad: scratch must be 16-byte aligned"
E_NR = "num_rendered out of range"
# every row has a fault in front of the first device call; rows with two faults pin which check is first
ROWS = [
    (dict(P=-1, W=0), E_P),
    (dict(W=0, geom=None), E_SIZE % (0, 16)),
    (dict(H=-2, dview=None), E_SIZE % (16, -2)),
    (dict(P=0, W=0), E_SIZE % (0, 16)),
    (dict(P=0, dview=None, means3D=None), E_GRAD),  # an empty scene still writes (zeros): outputs first
    (dict(means3D=None, dview=None), E_IN),
    (dict(opac=None, geom=None), E_BUF),  # as the backward: the opacities are not needed
    (dict(view=None, geom=None), E_IN),
    (dict(proj=None), E_IN),
    (dict(bg=None), E_IN),
    (dict(colors=X, dproj=None), E_COL),
    (dict(shs=None), E_COL),
    (dict(cov3D=X, geom=None), E_COV),
    (dict(D=4, geom=None), E_DEG % 4),
    (dict(campos=None, dview=None), E_CAMPOS),
    (dict(dview=None, geom=None), E_GRAD),
    (dict(dproj=None, scratch=ODD), E_GRAD),
    (dict(geom=None, scratch=ODD), E_BUF),
    (dict(scratch=None, num_rendered=-1), E_BUF),
    (dict(aux_valid=1, num_rendered=-1), E_BUF),  # aux_valid without the aux grad buffer
    (dict(scratch=ODD, num_rendered=-1), E_ALIGN),
    (dict(num_rendered=-1, dcampos=None), E_NR),
    (dict(num_rendered=1 << 31), E_NR),
    # precomputed colours: D, M and campos are not looked at
    (dict(shs=None, colors=X, campos=None, D=9, M=0, geom=None), E_BUF),
]


@pytest.mark.parametrize("over,text", ROWS, ids=[f"{i:02d}-" + ",".join(r[0]) for i, r in enumerate(ROWS)])
def test_backward_camera_early_return(over, text):
    from diff_gaussian_rasterization import _native

    assert not set(over) - set(PARAMS)
    assert len(PARAMS) == len(_native.SIGNATURES["gs_backward_camera"][1])
    lib = _native.load()
    args = [over[n] if n in over else DEFAULTS.get(n, X) for n in PARAMS]
    assert lib.gs_backward_camera(*args) == 1
    assert lib.gs_last_error().decode() == text


# ---- the reference's own consistency (fp64, CPU) ----
def test_reference_translation_identity_and_structural_zeros():
    """Moving every Gaussian by e equals moving the camera by -e: with view, proj and campos as
    independent leaves, sum_i dL/dmeans3D_i[r] = sum_k view[r][k] gV[3][k] + sum_c proj[r][c] gP[3][c]
    - gC[r].  Measured 3.7e-16 relative on this scene; held to 1e-10, a sanity bound on the
    reference far below every fp32 bound.  view column 3 and proj column 2 never enter the render:
    their gradients are exactly 0."""
    import dense_ref
    import gs_scenes

    W, H, P, deg = 64, 48, 60, 3
    f = torch.float64
    cam = gs_scenes.look_at_camera((0.7, -0.4, -1.1), (0.1, 0.2, 4.0), W, H)
    sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=3, scale_range=(0.05, 0.3))
    t = {k: getattr(sc, k).to(f).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    view = cam.world_view_transform.to(f).contiguous().requires_grad_(True)
    proj = cam.full_proj_transform.to(f).contiguous().requires_grad_(True)
    campos = cam.camera_center.to(f).contiguous().requires_grad_(True)
    img, radii = dense_ref.render(t["means3D"], torch.zeros((P, 3), dtype=f), t["opacities"], view, proj, campos,
                                  math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H, torch.zeros(3, dtype=f),
                                  shs=t["shs"], deg=deg, scales=t["scales"], rots=t["rotations"])
    assert int((radii > 0).sum()) >= 30
    (img * gs_scenes.dl_dimage(H, W, seed=4, scale=1.0).to(f)).sum().backward()
    gV, gP, gC = view.grad, proj.grad, campos.grad
    lhs = t["means3D"].grad.sum(0)
    rhs = view.detach()[:3, :3] @ gV[3, :3] + proj.detach()[:3, :] @ gP[3, :] - gC
    scale = float(lhs.abs().max())
    assert scale > 0
    print(f"translation identity: max|lhs - rhs| / max|lhs| = {float((lhs - rhs).abs().max()) / scale:.3e}")
    assert float((lhs - rhs).abs().max()) <= 1e-10 * scale
    assert torch.equal(gV[:, 3], torch.zeros(4, dtype=f))
    assert torch.equal(gP[:, 2], torch.zeros(4, dtype=f))
    assert float(gV.abs().max()) > 0 and float(gP.abs().max()) > 0 and float(gC.abs().max()) > 0
