"""The aux outputs' surface that needs no GPU: the header, the three C-ABI symbols, the sizing
function and the public argument."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gsrast.h")).read()


def test_header_defines_has_aux_and_keeps_abi_17():
    h = _header()
    assert re.search(r"^#define GSRAST_HAS_AUX 1\b", h, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", h).group(1)) == 17
    for name in ("gs_grad_buffer_bytes_aux", "gs_forward_render_aux", "gs_backward_accumulate_aux"):
        assert re.search(r"\b%s\(" % name, h), name


def test_aux_symbols_load():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_abi_version() == 17
    for name in ("gs_grad_buffer_bytes_aux", "gs_forward_render_aux", "gs_backward_accumulate_aux"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize("n,P", [(0, 0), (1, 1), (63, 1000), (1_000_000, 3), (3_000_000, 1_000_000),
                                 (12_345_678, 2_000_001)])
def test_grad_buffer_bytes_aux_holds_the_two_arrays(n, P):
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_grad_buffer_bytes_aux(n, P) >= lib.gs_grad_buffer_bytes(n) + 4 * (n + P)


def test_forward_has_aux_outputs_argument():
    from diff_gaussian_rasterization import GaussianRasterizer

    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert "aux_outputs" in p and p["aux_outputs"].default is False


def test_aux_outputs_with_cpu_tensors_raises_the_device_error():
    import gs_scenes
    from diff_gaussian_rasterization import GaussianRasterizer

    cam = gs_scenes.identity_camera(32, 32)
    sc = gs_scenes.random_gaussians(5, 0, cam=cam, seed=1)
    s = gs_scenes.raster_settings_for(cam, 0, device="cpu")
    with pytest.raises(RuntimeError, match="needs device tensors"):
        GaussianRasterizer(s)(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities,
                              shs=sc.shs, scales=sc.scales, rotations=sc.rotations, aux_outputs=True)
