"""What the GPU test files share (imported by name; not a conftest): the library handle, the numerics-mode
fixtures, the two acceptance rules and the bitwise comparison.  Both rules write their bound and the
measured figures to the parity report (tests/parity_report.py)."""
import numpy as np
import pytest
import torch

import parity_report

RTOL = 1e-5


def lib():
    from diff_gaussian_rasterization import _native

    return _native.load()


@pytest.fixture(params=[1, 0], ids=["exact", "fast"])
def mode(request):
    """Both numerics modes; the previous one is restored."""
    prev = lib().gs_set_exact_exp(request.param)
    yield request.param
    lib().gs_set_exact_exp(prev)


@pytest.fixture
def exact_mode():
    """The bit-exact numerics mode; the previous one is restored."""
    prev = lib().gs_set_exact_exp(1)
    yield
    lib().gs_set_exact_exp(prev)


@pytest.fixture
def fast_mode(exact_mode):
    """The fast mode inside a module that runs in exact_mode (which restores)."""
    lib().gs_set_exact_exp(0)
    yield


def to_np(x, keep=None):
    """float64 numpy copy of a tensor or array, restricted to `keep` (an index or mask) if given."""
    x = x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)
    return x if keep is None else x[keep]


def check_tol(got, ref, name, keep=None, rtol=RTOL, frac=RTOL, times=1):
    """the element-wise rule: |got - ref| <= times (rtol |ref| + frac max|ref|)"""
    got, ref = to_np(got, keep), to_np(ref, keep)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(np.abs(ref).max(initial=0.0))
    d = np.abs(got - ref)
    tol = times * (rtol * np.abs(ref) + frac * scale)
    parity_report.record(name, got, ref, times * rtol, times * frac)
    print(f"{name}: max|d| {d.max(initial=0.0):.3e}  max|ref| {scale:.3e}  "
          f"({float((d / np.maximum(tol, 1e-300)).max(initial=0.0)):.3f} of the bound)")
    bad = d > tol
    if bad.any():
        detail = "; ".join(f"{tuple(int(x) for x in i)}: got {got[tuple(i)]:.6e} ref {ref[tuple(i)]:.6e} "
                           f"tol {tol[tuple(i)]:.2e}" for i in np.argwhere(bad)[:5])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.size} beyond tol; max|d| {d.max():.3e} "
                             f"max|ref| {scale:.3e}; first: {detail}")


def check_4x(got, ref, f32, name, keep=None, enforce=True):
    """the conditioning rule: max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|f64|, and `got` finite
    (enforce=False: the figures are printed only; the report holds asserted bounds)"""
    g, r, n = to_np(got, keep), to_np(ref, keep), to_np(f32, keep)
    d_gpu, d_32, scale = np.abs(g - r).max(initial=0.0), np.abs(n - r).max(initial=0.0), np.abs(r).max(initial=0.0)
    bound = 4.0 * d_32 + RTOL * scale
    if scale > 0 and enforce:
        parity_report.record(name, g, r, 0.0, bound / scale)
    plain = float((np.abs(n - r) / (RTOL * np.abs(r) + RTOL * scale)).max(initial=0.0)) if scale > 0 else 0.0
    print(f"  {name}: max|hip - f64| {d_gpu:.3e}  max|dense f32 - f64| {d_32:.3e}  max|f64| {scale:.3e}  "
          f"bound {bound:.3e}  (hip {d_gpu / scale if scale else 0.0:.2e}, dense f32 {d_32 / scale if scale else 0.0:.2e} "
          f"of max; {d_gpu / bound if bound > 0 else 0.0:.2f} of the bound; dense f32 at {plain:.2f} of "
          f"1e-5 |ref| + 1e-5 max)")
    assert np.isfinite(g).all(), name
    assert d_gpu <= bound or not enforce, (name, d_gpu, d_32, scale)
