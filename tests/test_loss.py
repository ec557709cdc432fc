"""Fused SSIM / L1 (gs_loss, csrc/gs_loss.hip) against the reference loss
(/root/reference/utils/loss_utils.py via tests/golden/loss_golden.npz) and the fp64 CPU
restatement oracle/ssim_oracle.py.

Tolerances: the oracle is float64 and pinned to the reference's float32 outputs at 2e-6 (value)
and 1e-5 relative + 1e-5 x max (gradient); the HIP kernels compute in float32 with a separable
window, checked against the oracle at 2e-6 (value) and 1e-5 relative + 1e-5 x max (gradient).
Those figures hold on the high-variance content used here (rand against rand + 0.1 noise, windowed
variances about 0.08).  On smooth, near-converged content E[x^2] - m^2, A2 - A1 and 1/B1 - 1/B2 cancel
in float32 and the reference's own float32 formulation misses them by a factor of 30 and more (up to
7e-3 x max in the gradient, 3.4e-4 in the value); there the contract is the conditioning rule of
tests/test_gpu_loss.py, max|hip - f64| <= 4 max|ref f32 - f64| + 1e-5 max|f64|, of which the kernels
use at most 0.37 (gradient) and 0.21 (value) on MI355X, and an exactly 0 gradient where the image
equals the target."""
import numpy as np
import pytest
import torch

from oracle import ssim_oracle

G = np.load(__file__.rsplit("/", 1)[0] + "/golden/loss_golden.npz")
CASES = ["chw", "bchw", "tiny"]


def _close(a, b, rtol=1e-5, frac=1e-5, name=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = rtol * np.abs(b) + frac * max(np.abs(b).max(), 1e-30)
    assert (np.abs(a - b) <= tol).all(), f"{name}: max|d| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}"


def test_window_matches_reference():
    np.testing.assert_array_equal(ssim_oracle.window1d().numpy(), G["window1d"])


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference_golden(case):
    a = torch.tensor(G[f"{case}_img1"], requires_grad=True)
    b = torch.tensor(G[f"{case}_img2"])
    s = ssim_oracle.ssim(a, b)
    s.backward()
    assert abs(s.item() - float(G[f"{case}_ssim"])) < 2e-6
    _close(a.grad.numpy(), G[f"{case}_grad"], name="grad")
    assert abs(ssim_oracle.l1_loss(a, b).item() - float(G[f"{case}_l1"])) < 1e-6
    if f"{case}_ssim_per_image" in G.files:
        a3 = torch.tensor(G[f"{case}_img1"], requires_grad=True)
        s3 = ssim_oracle.ssim(a3, b, size_average=False)
        s3.sum().backward()
        np.testing.assert_allclose(s3.detach().numpy(), G[f"{case}_ssim_per_image"], atol=2e-6)
        _close(a3.grad.numpy(), G[f"{case}_grad_per_image_sum"], name="grad per image")


def test_gs_loss_window_and_cpu_refusal():
    import gs_loss

    np.testing.assert_array_equal(np.array(list(gs_loss._WIN), np.float32), G["window1d"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        gs_loss.ssim(torch.rand(3, 8, 8), torch.rand(3, 8, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_ssim_matches_reference_golden(case, device):
    import gs_loss

    a = torch.tensor(G[f"{case}_img1"], device=device, requires_grad=True)
    b = torch.tensor(G[f"{case}_img2"], device=device)
    s = gs_loss.ssim(a, b)
    s.backward()
    assert abs(s.item() - float(G[f"{case}_ssim"])) < 2e-6
    _close(a.grad.cpu().numpy(), G[f"{case}_grad"], name="grad")
    if f"{case}_ssim_per_image" in G.files:
        a3 = torch.tensor(G[f"{case}_img1"], device=device, requires_grad=True)
        s3 = gs_loss.ssim(a3, b, size_average=False)
        s3.sum().backward()
        np.testing.assert_allclose(s3.detach().cpu().numpy(), G[f"{case}_ssim_per_image"], atol=2e-6)
        _close(a3.grad.cpu().numpy(), G[f"{case}_grad_per_image_sum"], name="grad per image")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 270, 480), (2, 3, 64, 80), (3, 1080, 1920), (3, 5, 7), (3, 1, 40)])
def test_gpu_ssim_matches_oracle(shape, device):
    """Including the full 1080p frame of train.py (16x16 tiles, ragged borders)."""
    import gs_loss

    g = torch.Generator().manual_seed(5)
    a0 = torch.rand(shape, generator=g)
    b0 = (a0 + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    ref_a = a0.clone().requires_grad_(True)
    ref = ssim_oracle.ssim(ref_a, b0)
    ref.backward()
    a = a0.to(device).requires_grad_(True)
    s = gs_loss.ssim(a, b0.to(device))
    (2.5 * s).backward()
    assert abs(s.item() - ref.item()) < 2e-6
    _close(a.grad.cpu().numpy() / 2.5, ref_a.grad.numpy(), name="grad")
    l1 = gs_loss.l1_loss(a, b0.to(device))
    assert abs(l1.item() - ssim_oracle.l1_loss(a0, b0).item()) < 1e-6


def test_photometric_loss_cpu_refusal():
    import gs_loss

    with pytest.raises(RuntimeError, match="no CPU path"):
        gs_loss.photometric_loss(torch.rand(3, 8, 8), torch.rand(3, 8, 8))


def _oracle_photometric(a0, b0, lam):
    ref_a = a0.clone().requires_grad_(True)
    l1 = ssim_oracle.l1_loss(ref_a, b0)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim_oracle.ssim(ref_a, b0))
    loss.backward()
    return loss.item(), l1.item(), ref_a.grad.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lam", [((3, 270, 480), 0.2), ((2, 3, 64, 80), 0.2), ((3, 1080, 1920), 0.2),
                                       ((3, 37, 53), 0.7), ((1, 16, 16), 0.0), ((3, 20, 21), 1.0),
                                       ((3, 5, 7), 0.2), ((3, 1, 40), 0.2), ((2, 33, 1), 0.5)])
def test_gpu_photometric_loss_matches_oracle(shape, lam, device):
    """train.py:91-92 fused (gs_loss.photometric_loss) against the fp64 oracle of the same expression:
    value within 2e-6, gradient within 1e-5 relative + 1e-5 x max; pixels with image == gt (L1
    subgradient 0, as torch's abs backward) included."""
    import gs_loss

    g = torch.Generator().manual_seed(11)
    a0 = torch.rand(shape, generator=g)
    b0 = (a0 + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    eq = torch.rand(shape, generator=g) < 0.05
    b0 = torch.where(eq, a0, b0)
    ref_loss, ref_l1, ref_grad = _oracle_photometric(a0, b0, lam)
    a = a0.to(device).requires_grad_(True)
    loss, l1 = gs_loss.photometric_loss(a, b0.to(device), lam)
    assert not l1.requires_grad and loss.requires_grad and loss.dim() == 0
    (3.0 * loss).backward()
    assert abs(loss.item() - ref_loss) < 2e-6 and abs(l1.item() - ref_l1) < 1e-6
    _close(a.grad.cpu().numpy() / 3.0, ref_grad, name="grad")


@pytest.mark.gpu
def test_gpu_photometric_loss_matches_separate_terms(device):
    """The fused expression against gs_loss.l1_loss + gs_loss.ssim composed by torch as train.py does."""
    import gs_loss

    g = torch.Generator().manual_seed(12)
    a0 = torch.rand((3, 130, 170), generator=g).to(device)
    b0 = torch.rand((3, 130, 170), generator=g).to(device)
    a1 = a0.clone().requires_grad_(True)
    Ll1 = gs_loss.l1_loss(a1, b0)
    loss1 = 0.8 * Ll1 + 0.2 * (1.0 - gs_loss.ssim(a1, b0))
    loss1.backward()
    a2 = a0.clone().requires_grad_(True)
    loss2, Ll2 = gs_loss.photometric_loss(a2, b0, 0.2)
    loss2.backward()
    assert abs(loss1.item() - loss2.item()) <= 1e-6 * abs(loss1.item())
    assert abs(Ll1.item() - Ll2.item()) <= 1e-6 * abs(Ll1.item())
    _close(a2.grad.cpu().numpy(), a1.grad.cpu().numpy(), rtol=1e-5, frac=1e-6, name="grad")


def test_partial_count():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    assert lib.gs_ssim_partial_count(1, 32, 32) == 1
    assert lib.gs_ssim_partial_count(1, 33, 32) == 2
    assert lib.gs_ssim_partial_count(3, 1080, 1920) == 6120


def test_loss_abi_validation_without_gpu():
    """The argument checks of the four C entries; placeholder pointers, every call returns before a launch."""
    import ctypes

    from diff_gaussian_rasterization import _native

    lib = _native.load()
    fake = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(6)]
    win = ctypes.cast((ctypes.c_float * 11)(*[1.0 / 11] * 11), ctypes.c_void_p)

    def calls(planes, H, W, ptrs):
        w, a, b, c, d, e = ptrs
        return {"ssim": lambda: lib.gs_ssim_forward(planes, H, W, w, a, b, c, d, e, None),
                "photometric loss": lambda: lib.gs_photometric_loss_forward(planes, H, W, w, a, b, 0.2, c, d, e, None),
                "photometric loss ": lambda: lib.gs_photometric_loss_backward(planes, H, W, w, a, b, c, 0.2, d, e, None)}

    every = [win] + fake[:5]
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, -3, 8), (2, 8, -3)):
        for name, call in calls(*shape, every).items():
            assert call() != 0, (name, shape)
            assert _native.last_error() == f"{name.strip()}: empty image", (name, shape)
    for k in range(6):
        ptrs = list(every)
        ptrs[k] = None
        for name, call in calls(2, 8, 8, ptrs).items():
            assert call() != 0, (name, k)
            assert _native.last_error() == f"{name.strip()}: missing pointer", (name, k)

    def backward(planes, channels, H, W, ptrs=every):
        return lib.gs_ssim_backward(planes, channels, H, W, *ptrs, None)

    for bad in ((6, 0, 8, 8), (6, -3, 8, 8), (6, 4, 8, 8), (2, 3, 8, 8), (0, 3, 8, 8), (6, 3, 0, 8), (6, 3, 8, 0),
                (6, 3, -1, 8), (6, 3, 8, -1)):
        assert backward(*bad) != 0, bad
        assert _native.last_error() == "ssim: bad shape", bad
    for k in range(6):
        ptrs = list(every)
        ptrs[k] = None
        assert backward(6, 3, 8, 8, ptrs) != 0, k
        assert _native.last_error() == "ssim: missing pointer", k


@pytest.mark.parametrize("case", CASES)
def test_loss_ref_matches_oracle_and_golden(case):
    """tests/loss_ref.py, the reference of tests/test_gpu_loss.py: in float64 it is ssim_oracle bit for
    bit, in float32 (the reference project's own arithmetic) it meets the goldens' tolerance."""
    import loss_ref

    a0, b0 = torch.tensor(G[f"{case}_img1"]), torch.tensor(G[f"{case}_img2"])
    a = a0.double().requires_grad_(True)  # a float64 leaf: the oracle's gradient unrounded
    s = ssim_oracle.ssim(a, b0)
    s.backward()
    loss, l1, val, smap, grad = loss_ref.reference(a0, b0, None, torch.float64)
    assert smap.shape == a0.shape and grad.dtype == torch.float64
    assert val.item() == s.item() and loss.item() == s.item() and torch.equal(grad, a.grad)
    assert l1.item() == ssim_oracle.l1_loss(a0, b0).item()
    assert smap.mean().item() == s.item()
    want_loss, want_l1, want_grad = _oracle_photometric(a0.double(), b0, 0.2)
    loss, l1, _, _, grad = loss_ref.reference(a0, b0, 0.2, torch.float64)
    assert loss.item() == want_loss and l1.item() == want_l1 and np.array_equal(grad.numpy(), want_grad)
    if a0.dim() == 4:
        w = [1.0, -2.5, 0.25][:a0.shape[0]]
        a3 = a0.double().requires_grad_(True)
        s3 = ssim_oracle.ssim(a3, b0, size_average=False)
        (s3 * torch.tensor(w, dtype=torch.float64)).sum().backward()
        _, _, vals, _, grad = loss_ref.reference(a0, b0, None, torch.float64, weights=w)
        assert torch.equal(vals, s3.detach()) and torch.equal(grad, a3.grad)
    loss, l1, val, smap, grad = loss_ref.reference(a0, b0, None, torch.float32)
    assert grad.dtype == torch.float32 and smap.dtype == torch.float32
    assert abs(val.item() - float(G[f"{case}_ssim"])) < 2e-6
    _close(grad.numpy(), G[f"{case}_grad"], name="float32 grad")
    assert abs(l1.item() - float(G[f"{case}_l1"])) < 1e-6
    if f"{case}_ssim_per_image" in G.files:
        B = a0.shape[0]
        _, _, vals, _, grad = loss_ref.reference(a0, b0, None, torch.float32, weights=[1.0] * B)
        np.testing.assert_allclose(vals.numpy(), G[f"{case}_ssim_per_image"], atol=2e-6)
        _close(grad.numpy(), G[f"{case}_grad_per_image_sum"], name="float32 grad per image")
