"""The photometric loss (gs_loss, csrc/gs_loss.hip) in plain torch with autograd, in any float dtype:
the reference of tests/test_gpu_loss.py.

It is the 2-D formulation of oracle/ssim_oracle.py (the float32 window of window1d, its 11 x 11 outer
product, five zero-padded depthwise conv2d, C1 = 0.01^2, C2 = 0.03^2, the mean of the SSIM map),
evaluated wholly in `dtype`:

    loss = (1 - lam) mean|img - gt| + lam (1 - mean(ssim_map))

Run in float64 it is the exact reference and reproduces ssim_oracle bit for bit; in float32 it is
what the reference project's own arithmetic gives, the measure of what fp32 can give on the content
(the conditioning term of the GPU tests' bound)."""
import torch
import torch.nn.functional as F

from oracle import ssim_oracle


def ssim_map(x, y, size=11):
    """SSIM map [B, C, H, W] of x, y [B, C, H, W], in their dtype."""
    C = x.shape[1]
    w1 = ssim_oracle.window1d(size).to(x.dtype)
    w = (w1[:, None] @ w1[None, :]).expand(C, 1, size, size).contiguous()
    pad = size // 2
    conv = lambda t: F.conv2d(t, w, padding=pad, groups=C)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = conv(x * x) - mu1_sq
    s2 = conv(y * y) - mu2_sq
    s12 = conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def reference(img, gt, lam, dtype, weights=None):
    """(loss, l1, ssim, ssim_map, grad) as CPU tensors of `dtype`, img and gt [C, H, W] or [B, C, H, W].

    weights None: ssim is the mean of the map and grad = d loss / d img; with lam None the loss is
    the SSIM value itself (grad = d ssim / d img).
    weights (one per image, [B, C, H, W] only): ssim is the per-image means [B] (size_average=False)
    and grad = d (weights . ssim).sum() / d img; loss is that sum."""
    a = img.detach().to("cpu", dtype).requires_grad_(True)
    b = gt.detach().to("cpu", dtype)
    x, y = (a[None], b[None]) if a.dim() == 3 else (a, b)
    l1 = torch.abs(a - b).mean()  # before the map, as train.py orders the two terms (autograd sums in that order)
    m = ssim_map(x, y)
    if weights is not None:
        s = m.mean(1).mean(1).mean(1)
        loss = (torch.as_tensor(weights, dtype=dtype) * s).sum()
    else:
        s = m.mean()
        loss = s if lam is None else (1.0 - lam) * l1 + lam * (1.0 - s)
    loss.backward()
    return loss.detach(), l1.detach(), s.detach(), m.detach().reshape(a.shape), a.grad
