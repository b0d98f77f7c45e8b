"""Fused L1 + SSIM loss, image metrics (csrc/loss.hip) and Adam (csrc/optim.hip): float64 specifications and the seeded inputs
of test_loss_ref_host.py (which pins them to oracle/losses_ref, oracle/train_ref and the recorded reference values on the CPU),
test_gpu_loss_kernels.py and test_gpu_adam_kernels.py.  Host code only: nothing here touches the GPU.

SSIM: the 1-D Gaussian window is built in float32 exactly as ``make_window`` of loss.hip and
``oracle.losses_ref.gaussian_window_1d`` build it (the kernels take it as given); everything after that is float64.  Zero
padding: border windows are truncated and NOT renormalised.  With S = A1 A2 / (B1 B2),

    A1 = 2 mu1 mu2 + c1,  A2 = 2 s12 + c2,  B1 = mu1^2 + mu2^2 + c1,  B2 = s11 + s22 + c2,
    dS/dmu1 = 2 mu2 (A2 - A1)/(B1 B2) - 2 mu1 S/B1 + 2 mu1 S/B2,   dS/dE[x^2] = -S/B2,   dS/dE[xy] = 2 A1/(B1 B2)

(the three coefficient planes the forward kernel leaves for the backward one; ``coef64``).

Images are (N, H, W): N single-channel planes, as the C entry points take them.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle.losses_ref import gaussian_window_1d

WINDOWS = (3, 5, 7, 9, 11, 13, 15)
# (N, H, W): smaller than the halo, on and beside the tile edges (forward tile 32 x 32, backward tile 32 x 8), several blocks
SHAPES = ((1, 1, 1), (1, 1, 7), (2, 3, 5), (1, 5, 40), (1, 31, 33), (2, 32, 32), (1, 33, 31), (3, 7, 65), (1, 9, 64), (2, 8, 32),
          (1, 64, 96))
EVERY_WINDOW_SHAPES = ((1, 1, 1), (2, 3, 5), (1, 31, 33), (1, 33, 31), (3, 7, 65))      # run with all of WINDOWS in every test
ANTI_SHAPES = ((2, 20, 24), (1, 9, 33))      # anti_pair: batch-mean SSIM -0.64 and -0.44 with the 11-tap window
MIXED_SHAPE = (2, 20, 24)


def cover():
    """The (shape, window) pairs of the tests that do not run the full product: every window at EVERY_WINDOW_SHAPES, the
    reference's window 11 at every shape, and the widest halo (15) at the remaining shapes."""
    pairs = [(s, w) for s in EVERY_WINDOW_SHAPES for w in WINDOWS]
    pairs += [(s, w) for s in SHAPES if s not in EVERY_WINDOW_SHAPES for w in (11, 15)]
    return pairs


def window64(window_size: int, sigma: float) -> torch.Tensor:
    """(1, 1, ws, ws) float64 outer product of the float32 1-D window."""
    g = gaussian_window_1d(window_size, sigma).to(torch.float64)
    return torch.outer(g, g).view(1, 1, window_size, window_size)


def _planes64(t) -> torch.Tensor:
    t = torch.as_tensor(t)
    assert t.dim() == 3, f"expected (N, H, W), got {tuple(t.shape)}"
    return t.detach().to(torch.float64).unsqueeze(1)


def _moments(a, b, window_size, sigma):
    w = window64(window_size, sigma)
    blur = lambda t: F.conv2d(t, w, padding=window_size // 2)      # noqa: E731
    return blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)


def _terms(a, b, window_size, sigma, val_range):
    mu1, mu2, e11, e22, e12 = _moments(a, b, window_size, sigma)
    c1, c2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
    s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return mu1, mu2, 2 * mu1 * mu2 + c1, 2 * s12 + c2, mu1 * mu1 + mu2 * mu2 + c1, s11 + s22 + c2


def _ssim_map(a, b, window_size, sigma, val_range):
    _, _, A1, A2, B1, B2 = _terms(a, b, window_size, sigma, val_range)
    return (A1 * A2) / (B1 * B2)


def ssim_map64(a, b, window_size=11, sigma=1.5, val_range=1.0) -> torch.Tensor:
    """(N, H, W) float64 SSIM map of the planes a, b."""
    return _ssim_map(_planes64(a), _planes64(b), window_size, sigma, val_range).squeeze(1)


def coef64(a, b, window_size=11, sigma=1.5, val_range=1.0) -> torch.Tensor:
    """(3, N, H, W) float64: dS/dmu1, dS/dE[x^2], dS/dE[xy] (module docstring), x the FIRST image."""
    mu1, mu2, A1, A2, B1, B2 = _terms(_planes64(a), _planes64(b), window_size, sigma, val_range)
    S = A1 * A2 / (B1 * B2)
    d_mu1 = 2 * mu2 * (A2 - A1) / (B1 * B2) - 2 * mu1 * S / B1 + 2 * mu1 * S / B2
    return torch.stack([d_mu1, -S / B2, 2 * A1 / (B1 * B2)]).squeeze(2)


LossRef = namedtuple("LossRef", "total l1_mean ssim_mean ssim_planes l1_sums grad")


def loss_and_grad64(a, b, l1_w, ssim_w, window_size=11, sigma=1.5, val_range=1.0, upstream=1.0, clamp=True) -> LossRef:
    """The CombinedLoss scalar l1_w L1 + ssim_w (1 - clamp(mean SSIM, 0, 1)) in float64 with its gradient w.r.t. ``a`` by
    autograd, times ``upstream``.  Returns (total, L1 mean, UNCLAMPED mean SSIM, per-plane mean SSIM (N), per-plane sum |a - b|
    (N), gradient (N, H, W)).  ``clamp=False``: the bare ``ssim()`` form (mrisr_ssim_l1_backward without ``sums``)."""
    x = _planes64(a).requires_grad_(True)
    y = _planes64(b)
    m = _ssim_map(x, y, window_size, sigma, val_range)
    mean = m.mean()
    l1 = (x - y).abs()
    gated = torch.clamp(mean, 0.0, 1.0) if clamp else mean
    total = l1_w * l1.mean() + ssim_w * (1.0 - gated)
    grad, = torch.autograd.grad(total, x)
    return LossRef(total.item(), l1.mean().item(), mean.item(), m.detach().mean((1, 2, 3)).numpy(),
                   l1.detach().sum((1, 2, 3)).numpy(), (grad * upstream).squeeze(1).numpy())


def metrics64(a, b, window_size=11, sigma=1.5, val_range=1.0) -> np.ndarray:
    """(N, 5) float64 per image: ssim, mse, rmse, mae, psnr = 10 log10(val_range^2 / mse), 100 where mse < 1e-10."""
    ss = ssim_map64(a, b, window_size, sigma, val_range).mean((1, 2)).numpy()
    d = (_planes64(a) - _planes64(b)).squeeze(1).numpy()
    mse, mae = (d * d).mean((1, 2)), np.abs(d).mean((1, 2))
    psnr = np.array([100.0 if v < 1e-10 else 10.0 * math.log10(val_range * val_range / v) for v in mse])
    return np.stack([ss, mse, np.sqrt(mse), mae, psnr], 1)


# ------------------------------------------------------------------------------------------------ Adam
def adam64(p, g_list, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, grad_scale=1.0, skip_mask=None, decoupled=False,
           m0=None, v0=None, step0=0):
    """``torch.optim.Adam`` in float64: g = grad_scale g + wd p (L2 decay ADDED TO THE GRADIENT), m = b1 m + (1 - b1) g,
    v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  Returns [(p, m, v, t)] after each
    element of ``g_list``; a step with ``skip_mask[k]`` set leaves all four as they were (its gradient is not looked at).
    ``decoupled=True`` is AdamW instead (p *= 1 - lr wd before the update, no decay in g): what the kernels must NOT compute.
    ``m0``, ``v0``, ``step0``: the state before the first step (zeros, 0)."""
    b1, b2 = betas
    f64 = lambda t: np.array(torch.as_tensor(t).detach().to(torch.float64).numpy(), dtype=np.float64)      # noqa: E731
    p = f64(p)
    m = np.zeros_like(p) if m0 is None else f64(m0)
    v = np.zeros_like(p) if v0 is None else f64(v0)
    t, out = int(step0), []
    for k, g in enumerate(g_list):
        if skip_mask is None or not skip_mask[k]:
            t += 1
            g = f64(g) * grad_scale
            if decoupled:
                p = p * (1.0 - lr * wd)
            else:
                g = g + wd * p
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            p = p - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps)
        out.append((p.copy(), m.copy(), v.copy(), t))
    return out


ADAM_WRAP = 2048 * 256 * 4 + 4099      # past one sweep of the largest grid (2048 blocks x 256 threads x 4): the stride loop wraps
ADAM_SIZES = (1, 3, 4, 5, 1027, ADAM_WRAP)


def adam_inputs(n=1027, steps=5, seed=7, gmag=1.0):
    """(p0 ~ N(0, 1), [gradients ~ gmag N(0, 1)]) as float32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [gmag * torch.randn(n, generator=g) for _ in range(steps)]


# ------------------------------------------------------------------------------------------------ inputs
def _uniform(shape, seed):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def noisy_pair(shape, seed=101):
    """b = clamp(a + 0.2 (U - 0.5), 0, 1): mean SSIM about 0.98 at the larger shapes - inside the clamp gate."""
    a = _uniform(shape, seed)
    b = (a + 0.2 * (_uniform(shape, seed + 1) - 0.5)).clamp(0.0, 1.0)
    return a, b


def anti_pair(shape, seed=202):
    """b = 1 - a, uniform a: mean SSIM below 0 - the clamp gate is CLOSED."""
    a = _uniform(shape, seed)
    return a, 1.0 - a


def mixed_batch(shape=MIXED_SHAPE, seed=303):
    """Plane 0 anti-correlated (SSIM about -0.6), the other planes nearly identical (about 0.997): per-plane SSIM of opposite
    sign, the batch mean inside (0, 1)."""
    assert shape[0] >= 2
    a = _uniform(shape, seed)
    b = (a + 0.05 * (_uniform(shape, seed + 1) - 0.5)).clamp(0.0, 1.0)
    b[0] = 1.0 - a[0]
    return a, b


def tie_pair(shape, seed=404):
    """b == a on a checkerboard of pixels ((y + x) even), |b - a| in [0.05, 0.2] elsewhere (a in [0.25, 0.75]: nothing is
    clamped).  Returns (a, b, tie mask)."""
    a = 0.25 + 0.5 * _uniform(shape, seed)
    d = (0.05 + 0.15 * _uniform(shape, seed + 1)) * torch.where(_uniform(shape, seed + 2) < 0.5, -1.0, 1.0)
    n, h, w = shape
    tie = ((torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)) % 2 == 0).expand(n, h, w)
    b = torch.where(tie, a, a + d)
    assert bool(((b != a) == ~tie).all())
    return a, b, tie
