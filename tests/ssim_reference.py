"""SSIM restated in torch (the tests evaluate it on the CPU), the way torchmetrics' structural_similarity_index_measure evaluates it (which the reference's SSIMMeter calls,
nerf/utils.py:268-302): channel-first images, one grouped conv2d with the 11 x 11 outer product of the Gaussian taps (sigma 1.5) per moment, the
five moments, the SSIM formula, the mean over the valid region.  torchmetrics pads by reflection and crops the same 5-pixel border away again; the
valid convolution used here is that result without the detour.

The dtype is a parameter: the fp64 evaluation is the reference of tests/test_gpu_ssim.py, the distance of the fp32 evaluation from it sets the
tolerances there (``forward_bar`` / ``grad_bar``).  Its autograd is the gradient reference.
"""
import math

import torch
import torch.nn.functional as F

TAPS = 11
SIGMA = 1.5


def taps(dtype=torch.float64):
    """The 11 taps: computed in double, normalised to sum 1, rounded to fp32 (the values the kernel holds), then cast to ``dtype``."""
    g = [math.exp(-(((i - TAPS // 2) / SIGMA) ** 2) / 2) for i in range(TAPS)]
    s = sum(g)
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(torch.float32).to(dtype)


def data_range_of(pred, truth):
    """data_range=None: max(pred.max() - pred.min(), truth.max() - truth.min()) over the whole batch."""
    return torch.maximum(pred.max() - pred.min(), truth.max() - truth.min())


def ssim_per_image(pred, truth, data_range=None, dtype=torch.float64):
    """pred, truth [B, H, W, C] -> [B] in ``dtype``.  Differentiable in both arguments; the range of ``data_range=None`` is detached."""
    x = pred.to(dtype).permute(0, 3, 1, 2)
    y = truth.to(dtype).permute(0, 3, 1, 2)
    C = x.shape[1]
    R = data_range_of(x, y).detach() if data_range is None else torch.as_tensor(data_range, dtype=dtype)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    g = taps(dtype).to(x.device)
    w = (g[:, None] * g[None, :]).expand(C, 1, TAPS, TAPS).contiguous()
    mom = F.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), w.repeat(5, 1, 1, 1), groups=5 * C)
    mx, my, exx, eyy, exy = mom.split(C, 1)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    S = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return S.mean(dim=(1, 2, 3))


def ssim(pred, truth, data_range=None, dtype=torch.float64):
    return ssim_per_image(pred, truth, data_range, dtype).mean()


def forward_bar(pred, truth, data_range=None):
    """(fp64 per-image values, fp64 scalar, tolerance): 8 x |fp32 restatement - fp64 restatement| of the scalar on the same input, at least 5e-7."""
    with torch.no_grad():
        p64 = ssim_per_image(pred, truth, data_range, torch.float64)
        p32 = ssim_per_image(pred, truth, data_range, torch.float32)
    tol = max(8.0 * abs(float(p32.mean().double() - p64.mean())), 5e-7)
    return p64, p64.mean(), tol


def grad_ref(pred, truth, data_range, dtype=torch.float64, weights=None):
    """d(sum_b weights[b] ssim_b) / d pred through autograd; weights None: the scalar mean."""
    p = pred.detach().clone().to(dtype).requires_grad_()
    per = ssim_per_image(p, truth.detach(), data_range, dtype)
    (per.mean() if weights is None else (per * weights.to(dtype)).sum()).backward()
    return p.grad


def grad_bar(pred, truth, data_range, weights=None):
    """(fp64 gradient, tolerance on max|diff| / max|grad_ref|): 8 x the same quantity of the fp32 restatement, at least 1e-5."""
    g64 = grad_ref(pred, truth, data_range, torch.float64, weights)
    g32 = grad_ref(pred, truth, data_range, torch.float32, weights)
    scale = float(g64.abs().max())
    return g64, max(8.0 * float((g32.double() - g64).abs().max()) / scale, 1e-5)


def noise_pair(shape, seed):
    """Uniform noise against itself plus 0.1 noise, clamped to [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return b.contiguous(), a.contiguous()


def smooth_pair(shape, seed):
    """A smooth sinusoid (range about 1) against itself plus 0.02 noise."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C = shape
    i = torch.arange(H, dtype=torch.float32)[None, :, None, None]
    j = torch.arange(W, dtype=torch.float32)[None, None, :, None]
    b = torch.arange(B, dtype=torch.float32)[:, None, None, None]
    c = torch.arange(C, dtype=torch.float32)[None, None, None, :]
    a = 0.5 + 0.5 * torch.sin(0.37 * i + 0.9 * c + 0.5 * b) * torch.cos(0.29 * j - 0.4 * c)
    p = a + 0.02 * torch.randn(shape, generator=g)
    return p.contiguous(), a.contiguous()
