"""Image metrics on the device: SSIM as a differentiable op on the HIP kernels (csrc/pn_ssim.hip), and the reference's PSNR and SSIM
meters (nerf/utils.py:231-302).

    python -m pienerf_amd.metrics A.png B.png [--data_range 1]

prints the PSNR and the SSIM of two images of equal size.

The reference's SSIMMeter calls torchmetrics.structural_similarity_index_measure with its defaults; ``ssim`` computes the same quantity (the
definition is spelled out in include/pienerf_hip.h: pn_ssim_forward) in one launch over the channel-last images the renderer produces, and its
gradient with respect to ``pred`` in one more.  The LPIPS meter is not built: its network weights are not available.
"""
import math
import os

import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr

WINDOW = 11   # taps of the Gaussian window (sigma 1.5); an image is at least this large in both directions


class _SSIM(torch.autograd.Function):
    """[B] per-image SSIM over pn_ssim_range + pn_ssim_forward; backward is pn_ssim_backward.  No host synchronisation in either direction."""

    @staticmethod
    def forward(ctx, pred, truth, data_range):
        B, H, W, C = pred.shape
        dev = pred.device
        h = lib()
        work = torch.empty(int(h.pn_ssim_work_bytes(B, H, W)) // 8, dtype=torch.float64, device=dev)
        c12 = torch.empty(2, dtype=torch.float32, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        s = stream_ptr()
        if data_range is None:
            check(h.pn_ssim_range(ptr(pred), ptr(truth), pred.numel(), 0.0, ptr(work), ptr(c12), s), "ssim range")
        else:
            check(h.pn_ssim_range(None, None, 0, float(data_range), None, ptr(c12), s), "ssim range")
        maps = None
        if ctx.needs_input_grad[0]:
            maps = torch.empty(3, B, H - WINDOW + 1, W - WINDOW + 1, C, dtype=torch.float32, device=dev)
        check(h.pn_ssim_forward(ptr(pred), ptr(truth), B, H, W, C, ptr(c12), ptr(work), ptr(out), *((ptr(m) for m in maps) if maps is not None
                                                                                                   else (None, None, None)), s), "ssim forward")
        if maps is not None:
            ctx.save_for_backward(pred, truth, maps)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        pred, truth, maps = ctx.saved_tensors
        B, H, W, C = pred.shape
        grad_out = grad_out.to(torch.float32).contiguous()
        grad_pred = torch.empty_like(pred)
        check(lib().pn_ssim_backward(ptr(pred), ptr(truth), B, H, W, C, ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(grad_out), ptr(grad_pred),
                                     stream_ptr()), "ssim backward")
        return grad_pred, None, None


def ssim(pred, truth, data_range=None, per_image=False):
    """Structural similarity of ``pred`` and ``truth``, both [B, H, W, C] (channel-last, H, W >= 11) on the GPU: the scalar mean over the batch, or
    with ``per_image`` the [B] per-image values.  Gaussian window of 11 taps with sigma 1.5, evaluated where the whole window lies inside the image,
    c1 = (0.01 R)^2, c2 = (0.03 R)^2, the mean over positions and channels: torchmetrics.structural_similarity_index_measure's value.

    data_range: R.  None (what the reference's meter uses): R = max(pred.max() - pred.min(), truth.max() - truth.min()) over the whole batch,
    evaluated on the device.  Two constant images then give R = 0 and 0/0 = nan, as in the reference.

    Inputs are cast to fp32 (a half ``pred`` from autocast is fine).  Differentiable with respect to ``pred`` only: ``truth`` gets no gradient, and R
    is a constant in both forms — with ``data_range=None`` no gradient flows through the minima and maxima.  Two runs on the same inputs give
    the same bits, forward and backward.  Nothing here waits for the device."""
    if pred.dim() != 4 or truth.dim() != 4:
        raise RuntimeError(f"ssim: images are [B, H, W, C]; got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.shape != truth.shape:
        raise RuntimeError(f"ssim: shapes differ: {tuple(pred.shape)} and {tuple(truth.shape)}")
    B, H, W, C = pred.shape
    if H < WINDOW or W < WINDOW:
        raise RuntimeError(f"ssim: the {WINDOW} x {WINDOW} window does not fit into a {H} x {W} image")
    require_gpu(pred, truth)
    if B < 1 or C < 1 or B > 65535 or H * W * C >= 2 ** 31:
        raise RuntimeError(f"ssim: shape {tuple(pred.shape)} is outside the kernel's limits (1 <= B <= 65535, C >= 1, H W C < 2^31)")
    if data_range is not None and not (float(data_range) > 0 and math.isfinite(float(data_range))):
        raise RuntimeError(f"ssim: data_range = {data_range} is not a positive number")
    with torch.autocast("cuda", enabled=False):
        per = _SSIM.apply(pred.to(torch.float32).contiguous(), truth.detach().to(torch.float32).contiguous(), data_range)
        return per if per_image else per.mean()


class PSNRMeter:
    """nerf/utils.py:231-265, with the running sum kept on the device: ``measure`` is the only point that reads it back."""

    name = "PSNR"

    def __init__(self):
        self.clear()

    def clear(self):
        self.V = 0
        self.N = 0

    def _value(self, preds, truths):   # [B, N, 3] or [B, H, W, 3], range [0, 1]: max_pixel_value is 1
        return -10 * torch.log10(torch.mean((preds.to(torch.float32) - truths.to(torch.float32)) ** 2))

    @torch.no_grad()
    def update(self, preds, truths):
        self.V = self.V + self._value(preds, truths)
        self.N += 1

    def measure(self):
        return float(self.V) / self.N

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, self.name), self.measure(), global_step)

    def report(self):
        return f"{self.name} = {self.measure():.6f}"


class SSIMMeter(PSNRMeter):
    """nerf/utils.py:268-302: ``update(preds, truths)`` on [B, H, W, 3] adds ``ssim`` with data_range=None."""

    name = "SSIM"

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.clear()

    def _value(self, preds, truths):
        return ssim(preds.to(self.device), truths.to(self.device))


def main(argv=None):
    import argparse
    from . import io
    ap = argparse.ArgumentParser(description="PSNR and SSIM of two images of equal size")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--data_range", type=float, default=None, help="SSIM's data range; default: from the two images, like the reference's meter")
    ap.add_argument("--device", default="cuda:0")
    opt = ap.parse_args(argv)
    a, b = (io.load_image(p).to(opt.device)[None] for p in (opt.a, opt.b))
    if a.shape != b.shape:
        raise SystemExit(f"the images differ in size: {tuple(a.shape[1:3])} and {tuple(b.shape[1:3])}")
    psnr = PSNRMeter()
    psnr.update(a, b)
    value = float(ssim(a, b, opt.data_range))
    print(f"{psnr.report()}  SSIM = {value:.6f}")
    return psnr.measure(), value


if __name__ == "__main__":
    main()
