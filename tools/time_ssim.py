#!/usr/bin/env python
"""SSIM on the GPU (pienerf_amd.metrics.ssim, csrc/pn_ssim.hip) against the same computation as torch ops on the device: the restatement of
tests/ssim_reference.py in fp32, which is what torchmetrics' structural_similarity_index_measure runs (channel-first permute, five grouped 11 x 11
convolutions, a dozen element-wise ops), and its autograd.

    python tools/time_ssim.py [--reps 9] [--inner 20]

Cases: one 800 x 800 x 3 view (the meter's input) and 16 patches of 16 x 16 x 3 (the patch loss of a 4096-ray step), both with data_range = 1.
Timed: the forward call alone (no gradient asked for), and forward + backward of the scalar.  Device events around --inner back-to-back calls after a
warm-up, divided by --inner; the median of --reps such windows.  Both sides include their host-side launch work, as a training step pays it.
Prints one line per case; asserts nothing about the numbers.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_reference as ref  # noqa: E402
from pienerf_amd import metrics  # noqa: E402


def window_ms(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    print(f"{'case':>16} {'what':>10} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}   value hip / torch")
    for name, shape in (("1x800x800x3", (1, 800, 800, 3)), ("16x16x16x3", (16, 16, 16, 3))):
        p, t = (v.to(dev) for v in ref.noise_pair(shape, 0))
        x = p.clone().requires_grad_()

        def hip_fwd():
            return metrics.ssim(p, t, 1.0)

        def torch_fwd():
            with torch.no_grad():
                return ref.ssim(p, t, 1.0, torch.float32)

        def hip_both():
            x.grad = None
            metrics.ssim(x, t, 1.0).backward()

        def torch_both():
            x.grad = None
            ref.ssim(x, t, 1.0, torch.float32).backward()

        values = f"{float(hip_fwd()):.6f} / {float(torch_fwd()):.6f}"
        for what, a, b in (("forward", hip_fwd, torch_fwd), ("fwd + bwd", hip_both, torch_both)):
            ha, tb = window_ms(a, args.reps, args.inner), window_ms(b, args.reps, args.inner)
            print(f"{name:>16} {what:>10} {ha:9.4f} {tb:9.4f} {tb / ha:9.2f}   {values}", flush=True)


if __name__ == "__main__":
    main()
