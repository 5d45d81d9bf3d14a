#!/usr/bin/env python
"""Golden vectors of the hierarchical-sampling renderer, produced by RUNNING THE REFERENCE'S OWN `run` on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_run.py

The ORIGINAL definitions `sample_pdf` and `NeRFRenderer` of the reference's nerf/renderer.py are compiled, unmodified, through `ast`
(make_golden_ref.extract) into a namespace that holds torch, nn, math, np and a stand-in `raymarching` whose near_far_from_aabb is the CPU oracle's;
a subclass supplies density = oracle.sampling.nerf_density and color = zeros + oracle.nerf_forward(...)[1] on the masked rows; `.eval().run(...)`
runs on CPU tensors.  Nothing of the reference's text is written anywhere: run_kat.npz holds data only — rays, options, image / depth /
weights_sum, and per ray `n_doubt`, the number of samples whose final weight lies within 1e-3 relative of the 1e-4 colour mask threshold (the only
discontinuity of `run` in sigma; tests/test_gpu_hier.py widens the image bound by 1.001e-4 per doubtful sample).  The final weights are obtained
without touching the reference's text: the namespace's `torch` is a forwarding proxy that records the argument of the last cumprod call,
w = (1 - a[:, 1:]) * cumprod(a)[:, :-1].

Inputs: checkpoint scene.make_checkpoint(shaped=True, sigma_outside=1e-3) (regenerated from its seed by the tests, not stored), camera
scene.orbit_pose(2.6, 30, -20) with orbit_intrinsics(800, 800), every 311th ray of the frame.  The generator FAILS if more than 2 % of a case's
rays are doubtful, or if a sample_pdf row has a denominator within 1 % of the 1e-5 switch, where that function is discontinuous.
"""
import os
import sys

sys.dont_write_bytecode = True

import math

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from oracle.sampling import nerf_density  # noqa: E402
from make_golden_ref import extract  # noqa: E402
from pienerf_amd import scene  # noqa: E402

RAY_STRIDE = 311
POSE = (2.6, 30.0, -20.0)
# name -> (num_steps, upsample_steps, density_scale, per-ray background)
CASES = {"t128_128": (128, 128, 1.0, False), "t512_0": (512, 0, 1.0, False), "t64_64": (64, 64, 1.0, False), "t64_64_ds2_bg": (64, 64, 2.0, True),
         "t1_0": (1, 0, 1.0, False), "t2_0": (2, 0, 1.0, False), "t3_1": (3, 1, 1.0, False)}
BAND = 1e-3   # relative half-width of the doubt band around the 1e-4 mask threshold (ISSUE: eps <= 1e-4 on sigma times (1 + optical depth <= 9.2))
MAX_DOUBT_FRACTION = 0.02


class TorchProxy:
    """Forwards everything to torch; remembers the argument of the last cumprod call."""

    def __init__(self):
        self.last_cumprod_arg = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def cumprod(self, x, *a, **k):
        self.last_cumprod_arg = x.detach().clone()
        return torch.cumprod(x, *a, **k)


class Raymarching:
    @staticmethod
    def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.2):
        n, f = oracle.near_far_from_aabb(rays_o.numpy(), rays_d.numpy(), aabb.numpy(), min_near)
        return torch.from_numpy(n), torch.from_numpy(f)


def rays():
    pose = scene.orbit_pose(*POSE)
    o, d = oracle.get_rays(pose, scene.orbit_intrinsics(800, 800), 800, 800)
    idx = np.arange(0, 800 * 800, RAY_STRIDE)
    return np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])


def main():
    proxy = TorchProxy()
    ns = extract("nerf/renderer.py", ["sample_pdf", "NeRFRenderer"], {"torch": proxy, "nn": nn, "math": math, "np": np, "raymarching": Raymarching})
    ck = scene.make_checkpoint(shaped=True, sigma_outside=1e-3)
    bound = float(ck["bound"]) if "bound" in ck else 1.0

    class Model(ns["NeRFRenderer"]):
        def density(self, x):
            sig, geo = nerf_density(x.numpy(), ck, bound)
            return {"sigma": torch.from_numpy(sig), "geo_feat": torch.from_numpy(geo)}

        def color(self, x, d, mask=None, geo_feat=None, **kwargs):
            rgbs = torch.zeros(x.shape[0], 3)
            if mask is None:
                mask = torch.ones(x.shape[0], dtype=torch.bool)
            if mask.any():
                rgbs[mask] = torch.from_numpy(oracle.nerf_forward(x[mask].numpy(), d[mask].numpy(), ck, bound)[1])
            return rgbs

    o, d = rays()
    N = o.shape[0]
    out = {"rays_o": o, "rays_d": d, "ray_stride": np.int64(RAY_STRIDE), "pose": np.asarray(POSE, np.float64), "band": np.float64(BAND),
           "case_names": np.array(sorted(CASES))}
    near, far = oracle.near_far_from_aabb(o, d, np.array([-bound] * 3 + [bound] * 3, np.float32), 0.2)
    out["miss"] = (near == far)
    rng = np.random.default_rng(11)
    for name, (T, t, ds, per_ray_bg) in sorted(CASES.items()):
        m = Model(bound=bound, cuda_ray=False, density_scale=ds, min_near=0.2).eval()
        bg = torch.from_numpy(rng.random((N, 3), dtype=np.float32)) if per_ray_bg else 1
        with torch.no_grad():
            r = m.run(torch.from_numpy(o)[None], torch.from_numpy(d)[None], num_steps=T, upsample_steps=t, bg_color=bg, perturb=False)
        a = proxy.last_cumprod_arg                       # [N, T + t + 1]: [1, 1 - alpha + 1e-15]
        w = (1 - a[:, 1:]) * torch.cumprod(a, dim=-1)[:, :-1]
        # num_steps = 1: the reference's deltas are cat([N, 0], ones_like([N, 0])) = [N, 0] — no sample at all, weights_sum = depth = 0, image = background
        assert w.shape == (N, T + t if T > 1 else 0)
        assert torch.allclose(w.sum(-1), r["weights_sum"].view(-1), atol=1e-5)
        n_doubt = ((w - 1e-4).abs() <= BAND * 1e-4).sum(-1).numpy().astype(np.int32)
        frac = float((n_doubt > 0).mean())
        print(f"{name}: T={T} t={t} ds={ds} doubtful rays {int((n_doubt > 0).sum())} ({100 * frac:.2f} %), max per ray {int(n_doubt.max())}, "
              f"weights_sum > 0.5 on {int((r['weights_sum'] > 0.5).sum())}, NaN depth on {int(torch.isnan(r['depth']).sum())}")
        if frac > MAX_DOUBT_FRACTION:
            raise RuntimeError(f"{name}: {100 * frac:.1f} % of the rays have a sample at the mask threshold (> 2 %): choose other inputs")
        out.update({f"{name}_opts": np.array([T, t, ds, float(per_ray_bg)], np.float64), f"{name}_image": r["image"].view(-1, 3).numpy(),
                    f"{name}_depth": r["depth"].view(-1).numpy(), f"{name}_weights_sum": r["weights_sum"].view(-1).numpy(), f"{name}_n_doubt": n_doubt})
        if per_ray_bg:
            out[f"{name}_bg"] = bg.numpy()

    # ---- sample_pdf alone (det=True)
    g = np.random.default_rng(5)
    Tb = 17
    bins = np.sort(g.random((6, Tb), dtype=np.float32) * 3 + 0.2, axis=1)
    wts = g.random((6, Tb - 1), dtype=np.float32)
    wts[1] = 0.0                       # all-zero weights: the uniform pdf of the 1e-5 floor
    wts[2] = 0.0
    wts[2, 7] = 0.9                    # a single peak
    wts[3, :8] = 0.0                   # an empty head
    wts[4] *= 1e-3                     # weights of the floor's own size
    n_samples = 24
    smp = ns["sample_pdf"](torch.from_numpy(bins), torch.from_numpy(wts), n_samples, det=True).numpy()
    # no denominator within 1 % of the 1e-5 switch
    p = (wts + np.float32(1e-5))
    cdf = np.concatenate([np.zeros((6, 1), np.float32), np.cumsum(p / p.sum(-1, keepdims=True), -1, dtype=np.float32)], -1)
    u = np.linspace(0.5 / n_samples, 1 - 0.5 / n_samples, n_samples, dtype=np.float32)
    for r_ in range(6):
        inds = np.searchsorted(cdf[r_], u, side="right")
        den = cdf[r_][np.minimum(inds, Tb - 1)] - cdf[r_][np.maximum(inds - 1, 0)]
        if np.any(np.abs(den - 1e-5) <= 1e-7):
            raise RuntimeError(f"sample_pdf row {r_}: a denominator within 1 % of the 1e-5 switch")
    out.update(pdf_bins=bins, pdf_weights=wts, pdf_n=np.int64(n_samples), pdf_samples=smp)
    path = os.path.join(HERE, "run_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
