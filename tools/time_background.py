#!/usr/bin/env python
"""The background model's per-frame cost at 800 x 800: the fused kernel (pn_background_forward, blend mode: one launch) against the op sequence it
replaces (sph_from_ray, background_ops = 2-D grid encoder + SH encoder + cat + two GEMMs + ReLU + sigmoid, then the three torch blend ops).

    python tools/time_background.py [--W 800] [--reps 50] [--warmup 10] [--fp16]

Every figure is the median over --reps launches (>= 20) of device-event time around ONE frame's background work, alternating the two forms, after --warmup
launches of each; the spread (min .. max) is printed beside it.  Rays: the orbit camera at r = 5 inside the sphere of R = 32; random table and weights
(scene.make_checkpoint(bg_radius=32)); image / weights_sum random in [0, 1].  A run without a GPU fails: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import raymarching, scene  # noqa: E402
from pienerf_amd.nerf.network import NeRFNetwork  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fp16", action="store_true", help="both forms under autocast (Trainer(fp16=True))")
    args = ap.parse_args()
    assert args.reps >= 20
    dev, R = "cuda:0", 32.0
    model = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, bg_radius=R).to(dev).load_checkpoint_dict(scene.make_checkpoint(bg_radius=R))
    pose = torch.from_numpy(scene.orbit_pose(5.0)).unsqueeze(0).to(dev)
    rays = get_rays(pose, scene.orbit_intrinsics(args.W, args.W, 50.0), args.W, args.W, -1)
    o, d = rays["rays_o"].view(-1, 3).contiguous(), rays["rays_d"].view(-1, 3).contiguous()
    N = o.shape[0]
    image0, ws = torch.rand(N, 3, device=dev), torch.rand(N, device=dev)
    image = image0.clone()

    def fused():
        model.blend_background(o, d, ws, image)

    def ops():
        bg = model.background_ops(raymarching.sph_from_ray(o, d, R), d)
        return image0 + (1 - ws).unsqueeze(-1) * bg

    times = {"fused": [], "ops": []}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=args.fp16):
        for _ in range(args.warmup):
            fused()
            ops()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in (("fused", fused), ("ops", ops)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    res = {"rays": N, "fp16": bool(args.fp16), "reps": args.reps}
    for name, v in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res["ops_over_fused"] = round(res["ops_ms"]["median"] / res["fused_ms"]["median"], 2)
    # what the fused launch must move at the least: rays in (24 B), weights_sum (4 B), image in and out (24 B) per ray; the 5.6 MB table stays in cache
    res["fused_min_bytes_per_ray"] = 52
    res["fused_GBps_of_min_traffic"] = round(52 * N / (res["fused_ms"]["median"] * 1e-3) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
