#!/usr/bin/env python
"""Times the making of ONE training batch (rays + ground truth of 4096 pixels of a preloaded 800 x 800 view) on three paths:

    a  RayImageSet.batch          the rays of the whole view (pn_get_rays, 640 000 pixels), then torch indexing picks the batch
    b  get_rays(N, image=...)     uniform pixels, one launch of pn_train_batch
    c  get_rays(N, error_map, .)  pn_sample_cells on the view's error map, then pn_train_batch

    python tools/time_batch.py [--rays 4096] [--W 800] [--inner 50] [--reps 9]

Method: device events around ``inner`` consecutive batches (so the figure is what a batch costs on the stream, host-side launch gaps included),
after a warm-up of every path; the paths alternate inside each repetition, so that a drift of the clocks hits all three alike; the median of the
repetitions is reported with the minimum and the maximum.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402
from pienerf_amd.training import RayImageSet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--W", type=int, default=800)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
dev, W, V = "cuda:0", args.W, 4
torch.manual_seed(0)
intr = scene.orbit_intrinsics(W, W, 50.0)
poses = torch.from_numpy(np.stack([scene.orbit_pose(4.0, 90.0 * v, -20.0) for v in range(V)]).astype(np.float32)).to(dev)
images = torch.rand(V, W, W, 3, device=dev)
error_map = torch.rand(V, 128 * 128, device=dev) + 0.01
old = RayImageSet(poses, intr, images, generator=torch.Generator().manual_seed(2))
views = torch.randint(0, V, (args.inner,)).tolist()


def path_a():
    for _ in views:
        old.batch(args.rays)


def path_b():
    for v in views:
        get_rays(poses[v:v + 1], intr, W, W, args.rays, image=images[v])


def path_c():
    for v in views:
        get_rays(poses[v:v + 1], intr, W, W, args.rays, error_map[v:v + 1], image=images[v])


paths = {"a_ray_image_set": path_a, "b_uniform": path_b, "c_error_map": path_c}
for fn in paths.values():   # warm-up: allocator, code objects
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in paths}
for _ in range(args.reps):
    for k, fn in paths.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times[k].append(1e3 * t0.elapsed_time(t1) / args.inner)   # microseconds per batch
out = {"rays": args.rays, "W": W, "inner": args.inner, "reps": args.reps, "unit": "us_per_batch"}
for k, t in times.items():
    out[k] = {"median": round(float(np.median(t)), 2), "min": round(float(np.min(t)), 2), "max": round(float(np.max(t)), 2)}
out["a_over_b"] = round(out["a_ray_image_set"]["median"] / out["b_uniform"]["median"], 2)
out["a_over_c"] = round(out["a_ray_image_set"]["median"] / out["c_error_map"]["median"], 2)
print(json.dumps(out))
