#!/usr/bin/env python
"""Meshing the chair's density field on the GPU (Trainer.save_mesh's work): the lattice evaluation and the marching cubes' count, scan and emit
kernels, at 128^3, 256^3 and 512^3, with V and T.

    python tools/time_mesh.py [--reps 5] [--resolutions 128 256 512] [--threshold 10]

Field: lattice_field over aabb_infer with the shaped synthetic chair (fp32 network).  The kernel split (count = k_mc_count; scan = k_mc_scan_* +
k_mc_offsets; emit = k_mc_emit) comes from the profiler's device records, medians over --reps; `mc total` is the wall time of marching_cubes()
(pn_mc_count, the host read of the two totals, pn_mc_emit) between two synchronizations; `field` likewise for lattice_field.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.mesh import density_query, lattice_field, marching_cubes  # noqa: E402
from pienerf_amd.nerf.network import NeRFNetwork  # noqa: E402

GROUPS = (("count", ("k_mc_count",)), ("scan", ("k_mc_scan_reduce", "k_mc_scan_apply", "k_mc_offsets")), ("emit", ("k_mc_emit",)))


def kernel_split(field, thr, reps):
    """Per-group device milliseconds (median over reps) from torch.profiler's kernel records, or None when the profiler records none."""
    from torch.profiler import ProfilerActivity, profile
    per = {g: [] for g, _ in GROUPS}
    for _ in range(reps):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            marching_cubes(field, thr)
            torch.cuda.synchronize()
        sums = {g: 0.0 for g, _ in GROUPS}
        seen = False
        for ev in prof.events():
            dt = getattr(ev, "device_time", None)
            if dt is None:
                dt = getattr(ev, "cuda_time", 0.0)
            for g, names in GROUPS:
                if any(n in ev.name for n in names) and dt:
                    sums[g] += dt / 1000.0
                    seen = True
        if not seen:
            return None
        for g in sums:
            per[g].append(sums[g])
    return {g: statistics.median(v) for g, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--threshold", type=float, default=10.0)
    args = ap.parse_args()
    dev = "cuda:0"
    model = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to(dev)
    model.load_checkpoint_dict(scene.make_checkpoint(shaped=True))
    q = density_query(model)
    bmin, bmax = model.aabb_infer[:3], model.aabb_infer[3:]
    lattice_field(bmin, bmax, 64, q)
    marching_cubes(torch.zeros(4, 4, 4, device=dev), 0.5)   # warm-up: code objects loaded
    print(f"{'res':>5} {'field ms':>9} {'count ms':>9} {'scan ms':>8} {'emit ms':>8} {'mc total ms':>11} {'V':>9} {'T':>9}")
    for res in args.resolutions:
        ft = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u = lattice_field(bmin, bmax, res, q)
            torch.cuda.synchronize()
            ft.append((time.perf_counter() - t0) * 1e3)
        mt = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v, t = marching_cubes(u, args.threshold)
            torch.cuda.synchronize()
            mt.append((time.perf_counter() - t0) * 1e3)
        split = kernel_split(u, args.threshold, args.reps)
        s = {g: f"{split[g]:.3f}" if split else "n/a" for g, _ in GROUPS}
        print(f"{res:>5} {statistics.median(ft):9.2f} {s['count']:>9} {s['scan']:>8} {s['emit']:>8} {statistics.median(mt):11.3f} {v.shape[0]:>9} "
              f"{t.shape[0]:>9}", flush=True)
        del u, v, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
