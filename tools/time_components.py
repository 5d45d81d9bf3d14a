#!/usr/bin/env python
"""Connected-component labelling on the GPU (pienerf_amd.components.label_components, csrc/pn_components.hip) at 256^3 against the route it
replaces (the mask copied to the host, scipy.ndimage.label there) and against the streaming floor of its three launches.

    python tools/time_components.py [--reps 9] [--res 256] [--threshold 10]

Inputs: (a) the shaped synthetic chair's density lattice above --threshold (what extract_geometry(components=) labels), 26-connectivity;
(b) random occupancy p = 0.3, 6- and 26-connectivity.  GPU time: device events around the call after a warm-up, median of --reps; the per-launch
split comes from the profiler's device records.  Host route: wall time of mask.cpu() plus scipy.ndimage.label, median of 3.  Floor: the bytes every
launch must move whatever the data, at the 6.3 TB/s a streaming copy reaches on this part: tiles reads the mask (N bytes) and writes the labels
(4 N), merge reads the mask (N), compress reads the labels (4 N): 10 N bytes.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.components import label_components  # noqa: E402
from pienerf_amd.mesh import density_query, lattice_field  # noqa: E402
from pienerf_amd.nerf.network import NeRFNetwork  # noqa: E402

KERNELS = ("k_ccl_tiles", "k_ccl_merge", "k_ccl_compress")
STREAM_TBS = 6.3


def device_ms(occ, conn, reps):
    label_components(occ, conn)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        label_components(occ, conn)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def kernel_split(occ, conn, reps):
    """Per-launch device milliseconds (median over reps) from torch.profiler's kernel records, or None when the profiler records none."""
    from torch.profiler import ProfilerActivity, profile
    per = {k: [] for k in KERNELS}
    for _ in range(reps):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            label_components(occ, conn)
            torch.cuda.synchronize()
        sums = dict.fromkeys(KERNELS, 0.0)
        for ev in prof.events():
            dt = getattr(ev, "device_time", None)
            if dt is None:
                dt = getattr(ev, "cuda_time", 0.0)
            for k in KERNELS:
                if k in ev.name and dt:
                    sums[k] += dt / 1000.0
        if not any(sums.values()):
            return None
        for k in KERNELS:
            per[k].append(sums[k])
    return {k: statistics.median(v) for k, v in per.items()}


def host_ms(occ, conn):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, 1) if conn == 6 else np.ones((3, 3, 3), bool)
    copy, label = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = occ.cpu().numpy()
        t1 = time.perf_counter()
        _, n = ndimage.label(host, structure=structure)
        t2 = time.perf_counter()
        copy.append((t1 - t0) * 1e3)
        label.append((t2 - t1) * 1e3)
    return statistics.median(copy), statistics.median(label), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    args = ap.parse_args()
    dev = "cuda:0"
    model = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to(dev)
    model.load_checkpoint_dict(scene.make_checkpoint(shaped=True))
    field = lattice_field(model.aabb_infer[:3], model.aabb_infer[3:], args.res, density_query(model))
    chair = field.to(torch.float64) > args.threshold
    del field
    rand = torch.from_numpy(np.random.default_rng(0).random((args.res,) * 3) < 0.3).to(dev)
    n = args.res ** 3
    floor = 10.0 * n / (STREAM_TBS * 1e12) * 1e3
    print(f"{args.res}^3, floor {floor:.4f} ms (10 N bytes at {STREAM_TBS} TB/s)")
    print(f"{'input':>12} {'conn':>4} {'occupied':>9} {'comps':>7} {'gpu ms':>8} {'tiles':>7} {'merge':>7} {'compress':>8} {'floor/gpu':>9} {'d2h ms':>7} "
          f"{'scipy ms':>9} {'host/gpu':>9}")
    for name, occ, conns in (("chair", chair, (26,)), ("random 0.3", rand, (6, 26))):
        for conn in conns:
            g = device_ms(occ, conn, args.reps)
            split = kernel_split(occ, conn, min(args.reps, 5))
            s = {k: f"{split[k]:.3f}" if split else "n/a" for k in KERNELS}
            copy, label, comps = host_ms(occ, conn)
            print(f"{name:>12} {conn:>4} {int(occ.sum()):>9} {comps:>7} {g:8.3f} {s['k_ccl_tiles']:>7} {s['k_ccl_merge']:>7} {s['k_ccl_compress']:>8} "
                  f"{floor / g:9.3f} {copy:7.2f} {label:9.1f} {(copy + label) / g:9.1f}", flush=True)


if __name__ == "__main__":
    main()
