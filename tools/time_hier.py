#!/usr/bin/env python
"""One 800 x 800 frame of a model WITHOUT a density grid (NeRFRenderer.run, hierarchical sampling): the fused launch (pn_render_hier) against the op
sequence it replaces (run_ops, staged in batches of 4096 rays as the reference's render(staged=True) runs it).

    python tools/time_hier.py [--W 800] [--reps 7] [--warmup 2] [--steps 128,128 512,0] [--only fused|ops]

Every figure is the median over --reps frames of device-event time around ONE frame, alternating the two forms, after --warmup frames of each; the spread
(min .. max) is printed beside it.  Scene: the `shaped` synthetic chair (scene.make_checkpoint(shaped=True, sigma_outside=1e-3)) from the orbit camera
scene.orbit_pose(2.6, 30, -20).  --only runs one form (for a kernel trace of the fused launch alone).  A run without a GPU fails: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.nerf.network import NeRFNetwork  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", nargs="+", default=["128,128", "512,0"], help="num_steps,upsample_steps pairs")
    ap.add_argument("--only", choices=("fused", "ops"), default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    model = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=False).to(dev).load_checkpoint_dict(scene.make_checkpoint(shaped=True, sigma_outside=1e-3))
    pose = torch.from_numpy(scene.orbit_pose(2.6, 30.0, -20.0)).unsqueeze(0).to(dev)
    rays = get_rays(pose, scene.orbit_intrinsics(args.W, args.W, 50.0), args.W, args.W, -1)
    o, d = rays["rays_o"].contiguous(), rays["rays_d"].contiguous()   # [1, N, 3]
    N = o.shape[1]
    for pair in args.steps:
        T, t = (int(v) for v in pair.split(","))
        kw = dict(num_steps=T, upsample_steps=t, bg_color=1)

        def fused():
            return model.run(o, d, **kw)

        def ops():
            for head in range(0, N, 4096):
                model.run_ops(o[:, head:head + 4096], d[:, head:head + 4096], **kw)

        forms = [(n, f) for n, f in (("fused", fused), ("ops", ops)) if args.only in (None, n)]
        times = {n: [] for n, _ in forms}
        with torch.no_grad():
            assert model._hier_fused_ok(o, T, t, 1)
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name, fn in forms:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
        res = {"rays": N, "num_steps": T, "upsample_steps": t, "reps": args.reps, "density_queries": N * (T + t)}
        for name, v in times.items():
            res[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        if "fused" in times and "ops" in times:
            res["ops_over_fused"] = round(res["ops_ms"]["median"] / res["fused_ms"]["median"], 2)
        if "fused" in times:
            res["fused_density_queries_per_ms"] = round(N * (T + t) / res["fused_ms"]["median"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
