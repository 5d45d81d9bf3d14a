#!/usr/bin/env python
"""One PointBinding.warp (csrc/pn_warp_points.hip) on the shaped synthetic chair's mesh against the torch op sequence it replaces and against the
streaming floor of its tables.

    python tools/time_warp_points.py [--res 256] [--reps 9] [--inner 50] [--sim_dx 0.05]

The mesh: extract_geometry at --res on the shaped checkpoint, bound to the default harness's simulator.  Timed, with and without normals:
  hip    binding.warp(out=...) — one launch;
  torch  Simulator.update_pos's gather + einsum in fp64 on the same tables in their plain layout, plus (with normals) the gradient's einsum, the three
         cross products and the normalisation (binding.warp_torch);
  floor  the tables the launch must stream — 640 B per point (Nx), 2 560 B with normals (+ dNx) — plus topo (32 B), rest normals and outputs
         (12 B each), over the 6.3 TB/s a streaming copy reaches on this part.  dof stays in cache and is not counted.
Protocol: device events around --inner back-to-back calls after a warm-up, per-call time = window / inner, median of --reps windows, the two
routes alternating window by window.  A table smaller than the 256 MiB Infinity Cache may be served from it on repeated launches; the table size is
printed so that the floor can be read accordingly.  The outputs are compared before anything is timed.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.harness import SimRenderHarness  # noqa: E402
from pienerf_amd.mesh import density_query, vertex_normals  # noqa: E402
from pienerf_amd.nerf.utils import extract_geometry  # noqa: E402
from pienerf_amd.simulator.binding import warp_torch  # noqa: E402

STREAM_TBS = 6.3


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--sim_dx", type=float, default=0.05)
    ap.add_argument("--substeps", type=int, default=12, help="forced substeps before timing (a deformed state)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_warp_points: needs the GPU (nothing is timed on a CPU)")
    opt = scene.default_opt(sim_dx=args.sim_dx, W=64, H=64)
    h = SimRenderHarness(opt, ckpt=scene.make_checkpoint(bound=opt["bound"], shaped=True), device="cuda:0", overlap_sim=False)
    sim, m = h.sim, h.model
    v, t = extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], args.res, 10.0, density_query(m))
    n = vertex_normals(v, t)
    sim.update_force(sim.n_IP // 2, torch.tensor([300.0, 100.0, -200.0], dtype=torch.float64))
    for _ in range(args.substeps):
        sim.stepforward()
    torch.cuda.synchronize()
    V = len(v)
    print(f"mesh {args.res}^3: V {V}, T {len(t)}; simulator n_k {sim.n_k}, n_IP {sim.n_IP}", flush=True)
    for with_n in (False, True):
        b = sim.bind_points(v, n if with_n else None)
        topo, Nx, dNx = b.tables()
        out = (torch.empty((V, 3), dtype=torch.float32, device="cuda:0"), torch.empty((V, 3), dtype=torch.float32, device="cuda:0"))
        hip = (lambda: b.warp(out=out)) if with_n else (lambda: b.warp(out=out[0]))
        ref = lambda: warp_torch(topo, Nx, dNx, b.normals0, sim.dof)   # noqa: E731
        got, want = hip(), ref()
        torch.cuda.synchronize()
        gp, wp = (got[0], want[0]) if with_n else (got, want)
        diff = f"positions {float((gp.double() - wp.double()).abs().max()):.3g}"
        if with_n:
            diff += f", normals {float((got[1].double() - want[1].double()).abs().max()):.3g}"
        table = V * (640 + (1920 if with_n else 0))
        nbytes = table + V * (32 + 12 + (24 if with_n else 0))
        floor = nbytes / (STREAM_TBS * 1e12) * 1e3
        for f in (hip, ref):
            window_ms(f, 3)
        th, tt = [], []
        for _ in range(args.reps):
            th.append(window_ms(hip, args.inner))
            tt.append(window_ms(ref, max(args.inner // 10, 1)))
        mh, mt = statistics.median(th), statistics.median(tt)
        print(f"{'with normals' if with_n else 'positions   '}: fallback {b.n_fallback}, tables {table / 2 ** 20:.0f} MiB, max |hip - torch| {diff}; "
              f"hip {mh:.4f} ms [{min(th):.4f}, {max(th):.4f}], torch {mt:.3f} ms [{min(tt):.3f}, {max(tt):.3f}], floor {floor:.4f} ms; "
              f"floor/hip {floor / mh:.3f}, torch/hip {mt / mh:.1f}", flush=True)
        del b, topo, Nx, dNx, out


if __name__ == "__main__":
    main()
