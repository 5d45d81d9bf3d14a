#!/usr/bin/env python
"""The collider overlay (csrc/pn_colliders.hip: k_draw_colliders) on the GPU: the launch alone at 800 x 800 with a floor, a solid sphere
and a container (case `three`), with all eight slots holding boxes (`boxes`) and with all eight holding capsules (`capsules`), against the same law restated in torch ops on the device (pienerf_amd.colliders.draw_colliders_torch), and one eager step() of the
chair harness with and without the overlay.
    python tools/time_colliders.py [--W 800 --H 800] [--cases three,boxes,capsules] [--reps 5000] [--rounds 5] [--steps 200] [--out FILE.json]
HIP events on one stream.  The launch: a graph of 50 launches, replayed, so the figure is the launch's time on a busy stream and not a launch's latency;
the torch restatement: eager calls (dozens of launches each).  step(): a host clock around `--steps` steps ending in a device synchronise, the two
harnesses in alternating rounds; medians over the rounds with the rounds' spread.  Before timing, the launch is compared with the torch restatement on
the same inputs (largest differences reported; rays both forms hit)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from pienerf_amd.colliders import collider_style, draw_colliders_torch  # noqa: E402
from pienerf_amd.harness import SimRenderHarness  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402
from pienerf_amd.simulator import solver  # noqa: E402

LAUNCHES = 50
BYTES_PER_RAY = 12 + 12 + 4 + 4 + 12 + 12 + 4 + 4   # rays_o, rays_d, weights_sum, depth_0, image in and out, coverage, collider_t


def colliders(case="three"):
    if case == "three":
        return ([solver.contact_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0)), solver.contact_sphere((0.0, 0.0, 0.9), 0.5),
                 solver.contact_sphere((0.0, 0.0, 0.0), 1.6, inside=True)] + [None] * 5)
    spots = [(-0.9 + 0.6 * (k % 4), -0.6 + 0.9 * (k // 4), 0.3 - 0.2 * (k % 3)) for k in range(8)]   # two rows of four across the picture
    if case == "boxes":
        return [solver.contact_box(c, (0.2, 0.25, 0.15 + 0.02 * k)) for k, c in enumerate(spots)]
    if case == "capsules":
        return [solver.contact_capsule((c[0] - 0.15, c[1] - 0.2, c[2]), (c[0] + 0.15, c[1] + 0.2, c[2] + 0.1), 0.12) for c in spots]
    raise SystemExit(f"time_colliders.py: no case {case!r} (three, boxes, capsules)")


def time_events(fn, stream, reps):
    with torch.cuda.stream(stream):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / reps


def measure_launch(W, H, reps, rounds, case="three"):
    dev = torch.device("cuda:0")
    N = W * H
    pose = torch.from_numpy(scene.orbit_pose(3.3, 5.0, -10.0)).unsqueeze(0).to(dev)
    r = get_rays(pose, scene.orbit_intrinsics(W, H, 50.0), H, W, -1)
    o, d = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.rand(N, device=dev, generator=g)
    kind = torch.randint(0, 5, (N,), device=dev, generator=g)
    s = torch.where(kind == 0, torch.zeros_like(s), torch.where(kind == 1, torch.ones_like(s), s))
    acc = torch.rand(N, 3, device=dev, generator=g) * s.unsqueeze(-1)
    d0 = s * (2.0 + 2.5 * torch.rand(N, device=dev, generator=g))
    cols = colliders(case)
    state = torch.frombuffer(bytearray(solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.025), cols)), dtype=torch.float64).to(dev)
    style = collider_style(types=[0 if c is None else c[0] for c in cols], checker=0.25)
    image, cov, ct = acc.clone(), torch.empty(N, device=dev), torch.empty(N, device=dev)

    def launch():
        check(lib().pn_draw_colliders(ptr(state), C.byref(style), ptr(o), ptr(d), N, 0.2, 12.0, 1.0, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(ct),
                                      stream_ptr()), "draw_colliders")

    def restated():
        return draw_colliders_torch(cols, style, o, d, 0.2, 12.0, 1.0, s, d0, acc)

    launch()
    want = restated()
    torch.cuda.synchronize()
    both = torch.isfinite(ct) & torch.isfinite(want[2])
    agree = dict(rays=N, hit_by_the_launch=int(torch.isfinite(ct).sum()), hit_by_both=int(both.sum()),
                 hit_by_one_only=int((torch.isfinite(ct) != torch.isfinite(want[2])).sum()),
                 t_max_abs_diff=float((ct[both] - want[2][both]).abs().max()), coverage_max_abs_diff=float((cov - want[1]).abs().max()),
                 image_median_abs_diff=float((image - want[0]).abs().median()),
                 image_rays_over_1e_4=int(((image - want[0]).abs().amax(dim=1) > 1e-4).sum()))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _ in range(3):
            launch()
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        for _ in range(LAUNCHES):
            launch()   # in place in `image`: every launch moves the same bytes whatever the image holds
    hip, ops = [], []
    for _ in range(rounds):
        hip.append(time_events(graph.replay, st, max(reps // LAUNCHES, 4)) * 1e3 / LAUNCHES)
        ops.append(time_events(restated, st, max(reps // 10, 4)) * 1e3)
    med = statistics.median
    res = dict(case=case, W=W, H=H, rays=N, launch_us=med(hip), launch_us_rounds=hip, torch_restatement_us=med(ops), torch_restatement_us_rounds=ops,
               bytes_per_ray=BYTES_PER_RAY, launch_GB_per_s=N * BYTES_PER_RAY / (med(hip) * 1e-6) / 1e9, agreement=agree)
    print(f"launch at {W} x {H} ({N} rays, {'floor + sphere + container' if case == 'three' else 'eight ' + case}): {res['launch_us']:.2f} us ({min(hip):.2f}..{max(hip):.2f}), "
          f"{res['launch_GB_per_s']:.0f} GB/s of the {BYTES_PER_RAY} B per ray it has to move; torch restatement {res['torch_restatement_us']:.1f} us "
          f"({min(ops):.1f}..{max(ops):.1f}); agreement {agree}", flush=True)
    return res


def measure_step(W, H, steps, rounds):
    def harness(draw):
        h = SimRenderHarness(scene.default_opt(W=W, H=H), device="cuda:0")
        h.sim.enable_contact()
        h.sim.add_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0))
        h.sim.add_sphere((0.0, 0.0, 0.9), 0.5)
        h.sim.add_sphere((0.0, 0.0, 0.0), 1.6, inside=True)
        if draw:
            h.draw_colliders(collider_style(types=h.sim.collider_types(), checker=0.1))
        return h

    hs = {"plain": harness(False), "drawn": harness(True)}
    keep = {k: (h.sim.dof.clone(), h.sim.dof_vel.clone()) for k, h in hs.items()}
    times = {k: [] for k in hs}
    for _ in range(rounds + 1):   # the first round warms up
        for k, h in hs.items():
            h.sim.dof.copy_(keep[k][0])
            h.sim.dof_vel.copy_(keep[k][1])
            h.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                h.step()
            h.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e6)
    times = {k: v[1:] for k, v in times.items()}
    med = statistics.median
    res = dict(W=W, H=H, steps=steps, step_us=med(times["plain"]), step_us_rounds=times["plain"], step_with_overlay_us=med(times["drawn"]),
               step_with_overlay_us_rounds=times["drawn"], increase_us=med(times["drawn"]) - med(times["plain"]))
    print(f"eager step() at {W} x {H}: {res['step_us']:.1f} us ({min(times['plain']):.1f}..{max(times['plain']):.1f}), with the overlay "
          f"{res['step_with_overlay_us']:.1f} us ({min(times['drawn']):.1f}..{max(times['drawn']):.1f}): + {res['increase_us']:.1f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--H", type=int, default=800)
    ap.add_argument("--cases", default="three,boxes,capsules")
    ap.add_argument("--reps", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_colliders.py measures on a GPU; none is visible")
    launches = [measure_launch(args.W, args.H, args.reps, args.rounds, case) for case in args.cases.split(",")]
    out = dict(launch=launches[0], launches=launches, step=measure_step(args.W, args.H, args.steps, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
