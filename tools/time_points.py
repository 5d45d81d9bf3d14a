#!/usr/bin/env python
"""The point overlay (csrc/pn_points_overlay.hip: k_points_splat + k_points_resolve) on the GPU: the launch pair alone at 800 x 800 on the
chair's point cloud and on the stress configuration's dense one (scene.make_chair_points, sub_res 180), for footprints of radius 0 and 2, the colliders'
launch on the same frame for comparison, and one eager step() of the chair harness with and without the overlay.
    python tools/time_points.py [--W 800 --H 800] [--reps 5000] [--rounds 5] [--steps 200] [--out FILE.json]
HIP events on one stream.  The pair: a graph of 50 pairs, replayed, so the figure is the pair's time on a busy stream and not a launch's latency; the
variants take turns within every round.  step(): a host clock around `--steps` steps ending in a device synchronise, the two harnesses in alternating
rounds (the first round warms up); medians over the rounds with the rounds' spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from pienerf_amd.colliders import collider_style  # noqa: E402
from pienerf_amd.harness import SimRenderHarness  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402
from pienerf_amd.points_overlay import key_buffer, point_style  # noqa: E402
from pienerf_amd.simulator import solver  # noqa: E402

LAUNCHES = 50
BYTES_PER_PIXEL = 8 + 4 + 4   # the resolve launch's floor, what an undrawn pixel costs: the key read; point_id, point_t written


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


def captured(fn, stream):
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(LAUNCHES):
            fn()
    return graph


def measure_launch(W, H, reps, rounds):
    dev = torch.device("cuda:0")
    N = W * H
    opt = scene.default_opt(W=W, H=H)
    pose = torch.from_numpy(scene.orbit_pose(opt["radius"])).unsqueeze(0).to(dev)
    intr = scene.orbit_intrinsics(W, H, opt["fovy"])
    intr_c = (C.c_float * 4)(*[float(v) for v in intr])
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.rand(N, device=dev, generator=g)
    kind = torch.randint(0, 5, (N,), device=dev, generator=g)
    s = torch.where(kind == 0, torch.zeros_like(s), torch.where(kind == 1, torch.ones_like(s), s))
    d0 = s * (4.0 + 2.0 * torch.rand(N, device=dev, generator=g))
    ct = torch.where(torch.rand(N, device=dev, generator=g) < 0.3, torch.full_like(s, 5.0), torch.full_like(s, float("inf")))
    image = torch.rand(N, 3, device=dev, generator=g)
    pid, pt = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev)
    keys = key_buffer(W, H, dev)
    chair = np.ascontiguousarray(scene.make_chair_points(hgs=opt["hash_grid_size"], bound=opt["bound"])["pos"], np.float32)
    stress = np.ascontiguousarray(scene.make_chair_points(sub_res=scene.stress_opt()["sub_res"], hgs=opt["hash_grid_size"], bound=opt["bound"])["pos"], np.float32)
    # the worst case for the atomic: every point of the chair's cloud moved onto the view axis, so all of them contend for one pixel
    clouds = {"chair": (chair, (0, 2)), "stress": (stress, (0, 2)), "chair_on_one_pixel": (chair * np.array([0.0, 0.0, 1.0], np.float32), (0,))}
    st = torch.cuda.Stream()
    variants, alive = {}, []   # `alive`: a captured graph holds addresses, not references
    for name, (cloud, radii) in clouds.items():
        pos = torch.from_numpy(cloud).to(dev)
        F = torch.eye(3, device=dev).reshape(1, 9).repeat(pos.shape[0], 1).contiguous()
        alive += [pos, F]
        for radius in radii:
            style = point_style(radius=radius, mode="strain", hidden_alpha=0.25)

            def pair(pos=pos, F=F, style=style):
                check(lib().pn_draw_points(ptr(pos), ptr(F), None, pos.shape[0], ptr(pose), intr_c, W, H, 0.2, ptr(s), ptr(d0), ptr(ct), None, ptr(keys),
                                           style, ptr(image), ptr(pid), ptr(pt), stream_ptr()), "draw_points")
            with torch.cuda.stream(st):
                pair()
            st.synchronize()
            variants[f"{name}_r{radius}"] = dict(points=int(pos.shape[0]), radius=radius, pixels_drawn=int((pid >= 0).sum()), graph=captured(pair, st))
    # the colliders' launch on the same frame: what DESIGN.md 4.13 compares the pair with
    r = get_rays(pose, intr, H, W, -1)
    o, d = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    cols = [solver.contact_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0)), solver.contact_sphere((0.0, 0.0, 0.9), 0.5)] + [None] * 6
    state = torch.frombuffer(bytearray(solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.025), cols)), dtype=torch.float64).to(dev)
    cstyle = collider_style(types=[0 if c is None else c[0] for c in cols], checker=0.25)
    cov, cto = torch.empty(N, device=dev), torch.empty(N, device=dev)

    def colliders():
        check(lib().pn_draw_colliders(ptr(state), C.byref(cstyle), ptr(o), ptr(d), N, 0.2, 12.0, 1.0, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(cto),
                                      stream_ptr()), "draw_colliders")
    variants["colliders_launch"] = dict(graph=captured(colliders, st))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, v in variants.items():   # the variants take turns within a round
            times[k].append(time_events(v["graph"].replay, st, max(reps // LAUNCHES, 4)) * 1e3 / LAUNCHES)
    med = statistics.median
    res = dict(W=W, H=H, pixels=N, resolve_floor_bytes_per_pixel=BYTES_PER_PIXEL)
    for k, v in variants.items():
        res[k] = {kk: vv for kk, vv in v.items() if kk != "graph"}
        res[k].update(us=med(times[k]), us_rounds=times[k])
        print(f"{k} at {W} x {H}: {res[k]['us']:.2f} us ({min(times[k]):.2f}..{max(times[k]):.2f}) {res[k]}", flush=True)
    return res


def measure_step(W, H, steps, rounds):
    def harness(draw):
        h = SimRenderHarness(scene.default_opt(W=W, H=H), device="cuda:0")
        if draw:
            h.draw_points(point_style(radius=1, mode="strain", hidden_alpha=0.25))
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
    res = dict(W=W, H=H, steps=steps, points=int(hs["drawn"].sim.n_IP), step_us=med(times["plain"]), step_us_rounds=times["plain"],
               step_with_overlay_us=med(times["drawn"]), step_with_overlay_us_rounds=times["drawn"], increase_us=med(times["drawn"]) - med(times["plain"]))
    print(f"eager step() at {W} x {H}: {res['step_us']:.1f} us ({min(times['plain']):.1f}..{max(times['plain']):.1f}), with the {res['points']} integration "
          f"points drawn {res['step_with_overlay_us']:.1f} us ({min(times['drawn']):.1f}..{max(times['drawn']):.1f}): + {res['increase_us']:.1f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--H", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_points.py measures on a GPU; none is visible")
    out = dict(launch=measure_launch(args.W, args.H, args.reps, args.rounds), step=measure_step(args.W, args.H, args.steps, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
