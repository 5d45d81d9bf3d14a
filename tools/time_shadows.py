#!/usr/bin/env python
"""Shadows on the drawn colliders (csrc/pn_colliders.hip: k_draw_colliders_shadowed) on the GPU: the shadowed launch at 800 x 800 with a
256 x 256 map against pn_draw_colliders on the same inputs, and one eager step() of the chair harness with the overlay only and with shadows at map
resolutions 128, 256 and 512.
    python tools/time_shadows.py [--W 800 --H 800] [--S 256] [--reps 5000] [--rounds 5] [--steps 100] [--res 128 256 512] [--out FILE.json]
HIP events on one stream.  The launches: a graph of 50 launches each, replayed, the two graphs in alternating rounds in the same process, so the figures
are a launch's time on a busy stream and not its latency.  step(): a host clock around `--steps` steps ending in a device synchronise, a harness with the
overlay only and one with shadows in alternating rounds; medians over the rounds with the rounds' minimum and maximum.  The difference of the two step
times is the shadow pass (a full render of S^2 rays, colour included) plus the dearer launch."""
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
from pienerf_amd.colliders import collider_style, shadow_light  # noqa: E402
from pienerf_amd.harness import SimRenderHarness  # noqa: E402
from pienerf_amd.nerf.utils import get_rays  # noqa: E402
from pienerf_amd.simulator import solver  # noqa: E402
from time_colliders import LAUNCHES, colliders, time_events  # noqa: E402


def measure_launch(W, H, S, reps, rounds):
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
    # a map as a render leaves it: a disc of opaque texels around the centre, depth 1.5 .. 2.5, empty outside
    j, i = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    rad = torch.sqrt((i - S / 2 + 0.5) ** 2 + (j - S / 2 + 0.5) ** 2) / (S / 2)
    ws = (1.2 - 2.0 * rad).clamp(0, 1).reshape(-1).contiguous()
    wd = (ws * (1.5 + rad.reshape(-1))).contiguous()
    cols = colliders()
    state = torch.frombuffer(bytearray(solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.025), cols)), dtype=torch.float64).to(dev)
    style = collider_style(types=[0 if c is None else c[0] for c in cols], checker=0.25)
    light = shadow_light(resolution=S)
    image, cov, ct, sh = acc.clone(), torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)

    def plain():
        check(lib().pn_draw_colliders(ptr(state), C.byref(style), ptr(o), ptr(d), N, 0.2, 12.0, 1.0, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(ct),
                                      stream_ptr()), "draw_colliders")

    def shadowed():
        check(lib().pn_draw_colliders_shadowed(ptr(state), C.byref(style), ptr(o), ptr(d), N, 0.2, 12.0, 1.0, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(ct),
                                               light, ptr(ws), ptr(wd), ptr(sh), stream_ptr()), "draw_colliders_shadowed")

    shadowed()
    torch.cuda.synchronize()
    seen = torch.isfinite(ct)
    counts = dict(rays=N, hits=int(seen.sum()), shadowed=int((sh > 0).sum()), fully=int((sh == 1).sum()))
    st = torch.cuda.Stream()
    graphs = {}
    for name, fn in (("plain", plain), ("shadowed", shadowed)):
        with torch.cuda.stream(st):
            for _ in range(3):
                fn()
        st.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=st):
            for _ in range(LAUNCHES):
                fn()   # in place in `image`: every launch moves the same bytes whatever the image holds
    us = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            us[k].append(time_events(gr.replay, st, max(reps // LAUNCHES, 4)) * 1e3 / LAUNCHES)
    med = statistics.median
    res = dict(W=W, H=H, S=S, counts=counts, draw_colliders_us=med(us["plain"]), draw_colliders_us_rounds=us["plain"],
               draw_colliders_shadowed_us=med(us["shadowed"]), draw_colliders_shadowed_us_rounds=us["shadowed"])
    print(f"launch at {W} x {H}, map {S} x {S} ({counts}): pn_draw_colliders {res['draw_colliders_us']:.2f} us ({min(us['plain']):.2f}..{max(us['plain']):.2f}), "
          f"pn_draw_colliders_shadowed {res['draw_colliders_shadowed_us']:.2f} us ({min(us['shadowed']):.2f}..{max(us['shadowed']):.2f})", flush=True)
    return res


def measure_step(W, H, S, steps, rounds):
    def harness(shadows):
        h = SimRenderHarness(scene.default_opt(W=W, H=H), device="cuda:0")
        h.sim.enable_contact()
        h.sim.add_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0))
        h.sim.add_sphere((0.0, 0.0, 0.9), 0.5)
        h.draw_colliders(collider_style(types=h.sim.collider_types(), checker=0.1))
        if shadows:
            h.cast_shadows(resolution=S)
        return h

    hs = {"drawn": harness(False), "shadowed": harness(True)}
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
    m = hs["shadowed"].model
    st = m.render_status(slot=m.SHADOW_SLOT)
    main = m.render_status(slot=0)
    res = dict(W=W, H=H, S=S, steps=steps, step_overlay_us=med(times["drawn"]), step_overlay_us_rounds=times["drawn"],
               step_shadows_us=med(times["shadowed"]), step_shadows_us_rounds=times["shadowed"], increase_us=med(times["shadowed"]) - med(times["drawn"]),
               shadow_pass_samples=st["samples"], shadow_pass_trips=st["trips"], frame_samples=main["samples"], frame_trips=main["trips"])
    res["shadow_share_of_step"] = res["increase_us"] / res["step_shadows_us"]
    print(f"eager step() at {W} x {H}: overlay only {res['step_overlay_us']:.1f} us ({min(times['drawn']):.1f}..{max(times['drawn']):.1f}), shadows at S = {S} "
          f"{res['step_shadows_us']:.1f} us ({min(times['shadowed']):.1f}..{max(times['shadowed']):.1f}): + {res['increase_us']:.1f} us, "
          f"{100 * res['shadow_share_of_step']:.1f} % of the step; the shadow pass marched {st['samples']} samples in {st['trips']} trips, the frame "
          f"{main['samples']} in {main['trips']}", flush=True)
    del hs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--H", type=int, default=800)
    ap.add_argument("--S", type=int, default=256, help="map resolution of the launch measurement")
    ap.add_argument("--reps", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--res", type=int, nargs="*", default=[128, 256, 512], help="map resolutions of the step measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_shadows.py measures on a GPU; none is visible")
    out = dict(launch=measure_launch(args.W, args.H, args.S, args.reps, args.rounds),
               step=[measure_step(args.W, args.H, S, args.steps, args.rounds) for S in args.res])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
