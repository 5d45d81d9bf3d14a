#!/usr/bin/env python
"""The kinematic pins' per-substep launch (csrc/pn_pins.hip: k_pin_rhs + k_pin_tick) on the GPU, on the chair and on the 268 k-point cloud of
bench.py --config stress: the launch pair alone, and as the increase of a captured substep.
    python tools/time_pins.py [--clouds chair,stress] [--reps 1000] [--rounds 5] [--out FILE.json]
HIP events around graph replays on one stream.  Alone: a graph of 50 launch pairs, so the figure is the pair's time on a busy stream and not a graph launch's
latency.  Substep: two simulators on the same cloud, one with pin motion (shake + twist), their captured substeps replayed in alternating rounds; the medians
over the rounds and their difference are reported with the rounds' spread."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.simulator.solver import Simulator  # noqa: E402

PAIRS = 50


def make_sim(o, c, pins):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    if pins:
        sim.enable_pin_motion()
        sim.set_pin_motion(translate=((0.05, 0.02, -0.03), 2.0), rotate=((0.0, 1.0, 0.0), 10.0, 1.0))
    return sim


def graph_of(fn, stream, n=1):
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(n):
            fn()
    return g


def time_graph(g, stream, reps):
    """ms per replay over `reps` replays (after 20 more to warm up)."""
    with torch.cuda.stream(stream):
        for _ in range(20):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            g.replay()
        e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(name, o, c, reps, rounds):
    plain, pins = make_sim(o, c, False), make_sim(o, c, True)
    for s in (plain, pins):
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g_alone = graph_of(pins._enqueue_pin_rhs, st, PAIRS)
    g_plain, g_pins = graph_of(plain.stepforward, st), graph_of(pins.stepforward, st)
    alone, t_plain, t_pins = [], [], []
    for _ in range(rounds):   # alternating: other work shares the machine
        t_plain.append(time_graph(g_plain, st, reps) * 1e3)
        t_pins.append(time_graph(g_pins, st, reps) * 1e3)
        alone.append(time_graph(g_alone, st, reps) * 1e3 / PAIRS)
    runs = np.diff(pins.pin_bg.cpu().numpy())
    med = statistics.median
    res = dict(cloud=name, points=int(len(c["pin"])), n_pin=pins.n_pin, n_k=pins.n_k, n_IP=pins.n_IP, longest_run=int(runs.max()), sim_iters=int(o["sim_iters"]),
               pin_launch_pair_us=med(alone), pin_launch_pair_us_rounds=alone, substep_us=med(t_plain), substep_us_rounds=t_plain,
               substep_with_pins_us=med(t_pins), substep_with_pins_us_rounds=t_pins, increase_us=med(t_pins) - med(t_plain),
               max_disp_plain=float((plain.dof - plain.dof_rest).abs().max()), max_disp_pins=float((pins.dof - pins.dof_rest).abs().max()))
    print(f"{name}: {res['points']} points, {res['n_pin']} pins, n_k {res['n_k']}, longest run {res['longest_run']}: pin launch pair alone {res['pin_launch_pair_us']:.2f} us "
          f"({min(alone):.2f}..{max(alone):.2f}); substep {res['substep_us']:.1f} us ({min(t_plain):.1f}..{max(t_plain):.1f}), with pins "
          f"{res['substep_with_pins_us']:.1f} us ({min(t_pins):.1f}..{max(t_pins):.1f}): + {res['increase_us']:.2f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="chair,stress")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pins.py measures on a GPU; none is visible")
    out = []
    for name in args.clouds.split(","):
        o = scene.default_opt() if name == "chair" else scene.stress_opt()
        c = scene.make_chair_points(hgs=o["hash_grid_size"]) if name == "chair" else scene.make_chair_points(sub_res=o["sub_res"], hgs=o["hash_grid_size"])
        out.append(measure(name, o, c, args.reps, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
