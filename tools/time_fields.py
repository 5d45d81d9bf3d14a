#!/usr/bin/env python
"""The force-field stage's launches (csrc/pn_fields.hip: k_field_points + k_field_rhs + k_field_tick) on the GPU, on the chair (3 576 integration
points): the stage alone, and a captured substep with and without a wind.
    python tools/time_fields.py [--reps 1000] [--rounds 5] [--out FILE.json]
HIP events around graph replays on one stream.  Alone: a graph of 50 repetitions, so the figure is the launches' time on a busy stream and not a graph
launch's latency.  Substep: two simulators on the same cloud, one in a gusty wind (what main_render --wind 5 0 0 --gust 0.5 1 sets up), their captured
substeps replayed in alternating rounds; the medians over the rounds and their difference are reported with the rounds' spread.  On a tree without
force fields (the parent commit, for the comparison of DESIGN.md 4.15) the plain substep alone is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.simulator.solver import Simulator  # noqa: E402

LAUNCHES = 50
HAS_FIELDS = hasattr(Simulator, "enable_fields")


def make_sim(o, c, wind):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    if wind:
        sim.enable_fields()
        sim.add_wind((5.0, 0.0, 0.0), drag=2.0, gust=0.5, hz=1.0)
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


def measure(o, c, reps, rounds):
    sims = [make_sim(o, c, False)] + ([make_sim(o, c, True)] if HAS_FIELDS else [])
    for s in sims:
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    keep = [(s.dof.clone(), s.dof_vel.clone()) for s in sims]
    st = torch.cuda.Stream()
    plain = sims[0]
    graphs = [graph_of(s.stepforward, st) for s in sims]
    g_alone = graph_of(lambda: sims[1]._enqueue_fields_rhs(sims[1].rhs_gravity), st, LAUNCHES) if HAS_FIELDS else None
    t_step, alone = [[] for _ in sims], []
    for _ in range(rounds):   # alternating: other work shares the machine
        for s, k in zip(sims, keep):   # every round times the same stretch of the trajectory
            s.dof.copy_(k[0])
            s.dof_vel.copy_(k[1])
            if getattr(s, "fields_enabled", False):
                s.reset_field_clock(10)
        for t, g in zip(t_step, graphs):
            t.append(time_graph(g, st, reps) * 1e3)
        if g_alone is not None:
            alone.append(time_graph(g_alone, st, reps) * 1e3 / LAUNCHES)
    med = statistics.median
    res = dict(cloud="chair", points=int(len(c["pin"])), n_k=plain.n_k, n_IP=plain.n_IP, sim_iters=int(o["sim_iters"]), force_fields=HAS_FIELDS,
               substep_us=med(t_step[0]), substep_us_rounds=t_step[0], max_disp_plain=float((plain.dof - plain.dof_rest).abs().max()))
    said = f"chair: {res['points']} points, n_IP {res['n_IP']}, n_k {res['n_k']}: substep {res['substep_us']:.1f} us ({min(t_step[0]):.1f}..{max(t_step[0]):.1f})"
    if HAS_FIELDS:
        w = sims[1]
        res.update(fields_three_launches_us=med(alone), fields_three_launches_us_rounds=alone, substep_with_wind_us=med(t_step[1]),
                   substep_with_wind_us_rounds=t_step[1], increase_us=med(t_step[1]) - med(t_step[0]),
                   max_disp_wind=float((w.dof - w.dof_rest).abs().max()))
        said += (f", in a wind {res['substep_with_wind_us']:.1f} us ({min(t_step[1]):.1f}..{max(t_step[1]):.1f}): + {res['increase_us']:.2f} us; the stage alone, three launches "
                 f"{res['fields_three_launches_us']:.2f} us ({min(alone):.2f}..{max(alone):.2f})")
    print(said, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fields.py measures on a GPU; none is visible")
    o = scene.default_opt()
    c = scene.make_chair_points(hgs=o["hash_grid_size"])
    out = [measure(o, c, args.reps, args.rounds)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
