#!/usr/bin/env python
"""The contact launches (csrc/pn_contact.hip: k_contact_points + k_contact_rhs, and the one-launch form in which every entry evaluates its point itself)
on the GPU, on the chair and on the 268 k-point cloud of bench.py --config stress: each form alone, and the two-launch form as the increase of a captured
substep.  --cases: `floor` (a floor and a sphere), `boxes` (all eight slots hold boxes: eight slabs side by side whose tops are that floor),
`capsules` (all eight hold capsules: a grating of eight rods whose tops touch that floor's height).
    python tools/time_contact.py [--clouds chair,stress] [--cases floor,boxes,capsules] [--reps 1000] [--rounds 5] [--out FILE.json]
HIP events around graph replays on one stream.  Alone: a graph of 50 repetitions, so the figure is the launch's time on a busy stream and not a graph launch's
latency.  Substep: two simulators on the same cloud, one with a floor under the standing object (so that a realistic share of the integration points is
in contact) and a solid sphere beside it, their captured substeps replayed in alternating rounds; the medians over the rounds and their difference are
reported with the rounds' spread."""
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

LAUNCHES = 50


def make_sim(o, c, contact, case="floor"):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    if contact:
        sim.enable_contact()
        floor = float(np.asarray(c["pos"])[:, 1].min())     # the object stands on it: its lowest layers of integration points are in contact
        if case == "floor":
            sim.add_plane((0.0, floor, 0.0), (0.0, 1.0, 0.0))
            sim.add_sphere((0.0, 0.0, 0.9), 0.5)
        elif case == "boxes":       # eight slabs of width 0.25 side by side along x: together the floor under the object, seams included
            for k in range(8):
                sim.add_box((-0.875 + 0.25 * k, floor - 0.1, 0.0), (0.125, 0.1, 1.0))
        elif case == "capsules":    # eight rods along z, 0.25 apart: a grating under the object
            for k in range(8):
                x = -0.875 + 0.25 * k
                sim.add_capsule((x, floor - 0.1, -1.0), (x, floor - 0.1, 1.0), 0.1)
        else:
            raise SystemExit(f"time_contact.py: no case {case!r} (floor, boxes, capsules)")
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


def measure(name, o, c, reps, rounds, case="floor"):
    plain, con = make_sim(o, c, False), make_sim(o, c, True, case)
    for s in (plain, con):
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    in_contact = con.contact_count()
    keep = [(s.dof.clone(), s.dof_vel.clone()) for s in (plain, con)]
    st = torch.cuda.Stream()
    g_alone = graph_of(lambda: con._enqueue_contact_rhs(con.rhs_gravity), st, LAUNCHES)
    g_one = graph_of(lambda: con._enqueue_contact_rhs(con.rhs_gravity, one_launch=True), st, LAUNCHES)
    g_plain, g_con = graph_of(plain.stepforward, st), graph_of(con.stepforward, st)
    alone, one, t_plain, t_con = [], [], [], []
    for _ in range(rounds):   # alternating: other work shares the machine
        for s, k in zip((plain, con), keep):   # every round times the same stretch of the trajectory
            s.dof.copy_(k[0])
            s.dof_vel.copy_(k[1])
        t_plain.append(time_graph(g_plain, st, reps) * 1e3)
        t_con.append(time_graph(g_con, st, reps) * 1e3)
        alone.append(time_graph(g_alone, st, reps) * 1e3 / LAUNCHES)
        one.append(time_graph(g_one, st, reps) * 1e3 / LAUNCHES)
    runs = con.kernel_cnt.cpu().numpy()
    med = statistics.median
    res = dict(cloud=name, case=case, points=int(len(c["pin"])), n_k=con.n_k, n_IP=con.n_IP, longest_run=int(runs.max()), sim_iters=int(o["sim_iters"]),
               in_contact_after_10=in_contact, in_contact_at_end=con.contact_count(), contact_two_launches_us=med(alone), contact_two_launches_us_rounds=alone, contact_one_launch_us=med(one), contact_one_launch_us_rounds=one,
               substep_us=med(t_plain), substep_us_rounds=t_plain, substep_with_contact_us=med(t_con), substep_with_contact_us_rounds=t_con,
               increase_us=med(t_con) - med(t_plain), max_disp_plain=float((plain.dof - plain.dof_rest).abs().max()),
               max_disp_contact=float((con.dof - con.dof_rest).abs().max()))
    print(f"{name}, {case}: {res['points']} points, n_IP {res['n_IP']}, n_k {res['n_k']}, longest run {res['longest_run']}, {in_contact} points in contact: contact alone, two launches "
          f"{res['contact_two_launches_us']:.2f} us ({min(alone):.2f}..{max(alone):.2f}), one launch {res['contact_one_launch_us']:.2f} us ({min(one):.2f}..{max(one):.2f}); substep {res['substep_us']:.1f} us ({min(t_plain):.1f}..{max(t_plain):.1f}), with contact "
          f"{res['substep_with_contact_us']:.1f} us ({min(t_con):.1f}..{max(t_con):.1f}): + {res['increase_us']:.2f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="chair,stress")
    ap.add_argument("--cases", default="floor,boxes,capsules")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_contact.py measures on a GPU; none is visible")
    out = []
    for name in args.clouds.split(","):
        o = scene.default_opt() if name == "chair" else scene.stress_opt()
        c = scene.make_chair_points(hgs=o["hash_grid_size"]) if name == "chair" else scene.make_chair_points(sub_res=o["sub_res"], hgs=o["hash_grid_size"])
        for case in args.cases.split(","):
            out.append(measure(name, o, c, args.reps, args.rounds, case))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
