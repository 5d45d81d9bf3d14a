#!/usr/bin/env python
"""The rigid balls' launches (csrc/pn_bodies.hip: k_body_reaction + k_body_step, and the one-launch form in which the last workgroup to arrive does the
second launch's work) on the GPU, on the chair and on the 268 k-point cloud of bench.py --config stress: each form alone, and the two-launch form as the
increase of a captured substep over the same build with the same sphere as a kinematic collider.
    python tools/time_bodies.py [--clouds chair,stress] [--reps 1000] [--rounds 5] [--out FILE.json]
HIP events around graph replays on one stream.  Alone: a graph of 50 repetitions on a ball that overlaps the object and is too heavy to move, so every
repetition sums the same reaction.  Substep: two simulators on the same cloud with a floor under the standing object and a sphere in reach of it, dynamic
in one and kinematic in the other, their captured substeps replayed in alternating rounds from the same kept state; the medians over the rounds and
their difference are reported with the rounds' spread."""
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
from time_contact import graph_of, time_graph  # noqa: E402

LAUNCHES = 50
BALL = dict(centre=(0.0, 0.0, 0.9), radius=0.5)


def make_sim(o, c, dynamic, mass=200.0):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    sim.enable_contact()
    floor = float(np.asarray(c["pos"])[:, 1].min())     # the object stands on it, as in time_contact.py
    sim.add_plane((0.0, floor, 0.0), (0.0, 1.0, 0.0))
    if dynamic:
        sim.enable_bodies(gravity=(0.0, 0.0, 0.0))
        sim.ball = sim.add_body(mass=mass, **BALL)
    else:
        sim.ball = sim.add_sphere(**BALL)
    return sim


def measure(name, o, c, reps, rounds):
    kin, dyn, still = make_sim(o, c, False), make_sim(o, c, True), make_sim(o, c, True, mass=1e15)
    for s in (kin, dyn):
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    touching = int((dyn.contact_accel() != 0.0).any(dim=1).sum().item())
    keep = [s.keep_state() for s in (kin, dyn)]
    st = torch.cuda.Stream()
    g_two = graph_of(lambda: still._enqueue_bodies(still.rhs_gravity), st, LAUNCHES)
    g_one = graph_of(lambda: still._enqueue_bodies(still.rhs_gravity, one_launch=True), st, LAUNCHES)
    g_kin, g_dyn = graph_of(kin.stepforward, st), graph_of(dyn.stepforward, st)
    two, one, t_kin, t_dyn = [], [], [], []
    for _ in range(rounds):   # alternating: other work shares the machine
        for s, k in zip((kin, dyn), keep):   # every round times the same stretch of the trajectory
            s.restore_state(k)
        t_kin.append(time_graph(g_kin, st, reps) * 1e3)
        t_dyn.append(time_graph(g_dyn, st, reps) * 1e3)
        two.append(time_graph(g_two, st, reps) * 1e3 / LAUNCHES)
        one.append(time_graph(g_one, st, reps) * 1e3 / LAUNCHES)
    b = still.body_state()[still.ball]
    med = statistics.median
    res = dict(cloud=name, points=int(len(c["pin"])), n_k=dyn.n_k, n_IP=dyn.n_IP, workgroups=(dyn.n_IP + 255) // 256, sim_iters=int(o["sim_iters"]),
               in_contact_after_10=touching, reaction_on_the_still_ball=float(np.linalg.norm(b["reaction"])), bodies_two_launches_us=med(two),
               bodies_two_launches_us_rounds=two, bodies_one_launch_us=med(one), bodies_one_launch_us_rounds=one, substep_kinematic_us=med(t_kin),
               substep_kinematic_us_rounds=t_kin, substep_with_body_us=med(t_dyn), substep_with_body_us_rounds=t_dyn, increase_us=med(t_dyn) - med(t_kin))
    print(f"{name}: {res['points']} points, n_IP {res['n_IP']} ({res['workgroups']} workgroups), {touching} points in contact, |F| on the still ball "
          f"{res['reaction_on_the_still_ball']:.3e}: bodies alone, two launches {res['bodies_two_launches_us']:.2f} us ({min(two):.2f}..{max(two):.2f}), one launch "
          f"{res['bodies_one_launch_us']:.2f} us ({min(one):.2f}..{max(one):.2f}); substep with the sphere kinematic {res['substep_kinematic_us']:.1f} us "
          f"({min(t_kin):.1f}..{max(t_kin):.1f}), as a body {res['substep_with_body_us']:.1f} us ({min(t_dyn):.1f}..{max(t_dyn):.1f}): "
          f"+ {res['increase_us']:.2f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="chair,stress")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bodies.py measures on a GPU; none is visible")
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
