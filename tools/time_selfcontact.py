#!/usr/bin/env python
"""The self-contact stage's launches (csrc/pn_selfcontact.hip: points, count, scan, fill, sort, S_i, a_i and the per-kernel sum) on the GPU, on the chair
and on the cloud of bench.py --config stress: the stage alone, at rest (every neighbour visited, none eligible) and squeezed to a quarter of its height
(about half the points in contact), and a captured substep with and without the stage.
    python tools/time_selfcontact.py [--clouds chair,stress] [--reps 1000] [--rounds 5] [--out FILE.json]
HIP events around graph replays on one stream.  Alone: a graph of 50 repetitions, so the figure is the launches' time on a busy stream and not a graph
launch's latency.  Substep: two simulators on the same cloud, one with the stage enabled, their captured substeps replayed in alternating rounds; the
medians over the rounds and their difference are reported with the rounds' spread."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd._lib import lib  # noqa: E402
from pienerf_amd.simulator.solver import Simulator  # noqa: E402

REPEATS = 50


def make_sim(o, c, stage):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    if stage:
        sim.enable_self_contact()
    return sim


def squeezed_dof(sim, A):
    """dof of the global map x = A X: translation = A kernel_pos, affine columns = A."""
    dof = torch.zeros((sim.n_k, 10, 3), dtype=torch.float64, device=sim.device)
    At = torch.tensor(np.asarray(A, np.float64).T, device=sim.device)
    dof[:, 0, :] = sim.kernel_pos.to(torch.float64) @ At
    dof[:, 1:4, :] = At
    return dof.reshape(-1)


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
    plain, staged = make_sim(o, c, False), make_sim(o, c, True)
    sims = [plain, staged]
    rest = staged.dof.clone()
    squeezed = squeezed_dof(staged, np.diag([1.0, 0.25, 1.0]))
    st = torch.cuda.Stream()
    alone = {}
    for state, dof in (("rest", rest), ("squeezed", squeezed)):   # the stage alone, on a fixed state
        staged.dof.copy_(dof)
        g = graph_of(lambda: staged._enqueue_self_rhs(staged.rhs_gravity), st, REPEATS)
        alone[state] = [time_graph(g, st, max(reps // 10, 20)) * 1e3 / REPEATS for _ in range(rounds)]
        alone[state + "_points_in_contact"] = staged.self_contact_count()
    staged.dof.copy_(rest)
    for s in sims:
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    keep = [(s.dof.clone(), s.dof_vel.clone()) for s in sims]
    graphs = [graph_of(s.stepforward, st) for s in sims]
    t_step = [[], []]
    for _ in range(rounds):   # alternating: other work shares the machine
        for s, k in zip(sims, keep):   # every round times the same stretch of the trajectory
            s.dof.copy_(k[0])
            s.dof_vel.copy_(k[1])
        for t, g in zip(t_step, graphs):
            t.append(time_graph(g, st, reps) * 1e3)
    med = statistics.median
    res = dict(cloud=name, points=int(len(c["pin"])), n_k=plain.n_k, n_IP=plain.n_IP, sim_iters=int(o["sim_iters"]), launches=int(lib().pn_sim_self_launches()),
               buckets=int(2 ** int(np.ceil(np.log2(max(1024, 2 * plain.n_IP))))), work_bytes=int(lib().pn_sim_self_work_bytes(plain.n_IP)),
               stage_at_rest_us=med(alone["rest"]), stage_at_rest_us_rounds=alone["rest"], stage_squeezed_us=med(alone["squeezed"]),
               stage_squeezed_us_rounds=alone["squeezed"], squeezed_points_in_contact=alone["squeezed_points_in_contact"],
               substep_us=med(t_step[0]), substep_us_rounds=t_step[0], substep_with_stage_us=med(t_step[1]), substep_with_stage_us_rounds=t_step[1],
               increase_us=med(t_step[1]) - med(t_step[0]), overflows=staged.self_contact_overflows())
    print(f"{name}: {res['points']} points, n_IP {res['n_IP']}, n_k {res['n_k']}, {res['buckets']} buckets, {res['launches']} launches: the stage alone at rest "
          f"{res['stage_at_rest_us']:.2f} us ({min(alone['rest']):.2f}..{max(alone['rest']):.2f}), squeezed ({res['squeezed_points_in_contact']} points in contact) "
          f"{res['stage_squeezed_us']:.2f} us ({min(alone['squeezed']):.2f}..{max(alone['squeezed']):.2f}); substep {res['substep_us']:.1f} us "
          f"({min(t_step[0]):.1f}..{max(t_step[0]):.1f}), with the stage {res['substep_with_stage_us']:.1f} us ({min(t_step[1]):.1f}..{max(t_step[1]):.1f}): "
          f"+ {res['increase_us']:.2f} us; {res['overflows']} overflowed calls", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="chair,stress")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_selfcontact.py measures on a GPU; none is visible")
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
