#!/usr/bin/env python
"""The diagnostics launch pair (Simulator.diagnostics: k_diag_points + k_diag_finish) beside one substep of the same simulator, on the chair and on the
stress cloud: us per call of each from a captured graph, and their ratio.
    python tools/time_diagnostics.py [--reps 300] [--config chair|stress|both]
The substep's figure is tools/time_sim.py's on the same box; a state a few substeps into a pick force is what is measured (the SVD's sweep count
depends on the state)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.simulator.solver import Simulator  # noqa: E402


def graph_us(fn, reps):
    """us per replay of fn() captured into a graph on a stream of its own: 20 replays to warm up, then `reps` between two events."""
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    with torch.cuda.stream(s):
        for _ in range(20):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            g.replay()
        e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(name, reps):
    o = scene.default_opt() if name == "chair" else scene.stress_opt()
    c = scene.make_chair_points(hgs=o["hash_grid_size"]) if name == "chair" else scene.make_chair_points(sub_res=o["sub_res"], hgs=o["hash_grid_size"])
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device="cuda:0", persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    sim.update_force(sim.n_IP // 2, torch.tensor([300.0, 100.0, -200.0], dtype=torch.float64))
    for _ in range(20):
        sim.stepforward()
    row = torch.empty(25, dtype=torch.float64, device=sim.device)
    rec = torch.empty((sim.n_IP, 8), dtype=torch.float64, device=sim.device)
    sim.diagnostics(out=row, per_point=rec)   # the work area is made on first use: before the capture
    torch.cuda.synchronize()
    keep = sim.keep_state()
    t_row = graph_us(lambda: sim.diagnostics(out=row), reps)
    t_rec = graph_us(lambda: sim.diagnostics(out=row, per_point=rec), reps)
    d = sim.read_diagnostics(row)
    sim.restore_state(keep)
    t_step = graph_us(sim.stepforward, reps)
    return dict(config=name, n_k=sim.n_k, n_IP=sim.n_IP, sim_iters=int(sim.iters), diagnostics_us=round(t_row, 2), diagnostics_with_per_point_us=round(t_rec, 2),
                substep_us=round(t_step, 2), ratio=round(t_row / t_step, 4), kinetic=d["kinetic"], elastic=d["elastic"], strain_max=d["strain_max"],
                nonfinite=d["nonfinite"], inverted=d["inverted"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--config", choices=("chair", "stress", "both"), default="both")
    args = ap.parse_args()
    for name in (("chair", "stress") if args.config == "both" else (args.config,)):
        print(json.dumps(measure(name, args.reps)), flush=True)
