#!/usr/bin/env python
"""The block-sparse PCG global solve (Simulator(solver='pcg'), csrc/pn_sim_pcg.h) on the chair at kres 7, 11 and 15, with the dense form beside it where
it fits (kres 7 and 11):
    python tools/time_pcg.py [--kres 7,11,15] [--dense 7,11] [--reps 20] [--rounds 3] [--out FILE.json]
    python tools/time_pcg.py --reference-counts [--kres 7,11,15]      (CPU only: the numpy reference's iteration counts, cold start, tol 1e-10)
Per kres: substep time (HIP events around `reps` eager substeps on one stream, ending in a synchronise; the solver's cost includes the launches the host
enqueues up to the cap, so eager substeps are what a user pays), CG iterations per substep (per solve the largest of the three columns' counts, summed over
the local/global iterations, from Simulator.pcg_stats()), CG iterations per second, and the product alone (a graph of 50 pn_sim_bsr_matvec3 launches) as
GB/s against its algorithmic bytes nnzb * 800 + 2 * 240 * n_k.  A second pcg simulator with the cap set to 1.25 x the largest count seen shows what the
launches behind the last iteration cost.  Rounds alternate between the simulators; medians and ranges are reported."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pienerf_amd import scene  # noqa: E402
from pienerf_amd.simulator.solver import Simulator  # noqa: E402

LAUNCHES = 50
FORCE = (300.0, 100.0, -200.0)   # bench.py's pick force


def make_sim(o, c, kres, solver, device="cuda:0", **kw):
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device=device, persistent=False, kres=kres, solver=solver, **kw)
    if device == "cpu":
        sim.initialize = sim.precompute
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    return sim


def time_substeps(sim, keep, reps):
    """ms per eager substep over `reps` substeps from the kept state (3 more first)."""
    sim.dof.copy_(keep[0])
    sim.dof_vel.copy_(keep[1])
    sim.reset_warm_start()
    for _ in range(3):
        sim.stepforward()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        sim.stepforward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_spmv(sim, reps):
    """us per pn_sim_bsr_matvec3 with the system block, from a graph of LAUNCHES products."""
    st = torch.cuda.Stream()
    x = torch.randn(sim.n_k * 30, dtype=torch.float64, device=sim.device)
    with torch.cuda.stream(st):
        for _ in range(3):
            sim._bsr_matvec(sim.bsr_A, x)
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for _ in range(LAUNCHES):
            sim._bsr_matvec(sim.bsr_A, x)
    with torch.cuda.stream(st):
        for _ in range(20):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            g.replay()
        e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) / reps / LAUNCHES * 1e3


def cg_per_substep(sim):
    st = sim.pcg_stats()
    return int(st["iterations"].max(axis=1).sum()), st


def measure(o, c, kres, with_dense, reps, rounds):
    sims = {"pcg": make_sim(o, c, kres, "pcg")}
    if with_dense:
        sims["dense"] = make_sim(o, c, kres, "dense")
    vid = sims["pcg"].n_IP // 2
    for s in sims.values():
        s.update_force(vid, torch.tensor(FORCE, dtype=torch.float64))
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    p = sims["pcg"]
    _, st = cg_per_substep(p)
    sims["pcg_tight"] = make_sim(o, c, kres, "pcg", pcg_max_iters=int(np.ceil(1.25 * st["iterations_max"])))
    sims["pcg_tight"].update_force(vid, torch.tensor(FORCE, dtype=torch.float64))
    keep = (p.dof.clone(), p.dof_vel.clone())
    t = {k: [] for k in sims}
    cg = {}
    for _ in range(rounds):   # alternating: other work shares the machine
        for k, s in sims.items():
            t[k].append(time_substeps(s, keep, reps))
            if k != "dense":
                cg[k] = cg_per_substep(s)
    med = statistics.median
    n_cg, st = cg["pcg"]
    spmv_us = time_spmv(p, 200)
    nnzb = int(p.bsr_col.numel())
    nbytes = nnzb * 800 + 2 * 240 * p.n_k
    res = dict(kres=kres, n_k=p.n_k, active=int(p.active_kernels.numel()), n_IP=p.n_IP, nnzb=nnzb, blocks_per_row_max=int(torch.diff(p.bsr_rowptr).max()),
               sim_iters=int(o["sim_iters"]), tol=p.pcg_tol, cap=p.pcg_max_iters, unconverged=st["unconverged"], iterations_max=st["iterations_max"],
               cg_iterations_per_substep=n_cg, substep_ms=med(t["pcg"]), substep_ms_rounds=t["pcg"], cg_iterations_per_s=n_cg / (med(t["pcg"]) * 1e-3),
               tight_cap=sims["pcg_tight"].pcg_max_iters, tight_substep_ms=med(t["pcg_tight"]), tight_substep_ms_rounds=t["pcg_tight"],
               tight_unconverged=cg["pcg_tight"][1]["unconverged"], tight_cg_iterations_per_s=cg["pcg_tight"][0] / (med(t["pcg_tight"]) * 1e-3),
               spmv_us=spmv_us, spmv_bytes=nbytes, spmv_GBps=nbytes / (spmv_us * 1e-6) / 1e9,
               matrix_MB=(2 * nnzb * 800 + p.n_k * 800) / 1e6, dense_matrix_MB=(p.n_k * 10) ** 2 * 8 / 1e6)
    if with_dense:
        d = sims["dense"]
        res.update(dense_substep_ms=med(t["dense"]), dense_substep_ms_rounds=t["dense"],
                   pcg_vs_dense_rel=float((p.dof - d.dof).abs().max() / (d.dof - d.dof_rest).abs().max()))
    print(f"kres {kres}: n_k {res['n_k']} ({res['active']} active), n_IP {res['n_IP']}, {nnzb} blocks (row max {res['blocks_per_row_max']}), BSR {res['matrix_MB']:.1f} MB "
          f"(dense would be {res['dense_matrix_MB']:.0f} MB each); substep {res['substep_ms']:.2f} ms ({min(t['pcg']):.2f}..{max(t['pcg']):.2f}) at cap {res['cap']}, "
          f"{n_cg} CG iterations per substep (max {res['iterations_max']} per solve, {res['unconverged']} unconverged), {res['cg_iterations_per_s']:.0f} CG iterations/s; "
          f"cap {res['tight_cap']}: {res['tight_substep_ms']:.2f} ms ({min(t['pcg_tight']):.2f}..{max(t['pcg_tight']):.2f}), {res['tight_cg_iterations_per_s']:.0f} CG iterations/s, "
          f"{res['tight_unconverged']} unconverged; product alone {spmv_us:.2f} us = {res['spmv_GBps']:.0f} GB/s of its {nbytes / 1e6:.2f} MB"
          + (f"; dense substep {res['dense_substep_ms']:.3f} ms ({min(t['dense']):.3f}..{max(t['dense']):.3f}), pcg vs dense after the run {res['pcg_vs_dense_rel']:.2e}"
             if with_dense else ""), flush=True)
    return res


def reference_counts(o, c, kres_list):
    """The numpy reference (tests/pcg_reference.py) on the CPU: iterations to |r| <= 1e-10 |b| from a cold start for gravity and for seeded noise."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pcg_reference as R
    out = []
    for kres in kres_list:
        s = make_sim(o, c, kres, "pcg", device="cpu")
        args = (s.bsr_rowptr.numpy(), s.bsr_col.numpy(), s.bsr_A.numpy(), s.bsr_Dinv.numpy(), s.bsr_active.numpy())
        g = s.rhs_gravity.numpy().reshape(-1, 3)
        row = dict(kres=kres, n_k=s.n_k, active=int(s.active_kernels.numel()), nnzb=int(s.bsr_col.numel()))
        for label, B in (("gravity", g), ("noise", np.random.default_rng(3).normal(size=g.shape) * np.abs(g).max())):
            X, it, flag = R.pcg(*args, B, np.zeros_like(B), 1e-10, 4096)
            res = R.true_residual(*args[:3], args[4], B, X)
            row[label] = dict(iterations=it.tolist(), converged=bool((flag == R.CONVERGED).all()), true_residual=[float(v) for v in np.nan_to_num(res)])
        print(row, flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kres", default="7,11,15")
    ap.add_argument("--dense", default="7,11", help="kernel grids at which the dense form runs beside the pcg one")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference-counts", dest="reference_counts", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    o = scene.default_opt()
    c = scene.make_chair_points(hgs=o["hash_grid_size"])
    kres = [int(k) for k in args.kres.split(",")]
    if args.reference_counts:
        out = reference_counts(o, c, kres)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("time_pcg.py measures on a GPU; none is visible (--reference-counts runs on the CPU)")
        dense = [int(k) for k in args.dense.split(",") if k]
        out = [measure(o, c, k, k in dense, args.reps, args.rounds) for k in kres]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
