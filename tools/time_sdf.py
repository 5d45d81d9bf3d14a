#!/usr/bin/env python
"""Mesh colliders on the GPU (csrc/pn_sdf.hip): the grid build, the contact stage with a grid, and the substep with a floor as a plane
against the same floor as a grid.
    python tools/time_sdf.py [--res 64] [--mesh_resolution 128] [--reps 1000] [--rounds 5] [--out FILE.json]
The build: SdfGrid's launch (pn_sdf_build) at --res^3 nodes against the chair's rest mesh (the shaped synthetic field's level set, marching cubes at
--mesh_resolution), HIP events around each of --rounds launches; the cost is nodes x triangles and the pair rate is reported with it.  The stage:
_enqueue_contact_rhs with the floor as a plane (two launches) and with the same floor as a grid (three), each as a graph of 50 repetitions.  The
substep: two simulators on the chair, one with the floor as a plane (the path that exists without this feature), one with the floor as a 64^3 grid,
their captured substeps replayed in alternating rounds; medians over the rounds."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene  # noqa: E402
from pienerf_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from pienerf_amd.sdf import SdfGrid, clean_triangles  # noqa: E402
from time_contact import LAUNCHES, graph_of, time_graph  # noqa: E402

DEV = "cuda:0"


def chair_mesh(resolution, threshold=10.0):
    from pienerf_amd.harness import SimRenderHarness
    from pienerf_amd.mesh import density_query
    from pienerf_amd.nerf.utils import extract_geometry
    o = scene.default_opt(W=64, H=64)
    h = SimRenderHarness(o, cloud=scene.make_chair_points(hgs=o["hash_grid_size"]), ckpt=scene.make_checkpoint(bound=o["bound"], shaped=True), device=DEV)
    m = h.model
    return extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], resolution, threshold, density_query(m))


def time_build(v, t, res, rounds):
    lo, s, shape = SdfGrid.box_for(v, resolution=res)
    tri9, dropped = clean_triangles(v, t)
    nx, ny, nz = shape
    tri = torch.from_numpy(tri9).to(DEV)
    values = torch.empty((nz, ny, nx), dtype=torch.float32, device=DEV)
    lo_c = np.ascontiguousarray(lo, dtype=np.float64)
    ms = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().pn_sdf_build(ptr(tri), len(tri9), nx, ny, nz, lo_c.ctypes.data, s, ptr(values), None, stream_ptr()), "sdf_build")
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]   # the first launch loads the code object
    pairs = nx * ny * nz * len(tri9)
    med = statistics.median(ms)
    print(f"build: {nx} x {ny} x {nz} nodes x {len(tri9)} triangles ({dropped} dropped) = {pairs:.3e} pairs: {med:.2f} ms ({min(ms):.2f}..{max(ms):.2f}), "
          f"{pairs / med * 1e-6:.1f} G pairs/s", flush=True)
    return dict(nodes=[nx, ny, nz], triangles=len(tri9), dropped=dropped, pairs=pairs, build_ms=med, build_ms_rounds=ms, gpairs_per_s=pairs / med * 1e-6)


def make_sim(o, c, floor_as):
    from pienerf_amd.simulator.solver import Simulator
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device=DEV, persistent=False)
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    sim.enable_contact()
    y = float(np.asarray(c["pos"])[:, 1].min())     # the object stands on it
    if floor_as == "plane":
        sim.add_plane((0.0, y, 0.0), (0.0, 1.0, 0.0))
    else:
        s = 2.2 / 63
        sim.add_mesh_collider(SdfGrid.from_function(lambda p: p[:, 1] - y, (-1.1, -1.1, -1.1), s, (64, 64, 64), device=DEV))
    return sim


def time_stage(reps, rounds):
    o = scene.default_opt()
    c = scene.make_chair_points(hgs=o["hash_grid_size"])
    plane, grid = make_sim(o, c, "plane"), make_sim(o, c, "grid")
    for s in (plane, grid):
        for _ in range(10):
            s.stepforward()
    torch.cuda.synchronize()
    counts = (plane.contact_count(), grid.contact_count())
    keep = [(s.dof.clone(), s.dof_vel.clone()) for s in (plane, grid)]
    st = torch.cuda.Stream()
    g_a_plane = graph_of(lambda: plane._enqueue_contact_rhs(plane.rhs_gravity), st, LAUNCHES)
    g_a_grid = graph_of(lambda: grid._enqueue_contact_rhs(grid.rhs_gravity), st, LAUNCHES)
    g_plane, g_grid = graph_of(plane.stepforward, st), graph_of(grid.stepforward, st)
    a_plane, a_grid, t_plane, t_grid = [], [], [], []
    for _ in range(rounds):   # alternating: other work shares the machine
        for s, k in zip((plane, grid), keep):
            s.dof.copy_(k[0])
            s.dof_vel.copy_(k[1])
        t_plane.append(time_graph(g_plane, st, reps) * 1e3)
        t_grid.append(time_graph(g_grid, st, reps) * 1e3)
        a_plane.append(time_graph(g_a_plane, st, reps) * 1e3 / LAUNCHES)
        a_grid.append(time_graph(g_a_grid, st, reps) * 1e3 / LAUNCHES)
    med = statistics.median
    gap = float((plane.dof - grid.dof).abs().max())
    print(f"chair, n_IP {plane.n_IP}, {counts[0]} / {counts[1]} points in contact (plane / grid): stage alone {med(a_plane):.2f} us as a plane (two launches, "
          f"{min(a_plane):.2f}..{max(a_plane):.2f}), {med(a_grid):.2f} us as a grid (three, {min(a_grid):.2f}..{max(a_grid):.2f}); substep {med(t_plane):.1f} us "
          f"({min(t_plane):.1f}..{max(t_plane):.1f}) with the plane, {med(t_grid):.1f} us ({min(t_grid):.1f}..{max(t_grid):.1f}) with the grid: "
          f"+ {med(t_grid) - med(t_plane):.2f} us; the two trajectories differ by {gap:.1e}", flush=True)
    return dict(n_IP=plane.n_IP, in_contact=counts, stage_plane_us=med(a_plane), stage_plane_us_rounds=a_plane, stage_grid_us=med(a_grid),
                stage_grid_us_rounds=a_grid, substep_plane_us=med(t_plane), substep_plane_us_rounds=t_plane, substep_grid_us=med(t_grid),
                substep_grid_us_rounds=t_grid, increase_us=med(t_grid) - med(t_plane), max_dof_gap=gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--mesh_resolution", type=int, default=128)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sdf.py measures on a GPU; none is visible")
    v, t = chair_mesh(args.mesh_resolution)
    out = dict(build=time_build(np.asarray(v), np.asarray(t), args.res, args.rounds), stage=time_stage(args.reps, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
