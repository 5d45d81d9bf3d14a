"""Marching cubes on the GPU and the density lattice it meshes (nerf/utils.py:174-205 of the reference: extract_fields + mcubes.marching_cubes).

    python -m pienerf_amd.mesh --out DIR [--ckpt PATH] [--resolution 256] [--threshold 10] [--fp16] [--con N]

writes DIR/mesh.ply (Trainer.save_mesh's file) and DIR/points.ply (save_point_cloud's) for a checkpoint; default: the synthetic chair whose density
field has the solid's shape (scene.make_checkpoint(shaped=True)).

The triangulation is the project's own case table (tools/gen_mc_table.py), not PyMCubes': the vertex SET is the same (one vertex per crossed lattice
edge), the triangles between those vertices may differ.  INTEGRATION.md, "Meshing", states the conventions.
"""
import argparse
import itertools
import os
import time

import numpy as np
import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr


def marching_cubes(field, threshold):
    """field [nx, ny, nz] fp32 on the device (every dimension >= 2) -> (vertices fp64 [V,3], triangles int32 [T,3]) on the device, in index space
    (vertex = (i, j, k) with the crossed edge's axis moved by t).  Reads the two counts back to the host once (not capturable)."""
    require_gpu(field)
    if field.dim() != 3 or field.dtype != torch.float32:
        raise RuntimeError(f"marching_cubes: a [nx, ny, nz] float32 field, got {tuple(field.shape)} {field.dtype}")
    field = field.contiguous()
    nx, ny, nz = (int(s) for s in field.shape)
    h = lib()
    nbytes = int(h.pn_mc_work_bytes(nx, ny, nz))
    if nbytes == 0:
        raise RuntimeError(f"marching_cubes: lattice {nx}x{ny}x{nz} is outside the limits (every side >= 2, 3 nx ny nz < 2^31, "
                           "5 (nx-1)(ny-1)(nz-1) < 2^31)")
    dev = field.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    thr = float(threshold)
    check(h.pn_mc_count(ptr(field), nx, ny, nz, thr, ptr(work), ptr(totals), stream_ptr()), "mc_count")
    V, T = (int(v) for v in totals.tolist())
    vertices = torch.empty(V, 3, dtype=torch.float64, device=dev)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
    if V > 0:  # a crossed edge always lies in a cell with triangles, so V = 0 <=> T = 0
        check(h.pn_mc_emit(ptr(field), nx, ny, nz, thr, ptr(work), ptr(vertices), ptr(triangles), stream_ptr()), "mc_emit")
    return vertices, triangles


def _host_floats(b):
    return [float(v) for v in (b.detach().cpu().tolist() if torch.is_tensor(b) else b)]


@torch.no_grad()
def lattice_field(bound_min, bound_max, resolution, query_func, S=128, device=None):
    """The density lattice of extract_fields (nerf/utils.py:174-189), left on the device.  Node (i, j, k) sits at (xs[i], ys[j], zs[k]), the
    per-axis coordinates being torch.linspace(bound_min[a], bound_max[a], resolution) computed on the CPU.  The lattice is queried in cubes of S
    nodes per side, in the order x block, y block, z block; a cube's points are listed with z fastest ('ij' meshgrid order), so query_func sees
    the same batches of the same fp32 points as the reference's loop.  Returns [res, res, res] fp32 on `device` (default: bound_min's when it
    is a GPU tensor, else the current GPU)."""
    res = int(resolution)
    if device is None:
        device = bound_min.device if torch.is_tensor(bound_min) and bound_min.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lo, hi = _host_floats(bound_min), _host_floats(bound_max)
    axes = [torch.linspace(lo[a], hi[a], res).to(device) for a in range(3)]
    field = torch.empty((res, res, res), dtype=torch.float32, device=device)
    for i0, j0, k0 in itertools.product(range(0, res, S), repeat=3):
        cube = (slice(i0, i0 + S), slice(j0, j0 + S), slice(k0, k0 + S))
        grid = torch.stack(torch.meshgrid(*(ax[c] for ax, c in zip(axes, cube)), indexing="ij"), dim=-1)   # [bx, by, bz, 3]
        field[cube] = query_func(grid.view(-1, 3)).reshape(grid.shape[:3])
    return field


def density_query(model, fp16=False):
    """Trainer.save_mesh's query: model.density(pts)['sigma'] under no_grad and autocast(enabled=fp16) (trainer.py's query_func)."""
    dev = model.aabb_infer.device

    def query(pts):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=bool(fp16)):
            return model.density(pts.to(dev))["sigma"]
    return query


def vertex_normals(vertices, triangles):
    """Area-weighted vertex normals [V,3] fp64 (a torch tensor on the vertices' device; numpy input: on the CPU): per vertex the sum of
    cross(b - a, c - a) over its incident faces (a, b, c), normalised.  With the project's case table that cross product points out of the
    above-threshold region, so nothing is flipped.  The sum is ordered (gmls.index_add_ordered): equal meshes give equal bits.  A vertex whose sum is
    zero or not finite (no face, or faces that cancel) gets (0, 0, 1)."""
    from .simulator.gmls import index_add_ordered
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(np.asarray(vertices, np.float64)))
    v = v.detach().to(torch.float64).reshape(-1, 3)
    t = triangles if torch.is_tensor(triangles) else torch.from_numpy(np.ascontiguousarray(np.asarray(triangles, np.int64)))
    t = t.detach().to(device=v.device, dtype=torch.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    fn = torch.linalg.cross(b - a, c - a)
    acc = torch.zeros_like(v)
    if t.shape[0]:
        index_add_ordered(acc, t.t().reshape(-1), fn.repeat(3, 1))    # every face once per corner: corner 0 of all faces, then 1, then 2
    ln = torch.sqrt((acc * acc).sum(-1, keepdim=True))
    ok = (ln > 0.0) & torch.isfinite(ln)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=v.device)
    return torch.where(ok, acc / torch.where(ok, ln, torch.ones_like(ln)), up)


@torch.no_grad()
def vertex_colors(model, vertices, normals, chunk=1 << 20):
    """uint8 RGB [V,3] (numpy): the model's colour at each vertex seen along -normal, i.e. by a viewer looking straight at the surface; the model's
    own fused forward (NeRFNetwork.forward) in chunks of `chunk` points, the colour clipped to [0, 1], times 255, truncated (io.save_image's rule)."""
    dev = model.aabb_infer.device
    x = torch.as_tensor(vertices).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
    d = -torch.as_tensor(normals).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
    out = torch.empty((x.shape[0], 3), dtype=torch.uint8, device=dev)
    for s in range(0, x.shape[0], chunk):
        _, rgb = model(x[s:s + chunk], d[s:s + chunk])
        out[s:s + chunk] = (rgb.to(torch.float32).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return out.cpu().numpy()


def parser():
    ap = argparse.ArgumentParser(description="Mesh and surface point cloud of a density field (Trainer.save_mesh / save_point_cloud)")
    ap.add_argument("--out", default="output_mesh", help="directory for mesh.ply and points.ply")
    ap.add_argument("--ckpt", default=None, help="a reference-format .pth or a checkpoints directory; default: the shaped synthetic chair")
    ap.add_argument("--trust-ckpt", dest="trust_ckpt", action="store_true", help="allow a pickled (non-weights-only) checkpoint")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--fp16", action="store_true", help="query the density under autocast (Trainer(fp16=True))")
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--bg_radius", type=float, default=-1, help="> 0: the checkpoint holds a background model (its tensors are loaded; meshing does not use them)")
    ap.add_argument("--con", dest="components", type=int, default=0, help="mesh only this many largest connected components of the above-threshold nodes; 0 (default) "
                    "meshes everything.  The reference declares --con with default 1 and never reads it, so off is the faithful default")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    from . import io, scene
    from .nerf.network import NeRFNetwork
    from .nerf.utils import extract_geometry, write_to_ply

    args = parser().parse_args(argv)
    model = NeRFNetwork(encoding="hashgrid", bound=args.bound, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=args.bg_radius)
    model = model.to(args.device)
    if args.ckpt:
        path = args.ckpt if os.path.isfile(args.ckpt) else io.latest_checkpoint(args.ckpt)
        if path is None:
            raise FileNotFoundError(f"no checkpoint under {args.ckpt}")
        io.load_checkpoint(model, path, model_only=True, allow_pickle=args.trust_ckpt)
    else:
        model.load_checkpoint_dict(scene.make_checkpoint(bound=args.bound, shaped=True))
    model.eval()
    os.makedirs(args.out, exist_ok=True)
    query = density_query(model, args.fp16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vertices, triangles = extract_geometry(model.aabb_infer[:3], model.aabb_infer[3:], args.resolution, args.threshold, query, components=args.components)
    t1 = time.perf_counter()
    scene.write_mesh_ply(os.path.join(args.out, "mesh.ply"), vertices, triangles)
    t2 = time.perf_counter()
    write_to_ply(vertices, os.path.join(args.out, "points.ply"))
    t3 = time.perf_counter()
    print(f"resolution {args.resolution}^3, threshold {args.threshold}: V {len(vertices)}, T {len(triangles)}; extract_geometry {t1 - t0:.3f} s, "
          f"mesh.ply {t2 - t1:.3f} s, points.ply {t3 - t2:.3f} s -> {args.out}")


if __name__ == "__main__":
    main()
