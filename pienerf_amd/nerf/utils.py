"""``get_rays`` (inference and training forms), ``get_pnts_in_grids`` and the meshing functions ``extract_fields``, ``extract_geometry`` and ``write_to_ply`` with the reference's
signatures (nerf/utils.py:54-138, 355-386, 174-205, 341-351), backed by HIP kernels: the density lattice is evaluated and meshed on the device
(pienerf_amd.mesh, marching cubes in csrc/pn_mesh.hip).  The reference's PSNR and SSIM meters (:231-302) are in pienerf_amd/metrics.py; the rest
(the LPIPS meter, seeding) is off-path."""
import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream_ptr


def get_rays(poses, intrinsics, H, W, N=-1, error_map=None, patch_size=1, *, draws=None, image=None):
    """nerf/utils.py:54-138 for one pose: poses [1,4,4] cam2world, intrinsics (fx, fy, cx, cy).

    N = -1, the inference form: {'rays_o': [1,H*W,3], 'rays_d': [1,H*W,3]} fp32 on the pose's device (pn_get_rays).

    N > 0, the training forms, one launch of pn_train_batch: additionally 'inds' [1,N] int64, the sampled pixels (row * W + col), and 'inds_coarse'
    [1,N] with an error map.  N = min(N, H*W).  patch_size > 1 (:81-98): N / patch_size^2 patches with random top-left corners, the error map
    ignored.  error_map [1, 128*128] (:106-115): cells drawn without replacement by ``sample_cells``, each mapped to a pixel with a uniform jitter.
    Otherwise (:101) uniform pixels, duplicates allowed.  A pixel's direction is bit for bit the inference form's.

    The random numbers are drawn with torch on the pose's device, so torch.manual_seed reproduces a batch.  ``draws`` hands them in instead (the
    tests replay the reference's): {'inds': [N]} / {'cells': [N], 'u': [2,N]} / {'rows': [P], 'cols': [P]}.  ``image`` [H,W,C] fp32 on the device:
    the ground truth of the sampled pixels comes back as 'images' [1,N,C] from the same launch (nerf/provider.py:311-316)."""
    if poses.shape[0] != 1:
        raise RuntimeError("get_rays: one pose per call (the data set, the GUI and the render harness pass [1,4,4])")
    require_gpu(poses)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    H, W, dev = int(H), int(W), poses.device
    pose = poses[0].detach().to(torch.float32).contiguous()
    if N <= 0:
        rays_o = torch.empty(1, H * W, 3, dtype=torch.float32, device=dev)
        rays_d = torch.empty(1, H * W, 3, dtype=torch.float32, device=dev)
        check(lib().pn_get_rays(ptr(pose), fx, fy, cx, cy, H, W, ptr(rays_o), ptr(rays_d), stream_ptr()), "get_rays")
        return {"rays_o": rays_o, "rays_d": rays_d}
    N, patch_size, draws = min(int(N), H * W), int(patch_size), draws or {}

    def i64(t):
        return torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous().view(-1)

    results, a, b, u, mode = {}, None, None, None, 0
    if patch_size > 1:
        num_patch, mode = N // patch_size ** 2, 2
        if num_patch < 1 or num_patch * patch_size ** 2 != N or patch_size >= min(H, W):
            raise RuntimeError(f"get_rays: patch_size = {patch_size} needs N = {N} to be a multiple of its square and an image larger than a patch")
        a = i64(draws["rows"]) if "rows" in draws else torch.randint(0, H - patch_size, size=[num_patch], device=dev)
        b = i64(draws["cols"]) if "cols" in draws else torch.randint(0, W - patch_size, size=[num_patch], device=dev)
        if a.numel() != num_patch or b.numel() != num_patch:
            raise RuntimeError("get_rays: draws['rows'] / ['cols'] hold one corner per patch")
    elif error_map is None:
        a = i64(draws["inds"]) if "inds" in draws else torch.randint(0, H * W, size=[N], device=dev)
    else:
        mode = 1
        a = i64(draws["cells"]) if "cells" in draws else sample_cells(error_map.to(dev).view(-1), N)
        u = draws["u"].to(device=dev, dtype=torch.float32).contiguous() if "u" in draws else torch.rand(2, N, device=dev)
        if u.numel() != 2 * N:
            raise RuntimeError("get_rays: draws['u'] is [2, N]")
        results["inds_coarse"] = a.view(1, N)
    if mode != 2 and a.numel() != N:
        raise RuntimeError("get_rays: one draw per ray")
    pixels = None
    if image is not None:
        require_gpu(image)
        if image.dtype != torch.float32 or tuple(image.shape[:2]) != (H, W) or image.shape[-1] not in (3, 4) or not image.is_contiguous():
            raise RuntimeError("get_rays: image is a contiguous fp32 [H, W, 3 or 4] tensor")
        pixels = torch.empty(1, N, image.shape[-1], dtype=torch.float32, device=dev)
    inds = torch.empty(1, N, dtype=torch.int64, device=dev)
    rays_o = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
    check(lib().pn_train_batch(ptr(pose), fx, fy, cx, cy, H, W, N, mode, ptr(a), ptr(b), ptr(u), patch_size, ptr(image),
                               0 if image is None else image.shape[-1], ptr(inds), ptr(rays_o), ptr(rays_d), ptr(pixels), stream_ptr()), "get_rays")
    results.update(inds=inds, rays_o=rays_o, rays_d=rays_d)
    if pixels is not None:
        results["images"] = pixels
    return results


def sample_cells(weights, N, expo=None):
    """torch.multinomial(weights, N, replacement=False) for one row of the error map (nerf/utils.py:106), as pn_sample_cells: the N cells with the
    largest weights / expo, expo ~ Exp(1) drawn here with torch unless given, returned in ascending cell index as int64 [N].  Raises RuntimeError when
    fewer than N weights are positive (torch raises there too)."""
    require_gpu(weights, expo)
    w = weights.detach().to(torch.float32).contiguous().view(-1)
    e = torch.empty_like(w).exponential_() if expo is None else expo.to(torch.float32).contiguous().view(-1)
    if e.numel() != w.numel():
        raise RuntimeError("sample_cells: one exponential draw per cell")
    cells = torch.empty(int(N), dtype=torch.int64, device=w.device)
    status = torch.zeros(1, dtype=torch.int32, device=w.device)
    check(lib().pn_sample_cells(ptr(w), ptr(e), w.numel(), int(N), ptr(cells), ptr(status), stream_ptr()), "sample_cells")
    if int(status.item()) != 0:
        raise RuntimeError(f"sample_cells: {int(N)} cells asked for, fewer weights are positive (sampling without replacement)")
    return cells


def error_map_update(map_row, cells, err):
    """nerf/trainer.py:239-243 on one view's row of the error map, in place: map_row[cells] = 0.1 * map_row[cells] + 0.9 * err (pn_error_map_update).
    cells: distinct int64 indices [N]; err: the per-ray loss [N]."""
    require_gpu(map_row, cells, err)
    if map_row.dtype != torch.float32 or not map_row.is_contiguous() or map_row.numel() != 128 * 128:
        raise RuntimeError("error_map_update: map_row is a contiguous fp32 row of 128 * 128 cells")
    cells = cells.to(torch.int64).contiguous().view(-1)
    err = err.detach().to(torch.float32).contiguous().view(-1)
    if cells.numel() != err.numel():
        raise RuntimeError("error_map_update: one error per cell")
    check(lib().pn_error_map_update(ptr(map_row), ptr(cells), ptr(err), cells.numel(), stream_ptr()), "error_map_update")
    return map_row


def get_pnts_in_grids(n_vtx, n_grid, pnts, bbmin, bbmax, hgs, resolution):
    """nerf/utils.py:355-386: counting sort of the deformed IPs into `hgs` cells -> (pig_cnt, pig_bgn, pig_idx) int32.

    Slots inside a cell are in ascending point id (the reference's order is an atomic race)."""
    require_gpu(pnts, bbmin, resolution)
    n_vtx, n_grid = int(n_vtx), int(n_grid)
    pnts = pnts.to(torch.float32).contiguous()
    bbmin = bbmin.to(torch.float32).contiguous()
    resolution = resolution.to(torch.int32).contiguous()
    dev = pnts.device
    pig_idx = torch.zeros((n_vtx,), dtype=torch.int32, device=dev)
    pig_cnt = torch.zeros((n_grid,), dtype=torch.int32, device=dev)
    pig_bgn = torch.zeros((n_grid,), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().pn_pnts_in_grids(n_vtx, n_grid, ptr(pnts), ptr(bbmin), float(hgs), ptr(resolution), ptr(pig_cnt), ptr(pig_bgn), ptr(pig_idx),
                                 ptr(err), stream_ptr()), "get_pnts_in_grids")
    return pig_cnt, pig_bgn, pig_idx


def extract_fields(bound_min, bound_max, resolution, query_func, S=128):
    """nerf/utils.py:174-189: query_func on the resolution^3 lattice over [bound_min, bound_max] -> numpy float32 [res, res, res].  The lattice is
    built and queried on the device (pienerf_amd.mesh.lattice_field); only the result is copied back."""
    from ..mesh import lattice_field
    return lattice_field(bound_min, bound_max, resolution, query_func, S=S).cpu().numpy()


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, components=0):
    """nerf/utils.py:192-205: (vertices float64 [V,3] in world space, triangles int64 [T,3]) of the `threshold` level set of query_func.  Field and
    marching cubes stay on the device (pienerf_amd.mesh); the triangulation is the project's own ("Meshing").  World mapping with
    the reference's operations, order and types: index-space vertex / (resolution - 1), times the box's extent (bound_max - bound_min, taken in
    float32), plus bound_min; every step in float64.

    components > 0 (this project's option; 0 is the reference's behaviour): only the `components` largest 26-connected components of the nodes
    above the threshold are meshed (pienerf_amd.components).  The 8 corners of a cell are mutually 26-adjacent, so no cell holds a kept and a dropped
    node: the result is exactly the sub-mesh of the unfiltered surface that bounds the kept components, with bitwise-equal coordinates."""
    from ..mesh import lattice_field, marching_cubes
    field = lattice_field(bound_min, bound_max, resolution, query_func)
    if int(components) > 0:
        from ..components import largest_components
        above = field.to(torch.float64) > float(threshold)      # marching cubes' own predicate, (double)f > threshold: NaN is not above
        keep, _ = largest_components(above, int(components), connectivity=26)
        field = torch.where(above & ~keep, torch.full((), float("-inf"), dtype=field.dtype, device=field.device), field)   # -inf is never above
    idx, tri = marching_cubes(field, threshold)
    origin = _host_bound(bound_min)
    extent = _host_bound(bound_max) - origin              # float32 - float32, rounded once in float32
    scaled = idx.cpu().numpy() / (resolution - 1.0)
    world = scaled * extent.astype(np.float64) + origin.astype(np.float64)
    return world, tri.cpu().numpy().astype(np.int64)


def _host_bound(b):
    """A corner of the box as a float32 numpy [3] (the reference passes a float32 tensor)."""
    return (b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).astype(np.float32).reshape(3)


def write_to_ply(points, save_path):
    """nerf/utils.py:341-351: ASCII PLY of the points [N,3] as float64: a header of `ply`, `format ascii 1.0`, `element vertex N`, `property
    float` x / y / z and `end_header`, then one line per point, its coordinates as Python's str of the float, separated by single spaces."""
    rows = np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()
    head = ["ply", "format ascii 1.0", f"element vertex {len(rows)}"] + [f"property float {c}" for c in "xyz"] + ["end_header"]
    with open(save_path, "w") as f:
        f.writelines(line + "\n" for line in head)
        f.writelines("%s %s %s\n" % (x, y, z) for x, y, z in rows)
