"""Connected components of an occupancy lattice: the floater filter of the point sampler (sampling.py, `con`) and of the mesher
(nerf/utils.py extract_geometry, `components`).  The reference declares `--vres` and `--con` ("num of connected components to keep",
get_opts.py:71-72) and reads neither.

label_components runs on the GPU (csrc/pn_components.hip: three launches, no host synchronisation, capturable); there is no CPU
fallback.  select_components is plain torch on whatever device the labels live on.
"""
import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr


def label_components(occ, connectivity=26):
    """occ: bool or uint8 [nx, ny, nz] on the GPU (non-zero = occupied) -> int32 labels of the same shape: an occupied voxel's label is the
    smallest flat index (i*ny + j)*nz + k of its component, an empty voxel's -1.  connectivity 6 (faces) or 26 (faces, edges, corners)."""
    require_gpu(occ)
    if occ.dim() != 3 or occ.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"label_components: a [nx, ny, nz] bool or uint8 lattice, got {tuple(occ.shape)} {occ.dtype}")
    if int(connectivity) not in (6, 26):
        raise ValueError(f"label_components: connectivity is 6 or 26, got {connectivity}")
    occ = occ.contiguous()
    if occ.dtype == torch.bool:
        occ = occ.view(torch.uint8)  # a bool tensor stores one byte per element, 0 or 1
    nx, ny, nz = (int(s) for s in occ.shape)
    if min(nx, ny, nz) < 1 or nx * ny * nz >= 2 ** 31:
        raise RuntimeError(f"label_components: lattice {nx}x{ny}x{nz} is outside the limits (every side >= 1, nx ny nz < 2^31)")
    labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=occ.device)
    check(lib().pn_ccl_label(ptr(occ), nx, ny, nz, int(connectivity), ptr(labels), stream_ptr()), "ccl_label")
    return labels


def count_components(labels):
    """Number of components of a label lattice (a root carries its own flat index)."""
    flat = labels.reshape(-1)
    return int((flat == torch.arange(flat.numel(), dtype=flat.dtype, device=flat.device)).sum())


def select_components(labels, keep):
    """labels: label_components' output (any device) -> (mask, kept).  Components are ranked by voxel count, descending, ties to the smaller root
    label; mask (bool, labels' shape) marks the voxels of the first `keep` of them, kept is their [(root, size)] in rank order.  keep >= the number
    of components keeps everything; an empty lattice gives an empty selection."""
    keep = int(keep)
    if keep < 1:
        raise ValueError(f"select_components: keep must be at least 1, got {keep}")
    flat = labels.reshape(-1)
    roots, counts = torch.unique(flat[flat >= 0], return_counts=True)           # roots ascending
    order = torch.sort(counts, descending=True, stable=True).indices[:keep]     # stable: equal counts stay in ascending root order
    sel = roots[order]
    mask = torch.isin(labels, sel)
    return mask, list(zip(sel.tolist(), counts[order].tolist()))


def largest_components(occ, keep, connectivity=26):
    """-> (mask, kept) of the `keep` largest components of the occupancy lattice `occ` (label_components, then select_components)."""
    return select_components(label_components(occ, connectivity), keep)
