"""Vectorized numpy restatement of the device marching cubes (pienerf_amd/csrc/pn_mesh.hip), bit for bit, and mesh checks for the tests.

Conventions ("Meshing"): a node is above when (double)f > threshold (NaN is not above); node (i,j,k) owns its lattice edges toward
+x, +y, +z; an edge's vertex is lo_a + t on its axis, t = (threshold - f0) / (f1 - f0) in fp64 from the lower endpoint, the node's indices on the
other two; a NaN coordinate is the canonical quiet NaN.  Vertices are ordered by node linear index, then axis; triangles by cell origin, then the
case table's order.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from gen_mc_table import CORNERS, EDGES, case_table  # noqa: E402

TRI_COUNT, TRI_EDGES = case_table()
CANONICAL_NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def _edge_owner():
    """Per Bourke edge: (owner offset (di, dj, dk) from the cell origin, axis)."""
    off, axis = np.zeros((12, 3), np.int64), np.zeros(12, np.int64)
    for e, (p, q) in enumerate(EDGES):
        a = int(np.nonzero(CORNERS[p] != CORNERS[q])[0][0])
        off[e] = CORNERS[p] if CORNERS[p][a] < CORNERS[q][a] else CORNERS[q]
        axis[e] = a
    return off, axis


EDGE_OFF, EDGE_AXIS = _edge_owner()


def _popcount3(m):
    m = m.astype(np.int64)
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1)


def marching_cubes(field, threshold, origin=(0, 0, 0)):
    """field [nx, ny, nz] fp32 -> (vertices fp64 [V,3], triangles int32 [T,3]).  `origin`: absolute index of field[0,0,0] (a crop of a larger
    lattice is meshed with the lattice's own indices)."""
    f = np.ascontiguousarray(field, np.float32)
    nx, ny, nz = f.shape
    assert min(nx, ny, nz) >= 2
    thr = float(threshold)
    f64 = f.astype(np.float64)
    up = f64 > thr
    mask = np.zeros(f.shape, np.uint8)
    mask[:-1, :, :] |= (up[:-1, :, :] != up[1:, :, :]).astype(np.uint8)
    mask[:, :-1, :] |= (up[:, :-1, :] != up[:, 1:, :]).astype(np.uint8) << 1
    mask[:, :, :-1] |= (up[:, :, :-1] != up[:, :, 1:]).astype(np.uint8) << 2
    nv = _popcount3(mask).reshape(-1)
    voff = np.cumsum(nv) - nv                                     # exclusive, over node linear index
    V = int(nv.sum())
    verts = np.empty((V, 3), np.float64)
    o = np.asarray(origin, np.int64)
    for a in range(3):
        sel = np.nonzero(((mask >> a) & 1).astype(bool))
        if len(sel[0]) == 0:
            continue
        hi = list(sel)
        hi[a] = hi[a] + 1
        f0, f1 = f64[sel], f64[tuple(hi)]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (thr - f0) / (f1 - f0)
        node = (sel[0].astype(np.int64) * ny + sel[1]) * nz + sel[2]
        vid = voff[node] + _popcount3(mask[sel] & ((1 << a) - 1))
        c = np.stack([(sel[b].astype(np.int64) + o[b]).astype(np.float64) for b in range(3)], 1)
        with np.errstate(invalid="ignore"):
            c[:, a] = c[:, a] + t
        c[np.isnan(c)] = CANONICAL_NAN
        verts[vid] = c
    # cells: case bit m set when corner m is not above
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for m, (di, dj, dk) in enumerate(CORNERS):
        case |= (~up[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]).astype(np.int64) << m
    cnt = TRI_COUNT[case].reshape(-1)
    cells = np.nonzero(cnt)[0]
    ci, cj, ck = np.unravel_index(cells, case.shape)
    cnode = (ci.astype(np.int64) * ny + cj) * nz + ck
    E = TRI_EDGES[case.reshape(-1)[cells]].astype(np.int64)      # [nC, 15], -1 padded, slots in table order
    valid = E >= 0
    e = E[valid]
    owner = np.repeat(cnode, valid.sum(1)) + (EDGE_OFF[e, 0] * ny + EDGE_OFF[e, 1]) * nz + EDGE_OFF[e, 2]
    ax = EDGE_AXIS[e]
    ids = voff[owner] + _popcount3(mask.reshape(-1)[owner] & ((1 << ax) - 1))
    tris = ids.astype(np.int32).reshape(-1, 3)
    assert tris.shape[0] == int(cnt.sum())
    return verts, tris


# ------------------------------------------------------------------ mesh checks
def directed_edges_paired(tris, V):
    """True when every directed edge appears once and its reverse once: closed and consistently oriented."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return True
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    fwd = np.sort(a * V + b)
    if np.any(fwd[1:] == fwd[:-1]):
        return False
    rev = np.sort(b * V + a)
    return bool(np.array_equal(fwd, rev))


def euler_characteristic(verts, tris):
    t = np.asarray(tris, np.int64)
    used = np.unique(t)
    return len(used) - (3 * len(t)) // 2 + len(t)


def signed_volume(verts, tris):
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
