"""Arbitrary rest-space points bound to a ``Simulator`` and carried along by its GMLS field: ``Simulator.bind_points`` -> ``PointBinding.warp``.

The simulator's own forward map for the sampling cloud is ``update_pos`` (solver.py:604-617 of the reference: pos = sum N dof over the point's 8
kernels, what ``OutputToPly`` writes).  A binding evaluates the same field at points that are not the cloud's — the vertices of the marching-cubes
mesh — and pushes rest normals forward with the cofactor of the field's gradient.  Binding is initialisation-time torch; the per-frame warp is one
HIP launch (csrc/pn_warp_points.hip, include/pienerf_hip.h: pn_sim_warp_points).  INTEGRATION.md, "Deforming mesh".

Binding rule: a point uses the 8 kernels of its own kernel-grid cell floor((p - base) / kdx) when that cell lies inside the kres grid and all 8 are
active; otherwise the 8 kernels of the nearest integration point (distance to IP_pos, the lowest index on ties).  kernel_idx reads 0 for an inactive
corner, which is kernel 0 and not an error, so the second branch is a rule and not a fallback for rare cases: mesh vertices sit on the level set,
some of them in kernel cells that hold no integration point.
"""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from . import gmls

F64 = torch.float64
GROUP = 8              # points per table group = pn_sim_warp_points_group()
REPRODUCTION_TOL = 1e-9   # a validity gate (singular moment matrix), not an accuracy bar: good bindings reproduce their points to 1e-14
_CORNERS = [(S >> 2 & 1, S >> 1 & 1, S & 1) for S in range(8)]   # solver.py: precompute()'s corner order


def _as_points(x, device, dtype=F64):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    t = t.detach().to(device=device, dtype=dtype).reshape(-1, 3).contiguous()
    return t


def _to_groups(t, pairs):
    """[m,8,...] (2 pairs doubles per point and slot) -> [ceil(m / GROUP), pairs, GROUP, 8, 2], zero rows behind the last point: the launch's layout,
    lane = point * 8 + slot (include/pienerf_hip.h: pn_sim_warp_points)."""
    m = t.shape[0]
    gn = (m + GROUP - 1) // GROUP
    t = t.reshape(m, 8, pairs, 2)
    if gn * GROUP != m:
        t = torch.cat([t, torch.zeros((gn * GROUP - m, 8, pairs, 2), dtype=t.dtype, device=t.device)])
    return t.reshape(gn, GROUP, 8, pairs, 2).permute(0, 3, 1, 2, 4)


def nearest_ip(sim, pts, max_elems=1 << 24):
    """Index [n] (int64) of the integration point nearest to each of `pts` [n,3] fp64: squared distance (dx^2 + dy^2) + dz^2 to IP_pos in fp64, the
    lowest index on ties; in chunks of at most `max_elems` point-IP pairs."""
    n_IP = sim.IP_pos.shape[0]
    ip = sim.IP_pos.to(F64)
    ar = torch.arange(n_IP, device=pts.device)
    out = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    step = max(1, int(max_elems) // max(n_IP, 1))
    for s in range(0, pts.shape[0], step):
        d = pts[s:s + step, None, :] - ip[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = d2.min(dim=1, keepdim=True).values
        out[s:s + step] = torch.where(d2 == best, ar[None, :], n_IP).min(dim=1).values
    if pts.shape[0] and int(out.max()) >= n_IP:
        raise ValueError("bind_points: a point has no nearest integration point (non-finite coordinates)")
    return out


def point_topology(sim, pts):
    """The binding rule: (topo [V,8] int32, own [V] bool) for rest-space points `pts` [V,3] fp64 on the simulator's device; own = the point took its own
    cell's kernels, ~own = those of its nearest integration point."""
    kres = sim.kres
    cell = ((pts - sim.base) // sim.kdx).to(dtype=torch.int32).long()     # precompute()'s expression for pts2K
    in_grid = ((cell >= 0) & (cell <= kres - 2)).all(dim=1) & torch.isfinite(pts).all(dim=1)
    c = cell.clamp(0, kres - 2)
    idx = [(c[:, 0] + x, c[:, 1] + y, c[:, 2] + z) for x, y, z in _CORNERS]
    own = in_grid & torch.stack([sim.kernel_mask[i] for i in idx], dim=1).all(dim=1)
    topo = torch.stack([sim.kernel_idx[i] for i in idx], dim=1)
    far = torch.nonzero(~own).reshape(-1)
    if far.numel():
        topo[far] = sim.IP_kernel[nearest_ip(sim, pts[far])]
    return topo.to(torch.int32).contiguous(), own


def warp_torch(topo, Nx, dNx, normals0, dof):
    """The warp as fp64 torch ops on whatever device the tables are on, rounded to fp32 once: what PointBinding.warp computes on a CPU simulator and what
    the HIP launch is tested against.  topo [V,8], Nx [V,8,10], dNx [V,8,3,10] or None, normals0 [V,3] fp32 or None, dof [30 n_k] fp64.
    Returns pos [V,3] fp32, or (pos, normals) when dNx and normals0 are given."""
    d = dof.reshape(-1, 10, 3)[topo.long()]                                # [V,8,10,3]
    pos = torch.einsum("nic,nicr->nr", Nx, d).to(torch.float32)
    if dNx is None or normals0 is None:
        return pos
    F = torch.einsum("nijc,nicr->nrj", dNx, d)                             # F[r][j]
    f0, f1, f2 = F[:, :, 0], F[:, :, 1], F[:, :, 2]
    n = normals0.to(F64)
    c = n[:, 0:1] * torch.linalg.cross(f1, f2) + n[:, 1:2] * torch.linalg.cross(f2, f0) + n[:, 2:3] * torch.linalg.cross(f0, f1)   # cof(F) n
    ln = torch.sqrt((c * c).sum(-1, keepdim=True))
    ok = (ln > 0.0) & torch.isfinite(ln)
    out = torch.where(ok, (c / torch.where(ok, ln, torch.ones_like(ln))).to(torch.float32), normals0)
    return pos, out


class PointBinding:
    """V rest-space points with their neighbour kernels and Q-GMLS shape functions at their own positions.

    ``topo`` [V,8] int32, ``own`` [V] bool (the binding rule's branch per point, None for an explicit topology), ``n_fallback``, ``normals0`` [V,3]
    fp32 or None, ``n_k`` (the simulator's kernel count at bind time: warp() refuses a simulator that was re-initialised to another).
    On a GPU simulator only the launch's table layout is kept (include/pienerf_hip.h: pn_sim_warp_points); ``tables()`` rebuilds the plain one."""

    def __init__(self, sim, points, topo, normals=None, own=None, chunk=8192):
        dev = sim.device
        self.sim, self.device, self.n_k = sim, dev, int(sim.n_k)
        pts = _as_points(points, dev)
        V = pts.shape[0]
        topo = topo.to(device=dev, dtype=torch.int32).reshape(-1, 8).contiguous()
        if topo.shape[0] != V:
            raise ValueError(f"PointBinding: {V} points but {topo.shape[0]} topology rows")
        if V and (int(topo.min()) < 0 or int(topo.max()) >= self.n_k):
            raise ValueError(f"PointBinding: topology entries must lie in [0, {self.n_k})")
        self.V, self.points, self.topo, self.own = V, pts, topo, own
        self.n_fallback = int((~own).sum()) if own is not None else 0
        self.normals0 = None
        if normals is not None:
            self.normals0 = _as_points(normals, dev, torch.float32)
            if self.normals0.shape[0] != V:
                raise ValueError(f"PointBinding: {V} points but {self.normals0.shape[0]} normals")
        with_n = self.normals0 is not None
        kdx, rest = float(sim.kdx), sim.dof_rest.reshape(-1, 10, 3)
        cuda = dev.type == "cuda"
        G = (V + GROUP - 1) // GROUP
        if cuda:
            if int(lib().pn_sim_warp_points_group()) != GROUP:
                raise RuntimeError(f"libpienerf_hip.so groups {lib().pn_sim_warp_points_group()} points per wave, binding.py {GROUP}")
            self._topo_g = torch.zeros((G * GROUP, 8), dtype=torch.int32, device=dev)
            self._topo_g[:V] = topo
            self._Nx_g = torch.zeros((G, 5, GROUP, 8, 2), dtype=F64, device=dev)
            self._dNx_g = torch.zeros((G, 15, GROUP, 8, 2), dtype=F64, device=dev) if with_n else None
        else:
            self._Nx = torch.empty((V, 8, 10), dtype=F64, device=dev)
            self._dNx = torch.empty((V, 8, 3, 10), dtype=F64, device=dev) if with_n else None
        # shape functions in chunks of whole groups, checked and laid out chunk by chunk: nothing of size V x 8 x 3 x 10 exists twice
        chunk = max(GROUP, chunk // GROUP * GROUP)
        n_bad, worst = 0, 0.0
        for s in range(0, V, chunk):
            e = min(s + chunk, V)
            Nx, dNx, _ = gmls.init_GMLS(kdx, pts[s:e], topo[s:e], sim.kernel_pos, chunk=chunk, hessian=False, gradient=with_n, singular_ok=True)
            err = (torch.einsum("nic,nicr->nr", Nx, rest[topo[s:e].long()]) - pts[s:e]).abs().amax(dim=1)
            bad = ~(err <= REPRODUCTION_TOL)                    # NaN counts as bad
            if bool(bad.any()):
                n_bad += int(bad.sum())
                w = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))[bad].max()
                worst = max(worst, float(w))
            if cuda:
                g0, gn = s // GROUP, (e - s + GROUP - 1) // GROUP
                self._Nx_g[g0:g0 + gn] = _to_groups(Nx, 5)
                if with_n:
                    self._dNx_g[g0:g0 + gn] = _to_groups(dNx, 15)
            else:
                self._Nx[s:e] = Nx
                if with_n:
                    self._dNx[s:e] = dNx
        if n_bad:
            raise ValueError(f"bind_points: {n_bad} of {V} points are not reproduced by their binding at the rest state (worst error {worst:.3g}, "
                             f"allowed {REPRODUCTION_TOL:g}): their kernels do not determine the field there (singular moment matrix)")

    # ------------------------------------------------------------------ tables
    def tables(self):
        """(topo [V,8] int32, Nx [V,8,10], dNx [V,8,3,10] or None) fp64 in the plain layout, on the binding's device (rebuilt from the launch's layout on a GPU)."""
        if self.device.type != "cuda":
            return self.topo, self._Nx, self._dNx
        V = self.V

        def plain(t, pairs):
            return t.permute(0, 2, 3, 1, 4).reshape(-1, 8, pairs * 2)[:V]
        Nx = plain(self._Nx_g, 5).contiguous()
        dNx = plain(self._dNx_g, 15).reshape(V, 8, 3, 10).contiguous() if self._dNx_g is not None else None
        return self.topo, Nx, dNx

    def subset(self, sl):
        """The binding of points[sl] alone (a slice), with their tables copied: the same bits as rows `sl` of the whole binding's warp."""
        topo, Nx, dNx = self.tables()
        b = object.__new__(PointBinding)
        b.sim, b.device, b.n_k = self.sim, self.device, self.n_k
        b.points, b.topo = self.points[sl].contiguous(), topo[sl].contiguous()
        b.own = self.own[sl] if self.own is not None else None
        b.n_fallback = int((~b.own).sum()) if b.own is not None else 0
        b.normals0 = self.normals0[sl].contiguous() if self.normals0 is not None else None
        b.V = V = b.points.shape[0]
        Nx, dNx = Nx[sl], (dNx[sl] if dNx is not None else None)
        if self.device.type != "cuda":
            b._Nx, b._dNx = Nx.contiguous(), (dNx.contiguous() if dNx is not None else None)
            return b
        G = (V + GROUP - 1) // GROUP
        b._topo_g = torch.zeros((G * GROUP, 8), dtype=torch.int32, device=self.device)
        b._topo_g[:V] = b.topo
        b._Nx_g = _to_groups(Nx, 5).contiguous()
        b._dNx_g = _to_groups(dNx, 15).contiguous() if dNx is not None else None
        return b

    # ------------------------------------------------------------------ per frame
    def warp(self, dof=None, out=None):
        """Positions [V,3] fp32 of the bound points under `dof` (default: the simulator's current one; a [30 n_k] fp64 snapshot otherwise), and their
        normals [V,3] fp32 when the binding has rest normals: returns pos or (pos, normals).  `out`: the preallocated result (a tensor, or a pair with
        normals).  On a GPU: one launch on the current stream, no allocation when `out` is given, no host synchronisation, `dof` read at execution time —
        capturable, and a replay follows the simulator.  On a CPU simulator: the same formula as fp64 torch ops (warp_torch)."""
        sim = self.sim
        if int(sim.n_k) != self.n_k:
            raise RuntimeError(f"PointBinding: bound to a simulator with {self.n_k} kernels, which now has {sim.n_k}: bind the points again")
        dof = sim.dof if dof is None else dof
        if dof.dtype != F64 or dof.numel() != 30 * self.n_k or dof.device.type != self.device.type or not dof.is_contiguous():
            raise ValueError(f"PointBinding.warp: dof must be a contiguous fp64 tensor of {30 * self.n_k} entries on {self.device}")
        with_n = self.normals0 is not None
        V = self.V
        if out is None:
            pos = torch.empty((V, 3), dtype=torch.float32, device=self.device)
            nrm = torch.empty((V, 3), dtype=torch.float32, device=self.device) if with_n else None
        else:
            if with_n and not (isinstance(out, (tuple, list)) and len(out) == 2):
                raise ValueError("PointBinding.warp: a binding with normals takes out=(positions, normals)")
            pos, nrm = out if with_n else (out, None)
            for t in (pos, nrm) if with_n else (pos,):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (V, 3) or t.device.type != self.device.type or not t.is_contiguous():
                    raise ValueError(f"PointBinding.warp: out must be contiguous fp32 [{V}, 3] on {self.device}" + (" (a pair: positions, normals)" if with_n else ""))
        if self.device.type != "cuda":
            res = warp_torch(self.topo, self._Nx, self._dNx, self.normals0, dof)
            if with_n:
                pos.copy_(res[0])
                nrm.copy_(res[1])
            else:
                pos.copy_(res)
        elif V > 0:
            check(lib().pn_sim_warp_points(V, self.n_k, ptr(self._topo_g), ptr(self._Nx_g), ptr(self._dNx_g), ptr(dof), ptr(self.normals0), ptr(pos),
                                           ptr(nrm), stream_ptr()), "sim_warp_points")
        return (pos, nrm) if with_n else pos


def bind_points(sim, points, normals=None):
    """Simulator.bind_points: see there."""
    if sim.dof is None:
        raise RuntimeError("bind_points: the simulator has no rest state yet (InitializeFromArrays / precompute first)")
    pts = _as_points(points, sim.device)
    if pts.shape[0] == 0:
        return PointBinding(sim, pts, torch.zeros((0, 8), dtype=torch.int32, device=sim.device), normals, own=torch.zeros(0, dtype=torch.bool, device=sim.device))
    topo, own = point_topology(sim, pts)
    return PointBinding(sim, pts, topo, normals, own=own)
