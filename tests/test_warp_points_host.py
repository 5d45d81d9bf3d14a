"""Binding arbitrary points to the simulator and warping them, on the CPU (no kernel is launched): the binding rule's two branches, the validity
gate, the warp's index conventions under a rigid motion, vertex normals of a marching-cubes sphere, and the mesh PLY writer's optional fields
(pienerf_amd/simulator/binding.py, pienerf_amd/mesh.py, pienerf_amd/scene.py; INTEGRATION.md "Deforming mesh")."""
import numpy as np
import pytest
import torch

import mc_reference as R
from pienerf_amd import scene
from pienerf_amd.simulator import binding as B
from pienerf_amd.simulator.solver import Simulator

F64 = torch.float64


@pytest.fixture(scope="module")
def sim(small_cloud, small_opt):
    """A CPU simulator on the small scene, at rest: the fields InitializeFromArrays sets, then precompute() (nothing here needs the HIP library)."""
    o, c = small_opt, small_cloud
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
    s.pos = torch.from_numpy(np.asarray(c["pos"], np.float64))
    s.mass = torch.from_numpy(np.asarray(c["mass"], np.float64))
    s.mu = torch.from_numpy(np.asarray(c["mu"], np.float64))
    s.lam = torch.from_numpy(np.asarray(c["lam"], np.float64))
    s.is_pin = torch.from_numpy(np.asarray(c["pin"]).astype(bool))
    s.precompute()
    return s


def _reproduction(b):
    topo, Nx, _ = b.tables()
    rest = b.sim.dof_rest.reshape(-1, 10, 3)[topo.long()]
    return float((torch.einsum("nic,nicr->nr", Nx, rest) - b.points).abs().max())


def _brute_nearest(sim, p):
    d = p[:, None, :] - sim.IP_pos[None].to(F64)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return torch.from_numpy(np.argmin(d2.numpy(), axis=1))   # numpy: the first minimum


def _fallback_points(sim):
    """Points the rule must send to the nearest-IP branch: centres-ish of kernel cells that have an inactive corner but lie beside the object, and
    points below the kres grid (under the chair's legs, 0.005 outside)."""
    kres, kdx = sim.kres, float(sim.kdx)
    pts = []
    cells = torch.stack(torch.meshgrid(*[torch.arange(kres - 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    act = torch.stack([sim.kernel_mask[cells[:, 0] + x, cells[:, 1] + y, cells[:, 2] + z] for x, y, z in B._CORNERS], 1)
    partial = cells[act.any(1) & ~act.all(1)]
    assert len(partial) > 0
    ip = sim.IP_pos.to(F64)
    for c in partial:   # the integration point nearest to the cell, moved 0.01 into the cell along each axis where it lies outside; cells further
        # than 0.6 kdx from every integration point are left out
        lo = sim.base + c.to(F64) * kdx
        j = int(((ip - (lo + 0.5 * kdx)) ** 2).sum(1).argmin())
        p = torch.minimum(torch.maximum(ip[j], lo + 0.01), lo + kdx - 0.01)
        if float((p - ip[j]).norm()) < 0.6 * kdx:
            pts.append(p)
    low = ip[ip[:, 1] < ip[:, 1].min() + 1e-9][:5].clone()
    low[:, 1] = float(sim.base[1]) - 0.005
    return torch.stack(pts), low


def test_own_cell_branch_takes_the_cells_kernels(sim):
    b = sim.bind_points(sim.pos)
    assert b.V == sim.pos.shape[0] and b.topo.dtype == torch.int32 and tuple(b.topo.shape) == (b.V, 8)
    own = b.own
    assert int(own.sum()) > 0.5 * b.V
    assert torch.equal(b.topo[own], sim.pts_kernel[own])
    # every kernel of an own-cell row is active, and the row is the cell's 8 corners
    cell = ((sim.pos - sim.base) // sim.kdx).long()[own]
    for s, (x, y, z) in enumerate(B._CORNERS):
        assert bool(sim.kernel_mask[cell[:, 0] + x, cell[:, 1] + y, cell[:, 2] + z].all())
    # cloud points whose kernel cell has an inactive corner (pts_kernel holds kernel 0 there) go through their nearest integration point
    if int((~own).sum()):
        assert torch.equal(b.topo[~own].long(), sim.IP_kernel[_brute_nearest(sim, sim.pos[~own])].long())
    assert b.n_fallback == int((~own).sum())
    assert _reproduction(b) <= 1e-9
    print(f"cloud: {b.V} points, {b.n_fallback} through the nearest IP, reproduction {_reproduction(b):.3g}")


def test_fallback_branch_takes_the_nearest_integration_points_kernels(sim):
    partial, below = _fallback_points(sim)
    cell = ((below - sim.base) // sim.kdx).long()
    assert bool((cell[:, 1] < 0).all())                           # outside the kres grid
    pts = torch.cat([partial, below])
    b = sim.bind_points(pts)
    assert not bool(b.own.any()) and b.n_fallback == len(pts)
    j = _brute_nearest(sim, pts)
    assert torch.equal(b.topo.long(), sim.IP_kernel[j].long())
    assert torch.equal(B.nearest_ip(sim, pts, max_elems=7 * sim.n_IP), j)    # chunked: 7 points at a time
    err = _reproduction(b)
    print(f"{len(partial)} points in cells with an inactive corner, {len(below)} below the grid: reproduction {err:.3g}")
    assert err <= 1e-9


def test_a_tie_between_two_integration_points_takes_the_lower_index(sim):
    """Below the grid, under the midpoint of two x-neighbours of the lowest layer of integration points: both are nearest, at bit-equal distances."""
    ip = sim.IP_pos.to(F64)
    grid = sim.IP_grid.long()
    key = {tuple(g): i for i, g in enumerate(grid.tolist())}
    ymin = int(grid[:, 1].min())
    found = differ = 0
    for i, g in enumerate(grid.tolist()):
        k = key.get((g[0] + 1, g[1], g[2]))
        if g[1] != ymin or k is None:
            continue
        p = ip[i].clone()
        p[0] = (ip[i, 0] + ip[k, 0]) / 2
        p[1] = float(sim.base[1]) - 0.005
        if float(p[0] - ip[i, 0]) != float(ip[k, 0] - p[0]) or not torch.equal(ip[i, 1:], ip[k, 1:]):   # the midpoint must be exact for a tie
            continue
        d = p[None] - ip
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        lo, hi = min(i, k), max(i, k)
        assert float(d2[lo]) == float(d2[hi]) == float(d2.min())
        found += 1
        assert int(B.nearest_ip(sim, p[None])[0]) == lo
        topo, own = B.point_topology(sim, p[None])
        assert not bool(own[0]) and torch.equal(topo[0].long(), sim.IP_kernel[lo].long())
        differ += int(not torch.equal(sim.IP_kernel[lo], sim.IP_kernel[hi]))
    print(f"{found} ties, {differ} between integration points with different kernels")
    assert found > 0


def test_wrong_topology_is_refused(sim):
    ip = sim.IP_pos.to(F64)
    top, bottom = int(ip[:, 1].argmax()), int(ip[:, 1].argmin())
    q = sim.kernel_pos[sim.IP_kernel[bottom].long()]
    assert float(((q - ip[top]) ** 2).sum(1).sqrt().min()) > float(sim.kdx)      # every weight vanishes
    good = sim.bind_points(ip[[top, bottom]])
    assert good.V == 2
    with pytest.raises(ValueError, match=r"1 of 2 points"):
        B.PointBinding(sim, ip[[top, bottom]], torch.stack([sim.IP_kernel[bottom], sim.IP_kernel[bottom]]))
    with pytest.raises(ValueError, match="topology entries"):
        B.PointBinding(sim, ip[[top]], torch.full((1, 8), sim.n_k, dtype=torch.int32))


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return torch.from_numpy(q)


def rigid_dof(sim, Rm, t):
    dof = torch.zeros((sim.n_k, 10, 3), dtype=F64, device=sim.kernel_pos.device)
    Rm, t = Rm.to(dof.device), t.to(dof.device)
    dof[:, 0, :] = sim.kernel_pos @ Rm.T + t
    for j in range(3):
        dof[:, 1 + j, :] = Rm[:, j]
    return dof.reshape(-1).contiguous()


def test_rigid_motion_moves_points_and_normals_rigidly(sim):
    rng = np.random.default_rng(5)
    partial, below = _fallback_points(sim)
    pts = torch.cat([sim.pos[::7] + torch.from_numpy(rng.uniform(-0.02, 0.02, (len(sim.pos[::7]), 3))), partial, below])
    n = torch.from_numpy(rng.standard_normal((len(pts), 3)))
    n = (n / n.norm(dim=1, keepdim=True)).to(torch.float32)
    b = sim.bind_points(pts, n)
    Rm, t = _rotation(11), torch.tensor([0.3, -0.2, 0.45], dtype=F64)
    dof = rigid_dof(sim, Rm, t)
    topo, Nx, dNx = b.tables()
    d = dof.reshape(-1, 10, 3)[topo.long()]
    p64 = torch.einsum("nic,nicr->nr", Nx, d)
    F = torch.einsum("nijc,nicr->nrj", dNx, d)
    want_p, want_n = pts @ Rm.T + t, n.to(F64) @ Rm.T
    print(f"fp64: pos {float((p64 - want_p).abs().max()):.3g}, F {float((F - Rm).abs().max()):.3g}")
    assert float((p64 - want_p).abs().max()) <= 1e-13 and float((F - Rm).abs().max()) <= 1e-12
    pos, nrm = b.warp(dof)
    assert pos.dtype == torch.float32 and nrm.dtype == torch.float32
    assert float((pos.to(F64) - want_p).abs().max()) <= 2.4e-7
    assert float((nrm.to(F64) - want_n / want_n.norm(dim=1, keepdim=True)).abs().max()) <= 2.4e-7
    # rest state: the points themselves; a binding without normals returns positions only, into `out` when given
    out = torch.empty((b.V, 3), dtype=torch.float32)
    b2 = sim.bind_points(pts)
    assert b2.warp(out=out) is out and float((out.to(F64) - pts).abs().max()) <= 2.4e-7
    # a collapsed field keeps the rest normals
    pos0, nrm0 = b.warp(torch.zeros_like(dof))
    assert torch.equal(nrm0, n) and bool(torch.isfinite(pos0).all())
    with pytest.raises(ValueError):
        b.warp(dof[:-3])


def test_binding_refuses_a_reinitialised_simulator(sim):
    b = sim.bind_points(sim.pos[:4])
    keep = sim.n_k
    try:
        sim.n_k = keep + 1
        with pytest.raises(RuntimeError, match="bind the points again"):
            b.warp()
    finally:
        sim.n_k = keep


def test_init_gmls_keywords_leave_the_returned_tables_bit_identical(sim):
    from pienerf_amd.simulator import gmls
    kdx = float(sim.kdx)
    sl = slice(0, 300)
    full = gmls.init_GMLS(kdx, sim.pos[sl], sim.pts_kernel[sl], sim.kernel_pos)
    assert torch.equal(full[0], sim.pts_Nx[sl]) and torch.equal(full[2], sim.pts_ddNx[sl])
    nh = gmls.init_GMLS(kdx, sim.pos[sl], sim.pts_kernel[sl], sim.kernel_pos, hessian=False)
    assert nh[2] is None and torch.equal(nh[0], full[0]) and torch.equal(nh[1], full[1])
    ng = gmls.init_GMLS(kdx, sim.pos[sl], sim.pts_kernel[sl], sim.kernel_pos, gradient=False)
    assert ng[1] is None and ng[2] is None and torch.equal(ng[0], full[0])


# ------------------------------------------------------------------ mesh helpers
def _sphere_mesh(n=24, r=0.6):
    ax = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    v, t = R.marching_cubes((r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), 0.0)
    return v / (n - 1.0) * 2.0 - 1.0, t


def test_vertex_normals_of_a_sphere_point_outward():
    from pienerf_amd.mesh import vertex_normals
    v, t = _sphere_mesh()
    assert R.signed_volume(v, t) > 0
    n = vertex_normals(v, t)
    assert n.dtype == F64 and tuple(n.shape) == v.shape
    n = n.numpy()
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12
    radial = (n * v / np.linalg.norm(v, axis=1, keepdims=True)).sum(1)
    print(f"sphere: {len(v)} vertices, min n.r {radial.min():.4f}")
    assert radial.min() >= 0.99
    assert np.array_equal(vertex_normals(v, t).numpy(), n)                       # ordered sum: the same bits again
    # a vertex without faces, and one whose faces cancel, get (0, 0, 1)
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float64)
    n2 = vertex_normals(v2, np.array([[0, 1, 2], [0, 2, 1]])).numpy()
    assert np.array_equal(n2, np.tile([0.0, 0.0, 1.0], (4, 1)))
    assert np.array_equal(vertex_normals(v2, np.array([[0, 1, 2]])).numpy()[:3], np.tile([0.0, 0.0, 1.0], (3, 1)))


def _old_write_mesh_ply_bytes(vertices, triangles):
    """The writer as it was before the optional fields."""
    v = np.ascontiguousarray(np.asarray(vertices), dtype="<f4").reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    face = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = t
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
           f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(hdr) + "\n").encode() + v.tobytes() + face.tobytes()


def read_mesh_ply(path):
    """(header lines, vertex columns, faces [T,3]) of a write_mesh_ply file."""
    cols = scene.read_ply(path)
    with open(path, "rb") as f:
        hdr = []
        while True:
            line = f.readline().decode().strip()
            hdr.append(line)
            if line == "end_header":
                break
        nv = int(next(h for h in hdr if h.startswith("element vertex")).split()[2])
        nf = int(next(h for h in hdr if h.startswith("element face")).split()[2])
        f.read(nv * sum(v.dtype.itemsize for v in cols.values()))
        rec = np.frombuffer(f.read(), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert len(rec) == nf and np.all(rec["n"] == 3)
    return hdr, cols, rec["i"]


@pytest.mark.parametrize("n", [0, 1, 37])
def test_write_mesh_ply_optional_fields(tmp_path, n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal((n + 2 if n else 0, 3))
    t = rng.integers(0, max(len(v), 1), (n, 3)).astype(np.int64)
    p = str(tmp_path / "m.ply")
    scene.write_mesh_ply(p, v, t)
    assert open(p, "rb").read() == _old_write_mesh_ply_bytes(v, t)
    scene.write_mesh_ply(p, v, t, normals=None, colors=None)
    assert open(p, "rb").read() == _old_write_mesh_ply_bytes(v, t)
    nrm = rng.standard_normal(v.shape).astype(np.float32)
    col = rng.integers(0, 256, v.shape).astype(np.uint8)
    scene.write_mesh_ply(p, v, t, normals=nrm, colors=col)
    hdr, cols, faces = read_mesh_ply(p)
    assert hdr == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
                   "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
                   "property uchar blue", f"element face {n}", "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(np.stack([cols["x"], cols["y"], cols["z"]], 1), v.astype(np.float32).reshape(-1, 3))
    assert np.array_equal(np.stack([cols["nx"], cols["ny"], cols["nz"]], 1), nrm.reshape(-1, 3))
    assert np.array_equal(np.stack([cols["red"], cols["green"], cols["blue"]], 1), col.reshape(-1, 3)) and cols["red"].dtype == np.uint8
    assert np.array_equal(faces, t)
    scene.write_mesh_ply(p, v, t, colors=col)                                   # colours alone
    hdr, cols, faces = read_mesh_ply(p)
    assert "nx" not in cols and np.array_equal(cols["blue"], col.reshape(-1, 3)[:, 2]) and np.array_equal(faces, t)
    if n:
        with pytest.raises(ValueError):
            scene.write_mesh_ply(p, v, t, normals=nrm[:-1])
        with pytest.raises(ValueError):
            scene.write_mesh_ply(p, v, t, colors=col.astype(np.int32))
