"""PointBinding.warp on the device (csrc/pn_warp_points.hip: eight lanes per point, eight points per wave, four waves per workgroup) against the
fp64 torch restatement of the same tables on the CPU, and the deforming mesh it exists for (main_render --save_mesh).

Bars: positions 2.4e-7 and normals 1.2e-7 absolute — the device and the CPU sum the same fp64 products in different orders (~1e-14 apart) and both
round to fp32 once, so they differ by at most one fp32 ulp: 6e-8 for coordinates below 1 (1.2e-7 up to 2), 6e-8 for normal components."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from pienerf_amd import scene
from pienerf_amd.simulator import binding as B
from test_warp_points_host import read_mesh_ply, rigid_dof, _rotation

F64 = torch.float64
POS_TOL, NRM_TOL = 2.4e-7, 1.2e-7
# 1, 7, 8, 9: the partial group (= partial wave: a group of 8 points fills one wave); 31, 32, 33: the partial workgroup (4 waves); 63..65, 513: several
SIZES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 513]


def _make_sim(small_cloud, small_opt, deformed=True):
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cuda", persistent=False)
    s.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    if deformed:   # conftest.deformed_ip_state's state
        s.update_force(s.n_IP // 2, np.array([300.0, 100.0, -200.0]))
        for _ in range(12):
            s.stepforward()
    torch.cuda.synchronize()
    return s


@pytest.fixture(scope="module")
def sim(small_cloud, small_opt):
    """Deformed simulator shared by the tests that only read it."""
    return _make_sim(small_cloud, small_opt)


def _unit_normals(n, seed):
    """Random unit vectors in fp32 that normalise-and-round maps to themselves, so that 'unchanged' can be asserted bit for bit."""
    v = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3)))
    v = (v / v.norm(dim=1, keepdim=True)).to(torch.float32)
    for _ in range(8):
        w = v.to(F64)
        w = (w / w.norm(dim=1, keepdim=True)).to(torch.float32)
        if torch.equal(w, v):
            break
        v = w
    assert torch.equal(w, v)
    return v


@pytest.fixture(scope="module")
def pool(sim):
    """520 rest-space points [V,3] fp64 on the device, every fifth one on the nearest-IP branch: the cloud's points jittered by +-0.04, points below
    the kres grid under the lowest integration points, and points 0.12 outside the object's x and z faces."""
    rng = np.random.default_rng(3)
    cloud = sim.pos + torch.from_numpy(rng.uniform(-0.04, 0.04, tuple(sim.pos.shape))).to(sim.device)
    ip = sim.IP_pos.to(F64)
    below = ip[ip[:, 1] < ip[:, 1].min() + 1e-9].clone()
    below[:, 1] = float(sim.base[1]) - 0.005
    sides = []
    for axis, sign in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
        far = (sign * ip[:, axis]).max()
        side = ip[sign * ip[:, axis] > far - 1e-9].clone()
        side[:, axis] += sign * 0.12
        sides.append(side)
    cand = torch.cat([cloud, below] + sides)
    _, own = B.point_topology(sim, cand)
    a, f = cand[own], cand[~own]
    assert len(a) >= 416 and len(f) >= 104, (len(a), len(f))
    pts = torch.empty((520, 3), dtype=F64, device=sim.device)
    idx = torch.arange(520, device=sim.device)
    pts[idx % 5 != 4] = a[:416]
    pts[idx % 5 == 4] = f[:104]
    return pts


def _cpu_reference(b, dof):
    topo, Nx, dNx = b.tables()
    n0 = b.normals0.cpu() if b.normals0 is not None else None
    return B.warp_torch(topo.cpu(), Nx.cpu(), dNx.cpu() if dNx is not None else None, n0, dof.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_positions_match_the_cpu_einsum(sim, pool, V):
    b = sim.bind_points(pool[:V])
    assert b.n_fallback == V // 5
    pos = b.warp()
    assert pos.dtype == torch.float32 and tuple(pos.shape) == (V, 3) and pos.is_cuda
    want = _cpu_reference(b, sim.dof)
    err = float((pos.cpu().to(F64) - want.to(F64)).abs().max())
    moved = float((pos.cpu().to(F64) - pool[:V].cpu()).abs().max())
    print(f"V {V}: max |device - cpu| {err:.3g}, displacement {moved:.3g}")
    assert err <= POS_TOL
    assert V < 64 or moved > 1e-4      # a deformed state, not the rest state


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_normals_match_the_cpu_einsum(sim, pool, V):
    b = sim.bind_points(pool[:V], _unit_normals(V, V))
    pos, nrm = b.warp()
    wp, wn = _cpu_reference(b, sim.dof)
    ep = float((pos.cpu().to(F64) - wp.to(F64)).abs().max())
    en = float((nrm.cpu().to(F64) - wn.to(F64)).abs().max())
    print(f"V {V}: positions {ep:.3g}, normals {en:.3g}")
    assert ep <= POS_TOL and en <= NRM_TOL
    assert float((nrm.to(F64).norm(dim=1) - 1.0).abs().max()) <= 2e-7
    assert torch.equal(pos, sim.bind_points(pool[:V]).warp())        # the same positions with and without normals


@pytest.mark.gpu
def test_rigid_and_rest_dofs(sim, pool):
    n0 = _unit_normals(len(pool), 1)
    b = sim.bind_points(pool, n0)
    Rm, t = _rotation(11), torch.tensor([0.3, -0.2, 0.45], dtype=F64)
    pos, nrm = b.warp(rigid_dof(sim, Rm, t))
    want_p, want_n = pool.cpu() @ Rm.T + t, n0.to(F64) @ Rm.T
    want_n = want_n / want_n.norm(dim=1, keepdim=True)
    ep, en = float((pos.cpu().to(F64) - want_p).abs().max()), float((nrm.cpu().to(F64) - want_n).abs().max())
    print(f"rigid: positions {ep:.3g}, normals {en:.3g}")
    assert ep <= POS_TOL and en <= NRM_TOL
    pos, nrm = b.warp(sim.dof_rest)
    er = float((pos.cpu().to(F64) - pool.cpu()).abs().max())
    print(f"rest: positions {er:.3g}, normals changed {int((nrm.cpu() != n0).sum())}")
    assert er <= POS_TOL
    assert torch.equal(nrm.cpu(), n0)                                # bit for bit after the fp32 round


@pytest.mark.gpu
def test_degenerate_gradient_keeps_the_rest_normals(sim, pool):
    """F = 0 exactly: every dof zero (affine rows zero alone leave the gradient of the translation rows)."""
    n0 = _unit_normals(len(pool), 2)
    b = sim.bind_points(pool, n0)
    pos, nrm = b.warp(torch.zeros_like(sim.dof))
    assert torch.equal(nrm.cpu(), n0) and bool(torch.isfinite(pos).all())
    bad = sim.dof.clone()
    bad.view(-1, 10, 3)[:, 1:4, :] = float("inf")                    # a non-finite F: the rest normals again
    _, nrm = b.warp(bad)
    assert torch.equal(nrm.cpu(), n0)


@pytest.mark.gpu
def test_bits_are_reproducible_and_belong_to_the_point_alone(sim, pool):
    b = sim.bind_points(pool, _unit_normals(len(pool), 4))
    p1, n1 = b.warp()
    p2, n2 = b.warp()
    assert torch.equal(p1, p2) and torch.equal(n1, n2)
    for sl in (slice(100, 300), slice(3, 4), slice(505, 520)):       # other places in the group, the wave and the workgroup
        ps, ns = b.subset(sl).warp()
        assert torch.equal(ps, p1[sl]) and torch.equal(ns, n1[sl]), sl
    fresh = sim.bind_points(pool[100:300], b.normals0[100:300])      # bound on their own
    pf, nf = fresh.warp()
    assert float((pf - p1[100:300]).abs().max()) <= POS_TOL and float((nf - n1[100:300]).abs().max()) <= NRM_TOL


@pytest.mark.gpu
def test_snapshot_and_preallocated_outputs(small_cloud, small_opt, pool):
    s = _make_sim(small_cloud, small_opt)
    b = s.bind_points(pool, _unit_normals(len(pool), 5))
    snap = s.dof.clone()
    old_p, old_n = (t.clone() for t in b.warp())
    for _ in range(3):
        s.stepforward()
    new_p, _ = b.warp()
    assert not torch.equal(new_p, old_p)
    out = (torch.full_like(old_p, -7.0), torch.full_like(old_n, -7.0))
    res = b.warp(dof=snap, out=out)
    assert res[0] is out[0] and res[1] is out[1]
    assert torch.equal(out[0], old_p) and torch.equal(out[1], old_n)
    with pytest.raises(ValueError):
        b.warp(out=out[0])
    with pytest.raises(ValueError):
        b.warp(out=(out[0][:-1], out[1]))
    with pytest.raises(ValueError):
        b.warp(dof=snap.to(torch.float32))


@pytest.mark.gpu
def test_captured_warp_follows_the_simulator(small_cloud, small_opt, pool):
    from pienerf_amd.harness import _capture
    s = _make_sim(small_cloud, small_opt)
    b = s.bind_points(pool, _unit_normals(len(pool), 6))
    out = (torch.empty((b.V, 3), dtype=torch.float32, device="cuda"), torch.empty((b.V, 3), dtype=torch.float32, device="cuda"))
    b.warp(out=out)                                                   # warm-up outside the capture
    torch.cuda.synchronize()
    before = out[0].clone()
    g = torch.cuda.CUDAGraph()
    with _capture(g):                                                 # one stream, one kernel node
        b.warp(out=out)
    for _ in range(3):
        s.stepforward()
    g.replay()
    torch.cuda.synchronize()
    want_p, want_n = b.warp()
    assert torch.equal(out[0], want_p) and torch.equal(out[1], want_n)
    assert not torch.equal(out[0], before)


@pytest.fixture(scope="module")
def shaped_model():
    from pienerf_amd.nerf.network import NeRFNetwork
    m = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).to("cuda")
    m.load_checkpoint_dict(scene.make_checkpoint(bound=1.0, shaped=True))
    return m.eval()


def _rest_mesh(model, resolution=48, threshold=10.0):
    from pienerf_amd.mesh import density_query
    from pienerf_amd.nerf.utils import extract_geometry
    return extract_geometry(model.aabb_infer[:3], model.aabb_infer[3:], resolution, threshold, density_query(model))


@pytest.mark.gpu
@pytest.mark.parametrize("resolution", [48, 12])
def test_mesh_of_the_shaped_chair_moves_with_the_simulator(sim, shaped_model, resolution):
    """Resolution 48: every vertex lies in a kernel cell whose 8 kernels are active (the chair's faces are nowhere within a lattice spacing of a
    kernel cell without integration points), so the nearest-IP branch is not taken there.  It is at resolution 12: marching cubes puts a vertex up
    to a lattice spacing (0.18) outside the solid, into kernel cells with inactive corners."""
    from pienerf_amd.mesh import vertex_colors, vertex_normals
    v, t = _rest_mesh(shaped_model, resolution)
    assert len(v) > (1000 if resolution == 48 else 50) and len(t) > 0
    n = vertex_normals(v, t)
    b = sim.bind_points(v, n)                                         # no exception: every vertex is reproduced at rest
    print(f"mesh {resolution}: {b.V} vertices, {len(t)} triangles, {b.n_fallback} through the nearest IP")
    if resolution == 12:
        assert b.n_fallback >= 1
    pos, nrm = b.warp()
    assert bool(torch.isfinite(pos).all()) and bool(torch.isfinite(nrm).all())
    disp = float((pos.cpu().to(F64) - torch.from_numpy(v)).norm(dim=1).max())
    print(f"max displacement {disp:.4g}")
    assert 1e-4 < disp < 0.5
    col = vertex_colors(shaped_model, v, n)
    assert col.dtype == np.uint8 and col.shape == v.shape and col.min() < col.max()


@pytest.mark.gpu
def test_main_render_writes_the_mesh_sequence(tmp_path, shaped_model):
    from pienerf_amd import io, main_render
    flags = ["--frames", "3", "--W", "48", "--H", "48", "--sim_dx", "0.1", "--force", "300", "100", "-200", "--quiet"]
    mesh_flags = ["--save_mesh", "--mesh_resolution", "48", "--mesh_normals", "--mesh_color"]
    a = tmp_path / "a"
    main_render.run(main_render.parser().parse_args(flags + mesh_flags + ["--out", str(a)]))
    hdr0, c0, f0 = read_mesh_ply(str(a / "mesh_0.ply"))
    _, c1, f1 = read_mesh_ply(str(a / "mesh_1.ply"))
    _, c2, f2 = read_mesh_ply(str(a / "mesh_2.ply"))
    assert not (a / "mesh_3.ply").exists()
    assert "property float nx" in hdr0 and "property uchar blue" in hdr0
    assert len(f0) > 1000 and np.array_equal(f0, f1) and np.array_equal(f0, f2)
    xyz = lambda c: np.stack([c["x"], c["y"], c["z"]], 1)
    v, t = _rest_mesh(shaped_model)
    assert np.array_equal(f0, t) and xyz(c0).shape == v.shape
    assert np.abs(xyz(c0).astype(np.float64) - v).max() <= POS_TOL          # frame 0 is the rest state: the rest mesh to fp32
    moved = np.abs(xyz(c2) - xyz(c0)).max()
    print(f"mesh_2 against mesh_0: {moved:.4g}")
    assert moved > 0 and np.isfinite(xyz(c2)).all()
    nn = np.linalg.norm(np.stack([c2["nx"], c2["ny"], c2["nz"]], 1).astype(np.float64), axis=1)
    assert np.abs(nn - 1.0).max() <= 2e-7
    for k in ("red", "green", "blue"):                                       # colours are computed once at rest
        assert np.array_equal(c0[k], c2[k])
    # the same run without --save_mesh (the shaped checkpoint handed over as a file): byte-equal PNGs — the run rendered the shaped checkpoint, and
    # writing meshes disturbed nothing
    io.save_checkpoint(shaped_model, str(tmp_path / "ws" / "checkpoints" / "ngp_ep0001.pth"), epoch=1)
    bdir = tmp_path / "b"
    main_render.run(main_render.parser().parse_args(flags + ["--ckpt", str(tmp_path / "ws" / "checkpoints"), "--out", str(bdir)]))
    for f in range(3):
        assert open(a / f"img_{f}.png", "rb").read() == open(bdir / f"img_{f}.png", "rb").read(), f
    assert not list(bdir.glob("mesh_*.ply"))


def test_header_and_ctypes_signature_agree():
    from pienerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pn_sim_warp_points\s*\(([^)]*)\)\s*;", text)
    assert m, "pn_sim_warp_points is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    want = [_lib.P if "*" in p else {"int": _lib.i32, "double": _lib.f64}[p.split()[0]] for p in params]
    res, args = _lib.SIGNATURES["pn_sim_warp_points"]
    assert res is _lib.i32 and args == want and len(args) == 10
    assert re.search(r"\bint\s+pn_sim_warp_points_group\s*\(\s*void\s*\)\s*;", text) and _lib.SIGNATURES["pn_sim_warp_points_group"] == (_lib.i32, [])
    # argument checks happen before anything is enqueued (no GPU needed)
    import ctypes
    h, d = _lib.lib(), ctypes.c_void_p(256)
    assert h.pn_sim_warp_points_group() == B.GROUP
    assert h.pn_sim_warp_points(0, 4, d, d, d, d, d, d, d, None) == 1                  # no points
    assert h.pn_sim_warp_points(8, 0, d, d, d, d, d, d, d, None) == 1                  # no kernels
    assert h.pn_sim_warp_points(8, 4, None, d, d, d, d, d, d, None) == 1
    assert h.pn_sim_warp_points(8, 4, d, d, None, d, d, d, d, None) == 1               # normals asked for without gradients
    assert h.pn_sim_warp_points(8, 4, d, d, d, d, None, d, d, None) == 1               # ... or without rest normals
    assert h.pn_sim_warp_points(8, 4, d, ctypes.c_void_p(264), d, d, d, d, d, None) == 1   # a table that is not 16-byte aligned
