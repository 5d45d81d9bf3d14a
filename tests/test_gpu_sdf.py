"""Mesh colliders on the GPU (csrc/pn_sdf.hip; pienerf_amd/sdf.py: SdfGrid.from_mesh; Simulator.add_mesh_collider ...): the built
grid against the fp64 restatement of its law (tests/sdf_reference.py) — every node's sign, the distance by a measured bar —, the grids' contact term
against numpy at contact's own bar, a floor as a grid against the analytic plane, trajectories against the CPU oracle with the numpy term as its
`extra`, and the captured step."""
import warnings

import numpy as np
import pytest
import torch

import sdf_reference as R
from conftest import make_oracle_sim, rel_err
from contact_reference import OracleContact, contact_term, ip_state, plane, sphere
from pienerf_amd.harness import SimRenderHarness
from pienerf_amd.sdf import SdfGrid, clean_triangles, mesh_box, mesh_icosphere
from test_gpu_contact import FORCE, _bits, _disp, _sim
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

LO, S, RES = (-0.8, -0.8, -0.8), 0.107, (16, 16, 16)
# |GPU - fp64 restatement| of the distance on the two meshes of test_build_matches_the_reference, measured on an MI355X: 4.07e-8 (box, either orientation),
# 5.70e-8 / 5.94e-8 (icosphere / flipped) — fp32 rounding of the corner differences and of the closest point, in another order than numpy's; the bar is
# 8 x the largest, and stays below 1e-3 s
DIST_BAR = 8 * 5.94e-8
assert DIST_BAR <= 1e-3 * S

N_TRAJ = 24
SHELL = dict(centre=(0.0, 0.0, 0.0), radius=0.98, inside=True)
BALL_OFFSET, BALL_VEL = (0.0, 0.0, 0.9), (0.3, 0.0, -0.2)


def _build(v, t, lo=LO, s=S, res=RES):
    g = SdfGrid.from_mesh(v, t, lo=lo, spacing=s, res=res, device=DEV)
    tri9, dropped = clean_triangles(v, t)
    assert g.dropped == dropped and g.triangles == len(tri9) and g.shape == res[::-1] and g.values.dtype == torch.float32
    return g, R.build(tri9, lo, s, res)


def _compare(name, g, ref, bar=DIST_BAR):
    phi, w, dist = ref
    got = g.values.cpu().numpy().astype(np.float64)
    near = float(np.abs(phi).min())
    gap = float(np.abs(np.abs(got) - dist).max())
    wrong = int(((got < 0) != (phi < 0)).sum())
    print(f"{name}: {g.triangles} triangles, {got.size} nodes, {int((phi < 0).sum())} inside; nearest node to the surface {near:.2e}; "
          f"max |distance - fp64| {gap:.2e} (bar {bar:.2e}); signs that differ {wrong}; closedness {g.closedness:.1e}")
    assert near > 1e-4, name                 # no node lies near the surface: every sign is decided far from |w| = 0.5
    assert wrong == 0, (name, wrong)         # every node, no exemptions
    assert gap <= bar, (name, gap)
    assert (phi < 0).sum() > 0 and (phi > 0).sum() > 0, name
    return gap


# ---------------------------------------------------------------- 1: the builder
def test_build_matches_the_reference():
    gaps = {}
    for name, (v, t), n_t in (("box", mesh_box((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)), 12), ("icosphere", mesh_icosphere(2, 0.6), 320)):
        g, ref = _build(v, t)
        assert g.triangles == n_t and g.dropped == 0
        gaps[name] = _compare(name, g, ref)
        assert g.closedness < 1e-4, (name, g.closedness)
        w = ref[1]
        assert np.abs(np.abs(w) - np.round(np.abs(w))).max() < 1e-9
        again = SdfGrid.from_mesh(v, t, lo=LO, spacing=S, res=RES, device=DEV)
        assert torch.equal(g.values.view(torch.int32), again.values.view(torch.int32)), name     # no atomics: a second build, the same bits
        flipped, _ = _build(v, t[:, ::-1].copy())                                             # the other orientation: w = -1 inside, the same signs
        _compare(name + ", flipped", flipped, ref)
    print("measured distance gaps:", gaps)


def test_build_two_disjoint_boxes():
    """One mesh, two solids apart: the winding number is 1 inside either and 0 between them."""
    v1, t1 = mesh_box((-0.4, -0.1, 0.05), (0.2, 0.45, 0.3))
    v2, t2 = mesh_box((0.35, 0.2, -0.1), (0.25, 0.2, 0.4))
    v, t = np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])
    g, ref = _build(v, t)
    assert g.triangles == 24 and g.closedness < 1e-4
    _compare("two boxes", g, ref)
    phi = ref[0]
    q = R.node_positions(LO, S, RES)
    for c, h in (((-0.4, -0.1, 0.05), (0.2, 0.45, 0.3)), ((0.35, 0.2, -0.1), (0.25, 0.2, 0.4))):
        inside = (np.abs(q - np.array(c)) < np.array(h) - 0.01).all(axis=-1)
        assert inside.sum() > 20 and (phi[inside] < 0).all()
    between = (np.abs(q[..., 0] + 0.05) < 0.1)          # the gap between the two, -0.2 < x < 0.1
    assert between.sum() > 100 and (phi[between] > 0).all()


def test_build_two_solids_ragged_tile_and_ragged_brick():
    """A sphere of 320 triangles and a box of 12, apart: 332 triangles = two LDS tiles of 128 and one of 76; 13 x 16 x 9 nodes = bricks cut on x and z.
    Degenerate triangles mixed in are dropped by the wrapper and counted."""
    v1, t1 = mesh_icosphere(2, 0.3, (0.0, -0.35, 0.0))
    v2, t2 = mesh_box((0.05, 0.4, 0.02), (0.2, 0.15, 0.1))
    v = np.concatenate([v1, v2])
    t = np.concatenate([t1, t2 + len(v1)])
    lo, res = (-0.64, -0.8, -0.43), (13, 16, 9)
    g, ref = _build(v, t, lo, S, res)
    assert g.triangles == 332 and g.triangles % 128 != 0 and res[0] % 8 and res[2] % 4
    _compare("sphere and box", g, ref)
    phi = ref[0]
    q = R.node_positions(lo, S, res)
    in_box = np.abs(q - np.float32([0.05, 0.4, 0.02]).astype(np.float64)).max(axis=-1) < 0.09
    in_ball = np.linalg.norm(q - np.array([0.0, -0.35, 0.0]), axis=-1) < 0.25
    assert in_box.sum() > 0 and in_ball.sum() > 10 and (phi[in_box] < 0).all() and (phi[in_ball] < 0).all()      # both solids have an inside
    junk = np.array([[0, 0, 1], [5, 5, 5]], np.int32)
    g2 = SdfGrid.from_mesh(v, np.concatenate([junk[:1], t, junk[1:]]), lo=lo, spacing=S, res=res, device=DEV)
    assert g2.dropped == 2 and g2.triangles == 332 and torch.equal(g2.values.view(torch.int32), g.values.view(torch.int32))
    # an open mesh: the winding number leaves the integers, the wrapper warns
    with pytest.warns(UserWarning, match="the mesh is open"):
        open_box = SdfGrid.from_mesh(v2, t2[:-2], lo=lo, spacing=S, res=res, device=DEV)
    assert open_box.closedness > 0.1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        auto = SdfGrid.from_mesh(v2, t2, resolution=12, device=DEV)       # the default box: the bounds plus two voxels
    assert max(auto.res) == 12 and (auto.lo < v2.min(axis=0) - 1.9 * auto.spacing).all() and (auto.hi > v2.max(axis=0) + 1.9 * auto.spacing).all()
    assert float(auto.values.min()) < 0 and auto.closedness < 1e-4


# ---------------------------------------------------------------- 2: contact against the grids
@pytest.fixture(scope="module")
def grids():
    ball = SdfGrid.from_function(lambda p: np.sqrt((p * p).sum(axis=1)) - 0.5, (-0.625, -0.625, -0.625), 0.0625, (21, 21, 21), device=DEV)
    floor = SdfGrid.from_function(lambda p: p[:, 1] + 0.8125, (-1.0, -1.0, -1.0), 0.125, (17, 17, 17), device=DEV)
    assert np.array_equal(floor.values.cpu().numpy().astype(np.float64)[:, 3, :], np.full((17, 17), -1.0 + 3 * 0.125 + 0.8125))     # exact in fp32
    return dict(ball=ball, floor=floor)


def _ref_mesh(g, offset=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0)):
    return R.mesh_collider(g.values.cpu().numpy(), g.lo, g.spacing, offset, velocity)


def _sdf_extra(ref, meshes, par, touched_by):
    """The grids' term for the oracle's current state, as OracleContact's `extra`; touched_by gets, per substep, how many points each grid acts on."""
    def extra(k):
        topo = ref.IP_kernel.numpy()
        x, v = ip_state(topo, ref.IP_Nx, ref.dof, ref.dof_vel)
        a, _ = R.sdf_accel(meshes, x, v, ref.dt, *par)
        touched_by.append(tuple(int(R.sdf_accel([m], x, v, ref.dt, *par)[1].sum()) for m in meshes))
        return contact_term(ref.n_k, topo, ref.IP_Nx, ref.IP_rho * ref.dx ** 3, a)
    return extra


@pytest.fixture(scope="module")
def oracle_runs(small_cloud, small_opt, grids):
    """Computed once: the oracle under gravity and the pick force for 24 substeps without contact (its state after 12 of them: the deformed, moving
    state of the term tests), and with the container as a collider and the floor and ball grids as its `extra`."""
    plain = OracleContact(make_oracle_sim(small_cloud, small_opt), [])
    plain.ref.update_force(plain.ref.n_IP // 2, FORCE)
    free = []
    for k in range(N_TRAJ):
        free.append(plain.step().copy())
        if k == 11:
            state12 = (plain.ref.dof.copy(), plain.ref.dof_vel.copy())
    ref = make_oracle_sim(small_cloud, small_opt)
    meshes = [_ref_mesh(grids["floor"]), _ref_mesh(grids["ball"], BALL_OFFSET)]
    par = (0.5, 0.5, 0.5, 0.5 * ref.dx)
    by_grid = []
    con = OracleContact(ref, [sphere(SHELL["centre"], SHELL["radius"], inside=True)], extra=_sdf_extra(ref, meshes, par, by_grid))
    ref.update_force(ref.n_IP // 2, FORCE)
    touched = [con.step().copy() for _ in range(N_TRAJ)]
    return dict(free=free, state12=state12, touched=touched, by_grid=by_grid)


def _deformed(small_cloud, small_opt, oracle_runs):
    s = _sim(small_cloud, small_opt).enable_contact()
    dof, vel = oracle_runs["state12"]
    s.dof.copy_(torch.from_numpy(dof.reshape(-1)))
    s.dof_vel.copy_(torch.from_numpy(vel.reshape(-1)))
    assert np.abs(dof - s.dof_rest.cpu().numpy().reshape(-1, 3)).max() > 1e-2 and np.abs(vel).max() > 1e-2     # deformed and moving
    return s


def _numpy_term(s, colliders, meshes, par):
    topo, Nx = s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy()
    x, v = ip_state(topo, Nx, s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    a, hit = R.contact_and_sdf_accel(colliders, meshes, x, v, s.dt, *par)
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    return contact_term(s.n_k, topo, Nx, m, a), a, hit, x


def test_term_equals_the_numpy_term(small_cloud, small_opt, oracle_runs, grids):
    s = _deformed(small_cloud, small_opt, oracle_runs)
    g = s.rhs_gravity.clone()
    par = tuple(s._contact_params)
    assert par == (0.5, 0.5, 0.5, 0.05) and s.mesh_collider_state() is None         # nothing new is allocated without a mesh collider
    tilted = dict(point=(0.0, -0.8, 0.0), normal=(0.2, 1.0, -0.1), velocity=(0.0, 0.5, 0.1))
    assert s.add_plane(**tilted) == 0
    assert s.add_mesh_collider(grids["ball"], offset=BALL_OFFSET, velocity=BALL_VEL) == 0
    colliders = [plane(tilted["point"], tilted["normal"], tilted["velocity"])]
    meshes = [_ref_mesh(grids["ball"], BALL_OFFSET, BALL_VEL)]
    want, a, hit, x = _numpy_term(s, colliders, meshes, par)
    _, a_plane, hit_plane, _ = _numpy_term(s, colliders, [], par)
    by_grid = (a != a_plane).any(axis=1)
    out = s._enqueue_contact_rhs(g).clone()
    acc = s.contact_accel().clone()
    again = s._enqueue_contact_rhs(g)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(acc), _bits(s.contact_accel()))      # two runs, equal bits
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err((out - g).cpu().numpy().reshape(-1, 3), want)
    print(f"plane and sphere grid: {int(hit.sum())} of {s.n_IP} points in contact, {int(by_grid.sum())} of them with the grid, "
          f"{int((by_grid & hit_plane).sum())} with both; max|term| {np.abs(want).max():.3e}; rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert by_grid.sum() > 5 and hit_plane.sum() > 5 and np.abs(want).max() > 1.0
    assert e_a < 1e-12 and e_t < 1e-12, (e_a, e_t)
    assert s.contact_count() == int(hit.sum())                                     # contact_count() and contact_accel() include the mesh colliders
    assert np.array_equal(acc.cpu().numpy()[~hit], np.zeros((int((~hit).sum()), 3)))
    assert torch.equal(s.rhs_gravity, g)
    assert bytes(s.mesh_collider_state().view(torch.uint8).cpu().numpy().tobytes()) == s.mesh_collider_state_bytes()
    with pytest.raises(RuntimeError, match="one-launch form does not evaluate mesh colliders"):
        s._enqueue_contact_rhs(g, one_launch=True)
    # a scripted translation is followed: another offset and velocity, other numbers
    s.set_mesh_collider(0, offset=(0.1, 0.0, 0.8), velocity=(0.0, 0.0, 0.0))
    want2, a2, hit2, _ = _numpy_term(s, colliders, [_ref_mesh(grids["ball"], (0.1, 0.0, 0.8))], par)
    out2 = s._enqueue_contact_rhs(g)
    assert rel_err((out2 - g).cpu().numpy().reshape(-1, 3), want2) < 1e-12 and not np.array_equal(a2, a) and s.contact_count() == int(hit2.sum())
    assert bytes(s.mesh_collider_state().view(torch.uint8).cpu().numpy().tobytes()) == s.mesh_collider_state_bytes()
    # two grids that overlap at a point add up, in slot order
    assert s.add_mesh_collider(grids["floor"]) == 1
    want3, a3, hit3, _ = _numpy_term(s, colliders, [_ref_mesh(grids["ball"], (0.1, 0.0, 0.8)), _ref_mesh(grids["floor"])], par)
    out3 = s._enqueue_contact_rhs(g)
    assert rel_err((out3 - g).cpu().numpy().reshape(-1, 3), want3) < 1e-12 and rel_err(s.contact_accel().cpu().numpy(), a3) < 1e-12
    assert hit3.sum() > hit2.sum()
    # removed: the stage enqueues what it always did, and the one-launch form is back
    s.remove_mesh_collider(0)
    s.remove_mesh_collider(1)
    out4 = s._enqueue_contact_rhs(g).clone()
    assert torch.equal(_bits(out4), _bits(s._enqueue_contact_rhs(g, one_launch=True)))
    assert rel_err((out4 - g).cpu().numpy().reshape(-1, 3), _numpy_term(s, colliders, [], par)[0]) < 1e-12


def test_a_floor_as_a_grid_is_the_analytic_plane(small_cloud, small_opt, oracle_runs, grids):
    """The exactness test: the floor grid's values y + 0.8125 are exact in fp32 and linear, so the trilinear distance is the plane's and nh = (0, 1, 0)."""
    s = _deformed(small_cloud, small_opt, oracle_runs)
    g = s.rhs_gravity.clone()
    i = s.add_plane((0.0, -0.8125, 0.0), (0.0, 1.0, 0.0))
    want = s._enqueue_contact_rhs(g).clone()
    acc_want = s.contact_accel().clone()
    n_hit = s.contact_count()
    s.remove_collider(i)
    s.add_mesh_collider(grids["floor"])
    got = s._enqueue_contact_rhs(g).clone()
    acc = s.contact_accel().clone()
    x = ip_state(s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy(), s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())[0]
    assert (x >= -1.0).all() and (x < 1.0).all()              # every point lies inside the grid's box: the whole vector is compared
    e_r, e_a = rel_err(got.cpu().numpy(), want.cpu().numpy()), rel_err(acc.cpu().numpy(), acc_want.cpu().numpy())
    print(f"floor as a grid vs add_plane: {n_hit} of {s.n_IP} points in contact; rel err _rhs_contact {e_r:.2e}, accel {e_a:.2e}")
    assert n_hit > 5 and s.contact_count() == n_hit
    assert e_r <= 1e-12 and e_a <= 1e-12, (e_r, e_a)
    assert torch.equal(acc != 0, acc_want != 0)


def test_a_point_outside_the_box_and_an_empty_state_add_exactly_nothing(small_cloud, small_opt, oracle_runs, grids):
    s = _deformed(small_cloud, small_opt, oracle_runs)
    g = s.rhs_gravity.clone()
    g[g == 0.0] = -0.0
    s.add_plane((0.0, -0.8, 0.0), (0.2, 1.0, -0.1), velocity=(0.0, 0.5, 0.1))
    want = s._enqueue_contact_rhs(g).clone()
    acc_want = s.contact_accel().clone()
    assert s.contact_count() > 0 and s.mesh_collider_state() is None
    # every point lies outside the placed box: the three-launch path leaves the two-launch path's bits
    for off in ((10.0, 0.0, 0.0), (0.0, -1.3 - 0.625, 0.0), (0.0, 0.0, 1e300)):
        k = s.add_mesh_collider(grids["ball"], offset=off, velocity=(1.0, 2.0, 3.0))
        assert "mesh_colliders" in s.enabled_stage_names()
        got = s._enqueue_contact_rhs(g)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(s.contact_accel()), _bits(acc_want)), off
        s.remove_mesh_collider(k)
    # an empty second state, through the entry itself
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    assert s.mesh_collider_state() is not None and int(s.mesh_collider_state()[:1].view(torch.int32)[0].item()) == 0      # n = 0
    s.contact_accel().fill_(7.0)
    out = torch.full_like(want, 7.0)
    check(lib().pn_sim_contact_sdf_rhs(s.n_k, s.n_IP, ptr(s._contact_state), ptr(s.mesh_collider_state()), float(s.dt), float(s.dx), ptr(s.dof),
                                       ptr(s.dof_vel), ptr(s.IP_kernel), ptr(s.IP_rho), ptr(s.IP_Nx), ptr(s.kernel_bg), ptr(s.kernel_cnt), ptr(s.buffer),
                                       ptr(s.Nx_csr), ptr(g), ptr(out), ptr(s._contact_accel), stream_ptr()), "sim_contact_sdf_rhs")
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(s.contact_accel()), _bits(acc_want))
    # an inactive contact state: nothing from the grids either
    s.add_mesh_collider(grids["floor"])
    assert not torch.equal(_bits(s._enqueue_contact_rhs(g)), _bits(want))
    check(lib().pn_sim_contact_set_params(ptr(s._contact_state), 0, None, stream_ptr()), "sim_contact_set_params")
    assert torch.equal(_bits(s._enqueue_contact_rhs(g)), _bits(g)) and s.contact_count() == 0


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_runs, grids, monkeypatch, form):
    monkeypatch.setenv("PN_SIM_FORM", form)
    s = _sim(small_cloud, small_opt)
    assert s.cell_form == (form == "cells")
    s.enable_contact()
    s.add_sphere(**SHELL)
    s.add_mesh_collider(grids["floor"])
    s.add_mesh_collider(grids["ball"], offset=BALL_OFFSET)
    s.update_force(s.n_IP // 2, FORCE)
    got = []
    for _ in range(N_TRAJ):
        s.stepforward()
        got.append(_disp(s))
    errs = [rel_err(a, b) for a, b in zip(got, oracle_runs["touched"])]
    print(f"{form} form with a container and two grids vs oracle, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    for k, e in enumerate(errs):
        assert e < 1e-4, (k, e)
    diff = float(np.abs(got[-1] - oracle_runs["free"][-1]).max())
    print(f"points in contact in the last substep: {s.contact_count()}; last state vs a run without contact: max abs difference {diff:.3e}")
    assert s.contact_count() > 0 and diff > 1e-3      # the colliders really moved it
    by_grid = oracle_runs["by_grid"]                    # ... and the grids did, not the container alone: on the oracle each acts on points
    print(f"points the (floor, ball) grids act on, per oracle substep: {by_grid}")
    assert len(by_grid) == N_TRAJ and all(f > 0 for f, _ in by_grid) and max(b for _, b in by_grid) > 0


# ---------------------------------------------------------------- 3: the captured step
def _harness(small_opt, small_cloud, ckpt, grids, W=64):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_contact()
    h.sim.add_sphere(**SHELL)
    h.mesh = [h.sim.add_mesh_collider(grids["floor"]), h.sim.add_mesh_collider(grids["ball"], offset=BALL_OFFSET)]
    return h


def _raise_floor(h):
    h.sim.set_mesh_collider(h.mesh[0], offset=(0.0, 0.03, 0.0), velocity=(0.0, 5.0, 0.0))


def test_captured_step_with_mesh_colliders_equals_eager_steps(small_opt, small_cloud, ckpt, grids):
    e = _harness(small_opt, small_cloud, ckpt, grids)
    g = _harness(small_opt, small_cloud, ckpt, grids).capture(n_trips=8)
    assert "mesh_colliders" in g._captured_graph.stages and torch.equal(g.sim.dof, g.sim.dof_rest)
    counts, errs = [], []
    for f in range(6):
        if f == 3:      # a grid moved between two replays is followed without a recapture
            _raise_floor(e)
            _raise_floor(g)
        want = e.to_host(e.step())
        e.synchronize()
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        errs.append(rel_err(_disp(g.sim), _disp(e.sim)))
        counts.append((e.sim.contact_count(), g.sim.contact_count()))
        print(f"frame {f}: captured vs eager displacement rel err {errs[-1]:.2e}, points in contact {counts[-1]}")
        assert np.abs(b["image"][0].cpu().numpy() - want["image"]).max() < 1e-5, f
        assert torch.equal(_bits(g.sim.dof), _bits(e.sim.dof)) and torch.equal(_bits(g.sim.dof_vel), _bits(e.sim.dof_vel)), (f, errs[-1])
    assert all(a == b for a, b in counts) and min(a for a, _ in counts) > 0
    p = _harness(small_opt, small_cloud, ckpt, grids)      # without the raise the state would be another: the change really acted
    for _ in range(6):
        p.step()
    p.synchronize()
    assert np.abs(_disp(p.sim) - _disp(g.sim)).max() > 1e-4
    # a graph captured before the first mesh collider lacks its launch and refuses to run
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV)
    plain.sim.enable_contact()
    plain.sim.add_sphere(**SHELL)
    plain.capture(n_trips=8)
    plain.step_graph()
    plain.finish_graph_frame()
    k = plain.sim.add_mesh_collider(grids["floor"])
    with pytest.raises(RuntimeError, match=r"mesh colliders: the step graph was captured before add_mesh_collider\(\)"):
        plain.step_graph()
    plain.sim.remove_mesh_collider(k)      # none left: the captured launches are all there are again
    plain.step_graph()
    plain.finish_graph_frame()
    plain.synchronize()


# ---------------------------------------------------------------- 4: main_render --collide_mesh
def test_main_render_drops_the_chair_onto_a_mesh(tmp_path, small_cloud, capsys):
    """--unpin --collide_mesh slab.ply: a box mesh whose top is at y = -0.95, as test_gpu_contact.py's --floor -0.95; thickness 0.1."""
    import re
    from pienerf_amd import main_render, scene
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    scene.write_mesh_ply(str(tmp_path / "slab.ply"), *mesh_box((0.0, -0.2, 0.0), (1.2, 0.25, 1.2)))
    args = main_render.parser().parse_args(["--ply", str(tmp_path / "chair.ply"), "--out", str(tmp_path / "out"), "--W", "48", "--H", "48", "--sim_dx", "0.1",
                                            "--sim_iters", "4", "--unpin", "--collide_mesh", str(tmp_path / "slab.ply"), "0", "-1", "0",
                                            "--mesh_collider_res", "40", "--contact_thickness", "0.1", "--frames", "3", "--save_ply"])
    files = main_render.run(args)
    assert [f.split("/")[-1] for f in files] == [f"img_{f}.png" for f in range(3)]
    said = capsys.readouterr().out
    m = re.search(r"contact: (\d+) of (\d+) integration points", said)
    assert m and "--collide_mesh" in said and "12 triangles (0 dropped)" in said, said
    print(m.group(0))
    assert int(m.group(1)) > 0 and int(m.group(2)) == 432
    y0 = np.asarray(small_cloud["pos"], np.float64)[:, 1]
    pts = scene.read_ply(str(tmp_path / "out" / "points_2.ply"))
    drop = y0 - np.asarray(pts["y"], np.float64)
    print(f"points_2.ply: the points fell by {drop.min():.5f}..{drop.max():.5f}")
    assert drop.max() > 1e-3 and drop.min() > -0.05
