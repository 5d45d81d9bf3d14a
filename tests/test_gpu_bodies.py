"""Rigid balls on the GPU (csrc/pn_bodies.hip; Simulator.enable_bodies / add_body / set_body ...; main_render --ball): the reaction, the clamp and the
integrated ball against the numpy restatement (tests/bodies_reference.py), trajectories of object and ball against the CPU oracle in the cell and CSR
forms, keep_state / restore_state, and the harness forms (eager, captured step, pipelined).  All on the small cloud: 432 integration points are two
workgroups of 256 with a ragged second one."""
import numpy as np
import pytest
import torch

from bodies_reference import OracleBodies, body, step_bodies
from conftest import make_oracle_sim, rel_err
from contact_reference import OracleContact, ip_state, plane
from pienerf_amd.harness import SimRenderHarness
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

FORCE = np.array([300.0, 100.0, -200.0])            # conftest's pick force, on IP n_IP // 2
THROW = dict(centre=(0.0, 0.0, 1.3), radius=0.3, velocity=(0.0, 0.0, -4.0))
M_CLOUD, M_MID, M_LIGHT = 440.64, 4.4, 0.04          # the cloud's total mass; a ball that bounces back; one the clamp has to hold
N_TRAJ, N_LIGHT = 24, 16
TILTED = dict(point=(0.0, -0.45, 0.0), normal=(0.2, 1.0, -0.1), velocity=(0.0, 0.5, 0.1))
BALL5 = dict(centre=(0.0, 0.0, 0.9), radius=0.5, velocity=(0.3, 0.0, -0.2))
G5 = (0.3, -9.8, 0.1)


def _sim(cloud, opt):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV, persistent=False)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def _disp(s):
    return (s.dof - s.dof_rest).cpu().numpy().reshape(-1, 3)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _thrown(s, mass, gravity=(0.0, 0.0, 0.0)):
    s.enable_contact().enable_bodies(gravity=gravity)
    return s.add_body(mass=mass, **THROW)


def _ref_throw(cloud, opt, mass, n, clamp=True):
    o = OracleBodies(make_oracle_sim(cloud, opt), [body(THROW["centre"], THROW["radius"], mass, THROW["velocity"])], clamp=clamp)
    disp, balls, hits = [], [], []
    for _ in range(n):
        disp.append(o.step().copy())
        b = o.bodies()[0]
        balls.append((b["p"].copy(), b["v"].copy()))
        hits.append(o.hits)
    return dict(disp=disp, balls=balls, hits=hits, clamped=o.bodies()[0]["clamped"])


@pytest.fixture(scope="module")
def oracle_runs(small_cloud, small_opt):
    """Computed once: the oracle's deformed, moving state after 12 substeps under the pick force (test_gpu_contact's state12 recipe); the throw of the
    trajectory test with the heavy ball; the light ball with the clamp and without it."""
    plain = OracleContact(make_oracle_sim(small_cloud, small_opt), [])
    plain.ref.update_force(plain.ref.n_IP // 2, FORCE)
    for _ in range(12):
        plain.step()
    return dict(state12=(plain.ref.dof.copy(), plain.ref.dof_vel.copy()), heavy=_ref_throw(small_cloud, small_opt, M_CLOUD, N_TRAJ),
                light=_ref_throw(small_cloud, small_opt, M_LIGHT, N_LIGHT), unclamped=_ref_throw(small_cloud, small_opt, M_LIGHT, N_LIGHT, clamp=False))


# ---------------------------------------------------------------- 1: the reaction and the integrated ball against numpy
def _slot5(s, dynamic):
    """A tilted moving plane in slot 0 (it meets the ball and the object), slots 1-4 empty, the ball in slot 5: n = 6 with skipped slots."""
    s.enable_contact()
    if dynamic:
        s.enable_bodies(gravity=G5)
    s.add_plane(**TILTED)
    fill = [s.add_sphere((0.0, 5.0, 0.0), 0.1) for _ in range(4)]
    i = s.add_body(mass=50.0, damping=0.4, **BALL5) if dynamic else s.add_sphere(**BALL5)
    for j in fill:
        s.remove_collider(j)
    assert i == 5 and s.collider_types() == [1, 0, 0, 0, 0, 2, 0, 0]
    return i


def test_reaction_and_step_equal_numpy(small_cloud, small_opt, oracle_runs):
    s, kin = _sim(small_cloud, small_opt), _sim(small_cloud, small_opt)
    dof, vel = oracle_runs["state12"]
    for t in (s, kin):
        t.dof.copy_(torch.from_numpy(dof.reshape(-1)))
        t.dof_vel.copy_(torch.from_numpy(vel.reshape(-1)))
    assert (s.n_IP, s.n_k) == (432, 139)
    b = _slot5(s, True)
    _slot5(kin, False)
    # the object's side: bit-equal to the same sphere as a kinematic collider with the same velocity
    g = s.rhs_gravity.clone()
    out, acc = s._enqueue_contact_rhs(g).clone(), s.contact_accel().clone()
    assert torch.equal(_bits(out), _bits(kin._enqueue_contact_rhs(g))) and torch.equal(_bits(acc), _bits(kin.contact_accel()))
    assert s.contact_count() == kin.contact_count() > 0
    assert bytes(s._contact_state.view(torch.uint8).cpu().numpy().tobytes()) == s.contact_state_bytes()      # before its first substep the mirror holds
    assert bytes(s._bodies_state.view(torch.uint8).cpu().numpy().tobytes()) == s.bodies_state_bytes()
    # the numpy restatement from the same state
    par = tuple(s._contact_params)
    x, v = ip_state(s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy(), dof.reshape(-1), vel.reshape(-1))
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    ref = [plane(TILTED["point"], TILTED["normal"], TILTED["velocity"]), None, None, None, None,
           body(BALL5["centre"], BALL5["radius"], 50.0, BALL5["velocity"], damping=0.4)]
    step_bodies(ref, x, v, m, s.dt, G5, *par)
    want = ref[5]
    assert s._enqueue_bodies(g) is g                   # a link only for its place in the order
    got = s.body_state()[b]
    errs = {k: rel_err(got[k], want[w]) for k, w in (("reaction", "F"), ("centre", "p"), ("velocity", "v"))}
    e_d = abs(got["delta_max"] - want["delta_max"]) / want["delta_max"]
    n_touch = int((np.linalg.norm(x - np.asarray(BALL5["centre"]), axis=1) - BALL5["radius"] < par[3]).sum())
    print(f"slot 5: {n_touch} of {s.n_IP} points touch the ball, |F| {np.linalg.norm(want['F']):.4e}, delta_max {want['delta_max']:.4e}, s {want['s']:.4f}; "
          f"rel err F {errs['reaction']:.2e}, centre {errs['centre']:.2e}, velocity {errs['velocity']:.2e}, delta_max {e_d:.2e}")
    assert n_touch > 10 and np.linalg.norm(want["F"]) > 1.0        # so the bar means something
    assert np.abs(want["v"] - np.asarray(BALL5["velocity"])).max() > 1e-3   # ... and the static plane and the reaction really moved it
    assert max(errs.values()) < 1e-12 and e_d < 1e-12, (errs, e_d)
    assert abs(got["scale"] - want["s"]) <= 1e-12 and got["clamped"] == want["clamped"] and s.body_clock() == 1
    # contact's own buffers are left alone by the bodies' launches
    assert torch.equal(_bits(s._rhs_contact), _bits(out)) and torch.equal(_bits(s.contact_accel()), _bits(acc))
    # the same state again: equal bits
    s.set_body(b, centre=BALL5["centre"], velocity=BALL5["velocity"])
    s._enqueue_bodies(g)
    again = s.body_state()[b]
    for k in ("reaction", "centre", "velocity"):
        assert np.array_equal(got[k].view(np.int64), again[k].view(np.int64)), k
    assert (got["scale"], got["delta_max"]) == (again["scale"], again["delta_max"]) and s.body_clock() == 2
    # the one-launch form (the last workgroup to arrive does the second launch's work): the same bits, twice (the counter is left at zero)
    for k in (3, 4):
        s.set_body(b, centre=BALL5["centre"], velocity=BALL5["velocity"])
        s._enqueue_bodies(g, one_launch=True)
        one = s.body_state()[b]
        for name in ("reaction", "centre", "velocity"):
            assert np.array_equal(got[name].view(np.int64), one[name].view(np.int64)), (k, name)
        assert (got["scale"], got["delta_max"]) == (one["scale"], one["delta_max"]) and s.body_clock() == k
    # the kinematic twin's sphere is where it was
    assert bytes(kin._contact_state.view(torch.uint8).cpu().numpy().tobytes()) == kin.contact_state_bytes()


# ---------------------------------------------------------------- 2: a body nothing touches
def test_untouched_bodies_fall_freely_and_settle_on_a_floor(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt)
    s.enable_contact().enable_bodies()                 # the simulator's gravity
    g, dt, c = np.array([0.0, -9.8, 0.0]), s.dt, 0.7
    s.add_plane((0.0, -6.0, 0.0), (0.0, 1.0, 0.0))     # far below the object, which sags by a unit under gravity in these 200 substeps
    rest = s.add_body((0.0, -5.75, 0.0), 0.25, 3.0)    # resting on the floor
    far = s.add_body((3.0, 40.0, 0.5), 0.2, 2.0, velocity=(1.0, 2.0, -0.5), damping=c)
    p, u = np.array([3.0, 40.0, 0.5]), np.array([1.0, 2.0, -0.5])
    for k in range(200):
        s.stepforward()
        if k < 50:
            u = (u + dt * g) / (1.0 + dt * c)
            p = p + dt * u
        if k in (0, 9, 49):
            b = s.body_state()[far]
            e_p, e_u = rel_err(b["centre"], p), rel_err(b["velocity"], u)
            print(f"free fall after {k + 1} substeps: rel err centre {e_p:.2e}, velocity {e_u:.2e}")
            assert e_p < 1e-13 and e_u < 1e-13
            assert not b["reaction"].any() and not np.signbit(b["reaction"]).any() and b["scale"] == 1.0 and b["delta_max"] == 0.0 and b["clamped"] == 0
    assert s.contact_count() == 0 and s.body_clock() == 200
    b = s.body_state()[rest]
    pen = 0.25 - (b["centre"][1] + 6.0)
    print(f"ball on the floor after 200 substeps: penetration {pen:.6e}, speed {np.linalg.norm(b['velocity']):.3e}")
    assert abs(pen - 9.8 * dt * dt / 0.5) < 1e-6 and np.linalg.norm(b["velocity"]) < 1e-6
    assert not b["reaction"].any() and b["clamped"] == 0


# ---------------------------------------------------------------- 3: object and ball against the oracle, cell and CSR forms
@pytest.mark.parametrize("form", ["cells", "csr"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_runs, monkeypatch, form):
    monkeypatch.setenv("PN_SIM_FORM", form)
    s = _sim(small_cloud, small_opt)
    assert s.cell_form == (form == "cells")
    b = _thrown(s, M_CLOUD)
    want = oracle_runs["heavy"]
    e_obj, e_p, e_u, speed = [], [], [], []
    for k in range(N_TRAJ):
        s.stepforward()
        st = s.body_state()[b]
        e_obj.append(rel_err(_disp(s), want["disp"][k]))
        e_p.append(rel_err(st["centre"], want["balls"][k][0]))
        e_u.append(rel_err(st["velocity"], want["balls"][k][1]))
        speed.append(float(np.linalg.norm(st["velocity"])))
    print(f"{form} form, ball of mass {M_CLOUD} thrown at the cloud, vs oracle per substep:")
    print("  object: " + " ".join(f"{e:.1e}" for e in e_obj))
    print("  ball centre: " + " ".join(f"{e:.1e}" for e in e_p))
    print("  ball velocity: " + " ".join(f"{e:.1e}" for e in e_u))
    print(f"  points in contact on the oracle: {want['hits']}; on the device in the last substep: {s.contact_count()}; ball speed 4.0 -> {speed[-1]:.4f}")
    for k in range(N_TRAJ):
        assert e_obj[k] < 1e-4 and e_p[k] < 1e-4 and e_u[k] < 1e-4, (k, e_obj[k], e_p[k], e_u[k])
    assert want["hits"][10] == 0 and max(want["hits"]) >= 25 and s.contact_count() > 0      # contact happened, from substep 12 on
    assert speed[0] == 4.0 and speed[-1] < 3.0                                                                   # ... and the ball really slowed
    assert st["clamped"] == want["clamped"] == 0 and s.body_clock() == N_TRAJ


# ---------------------------------------------------------------- 4: the clamp
def test_a_light_ball_is_clamped(small_cloud, small_opt, oracle_runs):
    s = _sim(small_cloud, small_opt)
    b = _thrown(s, M_LIGHT)
    want, wild = oracle_runs["light"], oracle_runs["unclamped"]
    speeds, scales = [], []
    for k in range(N_LIGHT):
        s.stepforward()
        st = s.body_state()[b]
        speeds.append(float(np.linalg.norm(st["velocity"])))
        scales.append(st["scale"])
    wild_speed = max(float(np.linalg.norm(v)) for _, v in wild["balls"])
    print(f"mass {M_LIGHT}: clamped substeps {st['clamped']} (reference {want['clamped']}), scales {[f'{x:.3g}' for x in scales if x < 1.0]}, "
          f"largest speed {max(speeds):.3f}; unclamped reference {wild_speed:.1f}")
    assert st["clamped"] == want["clamped"] > 0
    assert max(speeds) < wild_speed and wild_speed > 100.0      # the unclamped law throws the ball off at 147 units/s
    assert rel_err(st["velocity"], want["balls"][-1][1]) < 1e-4 and rel_err(st["centre"], want["balls"][-1][0]) < 1e-4


# ---------------------------------------------------------------- 5: state
def test_keep_restore_and_the_setters(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt)
    s.enable_contact().enable_bodies()
    b = s.add_body((0.0, 0.0, 0.85), 0.3, M_MID, velocity=(0.0, 0.0, -4.0))      # in reach: the object pushes it from the first substeps on

    def three():
        for _ in range(3):
            s.stepforward()
        return s.dof.clone(), s.dof_vel.clone(), s._contact_state.clone(), s._bodies_state.clone(), s.contact_count()

    keep = s.keep_state()
    assert set(keep) == {"dof", "dof_vel", "clocks", "bodies"}
    first = three()
    assert first[4] > 0 and s.body_clock() == 3 and np.abs(s.body_state()[b]["reaction"]).max() > 0.0
    s.restore_state(keep)
    s.reset_warm_start()
    assert s.body_clock() == 0 and np.array_equal(s.body_state()[b]["centre"], [0.0, 0.0, 0.85])
    second = three()
    for x, y in zip(first[:4], second[:4]):
        assert torch.equal(_bits(x), _bits(y))
    # set_body(velocity=...) changes the velocity alone
    before = s.body_state()[b]
    s.set_body(b, velocity=(1.0, 2.0, 3.0))
    after = s.body_state()[b]
    assert after["velocity"].tolist() == [1.0, 2.0, 3.0]
    for k in ("centre", "reaction"):
        assert np.array_equal(before[k], after[k]), k
    assert (before["mass"], before["scale"], before["clamped"]) == (after["mass"], after["scale"], after["clamped"])
    s.set_body(b, mass=9.0, damping=0.25)
    again = s.body_state()[b]
    assert (again["mass"], again["damping"]) == (9.0, 0.25) and np.array_equal(again["centre"], after["centre"]) and again["velocity"].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="set_body"):
        s.set_collider(b, centre=(0.0, 0.0, 0.0))
    # stop_bodies: the ball stays where it is, the clock counts on
    s.stop_bodies()
    s.stepforward()
    held = s.body_state()[b]
    assert np.array_equal(held["centre"], again["centre"]) and s.body_clock() == 4
    s.enable_bodies()
    s.stepforward()
    assert not np.array_equal(s.body_state()[b]["centre"], again["centre"])
    s.reset_body_clock(40)
    assert s.body_clock() == 40
    # remove_body frees the slot
    s.remove_body(b)
    assert s.body_indices() == [] and s.collider_types() == [0] * 8 and s.body_state() == {}
    assert bytes(s._contact_state.view(torch.uint8).cpu().numpy().tobytes()) == s.contact_state_bytes()
    s.stepforward()
    assert s.contact_count() == 0
    assert s.add_body((0.0, 0.0, 2.0), 0.2, 1.0) == b
    fresh = s.body_state()[b]
    assert fresh["clamped"] == 0 and fresh["scale"] == 1.0 and not fresh["reaction"].any()


# ---------------------------------------------------------------- 6: the harness forms
NEAR = dict(centre=(0.0, 0.0, 0.9), radius=0.3, velocity=(0.0, 0.0, -4.0))


def _harness(small_opt, small_cloud, ckpt, overlay, W=48):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_contact().enable_bodies(gravity=(0.0, 0.0, 0.0))
    h.ball = h.sim.add_body(mass=M_CLOUD, **NEAR)
    if overlay:
        h.draw_colliders()
    return h


def _ball_bits(h):
    b = h.sim.body_state()[h.ball]
    return np.concatenate([b["centre"], b["velocity"], b["reaction"]]).view(np.int64)


def test_captured_step_with_bodies_equals_eager_steps(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt, True)
    g = _harness(small_opt, small_cloud, ckpt, True).capture(n_trips=8)
    start = g.sim.body_state()[g.ball]
    assert torch.equal(g.sim.dof, g.sim.dof_rest) and g.sim.body_clock() == 0             # capture's warm-up steps left the state where it was
    assert start["centre"].tolist() == list(NEAR["centre"]) and start["velocity"].tolist() == list(NEAR["velocity"])   # ... and the ball
    for f in range(6):
        want = e.to_host(e.step())
        e.synchronize()
        got = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(got["image"][0].cpu().numpy() - want["image"]).max() < 1e-5, f      # the drawn ball is this frame's own
        assert torch.equal(_bits(g.sim.dof), _bits(e.sim.dof)) and torch.equal(_bits(g.sim.dof_vel), _bits(e.sim.dof_vel)), f
        assert np.array_equal(_ball_bits(g), _ball_bits(e)), f
    moved = g.sim.body_state()[g.ball]
    print(f"after 6 frames: ball at z {moved['centre'][2]:.4f}, speed {np.linalg.norm(moved['velocity']):.4f}, {g.sim.contact_count()} points in contact")
    assert g.sim.contact_count() == e.sim.contact_count() > 0 and g.sim.body_clock() == 6 and moved["centre"][2] < 0.75
    # a graph captured without the bodies' launches refuses to run once they are enabled
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV)
    plain.sim.enable_contact()
    plain.capture(n_trips=8)
    plain.step_graph()
    plain.finish_graph_frame()
    plain.sim.enable_bodies()
    with pytest.raises(RuntimeError, match="captured before enable_bodies"):
        plain.step_graph()


def test_pipelined_frames_with_bodies(small_opt, small_cloud, ckpt):
    with pytest.raises(RuntimeError, match="bodies: the pipelined form"):
        _harness(small_opt, small_cloud, ckpt, True).capture_pipelined(lanes=2, depth=2, n_trips=8)
    e = _harness(small_opt, small_cloud, ckpt, False)
    p = _harness(small_opt, small_cloud, ckpt, False).capture_pipelined(lanes=2, depth=2, n_trips=8)
    n = 6
    for _ in range(n):
        p.step_pipelined()
    p.drain_pipeline()
    for _ in range(p.substeps_enqueued):     # the pipeline's simulator runs ahead of its frames
        e.step()
    e.synchronize()
    err = rel_err(_disp(p.sim), _disp(e.sim))
    bp, be = p.sim.body_state()[p.ball], e.sim.body_state()[e.ball]
    print(f"pipelined (lanes 2, depth 2) with a ball vs eager after {p.substeps_enqueued} substeps: {err:.2e}; {p.sim.contact_count()} points in contact")
    assert err < 1e-7 and p.sim.contact_count() == e.sim.contact_count() > 0
    assert rel_err(bp["centre"], be["centre"]) < 1e-7 and rel_err(bp["velocity"], be["velocity"]) < 1e-7 and p.sim.body_clock() == p.substeps_enqueued
