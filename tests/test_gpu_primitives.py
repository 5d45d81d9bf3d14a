"""Box and capsule colliders on the GPU (csrc/pn_contact_law.h, csrc/pn_colliders.hip; Simulator.add_box / add_capsule; main_render --collide_box /
--collide_capsule): the contact term against the numpy law (tests/primitives_reference.py), trajectories against the CPU oracle, the harness forms, a
ball on a box, the drawn frame and its shadows bit for bit against the float32 restatement, and main_render end to end.

Draw comparison rule: rays the restatement flags (two operands of one of the new decisions within a few ulp: a face tie, an edge graze, a part tie, the
near end against t_min) are left out, fewer than 1 % of the rays that hit; every other ray is compared bit for bit."""
import collections
import re

import numpy as np
import pytest
import torch

import colliders_reference as cr
import primitives_reference as pr
import shadows_reference as sr
import test_gpu_colliders as GC
import test_gpu_shadows as GS
from conftest import make_oracle_sim, rel_err
from contact_reference import OracleContact, contact_term, ip_state, plane, sphere
from pienerf_amd import scene
from pienerf_amd.colliders import collider_style, shadow_light
from pienerf_amd.harness import SimRenderHarness
from test_gpu_contact import BALL, FLOOR, FORCE, N_TRAJ, SHELL, _bits, _disp, _sim
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

# the term test's colliders, chosen on the CPU from the oracle's state after 12 substeps (the seat's two layers of points lie at y = -0.1 and 0.0, the legs
# below, the back and the arms above): with thickness 0.15 the box's hit points cover all 26 outside regions and the three inside axes, the capsule's
# both caps and the body — asserted below, from the reference alone
H_TERM = 0.15
TERM_BOX = dict(centre=(0.0, -0.09, 0.0), half_extents=(0.45, 0.05, 0.45), velocity=(0.3, 0.0, -0.2))
TERM_CAPSULE = dict(a=(-0.2, -0.05, 0.0), b=(0.3, -0.05, 0.1), radius=0.1, velocity=(0.0, 0.5, 0.1))
# the trajectories': a box under the legs (its +x edge inside the legs' footprint) and an upright rod beside the seat, on the side the pick force pushes to
UNDER = dict(centre=(-0.04, -1.03, 0.0), half_extents=(0.56, 0.2, 0.7))
BESIDE = dict(a=(0.72, -0.5, 0.0), b=(0.72, 0.5, 0.1), radius=0.15)
WIDE = dict(centre=(0.0, -1.33, 0.0), half_extents=(5.0, 0.5, 5.0))          # its top face is FLOOR's plane y = -0.83


def _ref_box(kw):
    return pr.box(kw["centre"], kw["half_extents"], kw.get("velocity", (0.0, 0.0, 0.0)))


def _ref_capsule(kw):
    return pr.capsule(kw["a"], kw["b"], kw["radius"], kw.get("velocity", (0.0, 0.0, 0.0)))


def _state_bytes(s):
    return bytes(s._contact_state.view(torch.uint8).cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def oracle_runs(small_cloud, small_opt):
    """Computed once: the oracle's state after 12 substeps under gravity and the pick force (the term test's), and 24 substeps with UNDER and BESIDE,
    their term evaluated from the oracle's own state at the start of each step and handed to OracleContact as `extra`."""
    plain = OracleContact(make_oracle_sim(small_cloud, small_opt), [])
    plain.ref.update_force(plain.ref.n_IP // 2, FORCE)
    for _ in range(12):
        plain.step()
    state12 = (plain.ref.dof.copy(), plain.ref.dof_vel.copy())
    ref = make_oracle_sim(small_cloud, small_opt)
    cols, hits = [_ref_box(UNDER), _ref_capsule(BESIDE)], []

    def extra(k):
        term, _, hit = pr.oracle_term(ref, cols, 0.5, 0.5, 0.5, 0.5 * ref.dx)
        hits.append(int(hit.sum()))
        return term
    con = OracleContact(ref, [], extra=extra)
    ref.update_force(ref.n_IP // 2, FORCE)
    touched = [con.step().copy() for _ in range(N_TRAJ)]
    return dict(state12=state12, touched=touched, hits=hits)


# ---------------------------------------------------------------- 6: the term against numpy
def _numpy_term(s, colliders, par):
    topo, Nx = s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy()
    x, v = ip_state(topo, Nx, s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    a, hit = pr.contact_accel(colliders, x, v, s.dt, *par)
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    return contact_term(s.n_k, topo, Nx, m, a), a, hit, x


def _check_term(s, colliders, par, name, g):
    """test_gpu_contact._check_term over primitives_reference's law.  Returns (hit mask, the points' positions)."""
    want, a, hit, x = _numpy_term(s, colliders, par)
    out = s._enqueue_contact_rhs(g).clone()
    acc = s.contact_accel().clone()
    again = s._enqueue_contact_rhs(g)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(acc), _bits(s.contact_accel())), name     # two runs, equal bits
    s.contact_accel().fill_(7.0)
    one = s._enqueue_contact_rhs(g, one_launch=True)      # the one-launch form: the same bits, accel left alone
    assert torch.equal(_bits(out), _bits(one)) and bool((s.contact_accel() == 7.0).all()), name
    s._enqueue_contact_rhs(g)
    got = (out - g).cpu().numpy().reshape(-1, 3)
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err(got, want)
    print(f"{name}: {int(hit.sum())} of {s.n_IP} points in contact, max|term| {np.abs(want).max():.3e}, rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert np.abs(want).max() > 1.0, name
    assert e_a < 1e-12 and e_t < 1e-12, (name, e_a, e_t)
    assert s.contact_count() == int(hit.sum()), name
    assert np.array_equal(acc.cpu().numpy()[~hit], np.zeros((int((~hit).sum()), 3)))
    untouched = np.ones(s.n_k, bool)
    untouched[np.unique(s.IP_kernel.cpu().numpy()[hit])] = False
    rows = torch.from_numpy(np.repeat(untouched, 30)).to(DEV)
    assert torch.equal(_bits(out[rows]), _bits(g[rows])), name
    assert _state_bytes(s) == s.contact_state_bytes(), name          # the device state is what the mirror says it is
    return hit, x


def _deformed(small_cloud, small_opt, oracle_runs):
    s = _sim(small_cloud, small_opt).enable_contact(thickness=H_TERM)
    dof, vel = oracle_runs["state12"]
    s.dof.copy_(torch.from_numpy(dof.reshape(-1)))
    s.dof_vel.copy_(torch.from_numpy(vel.reshape(-1)))
    assert np.abs(dof - s.dof_rest.cpu().numpy().reshape(-1, 3)).max() > 1e-2 and np.abs(vel).max() > 1e-2     # deformed and moving
    g = s.rhs_gravity.clone()
    g_neg = g.clone()
    g_neg[g_neg == 0.0] = -0.0
    assert int((g_neg == 0.0).sum()) > 100 and bool(torch.signbit(g_neg[g_neg == 0.0]).all())
    return s, g, g_neg


def test_term_equals_the_numpy_term(small_cloud, small_opt, oracle_runs):
    s, g, g_neg = _deformed(small_cloud, small_opt, oracle_runs)
    par = tuple(s._contact_params)
    assert par == (0.5, 0.5, 0.5, H_TERM)
    # a moving box: every region of the law among its hit points
    s.add_box(**TERM_BOX)
    ref = [_ref_box(TERM_BOX)]
    hit, x = _check_term(s, ref, par, "box", g)
    seen = collections.Counter(pr.regions(ref[0], x[hit]))
    faces, edges, corners = ([r for r in seen if not r.startswith("in") and 3 - r.count("0") == n] for n in (1, 2, 3))
    print(f"box regions among {int(hit.sum())} hit points: {dict(sorted(seen.items()))}")
    assert (len(faces), len(edges), len(corners)) == (6, 12, 8) and all(seen[f"in{k}"] > 0 for k in range(3))
    assert sorted(seen) == pr.BOX_REGIONS and 0 < hit.sum() < s.n_IP
    _check_term(s, ref, par, "box, -0.0 in rhs_in", g_neg)
    # a moving capsule: both caps and the body
    s.clear_colliders()
    s.add_capsule(**TERM_CAPSULE)
    ref = [_ref_capsule(TERM_CAPSULE)]
    hit, x = _check_term(s, ref, par, "capsule", g)
    seen = collections.Counter(pr.regions(ref[0], x[hit]))
    print(f"capsule regions among {int(hit.sum())} hit points: {dict(seen)}")
    assert all(seen[k] > 0 for k in ("A", "body", "B")) and 0 < hit.sum() < s.n_IP
    _check_term(s, ref, par, "capsule, -0.0 in rhs_in", g_neg)
    # both together with a plane, a sphere and the container
    s.clear_colliders()
    s.add_plane(**dict(FLOOR, velocity=(0.1, 0.0, 0.0)))
    s.add_sphere(**dict(BALL, velocity=(0.3, 0.0, -0.2)))
    s.add_sphere(**SHELL)
    s.add_box(**TERM_BOX)
    s.add_capsule(**TERM_CAPSULE)
    assert s.collider_types() == [1, 2, 3, 4, 5, 0, 0, 0]
    ref = [plane(FLOOR["point"], FLOOR["normal"], (0.1, 0.0, 0.0)), sphere(BALL["centre"], BALL["radius"], velocity=(0.3, 0.0, -0.2)),
           sphere(SHELL["centre"], SHELL["radius"], inside=True), _ref_box(TERM_BOX), _ref_capsule(TERM_CAPSULE)]
    hit, _ = _check_term(s, ref, par, "all five", g)
    assert 0 < hit.sum()
    _check_term(s, ref, par, "all five, -0.0 in rhs_in", g_neg)
    # a second parameter set: stiff, undamped, frictionless
    kw = dict(stiffness=1.0, damping=0.0, friction=0.0, thickness=0.2)
    s.set_contact_params(**kw)
    _check_term(s, ref, (1.0, 0.0, 0.0, 0.2), f"all five, {kw}", g)
    assert torch.equal(s.rhs_gravity, g)                                                    # the input is left alone


def test_a_capsule_whose_hit_points_clamp_to_its_first_end_gives_the_spheres_bits(small_cloud, small_opt, oracle_runs):
    s, g, _ = _deformed(small_cloud, small_opt, oracle_runs)
    vel, far = (0.3, 0.0, -0.2), (0.0, 0.0, 2.0)
    i = s.add_capsule(BALL["centre"], far, BALL["radius"], velocity=vel)
    cap = pr.capsule(BALL["centre"], far, BALL["radius"], vel)
    hit, x = _check_term(s, [cap], tuple(s._contact_params), "capsule from the ball's centre away from the chair", g)
    assert hit.sum() > 10 and (pr.capsule_s(cap, x[hit]) == 0.0).all()          # every hit point clamps to end A
    out, acc = s._rhs_contact.clone(), s.contact_accel().clone()
    s.remove_collider(i)
    assert s.add_sphere(BALL["centre"], BALL["radius"], velocity=vel) == i
    ball = s._enqueue_contact_rhs(g)
    assert torch.equal(_bits(out), _bits(ball)) and torch.equal(_bits(acc), _bits(s.contact_accel()))
    assert s.contact_count() == int(hit.sum())


# ---------------------------------------------------------------- 7: trajectories
def _run(s, n):
    s.update_force(s.n_IP // 2, FORCE)
    out = []
    for _ in range(n):
        s.stepforward()
        out.append(_disp(s))
    return out


@pytest.mark.parametrize("form", ["cells", "persistent"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_runs, monkeypatch, form):
    if form == "cells":
        monkeypatch.setenv("PN_SIM_FORM", "cells")
    s = _sim(small_cloud, small_opt, persistent=form == "persistent")
    assert s.persistent if form == "persistent" else s.cell_form
    s.enable_contact()
    assert (s.add_box(**UNDER), s.add_capsule(**BESIDE)) == (0, 1)
    got = _run(s, N_TRAJ)
    errs = [rel_err(a, b) for a, b in zip(got, oracle_runs["touched"])]
    print(f"{form} form over a box and beside a capsule vs oracle, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    print(f"points in contact on the oracle: {min(oracle_runs['hits'])}..{max(oracle_runs['hits'])}; on the device in the last substep: {s.contact_count()}")
    for k, e in enumerate(errs):
        assert e < 1e-4, (k, e)
    assert s.contact_count() > 0 and min(oracle_runs["hits"]) > 0          # points do come into contact
    if form == "persistent":
        assert s._coop is not None and not s.persistent_timed_out()


def test_a_wide_box_is_the_floor(small_cloud, small_opt):
    a, b = _sim(small_cloud, small_opt).enable_contact(), _sim(small_cloud, small_opt).enable_contact()
    a.add_plane(**FLOOR)
    b.add_box(**WIDE)
    assert WIDE["centre"][1] + WIDE["half_extents"][1] == pytest.approx(FLOOR["point"][1], abs=1e-15)
    ta, tb = _run(a, N_TRAJ), _run(b, N_TRAJ)
    errs = [rel_err(y, x) for x, y in zip(ta, tb)]
    print("on a wide box vs on the plane of its top face, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < 1e-4 and a.contact_count() == b.contact_count() > 0


# ---------------------------------------------------------------- 8: the harness forms
def _harness(small_opt, small_cloud, ckpt, W=64, draw=False):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_contact()
    h.colliders = [h.sim.add_box(**UNDER), h.sim.add_capsule(**BESIDE)]
    if draw:
        h.draw_colliders(collider_style(types=h.sim.collider_types(), checker=0.2))
    return h


def _raise_box(h):
    h.sim.set_collider(h.colliders[0], half_extents=(0.56, 0.2, 0.5), centre=(-0.04, -0.98, 0.0), velocity=(0.0, 5.0, 0.0))


def test_captured_step_with_a_box_equals_eager_steps(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt, draw=True)
    g = _harness(small_opt, small_cloud, ckpt, draw=True).capture(n_trips=8)
    counts = []
    for f in range(6):
        if f == 3:      # a box moved and resized between two replays is followed without a recapture
            _raise_box(e)
            _raise_box(g)
        want = e.to_host(e.step())
        e.synchronize()
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - want["image"]).max() < 1e-5, f
        assert np.isfinite(b["collider_t"].cpu().numpy()).sum() > 100, f          # the box and the capsule are in the frame
        err = rel_err(_disp(g.sim), _disp(e.sim))
        assert err < 1e-7, (f, err)
        counts.append((e.sim.contact_count(), g.sim.contact_count()))
    print(f"points in contact per frame (eager, captured): {counts}")
    assert all(a == b for a, b in counts) and min(a for a, _ in counts) > 0
    p = _harness(small_opt, small_cloud, ckpt, draw=True)      # without the move the state would be another: the change really acted
    for _ in range(6):
        p.step()
    p.synchronize()
    assert np.abs(_disp(p.sim) - _disp(g.sim)).max() > 1e-4
    assert _state_bytes(g.sim) == g.sim.contact_state_bytes()


def test_captured_step_with_shadows_and_points_on_a_box_equals_the_eager_step(small_opt, small_cloud, ckpt):
    def make():
        h = _harness(small_opt, small_cloud, ckpt, W=48, draw=True)
        h.cast_shadows(direction=(0.2, 1.0, 0.1), resolution=64)
        h.draw_points()
        return h
    e, g = make(), make().capture(n_trips=8)
    for f in range(3):
        want = e.to_host(e.step())
        e.synchronize()
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - want["image"]).max() < 1e-5, f
        sh = b["shadow"].cpu().numpy()
        assert (sh > 0.5).sum() > 0, f          # the box lies in the chair's shadow, or the capsule's


def test_pipelined_frames_with_a_box_equal_eager_steps(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt, draw=True)
    frames = []
    for _ in range(7):
        frames.append(e.to_host(e.step())["image"].copy())
    e.synchronize()
    p = _harness(small_opt, small_cloud, ckpt, draw=True).capture_pipelined(lanes=2, depth=2, n_trips=8)
    got = []
    for f in range(len(frames)):
        for idx, res in p.step_pipelined():
            got.append((idx, res["image"].copy()))
    for idx, res in p.drain_pipeline():
        got.append((idx, res["image"].copy()))
    assert [i for i, _ in got] == list(range(len(frames)))
    for f, (_, img) in enumerate(got):
        assert np.abs(img - frames[f]).max() < 1e-5, f
    for _ in range(p.substeps_enqueued - len(frames)):     # the pipeline's simulator runs ahead of its frames
        e.step()
    e.synchronize()
    err = rel_err(_disp(p.sim), _disp(e.sim))
    print(f"pipelined (lanes 2, depth 2) with a box vs eager after {p.substeps_enqueued} substeps: {err:.2e}; {p.sim.contact_count()} points in contact")
    assert err < 1e-7 and p.sim.contact_count() == e.sim.contact_count() > 0
    plain = _harness(small_opt, small_cloud, ckpt)
    assert np.abs(plain.to_host(plain.step())["image"] - frames[0]).max() > 0.1      # the colliders are in those frames


# ---------------------------------------------------------------- 9: a ball and a box
def test_a_ball_rests_on_a_box_and_another_leaves_it_over_the_edge(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt)
    s.enable_contact().enable_bodies()
    kappa, beta, mu, _ = s._contact_params
    g, dt, R = np.array([0.0, -9.8, 0.0]), s.dt, 0.25
    top = -6.0          # far below the object, which sags by a unit under gravity in these 200 substeps
    table = dict(centre=(0.0, top - 0.5, 0.0), half_extents=(1.0, 0.5, 1.0))
    s.add_box(**table)
    ref = [_ref_box(table)]
    falls = s.add_body((0.0, top + R + 0.02, 0.0), R, 3.0)                        # dropped from a little above the top
    leaves = s.add_body((0.9, top + R, 0.3), R, 2.0, velocity=(1.5, 0.0, 0.0))     # on the top, thrown towards the +x edge at x = 1
    p, u = np.array([0.9, top + R, 0.3]), np.array([1.5, 0.0, 0.0])
    worst = {"centre": 0.0, "velocity": 0.0}
    for k in range(200):
        s.stepforward()
        # pn_body_step's update in numpy: the law at the ball's centre with its radius as the thickness, then the semi-implicit step (no damping)
        a_st, _ = pr.contact_accel(ref, p[None], u[None], dt, kappa, beta, mu, R)
        u = u + dt * (g + a_st[0])
        p = p + dt * u
        if k in (0, 9, 24, 49, 99, 199):
            b = s.body_state()[leaves]
            # measured against the trajectory's own scales: the position's size and the throw's speed (the velocity passes through zero components)
            e_p, e_u = rel_err(b["centre"], p), float(np.abs(b["velocity"] - u).max() / 1.5)
            worst = {"centre": max(worst["centre"], e_p), "velocity": max(worst["velocity"], e_u)}
            print(f"thrown ball after {k + 1} substeps: centre {np.round(b['centre'], 4).tolist()}, rel err centre {e_p:.2e}, velocity {e_u:.2e}")
    # test_gpu_bodies' bar for one step with a static collider against numpy is 1e-12; the law removes the share kappa of a position error per
    # substep in contact and free flight adds none, so the errors of the steps do not pile up: the same bar holds along the trajectory
    assert worst["centre"] < 1e-12 and worst["velocity"] < 1e-12, worst
    assert s.contact_count() == 0 and s.body_clock() == 200          # no object contact
    st = s.body_state()
    b = st[leaves]
    print(f"thrown ball after 200 substeps: centre {b['centre'].tolist()}")
    assert b["centre"][0] > 1.0 and b["centre"][1] < top and not b["reaction"].any()          # it left the top and ended below it
    # at rest the law's push balances gravity: kappa delta / dt^2 = g, delta = g dt^2 / kappa (test_gpu_bodies' ball on a plane, and its bar)
    b = st[falls]
    pen = R - (b["centre"][1] - top)
    print(f"dropped ball after 200 substeps: penetration {pen:.6e} (the law's {9.8 * dt * dt / kappa:.6e}), speed {np.linalg.norm(b['velocity']):.3e}")
    assert abs(pen - 9.8 * dt * dt / kappa) < 1e-6 and np.linalg.norm(b["velocity"]) < 1e-6
    assert abs(b["centre"][0]) < 1e-12 and abs(b["centre"][2]) < 1e-12 and b["clamped"] == 0


# ---------------------------------------------------------------- 10: the drawn frame, bit for bit
RGB = cr.default_rgb()
AMBIENT, DIM = 0.3, 0.5


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare_bits(name, got, want, n_rays):
    keep = ~want.near
    hit = want.slot >= 0
    print(f"{name}: N {n_rays}, hits per slot {np.bincount(want.slot[hit], minlength=8).tolist()}, {int(want.near.sum())} rays masked")
    assert want.near.sum() < 0.01 * max(int(hit.sum()), 1), name
    for k, (a, b) in {"image": (got[0], want.image), "coverage": (got[1], want.coverage), "collider_t": (got[2], want.t)}.items():
        same = (_u32(a) == _u32(b)).reshape(n_rays, -1).all(axis=1)
        assert same[keep].all(), (name, k, int((~same[keep]).sum()), np.nonzero(~same & keep)[0][:8].tolist())
    return hit


@pytest.fixture(scope="module")
def eye_rays():
    return {k: GC._look_at_rays(eye, W=48, H=48) for k, eye in pr.EYES.items()}


@pytest.mark.parametrize("checker", [0.25, 0.0], ids=["checker", "plain"])
@pytest.mark.parametrize("eye", list(pr.EYES))
def test_launch_equals_the_restatement_bit_for_bit(eye, checker, eye_rays):
    cols = pr.mixed_scene()
    assert [None if c is None else c[0] for c in cols] == [1, 2, None, 4, 5, None, None, None]
    o, d = eye_rays[eye]
    N = o.shape[0]
    acc, s, d0 = cr.standard_inputs(N)
    got = GC._launch(GC._state(cols), GC._style(checker=checker, checker_dim=DIM, ambient=AMBIENT), o, d, GC._dev(s), GC._dev(d0), GC._dev(acc),
                     t_min=pr.T_MIN, t_max=pr.T_MAX)
    got = tuple(t.cpu().numpy() for t in got)
    want = pr.draw(cols, RGB, checker, DIM, AMBIENT, o.cpu().numpy(), d.cpu().numpy(), pr.T_MIN, pr.T_MAX, 1.0, s, d0, acc)
    hit = _compare_bits(f"{eye}, checker {checker}", got, want, N)
    if eye == "outside":
        assert (np.bincount(want.slot[hit], minlength=8)[[0, 1, 3, 4]] > 40).all()
    if eye == "inside_box":
        assert (want.slot == 3).all() and (np.bincount(want.face, minlength=3) > 100).all()          # the far faces, all three axes
    if eye == "inside_capsule":
        assert (want.slot[hit] == 4).sum() > 1000


def test_hand_made_rays_bit_for_bit():
    cols = cr.slots(pr.UNIT_BOX, pr.UNIT_CAPSULE)
    rays = pr.hand_rays()
    o = np.array([r[1] for r in rays], np.float32)
    d = np.array([r[2] for r in rays], np.float32)
    N = len(rays)
    z = np.zeros(N, np.float32)
    acc = np.zeros((N, 3), np.float32)
    got = GC._launch(GC._state(cols), GC._style(checker=0.25, checker_dim=DIM, ambient=AMBIENT), GC._dev(o), GC._dev(d), GC._dev(z), GC._dev(z), GC._dev(acc),
                     t_min=pr.T_MIN, t_max=pr.T_MAX)
    got = tuple(t.cpu().numpy() for t in got)
    want = pr.draw(cols, RGB, 0.25, DIM, AMBIENT, o, d, pr.T_MIN, pr.T_MAX, 1.0, z, z, acc)
    assert got[2].tolist() == [2.0, 1.0, 1.0, np.inf, np.inf, 1.5, 2.5, 0.5]          # the exact cases, the graze included
    for a, b in ((got[0], want.image), (got[1], want.coverage), (got[2], want.t)):
        assert np.array_equal(_u32(a), _u32(b))


def test_a_state_of_old_types_keeps_its_bits(eye_rays):
    """Planes, spheres and the container alone: colliders_reference's float32 evaluation, unchanged, on the rays it does not flag."""
    cols = cr.standard_scene()
    S = cr.STANDARD
    o, d = GC._look_at_rays(S["eye"])
    N = o.shape[0]
    acc, s, d0 = cr.standard_inputs(N)
    got = tuple(t.cpu().numpy() for t in GC._launch(GC._state(cols), GC._style(), o, d, GC._dev(s), GC._dev(d0), GC._dev(acc)))
    want = cr.draw(cols, RGB, S["checker"], S["checker_dim"], S["ambient"], o.cpu().numpy(), d.cpu().numpy(), S["t_min"], S["t_max"], S["bg"], s, d0, acc)
    keep = ~want.near
    assert (~keep).sum() <= 0.005 * N
    for k, (a, b) in {"image": (got[0], want.image), "coverage": (got[1], want.coverage), "collider_t": (got[2], want.t)}.items():
        same = (_u32(a) == _u32(b)).reshape(N, -1).all(axis=1)
        assert same[keep].all(), (k, int((~same[keep]).sum()))


# ---------------------------------------------------------------- 11: shadows
LIGHT = (0.2, 1.0, 0.1)          # from above


def _shadow_case(cols, spheres, eye_rays, res=32, strength=0.6):
    o, d = eye_rays["outside"]
    N = o.shape[0]
    acc, s, d0 = cr.standard_inputs(N)
    lt = shadow_light(direction=LIGHT, strength=strength, resolution=res, bound=1.0, min_near=pr.T_MIN, spheres=spheres)
    ws, wd = sr.synthetic_maps(res)
    style = GC._style(checker=0.25, checker_dim=DIM, ambient=AMBIENT)
    got = GS._launch(GC._state(cols), style, o, d, GC._dev(s), GC._dev(d0), GC._dev(acc), lt, GC._dev(ws), GC._dev(wd), t_min=pr.T_MIN, t_max=pr.T_MAX)
    got = tuple(t.cpu().numpy() for t in got)
    args = (cols, RGB, 0.25, DIM, AMBIENT, o.cpu().numpy(), d.cpu().numpy(), pr.T_MIN, pr.T_MAX, 1.0, s, d0, acc)
    return got, args, GS._light_dict(lt), ws, wd, N


@pytest.mark.parametrize("spheres", [True, False], ids=["casters", "no_casters"])
def test_shadowed_launch_equals_the_restatement_bit_for_bit(spheres, eye_rays):
    cols = pr.mixed_scene()
    got, args, lt, ws, wd, N = _shadow_case(cols, spheres, eye_rays)
    want = pr.draw(*args, lt=lt, shadow_ws=ws, shadow_depth_0=wd)
    _compare_bits(f"shadowed, spheres {spheres}", got[:3], want, N)
    keep = ~want.near
    assert np.array_equal(_u32(got[3])[keep], _u32(want.occ)[keep])
    # what the new casters add: the floor under the box and the capsule is dark where the map alone leaves it lit
    floor = keep & (want.slot == 0)
    lt_off = dict(lt, spheres=0)
    alone = pr.draw(*args, lt=lt_off, shadow_ws=ws, shadow_depth_0=wd)
    added = floor & (want.occ == 1.0) & (alone.occ < 1.0)
    print(f"spheres {spheres}: {int(floor.sum())} floor rays, {int(added.sum())} of them darkened by the box, the capsule or the sphere alone")
    if spheres:
        only_new = pr.draw(*((cr.slots(cols[0], None, None, cols[3], cols[4]),) + args[1:]), lt=lt, shadow_ws=ws, shadow_depth_0=wd)
        new = floor & (only_new.slot == 0) & (only_new.occ == 1.0) & (alone.occ < 1.0)
        assert new.sum() > 20          # the box and the capsule cast, not just the sphere
        assert added.sum() >= new.sum()
    else:
        assert added.sum() == 0 and np.array_equal(_u32(want.occ), _u32(alone.occ))          # spheres = 0 switches the new casters off too


def test_a_shadowed_state_of_old_types_keeps_its_bits(eye_rays):
    cols = cr.standard_scene()
    got, args, lt, ws, wd, N = _shadow_case(cols, True, eye_rays)
    want = sr.draw(*args, lt, ws, wd)          # shadows_reference, unchanged
    keep = ~want.near
    assert (~keep).sum() <= GS.MAX_FLAGGED * N and (want.occ > 0).sum() > 50
    for k, (a, b) in {"image": (got[0], want.image), "coverage": (got[1], want.coverage), "collider_t": (got[2], want.t), "shadow": (got[3], want.occ)}.items():
        same = (_u32(a) == _u32(b)).reshape(N, -1).all(axis=1)
        assert same[keep].all(), (k, int((~same[keep]).sum()))


# ---------------------------------------------------------------- 12: main_render end to end
def test_main_render_drops_the_chair_onto_a_box_beside_a_capsule(tmp_path, small_cloud, capsys):
    """The lowest integration points start at y = -0.86, so with the box's top at y = -0.95 the contact thickness is given as 0.1: the box carries them
    from the first frame (test_gpu_contact's floor)."""
    from pienerf_amd import io, main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--unpin", "--frames", "6",
            "--collide_box", "0", "-1.05", "0", "0.7", "0.1", "0.7", "--collide_capsule", "0.8", "-0.9", "-0.5", "0.8", "0.3", "0.5", "0.1",
            "--contact_thickness", "0.1", "--draw_points"]
    drawn = ["--draw_colliders", "--shadows", "--shadow_res", "64"]
    a = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "plain")]))
    capsys.readouterr()
    b = main_render.run(main_render.parser().parse_args(base + drawn + ["--out", str(tmp_path / "drawn")]))
    said = capsys.readouterr().out
    assert [f.split("/")[-1] for f in b] == [f"img_{f}.png" for f in range(6)] and len(a) == 6          # the PNGs are written
    m = re.search(r"contact: (\d+) of (\d+) integration points", said)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 432, said          # contact_count() > 0 by the last frame
    # the same frames through the same calls, for their collider_t
    args = main_render.parser().parse_args(base + drawn + ["--out", str(tmp_path / "unused")])
    h = main_render.build_harness(args)
    main_render.configure_contact(h.sim, args)
    main_render.configure_overlay(h, args)
    main_render.configure_points(h, args)
    assert h.sim.collider_types() == [4, 5, 0, 0, 0, 0, 0, 0]
    pose = scene.orbit_pose(args.radius, args.azimuth, args.elevation)
    for pa, pb in zip(a, b):
        ct = h.step(pose=pose)["collider_t"].reshape(48, 48).cpu().numpy()
        ia, ib = io.load_image(pa).numpy(), io.load_image(pb).numpy()
        differ = (ia != ib).any(axis=2)
        # from 5 units away at 48 pixels the box's front face (1.4 x 0.2) covers about 14 x 2 pixels and the rod (0.2 x 1.4) about 2 x 14
        assert np.isfinite(ct).sum() > 40 and differ.sum() > 40          # the box is visible
        assert not differ[~np.isfinite(ct)].any()                           # ... and nothing else changed
    h.synchronize()
    assert h.sim.contact_count() > 0
    for t in (h.sim.dof, h.sim.dof_vel):
        assert bool(torch.isfinite(t).all())
    assert _state_bytes(h.sim) == h.sim.contact_state_bytes()
