"""Contact with planes and spheres on the GPU (csrc/pn_contact.hip; Simulator.enable_contact / add_plane / add_sphere / set_collider ...; main_render
--floor / --unpin): the launch's accel_out and right-hand-side term against the numpy restatement (tests/contact_reference.py), trajectories against the
CPU oracle whose public rhs_gravity is set to g0 + term(state) before every stepforward(), in the three substep forms, with the kinematic pins, and in
the harness forms (eager, captured step, pipelined)."""
import re

import numpy as np
import pytest
import torch

from conftest import make_oracle_sim, rel_err
from contact_reference import OracleContact, contact_accel, contact_term, ip_state, plane, sphere
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
from test_gpu_parity import DEV
from test_pins_host import oracle_pins, pin_term, pin_u

pytestmark = pytest.mark.gpu

FORCE = np.array([300.0, 100.0, -200.0])            # conftest's pick force, on IP n_IP // 2
FLOOR = dict(point=(0.0, -0.83, 0.0), normal=(0.0, 1.0, 0.0))
BALL = dict(centre=(0.0, 0.0, 0.9), radius=0.5)
SHELL = dict(centre=(0.0, 0.0, 0.0), radius=0.98, inside=True)
THREE_REF = [plane(FLOOR["point"], FLOOR["normal"]), sphere(BALL["centre"], BALL["radius"]), sphere(SHELL["centre"], SHELL["radius"], inside=True)]
SHAKE = ((0.05, 0.02, -0.03), 4.0, 0.3)
N_TRAJ, N_BOTH = 24, 12


def _sim(cloud, opt, persistent=False, dx=None):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=dx or opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV, persistent=persistent)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def _three(s):
    s.enable_contact()
    return [s.add_plane(**FLOOR), s.add_sphere(**BALL), s.add_sphere(**SHELL)]


def _disp(s):
    return (s.dof - s.dof_rest).cpu().numpy().reshape(-1, 3)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.fixture(scope="module")
def oracle_runs(small_cloud, small_opt):
    """Computed once: the oracle under gravity and the pick force for 24 substeps without contact (its dof / dof_vel after 12 of them: the deformed,
    moving state of the term test) and with the three colliders at the defaults; 12 substeps with shaken pins and the colliders together."""
    plain = OracleContact(make_oracle_sim(small_cloud, small_opt), [])
    plain.ref.update_force(plain.ref.n_IP // 2, FORCE)
    free = []
    for k in range(N_TRAJ):
        free.append(plain.step().copy())
        if k == 11:
            state12 = (plain.ref.dof.copy(), plain.ref.dof_vel.copy())
    con = OracleContact(make_oracle_sim(small_cloud, small_opt), THREE_REF)
    con.ref.update_force(con.ref.n_IP // 2, FORCE)
    touched, hits = [], []
    for _ in range(N_TRAJ):
        touched.append(con.step().copy())
        hits.append(con.hits)
    ref = make_oracle_sim(small_cloud, small_opt)
    _, kern, Nx, X = oracle_pins(ref)
    both = OracleContact(ref, THREE_REF, extra=lambda k: pin_term(ref.n_k, ref.stiff, kern, Nx, pin_u(X, (k + 1) * ref.dt, translate=SHAKE)))
    shaken = [both.step().copy() for _ in range(N_BOTH)]
    return dict(free=free, state12=state12, touched=touched, hits=hits, shaken=shaken)


# ---------------------------------------------------------------- 1: accel_out and rhs_out - rhs_in against numpy
def _numpy_term(s, colliders, par):
    topo, Nx = s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy()
    x, v = ip_state(topo, Nx, s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    a, hit = contact_accel(colliders, x, v, s.dt, *par)
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    return contact_term(s.n_k, topo, Nx, m, a), a, hit


def _check_term(s, colliders, par, name, g):
    """One launch against numpy; two launches, equal bits; rows of kernels without a contacting point carry rhs_in's bits.  Returns the hit count."""
    want, a, hit = _numpy_term(s, colliders, par)
    out = s._enqueue_contact_rhs(g).clone()
    acc = s.contact_accel().clone()
    again = s._enqueue_contact_rhs(g)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(acc), _bits(s.contact_accel())), name     # two runs, equal bits
    s.contact_accel().fill_(7.0)
    one = s._enqueue_contact_rhs(g, one_launch=True)      # the one-launch form: every entry evaluates its point itself.  The same bits, accel left alone
    assert torch.equal(_bits(out), _bits(one)) and bool((s.contact_accel() == 7.0).all()), name
    s._enqueue_contact_rhs(g)
    got = (out - g).cpu().numpy().reshape(-1, 3)
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err(got, want)
    print(f"{name}: {int(hit.sum())} of {s.n_IP} points in contact, max|term| {np.abs(want).max():.3e}, rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert np.abs(want).max() > 1.0, name          # so the bar means something
    assert e_a < 1e-12 and e_t < 1e-12, (name, e_a, e_t)
    assert s.contact_count() == int(hit.sum()), name
    assert np.array_equal(acc.cpu().numpy()[~hit], np.zeros((int((~hit).sum()), 3)))
    untouched = np.ones(s.n_k, bool)
    untouched[np.unique(s.IP_kernel.cpu().numpy()[hit])] = False
    rows = torch.from_numpy(np.repeat(untouched, 30)).to(DEV)
    assert torch.equal(_bits(out[rows]), _bits(g[rows])), name
    return int(hit.sum()), int(untouched.sum())


def test_term_equals_the_numpy_term(small_cloud, small_opt, oracle_runs):
    s = _sim(small_cloud, small_opt).enable_contact()
    runs = s.kernel_cnt.cpu().numpy()
    long_runs = runs[runs > 64]
    print(f"n_IP {s.n_IP}, n_k {s.n_k}: runs of {runs.min()}..{runs.max()} entries, {len(long_runs)} longer than 64: {sorted(long_runs.tolist())}")
    assert (s.n_IP, s.n_k) == (432, 139) and runs.min() == 1 and runs.max() == 84 and runs.sum() == 8 * s.n_IP
    assert len(long_runs) == 9 and (long_runs % 64 != 0).all()      # more than one wave of the workgroup, ragged remainders
    dof, vel = oracle_runs["state12"]
    s.dof.copy_(torch.from_numpy(dof.reshape(-1)))
    s.dof_vel.copy_(torch.from_numpy(vel.reshape(-1)))
    assert np.abs(dof - s.dof_rest.cpu().numpy().reshape(-1, 3)).max() > 1e-2 and np.abs(vel).max() > 1e-2     # deformed and moving
    g = s.rhs_gravity.clone()
    # -0.0 entries in rhs_in: a copied row must keep them (g + 0.0 would not)
    g_neg = g.clone()
    g_neg[g_neg == 0.0] = -0.0
    assert int((g_neg == 0.0).sum()) > 100 and bool(torch.signbit(g_neg[g_neg == 0.0]).all())
    par = tuple(s._contact_params)
    assert par == (0.5, 0.5, 0.5, 0.05)
    # moving colliders, a tilted floor: every component of w and of the normal is in play
    sets = {"plane": ([dict(point=(0.0, -0.8, 0.0), normal=(0.2, 1.0, -0.1), velocity=(0.0, 0.5, 0.1))], None),
            "sphere": (None, [dict(BALL, velocity=(0.3, 0.0, -0.2))]),
            "container": (None, [dict(SHELL, velocity=(0.0, 0.1, 0.0))]),
            "all three": ([dict(FLOOR, velocity=(0.1, 0.0, 0.0))], [dict(BALL, velocity=(0.3, 0.0, -0.2)), SHELL])}
    for name, (planes, spheres) in sets.items():
        s.clear_colliders()
        ref = []
        for p in planes or []:
            s.add_plane(**p)
            ref.append(plane(p["point"], p["normal"], p.get("velocity", (0, 0, 0))))
        for q in spheres or []:
            s.add_sphere(**q)
            ref.append(sphere(q["centre"], q["radius"], q.get("inside", False), q.get("velocity", (0, 0, 0))))
        n_hit, n_free = _check_term(s, ref, par, name, g)
        assert 0 < n_hit < s.n_IP and n_free > 0, name
        _check_term(s, ref, par, name + ", -0.0 in rhs_in", g_neg)
        # the device state is what the mirror says it is
        assert bytes(s._contact_state.view(torch.uint8).cpu().numpy().tobytes()) == s.contact_state_bytes()
    # other parameters: stiff, undamped, frictionless / sticky
    for kw in (dict(stiffness=1.0, damping=0.0, friction=0.0, thickness=0.02), dict(stiffness=1.0, damping=1.0, friction=2.0, thickness=0.08)):
        s.set_contact_params(**kw)
        _check_term(s, ref, (kw["stiffness"], kw["damping"], kw["friction"], kw["thickness"]), f"all three, {kw}", g)
    s.set_contact_params(0.5, 0.5, 0.5, 0.05)
    assert torch.equal(s.rhs_gravity, g)                                                    # the input is left alone
    # a container of R = 0.1 puts every point in contact
    s.clear_colliders()
    s.add_sphere((0.0, 0.0, 0.0), 0.1, inside=True)
    n_hit, n_free = _check_term(s, [sphere((0.0, 0.0, 0.0), 0.1, inside=True)], par, "container R = 0.1", g)
    assert n_hit == s.n_IP == 432 and n_free == 0
    # a floor at y = -2 puts none in contact: the whole vector is rhs_in's bits, -0.0 included
    s.clear_colliders()
    i = s.add_plane((0.0, -2.0, 0.0), (0.0, 1.0, 0.0))
    for gin in (g, g_neg):
        out = s._enqueue_contact_rhs(gin)
        assert torch.equal(_bits(out), _bits(gin)) and s.contact_count() == 0 and not bool(s.contact_accel().any())
    # ... and so it is after clear_colliders() (n = 0), with a collider in reach before
    s.set_collider(i, point=(0.0, -0.8, 0.0))
    out = s._enqueue_contact_rhs(g_neg)
    assert not torch.equal(_bits(out), _bits(g_neg)) and s.contact_count() > 0
    s.clear_colliders()
    out = s._enqueue_contact_rhs(g_neg)
    assert torch.equal(_bits(out), _bits(g_neg)) and s.contact_count() == 0 and not bool(s.contact_accel().any())
    plain = _sim(small_cloud, small_opt)
    assert plain.Nx_csr is None and plain._contact_state is None and not plain.contact_enabled   # the tables exist only with the feature on


def test_term_on_runs_longer_than_the_workgroup(small_opt):
    """A 4 080-point chair at half the cell size: 3 047 integration points on the same 139 kernels, so runs of up to 770 entries — four passes of the
    256-thread workgroup, all four waves busy, ragged last passes — beside runs of 4.  The state is the rest state plus seeded noise: the term's
    restatement needs no physics."""
    cloud = scene.make_chair_points(sub_res=45, hgs=small_opt["hash_grid_size"])
    s = _sim(cloud, small_opt, dx=0.05).enable_contact()
    runs = s.kernel_cnt.cpu().numpy()
    print(f"dx 0.05: n_IP {s.n_IP}, n_k {s.n_k}, runs of {runs.min()}..{runs.max()} entries, {(runs > 256).sum()} longer than 256")
    assert s.n_k == 139 and runs.max() > 768 and (runs[runs > 256] % 256 != 0).all() and (runs < 64).any()
    rng = np.random.default_rng(11)
    s.dof.add_(torch.from_numpy(rng.normal(scale=0.01, size=s.dof.numel())).to(DEV))
    s.dof_vel.copy_(torch.from_numpy(rng.normal(scale=0.5, size=s.dof.numel())).to(DEV))
    s.add_plane(point=(0.0, -0.8, 0.0), normal=(0.2, 1.0, -0.1), velocity=(0.0, 0.5, 0.1))
    s.add_sphere(**dict(BALL, velocity=(0.3, 0.0, -0.2)))
    s.add_sphere(**SHELL)
    ref = [plane((0.0, -0.8, 0.0), (0.2, 1.0, -0.1), (0.0, 0.5, 0.1)), sphere(BALL["centre"], BALL["radius"], velocity=(0.3, 0.0, -0.2)), THREE_REF[2]]
    n_hit, n_free = _check_term(s, ref, tuple(s._contact_params), "dx 0.05, all three", s.rhs_gravity.clone())
    assert s._contact_params[3] == 0.025 and 0 < n_hit < s.n_IP


# ---------------------------------------------------------------- 2: trajectories against the oracle, cell and CSR forms
def _run(s, n, contact=True):
    if contact:
        _three(s)
    s.update_force(s.n_IP // 2, FORCE)
    out = []
    for _ in range(n):
        s.stepforward()
        out.append(_disp(s))
    return out


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_runs, monkeypatch, form):
    monkeypatch.setenv("PN_SIM_FORM", form)
    s = _sim(small_cloud, small_opt)
    assert s.cell_form == (form == "cells")
    got = _run(s, N_TRAJ)
    errs = [rel_err(a, b) for a, b in zip(got, oracle_runs["touched"])]
    print(f"{form} form with three colliders vs oracle, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    print(f"points in contact on the oracle: {min(oracle_runs['hits'])}..{max(oracle_runs['hits'])}; on the device in the last substep: {s.contact_count()}")
    for k, e in enumerate(errs):
        assert e < 1e-4, (k, e)
    assert s.contact_count() > 0 and min(oracle_runs["hits"]) > 0
    diff = float(np.abs(got[-1] - oracle_runs["free"][-1]).max())
    print(f"last state vs a run without contact: max abs difference {diff:.3e}")
    assert diff > 1e-3      # the colliders really moved it


# ---------------------------------------------------------------- 3: the persistent form against the cell form
def test_persistent_form_matches_the_cell_form(small_cloud, small_opt):
    def gap(contact):
        a, b = _sim(small_cloud, small_opt, False), _sim(small_cloud, small_opt, True)
        ta, tb = _run(a, N_TRAJ, contact), _run(b, N_TRAJ, contact)
        assert b.persistent and b._coop is not None and not b.persistent_timed_out() and a.cell_form
        return max(rel_err(y, x) for x, y in zip(ta, tb))
    g0 = gap(False)      # both forms are the substep's own code here: their gap without contact
    g1 = gap(True)
    print(f"persistent vs cell form over {N_TRAJ} substeps: gap {g0:.2e} without contact, {g1:.2e} with the three colliders")
    assert g1 <= max(1e-8, 20.0 * g0)


# ---------------------------------------------------------------- 4: pins and contact together
def test_pins_and_contact_together_match_the_oracle(small_cloud, small_opt, oracle_runs):
    s = _sim(small_cloud, small_opt)
    s.enable_pin_motion()
    s.set_pin_motion(translate=SHAKE)
    _three(s)
    errs = []
    for k in range(N_BOTH):
        s.stepforward()
        errs.append(rel_err(_disp(s), oracle_runs["shaken"][k]))
    print("shaken pins and three colliders vs oracle, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    for k, e in enumerate(errs):
        assert e < 1e-4, (k, e)
    assert s.pin_clock() == N_BOTH and s.contact_count() > 0
    assert not torch.equal(s._rhs_ext, s.rhs_gravity) and not torch.equal(s._rhs_contact, s._rhs_ext)   # gravity -> pins -> contact: three buffers


# ---------------------------------------------------------------- 5: the harness forms
def _harness(small_opt, small_cloud, ckpt, W=64):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.colliders = _three(h.sim)
    return h


def _raise_floor(h):
    h.sim.set_collider(h.colliders[0], point=(0.0, -0.78, 0.0), velocity=(0.0, 5.0, 0.0))


def test_captured_step_with_contact_equals_eager_steps(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt)
    g = _harness(small_opt, small_cloud, ckpt).capture(n_trips=8)
    assert torch.equal(g.sim.dof, g.sim.dof_rest)   # capture's warm-up steps left the state where it was
    counts = []
    for f in range(6):
        if f == 3:      # a floor raised between two replays is followed without a recapture
            _raise_floor(e)
            _raise_floor(g)
        want = e.to_host(e.step())
        e.synchronize()
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - want["image"]).max() < 1e-5, f
        err = rel_err(_disp(g.sim), _disp(e.sim))
        assert err < 1e-7, (f, err)
        counts.append((e.sim.contact_count(), g.sim.contact_count()))
    print(f"points in contact per frame (eager, captured): {counts}")
    assert all(a == b for a, b in counts) and min(a for a, _ in counts) > 0
    # without the raise the state would be another: the change really acted
    p = _harness(small_opt, small_cloud, ckpt)
    for _ in range(6):
        p.step()
    p.synchronize()
    assert np.abs(_disp(p.sim) - _disp(g.sim)).max() > 1e-4
    # a graph captured without the contact launch refuses to run once contact is enabled
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=8)
    plain.step_graph()
    plain.finish_graph_frame()
    plain.sim.enable_contact()
    with pytest.raises(RuntimeError, match="captured before enable_contact"):
        plain.step_graph()


def test_pipelined_frames_with_contact_equal_eager_steps(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt)
    frames = []
    for _ in range(7):
        frames.append(e.to_host(e.step())["image"].copy())
    e.synchronize()
    p = _harness(small_opt, small_cloud, ckpt).capture_pipelined(lanes=2, depth=2, n_trips=8)
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
    print(f"pipelined (lanes 2, depth 2) with contact vs eager after {p.substeps_enqueued} substeps: {err:.2e}; {p.sim.contact_count()} points in contact")
    assert err < 1e-7 and p.sim.contact_count() == e.sim.contact_count() > 0
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).capture_pipelined(lanes=2, depth=2, n_trips=8)
    plain.step_pipelined()
    plain.drain_pipeline()
    plain.sim.enable_contact()
    with pytest.raises(RuntimeError, match="captured before enable_contact"):
        plain.step_pipelined()


# ---------------------------------------------------------------- 6: main_render --unpin --floor
def test_main_render_drops_the_chair_onto_a_floor(tmp_path, small_cloud, capsys):
    """--unpin --floor -0.95 --frames 3 --save_ply.  The lowest integration points start at y = -0.86 and fall 0.006 in three substeps, so the contact
    thickness is given as 0.1 (contact from y < -0.85): the floor carries them from the first frame."""
    from pienerf_amd import main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    args = main_render.parser().parse_args(["--ply", str(tmp_path / "chair.ply"), "--out", str(tmp_path / "out"), "--W", "48", "--H", "48", "--sim_dx", "0.1",
                                            "--sim_iters", "4", "--unpin", "--floor", "-0.95", "--contact_thickness", "0.1", "--frames", "3", "--save_ply"])
    files = main_render.run(args)
    assert [f.split("/")[-1] for f in files] == [f"img_{f}.png" for f in range(3)]
    said = capsys.readouterr().out
    m = re.search(r"contact: (\d+) of (\d+) integration points", said)
    assert m, said
    print(m.group(0))
    assert int(m.group(1)) > 0 and int(m.group(2)) == 432      # contact_count() > 0
    # nothing holds the chair: points_2.ply lies below the cloud, by less than free fall (the floor pushes back)
    y0 = np.asarray(small_cloud["pos"], np.float64)[:, 1]
    pts = scene.read_ply(str(tmp_path / "out" / "points_2.ply"))
    drop = y0 - np.asarray(pts["y"], np.float64)
    print(f"points_2.ply: the points fell by {drop.min():.5f}..{drop.max():.5f}")
    assert drop.max() > 1e-3 and drop.min() > -0.05
