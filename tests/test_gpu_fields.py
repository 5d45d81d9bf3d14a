"""Force fields on the GPU (csrc/pn_fields.hip; Simulator.enable_fields / add_wind / add_air_drag / add_vortex / add_radial / set_field ...; main_render
--wind / --air_drag): the launches' accel_out and right-hand-side term against the numpy restatement (tests/fields_reference.py), on the small chair and
on synthetic tables that run the stride loop and all four waves; the bit copies; the clock; trajectories against the CPU oracle whose public rhs_gravity
is set to g0 + [pins + contact +] term(state, k dt) before every stepforward(), in the cell and CSR forms; and the harness forms (eager, captured step,
pipelined)."""
import numpy as np
import pytest
import torch

from conftest import make_oracle_sim, rel_err
from contact_reference import contact_term, ip_state, oracle_term, plane, sphere
from fields_reference import OracleFields, field_accel, radial, vortex, wind
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
from test_gpu_parity import DEV
from test_pins_host import oracle_pins, pin_term, pin_u

pytestmark = pytest.mark.gpu

GUSTY = dict(velocity=(5.0, 1.0, -2.0), drag=3.0, gust=0.6, hz=2.0, phase=0.4, wave=(0.5, 0.0, 0.25), origin=(0.1, 0.0, -0.2))
SWIRL = dict(point=(0.1, 0.0, -0.1), axis=(0.2, 1.0, -0.1), omega=6.0, radius=0.8, drag=4.0)
BLAST = dict(centre=(0.2, -0.3, 0.1), strength=400.0, radius=0.9)
MAKE = {"wind": wind, "vortex": vortex, "radial": radial}
K0, K1 = 5, 9            # the windowed cases act while K0 dt <= t < K1 dt
N_TRAJ = 20


def _sim(cloud, opt):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV, persistent=False)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def _add(s, kind, kw):
    return {"wind": s.add_wind, "vortex": s.add_vortex, "radial": s.add_radial}[kind](**kw)


def _disp(s):
    return (s.dof - s.dof_rest).cpu().numpy().reshape(-1, 3)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _neg_zeros(g):
    """g with every zero turned into -0.0: a copied row must keep them (g + 0.0 would not)."""
    g = g.clone()
    g[g == 0.0] = -0.0
    assert int((g == 0.0).sum()) > 100 and bool(torch.signbit(g[g == 0.0]).all())
    return g


def _device_state_bytes(s):
    return bytes(s._field_state.view(torch.uint8).cpu().numpy().tobytes())


# ---------------------------------------------------------------- 1: accel_out and rhs_out - rhs_in against numpy, on the small chair
def _numpy_term(s, fields, k):
    topo, Nx = s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy()
    x, v = ip_state(topo, Nx, s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    a = field_accel(fields, x, v, k * s.dt, s.dt)
    return contact_term(s.n_k, topo, Nx, (s.IP_rho * s.dx ** 3).cpu().numpy(), a), a


def _check_term(s, fields, k, g, name):
    """One substep's launches at clock k against numpy; where the reference adds nothing, rhs_in's bits.  Returns whether anything was added."""
    want, a = _numpy_term(s, fields, k)
    s.reset_field_clock(k)
    out = s._enqueue_fields_rhs(g).clone()
    acc = s.field_accel().clone()
    assert s.field_clock() == k + 1, name
    s.reset_field_clock(k)
    again = s._enqueue_fields_rhs(g)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(acc), _bits(s.field_accel())), name     # two runs, equal bits
    if not want.any():
        assert not a.any() and not bool(acc.any()) and torch.equal(_bits(out), _bits(g)), name                 # nothing acts: rhs_in, bit for bit
        print(f"{name}, k = {k}: outside every window, rhs_in's bits")
        return False
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err((out - g).cpu().numpy().reshape(-1, 3), want)
    print(f"{name}, k = {k}: max|accel| {np.abs(a).max():.3e}, max|term| {np.abs(want).max():.3e}, rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert np.abs(want).max() > 1.0, (name, k)          # so the bar means something
    assert e_a < 1e-12 and e_t < 1e-12, (name, k, e_a, e_t)
    idle = ~a.any(axis=1)                               # kernels none of whose points has a != 0 carry rhs_in's bits
    untouched = np.ones(s.n_k, bool)
    untouched[np.unique(s.IP_kernel.cpu().numpy()[~idle])] = False
    rows = torch.from_numpy(np.repeat(untouched, 30)).to(DEV)
    assert torch.equal(_bits(out[rows]), _bits(g[rows])), name
    return True


def test_term_equals_the_numpy_term(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt).enable_fields()
    runs = s.kernel_cnt.cpu().numpy()
    assert (s.n_IP, s.n_k) == (432, 139) and runs.min() == 1 and runs.max() == 84
    rng = np.random.default_rng(7)
    s.dof.add_(torch.from_numpy(rng.normal(scale=0.01, size=s.dof.numel())).to(DEV))         # a perturbed state with random velocities
    s.dof_vel.copy_(torch.from_numpy(rng.normal(scale=0.5, size=s.dof.numel())).to(DEV))
    g = s.rhs_gravity.clone()
    g_neg = _neg_zeros(g)
    assert K0 * s.dt == float(np.float64(K0) * np.float64(s.dt))                             # the device's t = (double)k * dt is the host's K0 * dt
    for kind, kw in (("wind", GUSTY), ("vortex", SWIRL), ("radial", BLAST)):
        # open for ever: k = 0 and a later substep
        s.clear_fields()
        _add(s, kind, kw)
        ref = [MAKE[kind](**kw)]
        for k in (0, 37):
            assert _check_term(s, ref, k, g, kind)
        # with a window: before it, at k dt == t0 exactly, inside, at t1, one step past t1
        win = dict(kw, start=K0 * s.dt, stop=K1 * s.dt)
        s.set_field(0, start=win["start"], stop=win["stop"])
        ref = [MAKE[kind](**win)]
        acted = [_check_term(s, ref, k, g_neg, kind + " in a window") for k in (0, K0 - 1, K0, K1 - 1, K1, K1 + 1)]
        assert acted == [False, False, True, True, False, False], (kind, acted)
        assert _device_state_bytes(s) == s.field_state_bytes(k=K1 + 2)                       # the device state is what the mirror says it is
    # all three together, a gap slot between them: wind for ever, vortex and blast in the window
    s.clear_fields()
    specs = [("wind", GUSTY), ("radial", BLAST), ("vortex", dict(SWIRL, start=K0 * s.dt, stop=K1 * s.dt)), ("radial", dict(BLAST, start=K0 * s.dt, stop=K1 * s.dt))]
    ids = [_add(s, kind, kw) for kind, kw in specs]
    s.remove_field(ids[1])
    ref = [MAKE[kind](**kw) for kind, kw in specs]
    ref[1] = None
    assert s.field_types() == [1, 0, 2, 3, 0, 0, 0, 0]
    for gin in (g, g_neg):
        for k in (0, K0, K1 + 1):
            assert _check_term(s, ref, k, gin, "all three with a gap slot")
    assert _device_state_bytes(s) == s.field_state_bytes(k=K1 + 2)
    # the clamps: c = 1e9 acts as c = 1 / dt, a blast of 1e12 as R / (2 dt^2)
    s.clear_fields()
    s.add_air_drag(1e9)
    s.add_radial(BLAST["centre"], -1e12, BLAST["radius"])
    assert _check_term(s, [wind((0, 0, 0), drag=1e9), radial(BLAST["centre"], -1e12, BLAST["radius"])], 3, g, "clamped drag and blast")
    out = s._enqueue_fields_rhs(g).clone()
    s.set_field(0, drag=1.0 / s.dt)
    s.set_field(1, strength=-BLAST["radius"] / (2.0 * s.dt * s.dt))
    assert torch.equal(_bits(out), _bits(s._enqueue_fields_rhs(g)))
    assert torch.equal(s.rhs_gravity, g)                                                     # the input is left alone
    plain = _sim(small_cloud, small_opt)
    assert plain.Nx_csr is None and plain._field_state is None and not plain.fields_enabled  # the tables exist only with the feature on


# ---------------------------------------------------------------- 2: synthetic tables: the stride loop and all four waves
def test_term_on_a_run_longer_than_two_passes_of_the_workgroup():
    """n_k = 3, n_IP = 76: points 0..74 have all 8 slots on kernel 0 (600 entries: more than 2 x 256 and not a multiple of 64), point 75 has all 8 on
    kernel 2, kernel 1 is empty.  The library is called on these tables directly; the restatement needs no physics."""
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    from pienerf_amd.simulator import solver
    n_k, n_IP, dt, dx = 3, 76, 1e-2, 0.1
    rng = np.random.default_rng(21)
    topo = np.zeros((n_IP, 8), np.int32)
    topo[75] = 2
    Nx = rng.normal(scale=0.4, size=(n_IP, 8, 10))
    dof, vel = rng.normal(scale=0.3, size=n_k * 30), rng.normal(scale=0.5, size=n_k * 30)
    rho = rng.uniform(500.0, 1500.0, size=n_IP)
    order = np.argsort(topo.reshape(-1), kind="stable").astype(np.int32)                    # entry = point 8 + slot, by kernel
    cnt = np.bincount(topo.reshape(-1), minlength=n_k).astype(np.int32)
    bg = (np.cumsum(cnt) - cnt).astype(np.int32)
    assert cnt.tolist() == [600, 0, 8] and bg.tolist() == [0, 600, 600] and 600 > 2 * 256 and 600 % 64 != 0
    g = rng.normal(size=n_k * 30)
    g[rng.random(g.size) < 0.2] = -0.0
    fs = [solver.field_wind(**GUSTY), None, solver.field_vortex(**SWIRL), solver.field_radial(**BLAST)] + [None] * 4
    ref = [wind(**GUSTY), None, vortex(**SWIRL), radial(**BLAST)]
    k = 11
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    state = dev(np.frombuffer(solver.pack_field_state(1, fs, k=k), np.float64).copy())
    t = dict(dof=dev(dof), vel=dev(vel), topo=dev(topo), rho=dev(rho), Nx=dev(Nx), bg=dev(bg), cnt=dev(cnt), buf=dev(order), csr=dev(Nx.reshape(-1, 10)[order]),
             g=dev(g))
    out, acc = torch.full_like(t["g"], 7.0), torch.full((n_IP, 3), 7.0, dtype=torch.float64, device=DEV)

    def launch(o):
        check(lib().pn_sim_fields_rhs(n_k, n_IP, ptr(state), dt, dx, ptr(t["dof"]), ptr(t["vel"]), ptr(t["topo"]), ptr(t["rho"]), ptr(t["Nx"]), ptr(t["bg"]),
                                      ptr(t["cnt"]), ptr(t["buf"]), ptr(t["csr"]), ptr(t["g"]), ptr(o), ptr(acc), stream_ptr()), "sim_fields_rhs")
    launch(out)
    x, v = ip_state(topo, Nx, dof, vel)
    a = field_accel(ref, x, v, k * dt, dt)
    want = contact_term(n_k, topo, Nx, rho * dx ** 3, a)
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err((out - t["g"]).cpu().numpy().reshape(-1, 3), want)
    print(f"600-entry run: max|term| {np.abs(want).max():.3e}, rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert np.abs(want).max() > 1.0 and np.abs(want[20:30]).max() > 1e-3 * np.abs(want).max()      # kernel 2's rows carry a term too
    assert e_a < 1e-12 and e_t < 1e-12
    assert torch.equal(_bits(out[30:60]), _bits(t["g"][30:60])) and bool(torch.signbit(out[30:60][out[30:60] == 0.0]).all())   # the empty kernel: rhs_in, bit for bit
    assert int(state[:1].view(torch.int64)[0].item()) == k + 1
    check(lib().pn_sim_fields_clock(ptr(state), k, stream_ptr()), "sim_fields_clock")
    again = torch.full_like(out, 3.0)
    launch(again)
    assert torch.equal(_bits(out), _bits(again))


# ---------------------------------------------------------------- 3: the bit copies
def test_inactive_empty_and_closed_states_copy_rhs_in(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt).enable_fields()
    s.dof_vel.copy_(torch.from_numpy(np.random.default_rng(3).normal(scale=0.5, size=s.dof.numel())).to(DEV))
    g = _neg_zeros(s.rhs_gravity)

    def copies():
        out = s._enqueue_fields_rhs(g)
        return torch.equal(_bits(out), _bits(g)) and not bool(s.field_accel().any())
    assert copies()                                                    # no field
    i = s.add_wind(**GUSTY)
    assert not copies()
    first = s._rhs_fields.clone()
    s.reset_field_clock(1)
    assert torch.equal(_bits(first), _bits(s._enqueue_fields_rhs(g)))   # two runs on the same input at the same clock: the same bits
    s.stop_fields()
    assert copies()                                                    # inactive, the field still in its slot
    s.enable_fields()
    assert not copies()
    s.set_field(i, start=100 * s.dt, stop=200 * s.dt)
    s.add_radial(**dict(BLAST, start=0.0, stop=2 * s.dt))
    s.reset_field_clock(50)
    assert copies()                                                    # outside every window: before one, past the other
    s.reset_field_clock(100)
    assert not copies()
    s.clear_fields()
    assert copies()                                                    # n = 0 again


# ---------------------------------------------------------------- 4: the clock
def test_the_clock_counts_substeps_and_changes_are_seen_by_the_next(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt).enable_fields()
    assert s.field_clock() == 0
    for n in range(1, 4):
        s.stepforward()
        assert s.field_clock() == n
    assert torch.equal(_bits(s._rhs_fields), _bits(s.rhs_gravity))     # no field set: the substeps ran on rhs_gravity's bits
    s.reset_field_clock(41)
    assert s.field_clock() == 41
    i = s.add_wind(**GUSTY)
    s.stepforward()                                                    # the field added is seen by the next substep, at the clock's time
    assert s.field_clock() == 42
    first = s.field_accel().clone()
    assert bool(first.any())
    s.set_field(i, velocity=(0.0, 0.0, 9.0), gust=0.0)                 # ... and so is a changed one
    s.stepforward()
    x, v = ip_state(s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy(), s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    s.reset_field_clock(42)
    s._enqueue_fields_rhs(s.rhs_gravity)
    want = field_accel([wind(**dict(GUSTY, velocity=(0.0, 0.0, 9.0), gust=0.0))], x, v, 42 * s.dt, s.dt)
    assert rel_err(s.field_accel().cpu().numpy(), want) < 1e-12 and s.field_clock() == 43
    s.stop_fields()
    s.stepforward()
    assert s.field_clock() == 44                                       # the clock counts substeps, acting or not
    s.reset_field_clock()
    assert s.field_clock() == 0
    with pytest.raises(ValueError):
        s.reset_field_clock(-1)
    # enabled and configured before initialize(): the state arrives with the cloud
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud
    t = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device=DEV, persistent=False).enable_fields()
    t.add_wind(**GUSTY)
    t.add_radial(**BLAST)
    t.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert t.field_clock() == 0 and _device_state_bytes(t) == t.field_state_bytes() and t.Nx_csr is not None


# ---------------------------------------------------------------- 5: trajectories against the oracle, cell and CSR forms
FORCE = np.array([300.0, 100.0, -200.0])
WIND = dict(velocity=(5.0, 0.0, 1.0), drag=2.0, gust=0.5, hz=3.0, wave=(0.5, 0.0, 0.0))
FLOOR = dict(point=(0.0, -0.83, 0.0), normal=(0.0, 1.0, 0.0))
BALL = dict(centre=(0.0, 0.0, 0.9), radius=0.5)
SHELL = dict(centre=(0.0, 0.0, 0.0), radius=0.98, inside=True)
THREE_REF = [plane(FLOOR["point"], FLOOR["normal"]), sphere(BALL["centre"], BALL["radius"]), sphere(SHELL["centre"], SHELL["radius"], inside=True)]
SHAKE = ((0.05, 0.02, -0.03), 4.0, 0.3)


def _blast(dt):
    return dict(centre=(0.0, -1.2, 0.0), strength=300.0, radius=1.5, start=5 * dt, stop=8 * dt)     # the window opens at step 5


@pytest.fixture(scope="module")
def oracle_runs(small_cloud, small_opt):
    """Computed once, 20 substeps each under gravity and the pick force: the plain oracle; with a gusty wind and a blast whose window opens at step 5;
    with shaken pins and three colliders; and with pins, colliders and the fields together (the chain's order)."""
    def chain(ref):
        _, kern, Nx, X = oracle_pins(ref)
        par = dict(kappa=0.5, beta=0.5, mu=0.5, h=0.5 * ref.dx)
        return lambda k: (pin_term(ref.n_k, ref.stiff, kern, Nx, pin_u(X, (k + 1) * ref.dt, translate=SHAKE)), oracle_term(ref, THREE_REF, **par)[0])
    out = {}
    for name, with_fields, with_chain in (("plain", False, False), ("fields", True, False), ("chain", False, True), ("chain+fields", True, True)):
        ref = make_oracle_sim(small_cloud, small_opt)
        o = OracleFields(ref, [wind(**WIND), radial(**_blast(ref.dt))] if with_fields else [], extra=chain(ref) if with_chain else None)
        ref.update_force(ref.n_IP // 2, FORCE)
        out[name] = [o.step().copy() for _ in range(N_TRAJ)]
    return out


def _run(s, fields, chain):
    if chain:
        s.enable_pin_motion()
        s.set_pin_motion(translate=SHAKE)
        s.enable_contact()
        s.add_plane(**FLOOR)
        s.add_sphere(**BALL)
        s.add_sphere(**SHELL)
    if fields:
        s.enable_fields()
        s.add_wind(**WIND)
        s.add_radial(**_blast(s.dt))
    s.update_force(s.n_IP // 2, FORCE)
    out = []
    for _ in range(N_TRAJ):
        s.stepforward()
        out.append(_disp(s))
    return out


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_runs, monkeypatch, form):
    """The bar of a run with fields is 10 x the error of the same run without them, measured here: the field term feeds one more differently rounded
    input into every step.  Plain substeps set the bar of the wind-and-blast run; the run with pins and contact enabled is held to its own run without
    fields by the same rule (contact's friction is not smooth, so that baseline is not the plain substeps')."""
    monkeypatch.setenv("PN_SIM_FORM", form)
    worst = {}
    for name, fields, chain in (("plain", False, False), ("fields", True, False), ("chain", False, True), ("chain+fields", True, True)):
        s = _sim(small_cloud, small_opt)
        assert s.cell_form == (form == "cells")
        got = _run(s, fields, chain)
        errs = [rel_err(a, b) for a, b in zip(got, oracle_runs[name])]
        worst[name] = max(errs)
        print(f"{form} form, {name}, GPU vs oracle per substep: " + " ".join(f"{e:.1e}" for e in errs))
        if fields:
            assert s.field_clock() == N_TRAJ
        if fields and chain:
            assert s.pin_clock() == N_TRAJ and s.contact_count() > 0
            assert not torch.equal(s._rhs_ext, s.rhs_gravity) and not torch.equal(s._rhs_contact, s._rhs_ext) and not torch.equal(s._rhs_fields, s._rhs_contact)
    print(f"{form} form, worst rel err over {N_TRAJ} substeps: plain {worst['plain']:.3e}, with fields {worst['fields']:.3e}; pins + contact {worst['chain']:.3e}, "
          f"with fields {worst['chain+fields']:.3e}")
    moved = float(np.abs(oracle_runs["fields"][-1] - oracle_runs["plain"][-1]).max())
    opened = float(np.abs(oracle_runs["fields"][4] - oracle_runs["plain"][4]).max())
    print(f"oracle with fields vs without: max abs difference {opened:.3e} before the blast's window opens, {moved:.3e} at the end")
    assert moved > 1e-3      # the fields really moved it
    assert worst["fields"] <= 10.0 * worst["plain"], (worst["fields"], worst["plain"])
    assert worst["chain+fields"] <= 10.0 * worst["chain"], (worst["chain+fields"], worst["chain"])


# ---------------------------------------------------------------- 6: the harness forms
def _harness(small_opt, small_cloud, ckpt, W=64):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_fields()
    h.sim.add_wind(**dict(WIND, velocity=(40.0, 0.0, 10.0)))     # a gusty wind, strong enough to show within a few frames
    return h


@pytest.fixture(scope="module")
def eager_frames(small_opt, small_cloud, ckpt):
    """6 eager frames in a gusty wind: host images / depth_0 and the displacements after every step."""
    e = _harness(small_opt, small_cloud, ckpt)
    frames, disp = [], []
    for _ in range(6):
        frames.append(e.to_host(e.step()))
        e.synchronize()
        disp.append(_disp(e.sim))
    assert e.sim.field_clock() == 6
    return frames, disp


def test_captured_step_in_a_wind_equals_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, disp = eager_frames
    g = _harness(small_opt, small_cloud, ckpt).capture(n_trips=8)
    assert "fields" in g._captured_graph.stages and g.sim.field_clock() == 0 and torch.equal(g.sim.dof, g.sim.dof_rest)   # the warm-up steps left neither the clock nor the state advanced
    for f in range(4):
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - frames[f]["image"]).max() < 1e-5 and np.abs(b["depth_0"][0].cpu().numpy() - frames[f]["depth_0"]).max() < 1e-4, f
        e = rel_err(_disp(g.sim), disp[f])
        assert e < 1e-7, (f, e)
    assert g.sim.field_clock() == 4
    plain = SimRenderHarness(dict(small_opt, W=64, H=64), cloud=small_cloud, ckpt=ckpt, device=DEV)
    for _ in range(4):
        plain.step()
    plain.synchronize()
    d = float(np.abs(_disp(plain.sim) - disp[3]).max())
    print(f"displacements after 4 steps with and without the wind differ by {d:.3e}")
    assert d > 1e-3
    # a graph captured without the field launches refuses to run once fields are enabled
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=8)
    assert "fields" not in plain._captured_graph.stages
    plain.step_graph()
    plain.finish_graph_frame()
    plain.sim.enable_fields()
    with pytest.raises(RuntimeError, match="captured before enable_fields"):
        plain.step_graph()


def test_pipelined_frames_in_a_wind_equal_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, disp = eager_frames
    p = _harness(small_opt, small_cloud, ckpt).capture_pipelined(lanes=2, depth=2, n_trips=8)
    assert "fields" in p._captured_pipe.stages and p.sim.field_clock() == 0
    got = []
    for f in range(4):
        for idx, res in p.step_pipelined():
            got.append((idx, {k: res[k].copy() for k in ("image", "depth_0")}))
    for idx, res in p.drain_pipeline():
        got.append((idx, {k: res[k].copy() for k in ("image", "depth_0")}))
    assert [i for i, _ in got] == list(range(4))
    for f, (_, res) in enumerate(got):
        assert np.abs(res["image"] - frames[f]["image"]).max() < 1e-5, f
        assert np.abs(res["depth_0"].reshape(-1) - frames[f]["depth_0"].reshape(-1)).max() < 1e-4, f
    n = p.substeps_enqueued                        # the pipeline's simulator runs ahead of its frames: the clock counts its substeps
    assert 4 <= n <= len(disp) and p.sim.field_clock() == n
    err = rel_err(_disp(p.sim), disp[n - 1])
    print(f"pipelined (lanes 2, depth 2) in a wind vs eager after {n} substeps: {err:.2e}")
    assert err < 1e-7
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).capture_pipelined(lanes=2, depth=2, n_trips=8)
    plain.step_pipelined()
    plain.drain_pipeline()
    plain.sim.enable_fields()
    with pytest.raises(RuntimeError, match="captured before enable_fields"):
        plain.step_pipelined()


# ---------------------------------------------------------------- 7: main_render --wind --air_drag
def test_main_render_blows_on_the_chair(tmp_path, small_cloud):
    from pienerf_amd import main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--frames", "3", "--save_ip_state", "--quiet"]
    still = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "still")]))
    blown = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "blown"), "--wind", "5", "0", "0", "--air_drag", "1"]))
    assert [f.split("/")[-1] for f in still] == [f.split("/")[-1] for f in blown] == [f"img_{f}.png" for f in range(3)]
    # a frame shows the state its substep starts from: frame 0 is the rest state in both runs, frames 1 and 2 have felt the wind
    pos = [[np.load(tmp_path / d / f"ip_pos_{f}.npy") for f in range(3)] for d in ("still", "blown")]
    assert np.array_equal(pos[0][0], pos[1][0])
    shift = [float((pos[1][f] - pos[0][f])[:, 0].mean()) for f in (1, 2)]
    print(f"mean x-shift of the integration points against the run without wind: frame 1 {shift[0]:.3e}, frame 2 {shift[1]:.3e}")
    assert shift[1] > shift[0] > 0.0
    raw = [[open(p, "rb").read() for p in run] for run in (still, blown)]
    assert raw[0][0] == raw[1][0] and raw[0][2] != raw[1][2]
