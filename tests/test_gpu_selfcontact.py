"""Self-contact on the GPU (csrc/pn_selfcontact.hip; Simulator.enable_self_contact ...; main_render --self_contact): the launches' accel_out and
right-hand-side term against the numpy restatement (tests/selfcontact_reference.py) on the small chair squeezed by global maps, and on synthetic tables
that run the per-kernel sum's stride loop and all four waves; reproducibility from zeroed and dirty work buffers; the bit copies; the overflow cap; a
block dropped onto a pinned block and the whole chain of stages against the CPU oracle whose public rhs_gravity is set to g0 + [the earlier stages' terms
+] term(state) before every stepforward(), in the cell and CSR forms; the harness forms (eager, captured step, pipelined); and main_render end to end."""
import re

import numpy as np
import pytest
import torch

import selfcontact_reference as R
from conftest import make_oracle_sim, rel_err
from contact_reference import contact_term, ip_state, oracle_term, plane, sphere
from fields_reference import oracle_field_term, wind
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
from test_gpu_fields import _bits, _disp, _neg_zeros, _sim
from test_gpu_parity import DEV
from test_pins_host import oracle_pins, pin_term, pin_u

pytestmark = pytest.mark.gpu

SQUEEZED, SHRUNK, COLLAPSED = np.diag([1.0, 0.25, 1.0]), 0.3 * np.eye(3), 0.02 * np.eye(3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _map_dof(s, A, seed=None):
    """dof of the global map x = A X, with `seed` plus a per-kernel perturbation of the translation dofs of 0.02 dx."""
    dof = R.global_map(s.kernel_pos.cpu().numpy(), A)
    if seed is not None:
        dof[:, 0, :] += np.random.default_rng(seed).normal(scale=0.02 * s.dx, size=(s.n_k, 3))
    return dof.reshape(-1)


def _set_state(s, dof, vel=None):
    s.dof.copy_(_dev(dof))
    s.dof_vel.copy_(_dev(vel) if vel is not None else torch.zeros_like(s.dof_vel))


def _numpy_term(s, mu=0.0, **par):
    """(term [10 n_k, 3], a [n_IP, 3]) of the simulator's current state, from its own tables."""
    topo, Nx = s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy()
    x, v = ip_state(topo, Nx, s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    a = R.self_accel(x, v, s.IP_pos.cpu().numpy().astype(np.float64), m, s.dt, **R.params(s.dx, mu=mu, **par))[0]
    return contact_term(s.n_k, topo, Nx, m, a), a


# ---------------------------------------------------------------- 1: accel_out and rhs_out - rhs_in against numpy, on the small chair
CASES = {"squeezed": (SQUEEZED, 31), "shrunk": (SHRUNK, 32)}


@pytest.fixture(scope="module")
def states(small_cloud, small_opt):
    """Computed once: for both maps the perturbed dof, random dof_vel, and the reference's (term, a) for mu = 0 and mu = 0.5."""
    s = _sim(small_cloud, small_opt)
    assert (s.n_IP, s.n_k) == (432, 139)
    out = {}
    for name, (A, seed) in CASES.items():
        dof = _map_dof(s, A, seed)
        vel = np.random.default_rng(seed + 100).normal(scale=0.5, size=dof.size)
        _set_state(s, dof, vel)
        out[name] = dict(dof=dof, vel=vel, ref={mu: _numpy_term(s, mu=mu) for mu in (0.0, 0.5)})
    return out


@pytest.mark.parametrize("mu", [0.0, 0.5])
@pytest.mark.parametrize("name", list(CASES))
def test_term_equals_the_numpy_term(small_cloud, small_opt, states, name, mu):
    s = _sim(small_cloud, small_opt).enable_self_contact(friction=mu)
    st = states[name]
    _set_state(s, st["dof"], st["vel"])
    want, a = st["ref"][mu]
    g = s.rhs_gravity.clone()
    out = s._enqueue_self_rhs(g)
    acc = s.self_contact_accel()
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err((out - g).cpu().numpy().reshape(-1, 3), want)
    n_ref = int(a.any(axis=1).sum())
    m = (s.IP_rho * s.dx ** 3).cpu().numpy()
    ma = m[:, None] * acc.cpu().numpy()
    mom = float(np.abs(ma.sum(axis=0)).max() / np.abs(ma).sum())
    print(f"{name}, mu = {mu}: {n_ref} points in contact, max|accel| {np.abs(a).max():.3e}, max|term| {np.abs(want).max():.3e}, rel err accel {e_a:.2e}, "
          f"term {e_t:.2e}, net momentum / sum |m a| {mom:.2e}")
    assert n_ref > 100 and np.abs(want).max() > 1.0          # so the bar means something
    assert e_a < 1e-12 and e_t < 1e-12, (e_a, e_t)
    assert s.self_contact_count() == n_ref
    assert mom <= 1e-12
    assert s.self_contact_overflows() == 0 and torch.equal(s.rhs_gravity, g)             # the input is left alone
    idle = ~a.any(axis=1)                                    # kernels none of whose points has a != 0 carry rhs_in's bits
    untouched = np.ones(s.n_k, bool)
    untouched[np.unique(s.IP_kernel.cpu().numpy()[~idle])] = False
    rows = _dev(np.repeat(untouched, 30))
    assert torch.equal(_bits(out[rows]), _bits(g[rows]))
    dev_state = bytes(s._self_state.view(torch.uint8).cpu().numpy().tobytes())
    assert dev_state == s.self_contact_state_bytes()         # the device state is what the mirror says it is
    if mu:                                                   # friction changed the term
        assert not np.array_equal(a, st["ref"][0.0][1])
    plain = _sim(small_cloud, small_opt)
    assert plain.Nx_csr is None and plain._self_state is None and not plain.self_contact_enabled   # the tables exist only with the feature on


# ---------------------------------------------------------------- 2: the same bits from every run
def test_two_runs_from_zeroed_and_dirty_work_buffers_give_equal_bits(small_cloud, small_opt, states):
    s = _sim(small_cloud, small_opt).enable_self_contact(friction=0.5)
    _set_state(s, states["shrunk"]["dof"], states["shrunk"]["vel"])
    g = s.rhs_gravity.clone()
    s._self_work.zero_()
    first, acc = s._enqueue_self_rhs(g).clone(), s.self_contact_accel().clone()
    assert bool(acc.any())
    for fill in (0x7F7F7F7F, -1, 0x00010001):               # huge counts and starts, negative ones, small ones; doubles that are NaNs or denormals
        s._self_work.view(torch.int32).fill_(fill)
        s._self_accel.fill_(7.0)
        s._rhs_self.fill_(3.0)
        again = s._enqueue_self_rhs(g)
        assert torch.equal(_bits(first), _bits(again)) and torch.equal(_bits(acc), _bits(s.self_contact_accel())), hex(fill & 0xFFFFFFFF)
    assert s.self_contact_overflows() == 0


# ---------------------------------------------------------------- 3: the bit copies
def test_rest_stopped_and_excluded_states_copy_rhs_in(small_cloud, small_opt, states):
    s = _sim(small_cloud, small_opt).enable_self_contact()
    g = _neg_zeros(s.rhs_gravity)

    def copies():
        out = s._enqueue_self_rhs(g)
        return torch.equal(_bits(out), _bits(g)) and not bool(s.self_contact_accel().any()) and s.self_contact_count() == 0
    s.dof_vel.copy_(_dev(states["squeezed"]["vel"]))
    assert copies()                                                    # at rest, whatever the velocities
    _set_state(s, states["squeezed"]["dof"], states["squeezed"]["vel"])
    assert not copies()
    s.stop_self_contact()
    assert copies()                                                    # inactive
    s.enable_self_contact()
    assert not copies()
    s.set_self_contact_params(exclusion=5.0)                           # larger than the body's diameter: no pair is eligible
    assert copies()
    s.set_self_contact_params(exclusion=3 * s.dx)
    assert not copies()
    assert s.self_contact_overflows() == 0


# ---------------------------------------------------------------- 4: the cap
def test_a_collapsed_body_overflows_and_adds_nothing(small_cloud, small_opt, states):
    s = _sim(small_cloud, small_opt).enable_self_contact()
    g = _neg_zeros(s.rhs_gravity)
    _set_state(s, _map_dof(s, COLLAPSED))
    x = ip_state(s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy(), s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())
    assert R.overflows(*x, s.dx) == (True, 86, 86)
    for n in range(1, 4):
        out = s._enqueue_self_rhs(g)
        assert torch.equal(_bits(out), _bits(g)) and not bool(s.self_contact_accel().any())
        assert s.self_contact_overflows() == n                         # one per substep enqueued; reading it back means the launches returned
    s._enqueue_self_rhs(s.rhs_gravity)
    assert s.self_contact_overflows() == 4
    st = states["shrunk"]                                              # the same simulator afterwards: the full term again
    _set_state(s, st["dof"], st["vel"])
    want, a = st["ref"][0.0]
    out = s._enqueue_self_rhs(g)
    assert rel_err(s.self_contact_accel().cpu().numpy(), a) < 1e-12 and rel_err((out - g).cpu().numpy().reshape(-1, 3), want) < 1e-12
    assert s.self_contact_overflows() == 4
    assert bytes(s._self_state.view(torch.uint8).cpu().numpy().tobytes()) == s.self_contact_state_bytes(overflowed=4)


# ---------------------------------------------------------------- 5: synthetic tables: the stride loop and all four waves
def test_term_on_a_run_longer_than_two_passes_of_the_workgroup():
    """n_k = 3, n_IP = 76: points 0..74 have all 8 slots on kernel 0 (600 entries: more than 2 x 256 and not a multiple of 64), point 75 has all 8 on
    kernel 2, kernel 1 is empty.  The library is called on these tables directly; the restatement needs no physics.  h = 0.8 over a cloud about two
    units wide gives most points several partners."""
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    from pienerf_amd.simulator import solver
    n_k, n_IP, dt, dx = 3, 76, 1e-2, 0.1
    rng = np.random.default_rng(21)
    topo = np.zeros((n_IP, 8), np.int32)
    topo[75] = 2
    Nx = rng.normal(scale=0.4, size=(n_IP, 8, 10))
    dof, vel = rng.normal(scale=0.3, size=n_k * 30), rng.normal(scale=0.5, size=n_k * 30)
    rho = rng.uniform(500.0, 1500.0, size=n_IP)
    X = rng.normal(scale=1.0, size=(n_IP, 3))
    order = np.argsort(topo.reshape(-1), kind="stable").astype(np.int32)                    # entry = point 8 + slot, by kernel
    cnt = np.bincount(topo.reshape(-1), minlength=n_k).astype(np.int32)
    bg = (np.cumsum(cnt) - cnt).astype(np.int32)
    assert cnt.tolist() == [600, 0, 8] and bg.tolist() == [0, 600, 600] and 600 > 2 * 256 and 600 % 64 != 0
    g = rng.normal(size=n_k * 30)
    g[rng.random(g.size) < 0.2] = -0.0
    par = dict(kappa=0.7, beta=0.4, mu=0.3, h=0.8, rho_x=1.2)
    state = _dev(np.frombuffer(solver.pack_self_contact_state(1, [par[k] for k in ("kappa", "beta", "mu", "h", "rho_x")]), np.float64).copy())
    work = torch.full((int(lib().pn_sim_self_work_bytes(n_IP)) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    t = dict(dof=_dev(dof), vel=_dev(vel), X=_dev(X), topo=_dev(topo), rho=_dev(rho), Nx=_dev(Nx), bg=_dev(bg), cnt=_dev(cnt), buf=_dev(order),
             csr=_dev(Nx.reshape(-1, 10)[order]), g=_dev(g))
    out, acc = torch.full_like(t["g"], 7.0), torch.full((n_IP, 3), 7.0, dtype=torch.float64, device=DEV)

    def launch(o, a):
        check(lib().pn_sim_self_rhs(n_k, n_IP, ptr(state), ptr(work), dt, dx, ptr(t["dof"]), ptr(t["vel"]), ptr(t["X"]), ptr(t["topo"]), ptr(t["rho"]),
                                    ptr(t["Nx"]), ptr(t["bg"]), ptr(t["cnt"]), ptr(t["buf"]), ptr(t["csr"]), ptr(t["g"]), ptr(o), a, stream_ptr()), "sim_self_rhs")
    launch(out, ptr(acc))
    x, v = ip_state(topo, Nx, dof, vel)
    m = rho * dx ** 3
    a, S, part = R.self_accel(x, v, X, m, dt, **par)
    want = contact_term(n_k, topo, Nx, m, a)
    e_a, e_t = rel_err(acc.cpu().numpy(), a), rel_err((out - t["g"]).cpu().numpy().reshape(-1, 3), want)
    print(f"600-entry run: {int(a.any(axis=1).sum())} of 76 points in contact, at most {max(len(p) for p in part)} partners, max|term| {np.abs(want).max():.3e}, "
          f"rel err accel {e_a:.2e}, term {e_t:.2e}")
    assert int(a.any(axis=1).sum()) > 30 and max(len(p) for p in part) >= 4 and np.abs(want).max() > 1.0
    assert e_a < 1e-12 and e_t < 1e-12
    assert torch.equal(_bits(out[30:60]), _bits(t["g"][30:60])) and bool(torch.signbit(out[30:60][out[30:60] == 0.0]).all())   # the empty kernel: rhs_in, bit for bit
    again = torch.full_like(out, 3.0)
    launch(again, None)                                                                     # accel_out NULL: a_i stays in the work area, the same bits
    assert torch.equal(_bits(out), _bits(again))


# ---------------------------------------------------------------- 6: a block dropped onto a pinned block, against the oracle
N_DROP = 60


def _two_blocks(opt):
    """A pinned block of 7 x 7 x 3 integration points low in the box and a free one of 4 x 4 x 2 a kernel cell above it (the kernel spacing is 2 / 6): the
    two share no GMLS kernel, so nothing but self-contact couples them.  The free block's lowest points start 0.5 above the pinned block's highest
    ones, fall 0.4 under gravity and arrive with 2.8 m/s, 0.028 a substep: well below h = 0.1 (no tunnelling)."""
    a = scene.make_block_points((-0.3, -0.98, -0.3), (0.3, -0.75, 0.3), sub_res=30, pinned=True, hgs=opt["hash_grid_size"])
    b = scene.make_block_points((-0.2, -0.28, -0.2), (0.2, -0.15, 0.2), sub_res=30, hgs=opt["hash_grid_size"])
    return scene.concat_clouds(a, b)


def _gap(x, low):
    return float(x[~low, 1].min() - x[low, 1].max())


@pytest.fixture(scope="module")
def drop_runs(small_opt):
    """Computed once on the CPU: the oracle's 60 substeps with the numpy term and without it, displacements and the gap after every substep; and the
    two conditions the reference alone must meet for the test to mean something."""
    cloud = _two_blocks(small_opt)
    out = {"cloud": cloud}
    for name, par in (("self", True), ("plain", False)):
        ref = make_oracle_sim(cloud, small_opt)
        low = np.asarray(ref.IP_pos, np.float64)[:, 1] < -0.5
        topo = ref.IP_kernel.numpy()
        assert (ref.n_IP, int(low.sum())) == (140, 108) and np.intersect1d(topo[low], topo[~low]).size == 0     # two pieces that share no kernel
        o = R.OracleSelf(ref, R.params(ref.dx) if par else None)
        disp, gaps, hits = [], [], 0
        for _ in range(N_DROP):
            disp.append(o.step().copy())
            gaps.append(_gap(o.ip_positions(), low))
            hits = max(hits, o.hits)
        out[name] = dict(disp=disp, gaps=gaps, hits=hits)
        out["low"], out["X"] = low, np.asarray(ref.IP_pos, np.float64)
    print(f"oracle, two blocks: smallest gap with the term {min(out['self']['gaps']):.4f} (at most {out['self']['hits']} points in contact), without it "
          f"{min(out['plain']['gaps']):.4f}")
    assert min(out["self"]["gaps"]) > 0.0 and out["self"]["hits"] > 0        # with the term the free block never drops below the pinned block's top ...
    assert min(out["plain"]["gaps"]) < 0.0                                   # ... and without it, it does
    return out


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_a_dropped_block_lands_on_a_pinned_block(small_opt, drop_runs, monkeypatch, form):
    """Measured on an MI355X: worst rel err over the 60 substeps 8.0e-7 without the stage and 8.0e-7 with it (cells), 3.2e-7 and 3.2e-7 (CSR); smallest gap
    0.0224 with the stage (the oracle's 0.0224), -1.2248 without.  The bar of the run with the stage is 10 x the error of the same run without it,
    measured here, the rule of test_gpu_fields.test_trajectory_matches_the_oracle; mu = 0 (friction is not smooth)."""
    monkeypatch.setenv("PN_SIM_FORM", form)
    low, worst, gaps = drop_runs["low"], {}, {}
    for name in ("plain", "self"):
        s = _sim(drop_runs["cloud"], small_opt)
        assert s.cell_form == (form == "cells") and np.array_equal(s.IP_pos.cpu().numpy().astype(np.float64), drop_runs["X"])
        if name == "self":
            s.enable_self_contact()
        errs, gp = [], []
        for k in range(N_DROP):
            s.stepforward()
            errs.append(rel_err(_disp(s), drop_runs[name]["disp"][k]))
            x = ip_state(s.IP_kernel.cpu().numpy(), s.IP_Nx.cpu().numpy(), s.dof.cpu().numpy(), s.dof_vel.cpu().numpy())[0]
            gp.append(_gap(x, low))
        worst[name], gaps[name] = max(errs), min(gp)
        print(f"{form} form, {name}, GPU vs oracle per substep: " + " ".join(f"{e:.1e}" for e in errs))
        if name == "self":
            assert s.self_contact_overflows() == 0
    print(f"{form} form, worst rel err over {N_DROP} substeps: plain {worst['plain']:.3e}, with self-contact {worst['self']:.3e}; smallest gap with the stage "
          f"{gaps['self']:.4f} (oracle {min(drop_runs['self']['gaps']):.4f}), without {gaps['plain']:.4f}")
    assert gaps["self"] > 0.0 and gaps["plain"] < 0.0
    assert worst["self"] <= 10.0 * worst["plain"], (worst["self"], worst["plain"])


# ---------------------------------------------------------------- 7: the whole chain on the squeezed chair
N_CHAIN, K_ALL = 20, 5      # the squeezed chair springs apart within eight substeps: the stages' buffers are compared after substep K_ALL, while all act
SHAKE = ((0.05, 0.02, -0.03), 4.0, 0.3)
WIND = dict(velocity=(5.0, 0.0, 1.0), drag=2.0, gust=0.5, hz=3.0, wave=(0.5, 0.0, 0.0))
FLOOR = dict(point=(0.0, -0.25, 0.0), normal=(0.0, 1.0, 0.0))        # under the squeezed legs
BALL = dict(centre=(0.0, 0.0, 0.9), radius=0.5)
SHELL = dict(centre=(0.0, 0.0, 0.0), radius=0.98, inside=True)
THREE_REF = [plane(FLOOR["point"], FLOOR["normal"]), sphere(BALL["centre"], BALL["radius"]), sphere(SHELL["centre"], SHELL["radius"], inside=True)]


@pytest.fixture(scope="module")
def chain_runs(small_cloud, small_opt):
    """Computed once: 20 oracle substeps from the squeezed chair with shaken pins, three colliders and a gusty wind, without and with self-contact."""
    out = {}
    for name in ("chain", "chain+self"):
        ref = make_oracle_sim(small_cloud, small_opt)
        ref.dof[:] = R.global_map(np.asarray(ref.kernel_pos, np.float64), SQUEEZED).reshape(ref.dof.shape)
        _, kern, Nx, Xp = oracle_pins(ref)
        par = dict(kappa=0.5, beta=0.5, mu=0.5, h=0.5 * ref.dx)

        def extra(k, ref=ref, kern=kern, Nx=Nx, Xp=Xp, par=par):
            return (pin_term(ref.n_k, ref.stiff, kern, Nx, pin_u(Xp, (k + 1) * ref.dt, translate=SHAKE)), oracle_term(ref, THREE_REF, **par)[0],
                    oracle_field_term(ref, [wind(**WIND)], k * ref.dt)[0])
        o = R.OracleSelf(ref, R.params(ref.dx) if name == "chain+self" else None, extra=extra)
        disp, hits = [], []
        for _ in range(N_CHAIN):
            disp.append(o.step().copy())
            hits.append(o.hits)
        out[name] = dict(disp=disp, hits=hits)
        out["X"] = np.asarray(ref.IP_pos, np.float64)
    print("oracle, the chain on the squeezed chair: points in self-contact per substep", out["chain+self"]["hits"])
    assert out["chain+self"]["hits"][0] > 100 and out["chain+self"]["hits"][K_ALL - 1] > 0
    return out


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_the_whole_chain_matches_the_oracle(small_cloud, small_opt, chain_runs, monkeypatch, form):
    monkeypatch.setenv("PN_SIM_FORM", form)
    worst = {}
    for name in ("chain", "chain+self"):
        s = _sim(small_cloud, small_opt)
        assert np.array_equal(s.IP_pos.cpu().numpy().astype(np.float64), chain_runs["X"])      # the same rest positions decide the same eligible pairs
        _set_state(s, _map_dof(s, SQUEEZED))
        s.enable_pin_motion()
        s.set_pin_motion(translate=SHAKE)
        s.enable_contact()
        s.add_plane(**FLOOR)
        s.add_sphere(**BALL)
        s.add_sphere(**SHELL)
        s.enable_fields()
        s.add_wind(**WIND)
        if name == "chain+self":
            s.enable_self_contact()
        errs = []
        for k in range(N_CHAIN):
            s.stepforward()
            errs.append(rel_err(_disp(s), chain_runs[name]["disp"][k]))
            if name == "chain+self" and k == K_ALL - 1:       # every stage's buffer differs from the one before it
                assert s.contact_count() > 0 and s.self_contact_count() > 0
                assert not torch.equal(s._rhs_ext, s.rhs_gravity) and not torch.equal(s._rhs_contact, s._rhs_ext)
                assert not torch.equal(s._rhs_fields, s._rhs_contact) and not torch.equal(s._rhs_self, s._rhs_fields)
        worst[name] = max(errs)
        print(f"{form} form, {name}, GPU vs oracle per substep: " + " ".join(f"{e:.1e}" for e in errs))
        assert s.pin_clock() == N_CHAIN and s.field_clock() == N_CHAIN
    print(f"{form} form, worst rel err over {N_CHAIN} substeps: pins + contact + wind {worst['chain']:.3e}, with self-contact {worst['chain+self']:.3e}")
    moved = float(np.abs(chain_runs["chain+self"]["disp"][-1] - chain_runs["chain"]["disp"][-1]).max())
    assert moved > 1e-3      # the stage really changed the run
    assert worst["chain+self"] <= 10.0 * worst["chain"], (worst["chain+self"], worst["chain"])


# ---------------------------------------------------------------- 8: the harness forms
N_FRAMES, K_SET = 6, 2      # in the captured run the parameters change in front of frame K_SET


def _harness(small_opt, small_cloud, ckpt, W=64, enable=True):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    _set_state(h.sim, _map_dof(h.sim, SQUEEZED))
    if enable:
        h.sim.enable_self_contact(friction=0.3)
    return h


def _change(sim):
    sim.set_self_contact_params(stiffness=1.0, damping=0.0, friction=0.0)


def _eager(small_opt, small_cloud, ckpt, n, change_at=None):
    """n eager frames from the squeezed chair: host images / depth_0, the displacements after every step, the points in self-contact per substep."""
    e = _harness(small_opt, small_cloud, ckpt)
    frames, disp, counts = [], [], []
    for f in range(n):
        if f == change_at:
            _change(e.sim)
        frames.append(e.to_host(e.step()))
        e.synchronize()
        disp.append(_disp(e.sim))
        counts.append(e.sim.self_contact_count())
    return frames, disp, counts


@pytest.fixture(scope="module")
def eager_frames(small_opt, small_cloud, ckpt):
    frames, disp, counts = _eager(small_opt, small_cloud, ckpt, N_FRAMES)
    print("eager frames from the squeezed chair: points in self-contact per substep", counts)
    assert counts[0] > 100 and counts[K_SET] > 0
    return frames, disp


def test_captured_step_equals_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, disp, _ = _eager(small_opt, small_cloud, ckpt, K_SET + 2, change_at=K_SET)
    assert np.array_equal(disp[K_SET - 1], eager_frames[1][K_SET - 1]) and rel_err(disp[K_SET], eager_frames[1][K_SET]) > 1e-6   # the change changes the run
    g = _harness(small_opt, small_cloud, ckpt).capture(n_trips=8)
    assert "self" in g._captured_graph.stages and rel_err(g.sim.dof.cpu().numpy(), _map_dof(g.sim, SQUEEZED)) == 0.0    # the warm-up steps left the state where it was
    for f in range(K_SET + 2):
        if f == K_SET:
            _change(g.sim)                                                 # followed without a recapture: the state is device memory
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - frames[f]["image"]).max() < 1e-5 and np.abs(b["depth_0"][0].cpu().numpy() - frames[f]["depth_0"]).max() < 1e-4, f
        e = rel_err(_disp(g.sim), disp[f])
        assert e < 1e-7, (f, e)
    plain = _harness(small_opt, small_cloud, ckpt, enable=False)
    for _ in range(K_SET):
        plain.step()
    plain.synchronize()
    d = float(np.abs(_disp(plain.sim) - disp[K_SET - 1]).max())
    print(f"displacements after {K_SET} steps with and without self-contact differ by {d:.3e}")
    assert d > 1e-3
    # a graph captured without the stage's launches refuses to run once it is enabled
    plain = _harness(small_opt, small_cloud, ckpt, W=32, enable=False).capture(n_trips=8)
    assert "self" not in plain._captured_graph.stages
    plain.step_graph()
    plain.finish_graph_frame()
    plain.sim.enable_self_contact()
    with pytest.raises(RuntimeError, match="captured before enable_self_contact"):
        plain.step_graph()


def test_pipelined_frames_equal_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, disp = eager_frames
    p = _harness(small_opt, small_cloud, ckpt).capture_pipelined(lanes=2, depth=2, n_trips=8)
    assert "self" in p._captured_pipe.stages
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
    n = p.substeps_enqueued                        # the pipeline's simulator runs ahead of its frames
    assert 4 <= n <= len(disp)
    err = rel_err(_disp(p.sim), disp[n - 1])
    print(f"pipelined (lanes 2, depth 2) from the squeezed chair vs eager after {n} substeps: {err:.2e}")
    assert err < 1e-7
    plain = _harness(small_opt, small_cloud, ckpt, W=32, enable=False).capture_pipelined(lanes=2, depth=2, n_trips=8)
    plain.step_pipelined()
    plain.drain_pipeline()
    plain.sim.enable_self_contact()
    with pytest.raises(RuntimeError, match="captured before enable_self_contact"):
        plain.step_pipelined()


# ---------------------------------------------------------------- 9: main_render --self_contact
def test_main_render_drops_a_block_onto_a_block(tmp_path, small_opt, capsys):
    """Two pieces in one PLY, the free one two cells above the pinned one.  With thickness = exclusion just under 0.2 the facing points are eligible
    (0.2 apart at rest) and touch as soon as gravity has moved the free block at all."""
    from pienerf_amd import main_render
    a = scene.make_block_points((-0.3, -0.98, -0.3), (0.3, -0.75, 0.3), sub_res=30, pinned=True, hgs=small_opt["hash_grid_size"])
    b = scene.make_block_points((-0.2, -0.6, -0.2), (0.2, -0.4, 0.2), sub_res=30, hgs=small_opt["hash_grid_size"])
    scene.write_ply(str(tmp_path / "blocks.ply"), scene.concat_clouds(a, b))
    argv = ["--ply", str(tmp_path / "blocks.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--frames", "4", "--save_ip_state",
            "--self_contact", "--self_thickness", "0.199999", "--self_exclusion", "0.199999", "--out", str(tmp_path / "out")]
    written = main_render.run(main_render.parser().parse_args(argv))
    assert [f.split("/")[-1] for f in written] == [f"img_{f}.png" for f in range(4)]
    said = capsys.readouterr().out
    print(said)
    m = re.search(r"self-contact: (\d+) of (\d+) integration points .* (\d+) substeps over the bucket cap", said)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) == 0
    pos = [np.load(tmp_path / "out" / f"ip_pos_{f}.npy") for f in range(4)]
    free = pos[0][:, 1] > -0.7
    assert free.any() and (pos[3][free, 1] < pos[0][free, 1]).all()     # the free block fell
