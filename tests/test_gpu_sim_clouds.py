"""The simulator on clouds beyond the chair (tests/sim_clouds.py: per-point materials with mu != lam, kernel-grid cells of two chunks, ragged chunks,
points that repeat a kernel) against the fp64 CPU oracle: initialisation, the elastic ops on a deformed state, eight substeps under a changing force
in the cell, CSR and persistent forms and with svd='mcadams', a captured cell-form substep, update_pos and the mesh warp on stray points, the
kinematic-pin term with repeated kernels, and the diagnostics.  tests/test_sim_clouds_host.py shows on the CPU that the 1e-4 bar used here tells
exchanged and mis-permuted materials apart (they move the oracle's displacements by 0.97 and by 28 .. 48 relative)."""
import numpy as np
import pytest
import torch

import oracle
import sim_clouds as SC
from conftest import make_oracle_sim, rel_err
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

FORMS = ("cells", "csr", "persistent", "mcadams")
# between two forms of the default decomposition: test_gpu_persistent.py's bar (summation orders, the SVD's stopping rule at 1e-11 / 1e-12)
FORM_BAR = 1e-8
# ... except the cell form on the beam: measured 8.95e-8 against the CSR form (substep 0, where gravity alone has moved the beam by very little), while
# every form is inside 1e-6 of the oracle (cell form 9.3e-8, CSR 3.8e-9, persistent 3.7e-9).  The cause is not the order of a sum (perturbing the
# right-hand side by 1e-16 relative moves the oracle's beam by 5e-12) but the stopping rule of the warm-started decomposition: the cell form stops at
# off-diagonals of 1e-11 of the diagonal (PN_CELL_SVD_TOL), the other two at 1e-12, and the beam — five times the chair's stiffness against the same
# 1e-3 regulariser — turns a rotation error into twenty times the displacement error the chair does.  The kernels' own decomposition run on the CPU
# with the two rules reproduces both figures (beam 1.06e-7, two_blocks 2.9e-10; two_blocks measured 2.86e-10).  Ten times the measurement, below 1e-6:
FORM_BAR_BEAM_CELLS = 9e-7


def _sim(cloud, form="cells"):
    from pienerf_amd.simulator.solver import Simulator
    o = SC.opt()
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device=DEV, persistent=form == "persistent", svd="mcadams" if form == "mcadams" else "jacobi")
    s.cell_form = True   # whatever PN_SIM_FORM says: the form is this module's parameter
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    if form == "csr":
        s.cell_form = False
    return s


@pytest.fixture(scope="module")
def refs():
    """name -> the cloud, its oracle after the eight scheduled substeps (every table of the initialisation is as it was at rest), the displacements
    behind every substep, and the deformed state.  Built once, read only."""
    out = {}
    for name in SC.NAMES:
        cloud = SC.make(name)
        ref = make_oracle_sim(cloud, SC.opt())
        SC.check_facts(name, SC.facts(ref))
        traj = []
        SC.run_schedule(ref, name, after_step=lambda k, r: traj.append(r.dof - r.dof_rest))
        for a in traj:
            a.setflags(write=False)
        out[name] = dict(cloud=cloud, ref=ref, traj=traj, dof=ref.dof.copy(), vel=ref.dof_vel.copy(), info=ref.get_IP_info())
    return out


_RUNS = {}


def _run(refs, name, form):
    """The scheduled substeps of one form on one cloud, run once per module: displacements behind every substep, the final velocity and IP state."""
    if (name, form) not in _RUNS:
        s = _sim(refs[name]["cloud"], form)
        traj = []
        SC.run_schedule(s, name, after_step=lambda k, sim: traj.append((sim.dof - sim.dof_rest).cpu().numpy().reshape(-1, 3)))   # (.cpu() synchronises)
        torch.cuda.synchronize()
        if form == "persistent":   # one persistent simulator at a time (test_gpu_persistent.test_persistent_substep_inside_a_captured_graph)
            assert s.persistent and s._coop is not None and not s.persistent_timed_out()
        else:
            assert s._coop is None and (s._cells_work is not None) and s.cell_form == (form != "csr")
        _RUNS[(name, form)] = dict(traj=traj, vel=s.dof_vel.cpu().numpy().reshape(-1, 3), info=tuple(t.cpu().numpy() for t in s.get_IP_info()))
    return _RUNS[(name, form)]


# ------------------------------------------------------------------------------------------------ initialisation
@pytest.mark.parametrize("name", SC.NAMES)
def test_initialisation_parity(refs, name):
    """test_gpu_parity.test_sim_kernels_and_step's bars, and collect_IP's means to round-off (2^-47: each side within 2^-48 of the exact mean,
    tests/test_sim_clouds_host.py)."""
    ref = refs[name]["ref"]
    s = _sim(refs[name]["cloud"])
    assert (s.n_IP, s.n_k) == (ref.n_IP, ref.n_k)
    assert np.array_equal(s.IP_kernel.cpu().numpy(), ref.IP_kernel.numpy()) and np.array_equal(s.pts_kernel.cpu().numpy(), ref.pts_kernel.numpy())
    e = dict(dNx=rel_err(s.IP_dNx.cpu().numpy(), ref.IP_dNx), Ainv=rel_err(s.Ainv.cpu().numpy(), ref.Ainv),
             rhs_rest=rel_err(s.rhs_rest.cpu().numpy().reshape(-1, 3), ref.rhs_rest))
    for k, want in (("mu", ref.IP_mu), ("lam", ref.IP_lam), ("rho", ref.IP_rho)):
        e[k] = float(np.abs(getattr(s, "IP_" + k).cpu().numpy() / want - 1.0).max())
    print(name, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["dNx"] < 1e-12 and e["Ainv"] < 1e-8 and e["rhs_rest"] < 1e-10
    assert max(e["mu"], e["lam"], e["rho"]) <= 2.0 ** -47
    c = s._cells
    src, valid = c["src"], c["valid"]
    assert torch.equal(c["mu"].view(valid.shape)[valid], s.IP_mu[src[valid]]) and torch.equal(c["lam"].view(valid.shape)[valid], s.IP_lam[src[valid]])


# ------------------------------------------------------------------------------------------------ the elastic ops on a deformed state
def _elastic(s):
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    RF = torch.empty((s.n_IP, 3, 3), dtype=torch.float64, device=DEV)
    VF = torch.empty_like(RF)
    check(lib().pn_sim_calc_elastic(s.n_IP, ptr(s.IP_kernel), ptr(s.IP_dNx), ptr(s.dof), ptr(RF), ptr(VF), None, 0, stream_ptr()), "calc_elastic")
    torch.cuda.synchronize()
    return RF.cpu().numpy(), VF.cpu().numpy()


@pytest.mark.parametrize("name", SC.NAMES)
def test_elastic_ops_on_the_deformed_state(refs, name):
    """pn_sim_calc_elastic (R and V F per point, 1e-9 as test_gpu_edges holds it to the oracle) and build_rhs() (1e-10, test_sim_kernels_and_step) on
    the oracle's state after the eight substeps; build_rhs() once more with IP_mu / IP_lam overwritten by seeded values of 1e4 .. 1e7 that have
    nothing to do with their neighbours', so that no lane can take another point's value unnoticed."""
    r = refs[name]
    ref = r["ref"]
    s = _sim(r["cloud"])
    s.dof.copy_(T(r["dof"].reshape(-1)))
    topo = ref.IP_kernel.numpy()
    RF_ref, VF_ref, _ = oracle.calc_elastic(topo, ref.IP_dNx, r["dof"])
    RF, VF = _elastic(s)
    eR, eV = np.abs(RF - RF_ref).max(), np.abs(VF - VF_ref).max()
    assert np.abs(RF_ref - np.eye(3)).max() > 1e-3                                     # a deformed state
    want = oracle.collect_rhs_IP(ref.dx, topo, ref.IP_mu, ref.IP_lam, ref.IP_dNx, RF_ref, VF_ref, ref.n_k * 10)
    e1 = rel_err(s.build_rhs().cpu().numpy().reshape(-1, 3), want)
    rng = np.random.default_rng(7)
    mu, lam = 10.0 ** rng.uniform(4, 7, s.n_IP), 10.0 ** rng.uniform(4, 7, s.n_IP)
    s.IP_mu.copy_(T(mu))
    s.IP_lam.copy_(T(lam))
    want2 = oracle.collect_rhs_IP(ref.dx, topo, mu, lam, ref.IP_dNx, RF_ref, VF_ref, ref.n_k * 10)
    e2 = rel_err(s.build_rhs().cpu().numpy().reshape(-1, 3), want2)
    swapped = rel_err(oracle.collect_rhs_IP(ref.dx, topo, lam, mu, ref.IP_dNx, RF_ref, VF_ref, ref.n_k * 10), want2)
    print(f"{name}: RF {eR:.2e} VF {eV:.2e} abs; build_rhs {e1:.2e}, with random materials {e2:.2e} (mu and lam exchanged would be {swapped:.2e})")
    assert eR < 1e-9 and eV < 1e-9
    assert e1 < 1e-10 and e2 < 1e-10
    assert swapped > 100 * 1e-10


def _set_materials(s, mu, lam):
    """Overwrites the integration points' materials everywhere a substep reads them: IP_mu / IP_lam (CSR and persistent form) and the cell form's copy."""
    s.IP_mu.copy_(T(mu))
    s.IP_lam.copy_(T(lam))
    c = s._cells
    c["mu"].copy_((s.IP_mu[c["src"]] * c["valid"]).reshape(-1))
    c["lam"].copy_((s.IP_lam[c["src"]] * c["valid"]).reshape(-1))


@pytest.mark.parametrize("form", ("cells", "csr", "persistent"))
@pytest.mark.parametrize("name", SC.NAMES)
def test_one_iteration_with_unrelated_materials(refs, name, form):
    """The smallest unit in which each FORM of the substep reads its materials: one substep of one local/global iteration from the deformed state, with
    mu and lam overwritten by seeded values of 1e4 .. 1e7 per point (the system matrices stay: the step is then one linear solve of a right-hand side
    that weighs every point's R by its mu and its V F by its lam).  Against the oracle's step with the same values, at the 1e-6 the default
    decomposition is held to; with mu and lam exchanged the oracle's result differs by more than 100 times that."""
    r = refs[name]
    ref = r["ref"]
    rng = np.random.default_rng(11)
    mu, lam = 10.0 ** rng.uniform(4, 7, ref.n_IP), 10.0 ** rng.uniform(4, 7, ref.n_IP)

    def oracle_step(m, l):
        st = dict(ref.state(), iters=1, IP_mu=m, IP_lam=l, dof=r["dof"].copy(), dof_vel=r["vel"].copy())
        oracle.stepforward(st)
        return st["dof"] - ref.dof_rest
    want, other = oracle_step(mu, lam), oracle_step(lam, mu)
    assert not ref.dof_f.any() and np.isfinite(want).all()
    s = _sim(r["cloud"], form)
    s.iters = 1
    s.dof.copy_(T(r["dof"].reshape(-1)))
    s.dof_vel.copy_(T(r["vel"].reshape(-1)))
    _set_materials(s, mu, lam)
    s.stepforward()
    torch.cuda.synchronize()
    assert form != "persistent" or (s._coop is not None and not s.persistent_timed_out())
    got = (s.dof - s.dof_rest).cpu().numpy().reshape(-1, 3)
    e, gap = rel_err(got, want), rel_err(other, want)
    print(f"{name} {form}: one iteration with unrelated materials vs the oracle {e:.2e} (mu and lam exchanged: {gap:.2e})")
    assert gap > 100 * 1e-6
    assert e < 1e-6


# ------------------------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_trajectory_against_the_oracle(refs, name, form):
    """Eight substeps, the pick force applied before substep 2, changed before 5, cleared before 6: the project's bars (displacements 1e-4 relative;
    get_IP_info: pos 1e-5 abs, F 1e-4 abs, dF 1e-4 rel), and for the forms with the default decomposition the 1e-6 of
    test_gpu_persistent.test_persistent_substep_full_size_against_the_oracle_and_reproducible."""
    r = refs[name]
    got = _run(refs, name, form)
    worst = 0.0
    for k, (x, y) in enumerate(zip(got["traj"], r["traj"])):
        e = rel_err(x, y)
        worst = max(worst, e)
        assert e < 1e-4, (name, form, k, e)
        assert form == "mcadams" or e < 1e-6, (name, form, k, e)
    ev = rel_err(got["vel"], r["vel"])
    (p1, F1, dF1), (p2, F2, dF2) = got["info"], r["info"]
    print(f"{name} {form}: worst displacement error vs the oracle {worst:.2e} (bar {1e-4 if form == 'mcadams' else 1e-6:g}), velocity {ev:.2e}; "
          f"get_IP_info pos {np.abs(p1 - p2).max():.2e} abs, F {np.abs(F1 - F2).max():.2e} abs, dF {rel_err(dF1, dF2):.2e} rel")
    assert np.abs(p1 - p2).max() < 1e-5 and np.abs(F1 - F2).max() < 1e-4 and rel_err(dF1, dF2) < 1e-4
    ref = r["ref"]
    assert np.abs(p2 - ref.IP_pos.numpy()).max() > 1e-3                                 # the configuration really moved
    det = np.linalg.det(F2.reshape(-1, 3, 3).astype(np.float64))
    assert 0.9 < det.min() and det.max() < 1.1                                          # ... and stayed a sane elastic state


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_forms_agree_among_themselves(refs, name):
    """Cell, CSR and persistent form on one cloud, substep by substep: test_gpu_persistent.py's 1e-8 of the displacements — but for the cell form on the
    beam (FORM_BAR_BEAM_CELLS)."""
    runs = {f: _run(refs, name, f) for f in ("cells", "csr", "persistent")}
    pairs = (("cells", "csr"), ("cells", "persistent"), ("csr", "persistent"))
    worst = {p: max(rel_err(x, y) for x, y in zip(runs[p[0]]["traj"], runs[p[1]]["traj"])) for p in pairs}
    bars = {p: FORM_BAR_BEAM_CELLS if name == "beam" and "cells" in p else FORM_BAR for p in pairs}
    for p in pairs:
        print(f"{name}: {p[0]} vs {p[1]}: worst relative difference of the displacements {worst[p]:.2e} (bar {bars[p]:g})")
    for p in pairs:
        assert worst[p] < bars[p], (name, p, worst[p])


def test_cell_form_replayed_from_a_graph_equals_eager_steps(refs):
    """The beam's cell form captured and replayed three times against eager substeps of a second simulator, bit for bit: the arrival counters of
    kernels that collect from two chunks of one cell re-arm inside a replay as they do between launches."""
    cloud = refs["beam"]["cloud"]
    a, b = _sim(cloud), _sim(cloud)
    assert int((a._cells["tab"][:, 0] == SC.CHUNK).sum()) >= 1 and a._cells["n_chunks"] > len(np.unique(SC.cell_of_ip(a)))
    for s in (a, b):
        SC.run_schedule(s, "beam", steps=3)             # the force is on from substep 2
    assert torch.equal(a.dof, b.dof) and torch.equal(a.dof_vel, b.dof_vel)
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=st):
        a.stepforward()
    with torch.cuda.stream(st):
        for _ in range(3):
            g.replay()
    st.synchronize()
    for _ in range(3):
        b.stepforward()
    torch.cuda.synchronize()
    assert torch.equal(a.dof, b.dof) and torch.equal(a.dof_vel, b.dof_vel)
    assert float((a.dof - a.dof_rest).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ points that repeat a kernel
def test_update_pos_and_the_mesh_warp_on_stray_points(refs):
    """two_blocks has free points whose pts_kernel row names kernel 0 several times, some of them with a weight on it.  Simulator.update_pos() and
    pn_sim_warp_points over the cloud's own rows (a PointBinding with the explicit topology pts_kernel) against the oracle's update_pos on the
    deformed state, and the normals against the fp64 restatement over the ORACLE's tables; test_gpu_warp_points.py's bars."""
    from pienerf_amd.simulator import binding as B
    from test_gpu_warp_points import NRM_TOL, POS_TOL, _unit_normals
    r = refs["two_blocks"]
    ref, cloud = r["ref"], r["cloud"]
    s = _sim(cloud)
    s.dof.copy_(T(r["dof"].reshape(-1)))
    rest = np.asarray(cloud["pos"], np.float64)
    topo = ref.pts_kernel.numpy()
    stray = SC.repeated_rows(topo) & ~ref.is_pin.numpy()
    weight = np.abs(ref.pts_Nx).sum(-1)                                                 # [n, 8]
    heavy = [i for i in np.nonzero(stray)[0] if (weight[i][topo[i] == np.bincount(topo[i]).argmax()] > 0).sum() >= 2]
    want = ref.update_pos()
    assert stray.sum() >= 40 and len(heavy) >= 1 and np.abs(want - rest)[stray].max() > 1e-4
    n0 = _unit_normals(len(rest), 4)
    b = B.PointBinding(s, rest, s.pts_kernel, n0)
    pos, nrm = b.warp()
    want_p, want_n = B.warp_torch(ref.pts_kernel, torch.from_numpy(ref.pts_Nx), torch.from_numpy(ref.pts_dNx), n0, torch.from_numpy(r["dof"].reshape(-1)))
    e_warp = np.abs(pos.cpu().numpy().astype(np.float64) - want)
    e_nrm = float((nrm.cpu().to(torch.float64) - want_n.to(torch.float64)).abs().max())
    assert np.abs(want_p.numpy().astype(np.float64) - want).max() <= 6e-8                # the restatement is the oracle's update_pos, rounded once
    got = s.update_pos().cpu().numpy()
    e_pos = np.abs(got - want)
    print(f"two_blocks: {int(stray.sum())} free points repeat a kernel ({len(heavy)} with weight on it): update_pos {e_pos.max():.2e} ({e_pos[stray].max():.2e} on "
          f"them), warp {e_warp.max():.2e} ({e_warp[stray].max():.2e}), normals {e_nrm:.2e}")
    assert e_pos.max() <= POS_TOL and e_warp.max() <= POS_TOL and e_nrm <= NRM_TOL


def test_pin_term_with_repeated_kernels(refs):
    """pn_sim_pins_rhs on the beam (64 of its 128 pins repeat a kernel: their runs of the per-kernel CSR hold one pin several times) under a scripted
    translation plus rotation plus offsets, against the np.add.at restatement of tests/test_pins_host.py over the ORACLE's tables; that file's and
    test_gpu_pins.py's bar."""
    from test_pins_host import oracle_pins, pin_term, pin_u
    r = refs["beam"]
    ref = r["ref"]
    vid, kern, Nx, X = oracle_pins(ref)
    assert len(vid) == 128 and int(SC.repeated_rows(kern).sum()) == 64
    s = _sim(r["cloud"]).enable_pin_motion()
    assert s.n_pin == 128 and np.array_equal(s.pin_kernel.cpu().numpy(), kern)
    g = s.rhs_gravity.clone()
    off = np.random.default_rng(5).normal(scale=0.02, size=X.shape)
    m = dict(translate=((0.05, 0.02, -0.03), 4.0, 0.3), rotate=((0.2, 1.0, -0.1), 12.0, 3.0, 0.5, X.mean(axis=0) + 0.1), offsets=off)
    s.set_pin_offsets(off)
    s.set_pin_motion(translate=m["translate"], rotate=m["rotate"])
    worst = 0.0
    for k in (0, 1, 37):
        s.reset_pin_clock(k)
        got = s._enqueue_pin_rhs().clone()
        want = pin_term(ref.n_k, ref.stiff, kern, Nx, pin_u(X, (k + 1) * ref.dt, **m))
        e = rel_err((got - g).cpu().numpy().reshape(-1, 3), want)
        worst = max(worst, e)
        assert np.abs(want).max() > 1.0 and e < 1e-12, (k, e)
    print(f"beam: rhs_ext - rhs_gravity vs numpy over the oracle's tables: worst rel err {worst:.2e}")
    assert torch.equal(s.rhs_gravity, g)


# ------------------------------------------------------------------------------------------------ diagnostics
def test_diagnostics_on_the_deformed_beam(refs):
    """pn_sim_diagnostics on the oracle's deformed state and velocity against tests/diagnostics_reference.py at test_gpu_diagnostics.py's bounds; the
    elastic energy of the same state with mu and lam exchanged lies more than 100 bounds away."""
    import diagnostics_reference as R
    from test_gpu_diagnostics import _compare, _dev
    r = refs["beam"]
    s = _sim(r["cloud"])
    tab = R.tables_from(s)
    d, w = _dev(r["dof"]), _dev(r["vel"])
    got, want, P = _compare(s, tab, d, w, "deformed beam")
    assert got["elastic"] > 0 and got["kinetic"] > 0 and got["nonfinite"] == 0 and got["inverted"] == 0
    _, tol = R.row(P)
    other, _ = R.row(R.per_point(dict(tab, mu=tab["lam"], lam=tab["mu"]), r["dof"], r["vel"]))
    gap = abs(other["elastic"] - got["elastic"])
    print(f"elastic energy {got['elastic']:.6e}; with mu and lam exchanged {other['elastic']:.6e}: {gap / tol['elastic']:.3g} bounds away")
    assert gap > 100 * tol["elastic"]
