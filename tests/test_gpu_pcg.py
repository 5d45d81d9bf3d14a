"""Simulator(solver='pcg') on the GPU (csrc/pn_sim_pcg.h): the block-sparse product, the solve against the numpy reference of tests/pcg_reference.py and
against a host fp64 residual, and eight scheduled substeps against solver='dense' on the same device — free, on a floor, run twice, and replayed from a
graph.  The bars are measured on the CPU by tests/test_pcg_host.py (pcg_reference.RESIDUAL_FACTOR, TRAJ_BAR).  Clouds: sim_clouds' beam and two_blocks at
kres 7 and 11."""
import numpy as np
import pytest
import torch

import pcg_reference as R
import sim_clouds as SC
from conftest import rel_err
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

CASES = [(name, kres) for name in SC.NAMES for kres in R.KRES]


def _sim(cloud, kres, solver, **kw):
    from pienerf_amd.simulator.solver import Simulator
    o = SC.opt()
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device=DEV, persistent=False, svd="jacobi", kres=kres, solver=solver, pcg_max_iters=R.CAP, **kw)
    s.cell_form = True   # whatever PN_SIM_FORM says for the dense simulator; solver='pcg' refuses the CSR form itself
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


@pytest.fixture(scope="module")
def clouds():
    return {name: SC.make(name) for name in SC.NAMES}


_SIMS = {}


def _pcg_sim(clouds, name, kres):
    """One solver='pcg' simulator per case for the op-level tests (read only: they use its tables, not its state)."""
    if (name, kres) not in _SIMS:
        _SIMS[(name, kres)] = _sim(clouds[name], kres, "pcg")
    return _SIMS[(name, kres)]


def _host_system(s):
    return dict(rowptr=s.bsr_rowptr.cpu().numpy(), col=s.bsr_col.cpu().numpy(), A=s.bsr_A.cpu().numpy(), M=s.bsr_M.cpu().numpy(),
                Dinv=s.bsr_Dinv.cpu().numpy(), active=s.bsr_active.cpu().numpy())


def _rhs(s, name):
    """pcg_reference.rhs_cases from the simulator's own tables: gravity, the schedule's first pick force, seeded noise."""
    g = s.rhs_gravity.cpu().numpy().reshape(-1, 3)
    s.update_force(SC.load_point(s, name), torch.from_numpy(np.array(SC.LOAD[name][0])))
    load = s.dof_f.cpu().numpy().reshape(-1, 3).copy()
    s.clear_force()
    noise = np.random.default_rng(3).normal(size=g.shape) * np.abs(g).max()
    return dict(gravity=g, load=load, noise=noise)


def _solve(s, B, X0, tol, max_iters, fill=None):
    """pn_sim_pcg_solve on the simulator's system: (X, iterations [3], flags [3], totals [2]).  fill: what the work area holds on entry (None: whatever
    the allocation held)."""
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    X = T(np.array(X0, np.float64).reshape(-1)).clone()
    Bd = T(np.asarray(B, np.float64).reshape(-1))
    work = torch.empty(int(lib().pn_sim_pcg_work_doubles(s.n_k)), dtype=torch.float64, device=DEV)
    if fill is not None:
        work.fill_(fill)
    stats = torch.zeros(8, dtype=torch.int32, device=DEV)
    check(lib().pn_sim_pcg_solve(s.n_k, ptr(s.bsr_rowptr), ptr(s.bsr_col), ptr(s.bsr_A), ptr(s.bsr_Dinv), ptr(s.bsr_active), ptr(Bd), ptr(X), float(tol),
                                 int(max_iters), ptr(work), ptr(stats), stream_ptr()), "pcg_solve")
    torch.cuda.synchronize()
    st = stats.cpu().numpy()
    return X.cpu().numpy().reshape(-1, 3), st[2:5].copy(), st[5:8].copy(), st[:2].copy()


# ------------------------------------------------------------------------------------------------ the product
@pytest.mark.parametrize("name,kres", CASES)
def test_bsr_matvec3(clouds, name, kres):
    """pn_sim_bsr_matvec3 for A and M against the fp64 dense product of the densified matrix, row by row to 1e-13 of |row|_1 |x|_inf, and rhs_rest =
    build_rhs() + M dof, which initialize() forms with this product."""
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    s = _pcg_sim(clouds, name, kres)
    y = _host_system(s)
    rng = np.random.default_rng(17)
    X = rng.normal(size=(s.n_k * 10, 3))
    for label in ("A", "M"):
        dense = R.bsr_to_dense(y["rowptr"], y["col"], y[label])
        Y = torch.empty(s.n_k * 30, dtype=torch.float64, device=DEV)
        check(lib().pn_sim_bsr_matvec3(s.n_k, ptr(s.bsr_rowptr), ptr(s.bsr_col), ptr(getattr(s, "bsr_" + label)), ptr(T(X.reshape(-1))), ptr(Y), stream_ptr()),
              "bsr_matvec3")
        got = Y.cpu().numpy().reshape(-1, 3)
        bound = 1e-13 * np.abs(dense).sum(1)[:, None] * np.abs(X).max()
        err = np.abs(got - dense @ X)
        print(f"{name} kres {kres} {label}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
        assert np.abs(got - R.bsr_matvec3(y["rowptr"], y["col"], y[label], X)).max() <= bound.max()
    # rhs_rest = build_rhs() + M dof through the product, against the dense simulator's (tests/test_gpu_sim_clouds.py holds that one to the oracle at 1e-10)
    want = s.build_rhs().cpu().numpy().reshape(-1, 3) + R.bsr_to_dense(y["rowptr"], y["col"], y["M"]) @ s.dof_rest.cpu().numpy().reshape(-1, 3)
    assert rel_err(s.rhs_rest.cpu().numpy().reshape(-1, 3), want) < 1e-13


def test_momentum_mode_is_the_composition_of_its_parts(clouds):
    """One substep from a moving state with the force on: the momentum launch (mode 1 of k_bsr_matvec3: dof + dt vel formed on the fly, dof copied out)
    leaves M (dof + dt vel) + dof_f + rhs_gravity and dof_last in the cell form's work area; both against their parts computed on the host, the product
    to 1e-13 of |row|_1 |x|_inf.  The substep's velocity is (dof - dof_last) / dt * 0.998 of what it leaves."""
    name, kres = "beam", 11
    s = _sim(clouds[name], kres, "pcg")
    SC.run_schedule(s, name, steps=3)                      # a moving state with the force on
    dof, vel, f = (t.cpu().numpy().reshape(-1, 3).copy() for t in (s.dof, s.dof_vel, s.dof_f))
    s.stepforward()
    torch.cuda.synchronize()
    n3 = s.n_k * 30
    last, momentum = (s._cells_work[i * n3:(i + 1) * n3].cpu().numpy().reshape(-1, 3) for i in (0, 1))
    y = _host_system(s)
    M = R.bsr_to_dense(y["rowptr"], y["col"], y["M"])
    xt = dof + s.dt * vel
    want = M @ xt + f + s.rhs_gravity.cpu().numpy().reshape(-1, 3)
    bound = 1e-13 * (np.abs(M).sum(1)[:, None] * np.abs(xt).max() + np.abs(want))
    assert np.array_equal(last, dof) and np.abs(f).max() > 0 and np.abs(vel).max() > 0
    assert (np.abs(momentum - want) <= bound).all()
    assert rel_err(s.dof_vel.cpu().numpy().reshape(-1, 3), (s.dof.cpu().numpy().reshape(-1, 3) - dof) / s.dt * 0.998) <= 1e-15


# ------------------------------------------------------------------------------------------------ the solve
@pytest.mark.parametrize("name,kres", CASES)
def test_pcg_solve(clouds, name, kres):
    """pn_sim_pcg_solve from a cold start at 1e-8, 1e-10, 1e-12: every column converged, the true residual (host fp64) within the factor measured on the
    CPU, zero columns exact zeros in 0 iterations, iteration counts within a few of the reference's (another order of additions can move a stop);
    a converged x0 comes back bit for bit in 0 iterations; a column's bits do not depend on the other columns; max_iters = 3 leaves three unconverged
    columns with x within 1e-12 of the reference's third iterate."""
    s = _pcg_sim(clouds, name, kres)
    y = _host_system(s)
    args = (y["rowptr"], y["col"], y["A"], y["Dinv"], y["active"])
    cases = _rhs(s, name)
    for label, B in cases.items():
        zero = ~np.any(B, axis=0)
        for tol in (1e-8, 1e-10, 1e-12):
            X, it, flag, tot = _solve(s, B, np.zeros_like(B), tol, R.CAP)
            res = R.true_residual(y["rowptr"], y["col"], y["A"], y["active"], B, X)
            print(f"{name} kres {kres} {label} tol {tol:g}: iterations {it.tolist()}, true residual / tol {np.round(res / tol, 3).tolist()} "
                  f"(bar {R.RESIDUAL_FACTOR[tol]:g})")
            if tol == 1e-10 and label == "gravity":   # (one reference solve per case: seconds of numpy at kres 11)
                _, it_ref, _ = R.pcg(*args, B, np.zeros_like(B), tol, R.CAP)
                assert np.abs(it - it_ref).max() <= 8, (it, it_ref)
            assert (flag == R.CONVERGED).all() and tot.tolist() == [1, 0] and it.max() <= R.CAP
            assert (it[zero] == 0).all() and not X[:, zero].any() and (it[~zero] > 0).all()
            assert np.isfinite(X).all() and np.nanmax(res) <= R.RESIDUAL_FACTOR[tol] * tol
            assert not X[np.repeat(y["active"] == 0, 10)].any()
            if tol == 1e-10:
                # x0 = a converged x: the start forms x0's TRUE residual, which sits at up to 1.11 tol on the CPU (tests/test_pcg_host.py) and 1.42 tol
                # here (printed above) where the recurrence had stopped, so it is handed back at 2 tol
                assert np.nanmax(res) <= 1.5 * tol
                X2, it2, flag2, _ = _solve(s, B, X, 2 * tol, R.CAP)
                assert np.array_equal(X2, X) and not it2.any() and (flag2 == R.CONVERGED).all()
                for c in np.nonzero(~zero)[0]:                                       # column c with the other right-hand sides zero
                    B1 = np.zeros_like(B)
                    B1[:, c] = B[:, c]
                    X1, it1, _, _ = _solve(s, B1, np.zeros_like(B), tol, R.CAP)
                    assert np.array_equal(X1[:, c], X[:, c]) and it1[c] == it[c] and it1.sum() == it[c]
    B = cases["noise"]
    X3, it3, flag3, tot3 = _solve(s, B, np.zeros_like(B), 1e-10, 3)
    Xr, itr, _ = R.pcg(*args, B, np.zeros_like(B), 1e-10, 3)
    e = rel_err(X3, Xr)
    print(f"{name} kres {kres}: after max_iters = 3 vs the reference's third iterate {e:.2e}")
    assert it3.tolist() == itr.tolist() == [3, 3, 3] and (flag3 == 0).all() and tot3.tolist() == [1, 3] and np.isfinite(X3).all()
    assert e <= 1e-12


@pytest.mark.parametrize("name", SC.NAMES)
def test_solve_does_not_depend_on_what_the_work_area_held(clouds, name):
    """kres 11 has active rows with inactive column kernels (340 such blocks on the beam, 290 on two_blocks, all zeros in value), whose entries of p no
    launch writes, and gravity has two columns frozen from the start, whose p is never written either.  A work area filled with NaN, with +inf and with
    zeros gives the same bits, iteration counts and flags: nothing of it that the solve has not written enters the arithmetic (0 x NaN would be NaN)."""
    s = _pcg_sim(clouds, name, 11)
    y = _host_system(s)
    row = np.repeat(np.arange(s.n_k), np.diff(y["rowptr"]))
    mixed = (y["active"][row] != 0) & (y["active"][y["col"]] == 0)
    assert mixed.sum() >= 100 and not y["A"][mixed].any()
    for label, B in _rhs(s, name).items():
        want = _solve(s, B, np.zeros_like(B), 1e-10, R.CAP, fill=0.0)
        assert (want[2] == R.CONVERGED).all() and want[1].max() > 100
        for fill in (float("nan"), float("inf")):
            got = _solve(s, B, np.zeros_like(B), 1e-10, R.CAP, fill=fill)
            assert np.array_equal(got[0], want[0]) and np.isfinite(got[0]).all(), (label, fill)
            assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), (label, fill, got[1], got[2])


def test_substep_does_not_depend_on_what_the_work_area_held(clouds):
    """The same through Simulator.stepforward(): the simulator's PCG work area overwritten with NaN between initialize() and the first substep."""
    a, b = _sim(clouds["two_blocks"], 11, "pcg"), _sim(clouds["two_blocks"], 11, "pcg")
    a._pcg_work.fill_(float("nan"))
    b._pcg_work.zero_()
    for s in (a, b):
        SC.run_schedule(s, "two_blocks", steps=3)
    torch.cuda.synchronize()
    assert torch.equal(a.dof, b.dof) and torch.equal(a.dof_vel, b.dof_vel) and bool(torch.isfinite(a.dof).all())
    assert a.pcg_stats()["unconverged"] == 0 and np.array_equal(a.pcg_stats()["iterations"], b.pcg_stats()["iterations"])
    # pcg_stats() reports the rows of the local/global iterations the last substep ran, also after iters was lowered
    a.iters = 2
    a.stepforward()
    st = a.pcg_stats()
    assert st["iterations"].shape == (2, 3) and st["iterations_max"] == st["iterations"].max() and st["solves"] == 3 * SC.SIM_ITERS + 2


# ------------------------------------------------------------------------------------------------ substeps
_RUNS = {}


def _run(clouds, name, kres, solver, floor=False):
    """The eight scheduled substeps once per (case, solver): displacements behind every substep, final velocity, statistics."""
    key = (name, kres, solver, floor)
    if key not in _RUNS:
        cloud = clouds[name]
        if floor:   # --unpin-style: nothing holds the object, it rests its weight on a floor just below its lowest integration points
            cloud = dict(cloud, pin=np.zeros_like(np.asarray(cloud["pin"])))
        s = _sim(cloud, kres, solver)
        if floor:
            s.enable_contact()
            s.add_plane((0.0, float(s.IP_pos[:, 1].min()) - 0.04, 0.0), (0.0, 1.0, 0.0))
        traj, touching, its = [], [], []

        def after(k, sim):
            traj.append((sim.dof - sim.dof_rest).cpu().numpy().reshape(-1, 3))
            if floor:
                touching.append(sim.contact_count())
            if solver == "pcg":
                its.append(sim.pcg_stats())
        SC.run_schedule(s, name, after_step=after)
        torch.cuda.synchronize()
        _RUNS[key] = dict(traj=traj, vel=s.dof_vel.cpu().numpy(), dof=s.dof.cpu().numpy(), touching=touching, stats=its, iters=int(s.iters))
    return _RUNS[key]


def _check_stats(run):
    last = run["stats"][-1]
    assert last["solves"] == SC.STEPS * run["iters"] and last["unconverged"] == 0
    for st in run["stats"]:
        assert st["iterations"].shape == (run["iters"], 3) and 0 < st["iterations_max"] <= R.CAP and st["iterations_max"] == st["iterations"].max()
    return max(st["iterations_max"] for st in run["stats"])


@pytest.mark.parametrize("name,kres", CASES)
def test_substeps_against_the_dense_solver(clouds, name, kres):
    """sim_clouds.run_schedule with solver='pcg' against solver='dense' on the GPU, substep by substep, at ten times the difference the reference PCG shows
    against the dense product on the CPU (pcg_reference.TRAJ_BAR; with max_iters = 5 the reference misses it by orders of magnitude)."""
    want, got = _run(clouds, name, kres, "dense"), _run(clouds, name, kres, "pcg")
    worst = R.worst_rel(got["traj"], want["traj"])
    most = _check_stats(got)
    print(f"{name} kres {kres}: pcg vs dense, worst relative displacement difference {worst:.3e} (bar {R.TRAJ_BAR:g}); CG iterations at most {most}")
    assert max(np.abs(d).max() for d in want["traj"]) > 1e-3
    assert worst <= R.TRAJ_BAR
    assert rel_err(got["vel"], want["vel"]) <= 100 * R.TRAJ_BAR   # a velocity is a difference of two displacements over dt = 1e-2


@pytest.mark.parametrize("name,kres", [("beam", 7), ("two_blocks", 11)])
def test_substeps_on_a_floor(clouds, name, kres):
    """The same comparison with every pin cleared and the body resting on a floor (enable_contact, add_plane): the contact stage writes the right-hand
    side chain, the solver sees only its sum."""
    want, got = _run(clouds, name, kres, "dense", floor=True), _run(clouds, name, kres, "pcg", floor=True)
    worst = R.worst_rel(got["traj"], want["traj"])
    most = _check_stats(got)
    print(f"{name} kres {kres} on a floor: pcg vs dense {worst:.3e} (bar {R.TRAJ_BAR:g}); in contact per substep {got['touching']}; CG iterations at most {most}")
    assert max(got["touching"]) > 0 and max(want["touching"]) > 0
    assert worst <= R.TRAJ_BAR


def test_two_runs_give_the_same_bits(clouds):
    a = _run(clouds, "beam", 11, "pcg")
    s = _sim(clouds["beam"], 11, "pcg")
    SC.run_schedule(s, "beam")
    torch.cuda.synchronize()
    assert np.array_equal(s.dof.cpu().numpy(), a["dof"]) and np.array_equal(s.dof_vel.cpu().numpy(), a["vel"])
    st = s.pcg_stats()
    assert np.array_equal(st["iterations"], a["stats"][-1]["iterations"]) and st["solves"] == a["stats"][-1]["solves"]


def test_substep_replayed_from_a_graph_equals_eager_steps(clouds):
    """One substep captured with torch.cuda.graph (a linear chain of plain launches, the early-exit flag inside it) and replayed three times against
    eager substeps of a second simulator, bit for bit."""
    a, b = _sim(clouds["beam"], 7, "pcg"), _sim(clouds["beam"], 7, "pcg")
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
    sa, sb = a.pcg_stats(), b.pcg_stats()
    assert sa["unconverged"] == sb["unconverged"] == 0 and np.array_equal(sa["iterations"], sb["iterations"])
