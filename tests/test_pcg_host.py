"""Simulator(solver='pcg') on the CPU: the block-sparse system precompute() builds against the dense path's matrices, what the constructor refuses, the
command line, and the facts about the numpy reference solve (tests/pcg_reference.py) that the bars of tests/test_gpu_pcg.py rest on.  No kernel is
launched.  Clouds: tests/sim_clouds.py's beam and two_blocks at kres 7 and 11 (54 .. 225 kernels: rows of 27 blocks and rows of a few, inactive kernels
at kres 11, pinned points that repeat a kernel, gravity's two zero columns)."""
import numpy as np
import pytest
import torch

import pcg_reference as R
import sim_clouds as SC

CASES = [(name, kres) for name in SC.NAMES for kres in R.KRES]
NONZERO_BLOCKS = {("beam", 7): (27, 14.2), ("beam", 11): (23, 11.2), ("two_blocks", 7): (27, 11.7), ("two_blocks", 11): (23, 10.9)}   # per active row: max, mean


def cpu_simulator(cloud, kres=7, solver="pcg", **kw):
    """A Simulator on the CPU up to precompute() (tests/test_sim_clouds_host.py: cpu_simulator), with the kernel grid and the solver given."""
    from pienerf_amd.simulator.solver import Simulator
    o = SC.opt()
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False, kres=kres, solver=solver, **kw)
    s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


@pytest.fixture(scope="module")
def built(monkeypatch_module_env):
    """(name, kres) -> dict(cloud, sim: the CPU Simulator with solver='pcg', ref: the OracleSimulator, sys: its system in block-sparse rows); built once."""
    out = {}
    for name, kres in CASES:
        cloud = SC.make(name)
        ref = R.make_oracle_sim(cloud, kres)
        out[(name, kres)] = dict(cloud=cloud, sim=cpu_simulator(cloud, kres), ref=ref, sys=R.system_from_oracle(ref))
    return out


@pytest.fixture(scope="module")
def monkeypatch_module_env():
    """The cell form whatever PN_SIM_FORM / PN_SIM_COOP say in the caller's environment, for this module."""
    mp = pytest.MonkeyPatch()
    mp.delenv("PN_SIM_FORM", raising=False)
    mp.delenv("PN_SIM_COOP", raising=False)
    yield mp
    mp.undo()


# ------------------------------------------------------------------------------------------------ the block-sparse system
@pytest.mark.parametrize("name,kres", CASES)
def test_bsr_system_against_the_dense_path(built, name, kres):
    """Densified A and M equal what the dense path assembles (gmls.assemble_IP_matrix, add_pin_penalty, +1e-3 on the active diagonal) to 1e-13 of the
    largest entry — the addends are the same, only the order of summation differs; nothing of the dense matrices lies outside the pattern; the pattern is
    symmetric, sorted, has its diagonal and is the union the oracle's topology gives; `active` is the dense path's rule."""
    from pienerf_amd.simulator import gmls
    b = built[(name, kres)]
    s, ref = b["sim"], b["ref"]
    n_k, dim = s.n_k, s.n_k * 10
    rowptr, col = s.bsr_rowptr.numpy(), s.bsr_col.numpy()
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and rowptr.shape == (n_k + 1,) and rowptr[0] == 0 and rowptr[-1] == len(col)
    assert s.bsr_A.shape == s.bsr_M.shape == (len(col), 10, 10) and s.bsr_Dinv.shape == (n_k, 10, 10) and s.bsr_active.dtype == torch.int32
    pat = np.zeros((n_k, n_k), bool)
    for k in range(n_k):
        c = col[rowptr[k]:rowptr[k + 1]]
        assert (np.diff(c) > 0).all() and k in c
        pat[k, c] = True
    assert np.array_equal(pat, pat.T)
    assert np.array_equal(rowptr, b["sys"]["rowptr"]) and np.array_equal(col, b["sys"]["col"])
    cnt = np.diff(rowptr)
    coupled = np.zeros((n_k, n_k), bool)      # pairs some integration point couples: what the pattern holds beyond them comes from pins and the diagonal
    tk = s.IP_kernel.numpy()
    for i in range(8):
        for j in range(8):
            coupled[tk[:, i], tk[:, j]] = True
    print(f"{name} kres {kres}: n_k {n_k}, active {int(s.bsr_active.sum())}, nnzb {len(col)}, blocks per row max {cnt.max()} mean {cnt.mean():.1f} "
          f"(from integration points alone: max {coupled.sum(1).max()} mean {coupled.sum(1).mean():.1f})")
    assert coupled.sum(1).max() == 27 and cnt.max() <= 28 and cnt.min() >= 1 and (cnt < 27).any()
    assert not (coupled & ~pat).any()
    # the numerically non-zero blocks of the active kernels' rows (a pair both of whose weights vanish is in the union but holds zeros): max / mean as measured
    nz = np.add.reduceat((np.abs(s.bsr_A.numpy()).max(axis=(1, 2)) > 0).astype(np.int64), rowptr[:-1].astype(np.int64))[s.bsr_active.numpy().astype(bool)]
    print(f"  non-zero blocks per active row: max {nz.max()} mean {nz.mean():.1f}")
    assert (int(nz.max()), round(float(nz.mean()), 1)) == NONZERO_BLOCKS[(name, kres)]
    # the dense path's matrices
    vid = torch.nonzero(s.is_pin).reshape(-1)
    mat = gmls.assemble_IP_matrix(dim, s.dx, s.dt, s.IP_kernel, s.IP_mu, s.IP_lam, s.IP_rho, s.IP_Nx, s.IP_dNx, s.IP_ddNx)
    mat = gmls.add_pin_penalty(mat, s.stiff, vid, s.pts_kernel, s.pts_Nx)
    active = torch.nonzero(mat.diagonal()[0::10] > 0.0).reshape(-1)
    assert torch.equal(active, s.active_kernels) and np.array_equal(active.numpy(), ref.active)
    assert np.array_equal(np.nonzero(s.bsr_active.numpy())[0], ref.active)
    assert (kres == 7) or len(ref.active) < n_k                                   # kres 11 has inactive kernels
    lst = (active[:, None] * 10 + torch.arange(10)[None, :]).reshape(-1)
    mat[lst, lst] += 1e-3
    zero = torch.zeros_like(s.IP_mu)
    mass = gmls.assemble_IP_matrix(dim, s.dx, s.dt, s.IP_kernel, zero, zero, s.IP_rho, s.IP_Nx, s.IP_dNx, s.IP_ddNx)
    for blocks, dense, label in ((s.bsr_A, mat, "A"), (s.bsr_M, mass, "M")):
        got = R.bsr_to_dense(rowptr, col, blocks.numpy())
        e = np.abs(got - dense.numpy()).max() / np.abs(dense.numpy()).max()
        _, outside = R.dense_to_bsr(dense.numpy(), rowptr, col)
        print(f"  {label}: densified vs dense path {e:.2e} of the largest entry; largest dense entry outside the pattern {outside:g}")
        assert e <= 1e-13 and outside == 0.0
    # ... and the oracle's, at the bar tests/test_sim_clouds_host.py holds Mmat to
    assert np.abs(s.bsr_A.numpy() - b["sys"]["A"]).max() <= 1e-12 * np.abs(b["sys"]["A"]).max()
    # Dinv: the inverse of the active diagonal blocks, zeros elsewhere
    diag = np.array([rowptr[k] + int(np.nonzero(col[rowptr[k]:rowptr[k + 1]] == k)[0][0]) for k in range(n_k)])
    D, A = s.bsr_Dinv.numpy(), s.bsr_A.numpy()
    on = s.bsr_active.numpy().astype(bool)
    assert (D[~on] == 0).all() and np.abs(np.einsum("kij,kjl->kil", D[on], A[diag[on]]) - np.eye(10)).max() < 1e-9
    assert (A[diag[~on]] == 0).all()                                               # an inactive kernel's diagonal gets no 1e-3


def test_pcg_builds_no_dense_matrix(monkeypatch, monkeypatch_module_env):
    """With solver='pcg' gmls.assemble_IP_matrix is never called and no attribute of the simulator is a [dim, dim] tensor; the dense names raise."""
    from pienerf_amd.simulator import gmls

    def boom(*a, **k):
        raise AssertionError("assemble_IP_matrix called with solver='pcg'")
    monkeypatch.setattr(gmls, "assemble_IP_matrix", boom)
    monkeypatch.setattr(gmls, "inverse_spd", boom)
    s = cpu_simulator(SC.make("beam"), 7)
    dim = s.n_k * 10
    for k, v in vars(s).items():
        assert not (torch.is_tensor(v) and v.dim() == 2 and tuple(v.shape) == (dim, dim)), k
    assert s.solver == "pcg" and s.pcg_tol == 1e-10 and s.pcg_max_iters == 576
    for name in ("Ainv", "Mmat", "global_matrix", "mass_matrix_invt2"):
        with pytest.raises(RuntimeError, match="solver='pcg'"):
            getattr(s, name)
    assert s.enable_persistent() is False and s.persistent is False
    with pytest.raises(AttributeError):
        s.no_such_attribute


def test_dense_default_is_untouched(monkeypatch_module_env):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(device="cpu", persistent=False)
    assert s.solver == "dense" and s.kres == 7 and not hasattr(s, "bsr_A")
    d = cpu_simulator(SC.make("beam"), 7, solver="dense")
    assert d.Ainv.shape == d.Mmat.shape == (d.n_k * 10, d.n_k * 10) and not hasattr(d, "bsr_A")


def test_rejected_combinations(monkeypatch):
    from pienerf_amd.simulator.solver import Simulator
    monkeypatch.delenv("PN_SIM_FORM", raising=False)
    monkeypatch.delenv("PN_SIM_COOP", raising=False)
    with pytest.raises(ValueError, match="pcg"):
        Simulator(device="cpu", solver="pcg", persistent=True)
    with pytest.raises(ValueError, match="solver"):
        Simulator(device="cpu", solver="cg", persistent=False)
    for bad in (1, 0):
        with pytest.raises(ValueError, match="kres"):
            Simulator(device="cpu", kres=bad, persistent=False)
    with pytest.raises(ValueError, match="pcg_max_iters"):
        Simulator(device="cpu", solver="pcg", persistent=False, pcg_max_iters=0)
    monkeypatch.setenv("PN_SIM_FORM", "csr")
    with pytest.raises(ValueError, match="PN_SIM_FORM"):
        Simulator(device="cpu", solver="pcg", persistent=False)
    Simulator(device="cpu", solver="dense", persistent=False)   # the CSR form keeps the dense solver
    monkeypatch.delenv("PN_SIM_FORM")
    monkeypatch.setenv("PN_SIM_COOP", "1")
    with pytest.raises(ValueError, match="persistent"):
        Simulator(device="cpu", solver="pcg")
    monkeypatch.delenv("PN_SIM_COOP")
    s = Simulator(device="cpu", solver="pcg", kres=2)
    assert s.enable_persistent() is False and s.persistent is False


def test_main_render_parses_the_solver_options():
    from pienerf_amd import main_render
    a = main_render.parser().parse_args([])
    assert (a.sim_kres, a.sim_solver, a.pcg_tol, a.pcg_max_iters) == (7, "dense", 1e-10, 576)
    a = main_render.parser().parse_args(["--sim_kres", "15", "--sim_solver", "pcg", "--pcg_tol", "1e-8", "--pcg_max_iters", "300"])
    assert (a.sim_kres, a.sim_solver, a.pcg_tol, a.pcg_max_iters) == (15, "pcg", 1e-8, 300)
    with pytest.raises(SystemExit):
        main_render.parser().parse_args(["--sim_solver", "cholesky"])
    from pienerf_amd import scene
    assert not {"sim_kres", "sim_solver", "pcg_tol", "pcg_max_iters"} & set(scene.default_opt())   # fixtures compare that dict


# ------------------------------------------------------------------------------------------------ the reference solve
@pytest.mark.parametrize("name,kres", CASES)
def test_reference_solve_facts(built, name, kres):
    """What tests/test_gpu_pcg.py's bars rest on, on the reference alone, cold start, cap 512: a zero column gives exact zeros in 0 iterations; gravity and
    the point load converge within 255 iterations at 1e-10 (seeded noise, which excites every mode, is printed: 258 at two_blocks kres 11, inside the
    cap); the true residual stays within RESIDUAL_FACTOR of the tolerance; a column's bits do not depend on the other columns' right-hand sides; a
    converged x0 comes back unchanged in 0 iterations."""
    b = built[(name, kres)]
    y = b["sys"]
    args = (y["rowptr"], y["col"], y["A"], y["Dinv"], y["active"])
    worst = {}
    for label, B in R.rhs_cases(b["ref"], name).items():
        for tol in (1e-8, 1e-10, 1e-12):
            X, it, flag = R.pcg(*args, B, np.zeros_like(B), tol, R.CAP)
            res = R.true_residual(y["rowptr"], y["col"], y["A"], y["active"], B, X)
            zero = ~np.any(B, axis=0)
            print(f"{name} kres {kres} {label} tol {tol:g}: iterations {it.tolist()}, true residual / tol {np.round(res / tol, 3).tolist()}")
            assert (flag == R.CONVERGED).all() and it.max() <= R.CAP
            assert (it[zero] == 0).all() and not X[:, zero].any() and (it[~zero] > 0).all()
            if label == "gravity":
                assert zero.tolist() == [True, False, True]
            if tol == 1e-10 and label != "noise":
                assert it.max() <= 255
            assert np.nanmax(res) <= R.RESIDUAL_FACTOR[tol] * tol
            worst[tol] = max(worst.get(tol, 0.0), float(np.nanmax(res) / tol))
            assert not X[np.repeat(y["active"] == 0, 10)].any()
            if tol == 1e-10:
                # a converged x0: the start forms the TRUE residual of x0, which at kres 11 can sit a few percent above tol |b| where the recurrence had
                # stopped (printed above: up to 1.11 tol here, 1.42 tol on the device), so "converged" is taken at the nearest round tolerance that
                # x0's true residual meets: 2 tol
                X2, it2, _ = R.pcg(*args, B, X, 2 * tol, R.CAP)
                assert np.array_equal(X2, X) and not it2.any()
                for c in np.nonzero(~zero)[0]:                                      # column c alone
                    B1 = np.zeros_like(B)
                    B1[:, c] = B[:, c]
                    X1, it1, _ = R.pcg(*args, B1, np.zeros_like(B), tol, R.CAP)
                    assert np.array_equal(X1[:, c], X[:, c]) and it1[c] == it[c] and it1.sum() == it[c]
        # the cap: the current x stands, the columns count as unconverged
    X3, it3, flag3 = R.pcg(*args, R.rhs_cases(b["ref"], name)["noise"], np.zeros_like(B), 1e-10, 3)
    assert it3.tolist() == [3, 3, 3] and (flag3 == 0).all() and np.isfinite(X3).all()
    print(f"{name} kres {kres}: largest true residual / tol {worst} (recorded: {R.RESIDUAL_MEASURED})")
    for tol, w in worst.items():
        assert w <= 1.05 * R.RESIDUAL_MEASURED[tol]   # the record in pcg_reference.py is this measurement


@pytest.mark.parametrize("name,kres", CASES)
def test_trajectory_bar_is_measured_and_discriminates(built, name, kres):
    """The composed oracle trajectory (8 scheduled substeps) with the reference PCG against the one with the dense product: the largest relative
    displacement difference is within the recorded TRAJ_MEASURED, no solve is unconverged and none needs more than 255 iterations; with max_iters = 5
    the trajectory misses the GPU tests' bar (10 x TRAJ_MEASURED) by orders of magnitude."""
    b = built[(name, kres)]
    dense, _ = R.trajectory(b["ref"], name, "dense")
    assert max(np.abs(d).max() for d in dense) > 1e-3                              # the configuration really moved
    got, sim = R.trajectory(b["ref"], name, "pcg", b["sys"])
    e = R.worst_rel(got, dense)
    its = np.array(sim.iterations)
    few, sim5 = R.trajectory(b["ref"], name, "pcg", b["sys"], max_iters=5, steps=3)   # (three substeps are enough to miss it: compared with the dense one's first three)
    e5 = R.worst_rel(few, dense)
    print(f"{name} kres {kres}: reference PCG vs dense product {e:.3e} relative (recorded largest {R.TRAJ_MEASURED:g}); iterations max {its.max()}, "
          f"mean {its.mean():.1f}; with max_iters = 5: {e5:.3e}, {sim5.unconverged} unconverged columns")
    assert sim.unconverged == 0 and its.shape == (SC.STEPS * SC.SIM_ITERS, 3) and its.max() <= 255
    assert e <= R.TRAJ_MEASURED
    assert e5 > 100 * R.TRAJ_BAR and sim5.unconverged > 0
