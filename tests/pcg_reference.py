"""numpy restatement of the simulator's block-sparse PCG global solve (pienerf_amd/csrc/pn_sim_pcg.h, include/pienerf_hip.h: pn_sim_pcg_solve): BSR <->
dense conversion, the product, the solve exactly as the header specifies it, and a CPU trajectory composed from the oracle's calc_elastic /
collect_rhs_IP / matvec3 whose global step is either the oracle's dense product or this solve.  A helper module like the other *_reference.py, not a
conftest.  Everything is fp64; the solve's reductions are numpy sums, so against the device only the order of additions differs."""
import numpy as np

import oracle
import sim_clouds as SC

CONVERGED, BROKEN = 1, 2
KRES = (7, 11)
CAP = 512                                  # max_iters of every test (the Simulator defaults to 576: DESIGN.md 4.19)

# --- measured on the CPU by tests/test_pcg_host.py, which asserts them; the GPU tests' bars rest on them ---------------------------------------------
# True residual |b - A x| / |b| of the reference solve against its tolerance, largest over both clouds, kres 7 and 11, the right-hand sides gravity, point
# load and seeded noise, cold start.  At 1e-8 and 1e-10 the recurrence residual is the true one (measured <= 1.11 tol): the factor 10 for recurrence
# drift holds.  At 1e-12 it does not at cond(A) ~ 1e10: the recurrence keeps shrinking while the true residual stalls at 6e-11 |b| (measured up to
# 63.6 tol), so that tolerance gets twice the measured ratio.
RESIDUAL_MEASURED = {1e-8: 0.97, 1e-10: 1.11, 1e-12: 63.6}
RESIDUAL_FACTOR = {1e-8: 10.0, 1e-10: 10.0, 1e-12: 2.0 * 63.6}
# Largest relative displacement difference over the 8 scheduled substeps between the composed oracle trajectory with the dense product and with the
# reference PCG (tol 1e-10, cap 512): beam 4.81e-8 (kres 7) and 6.72e-9 (11), two_blocks 1.39e-9 and 1.03e-8.  The GPU is allowed ten times the largest.
TRAJ_MEASURED = 4.82e-8
TRAJ_BAR = 10.0 * TRAJ_MEASURED


# ------------------------------------------------------------------------------------------------ BSR
def bsr_to_dense(rowptr, col, blocks):
    n_k = len(rowptr) - 1
    A = np.zeros((n_k, 10, n_k, 10))
    row = np.repeat(np.arange(n_k), np.diff(rowptr))
    A[row, :, np.asarray(col, np.int64), :] = np.asarray(blocks, np.float64)
    return A.reshape(n_k * 10, n_k * 10)


def dense_to_bsr(A, rowptr, col):
    """The blocks of dense `A` on the pattern, and the largest |entry| of A outside it."""
    n_k = len(rowptr) - 1
    A4 = np.asarray(A, np.float64).reshape(n_k, 10, n_k, 10)
    row = np.repeat(np.arange(n_k), np.diff(rowptr))
    c = np.asarray(col, np.int64)
    blocks = A4[row, :, c, :].copy()
    rest = np.abs(A4).max(axis=(1, 3))
    rest[row, c] = 0.0
    return blocks, float(rest.max())


def pattern_from_rows(n_k, *rows8):
    """rowptr, col of the union of all ordered kernel pairs of every row of the given [m, 8] tables, plus the diagonal (gmls.bsr_pattern, restated with sets)."""
    pairs = {(k, k) for k in range(n_k)}
    for rows in rows8:
        for r in {tuple(int(v) for v in r) for r in np.asarray(rows).reshape(-1, 8)}:
            pairs.update((a, b) for a in r for b in r)
    pairs = sorted(pairs)
    row = np.array([p[0] for p in pairs])
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_k))]).astype(np.int32)
    return rowptr, np.array([p[1] for p in pairs], np.int32)


def bsr_matvec3(rowptr, col, blocks, X):
    n_k = len(rowptr) - 1
    prod = np.einsum("bij,bjc->bic", blocks, np.asarray(X, np.float64).reshape(n_k, 10, 3)[np.asarray(col, np.int64)])
    return np.add.reduceat(prod, np.asarray(rowptr[:-1], np.int64), axis=0).reshape(n_k * 10, 3)   # (every row holds its diagonal block: no empty row)


# ------------------------------------------------------------------------------------------------ the solve
def pcg(rowptr, col, A, Dinv, active, B, X0, tol, max_iters):
    """(X, iterations [3], flags [3]): per column r = b - A x0; |b| = 0 -> x = 0, converged, 0 iterations; stop at |r|_2 <= tol |b|_2 on the recurrence
    residual, tested before the first iteration too; a stopped column is frozen; p.Ap <= 0 or not finite freezes it as BROKEN; after max_iters the current x
    stands with flag 0.  Rows and columns of inactive kernels are left out (their x is 0)."""
    n_k = len(rowptr) - 1
    on = np.repeat(np.asarray(active).astype(bool), 10)[:, None]
    X = np.where(on, np.array(X0, np.float64).reshape(n_k * 10, 3), 0.0)
    Bm = np.where(on, np.asarray(B, np.float64).reshape(n_k * 10, 3), 0.0)

    def mv(V):
        return np.where(on, bsr_matvec3(rowptr, col, A, V), 0.0)

    def prec(R):
        return np.einsum("kij,kjc->kic", Dinv, R.reshape(n_k, 10, 3)).reshape(n_k * 10, 3)

    r = Bm - mv(X)
    z = prec(r)
    p = z.copy()
    bb, rr, rz = (Bm * Bm).sum(0), (r * r).sum(0), (r * z).sum(0)
    flag, iters = np.zeros(3, np.int64), np.zeros(3, np.int64)

    def test():
        for c in range(3):
            if flag[c] == 0 and np.sqrt(rr[c]) <= tol * np.sqrt(bb[c]):
                flag[c] = CONVERGED
    for c in range(3):
        if bb[c] == 0.0:
            X[:, c] = 0.0
            flag[c] = CONVERGED
    test()
    rz_old = rz.copy()
    for k in range(max_iters):
        run = flag == 0
        if not run.any():
            break
        if k > 0:
            with np.errstate(all="ignore"):
                beta = rz / rz_old
            p[:, run] = z[:, run] + beta[run][None, :] * p[:, run]
        Ap = mv(p)
        pAp = (p * Ap).sum(0)
        for c in range(3):
            if run[c] and (not pAp[c] > 0.0 or not np.isfinite(pAp[c])):
                flag[c] = BROKEN
        run = flag == 0
        if not run.any():
            break
        alpha = np.zeros(3)
        alpha[run] = rz[run] / pAp[run]
        X[:, run] += alpha[run][None, :] * p[:, run]
        r[:, run] -= alpha[run][None, :] * Ap[:, run]
        z[:, run] = prec(r)[:, run]
        rz_old = rz.copy()
        rz[run], rr[run] = (r * z).sum(0)[run], (r * r).sum(0)[run]
        iters[run] += 1
        test()
    return X, iters, flag


def true_residual(rowptr, col, A, active, B, X):
    """|b - A x|_2 / |b|_2 per column over the active kernels' rows (nan for a zero column)."""
    on = np.repeat(np.asarray(active).astype(bool), 10)[:, None]
    Bm = np.where(on, np.asarray(B, np.float64).reshape(-1, 3), 0.0)
    r = np.where(on, Bm - bsr_matvec3(rowptr, col, A, np.where(on, np.asarray(X, np.float64).reshape(-1, 3), 0.0)), 0.0)
    with np.errstate(all="ignore"):
        return np.sqrt((r * r).sum(0)) / np.sqrt((Bm * Bm).sum(0))


# ------------------------------------------------------------------------------------------------ the oracle's system in block-sparse rows
def make_oracle_sim(cloud, kres):
    import torch
    from oracle.sim_init import OracleSimulator
    o = SC.opt()
    s = OracleSimulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), kres=kres, dx=o["sim_dx"], stiff=o["sim_stiff"],
                        base=torch.tensor([-o["bound"]] * 3))
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def system_from_oracle(ref):
    """dict(rowptr, col, A, M, Dinv, active) from an OracleSimulator's dense matrices: the pattern from its topology, A with +1e-3 on the active kernels'
    diagonal as solver.py:507 adds it; asserts that nothing of the dense matrices lies outside the pattern."""
    n_k = ref.n_k
    pin = ref.pts_kernel.numpy()[ref.is_pin.numpy()]
    rowptr, col = pattern_from_rows(n_k, ref.IP_kernel.numpy(), pin)
    active = np.zeros(n_k, np.int32)
    active[ref.active] = 1
    dense = ref.A.copy()
    lst = (ref.active[:, None] * 10 + np.arange(10)[None, :]).reshape(-1)
    dense[lst, lst] += 1e-3
    A, outA = dense_to_bsr(dense, rowptr, col)
    M, outM = dense_to_bsr(ref.Mmat, rowptr, col)
    assert outA == 0.0 and outM == 0.0
    diag = np.array([rowptr[k] + int(np.nonzero(col[rowptr[k]:rowptr[k + 1]] == k)[0][0]) for k in range(n_k)])
    Dinv = np.zeros((n_k, 10, 10))
    Dinv[ref.active] = np.linalg.inv(A[diag[ref.active]])
    return dict(rowptr=rowptr, col=col, A=A, M=M, Dinv=Dinv, active=active, dense=dense)


def rhs_cases(ref, name):
    """Right-hand sides [10 n_k, 3] for a cold solve: gravity (columns x and z all zero), the schedule's first pick force (three non-zero columns, a
    handful of non-zero kernels) and seeded white noise of gravity's size (every mode excited: the slowest of the three to converge)."""
    ref.update_force(SC.load_point(ref, name), np.array(SC.LOAD["beam" if name.startswith("beam") else name][0]))
    load = ref.dof_f.copy()
    ref.clear_force()
    noise = np.random.default_rng(3).normal(size=ref.rhs_gravity.shape) * np.abs(ref.rhs_gravity).max()
    return dict(gravity=ref.rhs_gravity.copy(), load=load, noise=noise)


class ComposedSim:
    """An OracleSimulator whose stepforward() is composed here from the oracle's ops (oracle/sim_oracle.cpp: orc_stepforward, restated): the global step is
    the oracle's dense product (solve='dense') or the reference PCG warm-started from dof - dof_rest (solve='pcg').  `iterations` collects the three
    iteration counts of every solve, `unconverged` the columns that did not converge."""

    def __init__(self, ref, solve="dense", system=None, tol=1e-10, max_iters=512):
        self.ref, self.solve, self.sys, self.tol, self.max_iters = ref, solve, system, tol, max_iters
        self.iterations, self.unconverged = [], 0

    def __getattr__(self, name):
        return getattr(self.ref, name)

    def update_force(self, vid, f):
        self.ref.update_force(vid, f)

    def clear_force(self):
        self.ref.clear_force()

    def stepforward(self):
        r = self.ref
        topo = r.IP_kernel.numpy()
        last = r.dof.copy()
        momentum = oracle.matvec3(r.Mmat, r.dof + r.dt * r.dof_vel) + r.dof_f + r.rhs_gravity
        for _ in range(r.iters):
            RF, VF, _ = oracle.calc_elastic(topo, r.IP_dNx, r.dof)
            tot = momentum + oracle.collect_rhs_IP(r.dx, topo, r.IP_mu, r.IP_lam, r.IP_dNx, RF, VF, r.n_k * 10) - r.rhs_rest
            if self.solve == "dense":
                x = oracle.matvec3(r.Ainv, tot)
            else:
                s = self.sys
                x, it, flag = pcg(s["rowptr"], s["col"], s["A"], s["Dinv"], s["active"], tot, r.dof - r.dof_rest, self.tol, self.max_iters)
                self.iterations.append(it)
                self.unconverged += int((flag != CONVERGED).sum())
            r.dof = r.dof_rest + x
        r.dof_vel = (r.dof - last) / r.dt * 0.998


def trajectory(ref, name, solve, system=None, tol=1e-10, max_iters=512, steps=SC.STEPS):
    """The displacements behind every scheduled substep (sim_clouds.run_schedule) of the composed trajectory from rest, and the ComposedSim.  `ref` (an
    OracleSimulator, one initialisation takes seconds) is put back to rest first and left in the final state."""
    ref.dof, ref.dof_vel, ref.dof_f = ref.dof_rest.copy(), np.zeros_like(ref.dof_rest), np.zeros_like(ref.dof_rest)
    sim = ComposedSim(ref, solve, system if solve == "pcg" else None, tol, max_iters)
    traj = []
    SC.run_schedule(sim, name, steps=steps, after_step=lambda k, s: traj.append(s.ref.dof - s.ref.dof_rest))
    return traj, sim


def worst_rel(a, b):
    """Largest relative displacement difference over a schedule: max over the substeps of max|a - b| / max|b|."""
    return max(float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)) for x, y in zip(a, b))
