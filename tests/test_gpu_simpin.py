"""What can be said about the simulator half WITHOUT the reference's Warp kernels (warp-lang is absent: SURVEY.md §8c, "parity unpinned").

The one convention of `wp.svd3` (cuda_utils.py:107) that the restatement has to ASSUME is what happens at an inverted element: with det F < 0
a decomposition may return proper rotations U, V and a negative smallest singular value (the contract this repository and its oracle state), or
reflections and positive singular values — and `R = U V^T`, `volume_invariant_project(sigma)` differ between the two.  For det F > 0 there is
nothing to assume: every SVD with sigma >= 0 gives the same polar rotation R and the same `U diag(sigma') V^T` (the projection is symmetric
in the singular values).  So the tests here run the trajectories of BASELINE.json's three single-GPU configurations — with the forces bench.py
applies — and check that det F stays positive at every integration point of every substep: on these workloads the assumed branch is dormant
and the simulator's results do not depend on it.  (A scene that does invert elements is covered by
test_gpu_edges.py::test_calc_elastic_jacobi_argument_on_adversarial_deformation_gradients against the oracle's contract only.)

Also here: the arrival counters of the chunked right-hand-side gather are cyclic (round-3 advisor finding)."""
import numpy as np
import pytest
import torch

from pienerf_amd import scene
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def _sim(cloud, opt):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def _det3(F9):
    """det of [n, 9] matrices (either index order: det F = det F^T)."""
    F = F9.double().view(-1, 3, 3)
    return torch.linalg.det(F)


CONFIGS = {
    # name: (opt, cloud kwargs, force) — the same scenes and forces as bench.py's make_config
    "chair": (lambda: scene.default_opt(), dict(), None),
    "chair_forced": (lambda: scene.default_opt(), dict(), (300.0, 100.0, -200.0)),
    "trex": (lambda: scene.trex_opt(radius=4.5), dict(bound=2.0), (250.0, 120.0, -180.0)),
    "stress": (lambda: scene.stress_opt(), dict(sub_res=180), (400.0, -150.0, 250.0)),
}


def _oracle_state(s):
    """The CPU oracle's state dict (oracle.stepforward) filled from a GPU-initialised Simulator: same attribute names, same layouts (the init itself
    is compared with the oracle's in test_gpu_parity.py: Ainv 1e-8, dNx 1e-12)."""
    g = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
    n3 = s.n_k * 10
    return dict(iters=int(s.iters), dt=float(s.dt), dx=float(s.dx), IP_kernel=g(s.IP_kernel).astype(np.int32), IP_mu=g(s.IP_mu), IP_lam=g(s.IP_lam),
                IP_dNx=g(s.IP_dNx), Ainv=g(s.Ainv), Mmat=g(s.Mmat), dof_rest=g(s.dof_rest).reshape(n3, 3), rhs_rest=g(s.rhs_rest).reshape(n3, 3),
                rhs_gravity=g(s.rhs_gravity).reshape(n3, 3), dof_f=g(s.dof_f).reshape(n3, 3), dof=g(s.dof).reshape(n3, 3).copy(),
                dof_vel=g(s.dof_vel).reshape(n3, 3).copy())


def _sim_with(cloud, opt, svd, form):
    import os
    from pienerf_amd.simulator.solver import Simulator
    old = os.environ.get("PN_SIM_FORM")
    os.environ["PN_SIM_FORM"] = form
    try:
        s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                      base=torch.tensor([-opt["bound"]] * 3), device=DEV, svd=svd)
    finally:
        if old is None:
            del os.environ["PN_SIM_FORM"]
        else:
            os.environ["PN_SIM_FORM"] = old
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


@pytest.mark.parametrize("name", list(CONFIGS))
def test_svd_gap_per_simulator_on_the_baseline_trajectories(name):
    """wp.svd3 (cuda_utils.py:107) is third-party and absent; the repository holds the contract (converged Jacobi: the oracle's default and the HIP
    kernels' default) and the published algorithm (McAdams et al.: the oracle's svd3_mcadams and the kernels' PN_SIM_SVD=mcadams mode); six simulators
    with their own svd= choice, which each passes to its launches as mcadams_sweeps.  On each
    BASELINE trajectory (configs[1], [1] forced, [2], [4]), 10 substeps of 10 local/global iterations from the same GPU-initialised state:
      * HIP default vs oracle(converged), HIP mcadams:8 vs oracle(mcadams 8), HIP mcadams:4 vs oracle(mcadams 4): <= 1e-9 of the displacements —
        each kernel mode IS its restatement (cell form and CSR form);
      * converged vs mcadams 8: <= 1e-5 (measured 3e-6 on the chair: the paper's 10-digit constants, mostly through rhs_rest at F = I); converged vs mcadams 4 is printed (2.6e-4 on the chair —
        the one figure above the 1e-4 bar, which is why the mode exists)."""
    import oracle
    from svd_cases import trajectory_scene
    opt, cloud, force = trajectory_scene(name)
    sims = {(svd, form): _sim_with(cloud, opt, svd, form) for svd in ("jacobi", "mcadams:8", "mcadams:4") for form in ("cells", "csr")}
    for s in sims.values():
        if force is not None:
            s.update_force(s.n_IP // 2, np.array(force))
    torch.cuda.synchronize()
    s0 = sims[("jacobi", "cells")]
    rest = _oracle_state(s0)["dof_rest"]
    ref = {}
    for key, mode in (("jacobi", dict(mode="converged")), ("mcadams:8", dict(mode="mcadams", sweeps=8)), ("mcadams:4", dict(mode="mcadams", sweeps=4))):
        # each mode's state from a simulator OF that mode: rhs_rest (solver.py:314) is a build_rhs() too, computed with the same svd3 as the steps
        st = _oracle_state(sims[(key, "cells")])
        assert np.abs(st["rhs_rest"] - _oracle_state(sims[(key, "csr")])["rhs_rest"]).max() <= 1e-12 * np.abs(st["rhs_rest"]).max()
        with oracle.svd_mode(**mode):
            for _ in range(10):
                oracle.stepforward(st)
        ref[key] = st["dof"].copy()
    disp = np.abs(ref["jacobi"] - rest).max()
    assert disp > 1e-2
    for (svd, form), s in sims.items():
        for _ in range(10):
            s.stepforward()
        torch.cuda.synchronize()
        got = s.dof.cpu().numpy().reshape(-1, 3)
        gap = np.abs(got - ref[svd]).max() / disp
        print(f"{name}: HIP {svd:9s} ({form:5s}) vs its oracle restatement: {gap:.2e} of max |displacement| {disp:.3e}")
        assert gap < 1e-9, (name, svd, form, gap)
    g8 = np.abs(ref["mcadams:8"] - ref["jacobi"]).max() / disp
    g4 = np.abs(ref["mcadams:4"] - ref["jacobi"]).max() / disp
    print(f"{name}: n_IP {s0.n_IP}: converged vs mcadams 8 sweeps {g8:.2e}, vs 4 sweeps {g4:.2e} (of max |displacement| after 10 substeps)")
    assert g8 < 1e-5 and g4 < 1e-2


def test_two_svd_choices_stepped_alternately_on_one_stream(small_cloud, small_opt):
    """A jacobi and a mcadams:4 simulator stepped in turn on one stream end bit-identical to each one stepped alone, in the cell and the CSR form:
    every launch carries its own decomposition (the mcadams_sweeps argument), nothing is left in the library for the next launch to read."""
    def run(svds, form, steps=6):
        sims = [_sim_with(small_cloud, small_opt, svd, form) for svd in svds]
        for _ in range(steps):
            for s in sims:
                s.stepforward()
        torch.cuda.synchronize()
        return [(s.dof.clone(), s.dof_vel.clone()) for s in sims]
    for form in ("cells", "csr"):
        both = run(("jacobi", "mcadams:4"), form)
        alone = run(("jacobi",), form) + run(("mcadams:4",), form)
        for (d, v), (d1, v1) in zip(both, alone):
            assert torch.equal(d, d1) and torch.equal(v, v1), form
        assert not torch.equal(both[0][0], both[1][0]), form   # the two choices do give different trajectories


def test_mcadams_sweeps_argument_on_the_adversarial_set():
    """pn_sim_calc_elastic with mcadams_sweeps 8 / 4 against the oracle's svd3_mcadams with the same sweep count on the adversarial
    deformation gradients (inverted, rank-deficient, repeated singular values, 1e-12- and 1e+8-scaled): the same algorithm, so the same R and
    U diag(sigma') V^T to rounding wherever they are finite — including where the algorithm and the contract part ways."""
    import oracle
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    from svd_cases import adversarial_F, elastic_inputs_for, well_conditioned
    Fs = adversarial_F()
    topo, dNx, dof = elastic_inputs_for(Fs)
    n = len(Fs)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    topo_d, dNx_d, dof_d = T(topo), T(dNx), T(dof.reshape(-1))
    scale = np.maximum(1.0, np.abs(Fs).max(axis=(1, 2)))[:, None, None]
    for sweeps in (8, 4):
        with oracle.svd_mode("mcadams", sweeps=sweeps):
            R0, V0, F0 = oracle.calc_elastic(topo, dNx, dof)
        RF, VF, FF = (torch.empty(n, 3, 3, dtype=torch.float64, device=DEV) for _ in range(3))
        check(lib().pn_sim_calc_elastic(n, ptr(topo_d), ptr(dNx_d), ptr(dof_d), ptr(RF), ptr(VF), ptr(FF), sweeps, stream_ptr()), "calc_elastic")
        torch.cuda.synchronize()
        RF, VF, FF = RF.cpu().numpy(), VF.cpu().numpy(), FF.cpu().numpy()
        fin = np.isfinite(V0).all(axis=(1, 2)) & np.isfinite(R0).all(axis=(1, 2))
        assert np.array_equal(np.isfinite(VF).all(axis=(1, 2)) & np.isfinite(RF).all(axis=(1, 2)), fin)
        # Where F^T F has (nearly) repeated eigenvalues — pure rotations, +-identity, repeated or vanishing singular values — the test
        # gamma sh^2 < ch^2 compares rounding noise, so the two builds may take the fallback rotation a different number of times; each
        # fallback leaves the quaternion 5e-10 short of unit length (the 10-digit constants), so R agrees to that noise level only (1e-7),
        # or — rank-deficient F — is not determined at all.  Everywhere else the two are the same arithmetic: 1e-9.
        eR = np.abs(RF - R0).max(axis=(1, 2))
        vs = np.maximum(1.0, np.abs(V0).max(axis=(1, 2)))
        eV = np.abs(VF - V0).max(axis=(1, 2)) / np.where(np.isfinite(vs), vs, 1.0)
        agree = fin & (eR < 1e-9)
        ok = fin & well_conditioned(Fs)
        print(f"mcadams {sweeps} sweeps on the adversarial set: {agree.sum()} of {fin.sum()} finite cases agree to 1e-9 (max |V - V_oracle| there "
              f"{eV[agree].max():.2e}); the others: {np.flatnonzero(fin & ~agree).tolist()}, of them determined: "
              f"{np.flatnonzero(ok & ~agree).tolist()} with |R - R_oracle| <= {eR[ok & ~agree].max() if (ok & ~agree).any() else 0.0:.2e}")
        assert agree[:380].all() and eV[agree].max() < 1e-9            # the 380 random / inverted gradients: the same arithmetic
        assert agree.sum() >= fin.sum() - 12 and eR[ok].max() < 1e-6    # the degenerate ones: the constants' noise level where R is determined
        assert np.abs((FF - F0) / scale)[agree].max() < 1e-9 and np.abs((FF - F0) / scale)[fin].max() < 1e-6


def test_configs0_as_baseline_states_it_on_the_gpu():
    """BASELINE configs[0] (chair cloud, ONE local/global iteration, sim_dx 0.05, simulator step only) through the HIP path against the oracle —
    the CPU half is tests/test_oracle_svd.py::test_configs0_as_baseline_states_it."""
    from conftest import make_oracle_sim, rel_err
    opt = scene.default_opt(sim_iters=1)
    cloud = scene.make_chair_points(hgs=opt["hash_grid_size"])
    s = _sim(cloud, opt)
    ref = make_oracle_sim(cloud, opt)
    assert (s.n_k, s.n_IP, int(s.iters)) == (ref.n_k, ref.n_IP, 1) == (139, 3576, 1)
    for step in range(3):
        s.stepforward()
        ref.stepforward()
        torch.cuda.synchronize()
        disp = s.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest
        assert rel_err(disp, ref.dof - ref.dof_rest) < 1e-6, step   # (measured 1.1e-8: the first substep's displacement is small against Ainv's 1e-8)
    p1, F1, dF1 = (t.cpu().numpy() for t in s.get_IP_info())
    p2, F2, dF2 = ref.get_IP_info()
    assert np.abs(p1 - p2).max() < 1e-6 and np.abs(F1 - F2).max() < 1e-5 and np.abs(dF1 - dF2).max() < 1e-4


@pytest.mark.parametrize("name", list(CONFIGS))
def test_det_F_stays_positive_on_the_baseline_trajectories(name):
    """min over integration points and substeps of det F on the configs[1] / [2] / [4] trajectories: > 0, i.e. the svd3 sign convention is never
    exercised there.  300 substeps = the length of the bench's timed region (prime + warm-up + 200 steps)."""
    mk, ckw, force = CONFIGS[name]
    opt = mk()
    cloud = scene.make_chair_points(hgs=opt["hash_grid_size"], **dict({"bound": opt["bound"]}, **ckw))
    s = _sim(cloud, opt)
    if force is not None:
        s.update_force(s.n_IP // 2, np.array(force))
    lo, hi = float("inf"), 0.0
    for step in range(300):
        s.stepforward()
        if step % 4 == 0 or step < 20:
            _, F, _ = s.get_IP_info()
            d = _det3(F)
            lo, hi = min(lo, float(d.min())), max(hi, float(d.max()))
    torch.cuda.synchronize()
    print(f"{name}: n_IP {s.n_IP}, det F in [{lo:.4f}, {hi:.4f}] over 300 substeps")
    assert lo > 0.2, (name, lo)          # far from inversion
    assert np.isfinite(hi) and hi < 5.0
    assert abs(hi - 1.0) > 1e-4 or abs(lo - 1.0) > 1e-4  # the body did deform


def test_gather_arrival_counters_are_cyclic():
    """k_rhs_gather_chunk's per-kernel arrival counters return to 0 at the end of every launch (the last arriver stores 0), so they cannot wrap
    however long a simulator lives; rounds 1-3 let them grow by `chunks` per local/global iteration and tested (n % chunks) == 0."""
    from pienerf_amd._lib import lib
    opt = scene.default_opt()   # 139 kernels, CSR lists of up to 770 entries: most kernels have several chunks of 64
    s = _sim(scene.make_chair_points(hgs=opt["hash_grid_size"]), opt)
    for _ in range(5):
        s.stepforward()
    torch.cuda.synchronize()
    n_k, n_IP = s.n_k, s.n_IP
    chunks_max = n_IP * 8 // 64 + n_k                       # pn_gather_chunks_max (PN_GCH = 64)
    part0 = 4 * n_k * 30 + n_IP * 9 + n_IP * 8 * 9           # doubles in front of the chunk sums
    kc_bg0 = (part0 + chunks_max * 30) * 2                  # int index of kc_bg in the work buffer
    slot = (n_k + 2) & ~1
    assert int(lib().pn_sim_work_doubles(n_k, n_IP)) == s._work.numel()
    ints = s._work.view(torch.int32)
    kc_bg = ints[kc_bg0:kc_bg0 + n_k + 1].cpu().numpy()
    kcount = ints[kc_bg0 + slot:kc_bg0 + slot + n_k].cpu().numpy()
    assert kc_bg[0] == 0 and (np.diff(kc_bg) >= 0).all() and kc_bg[-1] > 0   # we are looking at the plan
    assert (np.diff(kc_bg) > 1).any()                                        # kernels with several chunks exist: the counters are used
    assert not kcount.any()
