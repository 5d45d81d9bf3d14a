"""Simulator diagnostics on the host: the law (tests/diagnostics_reference.py) against the reference's own system matrix and against states whose
answer is known in closed form, and the C ABI / Python / CLI surface.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import diagnostics_reference as R
from conftest import ROOT, make_oracle_sim


@pytest.fixture(scope="module")
def osim(small_cloud, small_opt):
    return make_oracle_sim(small_cloud, small_opt)


@pytest.fixture(scope="module")
def T(osim):
    return R.tables_from(osim)


def _rest(osim):
    return np.asarray(osim.dof_rest, np.float64).reshape(-1, 3)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_energies_are_the_ones_the_system_matrix_stands_for(osim, T):
    """1/2 d^T A d of the reference's matrix (build_IP_global: as is, with rho = 0, with mu = lam = 0) equals the sum over the points of
    dx^3 (mu + lam)/2 |F|^2 + (dx^5 / 12) (mu + lam)/2 |H|^2 + (1/2 m |x|^2 + 1/2 j |F|^2) / dt^2 of the reference module's x, F, H; and its kinetic
    energy of a velocity w is 1/2 w^T M w dt^2.  Tolerance: the derived sum bound (TOL S per point + n eps sum |term|), plus the matrix side's own
    rounding: its entries and the quadratic form are sums of the same non-negative magnitudes, (n_IP + dim) eps sum S at the most."""
    from oracle.sim_init import build_IP_global
    rng = np.random.default_rng(5)
    n_k, n, dx, dt = T["n_k"], T["n_IP"], T["dx"], T["dt"]
    dim = n_k * 10
    d = rng.standard_normal((dim, 3))
    w = rng.standard_normal((dim, 3))
    K = R.kinematics(T, d, w)
    m, j, ml = T["rho"] * dx ** 3, T["rho"] * dx ** 5 / 12.0, T["mu"] + T["lam"]
    topo = T["topo"]

    def quad(mat, y):
        return 0.5 * float(np.einsum("ir,ij,jr->", y, mat, y))

    def terms(x2, F2, H2):
        el = dx ** 3 * ml / 2 * F2 + dx ** 5 / 12.0 * ml / 2 * H2
        kin = (0.5 * m * x2 + 0.5 * j * F2) / dt ** 2
        return el, kin

    el, kin = terms((K["x"] ** 2).sum(1), (K["F"] ** 2).sum((1, 2)), (K["H"] ** 2).sum((1, 2, 3)))
    S_el, S_kin = terms((K["S_x"] ** 2).sum(1), (K["S_F"] ** 2).sum((1, 2)), (K["S_H"] ** 2).sum((1, 2, 3)))

    def bound(t, S):
        return R.TOL * S.sum() + n * R.EPS * np.abs(t).sum() + (n + dim) * R.EPS * S.sum()

    zero = np.zeros(n)
    A = build_IP_global(dx, dt, topo, T["mu"], T["lam"], T["rho"], T["Nx"], T["dNx"], T["ddNx"], dim)
    got, want = quad(A, d), float((el + kin).sum())
    print("full", got, want, abs(got - want), bound(el + kin, S_el + S_kin))
    assert abs(got - want) <= bound(el + kin, S_el + S_kin)
    A = build_IP_global(dx, dt, topo, T["mu"], T["lam"], zero, T["Nx"], T["dNx"], T["ddNx"], dim)
    got, want = quad(A, d), float(el.sum())
    print("elastic", got, want, abs(got - want), bound(el, S_el))
    assert abs(got - want) <= bound(el, S_el)
    A = build_IP_global(dx, dt, topo, zero, zero, T["rho"], T["Nx"], T["dNx"], T["ddNx"], dim)
    got, want = quad(A, d), float(kin.sum())
    print("mass", got, want, abs(got - want), bound(kin, S_kin))
    assert abs(got - want) <= bound(kin, S_kin)
    # the law's kinetic energy of the velocity w is that matrix's form, times dt^2
    P = R.per_point(T, _rest(osim), w)
    ke, S_ke = P["ke"], P["S_ke"]
    got, want = quad(A, w) * dt ** 2, float(ke.sum())
    print("kinetic", got, want, abs(got - want), bound(ke, S_ke))
    assert abs(got - want) <= bound(ke, S_ke)
    # ... and at F = I, H = 0 its elastic energy is zero: the (dx^5/12) term is the matrix's c2 block and nothing else
    assert abs(P["ee"]).max() <= R.TOL * P["S_ee"].max()


def test_rotation_has_no_elastic_energy(osim, T):
    """dof = dof_rest A^T gives F = A at every point, by linearity of the basis: for a rotation every sig is 1, det is 1 and elastic is within bound of 0."""
    A = _rot((1.0, 2.0, -0.5), 0.7)
    P = R.per_point(T, _rest(osim) @ A.T, np.zeros_like(_rest(osim)))
    assert np.abs(P["F"] - A[None]).max() <= R.TOL * P["S_F"].max()
    r, tol = R.row(P)
    assert np.abs(P["sig"] - 1.0).max() <= R.TOL * P["S_sig"].max()
    assert np.abs(P["det"] - 1.0).max() <= R.TOL * P["S_det"].max()
    assert abs(r["elastic"]) <= tol["elastic"]
    assert r["nonfinite"] == 0 and r["inverted"] == 0
    assert abs(r["kinetic"]) == 0.0 and np.all(r["P"] == 0.0)
    # the centre of mass turns with the body
    r0, _ = R.row(R.per_point(T, _rest(osim), np.zeros_like(_rest(osim))))
    assert np.abs(r["com"] - A @ r0["com"]).max() <= tol["com"].max() + np.abs(A).sum(1).max() * tol["com"].max()


def test_stretch_and_inversion(osim, T):
    z = np.zeros_like(_rest(osim))
    P = R.per_point(T, _rest(osim) @ np.diag([1.3, 1.0, 1.0]).T, z)
    r, tol = R.row(P)
    assert np.abs(P["sig"] - np.array([1.3, 1.0, 1.0])[None]).max() <= R.TOL * P["S_sig"].max()
    assert abs(r["strain_max"] - 0.3) <= tol["strain_max"] and abs(r["sig_max"] - 1.3) <= tol["sig_max"] and abs(r["sig_min"] - 1.0) <= tol["sig_min"]
    assert abs(r["det_min"] - 1.3) <= tol["det_min"] and r["inverted"] == 0
    # mu/2 0.09 + lam/2 |sig - sp|^2 per unit volume, no second derivative: compare with the closed form through the law's own projection
    sp = R.volume_invariant_project(np.array([[1.3, 1.0, 1.0]]))[0]
    want = (T["dx"] ** 3 * (T["mu"] / 2 * 0.09 + T["lam"] / 2 * ((np.array([1.3, 1.0, 1.0]) - sp) ** 2).sum())).sum()
    assert abs(r["elastic"] - want) <= tol["elastic"]

    P = R.per_point(T, _rest(osim) @ np.diag([1.0, 1.0, -0.5]).T, z)
    r, tol = R.row(P)
    assert r["inverted"] == T["n_IP"] and r["nonfinite"] == 0
    assert abs(r["sig_min"] + 0.5) <= tol["sig_min"] and abs(r["det_min"] + 0.5) <= tol["det_min"]
    assert np.abs(P["sig"] - np.array([1.0, 1.0, -0.5])[None]).max() <= R.TOL * P["S_sig"].max()


def test_rigid_spin_momenta(osim, T):
    """dof_vel = dof_rest W^T gives v = W x and G = W: for a skew W (angular velocity omega) L is the discrete inertia tensor — the j term included —
    times omega, and P = mass W com."""
    om = np.array([0.3, -1.1, 0.6])
    W = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    rest = _rest(osim)
    P = R.per_point(T, rest, rest @ W.T)
    r, tol = R.row(P)
    x, m, j, F = P["x"], P["m"], P["j"], P["F"]
    I = (m[:, None, None] * ((x * x).sum(1)[:, None, None] * np.eye(3)[None] - x[:, :, None] * x[:, None, :])).sum(0)
    FFt = np.einsum("nrc,nsc->nrs", F, F)
    I = I + (j[:, None, None] * (np.trace(FFt, axis1=1, axis2=2)[:, None, None] * np.eye(3)[None] - FFt)).sum(0)
    assert np.abs(r["L"] - I @ om).max() <= 2 * tol["L"].max()
    assert np.abs(r["P"] - r["mass"] * (W @ r["com"])).max() <= 2 * tol["P"].max() + r["mass"] * np.abs(W).sum(1).max() * tol["com"].max()
    # 1/2 omega.L is the kinetic energy of a rigid spin
    assert abs(r["kinetic"] - 0.5 * om @ r["L"]) <= tol["kinetic"] + np.abs(om).sum() * tol["L"].max()
    assert abs(r["speed_max"] - np.linalg.norm(np.cross(om[None], x), axis=1).max()) <= tol["speed_max"]


def test_nonfinite_points_are_counted_and_left_out(osim, T):
    rest = _rest(osim).copy()
    k = int(T["topo"][T["n_IP"] // 2, 3])
    bad = rest.copy()
    bad[k * 10 + 2, 1] = np.nan
    P = R.per_point(T, bad, np.zeros_like(rest))
    r, _ = R.row(P)
    hit = (T["topo"] == k).any(1)
    assert r["nonfinite"] == int(hit.sum()) > 0
    assert all(np.all(np.isfinite(np.asarray(v, np.float64))) for v in r.values())
    rec, _ = R.record(P)
    assert np.isnan(rec[hit, 1:]).all() and np.isfinite(rec[~hit]).all() and np.isfinite(rec[:, 0]).all()
    # no finite point at all: sums 0, extrema NaN with index -1
    P = R.per_point(T, np.full_like(rest, np.nan), np.zeros_like(rest))
    r, _ = R.row(P)
    assert r["nonfinite"] == T["n_IP"] and r["mass"] == 0.0 and r["elastic"] == 0.0 and np.all(r["com"] == 0.0)
    assert np.isnan(r["sig_min"]) and r["sig_min_ip"] == -1 and np.isnan(r["speed_max"]) and r["speed_max_ip"] == -1


def test_symbols_fields_and_signatures():
    from pienerf_amd import _lib, build
    from pienerf_amd.simulator import diagnostics as D
    from pienerf_amd.simulator import solver
    import pienerf_amd.simulator as pkg
    text = open(os.path.join(ROOT, "include", "pienerf_hip.h")).read()
    assert re.search(r"\bint\s+pn_sim_diagnostics\s*\(\s*int n_k, int n_IP, double dx, const double\* g3_host, const double\* dof, const double\* dof_vel, "
                     r"const int\* topo, const double\* rho,\s*const double\* mu, const double\* lam, const double\* Nx, const double\* dNx, "
                     r"const double\* ddNx, double\* work, double\* row_out,\s*double\* per_point, void\* stream\)\s*;", text)
    assert re.search(r"\bint\s+pn_sim_diagnostics_doubles\s*\(\s*void\s*\)\s*;", text)
    assert re.search(r"\buint64_t\s+pn_sim_diagnostics_work_doubles\s*\(\s*int n_IP\s*\)\s*;", text)
    assert re.search(r"#define\s+PN_DIAG_DOUBLES\s+25\b", text) and "cuda_utils.py:48-55" in text
    i32, f64, u64, P = _lib.i32, _lib.f64, _lib.u64, _lib.P
    assert _lib.SIGNATURES["pn_sim_diagnostics"] == (i32, [i32, i32, f64] + [P] * 14)
    assert _lib.SIGNATURES["pn_sim_diagnostics_doubles"] == (i32, [])
    assert _lib.SIGNATURES["pn_sim_diagnostics_work_doubles"] == (u64, [i32])
    assert build.UNITS["pn_diagnostics.hip"] == ["-ffp-contract=fast"]
    h = _lib.lib()
    assert len(D.DIAG_FIELDS) == h.pn_sim_diagnostics_doubles() == 25 and D.DIAG_FIELDS == R.FIELDS and D.PER_POINT_FIELDS == R.PER_POINT
    assert h.pn_sim_diagnostics_work_doubles(1) == 25 and h.pn_sim_diagnostics_work_doubles(32) == 25 and h.pn_sim_diagnostics_work_doubles(33) == 50
    assert h.pn_sim_diagnostics_work_doubles(0) == 0
    # argument checks answer before anything is enqueued
    dummy, g = ctypes.c_void_p(16), (ctypes.c_double * 3)(0.0, -9.8, 0.0)
    ok = [4, 8, 0.1, g] + [dummy] * 12 + [None, None]
    for i, v in ((0, 0), (1, 0), (1, (1 << 27) + 1), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf")), (3, None), (4, None), (5, None), (6, None),
                 (10, None), (13, None), (14, None)):
        a = list(ok)
        a[i] = v
        assert h.pn_sim_diagnostics(*a) == 1, (i, v)   # PN_ERR_ARG
    # a readout beside the stages, not one of them
    assert issubclass(solver.Simulator, D.DiagnosticsMixin) and len(solver.Simulator.STAGES) == 6
    assert not any(st.name == "diagnostics" for st in solver.Simulator.STAGES)
    for name in ("DIAG_FIELDS", "DiagnosticsLog", "DiagnosticsMixin"):
        assert getattr(solver, name) is getattr(D, name) and getattr(pkg, name) is getattr(D, name)


def test_row_dict_and_log_on_the_host(tmp_path):
    from pienerf_amd.simulator.diagnostics import DIAG_FIELDS, DiagnosticsLog, diagnostics_dict
    row = np.arange(25, dtype=np.float64) + 0.5
    row[[14, 16, 18, 20, 22]] = [3, 4, 5, 6, -1]
    row[[23, 24]] = [2, 7]
    d = diagnostics_dict(row)
    assert d["mass"] == 0.5 and np.array_equal(d["com"], row[1:4]) and np.array_equal(d["P"], row[4:7]) and np.array_equal(d["L"], row[7:10])
    assert d["kinetic"] == 10.5 and d["gravity"] == 11.5 and d["elastic"] == 12.5 and d["sig_min"] == 13.5 and d["speed_max"] == 21.5
    assert (d["sig_min_ip"], d["sig_max_ip"], d["det_min_ip"], d["strain_max_ip"], d["speed_max_ip"]) == (3, 4, 5, 6, -1)
    assert d["nonfinite"] == 2 and d["inverted"] == 7 and all(isinstance(d[k], int) for k in ("sig_min_ip", "nonfinite", "inverted"))
    with pytest.raises(ValueError):
        diagnostics_dict(row[:24])
    log = DiagnosticsLog(2, device="cpu")
    with pytest.raises(ValueError):
        DiagnosticsLog(0, device="cpu")
    log.next_row().copy_(__import__("torch").from_numpy(row))
    log.next_row()
    with pytest.raises(RuntimeError, match="full"):
        log.next_row()
    path = log.write_csv(str(tmp_path / "d.csv"))
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(DIAG_FIELDS) and len(lines) == 3
    assert np.array_equal(np.array([float(v) for v in lines[1].split(",")]), row)   # 17 digits: the same doubles


@pytest.mark.parametrize("ke", ["0", "-1", "nan", "inf"])
def test_cli_rejects_a_bad_until_rest(ke, tmp_path):
    from pienerf_amd import main_render
    args = main_render.parser().parse_args(["--out", str(tmp_path / "o"), "--frames", "1", f"--until_rest={ke}", "--device", "cpu"])
    with pytest.raises(SystemExit, match="--until_rest"):
        main_render.run(args)
    assert not (tmp_path / "o").exists()   # refused before anything is built


def test_cli_diagnostics_paths(tmp_path):
    from pienerf_amd import main_render
    ap = main_render.parser()
    a = ap.parse_args(["--out", "O"])
    assert main_render.diagnostics_path(a) is None
    assert main_render.diagnostics_path(ap.parse_args(["--out", "O", "--diagnostics"])) == os.path.join("O", "diagnostics.csv")
    assert main_render.diagnostics_path(ap.parse_args(["--out", "O", "--diagnostics", "x.csv"])) == "x.csv"
    assert main_render.diagnostics_path(ap.parse_args(["--out", "O", "--until_rest", "1e-3"])) == os.path.join("O", "diagnostics.csv")
    rows = np.zeros((3, 25))
    rows[:, 10], rows[:, 12] = [0.0, 2.0, 1.5], [0.0, 3.0, 4.25]
    assert "no frame with a non-finite or inverted point" in main_render.report_diagnostics(rows)
    assert "kinetic 1.5" in main_render.report_diagnostics(rows) and "elastic 4.25" in main_render.report_diagnostics(rows)
    rows[1, 24], rows[2, 23] = 4, 1
    assert "first frame with a non-finite or inverted point: 1 (0 non-finite, 4 inverted)" in main_render.report_diagnostics(rows)
