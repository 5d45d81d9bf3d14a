"""The simulator diagnostics' law (include/pienerf_hip.h: pn_sim_diagnostics) restated in numpy, with the error bounds the tests use.

Both sides are fp64 and differ in summation order and contraction only, so every quantity q comes with its MAGNITUDE SUM S_q: the same expression
evaluated with the absolute value of every product, all the way down to |table entry| |dof entry|.  A sum of k products evaluated in any order, with or
without fused multiply-adds, is within k 2^-53 (1 + O(eps)) S of the exact value; the deepest chain here (80 products per component, squared, summed
over 27 components, a few scalar factors) stays below 2^9, and the two sides may err in opposite directions:

    per point      |device - reference| <= TOL S,   TOL = 2^10 2^-52
    sig            the singular values are 1-Lipschitz in F, so TOL |S_F|_F (S_F: the magnitude sums of F's nine components) bounds what the
                   perturbation of F moves them by; both decompositions (LAPACK here, converged Jacobi on the device) add a few eps |F| of their own
    quantities of sig   ((sig - 1)^2, (sig - sp)^2, strain) take |sig_i| <= |S_F|_F as sig's magnitude: S = (|S_F|_F + 1)^2 and so on, which bounds
                   2 |sig - 1| dsig as long as dsig <= TOL/2 (|S_F|_F + 1).  volume_invariant_project moves sp by about what sig moves while the
                   state is away from |sig[2]| -> 0, which is why:
    |sig[2]| < 0.25     only finiteness, counts and indices are compared (SIG_FLOOR): Jacobi on F^T F loses the small singular value there
    a global sum over n points      sum of the per-point bounds + n 2^-52 sum |term|

Singular values come from np.linalg.svd, the smallest one given the sign of det F."""
import numpy as np

EPS = 2.0 ** -52
TOL = 2.0 ** 10 * EPS
SIG_FLOOR = 0.25

FIELDS = ("mass", "com_x", "com_y", "com_z", "P_x", "P_y", "P_z", "L_x", "L_y", "L_z", "kinetic", "gravity", "elastic",
          "sig_min", "sig_min_ip", "sig_max", "sig_max_ip", "det_min", "det_min_ip", "strain_max", "strain_max_ip", "speed_max", "speed_max_ip",
          "nonfinite", "inverted")
PER_POINT = ("m", "ke", "ee", "det", "sig0", "sig1", "sig2", "strain")


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def tables_from(sim):
    """The tables of a Simulator (torch, any device) or an OracleSimulator (numpy) as fp64 numpy arrays."""
    n = int(sim.n_IP)
    return dict(n_k=int(sim.n_k), n_IP=n, dx=float(sim.dx), dt=float(sim.dt), g=_np(sim.gravity).astype(np.float64).reshape(3),
                topo=_np(sim.IP_kernel).astype(np.int64).reshape(n, 8), rho=_np(sim.IP_rho).astype(np.float64), mu=_np(sim.IP_mu).astype(np.float64),
                lam=_np(sim.IP_lam).astype(np.float64), Nx=_np(sim.IP_Nx).astype(np.float64).reshape(n, 8, 10),
                dNx=_np(sim.IP_dNx).astype(np.float64).reshape(n, 8, 3, 10), ddNx=_np(sim.IP_ddNx).astype(np.float64).reshape(n, 8, 3, 3, 10))


def volume_invariant_project(sig):
    """simulator/func_utils.py:21-40 on [n, 3]."""
    D = np.zeros_like(sig)
    for _ in range(3):
        a = sig + D
        C = a[:, 0] * a[:, 1] * a[:, 2] - 1.0
        g = np.stack([a[:, 1] * a[:, 2], a[:, 0] * a[:, 2], a[:, 0] * a[:, 1]], axis=1)
        coef = ((g * D).sum(1) - C) / (g * g).sum(1)
        D = coef[:, None] * g
    return sig + D


def _det(F):
    return (F[:, 0, 0] * (F[:, 1, 1] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 1]) - F[:, 0, 1] * (F[:, 1, 0] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 0])
            + F[:, 0, 2] * (F[:, 1, 0] * F[:, 2, 1] - F[:, 1, 1] * F[:, 2, 0]))


def _det_abs(F):
    return (F[:, 0, 0] * (F[:, 1, 1] * F[:, 2, 2] + F[:, 1, 2] * F[:, 2, 1]) + F[:, 0, 1] * (F[:, 1, 0] * F[:, 2, 2] + F[:, 1, 2] * F[:, 2, 0])
            + F[:, 0, 2] * (F[:, 1, 0] * F[:, 2, 1] + F[:, 1, 1] * F[:, 2, 0]))


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _cross_abs(a, b):
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)


def kinematics(T, dof, dof_vel):
    """x, v [n,3]; F, G [n,3,3] (row r, column c); H [n,3,3,3] (r, j, c), each with its magnitude sum under 'S_' + name."""
    n_k = T["n_k"]
    d = np.asarray(dof, np.float64).reshape(n_k, 10, 3)[T["topo"]]          # [n, 8, 10, 3]
    w = np.asarray(dof_vel, np.float64).reshape(n_k, 10, 3)[T["topo"]]
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for name, tab, sub in (("x", T["Nx"], "nib,nibr->nr"), ("F", T["dNx"], "nicb,nibr->nrc"), ("H", T["ddNx"], "nijcb,nibr->nrjc")):
            out[name] = np.einsum(sub, tab, d)
            out["S_" + name] = np.einsum(sub, np.abs(tab), np.abs(d))
        for name, tab, sub in (("v", T["Nx"], "nib,nibr->nr"), ("G", T["dNx"], "nicb,nibr->nrc")):
            out[name] = np.einsum(sub, tab, w)
            out["S_" + name] = np.einsum(sub, np.abs(tab), np.abs(w))
    return out


def per_point(T, dof, dof_vel):
    """Every per-point quantity of the law with its magnitude sum ('S_' + name), the mask `finite`, and the kinematics they come from."""
    K = kinematics(T, dof, dof_vel)
    n, dx = T["n_IP"], T["dx"]
    fin = np.ones(n, bool)
    for name in ("x", "v", "F", "G", "H"):
        fin &= np.isfinite(K[name].reshape(n, -1)).all(1)
    x, v, F, G, H = (np.where(fin.reshape((n,) + (1,) * (K[k].ndim - 1)), K[k], 0.0) for k in ("x", "v", "F", "G", "H"))
    Sx, Sv, SF, SG, SH = (np.where(fin.reshape((n,) + (1,) * (K[k].ndim - 1)), K["S_" + k], 0.0) for k in ("x", "v", "F", "G", "H"))
    F = np.where(fin[:, None, None], F, np.eye(3)[None])
    m, j = T["rho"] * dx ** 3, T["rho"] * dx ** 5 / 12.0
    mu, lam, g = T["mu"], T["lam"], T["g"]
    det = _det(F)
    sig = np.linalg.svd(F, compute_uv=False)
    sig[:, 2] = np.where(det < 0, -sig[:, 2], sig[:, 2])
    sp = volume_invariant_project(sig)
    nF = np.sqrt((SF * SF).sum((1, 2)))                                       # | |F| |_F: sig's magnitude
    e1, e2 = ((sig - 1.0) ** 2).sum(1), ((sig - sp) ** 2).sum(1)
    hh, S_hh = (H * H).sum((1, 2, 3)), (SH * SH).sum((1, 2, 3))
    P = dict(finite=fin, x=x, v=v, F=F, G=G, H=H, S_x=Sx, S_v=Sv, S_F=SF, S_G=SG, S_H=SH, m=m, j=j, sig=sig, sp=sp, det=det, S_det=_det_abs(SF), S_sig=nF)
    P["ke"] = 0.5 * m * (v * v).sum(1) + 0.5 * j * (G * G).sum((1, 2))
    P["S_ke"] = 0.5 * m * (Sv * Sv).sum(1) + 0.5 * j * (SG * SG).sum((1, 2))
    P["ee"] = dx ** 3 * (0.5 * mu * e1 + 0.5 * lam * e2) + dx ** 5 / 12.0 * 0.5 * (mu + lam) * hh
    P["S_ee"] = dx ** 3 * (0.5 * mu * 3.0 * (nF + 1.0) ** 2 + 0.5 * lam * 3.0 * (nF + np.abs(sp).max(1)) ** 2) + dx ** 5 / 12.0 * 0.5 * (mu + lam) * S_hh
    P["ge"] = -m * (x * g[None]).sum(1)
    P["S_ge"] = m * (Sx * np.abs(g)[None]).sum(1)
    P["mx"], P["S_mx"] = m[:, None] * x, m[:, None] * Sx
    P["P"], P["S_P"] = m[:, None] * v, m[:, None] * Sv
    P["L"] = m[:, None] * _cross(x, v) + j[:, None] * sum(_cross(F[:, :, c], G[:, :, c]) for c in range(3))
    P["S_L"] = m[:, None] * _cross_abs(Sx, Sv) + j[:, None] * sum(_cross_abs(SF[:, :, c], SG[:, :, c]) for c in range(3))
    P["strain"], P["S_strain"] = np.sqrt(e1), np.sqrt(3.0) * (nF + 1.0)
    P["speed"], P["S_speed"] = np.sqrt((v * v).sum(1)), np.sqrt((Sv * Sv).sum(1))
    P["comparable"] = fin & (np.abs(sig[:, 2]) >= SIG_FLOOR)
    return P


def record(P):
    """The per-point record [n, 8] = (m, ke, ee, det, sig0, sig1, sig2, strain), NaN behind m for a non-finite point, and its bounds [n, 8]."""
    rec = np.stack([P["m"], P["ke"], P["ee"], P["det"], P["sig"][:, 0], P["sig"][:, 1], P["sig"][:, 2], P["strain"]], axis=1)
    tol = TOL * np.stack([np.zeros_like(P["m"]), P["S_ke"], P["S_ee"], P["S_det"], P["S_sig"], P["S_sig"], P["S_sig"], P["S_strain"]], axis=1)
    tol[:, 0] = 4 * EPS * np.abs(P["m"])   # rho dx^3: two roundings
    rec[~P["finite"], 1:] = np.nan
    return rec, tol


def _first_arg(vals, fin, largest):
    if not fin.any():
        return np.nan, -1
    w = np.where(fin, vals, -np.inf if largest else np.inf)
    i = int(np.argmax(w) if largest else np.argmin(w))      # the first occurrence: the lowest index on equal values
    return float(vals[i]), i


def row(P):
    """The diagnostics row as a dict by FIELDS (com / P / L as arrays), and the bound of every value under the same key."""
    fin = P["finite"]
    n = int(fin.sum())

    def total(name):
        t, S = P[name][fin], P["S_" + name][fin]
        return t.sum(0), TOL * S.sum(0) + n * EPS * np.abs(t).sum(0)

    r, tol = {}, {}
    r["mass"], tol["mass"] = float(P["m"][fin].sum()), (n + 4) * EPS * float(P["m"][fin].sum())
    mx, t_mx = total("mx")
    mass = r["mass"]
    r["com"] = mx / mass if mass > 0 else np.zeros(3)
    tol["com"] = (t_mx + np.abs(mx) * tol["mass"] / mass) / mass + EPS * np.abs(r["com"]) if mass > 0 else np.zeros(3)
    for key, name in (("P", "P"), ("L", "L"), ("kinetic", "ke"), ("gravity", "ge"), ("elastic", "ee")):
        r[key], tol[key] = total(name)
    for key, vals, S, largest in (("sig_min", P["sig"][:, 2], P["S_sig"], False), ("sig_max", P["sig"][:, 0], P["S_sig"], True),
                                  ("det_min", P["det"], P["S_det"], False), ("strain_max", P["strain"], P["S_strain"], True),
                                  ("speed_max", P["speed"], P["S_speed"], True)):
        r[key], r[key + "_ip"] = _first_arg(vals, fin, largest)
        tol[key] = TOL * float(S[fin].max()) if n else 0.0
    r["nonfinite"], r["inverted"] = int((~fin).sum()), int((P["det"][fin] <= 0).sum())
    return r, tol
