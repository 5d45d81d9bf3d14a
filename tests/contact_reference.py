"""The contact law and its right-hand-side term in numpy (fp64, np.add.at): the restatement of include/pienerf_hip.h's text that csrc/pn_contact.hip is
checked against (tests/test_contact_host.py, tests/test_gpu_contact.py).  Colliders are dicts: dict(kind="plane", p=, n=, v=) with n normalised here once,
dict(kind="sphere" | "container", p=, R=, v=)."""
import numpy as np

DEFAULTS = dict(kappa=0.5, beta=0.5, mu=0.5)


def plane(point, normal, velocity=(0.0, 0.0, 0.0)):
    n = np.asarray(normal, np.float64)
    return dict(kind="plane", p=np.asarray(point, np.float64), n=n / np.linalg.norm(n), v=np.asarray(velocity, np.float64))


def sphere(centre, radius, inside=False, velocity=(0.0, 0.0, 0.0)):
    return dict(kind="container" if inside else "sphere", p=np.asarray(centre, np.float64), R=float(radius), v=np.asarray(velocity, np.float64))


def distance_normal(col, x):
    """(d [n], nh [n, 3]) of one collider at the points x [n, 3]: signed distance, unit normal out of the solid."""
    x = np.asarray(x, np.float64)
    r = x - col["p"][None, :]
    if col["kind"] == "plane":
        return r @ col["n"], np.broadcast_to(col["n"], x.shape).copy()
    L = np.sqrt((r * r).sum(axis=1))
    nh = np.zeros_like(x)
    ok = L > 0.0
    nh[ok] = r[ok] / L[ok, None]
    nh[~ok] = (0.0, 1.0, 0.0)
    if col["kind"] == "sphere":
        return L - col["R"], nh
    return col["R"] - L, -nh


def contact_parts(col, x, v, dt, kappa, beta, mu, h):
    """One collider's (delta, a_n, a_t, nh, w_t) at the points x with velocities v."""
    d, nh = distance_normal(col, x)
    delta = np.maximum(h - d, 0.0)
    w = np.asarray(v, np.float64) - col["v"][None, :]
    wn = (w * nh).sum(axis=1)
    wt = w - wn[:, None] * nh
    an = (kappa * delta + beta * np.minimum(np.maximum(-wn, 0.0) * dt, delta)) / (dt * dt)
    at = np.minimum(mu * an, np.sqrt((wt * wt).sum(axis=1)) / dt)
    an, at = np.where(delta > 0.0, an, 0.0), np.where(delta > 0.0, at, 0.0)   # delta = 0: exactly nothing (a_t is 0 there anyway: min(mu 0, .))
    return delta, an, at, nh, wt


def contact_accel(colliders, x, v, dt, kappa, beta, mu, h):
    """(a [n, 3], in_contact [n] bool): the colliders visited in index order; a collider with delta = 0 adds exactly nothing."""
    x = np.asarray(x, np.float64)
    a = np.zeros_like(x)
    hit = np.zeros(len(x), bool)
    for col in colliders:
        if col is None:
            continue
        delta, an, at, nh, wt = contact_parts(col, x, v, dt, kappa, beta, mu, h)
        on = delta > 0.0
        hit |= on
        a[on] += an[on, None] * nh[on]
        L = np.sqrt((wt * wt).sum(axis=1))
        fr = on & (L > 0.0)
        a[fr] -= (at[fr] / L[fr])[:, None] * wt[fr]
    return a, hit


def ip_state(topo, Nx, dof, dof_vel):
    """x_i, v_i [n_IP, 3] = sum_slot sum_c Nx[i, slot, c] dof[topo[i, slot] 10 + c, :] (and over dof_vel), fp64."""
    t = np.asarray(topo, np.int64)
    n_k = np.asarray(dof).size // 30
    N = np.asarray(Nx, np.float64)
    x = np.einsum("nic,nicr->nr", N, np.asarray(dof, np.float64).reshape(n_k, 10, 3)[t])
    v = np.einsum("nic,nicr->nr", N, np.asarray(dof_vel, np.float64).reshape(n_k, 10, 3)[t])
    return x, v


def contact_term(n_k, topo, Nx, m, a):
    """sum m_i Nx[i, slot, j] a_i[r] into row topo[i, slot] 10 + j, as [10 n_k, 3] (the layout of dof), exactly as collect_gravity adds gravity."""
    out = np.zeros((n_k * 10, 3))
    rows = (np.asarray(topo, np.int64)[:, :, None] * 10 + np.arange(10)[None, None, :]).reshape(-1)
    np.add.at(out, rows, (np.asarray(m)[:, None, None] * np.asarray(Nx, np.float64)).reshape(-1)[:, None] * np.repeat(a, 80, axis=0))
    return out


def oracle_term(ref, colliders, kappa, beta, mu, h):
    """(term [10 n_k, 3], a [n_IP, 3], in_contact [n_IP]) for the current state of an OracleSimulator."""
    topo = ref.IP_kernel.numpy()
    x, v = ip_state(topo, ref.IP_Nx, ref.dof, ref.dof_vel)
    a, hit = contact_accel(colliders, x, v, ref.dt, kappa, beta, mu, h)
    m = ref.IP_rho * ref.dx ** 3
    return contact_term(ref.n_k, topo, ref.IP_Nx, m, a), a, hit


class OracleContact:
    """The oracle with colliders: before every stepforward() its public rhs_gravity is g0 + extra() + term(state)."""

    def __init__(self, ref, colliders, kappa=0.5, beta=0.5, mu=0.5, h=None, extra=None):
        self.ref, self.colliders = ref, list(colliders)
        self.par = dict(kappa=kappa, beta=beta, mu=mu, h=0.5 * ref.dx if h is None else h)
        self.g0 = ref.rhs_gravity.copy()
        self.extra = extra          # callable(k) -> [10 n_k, 3] (the pins' term), or None
        self.k, self.hits = 0, 0

    def step(self):
        r = self.ref
        term, _, hit = oracle_term(r, self.colliders, **self.par)
        r.rhs_gravity = self.g0 + term
        if self.extra is not None:
            r.rhs_gravity = r.rhs_gravity + self.extra(self.k)
        r.stepforward()
        self.k += 1
        self.hits = int(hit.sum())
        return r.dof - r.dof_rest

    def ip_positions(self):
        return ip_state(self.ref.IP_kernel.numpy(), self.ref.IP_Nx, self.ref.dof, self.ref.dof_vel)[0]
