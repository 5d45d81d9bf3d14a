"""The rigid balls' law in numpy (fp64): the restatement of include/pienerf_hip.h's text (pn_bodies_state) that csrc/pn_bodies.hip is checked against
(tests/test_bodies_host.py, tests/test_gpu_bodies.py), built on tests/contact_reference.py.  A body is a sphere collider dict of contact_reference
(kind="sphere", p, R, v) with mass M and damping c beside it; its p and v are the collider's own, as on the device."""
import numpy as np

from contact_reference import OracleContact, contact_parts, ip_state


def body(centre, radius, mass, velocity=(0.0, 0.0, 0.0), damping=0.0):
    return dict(kind="sphere", p=np.asarray(centre, np.float64).copy(), R=float(radius), v=np.asarray(velocity, np.float64).copy(), M=float(mass),
                c=float(damping), F=np.zeros(3), s=1.0, delta_max=0.0, clamped=0)


def is_body(col):
    return col is not None and "M" in col


def one_collider_accel(col, x, v, dt, kappa, beta, mu, h):
    """(a [n, 3], delta [n]): one collider's own part of the contact law at the points x with velocities v."""
    delta, an, at, nh, wt = contact_parts(col, x, v, dt, kappa, beta, mu, h)
    a = an[:, None] * nh
    L = np.sqrt((wt * wt).sum(axis=1))
    fr = (delta > 0.0) & (L > 0.0)
    a[fr] -= (at[fr] / L[fr])[:, None] * wt[fr]
    a[delta <= 0.0] = 0.0
    return a, delta


def reaction(col, x, v, m, dt, kappa, beta, mu, h):
    """(F_b [3], delta_max): F_b = - sum_i m_i a_{i,b}, the deepest penetration among the points in contact (0: none)."""
    a, delta = one_collider_accel(col, x, v, dt, kappa, beta, mu, h)
    return -(np.asarray(m)[:, None] * a).sum(axis=0), float(delta.max()) if len(delta) else 0.0


def clamp_scale(F, M, delta_max, dt):
    Fn = float(np.sqrt((F * F).sum()))
    return 1.0 if Fn == 0.0 else min(1.0, M * delta_max / (dt * dt * Fn))


def static_accel(b, colliders, dt, kappa, beta, mu):
    """a_static of body b: the non-dynamic colliders in index order, the law at the ball's centre with its radius as the thickness."""
    a = np.zeros(3)
    for col in colliders:
        if col is None or col is b or is_body(col):
            continue
        ai, _ = one_collider_accel(col, b["p"][None, :], b["v"][None, :], dt, kappa, beta, mu, b["R"])
        a += ai[0]
    return a


def step_bodies(colliders, x, v, m, dt, g, kappa, beta, mu, h, clamp=True):
    """One substep of every body among `colliders`, in place, everything evaluated from the state on entry.  x, v, m: the integration points'
    positions, velocities and masses (x None: no object).  clamp False: the unclamped law (what the clamp is compared with)."""
    g = np.asarray(g, np.float64)
    new = []
    for b in colliders:
        if not is_body(b):
            continue
        if x is None:
            F, dmax = np.zeros(3), 0.0
        else:
            F, dmax = reaction(b, x, v, m, dt, kappa, beta, mu, h)
        s = clamp_scale(F, b["M"], dmax, dt)
        a_st = static_accel(b, colliders, dt, kappa, beta, mu)
        u = (b["v"] + dt * (g + (s if clamp else 1.0) * F / b["M"] + a_st)) / (1.0 + dt * b["c"])
        new.append((b, F, s, dmax, u, b["p"] + dt * u))
    for b, F, s, dmax, u, p in new:
        b["F"], b["s"], b["delta_max"], b["v"], b["p"] = F, s, dmax, u, p
        b["clamped"] += int(s < 1.0)


class OracleBodies(OracleContact):
    """OracleContact whose sphere colliders may be bodies: step() evaluates the object's contact term and the bodies' substep from the same state, then
    steps the oracle and moves the balls."""

    def __init__(self, ref, colliders, gravity=(0.0, 0.0, 0.0), clamp=True, **kw):
        super().__init__(ref, colliders, **kw)
        self.gravity, self.clamp = np.asarray(gravity, np.float64), clamp

    def step(self):
        r = self.ref
        x, v = ip_state(r.IP_kernel.numpy(), r.IP_Nx, r.dof, r.dof_vel)
        m = r.IP_rho * r.dx ** 3
        # the balls' new state from the state the substep starts from; the colliders the object meets stay as they are until it has stepped
        moved = [dict(c, p=c["p"].copy(), v=c["v"].copy()) if c is not None else None for c in self.colliders]
        step_bodies(moved, x, v, m, r.dt, self.gravity, self.par["kappa"], self.par["beta"], self.par["mu"], self.par["h"], clamp=self.clamp)
        out = super().step()
        for c, n in zip(self.colliders, moved):
            if is_body(c):
                c.update(n)
        return out

    def bodies(self):
        return [c for c in self.colliders if is_body(c)]
