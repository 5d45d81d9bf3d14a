"""The force-field law and its right-hand-side term in numpy (fp64): the restatement of include/pienerf_hip.h's text that csrc/pn_fields.hip is checked
against (tests/test_fields_host.py, tests/test_gpu_fields.py).  Fields are dicts: wind(...), vortex(...) with the axis normalised here once, radial(...);
a slot may be None (empty)."""
import numpy as np

from contact_reference import contact_term, ip_state


def wind(velocity, drag=2.0, gust=0.0, hz=0.0, phase=0.0, wave=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), start=0.0, stop=None):
    return dict(kind="wind", p=np.asarray(origin, np.float64), W=np.asarray(velocity, np.float64), c=float(drag), g=float(gust), f=float(hz),
                phi=float(phase), kv=np.asarray(wave, np.float64), t0=float(start), t1=np.inf if stop is None else float(stop))


def air_drag(drag):
    return wind((0.0, 0.0, 0.0), drag=drag)


def vortex(point, axis, omega, radius, drag=2.0, start=0.0, stop=None):
    n = np.asarray(axis, np.float64)
    return dict(kind="vortex", p=np.asarray(point, np.float64), n=n / np.linalg.norm(n), omega=float(omega), R=float(radius), c=float(drag),
                t0=float(start), t1=np.inf if stop is None else float(stop))


def radial(centre, strength, radius, start=0.0, stop=None):
    return dict(kind="radial", p=np.asarray(centre, np.float64), s=float(strength), R=float(radius), t0=float(start), t1=np.inf if stop is None else float(stop))


def fall(q, R):
    w = np.maximum(1.0 - q / R, 0.0)
    return w * w


def field_accel(fields, x, v, t, dt):
    """a [n, 3]: the fields visited in index order, each only while t0 <= t < t1; c_eff = min(c, 1 / dt), s_eff = sign(s) min(|s|, R / (2 dt^2)).  An
    empty slot (None), a closed window, a point at or beyond R and a point at a radial field's centre add exactly nothing."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    a = np.zeros_like(x)
    for f in fields:
        if f is None or not (f["t0"] <= t < f["t1"]):
            continue
        r = x - f["p"][None, :]
        if f["kind"] == "wind":
            c = min(f["c"], 1.0 / dt)
            u = f["W"][None, :] * (1.0 + f["g"] * np.sin(2.0 * np.pi * (f["f"] * t - r @ f["kv"]) + f["phi"]))[:, None]
            a += c * (u - v)
        elif f["kind"] == "vortex":
            c, n = min(f["c"], 1.0 / dt), f["n"]
            q = r - (r @ n)[:, None] * n[None, :]
            w = fall(np.sqrt((q * q).sum(axis=1)), f["R"])
            on = w > 0.0
            a[on] += (c * w[on])[:, None] * (f["omega"] * np.cross(n[None, :], r[on]) - v[on])
        else:
            L = np.sqrt((r * r).sum(axis=1))
            w = fall(L, f["R"])
            on = (L > 0.0) & (w > 0.0)
            s = np.copysign(min(abs(f["s"]), f["R"] / (2.0 * dt * dt)), f["s"])
            a[on] += (s * w[on] / L[on])[:, None] * r[on]
    return a


def oracle_field_term(ref, fields, t):
    """(term [10 n_k, 3], a [n_IP, 3]) for the current state of an OracleSimulator at time t."""
    topo = ref.IP_kernel.numpy()
    x, v = ip_state(topo, ref.IP_Nx, ref.dof, ref.dof_vel)
    a = field_accel(fields, x, v, t, ref.dt)
    return contact_term(ref.n_k, topo, ref.IP_Nx, ref.IP_rho * ref.dx ** 3, a), a


class OracleFields:
    """The oracle with force fields: before every stepforward() its public rhs_gravity is g0 + extra(k) + term(state, k dt), summed in that order.
    `extra`: callable(k) -> a sequence of [10 n_k, 3] terms, the pins' and contact's of the chain rhs_gravity -> pins -> contact -> fields (evaluated on
    this oracle's current state, before the field term), or None.  `fields` may be changed between steps; `k` is the fields' clock."""

    def __init__(self, ref, fields, extra=None):
        self.ref, self.fields = ref, list(fields)
        self.g0 = ref.rhs_gravity.copy()
        self.extra = extra
        self.k = 0

    def step(self):
        r = self.ref
        rhs = self.g0.copy()
        if self.extra is not None:
            for part in self.extra(self.k):     # the pins' term, then contact's: added one after the other, as the device's launches add them
                rhs = rhs + part
        term, self.accel = oracle_field_term(r, self.fields, self.k * r.dt)
        r.rhs_gravity = rhs + term
        r.stepforward()
        self.k += 1
        return r.dof - r.dof_rest

    def ip_positions(self):
        return ip_state(self.ref.IP_kernel.numpy(), self.ref.IP_Nx, self.ref.dof, self.ref.dof_vel)[0]

    def kinetic_energy(self):
        """1/2 sum_i m_i |v_i|^2 over the integration points."""
        v = ip_state(self.ref.IP_kernel.numpy(), self.ref.IP_Nx, self.ref.dof, self.ref.dof_vel)[1]
        return float(0.5 * ((self.ref.IP_rho * self.ref.dx ** 3) * (v * v).sum(axis=1)).sum())


def kernel_order_walk(bg, cnt, buf, Nx_csr, m, a, kid):
    """csrc/pn_fields.hip's k_field_rhs walked in numpy for kernel `kid`'s run: 256 threads striding the run in ascending order (an entry whose point has
    a = 0 is skipped), the shuffle tree 32, 16 ... 1 inside each of the four waves, the waves added as ((w0 + w1) + w2) + w3.  Returns the 30 sums."""
    lanes = np.zeros((256, 30))
    for e in range(bg[kid], bg[kid] + cnt[kid]):
        p = buf[e] >> 3
        if a[p].any():
            lanes[(e - bg[kid]) % 256] += np.outer(m[p] * Nx_csr[e], a[p]).reshape(-1)
    waves = lanes.reshape(4, 64, 30).copy()
    w = 32
    while w:
        waves[:, :w] += waves[:, w:2 * w]
        w //= 2
    return ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]
