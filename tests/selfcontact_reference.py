"""The self-contact law and its right-hand-side term in numpy (fp64): the restatement of include/pienerf_hip.h's text that csrc/pn_selfcontact.hip is
checked against (tests/test_selfcontact_host.py, tests/test_gpu_selfcontact.py).  Who is whose partner is decided by brute force over all pairs; the
header's cell and bucket rule is used only for what it fixes: the order of every sum and the overflow decision."""
import numpy as np

from contact_reference import contact_term, ip_state

DEFAULTS = dict(kappa=0.5, beta=0.5, mu=0.0)
BUCKET_CAP = 64
CELL_MAX = 2 ** 30


def params(dx, kappa=0.5, beta=0.5, mu=0.0, h=None, rho_x=None):
    h = float(dx) if h is None else float(h)
    return dict(kappa=float(kappa), beta=float(beta), mu=float(mu), h=h, rho_x=3.0 * h if rho_x is None else float(rho_x))


def n_buckets(n):
    T = 1024
    while T < 2 * n:
        T *= 2
    return T


def cells_of(x, h):
    """floor(x / h) per axis, clamped to [-2^30, 2^30] (valid points only)."""
    return np.clip(np.floor(np.asarray(x, np.float64) / h), -CELL_MAX, CELL_MAX).astype(np.int64)


def bucket_of(c, T):
    u = np.asarray(c, np.int64) & 0xFFFFFFFF
    k = ((u[..., 0] * 73856093) & 0xFFFFFFFF) ^ ((u[..., 1] * 19349663) & 0xFFFFFFFF) ^ ((u[..., 2] * 83492791) & 0xFFFFFFFF)
    return k & (T - 1)


def taking_part(x, v):
    return np.isfinite(x).all(axis=1) & np.isfinite(v).all(axis=1)


def overflows(x, v, h):
    """Whether a bucket of the hashed grid holds more than 64 points: the call then adds exactly nothing.  Also the largest bucket and the largest
    number of points in one cell."""
    ok = taking_part(x, v)
    c = cells_of(np.asarray(x)[ok], h)
    per_bucket = np.bincount(bucket_of(c, n_buckets(len(x))))
    per_cell = np.unique(c, axis=0, return_counts=True)[1]
    return bool(per_bucket.max(initial=0) > BUCKET_CAP), int(per_bucket.max(initial=0)), int(per_cell.max(initial=0))


def eligible(X, rho_x):
    """[n, n] bool: i != j and |X_i - X_j| >= rho_x, the squares summed as (q0 + q1) + q2."""
    d = X[:, None, :] - X[None, :, :]
    q = d * d
    e = np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2]) >= rho_x
    np.fill_diagonal(e, False)
    return e


def partners(x, v, X, h, rho_x):
    """For every point the list of (j, delta, L) of its partners in the header's visiting order: the 27 cells oz outermost, each offset -1, 0, 1, inside a
    cell ascending j.  Membership is brute force: eligible, both taking part, delta = h - L > 0."""
    x, X = np.asarray(x, np.float64), np.asarray(X, np.float64)
    n = len(x)
    ok = taking_part(x, v)
    xs = np.where(ok[:, None], x, 0.0)
    r = xs[:, None, :] - xs[None, :, :]
    L = np.sqrt((r * r).sum(axis=2))
    delta = h - L
    on = eligible(X, rho_x) & ok[:, None] & ok[None, :] & (delta > 0.0)
    c = cells_of(xs, h)
    out = []
    for i in range(n):
        js = np.nonzero(on[i])[0]
        o = c[js] - c[i]
        assert (np.abs(o) <= 1).all()                   # L < h: the partner's cell is one of the 27
        order = np.lexsort((js, o[:, 0], o[:, 1], o[:, 2]))
        out.append([(int(j), float(delta[i, j]), float(L[i, j])) for j in js[order]])
    return out


def point_sums(part):
    S = np.zeros(len(part))
    for i, ps in enumerate(part):
        s = 0.0
        for _, d, _ in ps:
            s += d
        S[i] = s
    return S


def pair_weights(part, S):
    """w_ij for every directed pair, as {(i, j): w}."""
    return {(i, j): d / max(S[i], S[j]) for i, ps in enumerate(part) for j, d, _ in ps}


def self_accel(x, v, X, m, dt, kappa, beta, mu, h, rho_x):
    """(a [n, 3], S [n], part): the law at every point.  An overflowed call gives zeros (overflows() decides)."""
    x, v, X, m = (np.asarray(t, np.float64) for t in (x, v, X, m))
    n = len(x)
    a, part = np.zeros((n, 3)), [[] for _ in range(n)]
    if overflows(x, v, h)[0]:
        return a, np.zeros(n), part
    part = partners(x, v, X, h, rho_x)
    S = point_sums(part)
    for i, ps in enumerate(part):
        acc = np.zeros(3)
        for j, delta, L in ps:
            r = x[i] - x[j]
            nh = r / L if L > 0.0 else np.array([0.0, 1.0 if i < j else -1.0, 0.0])
            wij = delta / max(S[i], S[j])
            w = v[i] - v[j]
            wn = float(w @ nh)
            wt = w - wn * nh
            g = wij * (kappa * delta + beta * min(max(-wn, 0.0) * dt, delta)) / (dt * dt)
            f = g * nh
            lt = float(np.sqrt(wt @ wt))
            if lt > 0.0:
                f = f - (min(mu * g, wij * lt / dt) / lt) * wt
            acc = acc + (m[j] / (m[i] + m[j])) * f
        a[i] = acc
    return a, S, part


def term_of(n_k, topo, Nx, m, a):
    return contact_term(n_k, topo, Nx, m, a)


def oracle_self_term(ref, par):
    """(term [10 n_k, 3], a [n_IP, 3]) for the current state of an OracleSimulator."""
    topo = ref.IP_kernel.numpy()
    x, v = ip_state(topo, ref.IP_Nx, ref.dof, ref.dof_vel)
    m = np.asarray(ref.IP_rho, np.float64) * ref.dx ** 3
    a = self_accel(x, v, np.asarray(ref.IP_pos, np.float64), m, ref.dt, **par)[0]
    return contact_term(ref.n_k, topo, ref.IP_Nx, m, a), a


class OracleSelf:
    """The oracle with self-contact: before every stepforward() its public rhs_gravity is g0 + extra(k) + term(state), summed in that order.  `extra`:
    callable(k) -> a sequence of [10 n_k, 3] terms, the earlier stages' of the chain rhs_gravity -> pins -> contact -> fields -> self (evaluated on this
    oracle's current state), or None.  par None: no self-contact term (the same run without the stage)."""

    def __init__(self, ref, par, extra=None):
        self.ref, self.par = ref, par
        self.g0 = ref.rhs_gravity.copy()
        self.extra = extra
        self.k, self.hits = 0, 0

    def step(self):
        r = self.ref
        rhs = self.g0.copy()
        if self.extra is not None:
            for part in self.extra(self.k):
                rhs = rhs + part
        if self.par is not None:
            term, a = oracle_self_term(r, self.par)
            self.hits = int(a.any(axis=1).sum())
            rhs = rhs + term
        r.rhs_gravity = rhs
        r.stepforward()
        self.k += 1
        return r.dof - r.dof_rest

    def ip_positions(self):
        return ip_state(self.ref.IP_kernel.numpy(), self.ref.IP_Nx, self.ref.dof, self.ref.dof_vel)[0]


def global_map(kernel_pos, A):
    """dof [n_k, 10, 3] of the global map x = A X: translation = A kernel_pos, affine columns = A, quadratic = 0."""
    A = np.asarray(A, np.float64)
    kp = np.asarray(kernel_pos, np.float64)
    dof = np.zeros((len(kp), 10, 3))
    dof[:, 0, :] = kp @ A.T
    dof[:, 1:4, :] = A.T[None, :, :]
    return dof
