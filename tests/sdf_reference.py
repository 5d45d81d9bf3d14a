"""The signed-distance grid laws in numpy, fp64: the restatement of include/pienerf_hip.h's text that csrc/pn_sdf.hip is checked against
(tests/test_sdf_host.py, tests/test_gpu_sdf.py).  The builder's law (exact point-to-triangle distance by regions, generalised winding number) and the
contact term of a placed grid (trilinear distance, analytic gradient, contact's response from tests/contact_reference.py)."""
import numpy as np

from contact_reference import contact_accel


# ---------------------------------------------------------------- the builder
def tri_dist2(a, b, c):
    """Squared distance from the origin to the triangles with corners a, b, c [n, 3], by the regions of the closest point, in the order the law
    names: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face."""
    ab, ac = b - a, c - a
    dot = lambda u, v: (u * v).sum(axis=-1)
    d1, d2 = -dot(ab, a), -dot(ac, a)
    d3, d4 = -dot(ab, b), -dot(ac, b)
    d5, d6 = -dot(ab, c), -dot(ac, c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        e_ab = a + (d1 / (d1 - d3))[..., None] * ab
        e_ac = a + (d2 / (d2 - d6))[..., None] * ac
        e_bc = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)
        den = 1.0 / (va + vb + vc)
        face = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    p = face
    for cond, cand in reversed(list(zip(conds, [a, b, e_ab, c, e_ac, e_bc]))):   # the first condition that holds wins
        p = np.where(cond[..., None], cand, p)
    return dot(p, p)


def tri_angle(a, b, c):
    """2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)"""
    la, lb, lc = (np.sqrt((u * u).sum(axis=-1)) for u in (a, b, c))
    det = (a * np.cross(b, c)).sum(axis=-1)
    return 2.0 * np.arctan2(det, la * lb * lc + (a * b).sum(axis=-1) * lc + (b * c).sum(axis=-1) * la + (c * a).sum(axis=-1) * lb)


def node_positions(lo, s, res, fp32=True):
    """[nz, ny, nx, 3]: lo + s (i, j, k) in fp64, rounded to fp32 as the builder's nodes are (fp32=True), returned as fp64."""
    nx, ny, nz = res
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    q = np.asarray(lo, np.float64) + float(s) * np.stack([i, j, k], axis=-1).astype(np.float64)
    return q.astype(np.float32).astype(np.float64) if fp32 else q


def build(tri9, lo, s, res):
    """(phi [nz, ny, nx], w [nz, ny, nx], dist [nz, ny, nx]) of the builder's law in fp64, over the fp32 corners tri9 [T, 9] and the fp32 nodes."""
    q = node_positions(lo, s, res).reshape(-1, 3)
    T = np.asarray(tri9, np.float64).reshape(-1, 3, 3)
    best = np.full(len(q), np.inf)
    w = np.zeros(len(q))
    for t in T:
        a, b, c = (t[m][None, :] - q for m in range(3))
        best = np.fmin(best, tri_dist2(a, b, c))
        w += tri_angle(a, b, c)
    w /= 4.0 * np.pi
    dist = np.sqrt(best)
    nx, ny, nz = res
    phi = np.where(np.abs(w) >= 0.5, -dist, dist)
    return phi.reshape(nz, ny, nx), w.reshape(nz, ny, nx), dist.reshape(nz, ny, nx)


def box_distance(p, centre, half):
    """The analytic signed distance of an axis-aligned box at the points p [n, 3]."""
    q = np.abs(np.asarray(p, np.float64) - np.asarray(centre, np.float64)) - np.asarray(half, np.float64)
    return np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0.0)


# ---------------------------------------------------------------- sampling a grid
def lerp(a, b, f):
    return a + f * (b - a)


def sample(values, lo, s, x):
    """(inside [n] bool, d [n], g [n, 3]) at the points x [n, 3]: the trilinear interpolant of `values` [nz, ny, nx] (widened to fp64) and its gradient
    in u = (x - lo) / s, lerp along x, then y, then z.  A point with u outside [0, n - 1) on any axis, or not finite, is not inside (d = g = 0)."""
    V = np.asarray(values, np.float64)
    nz, ny, nx = V.shape
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        u = (x - np.asarray(lo, np.float64)[None, :]) / float(s)
        ok = ((u >= 0.0) & (u < np.array([nx - 1, ny - 1, nz - 1], np.float64)[None, :])).all(axis=1)
    u = np.where(ok[:, None], u, 0.0)
    i0 = np.floor(u).astype(np.int64)
    f = u - i0
    i, j, k = i0[:, 0], i0[:, 1], i0[:, 2]
    v = {(a, b, c): V[k + c, j + b, i + a] for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
    c00, c10 = lerp(v[0, 0, 0], v[1, 0, 0], f0), lerp(v[0, 1, 0], v[1, 1, 0], f0)
    c01, c11 = lerp(v[0, 0, 1], v[1, 0, 1], f0), lerp(v[0, 1, 1], v[1, 1, 1], f0)
    c0, c1 = lerp(c00, c10, f1), lerp(c01, c11, f1)
    d = lerp(c0, c1, f2)
    g0 = lerp(lerp(v[1, 0, 0] - v[0, 0, 0], v[1, 1, 0] - v[0, 1, 0], f1), lerp(v[1, 0, 1] - v[0, 0, 1], v[1, 1, 1] - v[0, 1, 1], f1), f2)
    g1 = lerp(c10 - c00, c11 - c01, f2)
    g2 = c1 - c0
    g = np.stack([g0, g1, g2], axis=1)
    return ok, np.where(ok, d, 0.0), np.where(ok[:, None], g, 0.0)


# ---------------------------------------------------------------- contact against placed grids
def mesh_collider(values, lo, s, offset=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0)):
    return dict(values=np.asarray(values, np.float64), lo=np.asarray(lo, np.float64) + np.asarray(offset, np.float64), s=float(s),
                v=np.asarray(velocity, np.float64))


def sdf_accel(meshes, x, v, dt, kappa, beta, mu, h, a=None, hit=None):
    """(a [n, 3], in_contact [n]): the grids' terms added, in slot order, to the analytic colliders' `a` / `hit` (zeros / False when None): per
    slot, contact's response to the distance d and the unit normal nh = g / |g| ((0, 1, 0) for g = 0) at the points inside the grid's box."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    a = np.zeros_like(x) if a is None else np.array(a, np.float64)
    hit = np.zeros(len(x), bool) if hit is None else np.array(hit, bool)
    for m in meshes:
        if m is None:
            continue
        ok, d, g = sample(m["values"], m["lo"], m["s"], x)
        L = np.sqrt((g * g).sum(axis=1))
        nh = np.where((L > 0.0)[:, None], g / np.where(L > 0.0, L, 1.0)[:, None], np.array([0.0, 1.0, 0.0])[None, :])
        delta = np.where(ok, np.maximum(h - d, 0.0), 0.0)
        w = v - m["v"][None, :]
        wn = (w * nh).sum(axis=1)
        wt = w - wn[:, None] * nh
        an = (kappa * delta + beta * np.minimum(np.maximum(-wn, 0.0) * dt, delta)) / (dt * dt)
        Lt = np.sqrt((wt * wt).sum(axis=1))
        at = np.minimum(mu * an, Lt / dt)
        on = delta > 0.0
        hit |= on
        a[on] += an[on, None] * nh[on]
        fr = on & (Lt > 0.0)
        a[fr] -= (at[fr] / Lt[fr])[:, None] * wt[fr]
    return a, hit


def contact_and_sdf_accel(colliders, meshes, x, v, dt, kappa, beta, mu, h):
    """The analytic colliders in index order (contact_reference.contact_accel), then the grids in slot order."""
    a, hit = contact_accel(colliders, x, v, dt, kappa, beta, mu, h)
    return sdf_accel(meshes, x, v, dt, kappa, beta, mu, h, a, hit)
