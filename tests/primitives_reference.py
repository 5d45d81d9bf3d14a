"""numpy restatements for the box and capsule colliders (include/pienerf_hip.h: pn_contact_collider, pn_draw_colliders, pn_draw_colliders_shadowed).

The contact law: `distance_normal` adds dict(kind="box", p=centre, n=half-extents, v=) and dict(kind="capsule", p=A, n=B - A, R=, v=) to
contact_reference's colliders, and `contact_accel` / `oracle_term` are that module's functions over all five kinds, in fp64.  `regions` names where a
point lies with respect to a box (face, edge, corner, inside axis) or a capsule (cap A, body, cap B): the GPU test asserts its cases cover them all.

The drawn frame: `draw` evaluates the overlay's law for every ray in float32, one rounding per operation in the kernel's order, for all five types,
with the shadow lookup when a light is given (shadows_reference.occlusion for the map and the spheres; the boxes and capsules here).  A state of planes,
spheres and the container takes exactly colliders_reference.draw's operations.  Its flag `near` marks rays where two of the NEW decisions' operands lie
within a few ulp of each other (a box's face tie or edge graze, a capsule's part tie, the near root against t_min): the tests leave those out, and
assert that they are few.  Colliders are (type, geom10) as Simulator keeps them.
"""
from collections import namedtuple

import numpy as np

import colliders_reference as cr
import contact_reference as cref
import shadows_reference as sr

BOX, CAPSULE = 4, 5
ULPS = 4.0

Drawn = namedtuple("Drawn", "image coverage t slot face front near occ")


# ------------------------------------------------------------------------------------------------ the contact law
def box(centre, half_extents, velocity=(0.0, 0.0, 0.0)):
    return dict(kind="box", p=np.asarray(centre, np.float64), n=np.asarray(half_extents, np.float64), v=np.asarray(velocity, np.float64))


def capsule(a, b, radius, velocity=(0.0, 0.0, 0.0)):
    a = np.asarray(a, np.float64)
    return dict(kind="capsule", p=a, n=np.asarray(b, np.float64) - a, R=float(radius), v=np.asarray(velocity, np.float64))


def slot_of(col):
    """The reference's dict as the (type, geom10) the Simulator keeps."""
    g = np.zeros(10)
    g[0:3], g[7:10] = col["p"], col["v"]
    if col["kind"] == "box":
        g[3:6] = col["n"]
        return BOX, g
    assert col["kind"] == "capsule"
    g[3:6], g[6] = col["n"], col["R"]
    return CAPSULE, g


def capsule_s(col, x):
    n = col["n"]
    r = np.asarray(x, np.float64) - col["p"][None, :]
    return np.minimum(np.maximum((r[:, 0] * n[0] + r[:, 1] * n[1] + r[:, 2] * n[2]) / (n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 0.0), 1.0)


def distance_normal(col, x):
    """(d [n], nh [n, 3]) of one collider at the points x [n, 3]; planes, spheres and the container are contact_reference's."""
    x = np.asarray(x, np.float64)
    if col["kind"] == "box":
        r = x - col["p"][None, :]
        q = np.abs(r) - col["n"][None, :]
        sg = np.where(r >= 0.0, 1.0, -1.0)
        outside = q.max(axis=1) > 0.0
        e = np.maximum(q, 0.0)
        d_out = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        with np.errstate(all="ignore"):
            nh_out = sg * e / d_out[:, None]
        k = np.argmax(q, axis=1)          # the first axis that reaches the maximum: the lowest index on ties
        rows = np.arange(len(x))
        nh_in = np.zeros_like(x)
        nh_in[rows, k] = sg[rows, k]
        return np.where(outside, d_out, q[rows, k]), np.where(outside[:, None], nh_out, nh_in)
    if col["kind"] == "capsule":
        s = capsule_s(col, x)
        c = col["p"][None, :] + s[:, None] * col["n"][None, :]
        r = x - c
        L = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        nh = np.zeros_like(x)
        ok = L > 0.0
        nh[ok] = r[ok] / L[ok, None]
        nh[~ok] = (0.0, 1.0, 0.0)
        return L - col["R"], nh
    return cref.distance_normal(col, x)


def contact_parts(col, x, v, dt, kappa, beta, mu, h):
    """contact_reference.contact_parts over distance_normal above."""
    d, nh = distance_normal(col, x)
    delta = np.maximum(h - d, 0.0)
    w = np.asarray(v, np.float64) - col["v"][None, :]
    wn = (w * nh).sum(axis=1)
    wt = w - wn[:, None] * nh
    an = (kappa * delta + beta * np.minimum(np.maximum(-wn, 0.0) * dt, delta)) / (dt * dt)
    at = np.minimum(mu * an, np.sqrt((wt * wt).sum(axis=1)) / dt)
    an, at = np.where(delta > 0.0, an, 0.0), np.where(delta > 0.0, at, 0.0)
    return delta, an, at, nh, wt


def contact_accel(colliders, x, v, dt, kappa, beta, mu, h):
    """contact_reference.contact_accel over all five kinds."""
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


def oracle_term(ref, colliders, kappa, beta, mu, h):
    """(term [10 n_k, 3], a, in_contact) for the current state of an OracleSimulator: contact_reference.oracle_term over all five kinds."""
    topo = ref.IP_kernel.numpy()
    x, v = cref.ip_state(topo, ref.IP_Nx, ref.dof, ref.dof_vel)
    a, hit = contact_accel(colliders, x, v, ref.dt, kappa, beta, mu, h)
    return cref.contact_term(ref.n_k, topo, ref.IP_Nx, ref.IP_rho * ref.dx ** 3, a), a, hit


def regions(col, x):
    """Where the points lie.  Box: a string per point — 'in0'..'in2' (inside, the law's axis) or the outside region as three characters, one per axis,
    '-', '0', '+' (q_i > 0 with that sign, or '0'): one non-zero is a face, two an edge, three a corner.  Capsule: 'A', 'body' or 'B'."""
    x = np.asarray(x, np.float64)
    if col["kind"] == "box":
        r = x - col["p"][None, :]
        q = np.abs(r) - col["n"][None, :]
        out = []
        for ri, qi in zip(r, q):
            if qi.max() > 0.0:
                out.append("".join("0" if qv <= 0.0 else ("+" if rv >= 0.0 else "-") for rv, qv in zip(ri, qi)))
            else:
                out.append(f"in{int(np.argmax(qi))}")
        return out
    s = capsule_s(col, x)
    return ["A" if v == 0.0 else ("B" if v == 1.0 else "body") for v in s]


BOX_REGIONS = sorted({"".join(t) for t in np.array(np.meshgrid(*[list("-0+")] * 3)).T.reshape(-1, 3) if "".join(t) != "000"} | {"in0", "in1", "in2"})


def brute_distance(col, x, n=60):
    """The distance from every point of x to a dense sampling of the collider's surface, and the sampling's resolution (largest gap between samples)."""
    if col["kind"] == "box":
        p, h = col["p"], col["n"]
        pts = []
        for k in range(3):
            i, j = [a for a in range(3) if a != k]
            u, v = np.meshgrid(np.linspace(-h[i], h[i], n), np.linspace(-h[j], h[j], n), indexing="ij")
            for sgn in (-1.0, 1.0):
                f = np.zeros((n * n, 3))
                f[:, i], f[:, j], f[:, k] = u.reshape(-1), v.reshape(-1), sgn * h[k]
                pts.append(f + p)
        res = 2.0 * float(h.max()) / (n - 1)
    else:
        A, nn, R = col["p"], col["n"], col["R"]
        L = np.linalg.norm(nn)
        ax = nn / L
        e = np.eye(3)[np.argmin(np.abs(ax))]
        u = np.cross(ax, e)
        u /= np.linalg.norm(u)
        w = np.cross(ax, u)
        ph = np.linspace(0.0, 2.0 * np.pi, 2 * n, endpoint=False)
        ring = np.cos(ph)[:, None] * u + np.sin(ph)[:, None] * w
        zs = np.linspace(0.0, L, n)
        pts = [(A + z * ax)[None] + R * ring for z in zs]
        th = np.linspace(0.0, 0.5 * np.pi, n // 2)
        for t in th:
            pts.append((A - R * np.sin(t) * ax)[None] + R * np.cos(t) * ring)
            pts.append((A + nn + R * np.sin(t) * ax)[None] + R * np.cos(t) * ring)
        res = max(L / (n - 1), 2.0 * np.pi * R / (2 * n), 0.5 * np.pi * R / (n // 2 - 1))
    P = np.concatenate(pts)
    x = np.asarray(x, np.float64)
    d = np.empty(len(x))
    for b in range(0, len(x), 256):
        d[b:b + 256] = np.sqrt(((x[b:b + 256, None, :] - P[None]) ** 2).sum(axis=2)).min(axis=1)
    return d, res


# ------------------------------------------------------------------------------------------------ the drawn frame, float32
F = np.float32


def _close(a, b):
    """|a - b| within ULPS ulp of the larger: two correct evaluations may order them differently."""
    with np.errstate(all="ignore"):
        return np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= F(ULPS) * np.spacing(np.maximum(np.abs(a), np.abs(b))))


def box_interval(p, h, o, d):
    """pn_box_interval: (hit, t_enter, t_exit, f_enter, f_exit, near) for rays (o, d) [N, 3] against the box (p, h), all float32."""
    N = o.shape[0]
    te, tx = np.full(N, -np.inf, F), np.full(N, np.inf, F)
    fe, fx = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    inside = np.ones(N, bool)
    near = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            par = d[:, i] == F(0)
            inside &= ~par | (np.abs(o[:, i] - p[i]) < h[i])
            t1, t2 = ((p[i] - h[i]) - o[:, i]) / d[:, i], ((p[i] + h[i]) - o[:, i]) / d[:, i]
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            near |= ~par & (_close(lo, te) | _close(hi, tx))      # a face tie
            up, dn = ~par & (lo > te), ~par & (hi < tx)
            te, fe = np.where(up, lo, te), np.where(up, i, fe)
            tx, fx = np.where(dn, hi, tx), np.where(dn, i, fx)
        near |= _close(te, tx)                                    # the ray grazes an edge
    return inside & (te < tx), te, tx, fe, fx, near & inside


def sphere_interval(c, R, o, d, q):
    """pn_sphere_interval: (hit, t_near, t_far)."""
    with np.errstate(all="ignore"):
        oc = o - c[None]
        b = cr._dot(oc, d)
        disc = b * b - q * (cr._dot(oc, oc) - R * R)
        ok = disc > F(0)
        sq = np.sqrt(np.where(ok, disc, F(0)))
        return ok, (-b - sq) / q, (-b + sq) / q


def capsule_frame(p, n):
    """pn_load_slot's capsule fields in float32: (unit axis, B, len)."""
    ln = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    return (n / ln).astype(F), (p + n).astype(F), F(ln)


def capsule_interval(p, n, R, o, d, q):
    """pn_capsule_interval: (hit, t_near, t_far, near)."""
    ax, B, ln = capsule_frame(p, n)
    N = o.shape[0]
    inf = F(np.inf)
    with np.errstate(all="ignore"):
        okA, nA, fA = sphere_interval(p, R, o, d, q)
        okB, nB, fB = sphere_interval(B, R, o, d, q)
        tn, tf = np.where(okA, nA, inf), np.where(okA, fA, -inf)
        near = okA & okB & (_close(nA, nB) | _close(fA, fB))
        tn, tf = np.where(okB, np.minimum(tn, nB), tn), np.where(okB, np.maximum(tf, fB), tf)
        oc = o - p[None]
        ad, ao = cr._dot(ax[None], d), cr._dot(ax[None], oc)
        dp, op = d - ad[:, None] * ax[None], oc - ao[:, None] * ax[None]
        A2, b = cr._dot(dp, dp), cr._dot(op, dp)
        disc = b * b - A2 * (cr._dot(op, op) - R * R)
        okC = (A2 > F(0)) & (disc > F(0))
        sq = np.sqrt(np.where(okC, disc, F(0)))
        lo, hi = (-b - sq) / A2, (-b + sq) / A2
        par = ad == F(0)
        s1, s2 = (F(0) - ao) / ad, (ln - ao) / ad
        lo = np.where(par, lo, np.maximum(lo, np.minimum(s1, s2)))
        hi = np.where(par, hi, np.minimum(hi, np.maximum(s1, s2)))
        near |= okC & _close(lo, hi)
        okC &= np.where(par, (ao > F(0)) & (ao < ln), True) & (lo < hi)
        near |= okC & (okA | okB) & (_close(lo, tn) | _close(hi, tf))      # a part tie: which part gives the end
        tn, tf = np.where(okC, np.minimum(tn, lo), tn), np.where(okC, np.maximum(tf, hi), tf)
    hit = okA | okB | okC
    assert tn.dtype == F and tf.dtype == F
    return hit, tn, tf, near & hit


def _casters(lt, colliders, k_hit, x):
    """occ_sph's new part: 1 where a box or a capsule other than k_hit blocks the light ray x + s L, s > 0."""
    L = np.broadcast_to(np.asarray(lt["L"], F)[None], x.shape)
    qL = cr._dot(L, L)
    occ = np.zeros(x.shape[0], F)
    if not lt["spheres"]:
        return occ
    for k2, c2 in enumerate(colliders):
        if c2 is None or k2 == k_hit or c2[0] not in (BOX, CAPSULE):
            continue
        p, n, R = (np.asarray(v, np.float64).astype(F) for v in (c2[1][0:3], c2[1][3:6], c2[1][6]))
        if c2[0] == BOX:
            hit, te, tx, _, _, _ = box_interval(p, n, x, L)
            blocks = hit & (tx > F(0))
        else:
            hit, tn, tf, _ = capsule_interval(p, n, R, x, L, qL)
            blocks = hit & (tf > F(0))
        occ = np.where(blocks, F(1), occ)
    return occ


def draw(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, lt=None, shadow_ws=None,
         shadow_depth_0=None):
    """colliders_reference.draw's arguments; with `lt` (shadows_reference.light) and the two maps, the shadowed launch.  float32 throughout."""
    f = lambda v: np.asarray(np.asarray(v, np.float64), F)   # noqa: E731
    o, d, acc, s, d0 = (np.asarray(a, F) for a in (rays_o, rays_d, acc, weights_sum, depth_0))
    rgb = np.asarray(rgb, F)
    t_min, t_max, bg, checker, checker_dim, ambient = (F(v) for v in (t_min, t_max, bg, checker, checker_dim, ambient))
    N = o.shape[0]
    one, zero, inf = F(1), F(0), F(np.inf)
    q = cr._dot(d, d)
    t_hit = np.full(N, inf, F)
    k_hit = np.full(N, -1, np.int64)
    face_hit = np.zeros(N, np.int64)
    near = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for k, c in enumerate(colliders):
            if c is None or not (cr.PLANE <= c[0] <= CAPSULE):
                continue
            typ, g = c
            p, n, R = f(g[0:3]), f(g[3:6]), f(g[6])
            face = np.zeros(N, np.int64)
            if typ == CAPSULE and not capsule_frame(p, n)[2] > zero:
                typ = cr.SPHERE
            if typ == cr.PLANE:
                nd = cr._dot(n[None], d)
                t = cr._dot(n[None], p[None] - o) / nd
                ok = nd < zero
            elif typ == BOX:
                ok, te, tx, fe, fx, nr = box_interval(p, n, o, d)
                first = te > t_min
                near |= nr | (ok & _close(te, np.full(N, t_min, F)))
                t, face = np.where(first, te, tx), np.where(first, fe, fx)
            elif typ == CAPSULE:
                ok, tn, tf, nr = capsule_interval(p, n, R, o, d, q)
                near |= nr | (ok & _close(tn, np.full(N, t_min, F)))
                t = np.where(tn > t_min, tn, tf)
            else:
                oc = o - p[None]
                b = cr._dot(oc, d)
                disc = b * b - q * (cr._dot(oc, oc) - R * R)
                ok = disc > zero
                sq = np.sqrt(np.where(ok, disc, zero))
                t = (-b + sq) / q
                if typ == cr.SPHERE:
                    t_near = (-b - sq) / q
                    t = np.where(t_near > t_min, t_near, t)
            ok = ok & (t > t_min) & (t < t_max)
            t = np.where(ok, t, inf).astype(F)
            better = t < t_hit
            k_hit, face_hit, t_hit = np.where(better, k, k_hit), np.where(better, face, face_hit), np.where(better, t, t_hit)
        out, cov = acc.copy(), s.copy()
        front = np.zeros(N, bool)
        occ = np.zeros(N, F)
        t_obj = np.where(s > F(1e-4), d0 / np.where(s > zero, s, one), inf)
        for k, c in enumerate(colliders):
            m = k_hit == k
            if c is None or not m.any():
                continue
            typ, g = c
            p, n, R = f(g[0:3]), f(g[3:6]), f(g[6])
            if typ == CAPSULE and not capsule_frame(p, n)[2] > zero:
                typ = cr.SPHERE
            t = t_hit[m]
            dm = d[m]
            x = o[m] + t[:, None] * dm
            r = x - p[None]
            factor = np.full(t.shape, one, F)
            if typ == cr.PLANE:
                nd = cr._dot(n[None], dm)
                if checker > zero:
                    u, v = cr.tangent_frame(n)
                    cells = np.floor(cr._dot(u[None], r) / checker) + np.floor(cr._dot(v[None], r) / checker)
                    half = cells * F(0.5)
                    factor = np.where(half != np.floor(half), checker_dim, one).astype(F)
            elif typ == BOX:
                fc = face_hit[m]
                nd = np.where(fc == 0, dm[:, 0], np.where(fc == 1, dm[:, 1], dm[:, 2]))
                if checker > zero:
                    ra, rb = np.where(fc == 0, r[:, 1], r[:, 0]), np.where(fc == 2, r[:, 1], r[:, 2])
                    cells = np.floor(ra / checker) + np.floor(rb / checker)
                    half = cells * F(0.5)
                    factor = np.where(half != np.floor(half), checker_dim, one).astype(F)
            elif typ == CAPSULE:
                ax, _, ln = capsule_frame(p, n)
                hc = np.minimum(np.maximum(cr._dot(ax[None], r), zero), ln)
                nd = cr._dot((r - hc[:, None] * ax[None]) / R, dm)
            else:
                nd = cr._dot(r / R, dm)
            shade = ambient + (one - ambient) * (np.abs(nd) / np.sqrt(q[m]))
            col = rgb[k][None] * factor[:, None] * shade[:, None]
            if lt is not None:
                oc_, _, _, _, _ = sr.occlusion(lt, shadow_ws, shadow_depth_0, colliders, k, x, F)
                oc_ = np.maximum(oc_, _casters(lt, colliders, k, x))
                occ[m] = oc_
                col = col * (one - F(lt["strength"]) * oc_)[:, None]
            a = np.minimum(np.maximum((t_max - t) / (F(0.5) * t_max), zero), one)
            sm, am = s[m], acc[m]
            fr = t < t_obj[m]
            w = (one - sm) * a
            out[m] = np.where(fr[:, None], a[:, None] * col + (one - a)[:, None] * am, am + w[:, None] * col)
            cov[m] = np.where(fr, a + (one - a) * sm, sm + w)
            front[m] = fr
        image = out + ((one - cov) * bg)[:, None]
    assert image.dtype == F and cov.dtype == F and t_hit.dtype == F and occ.dtype == F
    return Drawn(image, cov, t_hit, k_hit, face_hit, front, near, occ)


# ------------------------------------------------------------------------------------------------ the tests' scenes
T_MIN, T_MAX = 0.2, 12.0
DRAW_BOX = (BOX, np.array([0.35, -0.3, 0.1, 0.4, 0.25, 0.3, 0.0, 0.0, 0.0, 0.0]))
DRAW_CAPSULE = (CAPSULE, np.array([-0.9, -0.2, 0.3, 0.5, 0.7, -0.4, 0.22, 0.0, 0.0, 0.0]))


def mixed_scene():
    """A plane, a sphere, an empty slot, a box and a capsule."""
    return cr.slots(cr.plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0)), cr.sphere((0.0, 0.45, -0.5), 0.35), None, DRAW_BOX, DRAW_CAPSULE)


EYES = {"outside": (0.25, 0.5, 2.0), "inside_box": (0.45, -0.25, 0.15), "inside_capsule": (-0.62, 0.15, 0.08)}


def hand_rays():
    """Host test 4's rays against UNIT_BOX / UNIT_CAPSULE, as (name, o, d): exact cases of the law."""
    return [("axial onto a face", (0.25, 0.1, 3.0), (0.0, 0.0, -1.0)),
            ("from inside: the far face", (0.25, 0.1, 0.0), (0.0, 0.0, -1.0)),
            ("parallel to a slab, inside it", (0.25, 0.25, 3.0), (0.0, 0.0, -2.0)),
            ("parallel to a slab, outside it", (0.25, 0.75, 3.0), (0.0, 0.0, -2.0)),
            ("grazing an edge", (2.0, 0.0, 0.0), (-1.0, 0.0, 1.0)),
            ("along the capsule's axis onto the cap", (-3.0, 2.0, 0.0), (1.0, 0.0, 0.0)),
            ("onto the cylinder's middle", (0.0, 2.0, 3.0), (0.0, 0.0, -1.0)),
            ("eye inside the capsule", (0.25, 2.0, 0.0), (0.0, 0.0, -1.0))]


UNIT_BOX = (BOX, np.array([0.0, 0.0, 0.0, 1.0, 0.5, 1.0, 0.0, 0.0, 0.0, 0.0]))                 # |x| <= 1, |y| <= 0.5, |z| <= 1
UNIT_CAPSULE = (CAPSULE, np.array([-1.0, 2.0, 0.0, 2.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0]))       # from (-1, 2, 0) to (1, 2, 0), R = 0.5
