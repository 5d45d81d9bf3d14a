"""numpy restatement of the collider overlay's law (include/pienerf_hip.h: pn_draw_colliders; csrc/pn_colliders.hip), parameterised by dtype.

`draw(...)` evaluates the law for every ray in float32 (one rounding per operation, in the kernel's order) or float64 (the same expressions on the same
fp32 inputs, the truth the tests' bars are measured against) and returns a `Drawn` with the image, the coverage, t, the decisions it took (hit slot,
checker parity, in front of / behind the object) and a per-ray flag `near`: the ray lies so close to one of the law's decisions that two correct
evaluations may take it differently.  The thresholds below are chosen so that the float32 and float64 evaluations agree on every decision of every
unflagged ray (tests/test_colliders_host.py checks that on the GPU tests' scenes) while flagging well under 0.5 % of the rays.
"""
from collections import namedtuple

import numpy as np

EMPTY, PLANE, SPHERE, CONTAINER = 0, 1, 2, 3
SLOTS = 8

# near a decision (all relative to the natural size of the quantity):
NEAR_DISC = 1e-4      # |disc| against b^2 + q |oc.oc - R^2|: a ray grazing a sphere
NEAR_ND = 1e-4        # |n.d| against |d|: a ray grazing a plane
NEAR_CELL = 1e-3      # a checker coordinate against the nearest integer, in cells
NEAR_T = 1e-4         # |t - t_obj|, t - t_min, t_max - t, the two roots' choice, two slots' t: against max(|t|, 1)

Drawn = namedtuple("Drawn", "image coverage t slot parity front near")


def plane(point, normal):
    n = np.asarray(normal, np.float64)
    g = np.zeros(10)
    g[0:3], g[3:6] = point, n / np.linalg.norm(n)
    return PLANE, g


def sphere(centre, radius, inside=False):
    g = np.zeros(10)
    g[0:3], g[6] = centre, radius
    return (CONTAINER if inside else SPHERE), g


def slots(*colliders):
    """Eight slots from the colliders given, in order; None leaves a gap."""
    out = list(colliders) + [None] * (SLOTS - len(colliders))
    assert len(out) == SLOTS
    return out


def default_rgb():
    return np.stack([np.array([0.9, 0.6, 0.3]) * (1.0 - 0.08 * k) + 0.01 * k for k in range(SLOTS)]).astype(np.float32)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def tangent_frame(n):
    """u = normalised n x e, e the coordinate axis on which |n| is smallest (lowest index on ties); v = n x u.  In n's dtype."""
    dt = n.dtype.type
    a = np.abs(n)
    if a[0] <= a[1] and a[0] <= a[2]:
        u = np.array([dt(0), n[2], -n[1]], dt)
    elif a[1] <= a[2]:
        u = np.array([-n[2], dt(0), n[0]], dt)
    else:
        u = np.array([n[1], -n[0], dt(0)], dt)
    L = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    u = (u / L).astype(dt)
    v = np.array([n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]], dt)
    return u, v


def draw(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, dtype=np.float32):
    """colliders: SLOTS entries, None or (type, geom10 = (p[3], n[3], R, v[3])) as Simulator keeps them; rgb [SLOTS, 3]; rays_o, rays_d, acc [N, 3],
    weights_sum, depth_0 [N] (fp32 data).  Every scalar and every collider field is rounded to fp32 first, as the kernel gets them."""
    dt = np.dtype(dtype).type
    f = lambda v: np.asarray(np.asarray(v, np.float32), dtype)   # noqa: E731 — fp32 data, lifted to the evaluation's dtype
    o, d, acc, s, d0 = f(rays_o), f(rays_d), f(acc), f(weights_sum), f(depth_0)
    rgb = f(rgb)
    t_min, t_max, bg, checker, checker_dim, ambient = (dt(np.float32(v)) for v in (t_min, t_max, bg, checker, checker_dim, ambient))
    N = o.shape[0]
    one, zero, inf = dt(1), dt(0), dt(np.inf)
    q = _dot(d, d)
    t_hit = np.full(N, inf, dtype)
    t_second = np.full(N, inf, dtype)   # the best t among the slots that lost: how close the choice of the slot was
    k_hit = np.full(N, -1, np.int64)
    near = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for k, c in enumerate(colliders):
            if c is None or not (PLANE <= c[0] <= CONTAINER):
                continue
            typ, g = c
            p, n, R = f(g[0:3]), f(g[3:6]), f(g[6])
            if typ == PLANE:
                nd = _dot(n[None], d)
                near |= np.abs(nd) < dt(NEAR_ND) * np.sqrt(q)
                t = _dot(n[None], p[None] - o) / nd
                ok = nd < zero
            else:
                oc = o - p[None]
                b = _dot(oc, d)
                cc = _dot(oc, oc) - R * R
                disc = b * b - q * cc
                near |= np.abs(disc) < dt(NEAR_DISC) * (b * b + q * np.abs(cc))
                ok = disc > zero
                sq = np.sqrt(np.where(ok, disc, zero))
                t = (-b + sq) / q
                if typ == SPHERE:
                    t_near = (-b - sq) / q
                    near |= ok & (np.abs(t_near - t_min) < dt(NEAR_T) * np.maximum(np.abs(t_near), one))
                    t = np.where(t_near > t_min, t_near, t)
            near |= ok & (np.abs(t - t_min) < dt(NEAR_T) * np.maximum(np.abs(t), one))
            near |= ok & (np.abs(t_max - t) < dt(NEAR_T) * np.maximum(np.abs(t), one))
            ok &= (t > t_min) & (t < t_max)
            t = np.where(ok, t, inf)
            better = t < t_hit
            t_second = np.where(better, t_hit, np.minimum(t_second, t))
            k_hit = np.where(better, k, k_hit)
            t_hit = np.where(better, t, t_hit)
        hit = k_hit >= 0
        near |= hit & np.isfinite(t_second) & (np.abs(t_second - t_hit) < dt(NEAR_T) * np.maximum(np.abs(t_hit), one))
        out, cov = acc.copy(), s.copy()
        parity = np.zeros(N, np.int64)
        front = np.zeros(N, bool)
        t_obj = np.where(s > dt(np.float32(1e-4)), d0 / np.where(s > zero, s, one), inf)
        for k, c in enumerate(colliders):
            m = k_hit == k
            if c is None or not m.any():
                continue
            typ, g = c
            p, n, R = f(g[0:3]), f(g[3:6]), f(g[6])
            t = t_hit[m]
            x = o[m] + t[:, None] * d[m]
            r = x - p[None]
            factor = np.full(t.shape, one, dtype)
            if typ == PLANE:
                nd = _dot(n[None], d[m])
                if checker > zero:
                    u, v = tangent_frame(n)
                    cu, cv = _dot(u[None], r) / checker, _dot(v[None], r) / checker
                    cells = np.floor(cu) + np.floor(cv)
                    half = cells * dt(0.5)
                    odd = half != np.floor(half)
                    factor = np.where(odd, checker_dim, one).astype(dtype)
                    parity[m] = odd
                    nm = (np.abs(cu - np.round(cu)) < dt(NEAR_CELL)) | (np.abs(cv - np.round(cv)) < dt(NEAR_CELL))
                    near[m] |= nm
            else:
                nd = _dot(r / R, d[m])
            shade = ambient + (one - ambient) * (np.abs(nd) / np.sqrt(q[m]))
            col = rgb[k][None] * factor[:, None] * shade[:, None]
            a = np.minimum(np.maximum((t_max - t) / (dt(0.5) * t_max), zero), one)
            sm, am = s[m], acc[m]
            fr = t < t_obj[m]
            near[m] |= np.isfinite(t_obj[m]) & (np.abs(t - t_obj[m]) < dt(NEAR_T) * np.maximum(np.abs(t), one))
            o_front = a[:, None] * col + (one - a)[:, None] * am
            c_front = a + (one - a) * sm
            w = (one - sm) * a
            o_back = am + w[:, None] * col
            c_back = sm + w
            out[m] = np.where(fr[:, None], o_front, o_back)
            cov[m] = np.where(fr, c_front, c_back)
            front[m] = fr
        image = out + ((one - cov) * bg)[:, None]
    return Drawn(image.astype(dtype), cov.astype(dtype), t_hit, k_hit, parity, front, near)


def bars(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc):
    """Both evaluations, the mask of rays to compare (unflagged in either) and the bar per output: 4 x the largest float32-versus-float64 difference on
    those rays (relative to max(|t|, 1) for t).  The factor 4 leaves room for a different but equally valid rounding order."""
    args = (colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc)
    r32, r64 = draw(*args, dtype=np.float32), draw(*args, dtype=np.float64)
    keep = ~(r32.near | r64.near)
    hit = keep & (r64.slot >= 0)
    diff = {"image": float(np.abs(r32.image[keep].astype(np.float64) - r64.image[keep]).max()) if keep.any() else 0.0,
            "coverage": float(np.abs(r32.coverage[keep].astype(np.float64) - r64.coverage[keep]).max()) if keep.any() else 0.0,
            "t": float(np.abs(r32.t[hit].astype(np.float64) - r64.t[hit]).max()) if hit.any() else 0.0}
    return r32, r64, keep, {k: 4.0 * v for k, v in diff.items()}, diff


def get_rays_numpy(eye, W, H, fx):
    """Pinhole rays through the pixel centres from `eye` looking at the origin, y up: ([N, 3] origins, [N, 3] unit directions), fp32."""
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = (i.reshape(-1) + 0.5 - 0.5 * W) / fx
    y = -(j.reshape(-1) + 0.5 - 0.5 * H) / fx
    d = fwd[None] + x[:, None] * right[None] + y[:, None] * up[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(eye, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def standard_inputs(N, seed=0):
    """acc, s, depth_0 of the GPU tests: random acc and s with a fifth of the rays at s = 0 and a fifth at s = 1; depth_0 = s U(2, 4.5)."""
    g = np.random.default_rng(seed)
    acc = g.uniform(0.0, 1.0, (N, 3)).astype(np.float32)
    s = g.uniform(0.0, 1.0, N).astype(np.float32)
    kind = g.integers(0, 5, N)
    s[kind == 0] = 0.0
    s[kind == 1] = 1.0
    acc *= s[:, None]
    d0 = (s * g.uniform(2.0, 4.5, N).astype(np.float32)).astype(np.float32)
    return acc, s, d0


STANDARD = dict(eye=(0.3, 0.6, 3.2), W=64, H=48, t_min=0.2, t_max=12.0, checker=0.25, checker_dim=0.5, ambient=0.3, bg=1.0)


def standard_scene():
    """The GPU tests' standard scene: floor y = -0.95 with checker 0.25, solid sphere (0, 0, 0.9) R 0.5, container R 1.6."""
    return slots(plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0)), sphere((0.0, 0.0, 0.9), 0.5), sphere((0.0, 0.0, 0.0), 1.6, inside=True))
