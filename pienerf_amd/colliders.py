"""The contact colliders drawn into a rendered frame (csrc/pn_colliders.hip; include/pienerf_hip.h: pn_draw_colliders has the law).

``collider_style`` builds the launch's by-value style; ``draw_colliders_torch`` restates the law in torch ops on the device, the baseline
tools/time_colliders.py times the HIP launch against (the tests compare the launch with tests/colliders_reference.py's numpy instead).

``shadow_light`` builds the directional light of the shadowed launch (pn_draw_colliders_shadowed) and ``shadow_rays`` the parallel rays its
opacity map is rendered along (NeRFRenderer.set_collider_shadows).  The renderer's side — the overlay's state, the shadow pass, the launch — is
nerf/overlay_colliders.py.
"""
import math

import torch

from ._lib import ColliderStyle, ShadowLight

SLOTS = 8
PLANE, SPHERE, CONTAINER = 1, 2, 3
BOX, CAPSULE = 4, 5
PLANE_GREY, OTHER_GREY = 0.8, 0.5   # the default colours: a light grey for a plane's slot, a mid grey for every other


def collider_style(rgb=None, types=None, checker=0.0, checker_dim=0.6, ambient=0.35):
    """A ColliderStyle (pn_collider_style).  `rgb`: colours in slot order, fewer than 8 leave the rest at their defaults — PLANE_GREY for a slot that
    `types` (8 collider types, 0 = empty; e.g. from Simulator.collider_types()) says holds a plane, OTHER_GREY otherwise.  `checker`: cell size of a
    plane's checker pattern in world units (<= 0: none), `checker_dim` the factor of its odd cells; `ambient` in [0, 1].  ValueError for a non-finite
    value, more than 8 colours or ambient outside [0, 1]."""
    st = ColliderStyle()
    types = list(types) if types is not None else [0] * SLOTS
    rgb = [tuple(float(v) for v in c) for c in (rgb or [])]
    if len(types) != SLOTS or len(rgb) > SLOTS or any(len(c) != 3 for c in rgb):
        raise ValueError(f"collider_style: at most {SLOTS} colours of 3 components and {SLOTS} types")
    for k in range(SLOTS):
        g = PLANE_GREY if types[k] == PLANE else OTHER_GREY
        c = rgb[k] if k < len(rgb) else (g, g, g)
        for j in range(3):
            st.rgb[k][j] = c[j]
    st.checker, st.checker_dim, st.ambient = float(checker), float(checker_dim), float(ambient)
    vals = [st.rgb[k][j] for k in range(SLOTS) for j in range(3)] + [st.checker, st.checker_dim, st.ambient]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("collider_style: every value must be finite")
    if not 0.0 <= st.ambient <= 1.0:
        raise ValueError(f"collider_style: ambient must be in [0, 1], got {ambient!r}")
    return st


def _light_frame(L):
    """U = normalised L x e, e the coordinate axis on which |L| is smallest (lowest index on ties), V = L x U: the checker's rule, in Python floats."""
    a = [abs(v) for v in L]
    if a[0] <= a[1] and a[0] <= a[2]:
        u = [0.0, L[2], -L[1]]
    elif a[1] <= a[2]:
        u = [-L[2], 0.0, L[0]]
    else:
        u = [L[1], -L[0], 0.0]
    n = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    u = [v / n for v in u]
    return u, [L[1] * u[2] - L[2] * u[1], L[2] * u[0] - L[0] * u[2], L[0] * u[1] - L[1] * u[0]]


def shadow_light(direction=(0.4, 1.0, 0.3), strength=0.6, resolution=256, bound=1.0, min_near=0.2, centre=(0, 0, 0), extent=None, bias=None, spheres=True):
    """A ShadowLight (pn_shadow_light), built in fp64 and rounded once.  `direction` points from the scene towards the light (any length); the map of
    `resolution`^2 texels is centred on `centre` and spans +-`extent` (None: sqrt(3) `bound`, which covers the box [-bound, bound]^3 from every direction);
    the light rays start half + 2 `min_near` from the centre, so each enters the box beyond min_near; `bias` (None: 1.5 texels) keeps a receiver from
    shadowing itself; `spheres`: solid sphere, box and capsule colliders cast analytic shadows.  ValueError for a zero or non-finite direction, strength outside [0, 1],
    resolution outside 2 .. 4096, a non-positive extent or a negative bias."""
    d = [float(v) for v in direction]
    c = [float(v) for v in centre]
    n = math.sqrt(sum(v * v for v in d)) if len(d) == 3 and all(math.isfinite(v) for v in d) else 0.0
    if not (math.isfinite(n) and n > 0.0):
        raise ValueError(f"shadow_light: direction must be three finite numbers, not all zero, got {direction!r}")
    if len(c) != 3 or not all(math.isfinite(v) for v in c):
        raise ValueError(f"shadow_light: centre must be three finite numbers, got {centre!r}")
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"shadow_light: strength must be in [0, 1], got {strength!r}")
    S = int(resolution)
    if S != resolution or not 2 <= S <= 4096:
        raise ValueError(f"shadow_light: resolution must be an integer in 2 .. 4096, got {resolution!r}")
    half = math.sqrt(3.0) * float(bound) if extent is None else float(extent)
    if not (math.isfinite(half) and half > 0.0):
        raise ValueError(f"shadow_light: the extent must be a positive finite number, got {half!r}")
    bias = 1.5 * 2.0 * half / S if bias is None else float(bias)
    if not (math.isfinite(bias) and bias >= 0.0):
        raise ValueError(f"shadow_light: bias must be a finite number >= 0, got {bias!r}")
    min_near = float(min_near)
    if not math.isfinite(min_near):
        raise ValueError(f"shadow_light: min_near must be finite, got {min_near!r}")
    L = [v / n for v in d]
    U, V = _light_frame(L)
    lt = ShadowLight()
    for j in range(3):
        lt.c[j], lt.L[j], lt.U[j], lt.V[j] = c[j], L[j], U[j], V[j]
    lt.half, lt.D, lt.S, lt.strength, lt.bias, lt.spheres = half, half + 2.0 * min_near, S, strength, bias, int(bool(spheres))
    return lt


def shadow_rays(light, device):
    """The light's parallel rays, (rays_o, rays_d) [S^2, 3] fp32 on `device`: texel (i, j) at index j S + i starts at
    c + D L + ((i + 1/2) 2 / S - 1) half U + ((j + 1/2) 2 / S - 1) half V and runs along -L.  Built in fp64 from the light's fp32 members, rounded once."""
    S = int(light.S)
    vec = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float64)   # noqa: E731
    c, L, U, V = vec(light.c), vec(light.L), vec(light.U), vec(light.V)
    g = ((torch.arange(S, dtype=torch.float64) + 0.5) * 2.0 / S - 1.0) * float(light.half)
    o = (c + float(light.D) * L).view(1, 1, 3) + g.view(1, S, 1) * U.view(1, 1, 3) + g.view(S, 1, 1) * V.view(1, 1, 3)   # [j, i, 3]
    rays_o = o.reshape(S * S, 3).to(torch.float32)
    rays_d = (-L).to(torch.float32).view(1, 3).expand(S * S, 3)
    return rays_o.contiguous().to(device), rays_d.contiguous().to(device)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _sphere_roots(o, d, q, c, R):
    oc = o - c
    b = _dot(oc, d)
    disc = b * b - q * (_dot(oc, oc) - R * R)
    sq = torch.sqrt(disc.clamp(min=0))
    return disc > 0, (-b - sq) / q, (-b + sq) / q


def _box_interval(o, d, p, h):
    """(hit, t_enter, t_exit, face of t_enter, face of t_exit) of the slab test; the lowest axis wins a tie."""
    inf = float("inf")
    zero = d == 0
    dd = torch.where(zero, torch.ones_like(d), d)
    t1, t2 = ((p - h) - o) / dd, ((p + h) - o) / dd
    lo = torch.where(zero, torch.full_like(d, -inf), torch.minimum(t1, t2))
    hi = torch.where(zero, torch.full_like(d, inf), torch.maximum(t1, t2))
    inside = (~zero | ((o - p).abs() < h)).all(dim=-1)
    te, fe = lo.max(dim=-1)
    tx, fx = hi.min(dim=-1)
    fe = (lo == te.unsqueeze(-1)).to(torch.int64).argmax(dim=-1)   # the first axis that reaches the extremum
    fx = (hi == tx.unsqueeze(-1)).to(torch.int64).argmax(dim=-1)
    return inside & (te < tx), te, tx, fe, fx


def _capsule_interval(o, d, q, A, n, R):
    """(hit, t_near, t_far): the convex union of the end spheres and the finite cylinder."""
    inf = float("inf")
    length = float(n.norm())
    ax = n / length
    okA, nA, fA = _sphere_roots(o, d, q, A, R)
    okB, nB, fB = _sphere_roots(o, d, q, A + n, R)
    tn = torch.where(okA, nA, torch.full_like(q, inf))
    tf = torch.where(okA, fA, torch.full_like(q, -inf))
    tn = torch.where(okB, torch.minimum(tn, nB), tn)
    tf = torch.where(okB, torch.maximum(tf, fB), tf)
    oc = o - A
    ad, ao = _dot(ax, d), _dot(ax, oc)
    dp, op = d - ad.unsqueeze(-1) * ax, oc - ao.unsqueeze(-1) * ax
    A2, b = _dot(dp, dp), _dot(op, dp)
    disc = b * b - A2 * (_dot(op, op) - R * R)
    okC = (A2 > 0) & (disc > 0)
    sq = torch.sqrt(disc.clamp(min=0))
    A2s = torch.where(A2 > 0, A2, torch.ones_like(A2))
    lo, hi = (-b - sq) / A2s, (-b + sq) / A2s
    par = ad == 0
    ads = torch.where(par, torch.ones_like(ad), ad)
    s1, s2 = (0 - ao) / ads, (length - ao) / ads
    lo = torch.where(par, lo, torch.maximum(lo, torch.minimum(s1, s2)))
    hi = torch.where(par, hi, torch.minimum(hi, torch.maximum(s1, s2)))
    okC = okC & (~par | ((ao > 0) & (ao < length))) & (lo < hi)
    tn = torch.where(okC, torch.minimum(tn, lo), tn)
    tf = torch.where(okC, torch.maximum(tf, hi), tf)
    return okA | okB | okC, tn, tf


@torch.no_grad()
def draw_colliders_torch(colliders, style, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, image):
    """The law in torch ops, fp32, on the device of the rays: (image, coverage, collider_t), nothing in place.  `colliders`: 8 entries, None or
    (type, geom10) as Simulator keeps them on the host."""
    o, d, s, acc = rays_o, rays_d, weights_sum, image
    dev, inf = o.device, float("inf")
    vec = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float32, device=dev)   # noqa: E731
    q = _dot(d, d)
    t_hit = torch.full_like(s, inf)
    k_hit = torch.full(s.shape, -1, dtype=torch.int64, device=dev)
    face_hit = torch.zeros_like(k_hit)
    for k, c in enumerate(colliders):
        if c is None:
            continue
        typ, g = c
        p, n, R = vec(g[0:3]), vec(g[3:6]), float(g[6])
        if typ == PLANE:
            nd = _dot(n, d)
            t = _dot(n, p - o) / nd
            ok = nd < 0
        elif typ == BOX:
            ok, te, tx, fe, fx = _box_interval(o, d, p, n)
            first = te > t_min
            t = torch.where(first, te, tx)
            face_hit = torch.where(ok & (t > t_min) & (t < t_max) & (t < t_hit), torch.where(first, fe, fx), face_hit)
        elif typ == CAPSULE:
            ok, tn, tf = _capsule_interval(o, d, q, p, n, R)
            t = torch.where(tn > t_min, tn, tf)
        else:
            oc = o - p
            b = _dot(oc, d)
            disc = b * b - q * (_dot(oc, oc) - R * R)
            ok = disc > 0
            sq = torch.sqrt(disc.clamp(min=0))
            t = (-b + sq) / q
            if typ == SPHERE:
                t_near = (-b - sq) / q
                t = torch.where(t_near > t_min, t_near, t)
        ok = ok & (t > t_min) & (t < t_max)
        t = torch.where(ok, t, torch.full_like(t, inf))
        better = t < t_hit
        k_hit = torch.where(better, torch.full_like(k_hit, k), k_hit)
        t_hit = torch.where(better, t, t_hit)
    out, cov = acc.clone(), s.clone()
    t_obj = torch.where(s > 1e-4, depth_0 / s.clamp(min=1e-30), torch.full_like(s, inf))
    dn = torch.sqrt(q)
    for k, c in enumerate(colliders):
        if c is None:
            continue
        typ, g = c
        p, n, R = vec(g[0:3]), vec(g[3:6]), float(g[6])
        m = k_hit == k
        t = torch.where(m, t_hit, torch.zeros_like(t_hit))
        r = o + t.unsqueeze(-1) * d - p
        factor = torch.ones_like(t)
        if typ == PLANE:
            nd = _dot(n, d)
            if style.checker > 0:
                a = [abs(float(v)) for v in n]
                e = 0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if a[1] <= a[2] else 2)
                u = torch.linalg.cross(n, torch.eye(3, device=dev)[e])
                u = u / u.norm()
                v = torch.linalg.cross(n, u)
                cells = torch.floor(_dot(u, r) / style.checker) + torch.floor(_dot(v, r) / style.checker)
                factor = torch.where(torch.remainder(cells, 2) != 0, torch.full_like(t, style.checker_dim), factor)
        elif typ == BOX:
            nd = torch.gather(d, 1, face_hit.unsqueeze(-1)).squeeze(-1)
            if style.checker > 0:
                ra = torch.where(face_hit == 0, r[..., 1], r[..., 0])
                rb = torch.where(face_hit == 2, r[..., 1], r[..., 2])
                cells = torch.floor(ra / style.checker) + torch.floor(rb / style.checker)
                factor = torch.where(torch.remainder(cells, 2) != 0, torch.full_like(t, style.checker_dim), factor)
        elif typ == CAPSULE:
            length = float(n.norm())
            ax = n / length
            hc = _dot(ax, r).clamp(0, length)
            nd = _dot((r - hc.unsqueeze(-1) * ax) / R, d)
        else:
            nd = _dot(r / R, d)
        shade = style.ambient + (1 - style.ambient) * (nd.abs() / dn)
        col = vec(style.rgb[k]) * (factor * shade).unsqueeze(-1)
        a = ((t_max - t) / (0.5 * t_max)).clamp(0, 1)
        front = t < t_obj
        w = (1 - s) * a
        o_k = torch.where(front.unsqueeze(-1), a.unsqueeze(-1) * col + (1 - a).unsqueeze(-1) * acc, acc + w.unsqueeze(-1) * col)
        c_k = torch.where(front, a + (1 - a) * s, s + w)
        out = torch.where(m.unsqueeze(-1), o_k, out)
        cov = torch.where(m, c_k, cov)
    return out + ((1 - cov) * bg).unsqueeze(-1), cov, t_hit
