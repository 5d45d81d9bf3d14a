"""numpy restatement of the shadowed collider overlay's law (include/pienerf_hip.h: pn_draw_colliders_shadowed; csrc/pn_colliders.hip), parameterised by
dtype and built on colliders_reference.draw: the hit search, its decisions and its flags are that function's; the hit point, the slot's colour, the
occlusion and the composite are evaluated here, operation for operation as the kernel does, in float32 (one rounding per operation) or float64 (the same
expressions on the same fp32 inputs).

`draw` returns a `Shadowed`; its flag `near` adds to colliders_reference's the rays that lie close to one of the NEW decisions:
  - fu or fv within NEAR_TEXEL of an integer (which four texels are read), where the footprint can touch the map;
  - |t_r - (t_o + bias)| below NEAR_T max(|t_r|, 1) on an in-map texel with s_m > 0 (lit or shadowed);
  - a caster's |disc| below NEAR_DISC (b^2 + |oc.oc - R^2|) (the light ray grazes a sphere);
  - a caster's far root within NEAR_ROOT of 0.
"""
from collections import namedtuple

import numpy as np

import colliders_reference as cr

NEAR_TEXEL = 1e-3
NEAR_T = 1e-4
NEAR_DISC = 1e-4
NEAR_ROOT = 1e-4

Shadowed = namedtuple("Shadowed", "image coverage t slot parity front near occ occ_map occ_sph")

LIGHTS = {"oblique": (0.4, 1.0, 0.3), "axis": (0.0, 1.0, 0.0), "low": (-0.7, 0.5, 0.2)}   # the GPU cases' lights


def light(direction=(0.4, 1.0, 0.3), strength=0.6, resolution=256, bound=1.0, min_near=0.2, centre=(0, 0, 0), extent=None, bias=None, spheres=True):
    """The light as pn_shadow_light holds it: a dict of float32 members (S and spheres ints), built in float64 and rounded once."""
    L = np.asarray(direction, np.float64)
    L = L / np.sqrt(L[0] * L[0] + L[1] * L[1] + L[2] * L[2])
    U, V = cr.tangent_frame(L)
    half = np.sqrt(3.0) * bound if extent is None else float(extent)
    S = int(resolution)
    f = np.float32
    return dict(c=np.asarray(centre, np.float64).astype(f), L=L.astype(f), U=U.astype(f), V=V.astype(f), half=f(half), D=f(half + 2.0 * min_near), S=S,
                strength=f(strength), bias=f(1.5 * 2.0 * half / S if bias is None else bias), spheres=int(bool(spheres)))


def light_rays(lt):
    """Origins and directions of the light's rays [S^2, 3] in float64, from the light's float32 members: texel (i, j) at index j S + i."""
    S = lt["S"]
    c, L, U, V = (lt[k].astype(np.float64) for k in "cLUV")
    g = ((np.arange(S) + 0.5) * 2.0 / S - 1.0) * float(lt["half"])
    o = (c + float(lt["D"]) * L)[None, None] + g[None, :, None] * U[None, None] + g[:, None, None] * V[None, None]
    return o.reshape(S * S, 3), np.broadcast_to(-L, (S * S, 3)).copy()


def synthetic_maps(S, seed=0):
    """The GPU launch tests' maps: s_m uniform in [0, 1] with a third of the texels at 0, t_o uniform in [1.5, 4]; (shadow_ws, shadow_depth_0 = s_m t_o)."""
    g = np.random.default_rng(1000 + seed)
    sm = g.uniform(0.0, 1.0, S * S).astype(np.float32)
    sm[g.integers(0, 3, S * S) == 0] = 0.0
    to = g.uniform(1.5, 4.0, S * S).astype(np.float32)
    return sm, (sm * to).astype(np.float32)


def occlusion(lt, shadow_ws, shadow_depth_0, colliders, k_hit, x, dtype=np.float32):
    """The law's occ for the hit points x [M, 3] (in `dtype`) of slot k_hit: (occ, occ_map, occ_sph, near, weights [M, 4])."""
    dt = np.dtype(dtype).type
    f = lambda v: np.asarray(np.asarray(v, np.float32), dtype)   # noqa: E731
    one, zero, inf = dt(1), dt(0), dt(np.inf)
    c, L, U, V = f(lt["c"]), f(lt["L"]), f(lt["U"]), f(lt["V"])
    half, D, bias = dt(np.float32(lt["half"])), dt(np.float32(lt["D"])), dt(np.float32(lt["bias"]))
    S = int(lt["S"])
    ws, d0 = f(shadow_ws), f(shadow_depth_0)
    M = x.shape[0]
    near = np.zeros(M, bool)
    with np.errstate(all="ignore"):
        r = x - c[None]
        u, v, w = cr._dot(U[None], r), cr._dot(V[None], r), cr._dot(L[None], r)
        t_r = D - w
        Sf = dt(S)
        scale = Sf / (dt(2) * half)
        fu, fv = (u + half) * scale - dt(0.5), (v + half) * scale - dt(0.5)
        i0, j0 = np.floor(fu), np.floor(fv)
        au, av = fu - i0, fv - j0
        touches = (i0 >= -2) & (i0 <= S) & (j0 >= -2) & (j0 <= S)   # the footprint, moved by one texel either way, can reach the map
        near |= touches & ((np.abs(fu - np.round(fu)) < dt(NEAR_TEXEL)) | (np.abs(fv - np.round(fv)) < dt(NEAR_TEXEL)))
        total = np.zeros(M, dtype)
        weights = np.zeros((M, 4), dtype)
        for n, (di, dj) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            fi, fj = i0 + dt(di), j0 + dt(dj)
            inside = (fi >= zero) & (fi < Sf) & (fj >= zero) & (fj < Sf)
            idx = np.where(inside, fj * Sf + fi, zero).astype(np.int64)
            sm = ws[idx]
            t_o = np.where(sm > dt(np.float32(1e-4)), d0[idx] / np.where(sm > zero, sm, one), inf)
            edge = t_o + bias
            wgt = (au if di else one - au) * (av if dj else one - av)
            weights[:, n] = wgt
            total = total + np.where(inside & (t_r > edge), wgt * sm, zero)
            near |= inside & (sm > zero) & np.isfinite(edge) & (np.abs(t_r - edge) < dt(NEAR_T) * np.maximum(np.abs(t_r), one))
        occ_map = np.minimum(np.maximum(total, zero), one)
        occ_sph = np.zeros(M, dtype)
        if lt["spheres"]:
            for k2, c2 in enumerate(colliders):
                if c2 is None or k2 == k_hit or c2[0] != cr.SPHERE:
                    continue
                p2, R = f(c2[1][0:3]), f(c2[1][6])
                oc = x - p2[None]
                b = cr._dot(oc, L[None])
                cc = cr._dot(oc, oc) - R * R
                disc = b * b - cc
                root = -b + np.sqrt(np.where(disc > zero, disc, zero))
                blocks = (disc > zero) & (root > zero)
                near |= np.abs(disc) < dt(NEAR_DISC) * (b * b + np.abs(cc))
                near |= (disc > zero) & (np.abs(root) < dt(NEAR_ROOT))
                occ_sph = np.where(blocks, one, occ_sph)
        occ = np.maximum(occ_map, occ_sph)
    return occ, occ_map, occ_sph, near, weights


def draw(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, lt, shadow_ws, shadow_depth_0,
         dtype=np.float32):
    """colliders_reference.draw's arguments plus the light (`light(...)`) and the two maps [S^2] (fp32 data)."""
    base = cr.draw(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, dtype=dtype)
    dt = np.dtype(dtype).type
    f = lambda v: np.asarray(np.asarray(v, np.float32), dtype)   # noqa: E731
    o, d, acc, s, d0 = f(rays_o), f(rays_d), f(acc), f(weights_sum), f(depth_0)
    rgb = f(rgb)
    t_max, bg, checker, checker_dim, ambient = (dt(np.float32(v)) for v in (t_max, bg, checker, checker_dim, ambient))
    strength = dt(np.float32(lt["strength"]))
    N = o.shape[0]
    one, zero, inf = dt(1), dt(0), dt(np.inf)
    q = cr._dot(d, d)
    out, cov = acc.copy(), s.copy()
    near = base.near.copy()
    occ, occ_map, occ_sph = np.zeros(N, dtype), np.zeros(N, dtype), np.zeros(N, dtype)
    with np.errstate(all="ignore"):
        t_obj = np.where(s > dt(np.float32(1e-4)), d0 / np.where(s > zero, s, one), inf)
        for k, c in enumerate(colliders):
            m = base.slot == k
            if c is None or not m.any():
                continue
            typ, g = c
            p, n, R = f(g[0:3]), f(g[3:6]), f(g[6])
            t = base.t[m]
            x = o[m] + t[:, None] * d[m]
            r = x - p[None]
            factor = np.full(t.shape, one, dtype)
            if typ == cr.PLANE:
                nd = cr._dot(n[None], d[m])
                if checker > zero:
                    factor = np.where(base.parity[m] != 0, checker_dim, one).astype(dtype)
            else:
                nd = cr._dot(r / R, d[m])
            shade = ambient + (one - ambient) * (np.abs(nd) / np.sqrt(q[m]))
            col = rgb[k][None] * factor[:, None] * shade[:, None]
            oc, om, os_, nr, _ = occlusion(lt, shadow_ws, shadow_depth_0, colliders, k, x, dtype)
            occ[m], occ_map[m], occ_sph[m] = oc, om, os_
            near[m] |= nr
            lit = one - strength * oc
            col = col * lit[:, None]
            a = np.minimum(np.maximum((t_max - t) / (dt(0.5) * t_max), zero), one)
            sm, am = s[m], acc[m]
            fr = t < t_obj[m]
            o_front = a[:, None] * col + (one - a)[:, None] * am
            c_front = a + (one - a) * sm
            w = (one - sm) * a
            o_back = am + w[:, None] * col
            c_back = sm + w
            out[m] = np.where(fr[:, None], o_front, o_back)
            cov[m] = np.where(fr, c_front, c_back)
        image = out + ((one - cov) * bg)[:, None]
    return Shadowed(image.astype(dtype), cov.astype(dtype), base.t, base.slot, base.parity, base.front, near, occ, occ_map, occ_sph)


def bars(colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, lt, shadow_ws, shadow_depth_0):
    """Both evaluations, the mask of rays to compare (unflagged in either) and the bar per output, as colliders_reference.bars: 4 x the largest
    float32-versus-float64 difference on those rays, with 'shadow' added."""
    args = (colliders, rgb, checker, checker_dim, ambient, rays_o, rays_d, t_min, t_max, bg, weights_sum, depth_0, acc, lt, shadow_ws, shadow_depth_0)
    r32, r64 = draw(*args, dtype=np.float32), draw(*args, dtype=np.float64)
    keep = ~(r32.near | r64.near)
    hit = keep & (r64.slot >= 0)
    mx = lambda a, b, m: float(np.abs(a[m].astype(np.float64) - b[m]).max()) if m.any() else 0.0   # noqa: E731
    diff = {"image": mx(r32.image, r64.image, keep), "coverage": mx(r32.coverage, r64.coverage, keep), "t": mx(r32.t, r64.t, hit),
            "shadow": mx(r32.occ, r64.occ, keep)}
    return r32, r64, keep, {k: 4.0 * v for k, v in diff.items()}, diff
