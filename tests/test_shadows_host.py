"""Shadows on the drawn colliders without a GPU: the light's frame and rays, properties of the numpy restatement
(tests/shadows_reference.py), the C ABI's declaration, export and binding, the light's ctypes mirror, and main_render's arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

import colliders_reference as cr
import shadows_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB = cr.default_rgb()
DTYPES = [np.float32, np.float64]
ST = cr.STANDARD


def _header():
    return open(os.path.join(ROOT, "include", "pienerf_hip.h")).read()


def _vec(a):
    return np.array([float(v) for v in a], np.float64)


# ---------------------------------------------------------------- the light's frame and its rays
def _directions():
    g = np.random.default_rng(5)
    return [tuple(v) for v in g.normal(size=(100, 3))] + [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, -2, 0)]


def test_light_frame_is_orthonormal_and_follows_the_checkers_rule():
    from pienerf_amd.colliders import shadow_light
    for d in _directions():
        lt = shadow_light(direction=d)
        L, U, V = _vec(lt.L), _vec(lt.U), _vec(lt.V)
        want = np.asarray(d, np.float64) / np.linalg.norm(d)
        assert np.abs(L - want).max() < 1e-7
        for a in (L, U, V):
            assert abs(a @ a - 1.0) < 1e-6
        assert abs(L @ U) < 1e-6 and abs(L @ V) < 1e-6 and abs(U @ V) < 1e-6
        u, v = cr.tangent_frame(want)          # the checker's rule, in fp64
        assert np.abs(U - u).max() < 1e-7 and np.abs(V - v).max() < 1e-7
        ref = sr.light(d)                      # the restatement's light is the same struct, member for member
        for k in "cLUV":
            assert np.array_equal(np.array(list(getattr(lt, k)), np.float32), ref[k]), k
        assert (lt.half, lt.D, lt.S, lt.strength, lt.bias, lt.spheres) == tuple(ref[k] for k in ("half", "D", "S", "strength", "bias", "spheres"))


def test_light_defaults_cover_the_box_from_every_direction():
    from pienerf_amd.colliders import shadow_light
    bound, min_near = 1.5, 0.2
    corners = np.array([[x, y, z] for x in (-bound, bound) for y in (-bound, bound) for z in (-bound, bound)])
    for d in _directions():
        lt = shadow_light(direction=d, bound=bound, min_near=min_near, resolution=128)
        L, U, V = _vec(lt.L), _vec(lt.U), _vec(lt.V)
        assert abs(lt.half - np.sqrt(3.0) * bound) < 1e-6 and abs(lt.D - (lt.half + 2 * min_near)) < 1e-6
        assert abs(lt.bias - 1.5 * 2 * lt.half / 128) < 1e-7 and lt.S == 128 and lt.spheres == 1
        assert (np.abs(corners @ U) <= lt.half + 1e-5).all() and (np.abs(corners @ V) <= lt.half + 1e-5).all()
        assert (lt.D - corners @ L > min_near).all()     # every corner lies more than min_near below the plane of the rays' origins
    lt = shadow_light(extent=0.7, bias=0.01, centre=(0.1, 0.2, 0.3), spheres=False, strength=1.0)
    assert abs(lt.half - 0.7) < 1e-7 and abs(lt.bias - 0.01) < 1e-8 and lt.spheres == 0 and abs(lt.c[1] - 0.2) < 1e-7 and lt.strength == 1.0


def test_light_arguments_are_checked():
    from pienerf_amd.colliders import shadow_light
    for bad in (dict(direction=(0, 0, 0)), dict(direction=(1, float("nan"), 0)), dict(direction=(float("inf"), 0, 0)), dict(strength=-0.1),
                dict(strength=1.1), dict(resolution=1), dict(resolution=4097), dict(extent=0.0), dict(extent=-1.0), dict(bias=-1e-3)):
        with pytest.raises(ValueError):
            shadow_light(**bad)
    shadow_light(resolution=2), shadow_light(resolution=4096), shadow_light(strength=0.0), shadow_light(bias=0.0)


def test_shadow_rays_put_texel_centres_where_fu_and_fv_are_integers():
    from pienerf_amd.colliders import shadow_light, shadow_rays
    for d, S in (((0.4, 1.0, 0.3), 8), ((0, 1, 0), 5), ((-0.7, 0.5, 0.2), 16)):
        lt = shadow_light(direction=d, resolution=S, centre=(0.1, -0.2, 0.05))
        o, dd = shadow_rays(lt, "cpu")
        assert o.shape == dd.shape == (S * S, 3) and o.dtype == dd.dtype
        o, dd = o.numpy().astype(np.float64), dd.numpy().astype(np.float64)
        ref_o, ref_d = sr.light_rays(sr.light(d, resolution=S, centre=(0.1, -0.2, 0.05)))
        assert np.abs(o - ref_o).max() < 1e-6 and np.array_equal(dd, ref_d.astype(np.float32).astype(np.float64))
        c, L, U, V = _vec(lt.c), _vec(lt.L), _vec(lt.U), _vec(lt.V)
        assert np.abs(dd + L[None]).max() == 0 and abs(np.linalg.norm(dd[0]) - 1) < 1e-6
        for t in (0.0, 1.3):     # anywhere along the ray: the law's map coordinates are the texel's indices
            r = o + t * dd - c[None]
            fu = (r @ U + lt.half) * (S / (2 * lt.half)) - 0.5
            fv = (r @ V + lt.half) * (S / (2 * lt.half)) - 0.5
            j, i = np.divmod(np.arange(S * S), S)
            assert np.abs(fu - i).max() < 1e-4 and np.abs(fv - j).max() < 1e-4
            assert np.abs((lt.D - r @ L) - t).max() < 1e-5     # t_r of a point on the ray is the render's t


# ---------------------------------------------------------------- the restatement's properties
def _standard(N=None, first=0):
    o, d = cr.get_rays_numpy(ST["eye"], ST["W"], ST["H"], 0.9 * ST["W"])
    acc, s, d0 = cr.standard_inputs(o.shape[0])
    sl = slice(first, o.shape[0] if N is None else first + N)
    return o[sl], d[sl], s[sl], d0[sl], acc[sl]


def _args(cols, o, d, s, d0, acc):
    return (cols, RGB, ST["checker"], ST["checker_dim"], ST["ambient"], o, d, ST["t_min"], ST["t_max"], ST["bg"], s, d0, acc)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strength_zero_and_an_empty_map_equal_the_unshadowed_draw_exactly(dtype):
    o, d, s, d0, acc = _standard()
    cols = cr.standard_scene()
    base = cr.draw(*_args(cols, o, d, s, d0, acc), dtype=dtype)
    ws, wd = sr.synthetic_maps(16)
    off = sr.draw(*_args(cols, o, d, s, d0, acc), sr.light(strength=0.0, resolution=16), ws, wd, dtype=dtype)
    assert (off.occ > 0).sum() > 300           # occlusion there is, it just does not darken
    empty = sr.draw(*_args(cols, o, d, s, d0, acc), sr.light(resolution=16, spheres=False), np.zeros_like(ws), np.zeros_like(wd), dtype=dtype)
    assert (empty.occ == 0).all()
    for r in (off, empty):
        assert np.array_equal(r.image, base.image) and np.array_equal(r.coverage, base.coverage) and np.array_equal(r.t, base.t, equal_nan=True)
        assert np.array_equal(r.slot, base.slot)
    full = sr.draw(*_args(cols, o, d, s, d0, acc), sr.light(resolution=16), ws, wd, dtype=dtype)
    lit = full.occ == 0
    assert lit.sum() > 300 and (~lit).sum() > 300
    assert np.array_equal(full.image[lit], base.image[lit])             # every ray with occ = 0 keeps its bits
    assert (full.image[~lit] <= base.image[~lit] + 1e-6).all() and (full.image[~lit] < base.image[~lit]).any()
    assert np.array_equal(full.coverage, base.coverage)


def _one_texel_map(S, sm, t_o):
    return np.full(S * S, sm, np.float32), np.full(S * S, np.float32(sm) * np.float32(t_o), np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_receiver_in_front_of_the_texels_depth_is_lit_and_behind_it_shadowed_by_s_m(dtype):
    lt = sr.light((0, 1, 0), resolution=64, bound=1.0, min_near=0.2)     # D = sqrt(3) + 0.4, bias 0.08; a point at height y has t_r = D - y
    D = float(lt["D"])
    x = np.array([[0.11, -0.5, 0.07]], dtype)
    t_r = D + 0.5
    for sm in (1.0, 0.37):
        for t_o, want in ((t_r - 0.3, sm), (t_r + 0.3, 0.0), (t_r - 0.5 * float(lt["bias"]), 0.0)):      # the last: behind, but within the bias
            ws, wd = _one_texel_map(64, sm, t_o)
            occ, occ_map, occ_sph, near, w = sr.occlusion(lt, ws, wd, cr.slots(), 0, x, dtype)
            assert abs(float(occ[0]) - want) < 1e-6 and occ_sph[0] == 0, (sm, t_o)
            assert abs(float(w.sum()) - 1.0) < 1e-6 and (w >= 0).all()        # the four bilinear weights
    ws, wd = _one_texel_map(64, 5e-5, 1.0)        # s_m <= 1e-4: no depth, no shadow
    assert sr.occlusion(lt, ws, wd, cr.slots(), 0, x, dtype)[0][0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_point_outside_the_map_gets_nothing_and_the_border_fades(dtype):
    lt = sr.light((0, 1, 0), resolution=8)
    half = float(lt["half"])
    ws, wd = _one_texel_map(8, 1.0, 0.5)
    U, V = lt["U"].astype(np.float64), lt["V"].astype(np.float64)
    at = lambda u, v: np.asarray([np.float64(u) * U + np.float64(v) * V + np.array([0, -0.9, 0])], dtype)   # noqa: E731
    occ = lambda x: float(sr.occlusion(lt, ws, wd, cr.slots(), 0, x, dtype)[0][0])   # noqa: E731
    assert occ(at(0.0, 0.0)) == pytest.approx(1.0, abs=1e-6)
    for u, v in ((half * 1.2, 0), (0, -half * 1.2), (5 * half, 5 * half), (1e30, 0)):
        assert occ(at(u, v)) == 0
    for bad in (np.inf, -np.inf, np.nan):        # a non-finite hit point reads nothing
        assert occ(np.asarray([[bad, -0.9, 0.0]], dtype)) == 0
    texel = 2 * half / 8
    assert occ(at(half - 0.25 * texel, 0.0)) == pytest.approx(0.75, abs=1e-4)      # a quarter of a texel inside the edge: three quarters of the weight in the map


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ball_shadows_the_floor_below_it_not_itself_and_container_and_planes_cast_nothing(dtype):
    R, c = 0.3, np.array([0.2, -0.3, 0.4])
    cols = cr.slots(cr.plane((0, -0.95, 0), (0, 1, 0)), cr.sphere(c, R), cr.sphere((0, 0, 0), 1.6, inside=True), cr.plane((0, 0.5, 0), (0, -1, 0)))
    lt = sr.light((0.4, 1.0, 0.3), resolution=8)
    L = lt["L"].astype(np.float64)
    ws, wd = np.zeros(64, np.float32), np.zeros(64, np.float32)
    occ = lambda x, k: float(sr.occlusion(lt, ws, wd, cols, k, np.asarray([x], dtype), dtype)[0][0])   # noqa: E731
    below = c - L * ((c[1] + 0.95) / L[1])         # straight down-light of the ball's centre, on the floor
    assert abs(below[1] + 0.95) < 1e-12 and occ(below, 0) == 1
    side = np.cross(L, [0, 1, 0])
    side /= np.linalg.norm(side)
    assert occ(below + 1.5 * R * side, 0) == 0     # a radius and a half to the side
    assert occ(below + 0.9 * R * side, 0) == 1
    assert occ(c + 3 * R * L, 0) == 0              # up-light of the ball: it is behind the point
    for p in (c + R * L, c - R * L, c + R * side):  # the ball does not shadow itself: neither its lit nor its unlit side
        assert occ(p, 1) == 0
    assert occ(c - R * L, 0) == 1                  # ... the same point as a floor's would be shadowed
    # container and planes: a point inside the container, under the ceiling plane, is lit by all of them
    assert occ(np.array([-0.8, -0.95, -0.5]), 0) == 0
    no = dict(lt, spheres=0)
    assert float(sr.occlusion(no, ws, wd, cols, 0, np.asarray([below], dtype), dtype)[0][0]) == 0


GPU_CASES = [(name, S) for name in sr.LIGHTS for S in (4, 16, 64)]


@pytest.mark.parametrize("name,S", GPU_CASES)
def test_dtype_agreement_on_the_gpu_cases(name, S):
    """float32 and float64 take every decision alike on the unflagged rays of the GPU launch cases, which are all but 1.5 % at most."""
    o, d, s, d0, acc = _standard()
    cols = cr.standard_scene()
    ws, wd = sr.synthetic_maps(S)
    r32, r64, keep, bar, diff = sr.bars(*_args(cols, o, d, s, d0, acc), sr.light(sr.LIGHTS[name], resolution=S), ws, wd)
    print(f"{name} S {S}: {int((~keep).sum())} of {keep.size} rays near a decision; occ > 0 on {int((r64.occ > 0).sum())}, casters block "
          f"{int((r64.occ_sph > 0).sum())}; float32 vs float64: {diff}")
    assert (~keep).mean() <= 0.015
    assert np.array_equal(r32.slot[keep], r64.slot[keep]) and np.array_equal(r32.parity[keep], r64.parity[keep])
    assert np.array_equal(r32.front[keep], r64.front[keep]) and np.array_equal(r32.occ_sph[keep], r64.occ_sph[keep])
    assert np.array_equal(r32.occ[keep] == 0, r64.occ[keep] == 0)
    assert np.abs(r32.occ[keep] - r64.occ[keep]).max() < 1e-3          # a decision taken differently would move occ by a texel's weight times s_m
    assert (r64.occ[keep] > 0.5).sum() > 100 and (r64.occ[keep] == 0).sum() > 500 and (r64.occ_sph[keep] > 0).sum() > 30
    assert ((r64.occ_map > 0) & (r64.occ_map < 1)).sum() > 100


# ---------------------------------------------------------------- the C ABI and its mirror
def test_symbol_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bpn_draw_colliders_shadowed\s*\(", text)
    assert "pn_draw_colliders_shadowed" in _lib.SIGNATURES and hasattr(so, "pn_draw_colliders_shadowed")
    res, args = _lib.SIGNATURES["pn_draw_colliders_shadowed"]
    decl = re.search(r"int\s+pn_draw_colliders_shadowed\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert res is ctypes.c_int and len(args) == len(decl.split(",")) == 18
    assert args[13] is _lib.ShadowLight and "pn_shadow_light light" in decl.split(",")[13]      # by value
    base = _lib.SIGNATURES["pn_draw_colliders"][1]
    assert args[:13] == base[:13] and args[-1] is base[-1]


def test_light_mirror_follows_the_header():
    """pienerf_amd._lib.ShadowLight is the ctypes mirror of pn_shadow_light: same members in the same order at the same offsets, 72 bytes."""
    from pienerf_amd._lib import ShadowLight
    text = _header()
    body = re.search(r"typedef\s+struct\s+pn_shadow_light\s*\{(.*?)\}\s*pn_shadow_light\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want, off = [], 0
    for typ, names in re.findall(r"\b(float|int)\s+([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            n = int(np.prod([int(v) for v in re.findall(r"\d+", dims)])) if dims else 1
            want.append((name, typ, off, 4 * n))
            off += 4 * n
    kind = lambda t: "int" if t is ctypes.c_int else "float"   # noqa: E731
    got = [(n, kind(t), getattr(ShadowLight, n).offset, getattr(ShadowLight, n).size) for n, t in ShadowLight._fields_]
    assert got == want == [("c", "float", 0, 12), ("L", "float", 12, 12), ("U", "float", 24, 12), ("V", "float", 36, 12), ("half", "float", 48, 4),
                           ("D", "float", 52, 4), ("S", "int", 56, 4), ("strength", "float", 60, 4), ("bias", "float", 64, 4), ("spheres", "int", 68, 4)]
    assert ctypes.sizeof(ShadowLight) == off == 72
    src = open(os.path.join(ROOT, "pienerf_amd", "csrc", "pn_colliders.hip")).read()
    assert re.search(r"static_assert\(sizeof\(pn_shadow_light\)\s*==\s*72", src)


# ---------------------------------------------------------------- renderer / harness, host side
def test_shadows_need_an_overlay_and_are_cleared_with_it():
    import torch
    from pienerf_amd.colliders import collider_style, shadow_light
    from pienerf_amd.nerf.overlay_colliders import ColliderOverlay
    from pienerf_amd.nerf.renderer import NeRFRenderer
    r = NeRFRenderer(bound=1, cuda_ray=True)
    with pytest.raises(RuntimeError, match="set_collider_overlay"):
        r.set_collider_shadows(shadow_light())
    r._overlay = ColliderOverlay(torch.zeros(93, dtype=torch.float64), collider_style(), 8.0)     # as if set: host memory is enough for the bookkeeping
    key0 = r.collider_overlay_key()
    with pytest.raises(ValueError, match="ShadowLight"):
        r.set_collider_shadows("sun")
    r.set_collider_shadows(shadow_light(resolution=8))
    assert r.shadow_ws.shape == r.shadow_depth_0.shape == (64,) and r._shadows.rays_o.shape == (64, 3)
    key1 = r.collider_overlay_key()
    assert key1[:len(key0)] == key0 and len(key1) == len(key0) + 3      # the light's bytes and the two maps' addresses, only with shadows
    assert key1[-2:] == (r.shadow_ws.data_ptr(), r.shadow_depth_0.data_ptr())
    r.set_collider_shadows(shadow_light(resolution=8, strength=0.5))
    assert r.collider_overlay_key() != key1                                 # another light: another key
    r.clear_collider_shadows()
    assert r.collider_overlay_key() == key0 and r.shadow_ws is None
    r.set_collider_shadows(shadow_light(resolution=8))
    r.clear_collider_overlay()
    assert r.collider_overlay_key() is None and r._shadows is None


# ---------------------------------------------------------------- main_render
def test_main_render_arguments_parse():
    from pienerf_amd import main_render
    a = main_render.parser().parse_args(["--floor", "-0.95", "--draw_colliders", "--shadows", "--light", "0", "1", "0", "--shadow_strength", "0.8",
                                         "--shadow_res", "128"])
    assert a.shadows and a.light == [0.0, 1.0, 0.0] and a.shadow_strength == 0.8 and a.shadow_res == 128
    d = main_render.parser().parse_args(["--floor", "-0.95", "--draw_colliders", "--shadows"])
    assert d.shadows and d.light is None and d.shadow_strength is None and d.shadow_res is None
    n = main_render.parser().parse_args([])
    assert not n.shadows
    for args in (a, d, n):
        main_render.check_overlay_args(args)


def test_main_render_refusals(tmp_path):
    from pienerf_amd import main_render
    run = lambda *argv: main_render.run(main_render.parser().parse_args(list(argv) + ["--out", str(tmp_path / "o"), "--device", "cpu"]))   # noqa: E731
    with pytest.raises(SystemExit, match="--shadows needs --draw_colliders"):
        run("--floor", "-1", "--shadows")
    for extra in (("--light", "0", "1", "0"), ("--shadow_strength", "0.5"), ("--shadow_res", "64")):
        with pytest.raises(SystemExit, match="need --shadows"):
            run("--floor", "-1", "--draw_colliders", *extra)
    with pytest.raises(SystemExit, match="--draw_colliders needs"):
        run("--draw_colliders", "--shadows")
    assert not (tmp_path / "o").exists()
