"""The point overlay without a GPU: the numpy restatement of the law (tests/points_overlay_reference.py) against a float64 projection and
against the reference's point painting, the style's validation, the C ABI's mirror and main_render's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import points_overlay_reference as pr
from conftest import ROOT
from pienerf_amd import _lib
from pienerf_amd.points_overlay import MODES, point_style


def test_restatement_agrees_with_a_float64_projection():
    """Every test point was built from a pixel: the fp32 projection and the float64 one floor to that pixel, and agree to fp32 rounding."""
    rng = np.random.default_rng(0)
    pix = [(int(rng.integers(0, pr.W)), int(rng.integers(0, pr.H))) for _ in range(200)]
    ts = pr.t_ladder(200)
    pos = np.stack([pr.point_at(pr.POSE, pr.INTR, px, py, t, *rng.uniform(-0.3, 0.3, 2)) for (px, py), t in zip(pix, ts)])
    u32, v32, t32, ok32 = pr.project(pr.POSE, pr.INTR, pos)
    u64, v64, t64, ok64 = pr.project(pr.POSE, pr.INTR, pos, dtype=np.float64)
    assert ok32.all() and ok64.all() and u32.dtype == np.float32
    assert np.array_equal(np.floor(u32), [p[0] for p in pix]) and np.array_equal(np.floor(v32), [p[1] for p in pix])
    assert np.array_equal(np.floor(u64), [p[0] for p in pix]) and np.array_equal(np.floor(v64), [p[1] for p in pix])
    assert np.abs(u32 - u64).max() < 1e-4 and np.abs(v32 - v64).max() < 1e-4 and np.abs(t32 / t64 - 1).max() < 1e-6
    assert np.abs(t64 / np.asarray(ts) - 1).max() < 1e-6      # t is the distance the point was placed at
    # every key of the splat is the nearest point of its pixel, the lowest index on ties
    keys = pr.splat(np.concatenate([pos, pos[:5]]), pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, 0)
    for p, key in enumerate(keys):
        here = [i for i, q in enumerate(pix) if q[1] * pr.W + q[0] == p]
        if not here:
            assert key == pr.EMPTY
        else:
            best = min(here, key=lambda i: (t32[i], i))
            assert key & 0xffffffff == best and np.array([key >> 32], np.uint32).view(np.float32)[0] == t32[best]


def test_restatement_paints_the_reference_pixel_set():
    """r = 0, xray, flat (0, 0, 1), alpha 1 on points in front of the camera that project inside the image: exactly the pixels the reference paints."""
    pos = pr.cloud(70, rejects=False)
    image, s, d0, ct = pr.frame_inputs()
    st = pr.style(radius=0, xray=True, rgb=(0, 0, 1), alpha=1.0)
    out, pid, pt = pr.draw(pos, None, None, pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, s, d0, None, None, st, image)
    mine = {(p // pr.W, p % pr.W) for p in np.nonzero(pid >= 0)[0]}
    assert mine == pr.reference_pixels(pos, pr.POSE, pr.INTR, pr.H, pr.W) and len(mine) > 40
    blue = (out == np.array([0, 0, 1], np.float32)).all(axis=1)
    assert np.array_equal(blue, pid >= 0) and np.array_equal(out[~blue].view(np.uint32), image[~blue].view(np.uint32))
    # the two documented deviations: a point behind the camera and one with u, v in (-1, 0) are painted by the reference and dropped by the law
    bad = np.stack([pr.point_at(pr.POSE, pr.INTR, 7, 7, -1.7), pr.point_at(pr.POSE, pr.INTR, -1, -1, 2.3, 0.2, 0.2)])
    assert len(pr.reference_pixels(bad, pr.POSE, pr.INTR, pr.H, pr.W)) == 2
    assert (pr.draw(bad, None, None, pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, s, d0, None, None, st, image)[1] < 0).all()


def test_restatement_depth_test_and_modes():
    pos = pr.cloud(70)
    image, s, d0, ct = pr.frame_inputs()
    n = pos.shape[0]
    x = pr.draw(pos, None, None, pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, s, d0, ct, None, pr.style(radius=2, xray=True), image)
    o = pr.draw(pos, None, None, pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, s, d0, ct, None, pr.style(radius=2), image)
    assert (x[1] >= 0).sum() > (o[1] >= 0).sum() > 20            # some points are hidden behind the object or the collider
    # never drawn: the duplicates (a lower index wins), the point behind the camera, the one nearer than t_min, the non-finite ones; the off-screen
    # points' discs do reach into the image (index n - 3 sits one pixel outside the corner)
    assert not set(x[1][x[1] >= 0].tolist()) & {n - 9, n - 8, n - 7, n - 6, n - 2, n - 1} and (n - 3) in set(x[1].tolist())
    F = pr.gradients(n)
    for mode in ("strain", "volume"):
        out = pr.draw(pos, F, None, pr.POSE, pr.INTR, pr.W, pr.H, pr.T_MIN, s, d0, ct, None, pr.style(radius=0, xray=True, mode=mode, lo=-0.2, hi=0.4), image)[0]
        assert len({tuple(c) for c in out[x[1] >= 0][:40].round(3)}) > 5      # a ramp, not one colour


@pytest.mark.parametrize("bad", [dict(radius=-1), dict(radius=9), dict(radius=1.5), dict(mode="heat"), dict(rgb=(0, float("nan"), 0)), dict(rgb=(0, 1)),
                                 dict(alpha=1.5), dict(alpha=-0.1), dict(hidden_alpha=2), dict(hidden_alpha=float("nan")), dict(bias=float("inf")),
                                 dict(mode="strain", lo=1.0, hi=1.0), dict(mode="values", lo=2.0, hi=1.0), dict(lo=float("nan")),
                                 dict(marker_radius=-1), dict(marker_thickness=float("inf")), dict(ramp=((0, 0, 0), (1, 1, 1)))])
def test_style_validation_raises_on_each_bad_field(bad):
    with pytest.raises(ValueError, match="point_style"):
        point_style(**bad)


def test_style_defaults_and_mirror_follow_the_header():
    st = point_style()
    assert (st.radius, st.mode, st.xray, st.alpha, st.hidden_alpha) == (1, 0, 0, 1.0, 0.0) and (st.marker_radius, st.marker_thickness) == (10.0, 5.0)
    assert tuple(st.rgb) == (0.0, 0.0, 1.0)                       # the reference's point colour
    assert point_style(mode="flat", lo=1.0, hi=1.0).mode == 0     # the range belongs to the ramp modes
    text = open(os.path.join(ROOT, "include", "pienerf_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+pn_point_style\s*\{(.*?)\}\s*pn_point_style\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\b(int|float)\s+(\w+)((?:\[\d+\])*)\s*;", body)
    got = [(n, C.sizeof(t)) for n, t in _lib.PointStyle._fields_]
    want = [(n, 4 * int(np.prod([int(d) for d in re.findall(r"\d+", dims)] or [1]))) for _, n, dims in decl]
    assert got == want and C.sizeof(_lib.PointStyle) == 88
    for (n, t), (ct, _, _) in zip(_lib.PointStyle._fields_, decl):
        base = t
        while hasattr(base, "_length_"):
            base = base._type_
        assert base is (C.c_int if ct == "int" else C.c_float), n
    enum = re.search(r"enum\s*\{\s*PN_POINT_FLAT\s*=\s*0,\s*PN_POINT_STRAIN\s*=\s*1,\s*PN_POINT_VOLUME\s*=\s*2,\s*PN_POINT_VALUES\s*=\s*3\s*\}", text)
    assert enum and MODES == {"flat": 0, "strain": 1, "volume": 2, "values": 3} and MODES == pr.MODES
    src = open(os.path.join(ROOT, "pienerf_amd", "csrc", "pn_points_overlay.hip")).read()
    assert re.search(r"static_assert\(sizeof\(pn_point_style\)\s*==\s*88", src)
    from pienerf_amd.build import UNITS
    assert UNITS["pn_points_overlay.hip"] == ["-ffp-contract=off"]


def test_c_abi_is_declared_exported_and_checks_its_arguments_on_the_host():
    h = _lib.lib()
    for name in ("pn_draw_points", "pn_points_keys_bytes"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.pn_points_keys_bytes(24, 16) == 24 * 16 * 8 and h.pn_points_keys_bytes(0, 16) == 0
    # refused before anything is enqueued: no GPU is touched
    d = C.c_void_p(4096)
    intr = (C.c_float * 4)(*pr.INTR)
    call = lambda st, n=10, W=24, Hh=16, F=None, values=None: h.pn_draw_points(d, F, values, n, d, intr, W, Hh, 0.2, d, d, None, None, d, st, d, None,  # noqa: E731
                                                                                 None, None)
    st = point_style()
    st.radius = 9
    assert call(st) == 1
    assert call(point_style(mode="strain")) == 1 and call(point_style(mode="values")) == 1      # without F / values
    assert call(point_style(), n=2 ** 31) == 1 and call(point_style(), W=2 ** 16, Hh=2 ** 15) == 1 and call(point_style(), n=-1) == 1


def test_main_render_flags_parse():
    from pienerf_amd import main_render as mr
    a = mr.parser().parse_args("--draw_points --point_radius 2 --point_color 1 0.5 0 --point_mode strain --point_range 0 0.1 --point_xray --point_alpha 0.8 "
                               "--point_hidden_alpha 0.25 --no_drag_marker --drag 10 10 20 20 --floor -0.9 --draw_colliders --shadows --bg_radius 32 "
                               "--save_ply".split())
    mr.check_overlay_args(a)
    st = mr.point_style_from(a)
    assert (st.radius, st.mode, st.xray) == (2, 1, 1) and tuple(st.rgb) == (1.0, 0.5, 0.0) and abs(st.hi - 0.1) < 1e-7 and abs(st.alpha - 0.8) < 1e-7
    assert abs(st.hidden_alpha - 0.25) < 1e-7 and a.no_drag_marker
    plain = mr.parser().parse_args([])
    assert not plain.draw_points and not mr.point_args_given(plain)
    mr.check_overlay_args(plain)
    for bad in ("--point_radius 2", "--point_xray", "--no_drag_marker", "--draw_points --point_radius 9", "--draw_points --point_alpha 2",
                "--draw_points --point_mode strain --point_range 1 0"):
        with pytest.raises(SystemExit):
            mr.check_overlay_args(mr.parser().parse_args(bad.split()))
    with pytest.raises(SystemExit):
        mr.parser().parse_args("--draw_points --point_mode values".split())      # no array to hand in on the command line
