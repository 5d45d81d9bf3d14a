"""The collider overlay without a GPU: properties of the numpy restatement (tests/colliders_reference.py), the C ABI's declaration,
export and binding, the style's ctypes mirror, and main_render's arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

import colliders_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB = cr.default_rgb()
DTYPES = [np.float32, np.float64]


def _header():
    return open(os.path.join(ROOT, "include", "pienerf_hip.h")).read()


def _draw(cols, o, d, s, d0, acc, dtype=np.float32, bg=1.0, t_min=0.2, t_max=12.0, checker=0.0, checker_dim=0.5, ambient=0.3):
    f = lambda v, w: np.asarray(v, np.float32).reshape(-1, w) if w > 1 else np.asarray(v, np.float32).reshape(-1)   # noqa: E731
    return cr.draw(cols, RGB, checker, checker_dim, ambient, f(o, 3), f(d, 3), t_min, t_max, bg, f(s, 1), f(d0, 1), f(acc, 3), dtype=dtype)


def _finish(acc, s, bg):
    """What the frame's epilogue writes: acc + (1 - s) bg in float32, multiply and add rounded separately."""
    acc, s = np.asarray(acc, np.float32), np.asarray(s, np.float32)
    k = ((np.float32(1) - s) * np.float32(bg)).astype(np.float32)
    return (acc + k[:, None]).astype(np.float32)


# ---------------------------------------------------------------- the restatement's properties
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_state_leaves_the_frames_own_pixels(dtype):
    o, d = cr.get_rays_numpy(cr.STANDARD["eye"], 16, 12, 14.4)
    acc, s, d0 = cr.standard_inputs(o.shape[0], seed=3)
    r = _draw(cr.slots(), o, d, s, d0, acc, dtype, bg=0.7)
    assert np.array_equal(r.image.astype(np.float32), _finish(acc, s, 0.7)) or dtype is np.float64
    if dtype is np.float64:
        want = acc.astype(np.float64) + ((1.0 - s.astype(np.float64)) * np.float64(np.float32(0.7)))[:, None]
        assert np.array_equal(r.image, want)
    assert np.array_equal(r.coverage, s.astype(dtype)) and np.isinf(r.t).all() and (r.slot == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_back_facing_plane_is_not_hit(dtype):
    floor = cr.slots(cr.plane((0, -1, 0), (0, 1, 0)))
    down = _draw(floor, [0, 1, 0], [0, -1, 0], [0.0], [0.0], [[0, 0, 0]], dtype)
    assert down.slot[0] == 0 and abs(down.t[0] - 2.0) < 1e-6
    up = _draw(floor, [0, -3, 0], [0, 1, 0], [0.0], [0.0], [[0, 0, 0]], dtype)     # from below: the back face
    assert up.slot[0] == -1 and np.isinf(up.t[0]) and np.array_equal(up.image, np.ones((1, 3), dtype))
    along = _draw(floor, [0, 1, 0], [1, 0, 0], [0.0], [0.0], [[0, 0, 0]], dtype)   # parallel: n.d = 0 is not < 0
    assert along.slot[0] == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_sphere_roots_and_the_containers_far_wall(dtype):
    ball, box = cr.slots(cr.sphere((0, 0, 0), 1.0)), cr.slots(cr.sphere((0, 0, 0), 1.0, inside=True))
    z = dict(s=[0.0], d0=[0.0], acc=[[0, 0, 0]])
    assert abs(_draw(ball, [0, 0, 3], [0, 0, -1], dtype=dtype, **z).t[0] - 2.0) < 1e-6          # outside: the near root
    assert abs(_draw(ball, [0, 0, 0.5], [0, 0, -1], dtype=dtype, **z).t[0] - 1.5) < 1e-6        # eye inside: the near root is behind t_min, the far one
    assert abs(_draw(box, [0, 0, 3], [0, 0, -1], dtype=dtype, **z).t[0] - 4.0) < 1e-6           # the container: its far wall only, also from outside
    assert abs(_draw(box, [0, 0, 0.5], [0, 0, -1], dtype=dtype, **z).t[0] - 1.5) < 1e-6
    assert _draw(ball, [0, 2, 3], [0, 0, -1], dtype=dtype, **z).slot[0] == -1                   # a miss
    # t is in units of rays_d as given: a direction of length 2 halves it
    assert abs(_draw(ball, [0, 0, 3], [0, 0, -2], dtype=dtype, **z).t[0] - 1.0) < 1e-6
    # the same shade for the same geometry, whatever the direction's length: normal.d_hat
    a = _draw(ball, [0, 0.3, 3], [0, 0, -1], dtype=dtype, **z).image
    b = _draw(ball, [0, 0.3, 3], [0, 0, -2], dtype=dtype, t_max=6.0, t_min=0.1, **z).image
    assert np.abs(a - b).max() < 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_nearest_slot_wins_and_ties_go_to_the_lower_index(dtype):
    z = dict(s=[0.0], d0=[0.0], acc=[[0, 0, 0]])
    two = cr.slots(cr.sphere((0, 0, -2), 0.5), cr.sphere((0, 0, 0), 0.5))
    assert _draw(two, [0, 0, 3], [0, 0, -1], dtype=dtype, **z).slot[0] == 1
    same = cr.slots(cr.sphere((0, 0, 0), 0.5), cr.sphere((0, 0, 0), 0.5))
    assert _draw(same, [0, 0, 3], [0, 0, -1], dtype=dtype, **z).slot[0] == 0
    gap = [None] * 7 + [cr.sphere((0, 0, 0), 0.5)]
    assert _draw(gap, [0, 0, 3], [0, 0, -1], dtype=dtype, **z).slot[0] == 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_collider_at_or_beyond_t_max_changes_nothing(dtype):
    floor = cr.slots(cr.plane((0, -1, 0), (0, 1, 0)))
    acc, s = [[0.2, 0.1, 0.05]], [0.4]
    far = _draw(floor, [0, 1, 0], [0, -1, 0], s, [1.0], acc, dtype, t_max=2.0, bg=0.6)   # t = 2 = t_max: outside (t_min, t_max)
    assert far.slot[0] == -1 and np.array_equal(far.image.astype(np.float32), _finish(acc, s, 0.6)) and far.coverage[0] == np.float32(0.4)
    fade = _draw(floor, [0, 1, 0], [0, -1, 0], s, [1.0], acc, dtype, t_max=2.0 + 1e-3, bg=0.6)   # just inside: a is almost 0
    assert fade.slot[0] == 0 and np.abs(fade.image.astype(np.float32) - _finish(acc, s, 0.6)).max() < 2e-3


def test_in_front_and_behind_on_hand_made_rays():
    ball = cr.slots(cr.sphere((0, 0, 0), 1.0))
    rgb, amb = RGB[0].astype(np.float64), 0.3
    col = rgb * (amb + (1 - amb) * 1.0)            # head-on: |normal.d_hat| = 1; t = 2 < t_max / 2: a = 1
    acc, s = np.array([0.3, 0.2, 0.1]), 0.5
    front = _draw(ball, [0, 0, 3], [0, 0, -1], [s], [s * 2.5], [acc], np.float64, bg=0.25)     # the object at t_obj = 2.5, behind the ball
    assert front.front[0] and np.allclose(front.image[0], col, atol=1e-7) and front.coverage[0] == 1.0
    behind = _draw(ball, [0, 0, 3], [0, 0, -1], [s], [s * 1.5], [acc], np.float64, bg=0.25)    # the object at 1.5, in front of it
    assert not behind.front[0] and np.allclose(behind.image[0], acc + (1 - s) * col, atol=1e-7) and behind.coverage[0] == 1.0
    # half faded: t_max = 8 / 3 gives a = (8/3 - 2) / (4/3) = 0.5
    t_max = 8.0 / 3.0
    f2 = _draw(ball, [0, 0, 3], [0, 0, -1], [s], [s * 2.5], [acc], np.float64, bg=0.25, t_max=t_max)
    assert np.allclose(f2.coverage[0], 0.5 + 0.5 * s, atol=1e-6) and np.allclose(f2.image[0], 0.5 * col + 0.5 * acc + (1 - (0.5 + 0.5 * s)) * 0.25, atol=1e-6)
    b2 = _draw(ball, [0, 0, 3], [0, 0, -1], [s], [s * 1.5], [acc], np.float64, bg=0.25, t_max=t_max)
    assert np.allclose(b2.coverage[0], s + (1 - s) * 0.5, atol=1e-6) and np.allclose(b2.image[0], acc + (1 - s) * 0.5 * col + (1 - s) * 0.5 * 0.25, atol=1e-6)
    # a ray with s <= 1e-4 has no object depth: the collider is in front
    thin = _draw(ball, [0, 0, 3], [0, 0, -1], [5e-5], [5e-5 * 0.5], [acc * 0], np.float64)
    assert thin.front[0]


def test_checker_pattern_and_the_tangent_frame():
    floor = cr.slots(cr.plane((0, 0, 0), (0, 1, 0)))
    z = dict(s=[0.0], d0=[0.0], acc=[[0, 0, 0]])
    px = lambda x, zz: _draw(floor, [x, 1, zz], [0, -1, 0], dtype=np.float64, checker=1.0, checker_dim=0.25, **z)   # noqa: E731
    a, b, c = px(0.5, 0.5), px(1.5, 0.5), px(1.5, 1.5)
    assert (a.parity[0], b.parity[0], c.parity[0]) in ((0, 1, 0), (1, 0, 1))
    assert np.allclose(np.minimum(a.image, b.image) * 4, np.maximum(a.image, b.image), atol=1e-7) and np.allclose(a.image, c.image)
    # n = (0, 1, 0): |n| is smallest on x (tie with z, lowest index): u = n x e_x normalised = (0, 0, -1), v = n x u = (-1, 0, 0)
    u, v = cr.tangent_frame(np.array([0.0, 1.0, 0.0]))
    assert np.array_equal(u, [0, 0, -1]) and np.array_equal(v, [-1, 0, 0])
    n = np.array([0.2, 1.0, 0.0]) / np.linalg.norm([0.2, 1.0, 0.0])
    u, v = cr.tangent_frame(n)      # smallest on z
    assert np.allclose(u, np.cross(n, [0, 0, 1]) / np.linalg.norm(np.cross(n, [0, 0, 1]))) and np.allclose(v, np.cross(n, u))
    assert abs(u @ n) < 1e-15 and abs(v @ n) < 1e-15 and abs(u @ v) < 1e-15
    off = _draw(floor, [0.5, 1, 0.5], [0, -1, 0], dtype=np.float64, checker=0.0, **z)
    assert off.parity[0] == 0


SCENES = {
    "standard": lambda: (cr.standard_scene(), cr.STANDARD["eye"]),
    "slot7": lambda: ([None] * 7 + [cr.sphere((0.0, 0.0, 0.9), 0.5)], cr.STANDARD["eye"]),
    "tilted": lambda: (cr.slots(cr.plane((0.0, -0.95, 0.0), (0.2, 1.0, 0.0))), cr.STANDARD["eye"]),
    "inside": lambda: (cr.slots(cr.sphere((0.0, 0.0, 0.9), 0.5)), (0.1, 0.05, 1.0)),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_coverage_bounds_and_dtype_agreement_on_the_gpu_tests_scenes(name):
    """cov in [s, 1]; float32 and float64 take every decision alike on the unflagged rays, which are all but 0.5 % at most."""
    S = cr.STANDARD
    cols, eye = SCENES[name]()
    o, d = cr.get_rays_numpy(eye, S["W"], S["H"], 0.9 * S["W"])
    acc, s, d0 = cr.standard_inputs(o.shape[0])
    r32, r64, keep, bar, diff = cr.bars(cols, RGB, S["checker"], S["checker_dim"], S["ambient"], o, d, S["t_min"], S["t_max"], S["bg"], s, d0, acc)
    for r in (r32, r64):
        assert (r.coverage >= s - 1e-6).all() and (r.coverage <= 1 + 1e-6).all()
    assert (~keep).mean() <= 0.005
    assert np.array_equal(r32.slot[keep], r64.slot[keep]) and np.array_equal(r32.parity[keep], r64.parity[keep])
    assert np.array_equal(r32.front[keep], r64.front[keep])
    hit = r64.slot >= 0
    print(f"{name}: {int((~keep).sum())} of {keep.size} rays near a decision; hits per slot {np.bincount(r64.slot[hit], minlength=8).tolist()}, "
          f"{r64.front[hit].mean():.2f} of them in front; float32 vs float64: {diff}")
    assert hit.sum() > 100
    if name == "standard":
        assert (np.bincount(r64.slot[hit], minlength=8)[:3] > 300).all() and 0.3 < r64.front[hit].mean() < 0.7


# ---------------------------------------------------------------- the C ABI and its mirror
def test_symbol_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bpn_draw_colliders\s*\(", text)
    assert "pn_draw_colliders" in _lib.SIGNATURES and hasattr(so, "pn_draw_colliders")
    res, args = _lib.SIGNATURES["pn_draw_colliders"]
    decl = re.search(r"int\s+pn_draw_colliders\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert res is ctypes.c_int and len(args) == len(decl.split(",")) == 14


def test_style_mirror_follows_the_header():
    """pienerf_amd._lib.ColliderStyle is the ctypes mirror of pn_collider_style: same members in the same order at the same offsets, 108 bytes."""
    from pienerf_amd._lib import ColliderStyle
    text = _header()
    body = re.search(r"typedef\s+struct\s+pn_collider_style\s*\{(.*?)\}\s*pn_collider_style\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\bfloat\s+(\w+)((?:\[\d+\])*)\s*;", body)
    want, off = [], 0
    for name, dims in decl:
        n = int(np.prod([int(v) for v in re.findall(r"\d+", dims)])) if dims else 1
        want.append((name, off, 4 * n))
        off += 4 * n
    got = [(n, getattr(ColliderStyle, n).offset, getattr(ColliderStyle, n).size) for n, _ in ColliderStyle._fields_]
    assert got == want == [("rgb", 0, 96), ("checker", 96, 4), ("checker_dim", 100, 4), ("ambient", 104, 4)]
    assert ctypes.sizeof(ColliderStyle) == off == 108
    src = open(os.path.join(ROOT, "pienerf_amd", "csrc", "pn_colliders.hip")).read()
    assert re.search(r"static_assert\(sizeof\(pn_collider_style\)\s*==\s*108", src)


def test_collider_style_defaults_and_checks():
    from pienerf_amd.colliders import OTHER_GREY, PLANE_GREY, collider_style
    st = collider_style(rgb=[(1, 0, 0)], types=[1, 1, 2, 3, 0, 0, 0, 0], checker=0.1)
    rows = [[st.rgb[k][j] for j in range(3)] for k in range(8)]
    assert rows[0] == [1, 0, 0] and rows[1] == [np.float32(PLANE_GREY)] * 3 and all(r == [np.float32(OTHER_GREY)] * 3 for r in rows[2:])
    assert st.checker == np.float32(0.1) and 0 <= st.ambient <= 1
    for bad in (dict(ambient=1.5), dict(checker=float("nan")), dict(rgb=[(0, 0, 0)] * 9), dict(rgb=[(0, 0)])):
        with pytest.raises(ValueError):
            collider_style(**bad)


def test_unit_is_built_without_contraction():
    from pienerf_amd.build import UNITS
    assert UNITS["pn_colliders.hip"] == ["-ffp-contract=off"]


# ---------------------------------------------------------------- Simulator / renderer, host side
def test_collider_state_needs_contact_enabled(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o = small_opt
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu")
    with pytest.raises(ValueError, match="enable_contact"):
        s.collider_state()
    s.enable_contact()
    s.add_plane((0, -1, 0), (0, 1, 0))
    s.add_sphere((0, 0, 0), 0.5, inside=True)
    assert s.collider_types() == [1, 3, 0, 0, 0, 0, 0, 0]


def test_overlay_arguments_are_checked_and_other_renders_refuse():
    import torch
    from pienerf_amd.nerf.overlay_colliders import ColliderOverlay
    from pienerf_amd.nerf.renderer import NeRFRenderer
    r = NeRFRenderer(bound=1, cuda_ray=True)
    assert r.collider_overlay_key() is None
    with pytest.raises(ValueError, match="93 doubles"):
        r.set_collider_overlay(torch.zeros(92, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        r.set_collider_overlay(torch.zeros(93, dtype=torch.float64))   # host memory: the launch reads the state on the device
    r._overlay = ColliderOverlay(torch.zeros(93, dtype=torch.float64), None, 8.0)     # as if set: the refusals need no device
    rays = torch.zeros(4, 3)
    for call in (lambda: r.rund_cuda(rays, rays, perturb=True), lambda: r.run_cuda(rays, rays), lambda: r.run(rays, rays),
                 lambda: r.rund_cuda_ops(rays, rays)):
        with pytest.raises(RuntimeError, match="only the deformed path"):
            call()
    r.clear_collider_overlay()
    assert r.collider_overlay_key() is None


# ---------------------------------------------------------------- main_render
def test_main_render_arguments_parse():
    from pienerf_amd import main_render
    a = main_render.parser().parse_args(["--floor", "-0.95", "--draw_colliders", "--collider_color", "1", "0.5", "0", "--collider_color", "0", "0", "1",
                                         "--checker", "0.2"])
    assert a.draw_colliders and a.collider_color == [[1.0, 0.5, 0.0], [0.0, 0.0, 1.0]] and a.checker == 0.2
    d = main_render.parser().parse_args([])
    assert not d.draw_colliders and d.collider_color is None and d.checker is None
    main_render.check_overlay_args(a)
    main_render.check_overlay_args(d)


def test_main_render_draw_colliders_needs_a_collider(tmp_path):
    from pienerf_amd import main_render
    with pytest.raises(SystemExit, match="--draw_colliders needs"):
        main_render.run(main_render.parser().parse_args(["--draw_colliders", "--out", str(tmp_path / "o"), "--device", "cpu"]))
    with pytest.raises(SystemExit, match="need --draw_colliders"):
        main_render.run(main_render.parser().parse_args(["--floor", "-1", "--checker", "0.3", "--out", str(tmp_path / "o"), "--device", "cpu"]))
    assert not (tmp_path / "o").exists()
