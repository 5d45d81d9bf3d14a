"""Shadows on the drawn colliders on the GPU (csrc/pn_colliders.hip: pn_draw_colliders_shadowed): the launch against the numpy
restatement (tests/shadows_reference.py) and against the unshadowed launch, the renderer's shadow pass, the harness forms and main_render.

Comparison rule, as in test_gpu_colliders.py: rays the restatement flags as near a decision (in float32 or float64) are left out, at most 1.5 % of a
case's rays; on every other ray the hit slot matches and image / coverage / collider_t / shadow lie within 4 x the largest float32-versus-float64
difference of the restatement on those same rays.  Rays the restatement leaves unshadowed are compared bit for bit with pn_draw_colliders on the same
inputs, and so are coverage and collider_t on every ray.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import colliders_reference as cr
import shadows_reference as sr
import test_gpu_colliders as GC
from pienerf_amd import scene
from pienerf_amd._lib import ShadowLight, check, lib, ptr, stream_ptr
from pienerf_amd.colliders import shadow_light, shadow_rays
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
S = cr.STANDARD
RGB = cr.default_rgb()
MAX_FLAGGED = 0.015
_dev, _bits, _same, _np = GC._dev, GC._bits, GC._same, GC._np


def _light_dict(lt):
    """A ShadowLight as the restatement takes it."""
    f = np.float32
    return dict(c=np.array(list(lt.c), f), L=np.array(list(lt.L), f), U=np.array(list(lt.U), f), V=np.array(list(lt.V), f), half=f(lt.half), D=f(lt.D),
                S=int(lt.S), strength=f(lt.strength), bias=f(lt.bias), spheres=int(lt.spheres))


def _launch(state, style, o, d, s, d0, acc, lt, ws, wd, t_min=S["t_min"], t_max=S["t_max"], bg=S["bg"], shadow=True):
    N = o.shape[0]
    image = acc.clone()
    cov, ct = (torch.full((N,), -7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    sh = torch.full((N,), -7.0, dtype=torch.float32, device=DEV) if shadow else None
    check(lib().pn_draw_colliders_shadowed(ptr(state), C.byref(style), ptr(o), ptr(d), N, t_min, t_max, bg, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(ct),
                                           lt, ptr(ws), ptr(wd), ptr(sh), stream_ptr()), "draw_colliders_shadowed")
    torch.cuda.synchronize()
    return image, cov, ct, sh


def _share(err, bar):
    return {k: (err[k] / bar[k] if bar[k] > 0 else (0.0 if err[k] == 0 else float("inf"))) for k in err}


def _compare(name, got, plain, args, lt, ws, wd, max_flagged=MAX_FLAGGED):
    """The comparison rule of this file's docstring.  got = (image, coverage, collider_t, shadow) and plain = pn_draw_colliders' (image, coverage,
    collider_t) on the same inputs, as numpy; args = colliders_reference.draw's."""
    image, cov, ct, sh = got
    r32, r64, keep, bar, diff = sr.bars(*args, lt, ws, wd)
    N = image.shape[0]
    flagged = int((~keep).sum())
    hit = r64.slot >= 0
    err = {"image": np.abs(image[keep].astype(np.float64) - r64.image[keep]).max(initial=0.0),
           "coverage": np.abs(cov[keep].astype(np.float64) - r64.coverage[keep]).max(initial=0.0),
           "t": np.abs(ct[keep & hit].astype(np.float64) - r64.t[keep & hit]).max(initial=0.0),
           "shadow": np.abs(sh[keep].astype(np.float64) - r64.occ[keep]).max(initial=0.0)}
    print(f"{name}: N {N}, {flagged} rays near a decision, {int(hit.sum())} hits, occ > 0 on {int((r64.occ > 0).sum())} (casters {int((r64.occ_sph > 0).sum())}), "
          f"bar {bar}, kernel-vs-float64 {err}, share of the bar {_share(err, bar)}")
    assert flagged <= max_flagged * N, (name, flagged, N)
    assert np.array_equal(np.isfinite(ct)[keep], hit[keep]), name
    for k in err:
        assert err[k] <= bar[k], (name, k, err[k], bar[k])
    lit = keep & (r64.occ == 0) & (r32.occ == 0)
    assert np.array_equal(_bits(sh[lit]), np.zeros(int(lit.sum()), np.uint32)), name
    assert np.array_equal(_bits(image[lit]), _bits(plain[0][lit])), name          # unshadowed rays: the unshadowed launch's bits
    assert np.array_equal(_bits(cov), _bits(plain[1])) and np.array_equal(_bits(ct), _bits(plain[2])), name      # on every ray
    assert ((sh >= 0) & (sh <= 1)).all() and (sh[~np.isfinite(ct)] == 0).all()
    return r64, keep


# ---------------------------------------------------------------- the launch
@pytest.fixture(scope="module")
def standard():
    o, d = GC._look_at_rays(S["eye"])
    acc, s, d0 = cr.standard_inputs(o.shape[0])
    return o, d, acc, s, d0, GC._state(cr.standard_scene()), GC._style()


RAYS = {"all": (0, None), "one_ray": (2026, 1), "partial_workgroup": (2208, 257)}   # the one ray is shadowed in seven of the nine cases; the 257 see all three slots


@pytest.mark.parametrize("rays", list(RAYS))
@pytest.mark.parametrize("res", [4, 16, 64])
@pytest.mark.parametrize("name", list(sr.LIGHTS))
def test_launch_equals_the_restatement(name, res, rays, standard):
    o, d, acc, s, d0, state, style = standard
    first, count = RAYS[rays]
    sl = slice(first, o.shape[0] if count is None else first + count)
    o, d, acc, s, d0 = o[sl].contiguous(), d[sl].contiguous(), acc[sl], s[sl], d0[sl]
    lt = shadow_light(direction=sr.LIGHTS[name], resolution=res)
    ws, wd = sr.synthetic_maps(res)
    dev = (o, d, _dev(s), _dev(d0), _dev(acc))
    got = tuple(t.cpu().numpy() for t in _launch(state, style, *dev, lt, _dev(ws), _dev(wd)))
    plain = tuple(t.cpu().numpy() for t in GC._launch(state, style, *dev))
    args = (cr.standard_scene(), RGB, S["checker"], S["checker_dim"], S["ambient"], o.cpu().numpy(), d.cpu().numpy(), S["t_min"], S["t_max"], S["bg"], s, d0, acc)
    r64, keep = _compare(f"{name} S {res} {rays}", got, plain, args, _light_dict(lt), ws, wd)
    if rays == "all":
        assert (r64.occ[keep] > 0.5).sum() > 100 and (r64.occ[keep] == 0).sum() > 500 and (r64.occ_sph[keep] > 0).sum() > 30
        assert (got[0] != plain[0]).any(axis=1).sum() > 300          # the shadows are in the picture


def test_strength_zero_and_zero_maps_equal_the_unshadowed_launch_bit_for_bit(standard):
    o, d, acc, s, d0, state, style = standard
    dev = (o, d, _dev(s), _dev(d0), _dev(acc))
    plain = GC._launch(state, style, *dev)
    ws, wd = (_dev(a) for a in sr.synthetic_maps(16))
    off = _launch(state, style, *dev, shadow_light(strength=0.0, resolution=16), ws, wd)
    assert int((off[3] > 0).sum()) > 300                             # the occlusion is reported, it just does not darken
    zero = torch.zeros_like(ws)
    empty = _launch(state, style, *dev, shadow_light(resolution=16, spheres=False), zero, zero)
    assert int((empty[3] != 0).sum()) == 0
    for got in (off, empty):
        for a, b in zip(got[:3], plain):
            assert _same(a, b)
    casters = _launch(state, style, *dev, shadow_light(resolution=16, spheres=True), zero, zero)      # the ball alone
    assert set(np.unique(casters[3].cpu().numpy())) == {0.0, 1.0} and not _same(casters[0], plain[0])
    assert _same(casters[1], plain[1]) and _same(casters[2], plain[2])


def test_null_shadow_out_and_argument_checks(standard):
    o, d, acc, s, d0, state, style = standard
    N = 300
    o, d = o[:N].contiguous(), d[:N].contiguous()
    acc, s, d0 = (_dev(a[:N]) for a in (acc, s, d0))
    lt = shadow_light(resolution=16)
    ws, wd = (_dev(a) for a in sr.synthetic_maps(16))
    full = _launch(state, style, o, d, s, d0, acc, lt, ws, wd)
    only = _launch(state, style, o, d, s, d0, acc, lt, ws, wd, shadow=False)
    assert only[3] is None and all(_same(a, b) for a, b in zip(only[:3], full[:3]))
    f = lib().pn_draw_colliders_shadowed
    img, cov, sh = acc.clone(), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    names = (("st", ptr(state)), ("style", C.byref(style)), ("o", ptr(o)), ("d", ptr(d)), ("N", N), ("t_min", 0.2), ("t_max", 12.0), ("bg", 1.0),
             ("s", ptr(s)), ("d0", ptr(d0)), ("img", ptr(img)), ("cov", ptr(cov)), ("ct", None), ("lt", lt), ("ws", ptr(ws)), ("wd", ptr(wd)),
             ("sh", ptr(sh)), ("stream", stream_ptr()))
    args = lambda **kw: [kw.get(k, v) for k, v in names]   # noqa: E731

    def light(**kw):
        bad = ShadowLight.from_buffer_copy(bytes(lt))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(bad, k)[v[0]] = v[1]
            else:
                setattr(bad, k, v)
        return bad
    assert f(*args()) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(lt=light(S=1)), dict(lt=light(S=4097)), dict(lt=light(S=0)), dict(lt=light(S=-16)),
                dict(lt=light(c=(0, nan))), dict(lt=light(L=(2, inf))), dict(lt=light(U=(1, nan))), dict(lt=light(V=(0, -inf))), dict(lt=light(half=nan)),
                dict(lt=light(D=inf)), dict(lt=light(bias=nan)), dict(lt=light(strength=nan)),
                dict(lt=light(strength=-0.01)), dict(lt=light(strength=1.01)),
                dict(ws=None), dict(wd=None),
                dict(img=ptr(ws)), dict(cov=ptr(wd)), dict(ct=ptr(ws)), dict(sh=ptr(wd.view(-1)[200:])),      # a map overlapping an output, also partly
                dict(sh=ptr(s)), dict(sh=ptr(cov)), dict(sh=ptr(img)),                                      # shadow_out aliasing an input / an output
                # pn_draw_colliders' own checks
                dict(st=None), dict(style=None), dict(o=None), dict(d=None), dict(s=None), dict(d0=None), dict(img=None), dict(img=ptr(o)),
                dict(t_max=0.2), dict(t_min=nan), dict(t_max=inf), dict(bg=nan), dict(N=(2 ** 31 - 1) // 3 + 1)):
        assert f(*args(**bad)) != 0, bad
    worse = GC._style()
    worse.ambient = nan
    assert f(*args(style=C.byref(worse))) != 0
    assert f(*args(N=0, o=None, d=None, s=None, d0=None, img=None, cov=None, sh=None, ws=None, wd=None)) == 0      # nothing to do, nothing launched
    assert f(*args(N=0, lt=light(S=1))) != 0                                                                      # ... but the light is still checked
    torch.cuda.synchronize()
    assert _same(img, full[0])   # the refused calls wrote nothing


# ---------------------------------------------------------------- the renderer, on the collider tests' small chair
RES, LIGHT = 32, (0.4, 1.0, 0.3)


@pytest.fixture(scope="module")
def chair(small_opt, small_cloud, ckpt):
    """One harness at rest: the light's rays rendered directly and the frame over 0 (no overlay), the frame with the overlay, the frame with shadows."""
    h = GC._harness(small_opt, small_cloud, ckpt, draw=False)
    lt = shadow_light(direction=LIGHT, resolution=RES, bound=h.opt["bound"], min_near=h.opt["min_near"])
    lo, ld = shadow_rays(lt, DEV)
    with torch.no_grad():
        direct = h.model.render_deformed(lo, ld, staged=True, bg_color=None, perturb=False, **h.render_kwargs())
    torch.cuda.synchronize()
    direct = {k: v.clone() for k, v in direct.items()}
    _, over0 = GC._render(h, bg_color=0)
    over0 = {k: _np(v) for k, v in over0.items()}
    h.draw_colliders(h.style)
    r, drawn = GC._render(h)
    drawn = {k: v.clone() for k, v in drawn.items()}
    h.cast_shadows(direction=LIGHT, resolution=RES)
    _, shad = GC._render(h, collect_stats=True)
    main_stats = dict(h.model.last_stats)
    shad = {k: v.clone() for k, v in shad.items()}
    return h, r, direct, over0, drawn, shad, main_stats


def test_render_with_shadows(chair):
    h, r, direct, over0, drawn, shad, main_stats = chair
    m = h.model
    assert set(shad) == set(drawn) | {"shadow"}
    # the map buffers: the light's rays through the existing render
    assert _same(m.shadow_ws, direct["weights_sum"]) and _same(m.shadow_depth_0, direct["depth_0"])
    assert int((m.shadow_ws > 0.5).sum()) > 20 and int((m.shadow_ws == 0).sum()) > 20
    assert bytes(m._shadows.light) == bytes(shadow_light(direction=LIGHT, resolution=RES, bound=h.opt["bound"], min_near=h.opt["min_near"]))
    # the frame's statistics stay the main frame's; the shadow slot has its own
    st = m.render_status(slot=m.SHADOW_SLOT)
    assert st["err"] == 0 and st["alive_at_exit"] == 0 and 0 < st["samples"] != main_stats["samples"]
    assert m.render_status(slot=0)["samples"] == main_stats["samples"]
    for k in ("weights_sum", "depth", "depth_0", "coverage", "collider_t"):
        assert _same(shad[k], drawn[k]), k
    sh = _np(shad["shadow"])
    got, base = _np(shad["image"]), _np(drawn["image"])
    assert np.array_equal(_bits(got[sh == 0]), _bits(base[sh == 0]))
    assert (got[sh > 0] <= base[sh > 0]).all() and (got[sh > 0] < base[sh > 0]).any()
    lt = _light_dict(m._shadows.light)
    ws, wd = _np(m.shadow_ws), _np(m.shadow_depth_0)
    args = (h.sim._colliders, GC._style_rgb(h.style), h.style.checker, h.style.checker_dim, h.style.ambient, _np(r["rays_o"]), _np(r["rays_d"]),
            h.opt["min_near"], 8.0 * h.opt["bound"], 1.0, over0["weights_sum"], over0["depth_0"], over0["image"])
    plain = (base, _np(drawn["coverage"]), _np(drawn["collider_t"]))
    r64, keep = _compare("small chair, floor + ball", (got, _np(shad["coverage"]), _np(shad["collider_t"]), sh), plain, args, lt, ws, wd)
    floor = r64.slot == 0
    dark, lit = floor & (sh > 0.5), floor & (sh == 0)
    ball_shadow = floor & (r64.occ_sph > 0)
    print(f"floor rays {int(floor.sum())}: shadow > 0.5 on {int(dark.sum())}, shadow == 0 on {int(lit.sum())}, in the ball's shadow {int(ball_shadow.sum())}; "
          f"ball rays {int((r64.slot == 1).sum())}, shadowed by the object {int(((r64.slot == 1) & (sh > 0)).sum())}")
    assert dark.any() and lit.any()


def test_light_along_a_coordinate_axis_renders_without_a_device_error(small_opt, small_cloud, ckpt):
    h = GC._harness(small_opt, small_cloud, ckpt, W=32)
    for axis in ((0, 1, 0), (1, 0, 0), (0, 0, -1)):
        h.cast_shadows(direction=axis, resolution=16)
        _, out = GC._render(h, collect_stats=True)       # a device error flag raises
        st = h.model.render_status(slot=h.model.SHADOW_SLOT)
        assert st["err"] == 0 and st["alive_at_exit"] == 0
        assert torch.isfinite(out["shadow"]).all() and torch.isfinite(out["image"]).all()
    assert int((h.model.shadow_ws > 0.5).sum()) > 5


def test_one_trip_render_finished_by_render_continue_equals_the_blocking_render(chair):
    h, r, direct, over0, drawn, shad, main_stats = chair
    m = h.model
    _, part = GC._render(h, async_trips=1, fused_from=-1)      # one trip as launches of its own: the fused launch would run the frame to its end
    assert m.render_status(slot=0)["alive_at_exit"] > 0
    assert m.render_status(slot=m.SHADOW_SLOT)["alive_at_exit"] > 0      # the shadow slot is unfinished as well
    assert not _same(part["image"], shad["image"]) and not _same(m.shadow_ws, direct["weights_sum"])
    with torch.no_grad():
        done = m.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1))
    torch.cuda.synchronize()
    assert m.last_stats["alive_at_exit"] == 0 and m.render_status(slot=m.SHADOW_SLOT)["alive_at_exit"] == 0
    assert _same(m.shadow_ws, direct["weights_sum"]) and _same(m.shadow_depth_0, direct["depth_0"])
    for k in ("image", "depth", "depth_0", "weights_sum", "coverage", "collider_t", "shadow"):
        assert _same(done[k], shad[k]), k
    # the main frame finished, the shadow pass not: the frame's continue still redraws the overlay over the finished map
    _, part = GC._render(h, async_trips=1, fused_from=-1)
    with torch.no_grad():
        m.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1))
        sh = m._shadows
        m.rund_cuda(sh.rays_o, sh.rays_d, bg_color=0, **dict(h.render_kwargs(), async_trips=1, fused_from=-1, frame_slot=m.SHADOW_SLOT,
                                                                    out_buffers=sh.out(), ray_tile_w=0, _shadow_pass=True))
        assert m.render_status(slot=0)["alive_at_exit"] == 0 and m.render_status(slot=m.SHADOW_SLOT)["alive_at_exit"] > 0
        done = m.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1))
    torch.cuda.synchronize()
    for k in ("image", "depth", "depth_0", "weights_sum", "coverage", "collider_t", "shadow"):
        assert _same(done[k], shad[k]), k


# ---------------------------------------------------------------- the harness forms
def test_captured_step_equals_the_eager_step_also_after_the_ball_moved(small_opt, small_cloud, ckpt):
    g = GC._harness(small_opt, small_cloud, ckpt).cast_shadows(direction=LIGHT, resolution=RES).capture(n_trips=8)
    keys = ("image", "coverage", "collider_t", "depth_0", "shadow")
    for moved in (False, True):
        for _ in range(2):
            g.step_graph()
            g.finish_graph_frame()
        g.synchronize()
        if moved:
            g.sim.set_collider(g.ids[1], centre=(-0.5, -0.2, 0.3), velocity=(0.0, 0.0, 0.0))
        dof = g.sim.dof.clone()
        out = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        got = {k: out[k].clone() for k in keys}
        maps = (g.model.shadow_ws.clone(), g.model.shadow_depth_0.clone())
        after = g.sim.dof.clone()
        g.sim.dof.copy_(dof)      # an eager step() at the state that frame was rendered from
        m = g.model
        m.p_def, m.IP_F, m.IP_dF = g.sim.get_IP_info()
        want = g.step(simulate=False)
        g.synchronize()
        for k in keys:
            assert _same(got[k], want[k]), (moved, k)
        assert _same(maps[0], m.shadow_ws) and _same(maps[1], m.shadow_depth_0)
        assert int((got["shadow"] > 0.5).sum()) > 0
        g.sim.dof.copy_(after)
        if moved:
            assert not _same(got["shadow"], first)      # the ball's shadow went with it, without a recapture
        first = got["shadow"]


def test_graph_captured_without_the_shadows_or_with_another_light_is_refused(small_opt, small_cloud, ckpt):
    h = GC._harness(small_opt, small_cloud, ckpt, W=32).capture(n_trips=8)
    h.step_graph()
    h.finish_graph_frame()
    h.cast_shadows(resolution=16)
    with pytest.raises(RuntimeError, match="captured before cast_shadows"):
        h.step_graph()
    h.capture(n_trips=8)
    out = h.step_graph()
    h.finish_graph_frame()
    assert "shadow" in out
    h.cast_shadows(direction=(0, 1, 0), resolution=16)
    with pytest.raises(RuntimeError, match="changed since the step graph was captured"):
        h.step_graph()
    h.hide_shadows()
    with pytest.raises(RuntimeError, match="changed since the step graph was captured"):
        h.step_graph()
    h.synchronize()


def test_pipelined_form_and_missing_overlay_raise(small_opt, small_cloud, ckpt):
    h = GC._harness(small_opt, small_cloud, ckpt, W=32, draw=False)
    with pytest.raises(RuntimeError, match="draw_colliders"):
        h.cast_shadows()
    h.draw_colliders(h.style).cast_shadows(resolution=16)
    with pytest.raises(RuntimeError, match="casts no shadows"):
        h.capture_pipelined(lanes=2, depth=2, n_trips=8)
    h.hide_colliders()      # clears the shadows too
    assert h.model.collider_overlay_key() is None and not h._shadows_set()


# ---------------------------------------------------------------- main_render --shadows
def test_main_render_casts_the_shadow_on_the_floor(tmp_path, small_cloud):
    from pienerf_amd import io, main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--unpin", "--floor", "-0.95",
            "--frames", "3", "--quiet", "--draw_colliders"]
    extra = ["--shadows", "--shadow_res", "64"]
    a = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "drawn")]))
    b = main_render.run(main_render.parser().parse_args(base + extra + ["--out", str(tmp_path / "shadowed")]))
    assert len(a) == len(b) == 3
    # the same frames through the same calls, for their 'shadow'
    args = main_render.parser().parse_args(base + extra + ["--out", str(tmp_path / "unused")])
    h = main_render.build_harness(args)
    main_render.configure_contact(h.sim, args)
    main_render.configure_overlay(h, args)
    pose = scene.orbit_pose(args.radius, args.azimuth, args.elevation)
    for pa, pb in zip(a, b):
        sh = h.step(pose=pose)["shadow"].reshape(48, 48).cpu().numpy()
        ia, ib = io.load_image(pa).numpy(), io.load_image(pb).numpy()
        assert np.array_equal(ia[sh == 0], ib[sh == 0])
        assert (ib <= ia).all() and (ib[sh > 0.5] < ia[sh > 0.5]).any()      # the floor is darker somewhere
        print(f"{int((sh > 0.5).sum())} pixels with shadow > 0.5, {int((sh == 0).sum())} with none")
