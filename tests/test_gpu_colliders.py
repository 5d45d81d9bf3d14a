"""The collider overlay on the GPU (csrc/pn_colliders.hip): the launch against the numpy restatement (tests/colliders_reference.py), the
renderer, the harness forms and main_render.

Comparison rule: rays the restatement flags as near a decision (in float32 or float64) are left out, at most 0.5 % of the rays; on every other ray the
hit slot matches and image / coverage / collider_t lie within 4 x the largest float32-versus-float64 difference of the restatement on those same rays —
a bar measured on the reference, never on the kernel.  Rays without a hit are compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import colliders_reference as cr
from pienerf_amd import scene
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from pienerf_amd.colliders import collider_style
from pienerf_amd.harness import SimRenderHarness
from pienerf_amd.nerf.utils import get_rays
from pienerf_amd.simulator import solver
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
S = cr.STANDARD
RGB = cr.default_rgb()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(cols, active=1):
    raw = solver.pack_contact_state(active, (0.5, 0.5, 0.5, 0.05), cols)
    return torch.frombuffer(bytearray(raw), dtype=torch.float64).to(DEV)


def _style(rgb=RGB, checker=S["checker"], checker_dim=S["checker_dim"], ambient=S["ambient"]):
    return collider_style(rgb=[tuple(c) for c in np.asarray(rgb, np.float64)], checker=checker, checker_dim=checker_dim, ambient=ambient)


def _style_rgb(style):
    return np.array([[style.rgb[k][j] for j in range(3)] for k in range(8)], np.float32)


def _look_at_rays(eye, W=S["W"], H=S["H"]):
    """get_rays (the device's) for a camera at `eye` looking at the origin, fx = 0.9 W: [N, 3] device tensors."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)   # down
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    r = get_rays(_dev(pose).unsqueeze(0), (0.9 * W, 0.9 * W, W / 2, H / 2), H, W, -1)
    return r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()


def _launch(state, style, o, d, s, d0, acc, t_min=S["t_min"], t_max=S["t_max"], bg=S["bg"], outputs=True):
    N = o.shape[0]
    image = acc.clone()
    cov = torch.full((N,), -7.0, dtype=torch.float32, device=DEV) if outputs else None
    ct = torch.full((N,), -7.0, dtype=torch.float32, device=DEV) if outputs else None
    check(lib().pn_draw_colliders(ptr(state), C.byref(style), ptr(o), ptr(d), N, t_min, t_max, bg, ptr(s), ptr(d0), ptr(image), ptr(cov), ptr(ct),
                                  stream_ptr()), "draw_colliders")
    torch.cuda.synchronize()
    return image, cov, ct


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit (a depth is NaN where the ray misses the object's box)."""
    return torch.equal(a.reshape(-1).contiguous().view(torch.int32), b.reshape(-1).contiguous().view(torch.int32))


def _finish(acc, s, bg):
    k = ((np.float32(1) - s) * np.float32(bg)).astype(np.float32)
    return (acc + k[:, None]).astype(np.float32)


def _compare(name, got, cols, rgb, checker, o, d, s, d0, acc, t_min, t_max, bg, checker_dim=S["checker_dim"], ambient=S["ambient"], max_flagged=0.005):
    """The comparison rule of this file's docstring; got = (image, coverage, collider_t) as numpy.  Returns the restatement's float64 evaluation."""
    image, cov, ct = got
    r32, r64, keep, bar, diff = cr.bars(cols, rgb, checker, checker_dim, ambient, o, d, t_min, t_max, bg, s, d0, acc)
    N = o.shape[0]
    assert (~keep).sum() <= max_flagged * N, (name, int((~keep).sum()), N)
    hit = r64.slot >= 0
    assert np.array_equal(np.isfinite(ct)[keep], hit[keep]), name
    assert (np.isposinf(ct) | np.isfinite(ct)).all()
    err = {"image": np.abs(image[keep].astype(np.float64) - r64.image[keep]).max(initial=0.0),
           "coverage": np.abs(cov[keep].astype(np.float64) - r64.coverage[keep]).max(initial=0.0),
           "t": np.abs(ct[keep & hit].astype(np.float64) - r64.t[keep & hit]).max(initial=0.0)}
    ratio = {k: (err[k] / bar[k] if bar[k] > 0 else (0.0 if err[k] == 0 else float("inf"))) for k in err}
    print(f"{name}: N {N}, {int((~keep).sum())} rays near a decision, {int(hit.sum())} hits ({np.bincount(r64.slot[hit], minlength=8).tolist()}), "
          f"float32-vs-float64 restatement {diff}, kernel-vs-float64 {err}, worst share of the bar {ratio}")
    for k in err:
        assert err[k] <= bar[k], (name, k, err[k], bar[k])
    # rays without a hit: the frame epilogue's own bits
    miss = ~np.isfinite(ct)
    assert np.array_equal(_bits(image[miss]), _bits(_finish(acc[miss], s[miss], bg))), name
    assert np.array_equal(_bits(cov[miss]), _bits(s[miss])), name
    return r64, keep


CASES = {
    # name: (colliders, eye, first ray, number of rays (None: all), active)
    "standard": (cr.standard_scene, S["eye"], 0, None, 1),
    "one_ray": (cr.standard_scene, S["eye"], 1500, 1, 1),
    "partial_workgroup": (cr.standard_scene, S["eye"], 1000, 257, 1),
    "slot7_only_inactive_state": (lambda: [None] * 7 + [cr.sphere((0.0, 0.0, 0.9), 0.5)], S["eye"], 0, None, 0),
    "tilted_plane": (lambda: cr.slots(cr.plane((0.0, -0.95, 0.0), (0.2, 1.0, 0.0))), S["eye"], 0, None, 1),
    "eye_inside_the_sphere": (lambda: cr.slots(cr.sphere((0.0, 0.0, 0.9), 0.5)), (0.1, 0.05, 1.0), 0, None, 1),
}


@pytest.fixture(scope="module")
def rays():
    return {eye: _look_at_rays(eye) for eye in {c[1] for c in CASES.values()}}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_equals_the_restatement(name, rays):
    make, eye, first, count, active = CASES[name]
    cols = make()
    o, d = rays[eye]
    n_all = o.shape[0]
    acc, s, d0 = cr.standard_inputs(n_all)
    sl = slice(first, n_all if count is None else first + count)
    o, d = o[sl].contiguous(), d[sl].contiguous()
    acc, s, d0 = acc[sl], s[sl], d0[sl]
    got = _launch(_state(cols, active), _style(), o, d, _dev(s), _dev(d0), _dev(acc))
    got = tuple(t.cpu().numpy() for t in got)
    r64, keep = _compare(name, got, cols, RGB, S["checker"], o.cpu().numpy(), d.cpu().numpy(), s, d0, acc, S["t_min"], S["t_max"], S["bg"])
    hit = r64.slot >= 0
    if name == "standard":
        assert (np.bincount(r64.slot[hit], minlength=8)[:3] > 300).all() and 0.3 < r64.front[hit].mean() < 0.7 and (~hit).sum() > 50
        assert (np.abs(s - 0.0) == 0).mean() > 0.15 and (s == 1).mean() > 0.15
    if name == "slot7_only_inactive_state":
        assert hit.sum() > 300 and (r64.slot[hit] == 7).all()
    if name == "tilted_plane":
        assert hit.sum() > 1000 and 100 < r64.parity[hit].sum() < hit.sum() - 100 and (r64.coverage[hit] < 1 - 1e-3).any()   # both parities, and the fade
    if name == "eye_inside_the_sphere":
        assert hit.all()   # every ray leaves through the wall: the second root


def test_null_outputs_and_argument_checks(rays):
    o, d = rays[S["eye"]]
    N = 300
    o, d = o[:N].contiguous(), d[:N].contiguous()
    acc, s, d0 = (_dev(a) for a in cr.standard_inputs(N))
    st, style = _state(cr.standard_scene()), _style()
    full = _launch(st, style, o, d, s, d0, acc)
    only, none_c, none_t = _launch(st, style, o, d, s, d0, acc, outputs=False)
    assert none_c is None and none_t is None and torch.equal(only, full[0])
    f = lib().pn_draw_colliders
    img = acc.clone()
    args = lambda **kw: [kw.get(k, v) for k, v in (("st", ptr(st)), ("style", C.byref(style)), ("o", ptr(o)), ("d", ptr(d)), ("N", N), ("t_min", 0.2),   # noqa: E731
                                                    ("t_max", 12.0), ("bg", 1.0), ("s", ptr(s)), ("d0", ptr(d0)), ("img", ptr(img)), ("cov", None),
                                                    ("ct", None), ("stream", stream_ptr()))]
    assert f(*args()) == 0
    for bad in (dict(st=None), dict(style=None), dict(o=None), dict(d=None), dict(s=None), dict(d0=None), dict(img=None),
                dict(img=ptr(o)), dict(img=ptr(acc.view(-1)[3:]), o=ptr(acc)),                 # image aliasing an input, also partly
                dict(t_max=0.2), dict(t_max=0.1), dict(t_min=float("nan")), dict(t_max=float("inf")), dict(bg=float("nan")),
                dict(N=(2 ** 31 - 1) // 3 + 1)):
        assert f(*args(**bad)) != 0, bad
    worse = _style()
    worse.ambient = float("nan")
    assert f(*args(style=C.byref(worse))) != 0
    assert f(*args(N=0, o=None, d=None, s=None, d0=None, img=None)) == 0      # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(img, full[0])   # the refused calls wrote nothing


# ---------------------------------------------------------------- the renderer, on the contact tests' small chair
FLOOR_Y, BALL = -0.95, ((0.2, -0.3, 0.8), 0.3)


def _harness(small_opt, small_cloud, ckpt, W=64, draw=True, **opt):
    h = SimRenderHarness(dict(small_opt, W=W, H=W, **opt), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_contact()
    h.ids = [h.sim.add_plane((0.0, FLOOR_Y, 0.0), (0.0, 1.0, 0.0)), h.sim.add_sphere(*BALL)]
    h.style = collider_style(types=h.sim.collider_types(), checker=0.2)
    if draw:
        h.draw_colliders(h.style)
    return h


def _render(h, **kw):
    r = get_rays(torch.from_numpy(np.asarray(h.pose, np.float32)).unsqueeze(0).to(DEV), h.intrinsics, h.opt["H"], h.opt["W"], -1)
    args = dict(h.render_kwargs(), **kw)
    bg = args.pop("bg_color", None)
    with torch.no_grad():
        out = h.model.render_deformed(r["rays_o"], r["rays_d"], staged=True, bg_color=bg, perturb=False, **args)
    torch.cuda.synchronize()
    return r, out


def _np(t):
    a = t.detach().cpu().numpy()
    return a.reshape(-1, 3) if a.ndim >= 2 and a.shape[-1] == 3 else a.reshape(-1)


@pytest.fixture(scope="module")
def chair(small_opt, small_cloud, ckpt):
    """One harness, rendered without the overlay (over the default background and over 0) and with it."""
    h = _harness(small_opt, small_cloud, ckpt, draw=False)
    _, plain = _render(h)
    _, over0 = _render(h, bg_color=0)
    h.draw_colliders(h.style)
    r, drawn = _render(h)
    return h, r, {k: _np(v) for k, v in plain.items()}, {k: _np(v) for k, v in over0.items()}, drawn


def test_render_with_the_overlay(chair):
    h, r, plain, over0, drawn = chair
    got = {k: _np(v) for k, v in drawn.items()}
    assert set(got) == {"image", "depth", "depth_0", "weights_sum", "coverage", "collider_t"}
    for k in ("weights_sum", "depth", "depth_0"):      # the object's own, untouched
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
        assert np.array_equal(_bits(got[k]), _bits(over0[k])), k
    miss = np.isposinf(got["collider_t"])
    hit = ~miss
    assert miss.sum() > 500 and hit.sum() > 500
    assert np.array_equal(_bits(got["image"][miss]), _bits(plain["image"][miss]))      # bit for bit where no collider is seen
    assert np.array_equal(_bits(got["coverage"][miss]), _bits(plain["weights_sum"][miss]))
    t_max = 8.0 * h.opt["bound"]
    r64, keep = _compare("small chair, floor + sphere", (got["image"], got["coverage"], got["collider_t"]), h.sim._colliders, _style_rgb(h.style),
                         h.style.checker, _np(r["rays_o"]), _np(r["rays_d"]), over0["weights_sum"], over0["depth_0"], over0["image"],
                         h.opt["min_near"], t_max, 1.0, checker_dim=h.style.checker_dim, ambient=h.style.ambient)
    seen = r64.slot >= 0
    assert (r64.slot[seen] == 0).sum() > 300 and (r64.slot[seen] == 1).sum() > 30
    obj = over0["weights_sum"] > 0.5
    print(f"object rays with a collider in front: {int(r64.front[seen & obj].sum())}, behind: {int((~r64.front[seen & obj]).sum())}")
    assert (~r64.front[seen & obj]).any()    # the floor seen through / behind the object


def test_fixed_trip_render_finished_by_render_continue_equals_the_blocking_render(chair):
    h, r, plain, over0, drawn = chair
    _, part = _render(h, async_trips=1, fused_from=-1)      # one trip as launches of its own: the fused launch would run the frame to its end
    st = h.model.render_status()
    assert st["alive_at_exit"] > 0       # one trip is not enough: the frame is unfinished, its overlay drawn over a partial composite
    assert not _same(part["image"], drawn["image"])
    with torch.no_grad():
        done = h.model.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1))
    torch.cuda.synchronize()
    assert h.model.last_stats["alive_at_exit"] == 0
    for k in ("image", "depth", "depth_0", "weights_sum", "coverage", "collider_t"):
        assert _same(done[k], drawn[k]), k


def test_out_buffers_receive_the_overlays_outputs(chair):
    h, r, plain, over0, drawn = chair
    N = h.opt["W"] * h.opt["H"]
    ob = {k: torch.empty((N, 3) if k == "image" else (N,), dtype=torch.float32, device=DEV)
          for k in ("image", "depth", "depth_0", "weights_sum", "coverage", "collider_t")}
    _, out = _render(h, out_buffers=ob)
    assert out["coverage"].data_ptr() == ob["coverage"].data_ptr() and out["collider_t"].data_ptr() == ob["collider_t"].data_ptr()
    for k in ob:
        assert _same(ob[k], drawn[k]), k
    del ob["coverage"], ob["collider_t"]
    _, out = _render(h, out_buffers=ob)      # absent from out_buffers: allocated
    assert torch.equal(out["coverage"], drawn["coverage"]) and torch.equal(out["collider_t"], drawn["collider_t"])


def test_tensor_background_is_blended_with_the_coverage(chair):
    h, r, plain, over0, drawn = chair
    colour = torch.tensor([0.1, 0.5, 0.9], device=DEV)
    _, out = _render(h, bg_color=colour)
    _, zero = _render(h, bg_color=0)
    want = zero["image"] + (1 - zero["coverage"]).unsqueeze(-1) * colour
    assert torch.equal(out["image"].reshape(-1, 3), want.reshape(-1, 3)) and torch.equal(out["coverage"], drawn["coverage"])
    full = out["coverage"] == 1
    assert int(full.sum()) > 300 and torch.equal(out["image"].reshape(-1, 3)[full], zero["image"].reshape(-1, 3)[full])


def test_other_renders_refuse_while_an_overlay_is_set(chair):
    h, r, plain, over0, drawn = chair
    m = h.model
    for call in (lambda: m.rund_cuda(r["rays_o"], r["rays_d"], perturb=True, **h.render_kwargs()), lambda: m.run_cuda(r["rays_o"], r["rays_d"]),
                 lambda: m.render(r["rays_o"], r["rays_d"]), lambda: m.run(r["rays_o"], r["rays_d"])):
        with pytest.raises(RuntimeError, match="only the deformed path"):
            call()


def test_background_model_is_blended_with_the_coverage(small_opt, small_cloud):
    import test_background_host as BH
    R = 32.0
    h = _harness(small_opt, small_cloud, BH.bg_checkpoint(), draw=False, bg_radius=R)
    _, plain = _render(h)
    h.draw_colliders(h.style)
    r, out = _render(h)
    img, cov, ct, ws = _np(out["image"]), _np(out["coverage"]), _np(out["collider_t"]), _np(out["weights_sum"])
    bgcol = _np(plain["image"])      # where the ray met nothing, the overlay-free frame is the model's colour
    empty = _np(plain["weights_sum"]) == 0
    floor_only = empty & (cov == 1)
    assert floor_only.sum() > 300 and np.abs(bgcol[floor_only] - img[floor_only]).max() > 0.05
    t_max = 8.0 * h.opt["bound"]
    args = (h.sim._colliders, _style_rgb(h.style), h.style.checker, h.style.checker_dim, h.style.ambient, _np(r["rays_o"]), _np(r["rays_d"]),
            h.opt["min_near"], t_max, 0.0, ws, _np(out["depth_0"]), np.zeros_like(img))
    r32, r64, keep, bar, diff = cr.bars(*args)
    m = floor_only & keep
    assert np.abs(img[m] - r64.image[m]).max() <= bar["image"]      # fully covered: the collider's colour and none of the background's
    fade = empty & keep & (cov > 0) & (cov < 1)
    assert fade.sum() > 50
    want = r64.image[fade] + (1.0 - r64.coverage[fade])[:, None] * bgcol[fade]
    # the restatement's own bars on the two terms (the collider over 0; the coverage times the background's colour, at most 1) + the blend's two roundings
    assert np.abs(img[fade] - want).max() <= bar["image"] + bar["coverage"] * float(bgcol.max()) + 4 * np.finfo(np.float32).eps
    miss = np.isposinf(ct)
    assert np.array_equal(_bits(img[miss]), _bits(bgcol[miss]))


# ---------------------------------------------------------------- the harness forms
def test_captured_step_follows_a_moved_collider_without_recapture(small_opt, small_cloud, ckpt):
    g = _harness(small_opt, small_cloud, ckpt).capture(n_trips=8)
    for _ in range(2):
        before = g.step_graph()
        g.finish_graph_frame()
    g.synchronize()
    t_before = before["collider_t"].clone()
    g.sim.set_collider(g.ids[1], centre=(-0.5, 0.2, 0.6), velocity=(0.0, 0.0, 0.0))
    dof = g.sim.dof.clone()
    out = g.step_graph()
    g.finish_graph_frame()
    g.synchronize()
    got = {k: out[k].clone() for k in ("image", "coverage", "collider_t", "depth_0")}
    assert not torch.equal(got["collider_t"], t_before)          # the sphere is drawn where it was moved to
    moved = cr.draw(g.sim._colliders, _style_rgb(g.style), 0.0, 1.0, 0.3, _np(out["rays_o"]), _np(out["rays_d"]), g.opt["min_near"], 8.0, 1.0,
                    np.zeros(got["coverage"].numel(), np.float32), np.zeros(got["coverage"].numel(), np.float32),
                    np.zeros((got["coverage"].numel(), 3), np.float32), dtype=np.float64)
    assert ((moved.slot == 1) & np.isfinite(_np(got["collider_t"]))).sum() > 30
    # an eager step() at the state that frame was rendered from
    g.sim.dof.copy_(dof)
    m = g.model
    m.p_def, m.IP_F, m.IP_dF = g.sim.get_IP_info()
    want = g.step(simulate=False)
    g.synchronize()
    for k in got:
        assert _same(got[k], want[k]), k


def test_graph_captured_before_draw_colliders_is_refused(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, W=32, draw=False).capture(n_trips=8)
    h.step_graph()
    h.finish_graph_frame()
    h.draw_colliders()
    with pytest.raises(RuntimeError, match="captured before draw_colliders"):
        h.step_graph()
    h.hide_colliders()
    h.step_graph()
    h.finish_graph_frame()
    h.synchronize()


def test_multi_rank_and_staged_forms_raise_while_an_overlay_is_set(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, W=32)
    for call in (lambda: h.capture_frame_parallel(lanes=2, n_trips=8), lambda: h.capture_tile_parallel(), lambda: h.capture_staged(batch=256)):
        with pytest.raises(RuntimeError, match="does not draw the colliders"):
            call()
    with pytest.raises(ValueError, match="enable_contact"):
        SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).draw_colliders()


def test_pipelined_frames_draw_the_colliders(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt, W=32)
    frames = [e.to_host(e.step())["image"].copy() for _ in range(5)]
    e.synchronize()
    p = _harness(small_opt, small_cloud, ckpt, W=32).capture_pipelined(lanes=2, depth=2, n_trips=8)
    got = []
    for _ in range(len(frames)):
        got += [(i, res["image"].copy()) for i, res in p.step_pipelined()]
    got += [(i, res["image"].copy()) for i, res in p.drain_pipeline()]
    assert [i for i, _ in got] == list(range(len(frames)))
    for f, (_, img) in enumerate(got):
        assert np.abs(img - frames[f]).max() < 1e-5, f
    plain = _harness(small_opt, small_cloud, ckpt, W=32, draw=False)
    assert np.abs(plain.to_host(plain.step())["image"] - frames[0]).max() > 0.1      # the colliders are in those frames
    late = _harness(small_opt, small_cloud, ckpt, W=32, draw=False).capture_pipelined(lanes=2, depth=2, n_trips=8)
    late.step_pipelined()
    late.drain_pipeline()
    late.draw_colliders()
    with pytest.raises(RuntimeError, match="captured before draw_colliders"):
        late.step_pipelined()


# ---------------------------------------------------------------- main_render --draw_colliders
def test_main_render_draws_the_floor(tmp_path, small_cloud):
    from pienerf_amd import io, main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--unpin", "--floor", "-0.95",
            "--frames", "3", "--quiet"]
    a = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "plain")]))
    b = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "drawn"), "--draw_colliders"]))
    assert len(a) == len(b) == 3
    for pa, pb in zip(a, b):
        ia, ib = io.load_image(pa).numpy(), io.load_image(pb).numpy()
        rows = np.nonzero((ia != 1.0).any(axis=(1, 2)))[0]     # the object's silhouette on the white background
        assert rows.size > 0
        top = rows.min()
        assert top > 2 and np.array_equal(ia[:top], ib[:top])   # above the silhouette: no collider in sight, the same pixels
        assert (ia[40:] != ib[40:]).any(axis=2).mean() > 0.5     # the lower rows show the floor
