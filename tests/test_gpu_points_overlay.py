"""The point overlay on the GPU (csrc/pn_points_overlay.hip): the launch pair against the numpy restatement of the header's law
(tests/points_overlay_reference.py) bit for bit — image, point_id, point_t — then the renderer, the harness forms and main_render.

Every test point is built from a pixel (points_overlay_reference.point_at), distinct points' distances differ by at least 1e-3 relative (exact
duplicates aside) and stay at least 1e-2 away from every depth-test threshold, so no decision is near a rounding and no case is excluded.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import points_overlay_reference as pr
from pienerf_amd import scene
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from pienerf_amd.harness import SimRenderHarness
from pienerf_amd.nerf.utils import get_rays
from pienerf_amd.points_overlay import key_buffer, point_style
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
W, H, N = pr.W, pr.H, pr.W * pr.H


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cstyle(st):
    """The restatement's style dict as the launch's by-value struct."""
    mode = next(k for k, v in pr.MODES.items() if v == st["mode"])
    return point_style(radius=st["radius"], mode=mode, xray=st["xray"], rgb=st["rgb"], ramp=st["ramp"], lo=float(st["lo"]), hi=float(st["hi"]),
                       alpha=float(st["alpha"]), hidden_alpha=float(st["hidden_alpha"]), bias=float(st["bias"]),
                       marker_radius=float(st["marker_radius"]), marker_thickness=float(st["marker_thickness"]))


def _drag_dev(drag):
    if drag is None:
        return None
    raw = np.zeros(5, np.float64)
    raw[:1].view(np.int32)[:] = (drag["vid"], drag["active"])
    raw[1:4] = drag["target"]
    raw[4] = 1.0
    return _dev(raw)


def _launch(pos, F, values, s, d0, ct, drag, st, image, keys=None, outputs=True, pose=pr.POSE, intr=pr.INTR, Wd=W, Hd=H):
    """pn_draw_points on device copies; returns (image, point_id, point_t, keys) as numpy (absent outputs None)."""
    n = 0 if pos is None else pos.shape[0]
    Nd = Wd * Hd
    img = _dev(np.asarray(image, np.float32).reshape(Nd, 3))
    pid = torch.full((Nd,), -7, dtype=torch.int32, device=DEV) if outputs else None
    pt = torch.full((Nd,), -7.0, dtype=torch.float32, device=DEV) if outputs else None
    keys = key_buffer(Wd, Hd, DEV) if keys is None else keys
    hold = [_dev(pos), _dev(F), _dev(values), _dev(np.asarray(pose, np.float32).reshape(16)), _dev(s), _dev(d0), _dev(ct), _drag_dev(drag)]
    check(lib().pn_draw_points(ptr(hold[0]), ptr(hold[1]), ptr(hold[2]), n, ptr(hold[3]), (C.c_float * 4)(*intr), Wd, Hd, pr.T_MIN, ptr(hold[4]),
                               ptr(hold[5]), ptr(hold[6]), ptr(hold[7]), ptr(keys), _cstyle(st), ptr(img), ptr(pid), ptr(pt), stream_ptr()), "draw_points")
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return cpu(img), cpu(pid), cpu(pt), keys


def _equal(name, got, want):
    img, pid, pt = got[:3]
    assert np.array_equal(pid, want[1]), name
    assert np.array_equal(_bits(pt), _bits(want[2])), name
    assert np.array_equal(_bits(img), _bits(want[0])), name


@pytest.fixture(scope="module")
def frame():
    return pr.frame_inputs()


CASES = {
    # name: (n, style, with collider_t)
    "one_point": (1, dict(radius=0, xray=True), False),
    "past_one_wave_r0_xray": (70, dict(radius=0, xray=True), True),
    "r2_occluded_hidden0": (70, dict(radius=2), True),
    "r2_occluded_hidden_half_no_colliders": (70, dict(radius=2, hidden_alpha=0.5), False),
    "r8_occluded_hidden_half_alpha06": (70, dict(radius=8, hidden_alpha=0.5, alpha=0.6), True),
    "r2_strain_alpha06": (70, dict(radius=2, mode="strain", lo=0.0, hi=0.4, alpha=0.6, xray=True), False),
    "r0_volume_occluded": (70, dict(radius=0, mode="volume", lo=-0.3, hi=0.3), True),
    "r2_values_hidden_half": (70, dict(radius=2, mode="values", lo=-1.0, hi=1.0, hidden_alpha=0.5), True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_equals_the_restatement(name, frame):
    n, kw, with_ct = CASES[name]
    image, s, d0, ct = frame
    ct = ct if with_ct else None
    pos = pr.cloud(n, borders=n > 1, duplicates=n > 1, rejects=True)
    F = pr.gradients(pos.shape[0])
    values = np.random.default_rng(3).uniform(-1.5, 1.5, pos.shape[0]).astype(np.float32)
    st = pr.style(**kw)
    want = pr.draw(pos, F, values, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, ct, None, st, image)
    got = _launch(pos, F, values, s, d0, ct, None, st, image)
    _equal(name, got, want)
    drawn = want[1] >= 0
    print(f"{name}: {pos.shape[0]} points, {int(drawn.sum())} of {N} pixels drawn, {len(set(want[1][drawn].tolist()))} distinct points")
    assert drawn.any() and np.array_equal(_bits(got[0][~drawn]), _bits(image[~drawn]))      # an undrawn pixel keeps its bits
    if n > 1:
        m = pos.shape[0]
        assert not set(want[1][drawn].tolist()) & {m - 9, m - 8, m - 7, m - 6, m - 2, m - 1}      # duplicates, behind, too near, non-finite
        if not st["xray"] and st["radius"] <= 2:      # (at radius 8 every pixel's nearest point is in front of everything)
            x = pr.draw(pos, F, values, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, ct, None, dict(st, xray=True), image)
            assert (x[1] >= 0).sum() > 0 and not np.array_equal(_bits(x[0]), _bits(want[0]))      # the depth test hides or dims something


def test_contention_on_one_pixel_and_permutation(frame):
    """4096 points on one pixel with distinct t: the nearest wins; the same points permuted, ids mapped back, give the same bits."""
    image, s, d0, ct = frame
    n = 4096
    rng = np.random.default_rng(11)
    ts = 0.3 * 1.00101 ** np.arange(n)
    rng.shuffle(ts)
    pos = np.stack([pr.point_at(pr.POSE, pr.INTR, 13, 6, t, *rng.uniform(-0.3, 0.3, 2)) for t in ts])
    st = pr.style(radius=1, xray=True, alpha=0.6)
    want = pr.draw(pos, None, None, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, None, None, st, image)
    got = _launch(pos, None, None, s, d0, None, None, st, image)
    _equal("contention", got, want)
    assert (got[1] >= 0).sum() == 5 and set(got[1][got[1] >= 0].tolist()) == {int(np.argmin(ts))}
    perm = rng.permutation(n)
    again = _launch(pos[perm], None, None, s, d0, None, None, st, image)
    back = np.where(again[1] >= 0, perm[np.maximum(again[1], 0)], -1)
    assert np.array_equal(back, got[1]) and np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(_bits(again[2]), _bits(got[2]))


def test_key_buffer_cleans_itself(frame):
    image, s, d0, ct = frame
    st = pr.style(radius=2)
    a, b = pr.cloud(70, seed=1), pr.cloud(40, seed=7)
    first = _launch(a, None, None, s, d0, ct, None, st, image)
    keys = first[3]
    assert lib().pn_points_keys_bytes(W, H) == keys.numel() * 8
    assert bool((keys == -1).all())                                   # all-empty again
    second = _launch(b, None, None, s, d0, ct, None, st, image, keys=keys)
    _equal("second call", second, pr.draw(b, None, None, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, ct, None, st, image))
    assert bool((keys == -1).all())


def test_null_optional_outputs_change_nothing_else(frame):
    image, s, d0, ct = frame
    st = pr.style(radius=2, hidden_alpha=0.5)
    pos = pr.cloud(70)
    full = _launch(pos, None, None, s, d0, ct, None, st, image)
    only = _launch(pos, None, None, s, d0, ct, None, st, image, outputs=False)
    assert only[1] is None and only[2] is None and np.array_equal(_bits(only[0]), _bits(full[0])) and bool((only[3] == -1).all())


def test_argument_checks_and_the_empty_call(frame):
    image, s, d0, ct = frame
    pos, F, vals = _dev(pr.cloud(20)), _dev(pr.gradients(40)), _dev(np.zeros(40, np.float32))
    n = pos.shape[0]
    pose, sd, dd, cd = _dev(pr.POSE.reshape(16)), _dev(s), _dev(d0), _dev(ct)
    img, keys = _dev(image), key_buffer(W, H, DEV)
    pid, pt = torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.float32, device=DEV)
    drag = _drag_dev(dict(vid=0, active=0, target=(0, 0, 0)))
    intr = (C.c_float * 4)(*pr.INTR)
    f = lib().pn_draw_points
    base = dict(pos=ptr(pos), F=ptr(F), values=ptr(vals), n=n, pose=ptr(pose), intr=intr, W=W, H=H, t_min=pr.T_MIN, s=ptr(sd), d0=ptr(dd), ct=ptr(cd),
                drag=None, keys=ptr(keys), style=point_style(radius=1), img=ptr(img), pid=ptr(pid), pt=ptr(pt), stream=stream_ptr())
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]   # noqa: E731
    before = img.clone()
    bad_styles = []
    for field, value in (("radius", -1), ("radius", 9), ("mode", 4), ("alpha", 1.5), ("alpha", -0.5), ("hidden_alpha", 2.0), ("hidden_alpha", float("nan")),
                         ("bias", float("inf")), ("lo", float("nan")), ("marker_radius", float("nan")), ("marker_thickness", float("inf"))):
        st = point_style(radius=1)
        setattr(st, field, value)
        bad_styles.append(st)
    for j in (0, 2):
        st = point_style(radius=1)
        st.rgb[j] = float("nan")
        bad_styles.append(st)
        st = point_style(radius=1)
        st.ramp[j][1] = float("inf")
        bad_styles.append(st)
    for mode in ("strain", "volume", "values"):
        st = point_style(mode=mode)
        st.lo, st.hi = 0.5, 0.5                                       # hi <= lo in a ramp mode
        bad_styles.append(st)
    for st in bad_styles:
        assert f(*args(style=st)) == 1, bytes(st)
    for bad in (dict(pos=None), dict(pose=None), dict(intr=None), dict(s=None), dict(d0=None), dict(keys=None), dict(img=None),
                dict(img=ptr(pos)), dict(img=ptr(sd)), dict(pid=ptr(dd)), dict(pt=ptr(cd)), dict(keys=ptr(pose)), dict(pid=ptr(img)), dict(pt=ptr(pid)),
                dict(keys=ptr(img)), dict(img=ptr(F)), dict(pt=ptr(vals)), dict(pid=ptr(drag), drag=ptr(drag)),
                dict(style=point_style(mode="strain"), F=None), dict(style=point_style(mode="volume"), F=None),
                dict(style=point_style(mode="values"), values=None),
                dict(n=2 ** 31), dict(n=-1), dict(W=2 ** 16, H=2 ** 15), dict(W=0), dict(H=-3), dict(t_min=float("nan"))):
        assert f(*args(**bad)) == 1, bad
    assert f(*args(style=point_style(mode="strain"))) == 0 and f(*args(style=point_style(mode="values"))) == 0      # ... and with F / values they run
    torch.cuda.synchronize()
    img.copy_(before)
    pid.fill_(-7)
    # n == 0 without a drag: success, nothing launched — the outputs are not even written
    assert f(*args(n=0, pos=None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(img, before) and bool((pid == -7).all()) and bool((keys == -1).all())
    # n == 0 with an inactive drag: the resolve launch alone, nothing painted
    assert f(*args(n=0, pos=None, drag=ptr(drag))) == 0
    torch.cuda.synchronize()
    assert torch.equal(img, before) and bool((pid == -1).all())


MARKERS = {
    # name: (vid, active, target as (px, py, t) through point_at, marker radius, thickness)
    "inactive": (3, 0, (15, 9, 2.0), 3.0, 1.5),
    "both_ends_on_screen": (3, 1, (18, 11, 2.0), 3.0, 1.5),
    "reference_sizes": (5, 1, (4, 12, 1.5), 10.0, 5.0),
    "target_behind_the_camera": (3, 1, (15, 9, -2.0), 3.0, 1.5),
    "handle_wholly_off_screen": (None, 1, (-40, -30, 2.0), 3.0, 1.5),
    "vid_out_of_range": (10 ** 6, 1, (15, 9, 2.0), 3.0, 1.5),
}


@pytest.mark.parametrize("name", list(MARKERS))
def test_markers_equal_the_restatement(name, frame):
    image, s, d0, ct = frame
    vid, active, (tx, ty, tt), mr, mt = MARKERS[name]
    pos = pr.cloud(30)
    if vid is None:      # the picked point off-screen too
        pos = np.concatenate([pos, pr.point_at(pr.POSE, pr.INTR, -60, -20, 2.1)[None]])
        vid = pos.shape[0] - 1
    drag = dict(vid=vid, active=active, target=pr.point_at(pr.POSE, pr.INTR, tx, ty, tt).astype(np.float64) + 1e-9)
    st = pr.style(radius=1, marker_radius=mr, marker_thickness=mt)
    want = pr.draw(pos, None, None, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, ct, drag, st, image)
    plain = pr.draw(pos, None, None, pr.POSE, pr.INTR, W, H, pr.T_MIN, s, d0, ct, None, st, image)
    got = _launch(pos, None, None, s, d0, ct, drag, st, image)
    _equal(name, got, want)
    assert np.array_equal(want[1], plain[1])                          # markers do not write point_id
    red = (want[0] == np.array([1, 0, 0], np.float32)).all(axis=1).sum()
    blue_more = (want[0] == np.array([0, 0, 1], np.float32)).all(axis=1).sum() - (plain[0] == np.array([0, 0, 1], np.float32)).all(axis=1).sum()
    changed = (_bits(want[0]) != _bits(plain[0])).any(axis=1).sum()
    print(f"{name}: {int(red)} red, {int(blue_more)} more blue, {int(changed)} pixels differ from the frame without markers")
    if name in ("inactive", "handle_wholly_off_screen"):
        assert changed == 0
    if name == "both_ends_on_screen":
        assert red > 3 and blue_more > 3 and changed > red + blue_more      # two discs (partly under the line) and a line between them
    if name == "target_behind_the_camera":
        assert red > 10 and changed == red - ((plain[0] == np.array([1, 0, 0], np.float32)).all(axis=1).sum())      # the red disc alone: no blue disc, no line
    if name == "vid_out_of_range":
        assert red == 0 and blue_more > 10


# ---------------------------------------------------------------- the renderer and the harness, on the contact tests' small chair
def _harness(small_opt, small_cloud, ckpt, W=48, draw=True, drag=False, style=None, **opt):
    h = SimRenderHarness(dict(small_opt, W=W, H=W, **opt), cloud=small_cloud, ckpt=ckpt, device=DEV)
    if drag:
        h.enable_drag()
    h.pstyle = point_style(radius=1, hidden_alpha=0.25) if style is None else style
    if draw:
        h.draw_points(h.pstyle)
    return h


def _np(t):
    a = t.detach().cpu().numpy()
    return a.reshape(-1, 3) if a.ndim >= 2 and a.shape[-1] == 3 else a.reshape(-1)


def _rstyle(st):
    """A PointStyle as the restatement's dict."""
    mode = next(k for k, v in pr.MODES.items() if v == int(st.mode))
    return pr.style(radius=st.radius, mode=mode, xray=bool(st.xray), rgb=tuple(st.rgb), ramp=[tuple(r) for r in st.ramp], lo=st.lo, hi=st.hi, alpha=st.alpha,
                    hidden_alpha=st.hidden_alpha, bias=st.bias, marker_radius=st.marker_radius, marker_thickness=st.marker_thickness)


def _restate(h, plain, st=None, drag=None, collider_t=None):
    """The law applied to the plain frame `plain` (a render without the point overlay) with the model's current integration-point state."""
    m, o = h.model, h.opt
    return pr.draw(_np(m.p_def.float()), _np(m.IP_F.float()).reshape(-1, 9), None, np.asarray(h.pose, np.float32), h.intrinsics, o["W"], o["H"], o["min_near"],
                   _np(plain["weights_sum"]), _np(plain["depth_0"]), collider_t, drag, _rstyle(h.pstyle if st is None else st), _np(plain["image"]))


def _render(h, **kw):
    pose = torch.from_numpy(np.asarray(h.pose, np.float32)).unsqueeze(0).to(DEV)
    r = get_rays(pose, h.intrinsics, h.opt["H"], h.opt["W"], -1)
    args = dict(h.render_kwargs(), point_pose=pose, **kw)
    with torch.no_grad():
        out = h.model.render_deformed(r["rays_o"], r["rays_d"], staged=True, bg_color=None, perturb=False, **args)
    torch.cuda.synchronize()
    return r, pose, out


@pytest.fixture(scope="module")
def chair(small_opt, small_cloud, ckpt):
    """One harness, stepped a few times under a force so that F is no identity, rendered without the overlay and with it."""
    h = _harness(small_opt, small_cloud, ckpt, draw=False)
    h.sim.update_force(h.sim.n_IP // 2, torch.tensor([300.0, 100.0, -200.0], dtype=torch.float64, device=DEV))
    for _ in range(4):
        h.step()
    h.synchronize()
    _, _, plain = _render(h)
    plain = {k: v.clone() for k, v in plain.items()}
    h.draw_points(h.pstyle)
    r, pose, drawn = _render(h)
    return h, r, pose, plain, drawn


def test_render_with_the_overlay(chair):
    h, r, pose, plain, drawn = chair
    assert set(drawn) == set(plain) | {"point_id", "point_t"}
    pid = _np(drawn["point_id"])
    for k in ("weights_sum", "depth", "depth_0"):
        assert np.array_equal(_bits(_np(drawn[k])), _bits(_np(plain[k]))), k
    off = pid < 0
    assert off.sum() > 200 and (~off).sum() > 200
    assert np.array_equal(_bits(_np(drawn["image"])[off]), _bits(_np(plain["image"])[off]))      # bit for bit wherever nothing was drawn
    want = _restate(h, plain)
    assert np.array_equal(pid, want[1]) and np.array_equal(_bits(_np(drawn["point_t"])), _bits(want[2]))
    assert np.array_equal(_bits(_np(drawn["image"])), _bits(want[0]))
    x = _restate(h, plain, st=point_style(radius=1, xray=True))
    assert ((x[1] >= 0) & (_bits(x[0]) != _bits(want[0])).any(axis=1)).sum() > 20      # points behind the chair's surface are dimmed, not painted full
    # the strain colouring, against the restatement as well
    h.draw_points(point_style(radius=2, mode="strain", lo=0.0, hi=0.05, xray=True))
    _, _, col = _render(h)
    want = _restate(h, plain, st=point_style(radius=2, mode="strain", lo=0.0, hi=0.05, xray=True))
    assert np.array_equal(_bits(_np(col["image"])), _bits(want[0])) and len(np.unique(_np(col["image"])[want[1] >= 0], axis=0)) > 10
    h.draw_points(h.pstyle)


def test_hide_points_restores_the_plain_frames(chair):
    h, r, pose, plain, drawn = chair
    h.hide_points()
    _, _, again = _render(h)
    assert set(again) == set(plain)
    for k in plain:
        assert np.array_equal(_bits(_np(again[k])), _bits(_np(plain[k]))), k
    h.draw_points(h.pstyle)
    _, _, back = _render(h)
    assert torch.equal(back["image"], drawn["image"]) and torch.equal(back["point_id"], drawn["point_id"])


def test_fixed_trip_render_finished_by_render_continue_equals_the_blocking_render(chair):
    h, r, pose, plain, drawn = chair
    _, _, part = _render(h, async_trips=1, fused_from=-1)
    assert h.model.render_status()["alive_at_exit"] > 0
    assert not torch.equal(part["image"], drawn["image"])
    with torch.no_grad():
        done = h.model.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1, point_pose=pose))
    torch.cuda.synchronize()
    assert h.model.last_stats["alive_at_exit"] == 0
    for k in ("image", "depth_0", "weights_sum", "point_id", "point_t"):
        assert torch.equal(done[k].reshape(-1), drawn[k].reshape(-1)), k


def test_other_renders_and_other_ray_counts_refuse(chair):
    h, r, pose, plain, drawn = chair
    m = h.model
    for call in (lambda: m.rund_cuda(r["rays_o"], r["rays_d"], perturb=True, **h.render_kwargs()), lambda: m.run_cuda(r["rays_o"], r["rays_d"]),
                 lambda: m.render(r["rays_o"], r["rays_d"]), lambda: m.run(r["rays_o"], r["rays_d"])):
        with pytest.raises(RuntimeError, match="point overlay: .* only the deformed path"):
            call()
    with pytest.raises(RuntimeError, match="N == W H"):
        m.render_deformed(r["rays_o"][:, :100].contiguous(), r["rays_d"][:, :100].contiguous(), bg_color=None, perturb=False,
                          **dict(h.render_kwargs(), point_pose=pose))
    with pytest.raises(RuntimeError, match="point_pose"):
        m.render_deformed(r["rays_o"], r["rays_d"], bg_color=None, perturb=False, **h.render_kwargs())


def test_points_behind_a_drawn_sphere_are_hidden(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, draw=False)
    h.sim.enable_contact()
    h.sim.add_sphere((0.0, 0.0, 1.2), 0.45)      # between the camera and a part of the chair
    h.draw_colliders()
    _, _, plain = _render(h)
    plain = {k: v.clone() for k, v in plain.items()}
    st = point_style(radius=0)
    h.draw_points(st)
    _, _, out = _render(h)
    h.draw_points(point_style(radius=0, xray=True))
    _, _, x = _render(h)
    ct = _np(plain["collider_t"])
    behind = (_np(x["point_id"]) >= 0) & (_np(x["point_t"]) > ct + 0.05)      # the nearest point of the pixel lies behind the sphere
    assert behind.sum() > 10
    pid = _np(out["point_id"])
    assert (pid[behind] < 0).all()                                             # the occluded mode hides every one of them
    assert np.array_equal(_bits(_np(out["image"])[behind]), _bits(_np(plain["image"])[behind]))
    want = _restate(h, plain, st=st, collider_t=ct)
    assert np.array_equal(pid, want[1]) and np.array_equal(_bits(_np(out["image"])), _bits(want[0]))
    free = _restate(h, plain, st=st, collider_t=None)
    assert (free[1][behind] >= 0).sum() > 0                                    # without collider_t in the test some of them would be painted


def test_captured_step_follows_the_drag_target_and_the_camera_without_recapture(small_opt, small_cloud, ckpt):
    g = _harness(small_opt, small_cloud, ckpt, drag=True, style=point_style(radius=1, marker_radius=4, marker_thickness=2)).capture(n_trips=8)
    for _ in range(2):
        g.step_graph()
        g.finish_graph_frame()
    g.synchronize()
    vid = g.sim.n_IP // 3
    g.sim.drag_hold(vid, (0.3, 0.4, 0.2))
    pose2 = scene.orbit_pose(g.opt["radius"], 25.0, 10.0)
    dof = g.sim.dof.clone()
    out = g.step_graph(pose=pose2)
    g.finish_graph_frame()
    g.synchronize()
    got = {k: out[k].clone() for k in ("image", "point_id", "point_t", "depth_0")}
    red = (got["image"].reshape(-1, 3) == torch.tensor([1.0, 0.0, 0.0], device=DEV)).all(dim=1)
    assert int(red.sum()) > 5                                           # the handle is in the captured frame, at the target set after the capture
    # an eager step() at the state and the pose that frame was rendered from
    g.sim.dof.copy_(dof)
    m = g.model
    m.p_def, m.IP_F, m.IP_dF = g.sim.get_IP_info()
    want = g.step(pose=pose2, simulate=False)
    g.synchronize()
    for k in got:
        assert torch.equal(got[k].reshape(-1), want[k].reshape(-1)), k
    # ... and the restatement of that frame, markers included
    g.hide_points()
    g.pose = pose2
    _, _, plain = _render(g)
    ref = _restate(g, plain, drag=dict(vid=vid, active=1, target=np.array((0.3, 0.4, 0.2))))
    assert np.array_equal(_bits(_np(got["image"])), _bits(ref[0])) and np.array_equal(_np(got["point_id"]), ref[1])


def test_graph_captured_before_draw_points_is_refused(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, W=32, draw=False).capture(n_trips=8)
    h.step_graph()
    h.finish_graph_frame()
    h.draw_points()
    with pytest.raises(RuntimeError, match="captured before draw_points"):
        h.step_graph()
    h.hide_points()
    h.step_graph()
    h.finish_graph_frame()
    h.synchronize()


def test_multi_rank_and_staged_forms_raise_while_the_points_are_drawn(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, W=32)
    for call in (lambda: h.capture_frame_parallel(lanes=2, n_trips=8), lambda: h.capture_tile_parallel(), lambda: h.capture_staged(batch=256)):
        with pytest.raises(RuntimeError, match="does not draw the points"):
            call()


def test_pipelined_frames_draw_the_points(small_opt, small_cloud, ckpt):
    e = _harness(small_opt, small_cloud, ckpt, W=32)
    frames = []
    for _ in range(5):
        out = e.step()
        frames.append((e.to_host(out)["image"].copy(), out["point_id"].cpu().numpy().copy()))
    e.synchronize()
    assert (frames[0][1] >= 0).sum() > 50
    ids = {}      # the device outputs belong to the workspace: read when the frame retires, before its next frame overwrites them
    p = _harness(small_opt, small_cloud, ckpt, W=32).capture_pipelined(lanes=2, depth=2, n_trips=8,
                                                                       on_retire=lambda f, res: ids.__setitem__(f, res["device"]["point_id"].clone()))
    got = []
    for _ in range(len(frames)):
        got += [(i, res["image"].copy()) for i, res in p.step_pipelined()]
    got += [(i, res["image"].copy()) for i, res in p.drain_pipeline()]
    assert [i for i, _ in got] == list(range(len(frames))) and sorted(ids) == list(range(len(frames)))
    for f, (_, img) in enumerate(got):
        pid = ids[f].cpu().numpy()
        assert np.array_equal(pid.reshape(-1), frames[f][1].reshape(-1)), f      # every frame draws the state it was rendered from
        assert np.abs(img - frames[f][0]).max() < 1e-5, f
    late = _harness(small_opt, small_cloud, ckpt, W=32, draw=False).capture_pipelined(lanes=2, depth=2, n_trips=8)
    late.step_pipelined()
    late.drain_pipeline()
    late.draw_points()
    with pytest.raises(RuntimeError, match="captured before draw_points"):
        late.step_pipelined()


def test_pick_drawn_returns_the_point_at_the_pixel(small_opt, small_cloud, ckpt):
    h = _harness(small_opt, small_cloud, ckpt, drag=True, style=point_style(radius=1))
    out = h.step(simulate=False)
    h.synchronize()
    pid = out["point_id"][0].cpu().numpy()
    rows, cols = np.nonzero(pid >= 0)
    y, x = int(rows[len(rows) // 2]), int(cols[len(rows) // 2])
    vid = h.pick_drawn(x, y)
    assert vid == int(pid[y, x]) and vid >= 0
    h.synchronize()
    state = h.sim._drag.cpu().numpy()
    assert tuple(state[:1].view(np.int32)) == (vid, 1)
    assert np.array_equal(state[1:4], h.model.p_def[vid].double().cpu().numpy())      # held at its own position: no force until move()
    y0, x0 = (int(v[0]) for v in np.nonzero(pid < 0))
    assert h.pick_drawn(x0, y0) == -1
    with pytest.raises(ValueError, match="outside"):
        h.pick_drawn(10 ** 4, 0)
    out2 = h.step(simulate=False)      # the handle sits on the picked point now: the red disc is under the blue one, a point's radius from the pixel
    h.synchronize()
    r_, g_, b_ = out2["image"][0, y, x].tolist()      # blue, or blue under the line's black where the pixel is within its half thickness
    assert (r_, g_) == (0.0, 0.0) and b_ > 0.5


def test_main_render_draws_the_points(tmp_path, small_cloud):
    from pienerf_amd import io, main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--frames", "2", "--quiet"]
    a = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "plain")]))
    b = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "drawn"), "--draw_points", "--point_color", "0", "1", "0",
                                                                "--point_xray"]))
    assert len(a) == len(b) == 2
    for pa, pb in zip(a, b):
        ia, ib = io.load_image(pa).numpy().reshape(-1, 3), io.load_image(pb).numpy().reshape(-1, 3)
        green = (ib == np.array([0.0, 1.0, 0.0], np.float32)).all(axis=1)
        assert green.sum() > 100 and not (ia == np.array([0.0, 1.0, 0.0], np.float32)).all(axis=1).any()
        assert np.array_equal(ia[~green], ib[~green])
