"""The GUI's mouse drag on the device (csrc/pn_drag.hip; Simulator.enable_drag / drag_pick / drag_to / release; SimRenderHarness.drag / move)
against the reference's host loop, restated below in numpy, and across the harness forms (eager, captured step, pipelined, persistent substep)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the reference's three GUI functions (nerf/gui.py), in numpy
def screen_to_world(depth, x, y, intrinsics, pose, exact_mean=False):
    """gui.py:647-657 for a pixel inside the image.  The fallback mean (gui.py:625) is np.mean of the fp32 nonzero depths, an fp32 pairwise sum;
    exact_mean=True: the same mean summed in fp64 and rounded to fp32 once (what the device computes; the two differ by a few fp32 ulps, which
    the 1e5 spring turns into ~1e-7 of the displacements).  pose @ cam_coords is written out left to right (the device's order).  Returns
    (point, whether the zero-depth fallback was taken)."""
    fx, fy, cx, cy = intrinsics
    d = depth.reshape(2 * int(cx), 2 * int(cy))[int(x), int(y)]
    fb = d == 0.0
    if fb:
        nz = depth[np.nonzero(depth)]
        d = np.float32(nz.astype(np.float64).sum() / nz.size) if exact_mean else np.mean(nz)
    xs, ys, zs = (x - cx) / fx * d, (y - cy) / fy * d, np.float64(d)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    return np.array([P[r, 0] * xs + P[r, 1] * ys + P[r, 2] * zs + P[r, 3] for r in range(3)]), bool(fb)


def pick(pts, p):
    """gui.py:833-841."""
    dp = pts.astype(np.float64) - p
    return int(np.argmin(np.sum(dp ** 2, axis=1)))


def spring_force(scale, p1, p0):
    """gui.py:576-581 (|f| as sqrt((fx^2 + fy^2) + fz^2)).  Returns (f, clamped)."""
    f = scale * 1e5 * (p1 - p0.astype(np.float64))
    n = np.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    if n > 5e5:
        return f * (5e5 / n), True
    return f, False


# ---------------------------------------------------------------- helpers
def _restart(h):
    """Back to the rest state with a cold SVD warm start; the model renders the rest IP state."""
    s = h.sim
    torch.cuda.synchronize()
    s.dof.copy_(s.dof_rest)
    s.dof_vel.zero_()
    s.reset_warm_start()
    m = h.model
    m.p_def, m.IP_F, m.IP_dF = s.get_IP_info()
    torch.cuda.synchronize()


def _cursor_path(depth, n, W, H, leave=True):
    """A pick pixel on the object (the nonzero depth nearest to the image centre), then a straight line of n positions: out of the silhouette
    (leave=True: the zero-depth fallback is hit), or to the farthest pixel whose whole line lies on the object in this frame."""
    d = depth.reshape(W, H)   # index [x, y] as the reference reads it
    xs, ys = np.nonzero(d)
    k = int(np.argmin((xs - W / 2) ** 2 + (ys - H / 2) ** 2))
    x0, y0 = xs[k] + 0.25, ys[k] + 0.25
    line = lambda x1, y1: [(x0 + (x1 - x0) * i / (n - 1), y0 + (y1 - y0) * i / (n - 1)) for i in range(n)]
    if leave:
        return line(min(x0 + 0.45 * W, W - 1.0), max(y0 - 0.3 * H, 0.0))
    best, far = line(x0, y0), 0.0
    for j in np.argsort(-((xs - x0) ** 2 + (ys - y0) ** 2))[::37]:
        cand = line(xs[j] + 0.25, ys[j] + 0.25)
        r = float((xs[j] - x0) ** 2 + (ys[j] - y0) ** 2)
        if r > far and all(d[int(x), int(y)] != 0 and d[min(int(x) + 1, W - 1), int(y)] != 0 and d[int(x), min(int(y) + 1, H - 1)] != 0
                           for x, y in cand):
            best, far = cand, r
            break
    return best


def _drag_target(sim):
    return sim._drag[1:4].cpu().numpy()


# ---------------------------------------------------------------- 2: the device drag IS the reference's host loop (chair, configs[1], eager steps)
@pytest.mark.parametrize("leave", [False, True], ids=["on_object", "leaves_object"])
def test_device_drag_equals_the_reference_host_loop(leave):
    opt = scene.default_opt()
    h = SimRenderHarness(opt, device=DEV)
    W, H, n = opt["W"], opt["H"], 20
    scales = [1.0] * 10 + [30.0] * 10   # the wheel moved between frames 9 and 10: both branches of the clamp occur
    intr, pose = h.intrinsics, h.pose

    # the reference's loop: get_IP_info() to the host, screen_to_world, argmin, force, clamp, update_force
    _restart(h)
    depth = h.to_host(h.step(simulate=False))["depth_0"]
    path = _cursor_path(depth, n, W, H, leave)
    p, _ = screen_to_world(depth, *path[0], intr, pose, exact_mean=True)
    sid = pick(h.model.p_def.cpu().numpy(), p)
    want_traj, want_t, clamped, fallback = [], [], 0, 0
    for k in range(n):
        h.synchronize()
        pts = h.sim.get_IP_info()[0].cpu().numpy()
        p1, fb = screen_to_world(depth, *path[k], intr, pose, exact_mean=True)
        f, c = spring_force(scales[k], p1, pts[sid])
        clamped += c
        fallback += fb
        want_t.append(screen_to_world(depth, *path[k], intr, pose)[0])   # the reference's own np.mean
        h.sim.update_force(sid, f)
        depth = h.to_host(h.step())["depth_0"]
        h.synchronize()
        want_traj.append(h.sim.dof.clone())
    h.sim.clear_force()

    # the device drag
    _restart(h)
    h.enable_drag()
    h.step(simulate=False)
    vid = h.drag(*path[0])
    assert vid == sid
    got_traj, got_t = [], []
    for k in range(n):
        if k:
            if scales[k] != scales[k - 1]:
                h.sim.drag_scale(scales[k])
            h.move(*path[k])
        got_t.append(_drag_target(h.sim))
        h.step()
        h.synchronize()
        got_traj.append(h.sim.dof.clone())

    rest = h.sim.dof_rest
    big = max(float((t - rest).abs().max()) for t in want_traj)
    worst_t = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got_t, want_t))
    worst = max(float((a - b).abs().max()) for a, b in zip(got_traj, want_traj)) / big
    bitwise = all(torch.equal(a, b) for a, b in zip(got_traj, want_traj))
    print(f"drag vs host loop: vid {vid}; {clamped} of {n} frames clamped, {fallback} on the zero-depth fallback; target rel err {worst_t:.2e}; "
          f"dof rel err {worst:.2e} of the largest displacement {big:.3e}; bitwise: {bitwise}")
    assert 0 < clamped < n, clamped
    assert worst_t < 1e-6
    assert worst < 1e-12
    assert big > 1e-3   # the drag moved the chair
    if fallback == 0:
        assert bitwise


# ---------------------------------------------------------------- 3: a captured step follows the cursor; a graph without the drag refuses it
def _small(small_opt, small_cloud, ckpt, drag):
    h = SimRenderHarness(small_opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    if drag:
        h.enable_drag(scale=3.0)
    return h


def _path_small(h, n):
    W, H = h.opt["W"], h.opt["H"]
    return _cursor_path(h.to_host(h.step(simulate=False))["depth_0"], n, W, H)


def test_captured_step_follows_the_cursor_bit_for_bit(small_opt, small_cloud, ckpt):
    n = 8
    e = _small(small_opt, small_cloud, ckpt, True)
    path = _path_small(e, n)
    _restart(e)
    e.step()
    e.drag(*path[0])
    eager = []
    for k in range(n):
        if k:
            e.move(*path[k])
        e.step()
        e.synchronize()
        eager.append(e.sim.dof.clone())

    g = _small(small_opt, small_cloud, ckpt, True)
    g.capture(n_trips=8)
    _restart(g)
    g.step_graph()
    vid = g.drag(*path[0])
    graph = []
    for k in range(n):
        if k:
            g.move(*path[k])
        g.step_graph()
        g.finish_graph_frame()
        torch.cuda.synchronize()
        graph.append(g.sim.dof.clone())
    assert vid == int(e.sim._drag[:1].view(torch.int32)[0])
    assert float((graph[-1] - g.sim.dof_rest).abs().max()) > 1e-4
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))

    plain = _small(small_opt, small_cloud, ckpt, False)
    plain.capture(n_trips=8)
    plain.step_graph()
    plain.enable_drag()
    with pytest.raises(RuntimeError, match="captured before enable_drag"):
        plain.drag(*path[0])


# ---------------------------------------------------------------- 4: pipelined substeps get the force of their own state; the persistent form
def _sim(cloud, opt, persistent=False):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV, persistent=persistent)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


TARGET = (0.4, 0.6, -0.3)


def test_pipelined_drag_equals_eager_steps(small_opt, small_cloud, ckpt):
    h = _small(small_opt, small_cloud, ckpt, True)
    vid = h.sim.n_IP // 3
    h.sim.drag_hold(vid, TARGET)
    h.capture_pipelined(lanes=2, depth=2, n_trips=8)
    for _ in range(10):
        h.step_pipelined()
    h.drain_pipeline()
    steps = h.substeps_enqueued
    s = _sim(small_cloud, small_opt)
    s.enable_drag(scale=3.0)
    s.drag_hold(vid, TARGET)
    for _ in range(steps):
        s.stepforward()
    torch.cuda.synchronize()
    print(f"pipelined: {steps} substeps, max |dof - rest| {float((s.dof - s.dof_rest).abs().max()):.3e}")
    assert float((s.dof - s.dof_rest).abs().max()) > 1e-4
    assert torch.equal(h.sim.dof, s.dof) and torch.equal(h.sim.dof_vel, s.dof_vel)


def test_persistent_substep_with_drag(small_opt, small_cloud):
    a, b = _sim(small_cloud, small_opt, False), _sim(small_cloud, small_opt, True)
    for s in (a, b):
        s.enable_drag(scale=3.0)
        s.drag_hold(s.n_IP // 3, TARGET)
    worst = 0.0
    for k in range(8):
        a.stepforward()
        b.stepforward()
        torch.cuda.synchronize()
        e = rel_err((b.dof - b.dof_rest).cpu().numpy(), (a.dof - a.dof_rest).cpu().numpy())
        worst = max(worst, e)
        assert e < 1e-8, (k, e)
    assert b.persistent and b._coop is not None and not b.persistent_timed_out()
    print(f"persistent vs cell form with drag: worst relative difference {worst:.2e}")


# ---------------------------------------------------------------- 5: release() is clear_force()
def test_release_equals_clear_force(small_opt, small_cloud):
    a, b = _sim(small_cloud, small_opt), _sim(small_cloud, small_opt)
    a.enable_drag(scale=3.0)
    a.drag_hold(a.n_IP // 3, TARGET)
    for _ in range(3):
        a.stepforward()
    a.release()
    torch.cuda.synchronize()
    b.dof.copy_(a.dof)
    b.dof_vel.copy_(a.dof_vel)
    a.reset_warm_start()
    b.reset_warm_start()
    b.clear_force()
    for k in range(4):
        a.stepforward()
        b.stepforward()
        torch.cuda.synchronize()
        assert not bool(a.dof_f.any())
        assert torch.equal(a.dof, b.dof) and torch.equal(a.dof_vel, b.dof_vel), k
