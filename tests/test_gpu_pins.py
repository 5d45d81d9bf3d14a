"""Kinematic pins on the GPU (csrc/pn_pins.hip; Simulator.enable_pin_motion / set_pin_motion / set_pin_offsets / stop_pin_motion / reset_pin_clock;
main_render --pin_shake / --pin_twist): the right-hand-side term against its numpy restatement (tests/test_pins_host.py), the substep clock, and
trajectories against the CPU oracle, whose public rhs_gravity is set to g0 + pin_term(u(t)) before every stepforward(), in the three substep forms
and the harness forms (eager, captured step, pipelined)."""
import numpy as np
import pytest
import torch

from conftest import make_oracle_sim, rel_err
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
from test_gpu_parity import DEV
from test_pins_host import oracle_pins, pin_term, pin_u

pytestmark = pytest.mark.gpu

SHAKE = ((0.05, 0.02, -0.03), 4.0, 0.3)                 # (A, hz, phase)


def twist(centre, deg=12.0):
    return ((0.2, 1.0, -0.1), deg, 3.0, 0.5, centre)     # (axis, degrees, hz, phase, centre)


def _sim(cloud, opt, persistent=False):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device=DEV, persistent=persistent)
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


def _centre(cloud):
    return np.asarray(cloud["pos"], np.float64)[np.nonzero(cloud["pin"])[0]].mean(axis=0)


class OraclePins:
    """The oracle with moving pins: before every stepforward() its rhs_gravity is g0 + pin_term(u((k + 1) dt)) for the motion in force at substep k."""

    def __init__(self, cloud, opt):
        self.ref = make_oracle_sim(cloud, opt)
        self.g0 = self.ref.rhs_gravity.copy()
        _, self.kern, self.Nx, self.X = oracle_pins(self.ref)
        self.k, self.motion = 0, None

    def step(self):
        r = self.ref
        r.rhs_gravity = self.g0.copy()
        if self.motion is not None:
            r.rhs_gravity += pin_term(r.n_k, r.stiff, self.kern, self.Nx, pin_u(self.X, (self.k + 1) * r.dt, **self.motion))
        r.stepforward()
        self.k += 1
        return r.dof - r.dof_rest


# ---------------------------------------------------------------- 1: the right-hand-side term against numpy; empty runs, inactive state, repeatability
# Three clouds of the same 1 208 points: the small chair as it is (16 pins: most kernels have no pin entry, runs of 4 entries), its lowest 0.5 pinned
# (128 pins, runs of up to 32: half a wave), its lowest 1.0 pinned (744 pins, runs of up to 200: several passes of the 64-lane workgroup, the last one
# ragged — 66, 68, 70, 82, 100, 148 ... entries)
@pytest.mark.parametrize("pin_height", [None, 0.5, 1.0], ids=["chair_16_pins", "pin_height_0.5", "pin_height_1.0"])
def test_rhs_term_equals_the_numpy_term(small_cloud, small_opt, pin_height):
    cloud = scene.make_chair_points(sub_res=30, pin_height=pin_height, hgs=small_opt["hash_grid_size"]) if pin_height else small_cloud
    s = _sim(cloud, small_opt).enable_pin_motion()
    kern, Nx, X = s.pin_kernel.cpu().numpy(), s.pin_Nx.cpu().numpy(), s.pin_rest.cpu().numpy()
    g = s.rhs_gravity.clone()
    runs = np.diff(s.pin_bg.cpu().numpy())
    print(f"{s.n_pin} pins, n_k {s.n_k}: {int((runs == 0).sum())} kernels without a pin entry, longest run {runs.max()}, runs % 64: {sorted(set(runs % 64))[:6]} ...")
    assert s.n_pin == int(np.asarray(cloud["pin"]).sum()) and runs.sum() == 8 * s.n_pin
    if pin_height == 1.0:
        assert s.n_pin >= 200 and runs.max() > 128 and (runs[runs > 64] % 64 != 0).any()   # more than one pass of the workgroup, a ragged last pass
    elif pin_height == 0.5:
        assert s.n_pin > 100 and 16 < runs.max() < 64 and (runs == 0).any()
    else:
        assert s.n_pin == 16 and (runs == 0).sum() > s.n_k // 2 and runs.max() < 64
    empty = torch.from_numpy(np.repeat(runs == 0, 30)).to(DEV)
    c = X.mean(axis=0)
    off = np.random.default_rng(5).normal(scale=0.02, size=X.shape)
    motions = {"translate": dict(translate=SHAKE), "rotate": dict(rotate=twist(c, 25.0)), "both+offsets": dict(translate=SHAKE, rotate=twist(c + 0.1), offsets=off)}
    worst = 0.0
    for name, m in motions.items():
        s.set_pin_offsets(m.get("offsets"))
        s.set_pin_motion(translate=m.get("translate"), rotate=m.get("rotate"))
        for k in (0, 1, 37):
            s.reset_pin_clock(k)
            got = s._enqueue_pin_rhs().clone()
            assert s.pin_clock() == k + 1
            s.reset_pin_clock(k)
            again = s._enqueue_pin_rhs().clone()
            assert torch.equal(got.view(torch.int64), again.view(torch.int64)), (name, k)       # two runs, equal bits
            assert torch.equal(got[empty].view(torch.int64), g[empty].view(torch.int64))         # rows of kernels without a pin entry: rhs_gravity's bits
            want = pin_term(s.n_k, s.stiff, kern, Nx, pin_u(X, (k + 1) * s.dt, **m))
            e = rel_err((got - g).cpu().numpy().reshape(-1, 3), want)
            worst = max(worst, e)
            assert np.abs(want).max() > 1.0 and e < 1e-12, (name, k, e)
    print(f"rhs_ext - rhs_gravity vs numpy: worst rel err {worst:.2e}")
    assert torch.equal(s.rhs_gravity, g)                                                          # the input is left alone
    s.stop_pin_motion()
    out = s._enqueue_pin_rhs()
    assert torch.equal(out.view(torch.int64), g.view(torch.int64))                                # active = 0: rhs_gravity, bit for bit


# ---------------------------------------------------------------- 2: the clock
def test_the_clock_counts_substeps(small_cloud, small_opt):
    s = _sim(small_cloud, small_opt).enable_pin_motion()
    assert s.pin_clock() == 0
    for n in range(1, 4):
        s.stepforward()
        assert s.pin_clock() == n
    assert torch.equal(s._rhs_ext, s.rhs_gravity)   # no motion set: the substeps ran on rhs_gravity's bits
    s.set_pin_motion(translate=SHAKE)
    s.reset_pin_clock(41)
    assert s.pin_clock() == 41
    s.stepforward()
    assert s.pin_clock() == 42
    s.stop_pin_motion()
    s.stepforward()
    assert s.pin_clock() == 43                       # the clock counts substeps, moving or not
    s.reset_pin_clock()
    assert s.pin_clock() == 0
    with pytest.raises(ValueError):
        s.reset_pin_clock(-1)
    with pytest.raises(ValueError):
        s.set_pin_offsets(np.zeros((s.n_pin + 1, 3)))
    with pytest.raises(ValueError):
        s.set_pin_motion(rotate=((0.0, 0.0, 0.0), 10.0, 1.0))
    with pytest.raises(ValueError, match="translate is"):
        s.set_pin_motion(translate=((0.1, 0.0, 0.0),))
    # rotate with the phase given and the centre left out: the centroid of the pinned rest points
    X = s.pin_rest.cpu().numpy()
    s.set_pin_motion(rotate=((0.2, 1.0, -0.1), 25.0, 3.0, 0.5))
    s.reset_pin_clock(5)
    got = (s._enqueue_pin_rhs() - s.rhs_gravity).cpu().numpy().reshape(-1, 3)
    want = pin_term(s.n_k, s.stiff, s.pin_kernel.cpu().numpy(), s.pin_Nx.cpu().numpy(), pin_u(X, 6 * s.dt, rotate=twist(X.mean(axis=0), 25.0)))
    assert np.abs(want).max() > 1.0 and rel_err(got, want) < 1e-12
    plain = _sim(small_cloud, small_opt)
    assert s.n_pin == 16 and plain.n_pin == 0 and plain.pin_bg is None   # the tables exist only with the feature on
    # enabled before initialize(): the state arrives with the cloud
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud
    t = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device=DEV).enable_pin_motion()
    t.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert t.pin_clock() == 0
    with pytest.raises(ValueError, match="pinned"):
        _sim(dict(c, pin=np.zeros_like(c["pin"])), o).enable_pin_motion()


# ---------------------------------------------------------------- 3: trajectories against the oracle, in the three substep forms
N_TRAJ = 12


@pytest.fixture(scope="module")
def oracle_traj(small_cloud, small_opt):
    """Displacements dof - dof_rest of the oracle after each of 12 substeps under gravity with shake and twist combined, and the last state of a run
    without pin motion."""
    o = OraclePins(small_cloud, small_opt)
    o.motion = dict(translate=SHAKE, rotate=twist(_centre(small_cloud)))
    moved = [o.step().copy() for _ in range(N_TRAJ)]
    p = OraclePins(small_cloud, small_opt)
    for _ in range(N_TRAJ):
        plain = p.step().copy()
    return moved, plain


def _run(s, cloud):
    s.enable_pin_motion()
    s.set_pin_motion(translate=SHAKE, rotate=twist(_centre(cloud)))
    out = []
    for _ in range(N_TRAJ):
        s.stepforward()
        out.append((s.dof - s.dof_rest).cpu().numpy().reshape(-1, 3))
    return out


@pytest.mark.parametrize("form", ["cells", "csr"])
def test_trajectory_matches_the_oracle(small_cloud, small_opt, oracle_traj, monkeypatch, form):
    monkeypatch.setenv("PN_SIM_FORM", form)
    s = _sim(small_cloud, small_opt)
    assert s.cell_form == (form == "cells")
    got = _run(s, small_cloud)
    moved, plain = oracle_traj
    errs = [rel_err(a, b) for a, b in zip(got, moved)]
    print(f"{form} form with moving pins vs oracle, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    for k, e in enumerate(errs):
        assert e < 1e-4, (k, e)
    diff = float(np.abs(got[-1] - plain).max())
    print(f"last state vs a run without pin motion: max abs difference {diff:.3e}")
    assert diff > 1e-3     # the pins really moved it


def test_persistent_form_matches_the_launch_form(small_cloud, small_opt):
    a, b = _sim(small_cloud, small_opt, False), _sim(small_cloud, small_opt, True)
    ta, tb = _run(a, small_cloud), _run(b, small_cloud)
    assert b.persistent and b._coop is not None and not b.persistent_timed_out()
    errs = [rel_err(y, x) for x, y in zip(ta, tb)]
    print("persistent vs cell form with moving pins, per substep: " + " ".join(f"{e:.1e}" for e in errs))
    for k, e in enumerate(errs):
        assert e < 1e-8, (k, e)
    assert a.pin_clock() == b.pin_clock() == N_TRAJ


# ---------------------------------------------------------------- 4: the harness forms
def _harness(small_opt, small_cloud, ckpt, W=64):
    h = SimRenderHarness(dict(small_opt, W=W, H=W), cloud=small_cloud, ckpt=ckpt, device=DEV)
    h.sim.enable_pin_motion()
    h.sim.set_pin_motion(translate=SHAKE, rotate=twist(_centre(small_cloud)))
    return h


@pytest.fixture(scope="module")
def eager_frames(small_opt, small_cloud, ckpt):
    """9 eager frames with moving pins: host images / depth_0 and the displacements after every step."""
    e = _harness(small_opt, small_cloud, ckpt)
    frames, disp = [], []
    for _ in range(9):
        frames.append(e.to_host(e.step()))
        e.synchronize()
        disp.append((e.sim.dof - e.sim.dof_rest).cpu().numpy())
    return frames, disp


def test_captured_step_with_moving_pins_equals_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, disp = eager_frames
    g = _harness(small_opt, small_cloud, ckpt).capture(n_trips=8)
    assert g.sim.pin_clock() == 0 and torch.equal(g.sim.dof, g.sim.dof_rest)   # capture's warm-up steps left neither the clock nor the state advanced
    for f in range(5):
        b = g.step_graph()
        g.finish_graph_frame()
        g.synchronize()
        assert np.abs(b["image"][0].cpu().numpy() - frames[f]["image"]).max() < 1e-5 and np.abs(b["depth_0"][0].cpu().numpy() - frames[f]["depth_0"]).max() < 1e-4, f
        e = rel_err((g.sim.dof - g.sim.dof_rest).cpu().numpy(), disp[f])
        assert e < 1e-7, (f, e)
    assert g.sim.pin_clock() == 5
    d = float(np.abs(frames[0]["image"] - frames[4]["image"]).max())
    print(f"images of frame 0 and frame 4 differ by {d:.3e}")
    assert d > 1e-3
    # a graph captured without the pin launch refuses to run once pin motion is enabled
    plain = SimRenderHarness(dict(small_opt, W=32, H=32), cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=8)
    plain.step_graph()
    plain.finish_graph_frame()
    plain.sim.enable_pin_motion()
    with pytest.raises(RuntimeError, match="captured before enable_pin_motion"):
        plain.step_graph()


def test_pipelined_frames_with_moving_pins_equal_eager_steps(small_opt, small_cloud, ckpt, eager_frames):
    frames, _ = eager_frames
    p = _harness(small_opt, small_cloud, ckpt).capture_pipelined(lanes=2, depth=2, n_trips=8)
    got = []
    for f in range(len(frames)):
        for idx, res in p.step_pipelined():
            got.append((idx, res["image"].copy()))
    for idx, res in p.drain_pipeline():
        got.append((idx, res["image"].copy()))
    assert [i for i, _ in got] == list(range(len(frames)))
    for f, (_, img) in enumerate(got):
        assert np.abs(img - frames[f]["image"]).max() < 1e-5, f
    assert p.substeps_enqueued == len(frames) + 2 == p.sim.pin_clock()
    s = _sim(small_cloud, small_opt).enable_pin_motion()
    s.set_pin_motion(translate=SHAKE, rotate=twist(_centre(small_cloud)))
    for _ in range(p.substeps_enqueued):
        s.stepforward()
    want = (s.dof - s.dof_rest).cpu().numpy()
    err = rel_err((p.sim.dof - p.sim.dof_rest).cpu().numpy(), want)
    print(f"pipelined (lanes 2, depth 2) with moving pins vs eager after {p.substeps_enqueued} substeps: {err:.2e}")
    assert err < 1e-7


# ---------------------------------------------------------------- 5: a change of the motion lands between two substeps
def test_motion_change_between_overlapped_steps_matches_oracle(small_cloud, small_opt, ckpt):
    """set_pin_motion / set_pin_offsets / stop_pin_motion while the substeps run on their own stream (harness.step with overlap_sim, and the pipelined
    form with the simulator running ahead): the change is enqueued on the simulator's stream, so it acts from the next substep — the trajectory equals
    the oracle's with the motion switched at the same substep index."""
    opt = dict(small_opt, W=32, H=32)
    c = _centre(small_cloud)
    n_pin = int(np.asarray(small_cloud["pin"]).sum())
    off = np.random.default_rng(9).normal(scale=0.01, size=(n_pin, 3))
    m1, m2, m3 = dict(translate=SHAKE), dict(rotate=twist(c, 20.0)), dict(translate=((0.0, 0.04, 0.0), 6.0, 1.0), rotate=twist(c), offsets=off)

    def apply(sim, ora, m):
        if m is None:
            sim.stop_pin_motion()
        else:
            sim.set_pin_offsets(m.get("offsets"))
            sim.set_pin_motion(translate=m.get("translate"), rotate=m.get("rotate"))
        ora.motion = m

    for rep in range(2):
        h = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)   # overlap_sim: the substep on a side stream
        assert h.sim.force_stream is h._sim_stream
        h.sim.enable_pin_motion()
        ora = OraclePins(small_cloud, opt)
        plan = {1: m1, 3: m2, 5: None, 6: m3}
        for step in range(8):
            if step in plan:
                apply(h.sim, ora, plan[step])
            h.step()     # no synchronisation in between
            want = ora.step()
        h.synchronize()
        e = rel_err(h.sim.dof.cpu().numpy().reshape(-1, 3) - ora.ref.dof_rest, want)
        assert e < 1e-6, (rep, e)
        assert np.abs(want).max() > 1e-3 and h.sim.pin_clock() == 8
    # pipelined: the simulator is ahead; a motion set now acts from substep `substeps_enqueued`
    p = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    p.sim.enable_pin_motion()
    p.capture_pipelined(lanes=2, n_trips=8)
    ora = OraclePins(small_cloud, opt)
    for frame in range(9):
        if frame in (2, 5):
            while ora.k < p.substeps_enqueued:
                want = ora.step()
            apply(p.sim, ora, m3 if frame == 2 else m1)
        p.step_pipelined()
    p.drain_pipeline()
    while ora.k < p.substeps_enqueued:
        want = ora.step()
    e = rel_err(p.sim.dof.cpu().numpy().reshape(-1, 3) - ora.ref.dof_rest, want)
    print(f"pipelined, motion changed at frames 2 and 5: rel err vs oracle {e:.2e}")
    assert e < 1e-6


# ---------------------------------------------------------------- 6: main_render --pin_shake
def test_main_render_shakes_the_chair_by_its_feet(tmp_path, small_cloud):
    from pienerf_amd import main_render
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    A, hz = (0.05, 0.02, -0.03), 5.0
    args = main_render.parser().parse_args(["--ply", str(tmp_path / "chair.ply"), "--out", str(tmp_path / "out"), "--frames", "4", "--W", "48", "--H", "48",
                                            "--sim_dx", "0.1", "--sim_iters", "4", "--pin_shake", *[str(v) for v in A], str(hz), "--save_ply", "--quiet"])
    files = main_render.run(args)
    assert [f.split("/")[-1] for f in files] == [f"img_{f}.png" for f in range(4)]
    from PIL import Image
    imgs = [np.asarray(Image.open(f)) for f in files]
    assert all(i.shape == (48, 48, 3) for i in imgs) and (imgs[0] != 255).any() and (imgs[0] != imgs[3]).any()
    # points_3.ply is the state after 4 substeps, the last of them with u(t) at t = 4 dt
    pin = np.nonzero(small_cloud["pin"])[0]
    X = np.asarray(small_cloud["pos"], np.float64)[pin]
    u = pin_u(X, 4 * scene.default_opt()["sim_dt"], translate=(A, hz, 0.0))
    pts = scene.read_ply(str(tmp_path / "out" / "points_3.ply"))
    x = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)[pin]
    lag = float(np.linalg.norm(x - X - u, axis=1).max() / np.linalg.norm(u[0]))
    print(f"pinned points of points_3.ply: worst distance to their targets {lag:.3f} |u(t3)|, |u| = {np.linalg.norm(u[0]):.4f}")
    assert lag < 0.3
    with pytest.raises(SystemExit):
        main_render.run(main_render.parser().parse_args(["--out", str(tmp_path / "o2"), "--frames", "1", "--pin_centre", "0", "0", "0"]))
    with pytest.raises(SystemExit, match="axis"):   # a zero axis is a usage error, not a traceback
        main_render.run(main_render.parser().parse_args(["--ply", str(tmp_path / "chair.ply"), "--out", str(tmp_path / "o3"), "--frames", "1", "--W", "48", "--H", "48",
                                                         "--sim_dx", "0.1", "--sim_iters", "4", "--pin_twist", "0", "0", "0", "10", "1", "--quiet"]))
