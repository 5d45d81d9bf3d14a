"""Rigid balls, host side, on CPU (no kernel is launched): the packed state against the header's layout, the Simulator's setters and their refusals,
configuration before initialize(), main_render's --ball, and the law's restatement (tests/bodies_reference.py) against physics: Newton's third law, free
fall in closed form, a ball at rest on a floor."""
import re

import numpy as np
import pytest

from bodies_reference import body, clamp_scale, one_collider_accel, reaction, step_bodies
from conftest import ROOT
from contact_reference import plane, sphere

DT = 1e-2


def _cpu_sim(dx=0.1):
    from pienerf_amd.simulator.solver import Simulator
    return Simulator(device="cpu", persistent=False, dx=dx)


# ---------------------------------------------------------------- layout
def test_struct_sizes_and_packed_bytes():
    from pienerf_amd.simulator import bodies, solver
    assert bodies.BODY_DTYPE.itemsize == 72 and bodies.BODIES_STATE_DTYPE.itemsize == 616 and bodies.BODIES_STATE_DOUBLES == 77
    assert bodies.BODIES_SLOTS == solver.CONTACT_SLOTS == 8 and bodies.STAGE.nbytes == 616 and bodies.STAGE.clock
    hdr = open(f"{ROOT}/include/pienerf_hip.h").read()
    assert "sizeof(pn_bodies_state) = 616" in hdr and re.search(r"#define PN_BODIES_SLOTS 8\b", hdr)
    for name in ("pn_sim_bodies_bytes", "pn_sim_bodies_work_bytes", "pn_sim_bodies_set_params", "pn_sim_bodies_set_body", "pn_sim_bodies_set_motion",
                 "pn_sim_bodies_step"):
        assert re.search(rf"\b{name}\(", hdr), name
    raw = solver.pack_bodies_state(1, (0.0, -9.8, 0.0), [None, (2.5, 0.25)] + [None] * 6, k=7)
    assert len(raw) == 616
    w = np.frombuffer(raw, np.float64)
    i = np.frombuffer(raw, np.int32)
    assert np.frombuffer(raw, np.int64)[0] == 7 and i[2] == 1 and i[3] == 0 and w[2:5].tolist() == [0.0, -9.8, 0.0]
    b0, b1 = 5, 5 + 9          # a record is 9 doubles: (dynamic, reserved), M, c, F[3], s, delta_max, clamped
    assert not w[b0:b0 + 9].any()
    assert i[2 * b1] == 1 and i[2 * b1 + 1] == 0 and w[b1 + 1:b1 + 9].tolist() == [2.5, 0.25, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert not w[b1 + 9:].any()
    assert [st.name for st in solver.Simulator.STAGES] == ["drag", "pins", "contact", "bodies", "fields", "self"]


def test_library_sizes():
    from pienerf_amd import _lib
    h = _lib.lib()
    assert h.pn_sim_bodies_bytes() == 616
    # 32 doubles per workgroup of 256 points, and the one-launch form's arrival counter behind them
    assert h.pn_sim_bodies_work_bytes(432) == (2 * 32 + 1) * 8 and h.pn_sim_bodies_work_bytes(256) == 33 * 8 and h.pn_sim_bodies_work_bytes(257) == 65 * 8
    assert h.pn_sim_bodies_work_bytes(268_000) == (1047 * 32 + 1) * 8      # the stress cloud's size
    assert h.pn_sim_bodies_work_bytes(0) == 0 and h.pn_sim_bodies_work_bytes(-3) == 0 and h.pn_sim_bodies_work_bytes((1 << 27) + 1) == 0


def test_c_setters_refuse_bad_arguments():
    """PN_REQUIRE returns before anything is enqueued, so a made-up state pointer is never touched."""
    import ctypes
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)
    g = np.zeros(3)
    bad = np.array([0.0, np.nan, 0.0])
    pv = np.zeros(6)
    assert h.pn_sim_bodies_set_params(None, 1, g.ctypes.data, None) != 0
    assert h.pn_sim_bodies_set_params(d, 2, g.ctypes.data, None) != 0
    assert h.pn_sim_bodies_set_params(d, 1, bad.ctypes.data, None) != 0
    for args in ((None, 0, 1, 1.0, 0.0), (d, -1, 1, 1.0, 0.0), (d, 8, 1, 1.0, 0.0), (d, 0, 2, 1.0, 0.0), (d, 0, 1, 0.0, 0.0), (d, 0, 1, -1.0, 0.0),
                 (d, 0, 1, float("nan"), 0.0), (d, 0, 1, float("inf"), 0.0), (d, 0, 1, 1.0, -0.5), (d, 0, 1, 1.0, float("nan"))):
        assert h.pn_sim_bodies_set_body(*args, None) != 0, args
    for args in ((None, 0, 3), (d, 8, 3), (d, -1, 1), (d, 0, 0), (d, 0, 4)):
        assert h.pn_sim_bodies_set_motion(*args, pv.ctypes.data, None) != 0, args
    assert h.pn_sim_bodies_set_motion(d, 0, 3, None, None) != 0
    pv[4] = np.inf
    assert h.pn_sim_bodies_set_motion(d, 0, 3, pv.ctypes.data, None) != 0
    assert h.pn_sim_bodies_clock(d, -1, None) != 0 and h.pn_sim_bodies_clock(None, 0, None) != 0
    ok = (4, 100, d, d, d, 0.01, 0.1, d, d, d, d, d, 0, None)
    for j, v in ((0, 0), (1, 0), (1, (1 << 27) + 1), (2, None), (3, None), (4, None), (5, 0.0), (5, float("nan")), (6, -1.0), (7, None), (11, None),
                 (12, 2), (12, -1)):
        a = list(ok)
        a[j] = v
        assert h.pn_sim_bodies_step(*a) != 0, (j, v)


# ---------------------------------------------------------------- the Simulator's setters
def test_refusals_and_configuration_before_initialize():
    from pienerf_amd.simulator import solver
    s = _cpu_sim()
    assert not s.bodies_enabled and s._bodies_state is None
    with pytest.raises(ValueError, match="enable_contact"):
        s.enable_bodies()
    with pytest.raises(ValueError, match="enable_contact"):
        s.add_body((0, 0, 1), 0.3, 1.0)
    s.enable_contact()
    with pytest.raises(RuntimeError, match="enable_bodies"):
        s.add_body((0, 0, 1), 0.3, 1.0)
    assert s.enable_bodies() is s and s.bodies_enabled and "bodies" in s.enabled_stage_names()
    assert [st.name for st in s.enabled_stages()] == ["contact", "bodies"]
    for kw in (dict(mass=0.0), dict(mass=-1.0), dict(mass=float("nan")), dict(mass=float("inf")), dict(mass=1.0, damping=-1.0),
               dict(mass=1.0, damping=float("nan")), dict(mass=1.0, radius=0.0), dict(mass=1.0, centre=(0.0, float("nan"), 0.0)),
               dict(mass=1.0, velocity=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            s.add_body(**dict(dict(centre=(0, 0, 1), radius=0.3), **kw))
    assert s.collider_types() == [0] * 8 and s.body_indices() == []       # a refused body takes no slot
    floor = s.add_plane((0, -1, 0), (0, 1, 0))
    b = s.add_body((0, 0, 1.3), 0.3, 440.64, velocity=(0, 0, -4), damping=0.5)
    assert (floor, b) == (0, 1) and s.body_indices() == [1] and s.collider_types()[1] == solver.CONTACT_SPHERE
    assert s.bodies_state_bytes() == solver.pack_bodies_state(1, (0.0, -9.8, 0.0), [None, (440.64, 0.5)] + [None] * 6)
    want = [solver.contact_plane((0, -1, 0), (0, 1, 0)), solver.contact_sphere((0, 0, 1.3), 0.3, velocity=(0, 0, -4))] + [None] * 6
    assert s.contact_state_bytes() == solver.pack_contact_state(1, s._contact_params, want)
    # set_collider on a body's slot: the mirror is stale, set_body is the way
    with pytest.raises(ValueError, match="set_body"):
        s.set_collider(b, centre=(0, 0, 0))
    s.set_collider(floor, point=(0, -0.9, 0))                           # the others still move
    with pytest.raises(ValueError, match="no body"):
        s.set_body(floor, mass=2.0)
    with pytest.raises(ValueError, match="mass"):
        s.set_body(b, mass=0.0)
    s.set_body(b, velocity=(1, 0, 0), mass=2.0)
    assert s._bodies[b] == (2.0, 0.5) and s._colliders[b][1][7:10].tolist() == [1.0, 0.0, 0.0] and s._colliders[b][1][0:3].tolist() == [0.0, 0.0, 1.3]
    # the GPU-only calls say so
    for call in (s.body_state, s.body_clock, s.reset_body_clock, s.stop_bodies):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    # a ninth collider
    for _ in range(6):
        s.add_body((0, 0, 2), 0.1, 1.0)
    with pytest.raises(ValueError, match="slots"):
        s.add_body((0, 0, 2), 0.1, 1.0)
    # remove_collider on a body's slot removes the body; remove_body frees the slot
    s.remove_collider(b)
    assert s.body_indices() == [2, 3, 4, 5, 6, 7] and s.collider_types()[b] == 0
    s.remove_body(7)
    assert s.body_indices() == [2, 3, 4, 5, 6] and s.collider_types()[7] == 0
    assert s.add_body((0, 0, 2), 0.1, 3.0) == 1
    s.clear_colliders()
    assert s.body_indices() == [] and s.collider_types() == [0] * 8
    # another gravity
    t = _cpu_sim().enable_contact().enable_bodies(gravity=(0, 0, 0))
    assert t.bodies_state_bytes() == solver.pack_bodies_state(1, (0, 0, 0), [None] * 8)
    with pytest.raises(ValueError, match="gravity"):
        _cpu_sim().enable_contact().enable_bodies(gravity=(0, float("nan"), 0))


def test_keep_state_without_bodies_keeps_its_keys(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
    s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
    s.enable_contact().enable_bodies()
    s.add_body((0, 0, 1.3), 0.3, 1.0)
    s.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    keep = s.keep_state()
    assert set(keep) == {"dof", "dof_vel", "clocks"}            # no device state on a CPU simulator: nothing more to keep
    assert [st.name for st, _ in keep["clocks"]] == ["pins", "bodies", "fields"]
    s.restore_state(keep)


# ---------------------------------------------------------------- main_render --ball
def test_main_render_ball_arguments():
    from pienerf_amd import main_render
    from pienerf_amd.simulator import solver
    ap = main_render.parser()
    a = ap.parse_args(["--ball", "0", "0.6", "1.5", "0.25", "200", "--ball", "0", "0", "2", "0.1", "3", "0", "0", "-3", "--ball_damping", "0.5", "--floor", "-0.95"])
    assert a.ball == [[0.0, 0.6, 1.5, 0.25, 200.0], [0.0, 0.0, 2.0, 0.1, 3.0, 0.0, 0.0, -3.0]] and main_render.wants_contact(a)
    specs = main_render.ball_specs(a)
    assert specs == [dict(centre=(0.0, 0.6, 1.5), radius=0.25, mass=200.0, velocity=None, damping=0.5),
                     dict(centre=(0.0, 0.0, 2.0), radius=0.1, mass=3.0, velocity=(0.0, 0.0, -3.0), damping=0.5)]
    s = _cpu_sim()
    assert main_render.configure_contact(s, a) == [0, 1, 2] and s.bodies_enabled and s.body_indices() == [1, 2]
    t = _cpu_sim().enable_contact(thickness=None).enable_bodies()
    t.add_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0))
    t.add_body((0.0, 0.6, 1.5), 0.25, 200.0, damping=0.5)
    t.add_body((0.0, 0.0, 2.0), 0.1, 3.0, velocity=(0.0, 0.0, -3.0), damping=0.5)
    assert s.contact_state_bytes() == t.contact_state_bytes() and s.bodies_state_bytes() == t.bodies_state_bytes()
    # --ball enables contact by itself
    s = _cpu_sim()
    assert main_render.configure_contact(s, ap.parse_args(["--ball", "0", "0", "1", "0.2", "5"])) == [0] and s.contact_enabled and s.bodies_enabled
    assert s.bodies_state_bytes() == solver.pack_bodies_state(1, (0.0, -9.8, 0.0), [(5.0, 0.0)] + [None] * 7)
    for n in (6, 4, 9):
        with pytest.raises(SystemExit, match="5 or 8 numbers"):
            main_render.ball_specs(ap.parse_args(["--ball"] + ["1"] * n))
    with pytest.raises(SystemExit, match="needs --ball"):
        main_render.ball_specs(ap.parse_args(["--ball_damping", "1"]))
    with pytest.raises(SystemExit, match="mass"):          # a usage error, not a traceback
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--ball", "0", "0", "1", "0.2", "0"]))
    d = ap.parse_args([])
    assert main_render.ball_specs(d) == [] and not main_render.wants_contact(d)
    # it composes with the other flags
    a = ap.parse_args(["--ball", "0", "0.6", "1.5", "0.25", "200", "0", "0", "-3", "--floor", "-0.95", "--unpin", "--draw_colliders", "--shadows", "--video"])
    main_render.check_overlay_args(a)
    assert a.unpin and a.draw_colliders and a.shadows and a.video is not None


# ---------------------------------------------------------------- the law's restatement against physics
def test_newtons_third_law():
    """F_b + sum_i m_i a_{i,b} = 0 to rounding, and with the ball as the only collider a_{i,b} is contact_accel's a_i."""
    from contact_reference import contact_accel
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, size=(3000, 3))
    v = rng.normal(scale=2.0, size=(3000, 3))
    m = rng.uniform(0.5, 2.0, size=3000)
    b = body((0.1, 0.0, 0.4), 0.6, 10.0, velocity=(0.3, -0.2, 0.5))
    F, dmax = reaction(b, x, v, m, DT, 0.5, 0.5, 0.5, 0.05)
    a, delta = one_collider_accel(b, x, v, DT, 0.5, 0.5, 0.5, 0.05)
    a_all, hit = contact_accel([b], x, v, DT, 0.5, 0.5, 0.5, 0.05)
    assert 100 < hit.sum() < 2900 and np.array_equal(a, a_all) and np.array_equal(hit, delta > 0.0)
    total = F + (m[:, None] * a).sum(axis=0)
    assert np.abs(total).max() <= 1e-12 * np.abs(F).max() and np.abs(F).max() > 1.0
    assert dmax == delta.max() > 0.0
    # the clamp: a heavy ball is never clamped, a light one moves by its deepest penetration at most
    assert clamp_scale(F, 1e9, dmax, DT) == 1.0 and clamp_scale(np.zeros(3), 1.0, 0.0, DT) == 1.0
    s = clamp_scale(F, 1e-3, dmax, DT)
    assert 0.0 < s < 1.0 and abs(DT * DT * s * np.linalg.norm(F) / 1e-3 - dmax) <= 1e-12 * dmax


def test_free_fall_is_the_closed_form_sequence():
    g, c = np.array([0.0, -9.8, 0.0]), 0.7
    b = body((0.2, 3.0, -0.1), 0.25, 2.0, velocity=(1.0, 2.0, -0.5), damping=c)
    far = body((5.0, 5.0, 5.0), 0.1, 1.0)              # a second ball: they do not see each other
    p, u = b["p"].copy(), b["v"].copy()
    for k in range(50):
        step_bodies([None, b, far], None, None, None, DT, g, 0.5, 0.5, 0.5, 0.05)
        u = (u + DT * g) / (1.0 + DT * c)
        p = p + DT * u
        assert np.array_equal(b["p"], p) and np.array_equal(b["v"], u), k
    assert b["clamped"] == 0 and b["s"] == 1.0 and not b["F"].any()
    # undamped: u_k = u_0 + k dt g, p_k = p_0 + k dt u_0 + dt^2 g k (k + 1) / 2
    b = body((0.0, 0.0, 0.0), 0.25, 2.0, velocity=(1.0, 0.0, 0.0))
    for _ in range(40):
        step_bodies([b], None, None, None, DT, g, 0.5, 0.5, 0.5, 0.05)
    assert np.allclose(b["v"], np.array([1.0, 0.0, 0.0]) + 40 * DT * g, rtol=0, atol=1e-13)
    assert np.allclose(b["p"], 40 * DT * np.array([1.0, 0.0, 0.0]) + DT * DT * g * 40 * 41 / 2, rtol=0, atol=1e-13)


def test_a_ball_alone_on_a_floor_settles():
    """Stationary under kappa delta / dt^2 = g: delta = g dt^2 / kappa = 1.96e-3 with dt = 0.01, kappa = 0.5."""
    g = np.array([0.0, -9.8, 0.0])
    floor = plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0))
    b = body((0.0, -1.0 + 0.25, 0.0), 0.25, 3.0)        # resting on the plane, at rest
    for _ in range(200):
        step_bodies([floor, b], None, None, None, DT, g, 0.5, 0.5, 0.5, 0.05)
    pen = b["R"] - (b["p"][1] + 1.0)
    print(f"penetration after 200 substeps {pen:.6e}, speed {np.linalg.norm(b['v']):.3e}")
    assert abs(pen - 9.8 * DT * DT / 0.5) < 1e-6 and abs(pen - 1.96e-3) < 1e-6
    assert np.linalg.norm(b["v"]) < 1e-6
    # a static solid sphere below and the container around act alike: the ball ends outside the one and inside the other
    below = sphere((0.0, -2.0, 0.0), 1.0)
    shell = sphere((0.0, 0.0, 0.0), 3.0, inside=True)
    b = body((0.0, -0.7, 0.0), 0.25, 3.0)
    for _ in range(300):
        step_bodies([below, shell, b], None, None, None, DT, g, 0.5, 0.5, 0.5, 0.05)
    gap = np.linalg.norm(b["p"] - below["p"]) - 1.0 - 0.25
    assert -3e-3 < gap < 0.0 and np.linalg.norm(b["v"]) < 1e-4
