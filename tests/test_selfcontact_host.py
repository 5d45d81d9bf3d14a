"""Self-contact, host side, on CPU (no kernel is launched): the C ABI and its argument checks, the packed state against the header's layout, the
Simulator's setters, main_render's arguments, scene.make_block_points, and the law's invariants on its numpy restatement
(tests/selfcontact_reference.py) on the small chair squeezed by the global maps diag(1, 0.25, 1) and 0.3 I."""
import ctypes
import re
import struct

import numpy as np
import pytest

import selfcontact_reference as R
from conftest import make_oracle_sim
from contact_reference import ip_state
from test_contact_host import _c_layout, _cpu_sim, _header

SELF_SYMBOLS = ("pn_sim_self_bytes", "pn_sim_self_work_bytes", "pn_sim_self_launches", "pn_sim_self_set_params", "pn_sim_self_rhs")
PN_ERR_ARG = 1
MAPS = {"rest": np.eye(3), "squeezed": np.diag([1.0, 0.25, 1.0]), "shrunk": 0.3 * np.eye(3), "collapsed": 0.02 * np.eye(3)}


# ---------------------------------------------------------------- the C ABI
def test_self_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    from pienerf_amd.simulator import solver
    text = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in SELF_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    h = _lib.lib()
    assert h.pn_sim_self_bytes() == solver.SELF_STATE_DOUBLES * 8 == solver.SELF_STATE_DTYPE.itemsize == 56
    assert len(_lib.SIGNATURES["pn_sim_self_rhs"][1]) == 20
    assert "#define PN_SELF_BUCKET_CAP 64" in text and R.BUCKET_CAP == 64
    # positions and velocities, S, a (10 doubles a point), cells and the members twice (6 ints a point), counts [T], starts [T + 1], two flag words
    for n, T in ((1, 1024), (432, 1024), (512, 1024), (513, 2048), (3576, 8192)):
        assert R.n_buckets(n) == T
        assert h.pn_sim_self_work_bytes(n) == (n * 80 + n * 24 + (2 * T + 1) * 4 + 8 + 7) // 8 * 8, n
    assert h.pn_sim_self_work_bytes(0) == 0 and h.pn_sim_self_work_bytes(-1) == 0 and h.pn_sim_self_work_bytes((1 << 27) + 1) == 0
    assert h.pn_sim_self_launches() == 8


def test_packed_state_has_the_headers_layout():
    from pienerf_amd.simulator import solver
    text = _header().replace("int64_t", "double")          # 8 bytes, 8-aligned: what the layout walk needs to know of it
    st, size, _ = _c_layout(text, "pn_selfcontact_state", {})
    dt = solver.SELF_STATE_DTYPE
    assert size == dt.itemsize == 56
    assert [(n, o) for n, o in st] == [(n, dt.fields[n][1]) for n in dt.names]
    b = solver.pack_self_contact_state(1, (0.4, 0.3, 0.2, 0.1, 0.35), overflowed=5)
    assert len(b) == 56 and struct.unpack("<iiq5d", b) == (1, 0, 5, 0.4, 0.3, 0.2, 0.1, 0.35)
    assert struct.unpack("<iiq5d", solver.pack_self_contact_state(0, (0.5, 0.5, 0.0, 0.1, 0.3))) == (0, 0, 0, 0.5, 0.5, 0.0, 0.1, 0.3)


def test_entries_refuse_bad_arguments():
    from pienerf_amd import _lib
    h, d, out = _lib.lib(), ctypes.c_void_p(16), ctypes.c_void_p(32)
    good = (0.5, 0.5, 0.0, 0.1, 0.3)

    def setp(state=d, active=1, p=good):
        a = np.array(p, np.float64) if p is not None else None
        return h.pn_sim_self_set_params(state, active, a.ctypes.data if a is not None else None, None)
    assert setp(state=None) == PN_ERR_ARG and setp(active=2) == PN_ERR_ARG and setp(active=-2) == PN_ERR_ARG
    for i in range(5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert setp(p=good[:i] + (bad,) + good[i + 1:]) == PN_ERR_ARG, (i, bad)
    for bad in ((0.0, 0.5, 0.0, 0.1, 0.3), (1.5, 0.5, 0.0, 0.1, 0.3), (0.5, -0.1, 0.0, 0.1, 0.3), (0.5, 1.1, 0.0, 0.1, 0.3), (0.5, 0.5, -1.0, 0.1, 0.3),
                (0.5, 0.5, 0.0, 0.0, 0.3), (0.5, 0.5, 0.0, -0.1, 0.3), (0.5, 0.5, 0.0, 0.1, 0.05)):     # kappa, beta, mu, h > 0, rho_x >= h
        assert setp(p=bad) == PN_ERR_ARG, bad
    assert b"argument check failed" in h.pn_last_error()

    def rhs(n_k=4, n_IP=3, dt=1e-2, dx=0.1, null=None, rin=d, rout=out):
        # state, work | dof, dof_vel, X_rest, topo, rho, Nx, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out, accel_out
        p = [d] * 12 + [rin, rout, d]
        if null is not None:
            p[null] = None
        return h.pn_sim_self_rhs(n_k, n_IP, p[0], p[1], dt, dx, *p[2:], None)
    for i in range(14):
        assert rhs(null=i) == PN_ERR_ARG, i                                                      # a NULL pointer, whichever (accel_out may be NULL)
    assert rhs(rout=d) == PN_ERR_ARG                                                             # rhs_out is another buffer than rhs_in
    assert rhs(dt=0.0) == PN_ERR_ARG and rhs(dt=-1.0) == PN_ERR_ARG and rhs(dt=float("nan")) == PN_ERR_ARG
    assert rhs(dx=0.0) == PN_ERR_ARG and rhs(dx=-1.0) == PN_ERR_ARG
    assert rhs(n_k=0) == PN_ERR_ARG and rhs(n_IP=0) == PN_ERR_ARG


# ---------------------------------------------------------------- the Simulator's side
def test_self_contact_state_machine_on_cpu():
    from pienerf_amd.simulator import solver
    s = _cpu_sim()
    assert not s.self_contact_enabled
    for call in (lambda: s.set_self_contact_params(stiffness=1.0), s.stop_self_contact, s.self_contact_accel, s.self_contact_count, s.self_contact_overflows,
                 s.self_contact_state_bytes):
        with pytest.raises(RuntimeError, match="enable_self_contact"):   # setters and getters before enabling
            call()
    assert s.enable_self_contact() is s and s.self_contact_enabled and s._self_state is None   # before initialize(): allocated by initialize() on a GPU
    assert np.array_equal(s._self_params, [0.5, 0.5, 0.0, s.dx, 3 * s.dx]) and s.dx == 0.1       # the defaults: thickness dx, exclusion 3 dx
    for call in (s.self_contact_accel, s.self_contact_count, s.self_contact_overflows):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert s.self_contact_state_bytes() == solver.pack_self_contact_state(1, (0.5, 0.5, 0.0, 0.1, 3 * 0.1))
    s.set_self_contact_params(friction=0.5, exclusion=0.45)                                     # what is left out keeps its value
    assert np.array_equal(s._self_params, [0.5, 0.5, 0.5, 0.1, 0.45])
    s.stop_self_contact()
    assert struct.unpack_from("<ii", s.self_contact_state_bytes(), 0) == (0, 0)                 # inactive; the parameters stay
    assert s.self_contact_state_bytes(overflowed=3) == solver.pack_self_contact_state(0, (0.5, 0.5, 0.5, 0.1, 0.45), 3)
    s.enable_self_contact(thickness=0.08)                                                       # switches it on again, exclusion 3 x thickness
    assert np.array_equal(s._self_params, [0.5, 0.5, 0.0, 0.08, 3.0 * 0.08]) and struct.unpack_from("<ii", s.self_contact_state_bytes(), 0) == (1, 0)
    before = s.self_contact_state_bytes()
    for bad in (dict(stiffness=0.0), dict(stiffness=1.5), dict(damping=-0.1), dict(damping=1.1), dict(friction=-1.0), dict(thickness=0.0), dict(thickness=-1.0),
                dict(exclusion=0.01), dict(thickness=1.0), dict(stiffness=float("nan")), dict(exclusion=float("inf"))):
        with pytest.raises(ValueError, match="self-contact"):
            s.set_self_contact_params(**bad)
        if bad != dict(thickness=1.0):                                                          # (enable's exclusion follows a new thickness)
            with pytest.raises(ValueError, match="self-contact"):
                _cpu_sim().enable_self_contact(**bad)
    assert s.self_contact_state_bytes() == before                                               # a refused change changes nothing


def test_self_contact_enabled_before_initialize_builds_the_tables(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud

    def sim():
        s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                      base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
        s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
        return s
    early = sim().enable_self_contact()
    early.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    late = sim()
    late.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert late.Nx_csr is None and not late.self_contact_enabled
    late.enable_self_contact()                                                                  # builds contact's tables when they are not there
    for s in (early, late):
        assert tuple(s.Nx_csr.shape) == (8 * s.n_IP, 10) and not s.contact_enabled and not s.fields_enabled
        assert np.array_equal(s.Nx_csr.numpy(), s.IP_Nx.numpy().reshape(-1, 10)[s.buffer.numpy().astype(np.int64)])
    assert early.self_contact_state_bytes() == late.self_contact_state_bytes()


# ---------------------------------------------------------------- main_render's arguments, the scene's blocks
def test_main_render_arguments_become_the_same_call():
    from pienerf_amd import main_render
    ap = main_render.parser()
    a = ap.parse_args(["--self_contact", "--self_thickness", "0.08", "--self_exclusion", "0.3", "--self_stiffness", "0.7", "--self_damping", "0.2",
                       "--self_friction", "0.4"])
    s = _cpu_sim()
    assert main_render.configure_self_contact(s, a) and s.self_contact_enabled
    assert s.self_contact_state_bytes() == _cpu_sim().enable_self_contact(0.7, 0.2, 0.4, 0.08, 0.3).self_contact_state_bytes()
    s = _cpu_sim()
    main_render.configure_self_contact(s, ap.parse_args(["--self_contact"]))                     # the defaults
    assert s.self_contact_state_bytes() == _cpu_sim().enable_self_contact().self_contact_state_bytes()
    s = _cpu_sim()
    assert not main_render.configure_self_contact(s, ap.parse_args([])) and not s.self_contact_enabled   # nothing asked for: nothing enabled
    for flag in ("--self_thickness", "--self_exclusion", "--self_stiffness", "--self_damping", "--self_friction"):
        with pytest.raises(SystemExit, match="need --self_contact"):                             # a usage error, not a traceback
            main_render.configure_self_contact(_cpu_sim(), ap.parse_args([flag, "0.5"]))
        with pytest.raises(SystemExit, match="need --self_contact"):
            main_render.run(ap.parse_args([flag, "0.5"]))                                        # ... before anything is built
    with pytest.raises(SystemExit, match="self-contact: .*exclusion"):
        main_render.configure_self_contact(_cpu_sim(), ap.parse_args(["--self_contact", "--self_exclusion", "0.01"]))
    # it composes with the other scripted inputs
    a = ap.parse_args(["--self_contact", "--wind", "5", "0", "0", "--floor", "-0.9", "--unpin", "--pin_shake", "0.05", "0", "0", "4", "--save_ply", "--video"])
    assert a.self_contact and main_render.wants_fields(a) and main_render.wants_contact(a)


def test_blocks_concatenate_into_one_cloud(small_cloud):
    from pienerf_amd import scene
    a = scene.make_block_points((-0.3, -0.6, -0.3), (0.3, -0.3, 0.3), sub_res=30, pinned=True)
    b = scene.make_block_points((-0.2, 0.1, -0.2), (0.2, 0.4, 0.2), sub_res=30)
    assert set(a) == set(small_cloud) and all(len(a[k]) == len(a["pos"]) for k in a)
    assert a["pin"].all() and not b["pin"].any() and a["pin"].dtype == small_cloud["pin"].dtype
    assert a["pos"][:, 1].max() < -0.3 and b["pos"][:, 1].min() > 0.1 and (a["mass"] > 0).all()
    both = scene.concat_clouds(a, b)
    assert len(both["pos"]) == len(a["pos"]) + len(b["pos"]) and np.array_equal(both["pos"][len(a["pos"]):], b["pos"])
    with pytest.raises(ValueError):
        scene.make_block_points((0.0, 0.0, 0.0), (0.001, 0.001, 0.001), sub_res=30)


# ---------------------------------------------------------------- the law's invariants, on the reference alone
@pytest.fixture(scope="module")
def chair(small_cloud, small_opt):
    """The small chair's tables (oracle), and for every global map x = A X the points' state with random dof_vel."""
    ref = make_oracle_sim(small_cloud, small_opt)
    assert (ref.n_IP, ref.n_k) == (432, 139) and ref.dx == 0.1
    topo, Nx = ref.IP_kernel.numpy(), ref.IP_Nx
    X = np.asarray(ref.IP_pos, np.float64)
    m = np.asarray(ref.IP_rho, np.float64) * ref.dx ** 3
    vel = np.random.default_rng(5).normal(scale=0.5, size=ref.dof.size)
    state = {}
    for name, A in MAPS.items():
        x, v = ip_state(topo, Nx, R.global_map(np.asarray(ref.kernel_pos, np.float64), A).reshape(-1), vel)
        assert np.abs(x - X @ A.T).max() < 1e-14                  # the dofs written really are the global map
        state[name] = (x, v)
    return dict(ref=ref, X=X, m=m, state=state, par=R.params(ref.dx))


def test_overflow_decision_through_the_stated_hash(chair):
    h = chair["par"]["h"]
    got = {name: R.overflows(*chair["state"][name], h) for name in MAPS}
    print("map: (overflow, largest bucket, most points in one cell)", got)
    assert [got[n][0] for n in ("rest", "squeezed", "shrunk", "collapsed")] == [False, False, False, True]
    assert [got[n][2] for n in ("rest", "squeezed", "shrunk", "collapsed")] == [1, 4, 17, 86]
    a, S, _ = R.self_accel(*chair["state"]["collapsed"], chair["X"], chair["m"], chair["ref"].dt, **chair["par"])
    assert not a.any() and not S.any()                            # an overflowed call adds exactly nothing
    # the hash itself, on cells worked out by hand (uint32 wrap-around included)
    assert int(R.bucket_of(np.array([1, 2, 3]), 1024)) == ((73856093 ^ (2 * 19349663) ^ (3 * 83492791)) & 1023)
    assert int(R.bucket_of(np.array([-1, 0, 0]), 1 << 20)) == ((0xFFFFFFFF * 73856093) & 0xFFFFFFFF) & ((1 << 20) - 1)
    # a point that is not finite takes no part
    x, v = (t.copy() for t in chair["state"]["squeezed"])
    x[7, 1], v[11, 0] = np.nan, np.inf
    a, S, part = R.self_accel(x, v, chair["X"], chair["m"], chair["ref"].dt, **chair["par"])
    assert not a[7].any() and not a[11].any() and S[7] == 0.0 and S[11] == 0.0 and np.isfinite(a).all()
    assert all(j not in (7, 11) for ps in part for j, _, _ in ps)


def test_zero_term_at_rest(chair):
    a, S, part = R.self_accel(*chair["state"]["rest"], chair["X"], chair["m"], chair["ref"].dt, **chair["par"])
    assert not a.any() and not S.any() and not any(part)


@pytest.mark.parametrize("name", ["squeezed", "shrunk"])
@pytest.mark.parametrize("mu", [0.0, 0.5])
def test_momentum_weights_and_continuity(chair, name, mu):
    x, v = chair["state"][name]
    X, m, dt, par = chair["X"], chair["m"], chair["ref"].dt, dict(chair["par"], mu=mu)
    a, S, part = R.self_accel(x, v, X, m, dt, **par)
    pairs = sum(len(p) for p in part) // 2
    print(f"{name}, mu = {mu}: {pairs} contacting pairs, {sum(1 for p in part if p)} points in contact, at most {max(len(p) for p in part)} partners, "
          f"max |a| {np.abs(a).max():.3e}")
    assert pairs > 100 and np.abs(a).max() > 1.0
    ma = m[:, None] * a
    assert np.abs(ma.sum(axis=0)).max() <= 1e-12 * np.abs(ma).sum()                    # no net momentum
    w = R.pair_weights(part, S)
    assert all(w[(i, j)] == w[(j, i)] for i, j in w)                                   # symmetric
    for i, ps in enumerate(part):
        assert sum(w[(i, j)] for j, _, _ in ps) <= 1.0 + 1e-12                         # sum_j w_ij <= 1 ...
        if ps:
            assert sum(w[(i, j)] * d for j, d, _ in ps) <= max(d for _, d, _ in ps) * (1.0 + 1e-12)   # ... so the total response is at most the deepest overlap's
    # continuity: one more point, eligible for everybody, at delta <= 1e-14 h from the body's outermost point and beyond h of nobody's reach
    h = par["h"]
    i = int(np.argmax(np.where(S > 0.0, x[:, 0], -np.inf)))
    assert x[i, 0] == x[:, 0].max()
    x2 = np.vstack([x, x[i] + np.array([h * (1.0 - 1e-14), 0.0, 0.0])])
    v2, X2, m2 = np.vstack([v, [[0.3, -0.2, 0.1]]]), np.vstack([X, [[50.0, 50.0, 50.0]]]), np.append(m, m[i])
    a2, S2, part2 = R.self_accel(x2, v2, X2, m2, dt, **par)
    assert any(j == len(x) for j, _, _ in part2[i]) and 0.0 < S2[-1] <= 1e-13 * h      # it is a partner, barely
    assert np.abs(a2[:-1] - a).max() <= 1e-12 * np.abs(a).max()
