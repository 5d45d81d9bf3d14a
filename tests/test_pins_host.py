"""Kinematic pins, host side, on CPU (no kernel is launched): the C ABI and its argument checks, the Simulator's state machine, and the numpy restatement of
the motion and of its right-hand-side term (csrc/pn_pins.hip, Simulator.enable_pin_motion) checked against physics on the CPU oracle.
tests/test_gpu_pins.py imports the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_oracle_sim

PIN_SYMBOLS = ("pn_sim_pins_bytes", "pn_sim_pins_set", "pn_sim_pins_clock", "pn_sim_pins_rhs")
PN_ERR_ARG = 1


# ---------------------------------------------------------------- the motion and its right-hand-side term, in numpy
def pin_u(X, t, translate=None, rotate=None, offsets=None):
    """u_p(t) = offset_p + T(t) + R(t)(X_p - c) - (X_p - c) for the rest positions X [n_pin, 3].  translate = (A, hz, phase); rotate = (axis, degrees,
    hz, phase, centre) with R(t) the Rodrigues rotation about axis / |axis| by degrees sin(2 pi hz t + phase)."""
    X = np.asarray(X, np.float64)
    u = np.zeros_like(X)
    if translate is not None:
        A, hz, ph = translate
        u += np.asarray(A, np.float64)[None, :] * np.sin(2 * np.pi * hz * t + ph)
    if rotate is not None:
        axis, deg, hz, ph, c = rotate
        n = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        a = np.deg2rad(deg) * np.sin(2 * np.pi * hz * t + ph)
        v = X - np.asarray(c, np.float64)[None, :]
        Rv = v * np.cos(a) + np.cross(n[None, :], v) * np.sin(a) + n[None, :] * (v @ n)[:, None] * (1.0 - np.cos(a))
        u += Rv - v
    if offsets is not None:
        u += np.asarray(offsets, np.float64)
    return u


def pin_term(n_k, stiff, pin_kernel, pin_Nx, u):
    """stiff sum_p N_p^T u_p as [10 n_k, 3] (the layout of dof): row kernel 10 + basis, over the pins' pts_kernel [n_pin, 8] / pts_Nx [n_pin, 8, 10] rows."""
    out = np.zeros((n_k * 10, 3))
    rows = (np.asarray(pin_kernel, np.int64)[:, :, None] * 10 + np.arange(10)[None, None, :]).reshape(-1)
    np.add.at(out, rows, (np.asarray(pin_Nx, np.float64)[:, :, :, None] * u[:, None, None, :]).reshape(-1, 3))
    return stiff * out


def oracle_pins(ref):
    """(pin ids, pts_kernel rows, pts_Nx rows, rest positions) of an OracleSimulator."""
    vid = np.nonzero(ref.is_pin.numpy())[0]
    return vid, ref.pts_kernel.numpy()[vid], np.asarray(ref.pts_Nx)[vid], ref.pos.numpy()[vid].copy()


def pin_positions(ref, kern, Nx):
    """The pinned points' current positions sum_i sum_b N[p, i, b] dof[kernel[p, i] 10 + b] (update_pos_kernel)."""
    d = ref.dof.reshape(ref.n_k, 10, 3)[kern.astype(np.int64)]
    return np.einsum("pib,pibr->pr", Nx, d)


# ---------------------------------------------------------------- the C ABI
def test_pin_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in PIN_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    assert "pn_pin_motion" in text
    # the size Python allocates (Simulator._alloc_pins: PIN_STATE_DOUBLES doubles)
    from pienerf_amd.simulator import solver
    assert _lib.lib().pn_sim_pins_bytes() == solver.PIN_STATE_DOUBLES * 8 == 128


def _set(state=16, n_pin=4, active=1, A=(0.1, 0.0, 0.0), axis=(0.0, 1.0, 0.0), theta=0.3):
    from pienerf_amd import _lib
    T = np.array(list(A) + [2.0, 0.0])
    R = np.array(list(axis) + [theta, 1.0, 0.0, 0.0, 0.0, 0.0])
    return _lib.lib().pn_sim_pins_set(ctypes.c_void_p(state) if state else None, n_pin, active, T.ctypes.data, R.ctypes.data, None)


def test_set_refuses_bad_arguments():
    assert _set(state=0) == PN_ERR_ARG                                  # no state
    assert _set(n_pin=0) == PN_ERR_ARG
    assert _set(A=(0.1, float("nan"), 0.0)) == PN_ERR_ARG                # non-finite amplitude
    assert _set(A=(float("inf"), 0.0, 0.0)) == PN_ERR_ARG
    assert _set(axis=(0.0, 2.0, 0.0)) == PN_ERR_ARG                      # not a unit axis, theta != 0
    assert _set(axis=(0.0, 0.0, 0.0)) == PN_ERR_ARG
    assert _set(theta=float("nan")) == PN_ERR_ARG
    assert _set(active=2) == PN_ERR_ARG
    from pienerf_amd import _lib
    assert b"argument check failed" in _lib.lib().pn_last_error()


def test_clock_and_rhs_refuse_bad_arguments():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)
    assert h.pn_sim_pins_clock(None, 0, None) == PN_ERR_ARG              # no state
    assert h.pn_sim_pins_clock(d, -1, None) == PN_ERR_ARG
    rhs = lambda n_k=4, n_pin=3, state=d, dt=1e-2, stiff=1e5, out=d: h.pn_sim_pins_rhs(n_k, n_pin, state, dt, stiff, d, d, d, d, d, None, out, None)
    assert rhs(state=None) == PN_ERR_ARG                                 # no state
    assert rhs(n_pin=0) == PN_ERR_ARG
    assert rhs(n_k=0) == PN_ERR_ARG
    assert rhs(dt=float("nan")) == PN_ERR_ARG
    assert rhs(stiff=float("inf")) == PN_ERR_ARG
    assert rhs(out=None) == PN_ERR_ARG


# ---------------------------------------------------------------- the Simulator's state machine
def test_pin_motion_state_machine_on_cpu(small_cloud):
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(device="cpu", persistent=False)
    assert not s.pin_enabled
    for call in (lambda: s.set_pin_motion(translate=((0.1, 0.0, 0.0), 2.0)), lambda: s.set_pin_offsets(np.zeros((1, 3))), s.stop_pin_motion,
                 s.reset_pin_clock, s.pin_clock):
        with pytest.raises(RuntimeError, match="enable_pin_motion"):   # setters before enabling
            call()
    assert s.enable_pin_motion() is s and s.pin_enabled and s._pin_state is None   # before initialize(): allocated by initialize() on a GPU
    with pytest.raises(RuntimeError, match="GPU"):
        s.set_pin_motion(translate=((0.1, 0.0, 0.0), 2.0))
    with pytest.raises(RuntimeError, match="GPU"):
        s.pin_clock()


def test_motion_tuples_of_every_documented_length():
    """translate = (A, hz[, phase]), rotate = (axis, degrees, hz[, phase[, centre]]): what is left out is 0 / the default centre; anything else is a
    ValueError that says which."""
    from pienerf_amd.simulator.solver import pin_motion_params
    cen = lambda: np.array([1.0, 2.0, 3.0])
    T, R = pin_motion_params(((0.1, 0.2, 0.3), 2.0), ((0.0, 3.0, 4.0), 90.0, 1.5), cen)
    assert np.array_equal(T, [0.1, 0.2, 0.3, 2.0, 0.0])
    assert np.allclose(R, [0.0, 0.6, 0.8, np.pi / 2, 1.5, 0.0, 1.0, 2.0, 3.0], rtol=0, atol=1e-15)
    T, R = pin_motion_params(((0.1, 0.2, 0.3), 2.0, 0.7), ((0.0, 3.0, 4.0), 90.0, 1.5, 0.25), cen)          # phase given, centre left out
    assert T[4] == 0.7 and R[5] == 0.25 and np.array_equal(R[6:], [1.0, 2.0, 3.0])
    _, R = pin_motion_params(None, ((0.0, 3.0, 4.0), 90.0, 1.5, 0.25, None), cen)
    assert np.array_equal(R[6:], [1.0, 2.0, 3.0])
    T, R = pin_motion_params(None, ((0.0, 3.0, 4.0), 90.0, 1.5, 0.25, (-1.0, 0.5, 0.0)), cen)
    assert np.array_equal(R[6:], [-1.0, 0.5, 0.0]) and not T.any()
    T, R = pin_motion_params(None, None, cen)
    assert not T.any() and R[3] == 0.0 and abs(np.linalg.norm(R[:3]) - 1.0) < 1e-15                         # no motion: still a unit axis
    for bad, what in ((dict(translate=((0.1, 0.2, 0.3),)), "translate is"), (dict(translate=((0.1, 0.2, 0.3), 1.0, 0.0, 0.0)), "translate is"),
                      (dict(translate=((0.1, 0.2), 1.0)), "3-vector"), (dict(rotate=((0.0, 1.0, 0.0), 10.0)), "rotate is"),
                      (dict(rotate=((0.0, 1.0, 0.0), 10.0, 1.0, 0.0, (0.0, 0.0, 0.0), 1.0)), "rotate is"), (dict(rotate=((0.0, 1.0), 10.0, 1.0)), "3-vector"),
                      (dict(rotate=((0.0, 1.0, 0.0), 10.0, 1.0, 0.0, 0.0)), "3-vector"), (dict(rotate=((0.0, 0.0, 0.0), 10.0, 1.0)), "nonzero"),
                      (dict(translate=((0.1, float("nan"), 0.0), 1.0)), "finite")):
        with pytest.raises(ValueError, match=what):
            pin_motion_params(bad.get("translate"), bad.get("rotate"), cen)


def test_a_cloud_without_pins_is_refused(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud

    def sim():
        s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                      base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
        s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
        return s
    a = sim()
    a.enable_pin_motion()             # enabled first: refused when the cloud arrives
    with pytest.raises(ValueError, match="pinned"):
        a.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], np.zeros_like(c["pin"]))
    b = sim()
    b.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], np.zeros_like(c["pin"]))
    with pytest.raises(ValueError, match="pinned"):
        b.enable_pin_motion()
    assert not b.pin_enabled
    # with pins: the rest positions are a copy of their own, the CSR holds every (pin, slot) pair once, ascending inside a kernel's run
    g = sim()
    g.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    g.enable_pin_motion()
    vid = np.nonzero(c["pin"])[0]
    assert g.n_pin == len(vid) > 0 and np.array_equal(g.pin_rest.numpy(), np.asarray(c["pos"], np.float64)[vid])
    assert g.pin_rest.data_ptr() != g.pos.data_ptr()
    bg, of = g.pin_bg.numpy(), g.pin_of.numpy()
    assert bg[0] == 0 and bg[-1] == 8 * g.n_pin and len(bg) == g.n_k + 1 and (np.diff(bg) >= 0).all()
    kern = g.pin_kernel.numpy()
    for k in np.nonzero(np.diff(bg))[0]:
        run = of[bg[k]:bg[k + 1]]
        assert (np.diff(run) >= 0).all() and all((kern[p] == k).any() for p in run)
    assert np.array_equal(np.sort(np.bincount(of, minlength=g.n_pin)), np.full(g.n_pin, 8))


def test_the_kernels_order_of_summation_walked_in_numpy(small_opt):
    """csrc/pn_pins.hip's k_pin_rhs walked in numpy over the simulator's own tables (pin_bg / pin_of / pin_N_csr / pin_rest): 64 lanes striding each
    kernel's run in ascending order, the shuffle tree 32, 16 ... 1, (R - I)v as (n x v) sin a + (n (n.v) - v) 2 sin^2(a / 2).  On the 744-pin set (runs
    of up to 200 entries, ragged last passes) it equals the np.add.at restatement to round-off: the tables and the formula are the term."""
    import torch
    from pienerf_amd import scene
    from pienerf_amd.simulator.solver import Simulator, pin_motion_params
    o = small_opt
    c = scene.make_chair_points(sub_res=30, pin_height=1.0, hgs=o["hash_grid_size"])
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
    s.initialize = s.precompute
    s.enable_pin_motion()
    s.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    bg, of, N, X = s.pin_bg.numpy(), s.pin_of.numpy(), s.pin_N_csr.numpy(), s.pin_rest.numpy()
    assert s.n_pin == 744 and np.diff(bg).max() == 200
    off = np.random.default_rng(5).normal(scale=0.02, size=X.shape)
    tr, ro = ((0.05, 0.02, -0.03), 4.0, 0.3), ((0.2, 1.0, -0.1), 12.0, 3.0, 0.5, X.mean(axis=0) + 0.1)
    T, R = pin_motion_params(tr, ro, None)
    t = (37 + 1) * s.dt
    Tt = T[:3] * np.sin((2 * np.pi * T[3]) * t + T[4])
    a = R[3] * np.sin((2 * np.pi * R[4]) * t + R[5])
    n, cen, sa, ca1 = R[:3], R[6:], np.sin(a), 2.0 * np.sin(0.5 * a) ** 2
    out = np.zeros((s.n_k, 30))
    for kid in range(s.n_k):
        lanes = np.zeros((64, 30))
        for e in range(bg[kid], bg[kid + 1]):
            v = X[of[e]] - cen
            u = Tt + np.cross(n, v) * sa + (n * (n @ v) - v) * ca1 + off[of[e]]
            lanes[(e - bg[kid]) % 64] += np.outer(N[e], u).reshape(-1)
        w = 32
        while w:
            lanes[:w] += lanes[w:2 * w]
            w //= 2
        out[kid] = s.stiff * lanes[0]
    want = pin_term(s.n_k, s.stiff, s.pin_kernel.numpy(), s.pin_Nx.numpy(), pin_u(X, t, translate=tr, rotate=ro, offsets=off))
    err = float(np.abs(out.reshape(-1, 3) - want).max() / np.abs(want).max())
    print(f"kernel-order walk vs np.add.at restatement: rel err {err:.2e}")
    assert err < 1e-13   # fp64 sums of at most 200 terms of one sign pattern each: a few hundred ulps at the very most


# ---------------------------------------------------------------- the restatement against physics (oracle only)
def test_constant_pin_displacement_carries_the_object_on_the_oracle(small_cloud, small_opt):
    """Gravity off, every pin given u = (0.05, 0.02, -0.03) through the right-hand-side term alone: the pinned points arrive at X_p + u through the
    penalty's transient (max |x_p - X_p - u| / |u| over the pins: > 0.1 after one substep, <= 0.05 after 60) and the object follows its base."""
    ref = make_oracle_sim(small_cloud, small_opt)
    vid, kern, Nx, X = oracle_pins(ref)
    assert len(vid) == 16
    u = np.array([0.05, 0.02, -0.03])
    U = pin_u(X, 0.0, offsets=np.tile(u, (len(vid), 1)))
    assert np.array_equal(U, np.tile(u, (len(vid), 1)))
    ref.rhs_gravity = pin_term(ref.n_k, ref.stiff, kern, Nx, U)   # g0 = 0
    assert np.abs(pin_positions(ref, kern, Nx) - X).max() < 1e-12
    err = []
    for k in range(60):
        ref.stepforward()
        err.append(float(np.abs(pin_positions(ref, kern, Nx) - X - u[None, :]).max() / np.linalg.norm(u)))
    print(f"pins' max |x_p - X_p - u| / |u|: {err[0]:.4f} after 1 substep, {err[9]:.4f} after 10, {err[59]:.4f} after 60")
    assert err[0] > 0.1
    assert err[59] <= 0.05
    # the 50 top-most points moved with the base
    pos = ref.pos.numpy()
    top = np.argsort(-pos[:, 1])[:50]
    d = ref.dof.reshape(ref.n_k, 10, 3)[ref.pts_kernel.numpy()[top].astype(np.int64)]
    moved = (np.einsum("pib,pibr->pr", np.asarray(ref.pts_Nx)[top], d) - pos[top]).mean(axis=0)
    print("mean displacement of the 50 top-most points:", moved)
    assert np.abs(moved - u).max() < 0.1 * np.linalg.norm(u)


def test_rotation_restatement_is_a_rotation():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(7, 3))
    c = np.array([0.1, -0.2, 0.3])
    rot = ((1.0, 2.0, -0.5), 40.0, 1.5, 0.2, c)
    t = 0.37
    Y = X + pin_u(X, t, rotate=rot)
    assert np.allclose(np.linalg.norm(Y - c, axis=1), np.linalg.norm(X - c, axis=1), rtol=0, atol=1e-14)   # distances to the centre kept
    n = np.array(rot[0]) / np.linalg.norm(rot[0])
    assert np.allclose((Y - c) @ n, (X - c) @ n, rtol=0, atol=1e-14)                                        # ... and the component along the axis
    a = np.deg2rad(40.0) * np.sin(2 * np.pi * 1.5 * t + 0.2)
    p, q = (X - c) - ((X - c) @ n)[:, None] * n, (Y - c) - ((Y - c) @ n)[:, None] * n
    assert np.allclose(np.einsum("ij,ij->i", p, q), np.cos(a) * np.einsum("ij,ij->i", p, p), rtol=0, atol=1e-13)
    assert np.allclose(np.einsum("ij,j->i", np.cross(p, q), n), np.sin(a) * np.einsum("ij,ij->i", p, p), rtol=0, atol=1e-13)   # right-handed about n
    assert np.array_equal(pin_u(X, 0.0, translate=((0.3, 0.0, 0.0), 2.0, 0.0)), np.zeros_like(X))
