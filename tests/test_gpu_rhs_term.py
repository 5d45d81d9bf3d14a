"""The device code the simulator's right-hand-side stages share (csrc/pn_sim_rhs.h) and the scaffold they share in Python (simulator/_stage.py): the
per-kernel sum on its own (pn_sim_accel_rhs) on synthetic tables whose runs cover every path of the workgroup's stride loop; the same sum behind
contact, force fields and self-contact, bit for bit; and Simulator.keep_state / restore_state."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from contact_reference import contact_term
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from test_gpu_fields import GUSTY, _bits, _neg_zeros, _sim
from test_gpu_parity import DEV
from test_gpu_selfcontact import BALL, FLOOR, SHAKE, SHELL, SQUEEZED, WIND, _dev, _map_dof, _set_state

pytestmark = pytest.mark.gpu


def _accel_rhs(n_k, n_IP, dx, rho, bg, cnt, buf, csr, accel, g, out):
    check(lib().pn_sim_accel_rhs(n_k, n_IP, float(dx), ptr(rho), ptr(bg), ptr(cnt), ptr(buf), ptr(csr), ptr(accel), ptr(g), ptr(out), stream_ptr()),
          "sim_accel_rhs")
    return out


# ---------------------------------------------------------------- 1: the shared sum on synthetic tables
RUNS = [600, 0, 1, 256, 257, 6]   # > 2 passes and no multiple of 64 | empty | one lane | exactly one pass | one pass + 1 | less than a wave


def test_the_shared_sum_on_runs_of_every_kind():
    """n_k = 6, n_IP = 140: the 1120 (point, slot) entries are dealt to the kernels at random so that the runs have the lengths RUNS.  Every point of
    the 6-entry run has accel = 0, so that run adds nothing; a few single components elsewhere are -0.0, which is a zero to the a == 0 skip and a
    factor like any other where the point's other components are not zero."""
    n_k, n_IP, dx = 6, 140, 0.1
    rng = np.random.default_rng(47)
    topo = rng.permutation(np.repeat(np.arange(n_k), RUNS)).astype(np.int32).reshape(n_IP, 8)
    Nx = rng.normal(scale=0.4, size=(n_IP, 8, 10))
    rho = rng.uniform(500.0, 1500.0, size=n_IP)
    order = np.argsort(topo.reshape(-1), kind="stable").astype(np.int32)                    # entry = point 8 + slot, by kernel
    cnt = np.bincount(topo.reshape(-1), minlength=n_k).astype(np.int32)
    bg = (np.cumsum(cnt) - cnt).astype(np.int32)
    assert cnt.tolist() == RUNS and sum(RUNS) == 8 * n_IP
    accel = rng.normal(scale=30.0, size=(n_IP, 3))
    quiet = np.unique(np.nonzero(topo == 5)[0])                                             # the points of the 6-entry run
    accel[quiet] = 0.0
    loud = np.setdiff1d(np.arange(n_IP), quiet)
    accel[loud[::9], rng.integers(0, 3, size=loud[::9].size)] = -0.0
    assert 1 <= quiet.size <= 6 and accel[loud].any(axis=1).all() and int(np.signbit(accel[loud]).sum() - (accel[loud] < 0).sum()) >= 10
    g = rng.normal(size=n_k * 30)
    g[rng.random(g.size) < 0.2] = -0.0
    t = dict(rho=_dev(rho), bg=_dev(bg), cnt=_dev(cnt), buf=_dev(order), csr=_dev(Nx.reshape(-1, 10)[order]), accel=_dev(accel), g=_dev(g))
    keep = {k: v.clone() for k, v in t.items()}

    def launch(fill):
        out = torch.full_like(t["g"], fill)
        return _accel_rhs(n_k, n_IP, dx, t["rho"], t["bg"], t["cnt"], t["buf"], t["csr"], t["accel"], t["g"], out)
    out = launch(7.0)
    want = contact_term(n_k, topo, Nx, rho * dx ** 3, accel)
    got = (out - t["g"]).cpu().numpy().reshape(-1, 3)
    e = rel_err(got, want)
    per_run = [float(np.abs(want[k * 10:(k + 1) * 10]).max()) for k in range(n_k)]
    print(f"runs {RUNS}: max|term| per run " + " ".join(f"{v:.2e}" for v in per_run) + f", rel err {e:.2e}")
    assert all(per_run[k] > 1e-3 * max(per_run) for k in (0, 2, 3, 4)) and per_run[1] == 0.0 and per_run[5] == 0.0    # every acting run carries a term
    assert e < 1e-12
    for k in (1, 5):                                                                        # the empty run and the all-zero run: rhs_in, bit for bit
        rows = slice(k * 30, (k + 1) * 30)
        assert torch.equal(_bits(out[rows]), _bits(t["g"][rows]))
        assert bool((out[rows] == 0.0).any()) and bool(torch.signbit(out[rows][out[rows] == 0.0]).all())
    for k, v in t.items():                                                                  # rhs_in, accel and the tables are left alone
        assert torch.equal(_bits(v) if v.dtype == torch.float64 else v, _bits(keep[k]) if v.dtype == torch.float64 else keep[k]), k
    assert torch.equal(_bits(out), _bits(launch(3.0)))                                      # a second run into a buffer that held something else


# ---------------------------------------------------------------- 2: one sum for three stages
def test_contact_fields_and_self_contact_end_in_the_shared_sum(small_cloud, small_opt):
    """The chain's state (tests/test_gpu_selfcontact.py: the squeezed chair with shaken pins, three colliders, a gusty wind, self-contact) after four
    substeps, while every stage acts: a stage's rhs_out is pn_sim_accel_rhs of its own accel buffer and the same rhs_in, bit for bit."""
    s = _sim(small_cloud, small_opt)
    _set_state(s, _map_dof(s, SQUEEZED))
    s.enable_pin_motion()
    s.set_pin_motion(translate=SHAKE)
    s.enable_contact()
    for add, c in ((s.add_plane, FLOOR), (s.add_sphere, BALL), (s.add_sphere, SHELL)):
        add(**c)
    s.enable_fields()
    s.add_wind(**WIND)
    s.enable_self_contact()
    for _ in range(4):
        s.stepforward()
    g = _neg_zeros(s._rhs_ext)
    assert not torch.equal(s._rhs_ext, s.rhs_gravity)                                       # the pins act too: g is a link of the chain
    stages = (("contact", s._enqueue_contact_rhs, s.contact_accel), ("fields", s._enqueue_fields_rhs, s.field_accel),
              ("self-contact", s._enqueue_self_rhs, s.self_contact_accel))
    for name, enqueue, accel in stages:
        out = enqueue(g).clone()
        a = accel()
        n_act = int(a.any(dim=1).sum())
        print(f"{name}: {n_act} of {s.n_IP} points act, max|rhs_out - rhs_in| {float((out - g).abs().max()):.3e}")
        assert 0 < n_act and not torch.equal(_bits(out), _bits(g)), name
        alone = _accel_rhs(s.n_k, s.n_IP, s.dx, s.IP_rho, s.kernel_bg, s.kernel_cnt, s.buffer, s.Nx_csr, a, g, torch.full_like(g, 7.0))
        assert torch.equal(_bits(out), _bits(alone)), name
    assert torch.equal(_bits(s._enqueue_contact_rhs(g, one_launch=True)), _bits(s._enqueue_contact_rhs(g).clone()))   # and contact's one-launch form


# ---------------------------------------------------------------- 3: keep_state / restore_state
def test_restore_state_replays_the_trajectory_and_the_clocks(small_cloud, small_opt):
    """Moving pins and a gusty wind: three substeps, keep_state(), two substeps recorded, restore_state() + reset_warm_start(), the two substeps again:
    the clocks read 3 after the restore and the replay has the first recording's bits.  The SVD warm start is no part of the kept state
    (Simulator.reset_warm_start: a replay's BITS depend on it, at 1e-10 of the displacements), so the first recording starts from a reset warm start
    as well — the capture's situation, where the warm-up's V is forgotten before the first replay.  Without that reset the two recordings differ in
    the last digits (measured: 1e-11 relative), which is the warm start's doing and not restore_state's."""
    s = _sim(small_cloud, small_opt)
    s.enable_pin_motion()
    s.set_pin_motion(translate=SHAKE)
    s.enable_fields()
    s.add_wind(**GUSTY)

    def two_steps():
        rec = []
        for _ in range(2):
            s.stepforward()
            rec.append(s.dof.clone())
        return rec
    for _ in range(3):
        s.stepforward()
    keep = s.keep_state()
    s.reset_warm_start()
    first = two_steps()
    assert (s.pin_clock(), s.field_clock()) == (5, 5)
    s.restore_state(keep)
    s.reset_warm_start()
    assert (s.pin_clock(), s.field_clock()) == (3, 3)
    assert torch.equal(_bits(s.dof), _bits(keep["dof"])) and torch.equal(_bits(s.dof_vel), _bits(keep["dof_vel"]))
    second = two_steps()
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[0], keep["dof"])   # the body moves
    print("replay - first recording, max abs per substep:", [float((a - b).abs().max()) for a, b in zip(first, second)])
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))
    assert (s.pin_clock(), s.field_clock()) == (5, 5)
