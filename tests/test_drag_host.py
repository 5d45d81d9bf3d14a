"""The device mouse drag's host side, on CPU (no kernel is launched): the C ABI, its argument checks, the wheel rule and the Simulator's drag state
machine (csrc/pn_drag.hip, Simulator.enable_drag)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

DRAG_SYMBOLS = ("pn_sim_drag_bytes", "pn_sim_drag_work_doubles", "pn_sim_drag_force", "pn_sim_drag_set", "pn_sim_drag_unproject")
PN_ERR_ARG = 1


def test_drag_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in DRAG_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    h = _lib.lib()
    assert h.pn_sim_drag_bytes() == 40 and h.pn_sim_drag_work_doubles() >= 2


def _unproject(x, y, W=8, H=8, intr=(10.0, 10.0, 4.0, 4.0), n_IP=0, drag=16):
    from pienerf_amd import _lib
    d = ctypes.c_void_p(16)
    i4 = np.ascontiguousarray(intr, np.float64)
    p16 = np.ascontiguousarray(np.eye(4), np.float64)
    return _lib.lib().pn_sim_drag_unproject(d, W, H, float(x), float(y), i4.ctypes.data, p16.ctypes.data, d if n_IP else None, n_IP,
                                            ctypes.c_void_p(drag) if drag else None, d, None)


@pytest.mark.parametrize("x,y", [(-0.5, 2.0), (8.0, 2.0), (2.0, 8.0), (2.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))])
def test_unproject_refuses_a_pixel_outside_the_image(x, y):
    assert _unproject(x, y) == PN_ERR_ARG


def test_unproject_refuses_bad_arguments():
    assert _unproject(1.0, 1.0, drag=0) == PN_ERR_ARG                     # no drag state
    assert _unproject(1.0, 1.0, W=8, H=6) == PN_ERR_ARG                   # 2 int(cx) x 2 int(cy) != W H (the reference's reshape would fail)
    assert _unproject(1.0, 1.0, intr=(0.0, 10.0, 4.0, 4.0)) == PN_ERR_ARG  # fx = 0
    from pienerf_amd import _lib
    d = ctypes.c_void_p(16)
    i4 = np.array([10.0, 10.0, 4.0, 4.0])
    p16 = np.eye(4)
    assert _lib.lib().pn_sim_drag_unproject(d, 8, 8, 1.0, 1.0, i4.ctypes.data, p16.ctypes.data, None, 5, d, d, None) == PN_ERR_ARG  # pick, no IPs


def test_set_and_force_refuse_bad_arguments():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)
    assert h.pn_sim_drag_set(d, 10, 10, 1, 1.0, None, None) == PN_ERR_ARG          # vid out of range
    assert h.pn_sim_drag_set(None, 10, 3, 1, 1.0, None, None) == PN_ERR_ARG        # no drag state
    assert h.pn_sim_drag_set(d, 10, 3, 2, 1.0, None, None) == PN_ERR_ARG           # active is 0 or 1
    assert h.pn_sim_drag_set(d, 10, 3, 1, float("inf"), None, None) == PN_ERR_ARG
    t = np.array([0.0, np.nan, 0.0])
    assert h.pn_sim_drag_set(d, 10, 3, 1, 1.0, t.ctypes.data, None) == PN_ERR_ARG  # non-finite target
    assert h.pn_sim_drag_force(4, 10, None, d, 0.1, d, d, d, d, None) == PN_ERR_ARG  # no drag state
    assert h.pn_sim_drag_force(4, 0, d, d, 0.1, d, d, d, d, None) == PN_ERR_ARG


def test_wheel_rule():
    """gui.py:857-865: +-0.5 per notch above 1, +-0.1 at or below 1, clamped to [1e-3, 50]."""
    from pienerf_amd.simulator.solver import wheel_force_scale
    assert wheel_force_scale(1.0, 1) == pytest.approx(1.1)
    assert wheel_force_scale(1.1, 1) == pytest.approx(1.6)
    assert wheel_force_scale(2.0, -1) == pytest.approx(1.5)
    assert wheel_force_scale(1.0, -1) == pytest.approx(0.9)
    assert wheel_force_scale(0.05, -1) == 1e-3
    assert wheel_force_scale(49.8, 3) == 50.0
    s = 1.0
    for _ in range(200):
        s = wheel_force_scale(s, 1)
    assert s == 50.0


def test_drag_owns_dof_f_and_can_be_enabled_before_initialize():
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(device="cpu", persistent=False)
    assert not s.drag_enabled
    s.enable_drag(scale=2.5)
    assert s.drag_enabled and s.drag_force_scale == 2.5 and s._drag is None   # allocated by initialize() on a GPU
    with pytest.raises(RuntimeError, match="drag"):
        s.update_force(0, np.array([1.0, 2.0, 3.0]))
    with pytest.raises(RuntimeError, match="drag"):
        s.clear_force()
    with pytest.raises(RuntimeError, match="GPU"):
        s.release()
    with pytest.raises(ValueError):
        s.enable_drag(scale=0.0)
    assert s.enable_drag() is s and s.drag_force_scale == 2.5
    t = Simulator(device="cpu", persistent=False)
    with pytest.raises(RuntimeError, match="enable_drag"):
        t.release()
