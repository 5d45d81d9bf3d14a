"""Kinematic pins: the pinned points follow a scripted motion (csrc/pn_pins.hip).  A pn_pin_motion in device memory with its own
substep clock, read by a k_pin_rhs launch in front of every substep that writes _rhs_ext = rhs_gravity + the pins' right-hand-side term; the substep
then takes _rhs_ext in its rhs_gravity slot."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, npfloat, torchfloat

__all__ = ["PIN_STATE_DOUBLES", "pin_motion_params", "PinsMixin"]   # what solver.py re-exports

PIN_STATE_DOUBLES = 16   # pn_pin_motion (include/pienerf_hip.h) as doubles: 128 bytes = pn_sim_pins_bytes(), checked in _alloc_pins

STAGE = Stage(name="pins", flag="pin_enabled", state="_pin_state", subject="pin motion is", owner="the pin motion's state", enable="enable_pin_motion",
              struct="pn_pin_motion", nbytes=PIN_STATE_DOUBLES * 8, sized_by="solver.py allocates", init="_init_pins", alloc="_alloc_pins",
              enqueue="_enqueue_pin_rhs", tables="_build_pins", writes="rhs", clock=True)


def pin_motion_params(translate, rotate, default_centre):
    """Simulator.set_pin_motion's arguments as the arrays of pn_sim_pins_set (include/pienerf_hip.h): T = (A[3], hz, phase), R = (unit axis[3],
    radians, hz, phase, centre[3]).  translate = (A, hz[, phase]) or None; rotate = (axis, degrees, hz[, phase[, centre]]) or None; `default_centre()`
    gives the centre where it is left out or None.  ValueError for a tuple of another length, a vector that is not a 3-vector, a zero axis with
    degrees != 0, a non-finite value."""
    T, R = np.zeros(5), np.zeros(9)
    R[2] = 1.0
    if translate is not None:
        tr = tuple(translate)
        if not 2 <= len(tr) <= 3:
            raise ValueError(f"set_pin_motion: translate is (A, hz) or (A, hz, phase), got {len(tr)} entries")
        A = np.asarray(tr[0], npfloat)
        if A.size != 3:
            raise ValueError(f"set_pin_motion: the amplitude A of translate is a 3-vector, got shape {A.shape}")
        T[:3], T[3], T[4] = A.reshape(3), float(tr[1]), float(tr[2]) if len(tr) > 2 else 0.0
    if rotate is not None:
        r = tuple(rotate)
        if not 3 <= len(r) <= 5:
            raise ValueError(f"set_pin_motion: rotate is (axis, degrees, hz[, phase[, centre]]), got {len(r)} entries")
        axis, deg, hz = r[:3]
        ph = r[3] if len(r) > 3 else 0.0
        centre = r[4] if len(r) > 4 else None
        axis = np.asarray(axis, npfloat)
        if axis.size != 3 or (centre is not None and np.asarray(centre).size != 3):
            raise ValueError("set_pin_motion: the axis and the centre of rotate are 3-vectors")
        axis = axis.reshape(3)
        n = float(np.linalg.norm(axis))
        if float(deg) != 0.0 and not (np.isfinite(n) and n > 0.0):
            raise ValueError(f"set_pin_motion: the rotation axis must be a finite nonzero vector, got {axis!r}")
        R[:3] = axis / n if n > 0.0 and np.isfinite(n) else (0.0, 0.0, 1.0)
        R[3], R[4], R[5] = np.deg2rad(float(deg)), float(hz), float(ph)
        R[6:] = np.asarray(default_centre() if centre is None else centre, npfloat).reshape(3)
    if not (np.isfinite(T).all() and np.isfinite(R).all()):
        raise ValueError("set_pin_motion: every parameter must be finite")
    return T, R


class PinsMixin:
    def _init_pins(self):
        self.pin_enabled = False
        self._pin_state = self._rhs_ext = self._pin_offsets = None
        self.n_pin = 0

    def _build_pins(self):
        """The pinned points' rest positions (a copy: update_pos() overwrites self.pos), their pts_Nx rows and the per-kernel CSR of their (pin, neighbour
        slot) pairs, stably sorted by kernel as `buffer` / `kernel_bg` are for the integration points (include/pienerf_hip.h: pn_sim_pins_rhs).  Only
        with pin motion enabled: a simulator without it does none of this.  ValueError for a cloud without pinned points.  Like the other tables of a
        layout these are new tensors after every precompute(): a substep captured into a graph before a re-layout holds the old ones, capture again."""
        dev, n_k = self.device, self.n_k
        vid = torch.nonzero(self.is_pin).reshape(-1)
        if vid.numel() == 0:
            raise ValueError("Simulator: pin motion needs pinned points, this cloud has none")
        self.pin_ids = vid
        self.n_pin = int(vid.numel())
        self.pin_rest = self.pos[vid].clone().contiguous()                              # [n_pin, 3]
        self.pin_Nx = self.pts_Nx[vid].contiguous()                                     # [n_pin, 8, 10]
        self.pin_kernel = self.pts_kernel[vid].contiguous()                             # [n_pin, 8]
        keys = self.pin_kernel.reshape(-1).long()
        order = torch.sort(keys, stable=True).indices                                   # entry = pin * 8 + slot
        cnt = torch.bincount(keys, minlength=n_k)
        self.pin_bg = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)]).to(torch.int32).contiguous()
        self.pin_of = (order // 8).to(torch.int32).contiguous()
        self.pin_N_csr = self.pin_Nx.reshape(self.n_pin * 8, 10)[order].contiguous()

    def enable_pin_motion(self):
        """From now on every stepforward() first writes rhs_gravity + stiff sum_p N_p^T u_p(t) (csrc/pn_pins.hip: k_pin_rhs) and runs the substep with
        it in the rhs_gravity slot: the pinned points follow u_p(t) (set_pin_motion, set_pin_offsets) through the reference's own penalty, the system
        matrix and Ainv unchanged.  t comes from a substep clock in device memory (substep k uses (k + 1) dt), so substeps captured into graphs after
        this call, or run frames ahead, move the pins at their own time.  No motion until set_pin_motion().  May be called before initialize();
        ValueError for a cloud without pinned points."""
        self._switch_on(STAGE)
        return self

    def _alloc_pins(self):
        self._new_state(STAGE)    # clock 0, active 0, no motion
        self._rhs_ext = self.rhs_gravity.clone()
        # offset_p, zeros until set_pin_offsets(): allocated here and always passed, so that a substep captured into a graph holds its address
        self._pin_offsets = torch.zeros((self.n_pin, 3), dtype=torchfloat, device=self.device)

    def _enqueue_pin_rhs(self, rhs_in=None):
        """_rhs_ext = rhs_in (None: rhs_gravity, the head of the chain) + the pins' term at the clock's substep, then the clock + 1: two launches on
        the current stream.  Returns _rhs_ext."""
        check(lib().pn_sim_pins_rhs(self.n_k, self.n_pin, ptr(self._stage_state(STAGE)), float(self.dt), float(self.stiff),
                                    ptr(self.rhs_gravity if rhs_in is None else rhs_in), ptr(self.pin_bg), ptr(self.pin_of), ptr(self.pin_N_csr),
                                    ptr(self.pin_rest), ptr(self._pin_offsets), ptr(self._rhs_ext), stream_ptr()), "sim_pins_rhs")
        return self._rhs_ext

    def set_pin_motion(self, translate=None, rotate=None):
        """The motion of the pinned points from the next substep on: u_p(t) = offset_p + T(t) + R(t)(X_p - c) - (X_p - c).
        translate = (A, hz, phase): T(t) = A sin(2 pi hz t + phase), A a 3-vector.  rotate = (axis, degrees, hz, phase, centre): R(t) the rotation about
        `axis` (normalised here) through `centre` (None: the centroid of the pinned rest points) by degrees sin(2 pi hz t + phase).  phase and centre may
        be left out; a part left out (None) is no motion of that kind.  Written on force_stream, between two substeps; the clock is left alone
        (reset_pin_clock)."""
        st = self._stage_state(STAGE)
        T, R = pin_motion_params(translate, rotate, lambda: self.pin_rest.mean(dim=0).cpu().numpy())
        with self._on_force_stream():
            check(lib().pn_sim_pins_set(ptr(st), self.n_pin, 1, T.ctypes.data, R.ctypes.data, stream_ptr()), "sim_pins_set")

    def set_pin_offsets(self, u):
        """offset_p: a displacement per pinned point ([n_pin, 3], in the order of pin_ids), added to the scripted motion: host-scripted handles.  None
        zeroes it.  Copied into the simulator's own buffer on force_stream, between two substeps; offsets alone move the pins only once the motion is
        active (set_pin_motion(), with no arguments for offsets only)."""
        self._stage_state(STAGE)
        if u is None:
            with self._on_force_stream():
                self._pin_offsets.zero_()
            return
        u = torch.as_tensor(u, dtype=torchfloat)
        if tuple(u.shape) != (self.n_pin, 3) or not bool(torch.isfinite(u).all()):
            raise ValueError(f"set_pin_offsets: expected finite values of shape [{self.n_pin}, 3], got {tuple(u.shape)}")
        u = u.to(self.device)
        with self._on_force_stream():
            self._pin_offsets.copy_(u)

    def stop_pin_motion(self):
        """active = 0: every following substep gets rhs_gravity itself (the pins go back to their rest positions); the clock keeps counting."""
        st = self._stage_state(STAGE)
        with self._on_force_stream():
            check(lib().pn_sim_pins_set(ptr(st), self.n_pin, 0, None, None, stream_ptr()), "sim_pins_set")

    def reset_pin_clock(self, k=0):
        """The next substep is substep `k` of the motion (t = (k + 1) dt)."""
        st = self._stage_state(STAGE)
        if int(k) < 0:
            raise ValueError("reset_pin_clock: k >= 0")
        with self._on_force_stream():
            check(lib().pn_sim_pins_clock(ptr(st), int(k), stream_ptr()), "sim_pins_clock")

    def pin_clock(self):
        """Substeps since the last reset: the pin motion's one read back to the host.  It waits for force_stream (or the current stream) only: where
        the substeps run on other streams (the pipelined harness, a caller's own side stream) the value is defined after those have been waited for —
        drain_pipeline() / synchronize()."""
        return self._read_clock(STAGE)
