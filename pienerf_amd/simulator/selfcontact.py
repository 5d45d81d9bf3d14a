"""Self-contact: the body collides with itself and its own pieces (csrc/pn_selfcontact.hip).  A pn_selfcontact_state in device memory,
read by eight launches in front of every substep (a hashed grid over the deformed integration points, two gather passes, the per-kernel sum) that
write _rhs_self = (the chain so far) + the self-contact term of the state the substep starts from.  The parameters are mirrored on the host, so they
may be set before initialize()."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, torchfloat

__all__ = ["SELF_STATE_DTYPE", "SELF_STATE_DOUBLES", "self_contact_params", "pack_self_contact_state", "SelfContactMixin"]   # what solver.py re-exports

# pn_selfcontact_state (include/pienerf_hip.h) as a numpy record: 56 bytes = pn_sim_self_bytes(), checked in _alloc_self_contact
SELF_STATE_DTYPE = np.dtype([("active", "<i4"), ("reserved", "<i4"), ("overflowed", "<i8"), ("kappa", "<f8"), ("beta", "<f8"), ("mu", "<f8"), ("h", "<f8"),
                             ("rho_x", "<f8")])
SELF_STATE_DOUBLES = SELF_STATE_DTYPE.itemsize // 8

STAGE = Stage(name="self", flag="self_contact_enabled", state="_self_state", subject="self-contact is", owner="the self-contact state",
              enable="enable_self_contact", struct="pn_selfcontact_state", nbytes=SELF_STATE_DOUBLES * 8, sized_by="solver.py's SELF_STATE_DTYPE",
              init="_init_self_contact", alloc="_alloc_self_contact", enqueue="_enqueue_self_rhs", tables="_need_Nx_csr", writes="rhs", clock=False)


def self_contact_params(stiffness, damping, friction, thickness, exclusion):
    """(kappa, beta, mu, h, rho_x) of pn_sim_self_set_params, checked: kappa in (0, 1], beta in [0, 1] (a pair's relative response is at most
    (kappa + beta) delta w_ij: contact's stability argument), mu >= 0, h > 0, rho_x >= h, everything finite.  ValueError otherwise."""
    p = np.array([float(stiffness), float(damping), float(friction), float(thickness), float(exclusion)])
    if not np.isfinite(p).all():
        raise ValueError(f"self-contact: every parameter must be finite, got {p.tolist()}")
    if not 0.0 < p[0] <= 1.0:
        raise ValueError(f"self-contact: stiffness must be in (0, 1], got {p[0]!r}")
    if not 0.0 <= p[1] <= 1.0:
        raise ValueError(f"self-contact: damping must be in [0, 1], got {p[1]!r}")
    if p[2] < 0.0:
        raise ValueError(f"self-contact: friction must be >= 0, got {p[2]!r}")
    if not p[3] > 0.0:
        raise ValueError(f"self-contact: thickness must be > 0, got {p[3]!r}")
    if p[4] < p[3]:
        raise ValueError(f"self-contact: exclusion must be >= thickness ({p[3]!r}), got {p[4]!r}")
    return p


def pack_self_contact_state(active, params, overflowed=0):
    """The bytes of a pn_selfcontact_state (include/pienerf_hip.h) holding `params` = (kappa, beta, mu, h, rho_x) after `overflowed` overflowed calls."""
    st = np.zeros((), SELF_STATE_DTYPE)
    st["active"], st["overflowed"] = int(active), int(overflowed)
    st["kappa"], st["beta"], st["mu"], st["h"], st["rho_x"] = (float(v) for v in params)
    return st.tobytes()


class SelfContactMixin:
    def _init_self_contact(self):
        self.self_contact_enabled = False
        self._self_active = False
        self._self_state = self._self_work = self._rhs_self = self._self_accel = self._self_X = None
        self._self_params = None

    def enable_self_contact(self, stiffness=0.5, damping=0.5, friction=0.0, thickness=None, exclusion=None):
        """From now on every stepforward() first writes rhs + the self-contact term (csrc/pn_selfcontact.hip; include/pienerf_hip.h has the law) and runs
        the substep with it in the rhs_gravity slot, last in the chain rhs_gravity -> pins -> contact -> fields -> self: an explicit penalty between
        integration points that are closer than `thickness` (None: dx, two cell centres touch a cell apart) and were at least `exclusion` apart at rest
        (None: 3 x thickness), so the body stays out of itself and separate pieces of one cloud collide; the system matrix and Ainv unchanged.  The
        state lives in device memory, so substeps captured into graphs after this call follow set_self_contact_params without a recapture.  After
        stop_self_contact() it switches the stage on again.  There is no continuous collision detection: a piece moving more than `thickness` per
        substep can tunnel.  May be called before initialize(); ValueError for parameters out of range (self_contact_params)."""
        h = float(self.dx) if thickness is None else thickness
        self._self_params = self_contact_params(stiffness, damping, friction, h, 3.0 * float(h) if exclusion is None else exclusion)
        self._self_active = True
        if not self._switch_on(STAGE) and self._self_state is not None:
            self._upload_self_params()
        return self

    def _alloc_self_contact(self):
        self._new_state(STAGE)   # inactive, nothing overflowed
        self._self_work = torch.zeros(int(lib().pn_sim_self_work_bytes(self.n_IP)) // 8, dtype=torchfloat, device=self.device)
        self._rhs_self = self.rhs_gravity.clone()
        self._self_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        self._self_X = self.IP_pos.to(dtype=torchfloat).contiguous()
        self._upload_self_params()

    def _upload_self_params(self):
        p = np.ascontiguousarray(self._self_params)
        with self._on_force_stream():
            check(lib().pn_sim_self_set_params(ptr(self._self_state), int(self._self_active), p.ctypes.data, stream_ptr()), "sim_self_set_params")

    def set_self_contact_params(self, stiffness=None, damping=None, friction=None, thickness=None, exclusion=None):
        """New values for the parameters given (None keeps one), from the next substep on.  ValueError for a value out of range."""
        self._stage_state(STAGE, gpu=False)
        new = [o if v is None else v for o, v in zip(self._self_params, (stiffness, damping, friction, thickness, exclusion))]
        self._self_params = self_contact_params(*new)
        if self._self_state is not None:
            self._upload_self_params()

    def stop_self_contact(self):
        """active = 0: every following substep gets its right-hand side without the self-contact term, bit for bit; the parameters stay.
        enable_self_contact() switches the stage on again."""
        self._stage_state(STAGE, gpu=False)
        self._self_active = False
        if self._self_state is not None:
            self._upload_self_params()

    def self_contact_state_bytes(self, overflowed=0):
        """What the device state holds after `overflowed` overflowed substeps, packed from the mirror kept here (pack_self_contact_state): tests
        compare the device's bytes with it."""
        self._stage_state(STAGE, gpu=False)
        return pack_self_contact_state(int(self._self_active), self._self_params, overflowed)

    def _enqueue_self_rhs(self, rhs_in):
        """_rhs_self = rhs_in + the self-contact term of the current dof / dof_vel: eight launches on the current stream.  Returns _rhs_self."""
        check(lib().pn_sim_self_rhs(self.n_k, self.n_IP, ptr(self._stage_state(STAGE)), ptr(self._self_work), float(self.dt), float(self.dx),
                                    ptr(self.dof), ptr(self.dof_vel), ptr(self._self_X), ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx),
                                    ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer), ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_self),
                                    ptr(self._self_accel), stream_ptr()), "sim_self_rhs")
        return self._rhs_self

    def self_contact_accel(self):
        """[n_IP, 3]: the self-contact acceleration a_i of every integration point in the last substep enqueued (zeros for a point without a partner).
        The simulator's own buffer, overwritten by the next substep."""
        self._stage_state(STAGE)
        return self._self_accel

    def self_contact_count(self):
        """Integration points with a_i != 0 in the last substep.  Like contact_count() it waits for force_stream (or the current stream) only."""
        self._stage_state(STAGE)
        return self._host_read(lambda: int((self._self_accel != 0.0).any(dim=1).sum().item()))

    def self_contact_overflows(self):
        """Substeps whose stage was switched off because a bucket of the hashed grid held more than 64 points (the body has collapsed): the state's
        counter read back to the host."""
        st = self._stage_state(STAGE)
        return self._host_read(lambda: int(st[1:2].view(torch.int64).item()))
