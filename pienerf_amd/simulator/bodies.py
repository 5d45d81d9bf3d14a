"""Rigid balls: dynamic sphere colliders the object pushes back (csrc/pn_bodies.hip).  A pn_bodies_state in device memory (a substep
clock, gravity, a record per collider slot) and two launches in front of every substep, behind contact's (k_body_reaction, k_body_step), that sum the
object's reaction on every dynamic sphere and integrate it.  A body's centre and velocity are its collider slot's own p and v in the pn_contact_state:
contact, the drawn frame and the shadows follow a moving ball as they are.  Masses and dampings are mirrored on the host, so bodies may be added
before initialize(); the motion lives on the device alone.  No rotation, no contact between two balls."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, _vec3, torchfloat
from .contact import CONTACT_SLOTS, CONTACT_SPHERE, CONTACT_STATE_DOUBLES, CONTACT_STATE_DTYPE, contact_sphere

__all__ = ["BODIES_SLOTS", "BODY_DTYPE", "BODIES_STATE_DTYPE", "BODIES_STATE_DOUBLES", "body_params", "pack_bodies_state", "BodiesMixin"]   # what solver.py re-exports

BODIES_SLOTS = CONTACT_SLOTS   # body b lives in collider slot b (include/pienerf_hip.h: PN_BODIES_SLOTS)
# pn_body / pn_bodies_state (include/pienerf_hip.h) as numpy records: 72 and 616 bytes = pn_sim_bodies_bytes(), checked in _alloc_bodies
BODY_DTYPE = np.dtype([("dynamic", "<i4"), ("reserved", "<i4"), ("M", "<f8"), ("c", "<f8"), ("F", "<f8", (3,)), ("s", "<f8"), ("delta_max", "<f8"),
                       ("clamped", "<i8")])
BODIES_STATE_DTYPE = np.dtype([("k", "<i8"), ("active", "<i4"), ("reserved", "<i4"), ("g", "<f8", (3,)), ("b", BODY_DTYPE, (BODIES_SLOTS,))])
BODIES_STATE_DOUBLES = BODIES_STATE_DTYPE.itemsize // 8

STAGE = Stage(name="bodies", flag="bodies_enabled", state="_bodies_state", subject="the rigid balls are", owner="the bodies state", enable="enable_bodies",
              struct="pn_bodies_state", nbytes=BODIES_STATE_DOUBLES * 8, sized_by="bodies.py lays out", init="_init_bodies", alloc="_alloc_bodies",
              enqueue="_enqueue_bodies", tables=None, writes="rhs", clock=True)


def body_params(mass, damping):
    """(M, c) of pn_sim_bodies_set_body, checked: M finite and > 0, c finite and >= 0.  ValueError otherwise."""
    M, c = float(mass), float(damping)
    if not (np.isfinite(M) and M > 0.0):
        raise ValueError(f"bodies: a body's mass must be a finite number > 0, got {mass!r}")
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError(f"bodies: a body's damping must be a finite number >= 0, got {damping!r}")
    return M, c


def pack_bodies_state(active, gravity, bodies, k=0):
    """The bytes of a pn_bodies_state (include/pienerf_hip.h) at clock `k` holding `gravity` and `bodies` = BODIES_SLOTS entries, each None or
    (mass, damping): what the device state holds after the setters and before a body's first substep (F = 0, s = 1, nothing clamped)."""
    st = np.zeros((), BODIES_STATE_DTYPE)
    st["k"], st["active"], st["g"] = int(k), int(active), _vec3(gravity, "gravity", "bodies")
    assert len(bodies) == BODIES_SLOTS
    for i, b in enumerate(bodies):
        if b is not None:
            st["b"][i]["dynamic"], st["b"][i]["M"], st["b"][i]["c"], st["b"][i]["s"] = 1, float(b[0]), float(b[1]), 1.0
    return st.tobytes()


class BodiesMixin:
    def _init_bodies(self):
        self.bodies_enabled = False
        self._bodies_state = self._bodies_work = None
        self._bodies = [None] * BODIES_SLOTS      # (mass, damping) per collider slot that holds a body
        self._bodies_gravity = None

    def enable_bodies(self, gravity=None):
        """From now on every stepforward() moves the dynamic balls added with add_body (csrc/pn_bodies.hip: k_body_reaction, k_body_step;
        include/pienerf_hip.h has the law): the object's contact force on a ball, summed in a fixed order and clamped to the ball's deepest penetration,
        the static colliders, `gravity` (None: the simulator's) and the ball's damping, integrated semi-implicitly into the collider slot's own centre
        and velocity.  Contact has read the slot before the ball moves, everything else sees the new position from the next substep on.  Needs
        enable_contact() first (ValueError); may be called before initialize()."""
        if not self.contact_enabled:
            raise ValueError("bodies: the balls are colliders of the contact stage: call enable_contact() first")
        g = self.gravity.detach().cpu().numpy() if gravity is None else gravity
        self._bodies_gravity = _vec3(g, "gravity", "bodies")
        if not self._switch_on(STAGE) and self._bodies_state is not None:
            self._upload_bodies_params(1)
        return self

    def _alloc_bodies(self):
        if self._contact_state is None:
            raise RuntimeError("Simulator: the bodies stage moves colliders of the contact state, which is not allocated")
        self._new_state(STAGE)    # clock 0, active 0, no body
        nb = int(lib().pn_sim_bodies_work_bytes(self.n_IP))
        if nb <= 0:
            raise RuntimeError(f"pn_sim_bodies_work_bytes({self.n_IP}) gave {nb}")
        self._bodies_work = torch.zeros(nb // 8, dtype=torchfloat, device=self.device)
        self._upload_bodies_params(1)
        for i, b in enumerate(self._bodies):
            if b is not None:
                self._upload_body(i)

    def _upload_bodies_params(self, active):
        g = np.ascontiguousarray(self._bodies_gravity)
        with self._on_force_stream():
            check(lib().pn_sim_bodies_set_params(ptr(self._bodies_state), int(active), g.ctypes.data, stream_ptr()), "sim_bodies_set_params")

    def _upload_body(self, i):
        b = self._bodies[i]
        with self._on_force_stream():
            check(lib().pn_sim_bodies_set_body(ptr(self._bodies_state), int(i), 0 if b is None else 1, 0.0 if b is None else b[0], 0.0 if b is None else b[1],
                                               stream_ptr()), "sim_bodies_set_body")

    def _body_slot(self, index):
        self._stage_state(STAGE, gpu=False)
        i = int(index)
        if not 0 <= i < BODIES_SLOTS or self._bodies[i] is None:
            raise ValueError(f"bodies: there is no body {index!r}")
        return i

    def _is_body(self, i):
        return self._bodies[int(i)] is not None

    def add_body(self, centre, radius, mass, velocity=None, damping=0.0):
        """A dynamic ball: a solid sphere in a free collider slot that the object pushes back.  `velocity` (None: at rest) throws it.  Returns the
        collider's index, which is the body's.  ValueError without enable_contact(), for mass <= 0, damping < 0, radius <= 0, a non-finite value or a
        ninth collider."""
        if not self.contact_enabled:
            raise ValueError("bodies: the balls are colliders of the contact stage: call enable_contact() first")
        self._stage_state(STAGE, gpu=False)
        b = body_params(mass, damping)
        c = contact_sphere(centre, radius, False, velocity)
        i = self._put_collider(self._free_slot(), c)
        self._bodies[i] = b
        if self._bodies_state is not None:
            self._upload_body(i)
        return i

    def set_body(self, index, centre=None, velocity=None, mass=None, damping=None):
        """Changes body `index` from the next substep on; what is left None keeps the DEVICE's value (the ball has moved since it was added).  With
        `velocity` it throws the ball.  ValueError for an index without a body or a value add_body would refuse."""
        i = self._body_slot(index)
        M, c = self._bodies[i]
        new = body_params(M if mass is None else mass, c if damping is None else damping)
        t, g = self._colliders[i]
        g = g.copy()    # the mirror keeps what the host last gave: the contact state's bytes for this slot are the device's (contact_state_bytes)
        mask = 0
        if centre is not None:
            g[0:3], mask = _vec3(centre, "a body's centre", "bodies"), mask | 1
        if velocity is not None:
            g[7:10], mask = _vec3(velocity, "a body's velocity", "bodies"), mask | 2
        self._bodies[i], self._colliders[i] = new, (t, g)
        if self._bodies_state is None:
            return
        if new != (M, c):
            self._upload_body(i)
        if mask:
            pv = np.ascontiguousarray(np.concatenate([g[0:3], g[7:10]]))
            with self._on_force_stream():
                check(lib().pn_sim_bodies_set_motion(ptr(self._contact_state), i, mask, pv.ctypes.data, stream_ptr()), "sim_bodies_set_motion")

    def remove_body(self, index):
        """The body and its collider leave: the slot is empty from the next substep on, its index may be handed out again."""
        i = self._body_slot(index)
        self._drop_body(i)
        self._put_collider(i, None)

    def _drop_body(self, i):
        if self._bodies[i] is not None:
            self._bodies[i] = None
            if self._bodies_state is not None:
                self._upload_body(i)

    def body_indices(self):
        """The collider slots that hold a body, ascending (host mirror)."""
        return [i for i, b in enumerate(self._bodies) if b is not None]

    def _enqueue_bodies(self, rhs_in, one_launch=False):
        """The balls' substep on the current stream, behind contact's launches: two launches that read dof / dof_vel and the contact state this substep
        starts from and write the dynamic slots' p and v.  A link of the chain only for its place in the order: returns rhs_in unchanged.
        one_launch=True (tools/time_bodies.py, tests): the form in which the last workgroup to arrive does the second launch's work — the same bits,
        measured slower."""
        check(lib().pn_sim_bodies_step(self.n_k, self.n_IP, ptr(self._stage_state(STAGE)), ptr(self._contact_state), ptr(self._bodies_work), float(self.dt),
                                       float(self.dx), ptr(self.dof), ptr(self.dof_vel), ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), 1 if one_launch else 0,
                                       stream_ptr()), "sim_bodies_step")
        return rhs_in

    def body_state(self):
        """{index: dict(centre, velocity, radius, mass, damping, reaction, scale, delta_max, clamped)} of every body, from the device: the stage's one
        read back to the host.  reaction / scale / delta_max are the last substep's F_b, s and deepest penetration; clamped counts the substeps with
        s < 1.  Like pin_clock() it waits for force_stream (or the current stream) only."""
        bs = self._stage_state(STAGE)
        raw = self._host_read(lambda: torch.cat([self._contact_state, bs]).cpu().numpy())
        cs = raw[:CONTACT_STATE_DOUBLES].view(CONTACT_STATE_DTYPE)[0]
        st = raw[CONTACT_STATE_DOUBLES:].view(BODIES_STATE_DTYPE)[0]
        out = {}
        for i in self.body_indices():
            c, b = cs["c"][i], st["b"][i]
            out[i] = dict(centre=c["p"].copy(), velocity=c["v"].copy(), radius=float(c["R"]), mass=float(b["M"]), damping=float(b["c"]),
                          reaction=b["F"].copy(), scale=float(b["s"]), delta_max=float(b["delta_max"]), clamped=int(b["clamped"]))
        return out

    def body_clock(self):
        """Substeps the stage has run since the last reset (one read back, as pin_clock())."""
        return self._read_clock(STAGE)

    def reset_body_clock(self, k=0):
        st = self._stage_state(STAGE)
        if int(k) < 0:
            raise ValueError("reset_body_clock: k >= 0")
        with self._on_force_stream():
            check(lib().pn_sim_bodies_clock(ptr(st), int(k), stream_ptr()), "sim_bodies_clock")

    def stop_bodies(self):
        """active = 0: no ball moves in the following substeps (each stays a collider where it is, with the velocity it has); the clock keeps
        counting.  enable_bodies() switches them on again."""
        self._stage_state(STAGE)
        self._upload_bodies_params(0)

    def bodies_state_bytes(self):
        """What the device state holds before a body's first substep, packed from the mirror kept here (pack_bodies_state)."""
        self._stage_state(STAGE, gpu=False)
        return pack_bodies_state(1, self._bodies_gravity, self._bodies)
