"""Contact with planes, spheres, boxes and capsules (csrc/pn_contact.hip).  A pn_contact_state in device memory, read by two launches in front of every
substep (k_contact_points, k_contact_rhs) that write _rhs_contact = (the chain so far) + the contact term of the state the substep starts from.  The
parameters and the collider slots are mirrored on the host, so they may be set before initialize() and are uploaded when the state is allocated."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, _vec3, torchfloat

__all__ = ["CONTACT_SLOTS", "CONTACT_EMPTY", "CONTACT_PLANE", "CONTACT_SPHERE", "CONTACT_CONTAINER", "CONTACT_BOX", "CONTACT_CAPSULE",
           "CONTACT_COLLIDER_DTYPE", "CONTACT_STATE_DTYPE", "CONTACT_STATE_DOUBLES", "contact_params", "contact_plane", "contact_sphere", "contact_box",
           "contact_capsule", "pack_contact_state", "SDF_SLOTS", "SDF_SLOT_DTYPE", "SDF_STATE_DTYPE", "pack_sdf_state",
           "ContactMixin"]   # what solver.py re-exports

CONTACT_SLOTS = 8          # pn_contact_state's collider slots (include/pienerf_hip.h: PN_CONTACT_SLOTS)
CONTACT_EMPTY, CONTACT_PLANE, CONTACT_SPHERE, CONTACT_CONTAINER = 0, 1, 2, 3
CONTACT_BOX, CONTACT_CAPSULE = 4, 5
# pn_contact_collider / pn_contact_state (include/pienerf_hip.h) as numpy records: 88 and 744 bytes = pn_sim_contact_bytes(), checked in _alloc_contact
CONTACT_COLLIDER_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("R", "<f8"), ("v", "<f8", (3,))])
CONTACT_STATE_DTYPE = np.dtype([("active", "<i4"), ("n", "<i4"), ("kappa", "<f8"), ("beta", "<f8"), ("mu", "<f8"), ("h", "<f8"),
                                ("c", CONTACT_COLLIDER_DTYPE, (CONTACT_SLOTS,))])
CONTACT_STATE_DOUBLES = CONTACT_STATE_DTYPE.itemsize // 8
# mesh colliders: pn_sdf_slot / pn_sdf_state (include/pienerf_hip.h) as numpy records, 80 and 328 bytes = pn_sim_sdf_bytes(), checked
# in _alloc_sdf.  The contact stage's optional second state: allocated with the first mesh collider, never before
SDF_SLOTS = 4              # PN_SDF_SLOTS
SDF_SLOT_DTYPE = np.dtype([("grid", "<u8"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"), ("reserved", "<i4"), ("lo", "<f8", (3,)), ("s", "<f8"), ("v", "<f8", (3,))])
SDF_STATE_DTYPE = np.dtype([("n", "<i4"), ("reserved", "<i4"), ("c", SDF_SLOT_DTYPE, (SDF_SLOTS,))])

STAGE = Stage(name="contact", flag="contact_enabled", state="_contact_state", subject="contact is", owner="the contact state", enable="enable_contact",
              struct="pn_contact_state", nbytes=CONTACT_STATE_DOUBLES * 8, sized_by="solver.py allocates", init="_init_contact", alloc="_alloc_contact",
              enqueue="_enqueue_contact_rhs", tables="_need_Nx_csr", writes="rhs", clock=False)


def contact_params(stiffness, damping, friction, thickness):
    """(kappa, beta, mu, h) of pn_sim_contact_set_params, checked: the system matrix is at least M / dt^2, so a point's response to its own contact term
    is at most (kappa + beta) times its penetration, and with kappa in (0, 1], beta in [0, 1] no step pushes a point further out than it was in;
    mu >= 0, h >= 0, everything finite.  ValueError otherwise."""
    p = np.array([float(stiffness), float(damping), float(friction), float(thickness)])
    if not np.isfinite(p).all():
        raise ValueError(f"contact: every parameter must be finite, got {p.tolist()}")
    if not 0.0 < p[0] <= 1.0:
        raise ValueError(f"contact: stiffness must be in (0, 1], got {p[0]!r}")
    if not 0.0 <= p[1] <= 1.0:
        raise ValueError(f"contact: damping must be in [0, 1], got {p[1]!r}")
    if p[2] < 0.0:
        raise ValueError(f"contact: friction must be >= 0, got {p[2]!r}")
    if p[3] < 0.0:
        raise ValueError(f"contact: thickness must be >= 0, got {p[3]!r}")
    return p


def contact_plane(point, normal, velocity=None):
    """(type, geom10 = (p, n, R, v)) of pn_sim_contact_set_collider for the plane through `point` with `normal` out of the solid, normalised here once.
    ValueError for a zero or non-finite normal."""
    n = _vec3(normal, "a plane's normal")
    L = float(np.linalg.norm(n))
    if not (np.isfinite(L) and L > 0.0):
        raise ValueError(f"contact: a plane's normal must be a nonzero vector, got {normal!r}")
    g = np.zeros(10)
    g[0:3], g[3:6] = _vec3(point, "a plane's point"), n / L
    g[7:10] = _vec3(velocity, "a collider's velocity") if velocity is not None else 0.0
    return CONTACT_PLANE, g


def contact_sphere(centre, radius, inside=False, velocity=None):
    """(type, geom10) for a solid sphere, or with inside=True the container sphere the object lives in.  ValueError for a radius that is not > 0."""
    R = float(radius)
    if not (np.isfinite(R) and R > 0.0):
        raise ValueError(f"contact: a sphere's radius must be a finite number > 0, got {radius!r}")
    g = np.zeros(10)
    g[0:3], g[6] = _vec3(centre, "a sphere's centre"), R
    g[7:10] = _vec3(velocity, "a collider's velocity") if velocity is not None else 0.0
    return (CONTACT_CONTAINER if inside else CONTACT_SPHERE), g


def contact_box(centre, half_extents, velocity=None):
    """(type, geom10) for a solid axis-aligned box: p the centre, n the three half-extents, R = 0 (reserved).  ValueError for a half-extent that is
    not a finite number > 0."""
    h = _vec3(half_extents, "a box's half-extents")
    if not (np.isfinite(h).all() and (h > 0.0).all()):
        raise ValueError(f"contact: a box's half-extents must be three finite numbers > 0, got {half_extents!r}")
    g = np.zeros(10)
    g[0:3], g[3:6] = _vec3(centre, "a box's centre"), h
    g[7:10] = _vec3(velocity, "a collider's velocity") if velocity is not None else 0.0
    return CONTACT_BOX, g


def contact_capsule(a, b, radius, velocity=None):
    """(type, geom10) for a solid capsule, the points within `radius` of the segment from `a` to `b`: p = a, n = b - a (not normalised), R = radius.
    ValueError for a radius that is not > 0 or coinciding end points."""
    R = float(radius)
    if not (np.isfinite(R) and R > 0.0):
        raise ValueError(f"contact: a capsule's radius must be a finite number > 0, got {radius!r}")
    A = _vec3(a, "a capsule's end point a")
    n = _vec3(b, "a capsule's end point b") - A
    nn = float(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    if not (np.isfinite(nn) and nn > 0.0):
        raise ValueError(f"contact: a capsule's end points must be finite and distinct, got {a!r}, {b!r}")
    g = np.zeros(10)
    g[0:3], g[3:6], g[6] = A, n, R
    g[7:10] = _vec3(velocity, "a collider's velocity") if velocity is not None else 0.0
    return CONTACT_CAPSULE, g


def pack_contact_state(active, params, colliders):
    """The bytes of a pn_contact_state (include/pienerf_hip.h) holding `params` = (kappa, beta, mu, h) and `colliders` = CONTACT_SLOTS entries, each
    None or (type, geom10): what the device state holds after the setters (n = 1 + the highest slot in use)."""
    st = np.zeros((), CONTACT_STATE_DTYPE)
    st["active"] = int(active)
    st["kappa"], st["beta"], st["mu"], st["h"] = (float(v) for v in params)
    assert len(colliders) == CONTACT_SLOTS
    n = 0
    for i, c in enumerate(colliders):
        if c is None:
            continue
        t, g = c
        st["c"][i]["type"], st["c"][i]["p"], st["c"][i]["n"], st["c"][i]["R"], st["c"][i]["v"] = int(t), g[0:3], g[3:6], g[6], g[7:10]
        n = i + 1
    st["n"] = n
    return st.tobytes()


def pack_sdf_state(colliders):
    """The bytes of a pn_sdf_state holding `colliders` = SDF_SLOTS entries, each None or (grid, offset3, velocity3) with grid an SdfGrid: what the
    device state holds after the setters (n = 1 + the highest slot in use; a slot's lo is the grid's lo plus the offset)."""
    st = np.zeros((), SDF_STATE_DTYPE)
    assert len(colliders) == SDF_SLOTS
    n = 0
    for i, c in enumerate(colliders):
        if c is None:
            continue
        g, off, vel = c
        nz, ny, nx = g.shape
        r = st["c"][i]
        r["grid"], r["nx"], r["ny"], r["nz"], r["lo"], r["s"], r["v"] = g.values.data_ptr(), nx, ny, nz, g.lo + off, g.spacing, vel
        n = i + 1
    st["n"] = n
    return st.tobytes()


class ContactMixin:
    def _init_contact(self):
        self._sdf_state = None
        self._mesh_colliders = [None] * SDF_SLOTS   # (SdfGrid, offset, velocity): the host mirror, and what keeps a placed grid's memory alive
        self.contact_enabled = False
        self._contact_state = self._rhs_contact = self._contact_accel = None
        self._contact_params = None
        self._colliders = [None] * CONTACT_SLOTS

    def enable_contact(self, stiffness=0.5, damping=0.5, friction=0.5, thickness=None):
        """From now on every stepforward() first writes rhs + the contact term (csrc/pn_contact.hip: k_contact_points, k_contact_rhs; include/pienerf_hip.h has the law) and
        runs the substep with it in the rhs_gravity slot: an explicit penalty against the colliders added with add_plane / add_sphere / add_box / add_capsule, evaluated at the
        integration points from the dof / dof_vel that substep starts from; the system matrix and Ainv unchanged.  thickness None: dx / 2 (integration
        points are cell centres, the visible surface lies about half a cell outside them).  The state lives in device memory, so substeps captured into
        graphs after this call follow set_collider / set_contact_params without a recapture.  May be called before initialize(); ValueError for
        parameters out of range (contact_params)."""
        self._contact_params = contact_params(stiffness, damping, friction, 0.5 * float(self.dx) if thickness is None else thickness)
        if not self._switch_on(STAGE) and self._contact_state is not None:
            self._upload_contact_params()
        return self

    def _alloc_contact(self):
        self._new_state(STAGE)
        self._rhs_contact = self.rhs_gravity.clone()
        self._contact_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        self._upload_contact_params()
        for i, c in enumerate(self._colliders):
            if c is not None:
                self._upload_collider(i)
        if any(c is not None for c in self._mesh_colliders):
            self._alloc_sdf()

    def _upload_contact_params(self):
        p = np.ascontiguousarray(self._contact_params)
        with self._on_force_stream():
            check(lib().pn_sim_contact_set_params(ptr(self._contact_state), 1, p.ctypes.data, stream_ptr()), "sim_contact_set_params")

    def _upload_collider(self, i):
        c = self._colliders[i]
        t, g = (CONTACT_EMPTY, None) if c is None else (c[0], np.ascontiguousarray(c[1]))
        with self._on_force_stream():
            check(lib().pn_sim_contact_set_collider(ptr(self._contact_state), int(i), int(t), g.ctypes.data if g is not None else None, stream_ptr()),
                  "sim_contact_set_collider")

    def _put_collider(self, i, c):
        self._colliders[i] = c
        if self._contact_state is not None:
            self._upload_collider(i)   # on force_stream: the change lands between two substeps
        return i

    def _free_slot(self):
        for i, c in enumerate(self._colliders):
            if c is None:
                return i
        raise ValueError(f"contact: all {CONTACT_SLOTS} collider slots are in use (remove_collider frees one)")

    def set_contact_params(self, stiffness=None, damping=None, friction=None, thickness=None):
        """New values for the parameters given (None keeps one), from the next substep on.  ValueError for a value out of range."""
        self._stage_state(STAGE, gpu=False)
        old = self._contact_params
        new = [o if v is None else v for o, v in zip(old, (stiffness, damping, friction, thickness))]
        self._contact_params = contact_params(*new)
        if self._contact_state is not None:
            self._upload_contact_params()

    def add_plane(self, point, normal, velocity=None):
        """A half-space: the solid lies behind the plane through `point`, `normal` (normalised here) points out of it.  `velocity` (None: at rest) is the
        collider's own, for the relative velocity of damping and friction; the plane itself moves only when set_collider moves it.  Returns the
        collider's index; ValueError for a zero normal or a ninth collider."""
        self._stage_state(STAGE, gpu=False)
        c = contact_plane(point, normal, velocity)
        return self._put_collider(self._free_slot(), c)

    def add_sphere(self, centre, radius, inside=False, velocity=None):
        """A solid sphere, or with inside=True a container the object lives in.  Returns the collider's index; ValueError for radius <= 0 or a ninth
        collider."""
        self._stage_state(STAGE, gpu=False)
        c = contact_sphere(centre, radius, inside, velocity)
        return self._put_collider(self._free_slot(), c)

    def add_box(self, centre, half_extents, velocity=None):
        """A solid axis-aligned box about `centre` with the three `half_extents` (> 0).  Returns the collider's index; ValueError for a half-extent that
        is not > 0 or a ninth collider."""
        self._stage_state(STAGE, gpu=False)
        c = contact_box(centre, half_extents, velocity)
        return self._put_collider(self._free_slot(), c)

    def add_capsule(self, a, b, radius, velocity=None):
        """A solid capsule: everything within `radius` of the segment from `a` to `b`.  Returns the collider's index; ValueError for radius <= 0,
        a == b or a ninth collider."""
        self._stage_state(STAGE, gpu=False)
        c = contact_capsule(a, b, radius, velocity)
        return self._put_collider(self._free_slot(), c)

    def _slot(self, index):
        self._stage_state(STAGE, gpu=False)
        i = int(index)
        if not 0 <= i < CONTACT_SLOTS or self._colliders[i] is None:
            raise ValueError(f"contact: there is no collider {index!r}")
        return i

    def set_collider(self, index, point=None, normal=None, centre=None, radius=None, inside=None, velocity=None, half_extents=None, a=None, b=None):
        """Changes collider `index` from the next substep on; what is left None keeps its value.  A plane takes point / normal, a sphere centre / radius /
        inside, a box centre / half_extents, a capsule a / b / radius, all of them velocity.  A moving collider is scripted from the host with this, per frame, with `velocity` given for the relative velocity.
        ValueError for an index without a collider, an argument of the other kind, a value add_plane / add_sphere would refuse, or a slot that holds
        a dynamic body (bodies.py): the ball moves on the device, so the mirror this call edits is stale — set_body changes it."""
        i = self._slot(index)
        if self._is_body(i):
            raise ValueError(f"contact: collider {i} is a dynamic body that moves on the device: use set_body, not set_collider")
        t, g = self._colliders[i]
        vel = g[7:10] if velocity is None else velocity
        if t == CONTACT_PLANE:
            if any(v is not None for v in (centre, radius, inside, half_extents, a, b)):
                raise ValueError(f"contact: collider {i} is a plane: it takes point, normal and velocity")
            c = contact_plane(g[0:3] if point is None else point, g[3:6] if normal is None else normal, vel)
        elif t == CONTACT_BOX:
            if any(v is not None for v in (point, normal, radius, inside, a, b)):
                raise ValueError(f"contact: collider {i} is a box: it takes centre, half_extents and velocity")
            c = contact_box(g[0:3] if centre is None else centre, g[3:6] if half_extents is None else half_extents, vel)
        elif t == CONTACT_CAPSULE:
            if any(v is not None for v in (point, normal, centre, inside, half_extents)):
                raise ValueError(f"contact: collider {i} is a capsule: it takes a, b, radius and velocity")
            c = contact_capsule(g[0:3] if a is None else a, g[0:3] + g[3:6] if b is None else b, g[6] if radius is None else radius, vel)
        else:
            if point is not None or normal is not None or half_extents is not None or a is not None or b is not None:
                raise ValueError(f"contact: collider {i} is a sphere: it takes centre, radius, inside and velocity")
            c = contact_sphere(g[0:3] if centre is None else centre, g[6] if radius is None else radius, (t == CONTACT_CONTAINER) if inside is None else inside, vel)
        self._put_collider(i, c)

    def remove_collider(self, index):
        """Empties the slot: the collider acts on no further substep, its index may be handed out again.  A dynamic body in the slot (bodies.py) is
        removed with it."""
        i = self._slot(index)
        self._drop_body(i)
        self._put_collider(i, None)

    def clear_colliders(self):
        self._stage_state(STAGE, gpu=False)
        for i, c in enumerate(self._colliders):
            if c is not None:
                self._drop_body(i)
                self._put_collider(i, None)

    def contact_state_bytes(self):
        """What the device state holds, packed from the mirror kept here (pack_contact_state): tests compare the device's bytes with it.  A slot that
        holds a dynamic body (bodies.py) is the exception: on the device its p and v are the ball's motion, here what the host last gave it
        (body_state() reads the device's)."""
        self._stage_state(STAGE, gpu=False)
        return pack_contact_state(1, self._contact_params, self._colliders)

    def collider_state(self):
        """The pn_contact_state on the device (93 doubles), the simulator's own buffer: what the renderer's collider overlay reads
        (NeRFRenderer.set_collider_overlay; SimRenderHarness.draw_colliders), so a drawn collider is where set_collider last put it.  ValueError before
        enable_contact()."""
        if not self.contact_enabled:
            raise ValueError("collider_state: contact is not enabled (call enable_contact() first)")
        return self._stage_state(STAGE)

    def collider_types(self):
        """The type of every collider slot (CONTACT_EMPTY / _PLANE / _SPHERE / _CONTAINER / _BOX / _CAPSULE), from the host mirror."""
        return [CONTACT_EMPTY if c is None else int(c[0]) for c in self._colliders]

    # ------------------------------------------------------------------ mesh colliders: signed-distance grids
    def _contact_capture_names(self):
        """StageHost.enabled_stage_names(): while a mesh collider exists the stage enqueues one launch more, which a graph captured before lacks."""
        return ("mesh_colliders",) if any(c is not None for c in self._mesh_colliders) else ()

    def _alloc_sdf(self):
        nb = int(lib().pn_sim_sdf_bytes())
        if nb != SDF_STATE_DTYPE.itemsize:
            raise RuntimeError(f"libpienerf_hip.so's pn_sdf_state has {nb} bytes, contact.py lays out {SDF_STATE_DTYPE.itemsize}")
        self._sdf_state = torch.zeros(SDF_STATE_DTYPE.itemsize // 8, dtype=torchfloat, device=self.device)
        for i, c in enumerate(self._mesh_colliders):
            if c is not None:
                self._upload_mesh_collider(i)

    def _upload_mesh_collider(self, i):
        c = self._mesh_colliders[i]
        if c is not None and c[0].values.device != self._sdf_state.device:
            self._mesh_colliders[i] = None
            raise ValueError(f"contact: a mesh collider's grid lives on {c[0].values.device}, the simulator on {self._sdf_state.device}")
        with self._on_force_stream():
            if c is None:
                check(lib().pn_sim_sdf_set_collider(ptr(self._sdf_state), int(i), None, 0, 0, 0, None, stream_ptr()), "sim_sdf_set_collider")
                return
            g, off, vel = c
            g.values.record_stream(torch.cuda.current_stream(self.device))   # force_stream (or the current one): the stream of eager substeps
            nz, ny, nx = g.shape
            geom = np.ascontiguousarray(np.concatenate([g.lo + off, [g.spacing], vel]), dtype=np.float64)
            check(lib().pn_sim_sdf_set_collider(ptr(self._sdf_state), int(i), ptr(g.values), nx, ny, nz, geom.ctypes.data, stream_ptr()),
                  "sim_sdf_set_collider")

    def _put_mesh_collider(self, i, c):
        self._mesh_colliders[i] = c
        if self._contact_state is not None:   # on a GPU and initialised: the second state comes with the first mesh collider
            if self._sdf_state is None:
                self._alloc_sdf()
            else:
                self._upload_mesh_collider(i)   # on force_stream: the change lands between two substeps
        return i

    def add_mesh_collider(self, grid, offset=(0.0, 0.0, 0.0), velocity=None):
        """A static solid given by a signed-distance grid (pienerf_amd.sdf.SdfGrid: from_mesh, from_function), placed at `offset` from where it was
        built: contact's own response, with its parameters, at the trilinear distance and gradient of the grid (include/pienerf_hip.h:
        pn_sim_contact_sdf_rhs has the law).  A point outside the grid's box gets nothing from it.  `velocity` (None: at rest) is the collider's own,
        for the relative velocity of damping and friction; the solid moves only when set_mesh_collider moves it.  Translation only: rotate or scale
        the mesh before building.  The rigid balls (bodies.py) ignore mesh colliders, and the one-launch form of the stage does not exist with
        them.  Returns the collider's index 0..3; ValueError for a fifth, a grid that is not an SdfGrid or a non-finite offset."""
        self._stage_state(STAGE, gpu=False)
        from ..sdf import SdfGrid
        if not isinstance(grid, SdfGrid):
            raise ValueError(f"contact: a mesh collider is an SdfGrid (pienerf_amd.sdf), got {type(grid).__name__}")
        c = (grid, _vec3(offset, "a mesh collider's offset"), _vec3(velocity, "a collider's velocity") if velocity is not None else np.zeros(3))
        for i, have in enumerate(self._mesh_colliders):
            if have is None:
                return self._put_mesh_collider(i, c)
        raise ValueError(f"contact: all {SDF_SLOTS} mesh collider slots are in use (remove_mesh_collider frees one)")

    def _mesh_slot(self, index):
        self._stage_state(STAGE, gpu=False)
        i = int(index)
        if not 0 <= i < SDF_SLOTS or self._mesh_colliders[i] is None:
            raise ValueError(f"contact: there is no mesh collider {index!r}")
        return i

    def set_mesh_collider(self, index, offset=None, velocity=None):
        """Moves mesh collider `index` to `offset` and / or gives it `velocity`, from the next substep on (None keeps a value): a scripted translation,
        followed by captured graphs without a recapture.  ValueError for an index without a mesh collider or a non-finite value."""
        i = self._mesh_slot(index)
        g, off, vel = self._mesh_colliders[i]
        self._put_mesh_collider(i, (g, off if offset is None else _vec3(offset, "a mesh collider's offset"),
                                    vel if velocity is None else _vec3(velocity, "a collider's velocity")))

    def remove_mesh_collider(self, index):
        """Empties the slot: the grid acts on no further substep, its index may be handed out again.  The simulator drops its reference to the grid
        with it.  Substeps already enqueued on other streams than force_stream (a captured graph's, a pipeline's) may still read the grid: wait for
        them (synchronize) before the last reference to the grid goes."""
        self._put_mesh_collider(self._mesh_slot(index), None)

    def mesh_collider_state(self):
        """The pn_sdf_state on the device (41 doubles), the simulator's own buffer, or None while no mesh collider was ever added on the device.
        RuntimeError before enable_contact()."""
        self._stage_state(STAGE, gpu=False)
        return self._sdf_state

    def mesh_collider_state_bytes(self):
        """What the device state holds, packed from the mirror kept here (pack_sdf_state): tests compare the device's bytes with it."""
        self._stage_state(STAGE, gpu=False)
        return pack_sdf_state(self._mesh_colliders)

    def _enqueue_contact_rhs(self, rhs_in, one_launch=False):
        """_rhs_contact = rhs_in + the contact term of the current dof / dof_vel, on the current stream.  Returns _rhs_contact.  Two launches: the law at
        every point into _contact_accel, then the per-kernel sums (the measured faster form).  one_launch=True (tools/time_contact.py, tests):
        the form in which every entry evaluates its point itself — the same bits in _rhs_contact, _contact_accel left as it is.  With a mesh collider
        present: three launches, the grids' terms added to _contact_accel between the two (pn_sim_contact_sdf_rhs); one_launch then raises."""
        if any(c is not None for c in self._mesh_colliders):
            if one_launch:
                raise RuntimeError("contact: the one-launch form does not evaluate mesh colliders (remove_mesh_collider first)")
            check(lib().pn_sim_contact_sdf_rhs(self.n_k, self.n_IP, ptr(self._stage_state(STAGE)), ptr(self._sdf_state), float(self.dt), float(self.dx),
                                               ptr(self.dof), ptr(self.dof_vel), ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.kernel_bg),
                                               ptr(self.kernel_cnt), ptr(self.buffer), ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_contact),
                                               ptr(self._contact_accel), stream_ptr()), "sim_contact_sdf_rhs")
            return self._rhs_contact
        check(lib().pn_sim_contact_rhs(self.n_k, self.n_IP, ptr(self._stage_state(STAGE)), float(self.dt), float(self.dx), ptr(self.dof), ptr(self.dof_vel),
                                       ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer),
                                       ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_contact), None if one_launch else ptr(self._contact_accel), stream_ptr()),
              "sim_contact_rhs")
        return self._rhs_contact

    def contact_accel(self):
        """[n_IP, 3]: the contact acceleration a_i of every integration point in the last substep enqueued (zeros for a point not in contact).  The
        simulator's own buffer, overwritten by the next substep."""
        self._stage_state(STAGE)
        return self._contact_accel

    def contact_count(self):
        """Integration points in contact in the last substep (a_i != 0: a penetrated collider always pushes, a_n > 0): contact's one read back to the
        host.  Like pin_clock() it waits for force_stream (or the current stream) only."""
        self._stage_state(STAGE)
        return self._host_read(lambda: int((self._contact_accel != 0.0).any(dim=1).sum().item()))
