"""``Simulator`` with the reference's public surface (simulator/solver.py:12-617, /root/reference).

Kept: constructor arguments, ``InitializeFromPly``, ``get_IP_info`` (fp32, permuted layouts of solver.py:422-424),
``stepforward`` (+ alias ``step``), ``update_force`` / ``clear_force``, ``OutputToPly``, attributes ``dx``, ``IP_pos``,
``dof`` ... as torch tensors on the GPU.  Changed on purpose:
  * the per-substep work is HIP (libpienerf_hip.so: pn_sim_stepforward / pn_sim_update_F / pn_sim_update_force);
  * ``global_matrix`` / ``mass_matrix_invt2`` are stored in their kron(A, I3) factor form ``Ainv`` / ``Mmat``
    ([10 n_k]^2 instead of [30 n_k]^2, solver.py:493-496,532-538) — same products, 9x fewer bytes;
  * importing this module does not call ``torch.set_default_device("cuda")`` (func_utils.py:6).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from .. import scene
from .._lib import check, lib, ptr, stream_ptr
from . import gmls

torchfloat = torch.float64
npfloat = np.float64


class _null_ctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


CELL_CHUNK_IPS = 32   # points per chunk of the substep's cell form = pn_sim_cells_chunk_ips() (csrc/pn_sim_cells.h: PN_CELL_IPS), checked in _prepare_cells


DRAG_SCALE_MIN, DRAG_SCALE_MAX = 1e-3, 5e1   # gui.py:865
PIN_STATE_DOUBLES = 16   # pn_pin_motion (include/pienerf_hip.h) as doubles: 128 bytes = pn_sim_pins_bytes(), checked in _alloc_pins


CONTACT_SLOTS = 8          # pn_contact_state's collider slots (include/pienerf_hip.h: PN_CONTACT_SLOTS)
CONTACT_EMPTY, CONTACT_PLANE, CONTACT_SPHERE, CONTACT_CONTAINER = 0, 1, 2, 3
# pn_contact_collider / pn_contact_state (include/pienerf_hip.h) as numpy records: 88 and 744 bytes = pn_sim_contact_bytes(), checked in _alloc_contact
CONTACT_COLLIDER_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("R", "<f8"), ("v", "<f8", (3,))])
CONTACT_STATE_DTYPE = np.dtype([("active", "<i4"), ("n", "<i4"), ("kappa", "<f8"), ("beta", "<f8"), ("mu", "<f8"), ("h", "<f8"),
                                ("c", CONTACT_COLLIDER_DTYPE, (CONTACT_SLOTS,))])
CONTACT_STATE_DOUBLES = CONTACT_STATE_DTYPE.itemsize // 8


FIELD_SLOTS = 8            # pn_field_state's field slots (include/pienerf_hip.h: PN_FIELD_SLOTS)
FIELD_EMPTY, FIELD_WIND, FIELD_VORTEX, FIELD_RADIAL = 0, 1, 2, 3
# pn_force_field / pn_field_state (include/pienerf_hip.h) as numpy records: 144 and 1168 bytes = pn_sim_fields_bytes(), checked in _alloc_fields
FIELD_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("c", "<f8"), ("s", "<f8"), ("R", "<f8"),
                        ("g", "<f8"), ("f", "<f8"), ("phi", "<f8"), ("kv", "<f8", (3,)), ("t0", "<f8"), ("t1", "<f8")])
FIELD_STATE_DTYPE = np.dtype([("k", "<i8"), ("active", "<i4"), ("n", "<i4"), ("f", FIELD_DTYPE, (FIELD_SLOTS,))])
FIELD_STATE_DOUBLES = FIELD_STATE_DTYPE.itemsize // 8
# the arguments each kind of field takes, with the defaults of add_wind / add_vortex / add_radial: what set_field(index, **changed) may change
FIELD_ARGS = {
    FIELD_WIND: dict(velocity=None, drag=2.0, gust=0.0, hz=0.0, phase=0.0, wave=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), start=0.0, stop=None),
    FIELD_VORTEX: dict(point=None, axis=None, omega=None, radius=None, drag=2.0, start=0.0, stop=None),
    FIELD_RADIAL: dict(centre=None, strength=None, radius=None, start=0.0, stop=None),
}
FIELD_KINDS = {FIELD_WIND: "a wind", FIELD_VORTEX: "a vortex", FIELD_RADIAL: "a radial field"}

# pn_selfcontact_state (include/pienerf_hip.h) as a numpy record: 56 bytes = pn_sim_self_bytes(), checked in _alloc_self_contact
SELF_STATE_DTYPE = np.dtype([("active", "<i4"), ("reserved", "<i4"), ("overflowed", "<i8"), ("kappa", "<f8"), ("beta", "<f8"), ("mu", "<f8"), ("h", "<f8"),
                             ("rho_x", "<f8")])
SELF_STATE_DOUBLES = SELF_STATE_DTYPE.itemsize // 8


def _vec3(v, what, who="contact"):
    a = np.asarray(v, npfloat)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError(f"{who}: {what} is a finite 3-vector, got {v!r}")
    return a.reshape(3).copy()


def _field_number(v, what, lo=None, hi=None, above=None):
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"fields: {what} is a number, got {v!r}") from None
    if not (np.isfinite(x) and (lo is None or x >= lo) and (hi is None or x <= hi) and (above is None or x > above)):
        want = ["finite"] + [f"{op} {b}" for op, b in ((">=", lo), ("<=", hi), (">", above)) if b is not None]
        raise ValueError(f"fields: {what} must be {' and '.join(want)}, got {v!r}")
    return x


def _field_window(g, start, stop):
    g[15] = _field_number(start, "start")
    g[16] = np.inf if stop is None or (isinstance(stop, float) and stop == np.inf) else _field_number(stop, "stop")
    if g[16] < g[15]:
        raise ValueError(f"fields: stop must not be before start, got start={start!r}, stop={stop!r}")


def field_wind(velocity, drag=2.0, gust=0.0, hz=0.0, phase=0.0, wave=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), start=0.0, stop=None):
    """(type, geom17 = (p, n, c, s, R, g, f, phi, kv, t0, t1)) of pn_sim_fields_set_field for a wind of `velocity` that drags the body toward it at
    `drag` per second; gust in [0, 1] modulates the velocity by 1 + gust sin(2 pi (hz t - wave.(x - origin)) + phase).  Acts while
    start <= t < stop (None: for ever).  ValueError for what the library would refuse."""
    g = np.zeros(17)
    g[0:3], g[3:6] = _vec3(origin, "a wind's origin", "fields"), _vec3(velocity, "a wind's velocity", "fields")
    g[6] = _field_number(drag, "drag", lo=0.0)
    g[9], g[10], g[11] = _field_number(gust, "gust", lo=0.0, hi=1.0), _field_number(hz, "hz"), _field_number(phase, "phase")
    g[12:15] = _vec3(wave, "a gust's wave vector", "fields")
    _field_window(g, start, stop)
    return FIELD_WIND, g


def field_vortex(point, axis, omega, radius, drag=2.0, start=0.0, stop=None):
    """(type, geom17) for a vortex about the line through `point` along `axis` (normalised here once): it drags the body toward the rigid rotation
    omega (axis x r) with drag `drag` at the axis, falling to nothing at `radius`.  ValueError for a zero axis or a radius that is not > 0."""
    n = _vec3(axis, "a vortex's axis", "fields")
    L = float(np.linalg.norm(n))
    if not (np.isfinite(L) and L > 0.0):
        raise ValueError(f"fields: a vortex's axis must be a nonzero vector, got {axis!r}")
    g = np.zeros(17)
    g[0:3], g[3:6] = _vec3(point, "a vortex's point", "fields"), n / L
    g[6], g[7], g[8] = _field_number(drag, "drag", lo=0.0), _field_number(omega, "omega"), _field_number(radius, "radius", above=0.0)
    _field_window(g, start, stop)
    return FIELD_VORTEX, g


def field_radial(centre, strength, radius, start=0.0, stop=None):
    """(type, geom17) for a radial field: the acceleration `strength` away from `centre` (toward it for strength < 0), falling to nothing at `radius`.
    With a short window it is a blast.  ValueError for a radius that is not > 0."""
    g = np.zeros(17)
    g[0:3] = _vec3(centre, "a radial field's centre", "fields")
    g[7], g[8] = _field_number(strength, "strength"), _field_number(radius, "radius", above=0.0)
    _field_window(g, start, stop)
    return FIELD_RADIAL, g


FIELD_BUILDERS = {FIELD_WIND: field_wind, FIELD_VORTEX: field_vortex, FIELD_RADIAL: field_radial}


def pack_field_state(active, fields, k=0):
    """The bytes of a pn_field_state (include/pienerf_hip.h) with the clock at `k` holding `fields` = FIELD_SLOTS entries, each None or
    (type, geom17): what the device state holds after the setters (n = 1 + the highest slot in use)."""
    st = np.zeros((), FIELD_STATE_DTYPE)
    st["k"], st["active"] = int(k), int(active)
    assert len(fields) == FIELD_SLOTS
    n = 0
    for i, fld in enumerate(fields):
        if fld is None:
            continue
        t, g = fld
        f = st["f"][i]
        f["type"], f["p"], f["n"], f["c"], f["s"], f["R"], f["g"], f["f"], f["phi"], f["kv"], f["t0"], f["t1"] = (
            int(t), g[0:3], g[3:6], g[6], g[7], g[8], g[9], g[10], g[11], g[12:15], g[15], g[16])
        n = i + 1
    st["n"] = n
    return st.tobytes()


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


def wheel_force_scale(scale, delta):
    """The GUI's mouse-wheel rule for the drag's force scale (gui.py:857-865): +-0.5 per notch above 1, +-0.1 at or below, clamped to [1e-3, 50]."""
    scale = float(scale)
    scale += delta * 0.5 if scale > 1.0 else delta * 0.1
    return max(DRAG_SCALE_MIN, min(scale, DRAG_SCALE_MAX))


def _check_scale(s):
    s = float(s)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"drag force scale must be a positive finite number, got {s!r}")
    return s


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


class Simulator:
    def __init__(self, dt=1e-2, iters=20, bbox=torch.tensor([1.0, 1.0, 1.0], dtype=torchfloat), kres=7, dx=1,
                 gravity=torch.tensor([0.0, -9.8, 0.0], dtype=torchfloat), stiff=1e5, base=torch.tensor([-0.5, -0.5, -0.5], dtype=torchfloat),
                 device="cuda", persistent=None, svd=None):
        self.device = torch.device(device)
        # svd: which decomposition stands in for wp.svd3 (cuda_utils.py:107) in calc_elastic.  "jacobi" (default): the converged, warm-started threshold
        # Jacobi; "mcadams" / "mcadams:N": the published algorithm wp.svd3 implements (McAdams et al., TR1690) with N fixed sweeps (default 8, the setting
        # of double-precision builds; 4 is the paper's single-precision setting) — csrc/pn_sim_svd.h: svd3_mcadams.  None: environment PN_SIM_SVD.
        svd = (svd if svd is not None else os.environ.get("PN_SIM_SVD", "jacobi")).strip().lower()
        name, _, n = svd.partition(":")
        if name not in ("jacobi", "mcadams") or (n and not n.isdigit()) or (name == "jacobi" and n):
            raise ValueError(f"Simulator: svd must be 'jacobi', 'mcadams' or 'mcadams:<sweeps>', got {svd!r}")
        self.svd_sweeps = 0 if name == "jacobi" else int(n or 8)
        if self.svd_sweeps == 0 and name == "mcadams" or self.svd_sweeps > 64:
            raise ValueError("Simulator: mcadams sweeps must be in 1..64")
        # persistent: run the local/global iterations of a substep as ONE cooperative kernel (pn_sim_stepforward_coop) instead of four launches per
        # iteration.  None: environment PN_SIM_COOP (1 / 0), default off — the persistent kernel wants every CU for itself, which suits a GPU that
        # only simulates (the owner rank of a frame-parallel job, a latency-bound single frame) and not one that renders three frames beside it
        if persistent is None:
            persistent = os.environ.get("PN_SIM_COOP", "") == "1"
        self.persistent = bool(persistent)
        if self.persistent and self.svd_sweeps:
            raise ValueError("Simulator: the persistent substep has the default decomposition only; svd='mcadams' runs on the cell and CSR forms")
        self._coop = None
        # cell_form: calc_elastic + collect_rhs_IP of a local/global iteration as one launch per kernel-grid cell chunk (pn_sim_stepforward_cells, 21
        # launches per substep instead of 31); PN_SIM_FORM=csr keeps the round-1-4 launch form (three launches per iteration over per-kernel CSR lists)
        self.cell_form = os.environ.get("PN_SIM_FORM", "cells") != "csr"
        bbox = bbox.clone() * 1.02   # solver.py:24-25 multiply in the caller's dtype (main_gui.py passes float32), then widen
        base = base.clone() * 1.01
        self.dt, self.iters, self.dx, self.kres, self.stiff = dt, iters, dx, kres, stiff
        bbox = bbox.to(dtype=torchfloat)
        self.res = (bbox // dx).to(dtype=torch.int32).to(self.device)
        self.base = base.to(dtype=torchfloat).to(self.device)
        self.gravity = gravity.to(dtype=torchfloat).to(self.device)
        self.dof = None
        self._work = None
        self._prepared = False   # pn_sim_prepare has run on _work (with the first substep: the CSR lists it reads are built by precompute)
        self._cells = self._cells_work = None
        # stream on which update_force / clear_force are enqueued (None: the caller's current stream).  A harness that runs the substeps
        # on a stream of their own (harness.py: overlap_sim, capture_pipelined) sets it to that stream, so that a force change is ordered
        # BETWEEN two substeps instead of racing with one
        self.force_stream = None
        self.force_hooks = None   # (before, after): a pipeline whose substeps do not run on force_stream orders the change between two of them (frames.FramePipeline)
        # the GUI's mouse drag on the device (enable_drag): a pn_drag_state in device memory, read by a k_drag_force launch in front of every substep
        self.drag_enabled = False
        self.drag_force_scale = 1.0
        self._drag = self._drag_work = None
        # kinematic pins (enable_pin_motion): a pn_pin_motion in device memory with its own substep clock, read by a k_pin_rhs launch in front of every
        # substep that writes _rhs_ext = rhs_gravity + the pins' right-hand-side term; the substep then takes _rhs_ext in its rhs_gravity slot
        self.pin_enabled = False
        self._pin_state = self._rhs_ext = self._pin_offsets = None
        self.n_pin = 0
        # contact with planes and spheres (enable_contact): a pn_contact_state in device memory, read by two launches in front of every substep
        # (k_contact_points, k_contact_rhs) that write _rhs_contact = (rhs_gravity or _rhs_ext) + the contact term of the state the substep starts from.  The parameters and the
        # collider slots are mirrored here, so they may be set before initialize() and are uploaded when the state is allocated
        self.contact_enabled = False
        self._contact_state = self._rhs_contact = self._contact_accel = None
        self._contact_params = None
        self._colliders = [None] * CONTACT_SLOTS
        self.Nx_csr = None
        # force fields (enable_fields): a pn_field_state in device memory with its own substep clock, read by three launches in front of every substep
        # (k_field_points, k_field_rhs, k_field_tick) that write _rhs_fields = (rhs_gravity, _rhs_ext or _rhs_contact) + the field term of the state and
        # the time the substep starts from.  The slots are mirrored here, so they may be set before initialize() and are uploaded when the state is allocated
        self.fields_enabled = False
        self._fields_active = False
        self._field_state = self._rhs_fields = self._field_accel = None
        self._fields = [None] * FIELD_SLOTS        # (type, geom17) per slot
        self._field_args = [None] * FIELD_SLOTS    # the arguments each was built from: what set_field() changes
        # self-contact (enable_self_contact): a pn_selfcontact_state in device memory, read by eight launches in front of every substep (a hashed grid
        # over the deformed integration points, two gather passes, the per-kernel sum) that write _rhs_self = (the chain so far) + the self-contact term
        # of the state the substep starts from.  The parameters are mirrored here, so they may be set before initialize()
        self.self_contact_enabled = False
        self._self_active = False
        self._self_state = self._self_work = self._rhs_self = self._self_accel = self._self_X = None
        self._self_params = None

    # ------------------------------------------------------------------ IO (solver.py:109-137)
    def InitializeFromPly(self, path):
        c = scene.cloud_from_ply(path)
        self.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])

    def InitializeFromArrays(self, pos, mass, mu, lam, pin):
        dev = self.device
        self.pos = torch.from_numpy(np.asarray(pos, npfloat)).to(dev)
        assert self.pos.shape[0] > 0
        self.mass = torch.from_numpy(np.asarray(mass, npfloat)).to(dev)
        self.mu = torch.from_numpy(np.asarray(mu, npfloat)).to(dev)
        self.lam = torch.from_numpy(np.asarray(lam, npfloat)).to(dev)
        self.is_pin = torch.from_numpy(np.asarray(pin).astype(bool)).to(dev)
        if not bool((self.mass > 0).all()):  # collect_IP divides by the summed mass of every occupied cell (solver.py:450)
            raise ValueError("Simulator: every point needs mass > 0 (a PLY written by OutputToPly carries positions only)")
        self.initialize()

    def OutputToPly(self, path):
        """solver.py:109-113: the deformed point positions as a vertex element with double x, y, z only."""
        p = self.update_pos().cpu().numpy().astype(np.float64)
        scene.write_ply(path, dict(pos=p), props=("x", "y", "z"))

    # ------------------------------------------------------------------ init (solver.py:139-331)
    def initialize(self):
        self.precompute()
        self._work = torch.empty(int(lib().pn_sim_work_doubles(self.n_k, self.n_IP)), dtype=torchfloat, device=self.device)
        self._prepared = False
        self.rhs_rest = (self.build_rhs() + self._matvec(self.Mmat, self.dof)).contiguous()   # solver.py:314
        if self.drag_enabled and self.device.type == "cuda":
            self._alloc_drag()
        if self.pin_enabled and self.device.type == "cuda":
            self._alloc_pins()
        if self.contact_enabled and self.device.type == "cuda":
            self._alloc_contact()
        if self.fields_enabled and self.device.type == "cuda":
            self._alloc_fields()
        if self.self_contact_enabled and self.device.type == "cuda":
            self._alloc_self_contact()

    def precompute(self):
        """Everything of initialize() that is tensor bookkeeping / torch.linalg (device-agnostic), and on a GPU the cell form's work area for the
        layout built here; the HIP-backed rest state (rhs_rest) is finished by initialize()."""
        dev, res, kres = self.device, self.res, self.kres
        r0, r1, r2 = (int(v) for v in res.cpu())
        self.grid_idx = ((self.pos - self.base) // self.dx).to(dtype=torch.int32).long()
        gi = self.grid_idx
        self.IP_mask = torch.zeros((r0, r1, r2), dtype=torch.bool, device=dev)
        self.IP_mask[gi[:, 0], gi[:, 1], gi[:, 2]] = True
        n_IP = int(self.IP_mask.sum())
        self.IP_idx = -torch.ones((r0, r1, r2), dtype=torch.int32, device=dev)
        self.IP_idx[self.IP_mask] = torch.arange(0, n_IP, 1, dtype=torch.int32, device=dev)
        self.pts_IP = self.IP_idx[gi[:, 0], gi[:, 1], gi[:, 2]]
        # kornia.create_meshgrid3d + channel swap (solver.py:162-169) == grid[i,j,k] = (i,j,k)
        ax = [torch.arange(r, dtype=torch.int32, device=dev) for r in (r0, r1, r2)]
        cell_ijk = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)
        self.IP_grid = cell_ijk[self.IP_mask, :]
        self.IP_pos = (self.IP_grid + 0.5) * self.dx + self.base          # float32 product, then float64 sum (:177)
        self.kernel_mask = torch.zeros((kres, kres, kres), dtype=torch.bool, device=dev)
        self.kdx = ((res.max()) * self.dx) / (kres - 1)                  # 0-dim float32 tensor (:184)
        IP2K = ((self.IP_pos - self.base) // self.kdx).to(dtype=torch.int32).long()
        corners = [(S >> 2 & 1, S >> 1 & 1, S & 1) for S in range(8)]
        for x, y, z in corners:
            self.kernel_mask[IP2K[:, 0] + x, IP2K[:, 1] + y, IP2K[:, 2] + z] |= True
        n_k = int(self.kernel_mask.sum())
        self.kernel_idx = torch.zeros((kres, kres, kres), dtype=torch.int32, device=dev)
        self.kernel_idx[self.kernel_mask] = torch.arange(0, n_k, 1, dtype=torch.int32, device=dev)
        pts2K = ((self.pos - self.base) // self.kdx).to(dtype=torch.int32).long()
        self.IP_kernel = torch.stack([self.kernel_idx[IP2K[:, 0] + x, IP2K[:, 1] + y, IP2K[:, 2] + z] for x, y, z in corners], dim=1).contiguous()
        self.pts_kernel = torch.stack([self.kernel_idx[pts2K[:, 0] + x, pts2K[:, 1] + y, pts2K[:, 2] + z] for x, y, z in corners], dim=1).contiguous()
        ka = torch.arange(kres, dtype=torch.int32, device=dev)
        self.kernel_grid = torch.stack(torch.meshgrid(ka, ka, ka, indexing="ij"), dim=-1)[self.kernel_mask, :]
        self.kernel_pos = self.kernel_grid * self.kdx + self.base       # float32 product, then float64 sum (:248)
        self.n_k, self.n_IP = n_k, n_IP

        kdx = float(self.kdx)
        self.pts_Nx, self.pts_dNx, self.pts_ddNx = gmls.init_GMLS(kdx, self.pos, self.pts_kernel, self.kernel_pos)
        self.IP_Nx, self.IP_dNx, self.IP_ddNx = gmls.init_GMLS(kdx, self.IP_pos, self.IP_kernel, self.kernel_pos)
        self.IP_mu, self.IP_lam, self.IP_rho = self.collect_IP()
        self.build_global()

        # rest state: translation = kernel position, affine = identity, quadratic = 0 (solver.py:258-275)
        dof = torch.zeros((n_k, 10, 3), dtype=torchfloat, device=dev)
        dof[:, 0, :] = self.kernel_pos
        for x in range(3):
            dof[:, 1 + x, x] = 1.0
        self.dof = dof.reshape(-1).contiguous()
        self.dof_tilde = self.dof.clone()
        self.dof_rest = self.dof.clone()
        self.dof_vel = torch.zeros_like(self.dof)
        self.dof_f = torch.zeros_like(self.dof)

        # per-kernel CSR of (IP, neighbour slot) pairs (count_IP_kernel / allocate_IP_kernel, solver.py:277-313), in ascending order
        keys = self.IP_kernel.reshape(-1).long()
        order = torch.sort(keys, stable=True).indices
        self.buffer = order.to(torch.int32).contiguous()                 # entry = vid*8 + dir
        self.kernel_cnt = torch.bincount(keys, minlength=n_k).to(torch.int32).contiguous()
        self.kernel_bg = (torch.cumsum(self.kernel_cnt, dim=0, dtype=torch.int32) - self.kernel_cnt).contiguous()
        self.tot = int(self.kernel_cnt.sum())
        # dNx rows in CSR order (6.9 MB on the chair): the step driver's collect_rhs then reads each kernel's entries as one
        # contiguous stream instead of chasing `buffer` (pn_sim_stepforward, dNx_csr)
        self.dNx_csr = self.IP_dNx.reshape(n_IP * 8, 30)[order].contiguous()
        self.csr_pos = torch.empty_like(self.buffer)
        self.csr_pos[order] = torch.arange(order.numel(), dtype=torch.int32, device=dev)   # inverse of `buffer`

        self._IP2K = IP2K
        self._cells = self._cells_work = None
        if self.cell_form:   # (torch bookkeeping only; the work area and the check against the library's chunk size: _prepare_cells, below)
            self._build_cells()

        m = (self.IP_rho * self.dx * self.dx * self.dx)                                      # collect_gravity, cuda_utils.py:262-279
        rg = torch.zeros((n_k * 10, 3), dtype=torchfloat, device=dev)
        rows = (self.IP_kernel.long()[:, :, None] * 10 + torch.arange(10, device=dev)[None, None, :]).reshape(-1)
        gmls.index_add_ordered(rg, rows, (m[:, None, None] * self.IP_Nx).reshape(-1)[:, None] * self.gravity[None, :])
        self.rhs_gravity = rg.reshape(-1).contiguous()
        self.n_pin, self.pin_bg = 0, None   # the pins' tables belong to the layout: built with it when pin motion is enabled, else by enable_pin_motion()
        if self.pin_enabled:
            self._build_pins()
        self.Nx_csr = None                  # ... and so do the contact launch's: built with the layout when contact is enabled, else by enable_contact()
        if self.contact_enabled or self.fields_enabled or self.self_contact_enabled:
            self._build_contact()
        if self._cells is not None and self.device.type == "cuda":   # a new layout gets a new work area, here and never inside a substep
            self._prepare_cells()

    def _build_cells(self):
        """Layout of the substep's CELL form (include/pienerf_hip.h: pn_sim_stepforward_cells): the integration points of one kernel-grid cell share
        their 8 neighbour kernels (IP_kernel rows are equal, solver.py:186-205), so they are sorted by cell and every cell is cut into chunks of at most
        pn_sim_cells_chunk_ips() points — one workgroup each, computing calc_elastic and the points' contributions to collect_rhs_IP in one launch."""
        dev, n_IP, n_k, kres = self.device, self.n_IP, self.n_k, self.kres
        B = CELL_CHUNK_IPS
        cell = (self._IP2K[:, 0] * kres + self._IP2K[:, 1]) * kres + self._IP2K[:, 2]
        order = torch.sort(cell, stable=True).indices                                  # points by cell, ascending point index inside a cell
        cs = cell[order]
        first = torch.ones(n_IP, dtype=torch.bool, device=dev)
        first[1:] = cs[1:] != cs[:-1]
        start = torch.nonzero(first).reshape(-1)                                       # where each cell begins in the sorted order
        cnt = torch.diff(torch.cat([start, torch.tensor([n_IP], device=dev)]))
        nch = (cnt + B - 1) // B                                                       # chunks per cell
        n_chunks = int(nch.sum())
        ch_cell = torch.repeat_interleave(torch.arange(len(cnt), device=dev), nch)     # chunk -> cell
        ch_first = torch.cumsum(nch, 0) - nch                                          # first chunk of each cell
        ch_j = torch.arange(n_chunks, device=dev) - ch_first[ch_cell]                  # chunk's index inside its cell
        ch_begin = start[ch_cell] + ch_j * B                                           # first point (sorted order) of the chunk
        ch_count = torch.minimum(cnt[ch_cell] - ch_j * B, torch.tensor(B, device=dev))
        local = torch.arange(B, device=dev)[None, :]
        valid = local < ch_count[:, None]                                              # [n_chunks, B]
        src = order[torch.clamp(ch_begin[:, None] + local, max=n_IP - 1)]              # original point index per chunk position
        topo = self.IP_kernel.long()
        assert bool((topo[src[valid]] == topo[src[:, :1].expand(-1, B)[valid]]).all()), "points of one kernel-grid cell must share their 8 kernels"
        tab = torch.zeros((n_chunks, 12), dtype=torch.int32, device=dev)
        tab[:, 0] = ch_count.to(torch.int32)
        tab[:, 1:9] = topo[src[:, 0]].to(torch.int32)
        g = self.IP_dNx.reshape(n_IP, 8, 30)[src] * valid[:, :, None, None].to(torchfloat)   # [n_chunks, B, 8, 30]
        # lane l of wave w = point w * 8 + l // 8, slot l % 8: [chunk][wave][15][64][2]
        g = g.reshape(n_chunks, B // 8, 8, 8, 15, 2).permute(0, 1, 4, 2, 3, 5).reshape(n_chunks, B // 8, 15, 64, 2)
        self._cells = dict(n_chunks=n_chunks, B=B, tab=tab.contiguous(), dNx=g.contiguous(),
                           mu=(self.IP_mu[src] * valid).reshape(-1).contiguous(), lam=(self.IP_lam[src] * valid).reshape(-1).contiguous(), src=src, valid=valid)
        # per kernel: the (chunk, slot) pairs that refer to it, ascending
        keys = tab[:, 1:9].reshape(-1).long()
        kp = torch.sort(keys, stable=True).indices
        kcnt = torch.bincount(keys, minlength=n_k)
        self._cells["kp_list"] = kp.to(torch.int32).contiguous()
        pos = torch.empty_like(kp)
        pos[kp] = torch.arange(kp.numel(), device=dev)
        self._cells["kp_pos"] = pos.to(torch.int32).contiguous()                       # where (chunk, slot) stores its partial sum: its rank in its kernel's run
        self._cells["kp_bg"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(kcnt, 0)]).to(torch.int32).contiguous()

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

    def _build_contact(self):
        """The Nx rows in CSR order (as dNx_csr is for the substep): the contact launch reads a kernel's run as one contiguous stream.  Only with contact
        enabled.  A new tensor after every precompute(), like the other tables of a layout."""
        self.Nx_csr = self.IP_Nx.reshape(self.n_IP * 8, 10)[self.buffer.long()].contiguous()

    def _prepare_cells(self):
        """The cell form's work area: identity rotations for the warm-started SVD, arrival counters (never inside a stream capture)."""
        if int(lib().pn_sim_cells_chunk_ips()) != CELL_CHUNK_IPS:
            raise RuntimeError(f"libpienerf_hip.so cuts cells into chunks of {lib().pn_sim_cells_chunk_ips()} points, solver.py into {CELL_CHUNK_IPS}")
        n_chunks = self._cells["n_chunks"]
        self._cells_work = torch.empty(int(lib().pn_sim_cells_work_doubles(self.n_k, n_chunks)), dtype=torchfloat, device=self.device)
        check(lib().pn_sim_cells_prepare(self.n_k, n_chunks, ptr(self._cells_work), stream_ptr()), "sim_cells_prepare")

    def reset_warm_start(self):
        """Forget the SVD warm start (the V of every integration point's previous local/global iteration, kept in the cell form's work area).  Results
        do not depend on it beyond the decomposition's stopping rule (off-diagonals <= 1e-11 of the diagonal: 1e-10 relative on the displacements), but
        BIT-equal replays of a trajectory do: whoever restores dof / dof_vel to replay (harness.capture, tests) calls this as well."""
        if self._cells_work is not None:
            check(lib().pn_sim_cells_prepare(self.n_k, self._cells["n_chunks"], ptr(self._cells_work), stream_ptr()), "sim_cells_prepare")
        if self._prepared:
            check(lib().pn_sim_prepare(self.n_k, self.n_IP, ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self._work), stream_ptr()), "sim_prepare")

    def collect_IP(self):  # solver.py:427-450
        n_IP, idx = self.n_IP, self.pts_IP.long()
        z = torch.zeros(n_IP, dtype=torchfloat, device=self.device)
        s_mu = gmls.index_add_ordered(z.clone(), idx, self.mu * self.mass)
        s_lam = gmls.index_add_ordered(z.clone(), idx, self.lam * self.mass)
        s_m = gmls.index_add_ordered(z.clone(), idx, self.mass)
        return (s_mu / s_m).contiguous(), (s_lam / s_m).contiguous(), (s_m / (self.dx ** 3)).contiguous()

    def build_global(self):  # solver.py:453-538
        dim = self.n_k * 10
        mat = gmls.assemble_IP_matrix(dim, self.dx, self.dt, self.IP_kernel, self.IP_mu, self.IP_lam, self.IP_rho, self.IP_Nx, self.IP_dNx, self.IP_ddNx)
        assert self.pts_kernel.min() >= 0 and self.pts_kernel.max() < self.n_k
        vid = torch.nonzero(self.is_pin).reshape(-1)
        mat = gmls.add_pin_penalty(mat, self.stiff, vid, self.pts_kernel, self.pts_Nx)
        diag = mat.diagonal()[0::10]
        self.active_kernels = torch.nonzero(diag > 0.0).reshape(-1)                      # `global_matrix[i*30, i*30] > 0` (:499-504)
        lst = (self.active_kernels[:, None] * 10 + torch.arange(10, device=self.device)[None, :]).reshape(-1)
        sub = mat[lst][:, lst].clone()
        sub.diagonal().add_(1e-3)                                                         # :507
        inv = gmls.inverse_spd(sub)
        self.Ainv = torch.zeros((dim, dim), dtype=torchfloat, device=self.device)
        self.Ainv[lst[:, None], lst[None, :]] = inv
        self.Ainv = self.Ainv.contiguous()
        zero = torch.zeros_like(self.IP_mu)
        self.Mmat = gmls.assemble_IP_matrix(dim, self.dx, self.dt, self.IP_kernel, zero, zero, self.IP_rho, self.IP_Nx, self.IP_dNx, self.IP_ddNx).contiguous()

    # the reference's (30 n_k)^2 forms, materialised on demand (tests / interop only)
    @property
    def global_matrix(self):
        return torch.kron(self.Ainv, torch.eye(3, dtype=torchfloat, device=self.device))

    @property
    def mass_matrix_invt2(self):
        return torch.kron(self.Mmat, torch.eye(3, dtype=torchfloat, device=self.device))

    # ------------------------------------------------------------------ per-frame (HIP)
    def _matvec(self, A, x):
        y = torch.empty_like(x)
        check(lib().pn_sim_matvec3(A.shape[0], ptr(A), ptr(x), ptr(y), stream_ptr()), "sim_matvec3")
        return y

    def build_rhs(self):  # solver.py:541-571
        n = self.n_IP
        RF = torch.empty((n, 3, 3), dtype=torchfloat, device=self.device)
        VF = torch.empty_like(RF)
        check(lib().pn_sim_calc_elastic(n, ptr(self.IP_kernel), ptr(self.IP_dNx), ptr(self.dof), ptr(RF), ptr(VF), None, self.svd_sweeps, stream_ptr()),
              "calc_elastic")
        rhs = torch.empty_like(self.dof)
        check(lib().pn_sim_collect_rhs(self.n_k, float(self.dx), ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer), ptr(self.IP_mu),
                                       ptr(self.IP_lam), ptr(self.IP_dNx), ptr(RF), ptr(VF), ptr(rhs), stream_ptr()), "collect_rhs")
        return rhs

    def get_IP_info(self, dof=None, out=None):  # solver.py:402-424
        """(IP_pos, IP_F, IP_dF) of the current state.  `dof` (a [30 n_k] fp64 snapshot of self.dof) and `out` (three preallocated
        fp32 tensors) are extensions for the pipelined harness: frames in flight each own a snapshot and a set of IP buffers."""
        n, dev = self.n_IP, self.device
        if out is None:
            pos = torch.empty((n, 3), dtype=torch.float32, device=dev)
            F = torch.empty((n, 9), dtype=torch.float32, device=dev)
            dF = torch.empty((n, 27), dtype=torch.float32, device=dev)
        else:
            pos, F, dF = out
        check(lib().pn_sim_update_F(n, ptr(self.IP_kernel), ptr(self.dof if dof is None else dof), ptr(self.IP_Nx), ptr(self.IP_dNx), ptr(self.IP_ddNx),
                                    ptr(pos), ptr(F), ptr(dF), stream_ptr()), "update_F")
        return pos, F, dF

    def _prepare_persistent(self):
        """Lays out the persistent kernel's pieces (one host read-back of the CSR counts); falls back to the launch form when the scene does not fit."""
        # one workgroup per CU, minus a few CUs left to whatever else runs on the device meanwhile (a collective's kernels, a copy kernel): a
        # persistent workgroup takes a CU's whole register file, and with no CU to spare the launch would wait for those kernels to end
        n_wg = min(max(int(lib().pn_device_cu_count()) - int(os.environ.get("PN_SIM_COOP_RESERVE", "8")), 8), 256)
        nbytes = int(lib().pn_sim_coop_bytes(self.n_k, self.n_IP, n_wg))
        self._coop = None
        if nbytes == 0:
            self.persistent = False
            return
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        plan = (C.c_int32 * 3)()
        rc = lib().pn_sim_coop_prepare(self.n_k, self.n_IP, n_wg, ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(buf), plan, stream_ptr())
        if rc != 0:  # PN_ERR_ARG: lists too long for register-resident pieces
            self.persistent = False
            return
        self._coop = (buf, n_wg, plan)

    def enable_persistent(self):
        """Switch to the persistent substep (a harness calls this for a GPU that only simulates: the owner rank of a frame-parallel job with a
        dedicated simulator).  PN_SIM_COOP=0 vetoes it, so does svd='mcadams' (the persistent form has the default decomposition only); scenes that
        do not fit keep the launch form.  Returns whether it is on."""
        if os.environ.get("PN_SIM_COOP", "") == "0" or self.svd_sweeps:
            return False
        self.persistent = True
        if self._prepared and self._coop is None:
            self._prepare_persistent()
        return self.persistent and (self._coop is not None or not self._prepared)

    def persistent_timed_out(self):
        """True if a persistent substep gave up waiting at a device-wide barrier (its workgroups could not all become resident): results invalid."""
        if self._coop is None:
            return False
        flag = C.c_int32(0)
        check(lib().pn_sim_coop_status(ptr(self._coop[0]), C.byref(flag)), "sim_coop_status")
        return flag.value != 0

    def stepforward(self):  # solver.py:595-602
        if self.drag_enabled:   # the spring force of THIS substep's state (gui.py:556-586), on the substep's stream, captured with it into graphs
            check(lib().pn_sim_drag_force(self.n_k, self.n_IP, ptr(self._drag), ptr(self.dof), float(self.dx), ptr(self.IP_kernel), ptr(self.IP_rho),
                                          ptr(self.IP_Nx), ptr(self.dof_f), stream_ptr()), "sim_drag_force")
        if not self._prepared:
            check(lib().pn_sim_prepare(self.n_k, self.n_IP, ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self._work), stream_ptr()), "sim_prepare")
            self._prepared = True
            if self.persistent:
                self._prepare_persistent()
        rhs_g = self.rhs_gravity
        if self.pin_enabled:    # rhs_gravity + the pins' term at THIS substep's time, on the substep's stream, captured with it into graphs
            rhs_g = self._enqueue_pin_rhs()
        if self.contact_enabled:   # ... + the contact term of THIS substep's state, into a buffer of its own, on the substep's stream, captured with it
            rhs_g = self._enqueue_contact_rhs(rhs_g)
        if self.fields_enabled:    # ... + the field term of THIS substep's state and time, last in the chain: rhs_gravity -> pins -> contact -> fields
            rhs_g = self._enqueue_fields_rhs(rhs_g)
        if self.self_contact_enabled:   # ... + the self-contact term of THIS substep's state, behind fields: rhs_gravity -> pins -> contact -> fields -> self
            rhs_g = self._enqueue_self_rhs(rhs_g)
        if self.persistent and self._coop is not None and 1 <= self.iters <= 32:
            buf, n_wg, plan = self._coop
            check(lib().pn_sim_stepforward_coop(self.n_k, self.n_IP, int(self.iters), float(self.dt), float(self.dx), ptr(self.IP_kernel), ptr(self.IP_mu),
                                                ptr(self.IP_lam), ptr(self.IP_dNx), ptr(self.dNx_csr), ptr(self.csr_pos), ptr(self.Ainv), ptr(self.Mmat),
                                                ptr(self.dof_rest), ptr(self.rhs_rest), ptr(rhs_g), ptr(self.dof_f), ptr(self.dof), ptr(self.dof_vel),
                                                ptr(self._work), ptr(buf), n_wg, plan, stream_ptr()), "stepforward_coop")
            return
        if self.cell_form and self._cells is not None and int(self.iters) >= 1:
            if self._cells_work is None:
                raise RuntimeError("Simulator: the cell form's work area is missing (precompute() prepares it on a GPU device)")
            c = self._cells
            check(lib().pn_sim_stepforward_cells(self.n_k, c["n_chunks"], int(self.iters), float(self.dt), float(self.dx), ptr(c["tab"]), ptr(c["dNx"]),
                                                 ptr(c["mu"]), ptr(c["lam"]), ptr(c["kp_bg"]), ptr(c["kp_pos"]), ptr(self.Ainv), ptr(self.Mmat),
                                                 ptr(self.dof_rest), ptr(self.rhs_rest), ptr(rhs_g), ptr(self.dof_f), ptr(self.dof), ptr(self.dof_vel),
                                                 ptr(self._cells_work), self.svd_sweeps, stream_ptr()), "stepforward_cells")
            return
        check(lib().pn_sim_stepforward(self.n_k, self.n_IP, int(self.iters), float(self.dt), float(self.dx), ptr(self.IP_kernel), ptr(self.kernel_bg),
                                       ptr(self.kernel_cnt), ptr(self.buffer), ptr(self.IP_mu), ptr(self.IP_lam), ptr(self.IP_dNx), ptr(self.dNx_csr), ptr(self.csr_pos), ptr(self.Ainv),
                                       ptr(self.Mmat), ptr(self.dof_rest), ptr(self.rhs_rest), ptr(rhs_g), ptr(self.dof_f), ptr(self.dof),
                                       ptr(self.dof_vel), ptr(self._work), 1, self.svd_sweeps, stream_ptr()), "stepforward")

    step = stepforward  # BASELINE.json's name for the same entry point

    @contextlib.contextmanager
    def _on_force_stream(self):
        """Runs the enclosed launches on `force_stream` (or the current stream), ordered BETWEEN two substeps."""
        st = self.force_stream
        if st is not None:  # ordered between two substeps of the simulator's own stream, after whatever the caller has enqueued so far
            st.wait_stream(torch.cuda.current_stream(self.device))
            if self.force_hooks:
                self.force_hooks[0]()
        with torch.cuda.stream(st) if st is not None else _null_ctx():
            yield
        if st is not None:
            # ... and before whatever the caller enqueues next on ITS stream: a substep launched there (sim.stepforward(), a whole-step graph) must
            # not read dof_f while the kernel above is still writing it
            ev = torch.cuda.Event()
            ev.record(st)
            torch.cuda.current_stream(self.device).wait_event(ev)
            if self.force_hooks:
                self.force_hooks[1]()

    def _force_launch(self, vid, f3):
        if self.drag_enabled:
            raise RuntimeError("Simulator: the drag state owns dof_f while drag is enabled (enable_drag); use drag_to / release instead of update_force / clear_force")
        with self._on_force_stream():
            check(lib().pn_sim_update_force(self.n_k, int(vid), f3.ctypes.data if f3 is not None else None, float(self.dx), ptr(self.IP_kernel),
                                            ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.dof_f), stream_ptr()), "update_force")

    def update_force(self, vid, f):  # solver.py:578-588
        """dof_f = the pick force `f` on IP `vid`, written whole by one launch on `force_stream` (or the current stream): it acts from the
        next substep enqueued after this call."""
        if self.drag_enabled:
            self._force_launch(vid, None)   # raises
        f3 = np.ascontiguousarray(f.detach().cpu().numpy() if torch.is_tensor(f) else f, dtype=np.float64)
        assert 0 <= int(vid) < self.n_IP and f3.shape == (3,)
        self._force_launch(vid, f3)

    def clear_force(self):  # solver.py:590-593
        self._force_launch(-1, None)

    # ------------------------------------------------------------------ the GUI's mouse drag on the device (gui.py:556-586, :833-841, :857-865)
    def enable_drag(self, scale=None):
        """From now on every stepforward() first writes dof_f with the GUI's spring force from the drag state (csrc/pn_drag.hip: k_drag_force):
        f = scale 1e5 (target - p0), |f| <= 5e5, p0 = the picked IP's get_IP_info() position of the state that substep starts from; all zero until
        drag_pick().  The state lives in device memory, so substeps captured into graphs after this call follow drag_to() without a recapture.
        While drag is enabled the drag state owns dof_f: update_force / clear_force raise.  May be called before initialize()."""
        if scale is not None:
            self.drag_force_scale = _check_scale(scale)
        if not self.drag_enabled:
            self.drag_enabled = True
            if self.dof is not None and self.device.type == "cuda":
                self._alloc_drag()
        return self

    def _alloc_drag(self):
        nb = int(lib().pn_sim_drag_bytes())
        if nb != 40:
            raise RuntimeError(f"libpienerf_hip.so's pn_drag_state has {nb} bytes, solver.py allocates 40")
        self._drag = torch.zeros(5, dtype=torchfloat, device=self.device)          # vid, active = 0; target = 0
        self._drag_work = torch.zeros(int(lib().pn_sim_drag_work_doubles()), dtype=torchfloat, device=self.device)
        check(lib().pn_sim_drag_set(ptr(self._drag), self.n_IP, -1, -1, float(self.drag_force_scale), None, stream_ptr()), "sim_drag_set")
        self.dof_f.zero_()

    def _drag_state(self):
        if not self.drag_enabled:
            raise RuntimeError("Simulator: drag is not enabled (call enable_drag() first)")
        if self._drag is None:
            raise RuntimeError("Simulator: the drag state lives on a GPU: initialize the simulator on a cuda device first")
        return self._drag

    def _unproject(self, depth0, x, y, pose, intrinsics, ip_pos):
        drag = self._drag_state()
        d = depth0.reshape(depth0.shape[-2], depth0.shape[-1]) if depth0.dim() >= 2 else depth0
        if d.dtype != torch.float32 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("drag: depth0 must be a contiguous fp32 [H, W] tensor on the GPU (a frame's depth_0)")
        H, W = d.shape
        intr = np.ascontiguousarray(np.asarray(intrinsics, np.float64).reshape(4))
        pose16 = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(-1)[-16:])
        n = 0
        if ip_pos is not None:
            if ip_pos.dtype != torch.float32 or not ip_pos.is_cuda or tuple(ip_pos.shape) != (self.n_IP, 3) or not ip_pos.is_contiguous():
                raise ValueError("drag_pick: ip_pos must be the contiguous fp32 [n_IP, 3] IP positions of a frame, on the GPU")
            n = self.n_IP
        with self._on_force_stream():
            check(lib().pn_sim_drag_unproject(ptr(d), W, H, float(x), float(y), intr.ctypes.data, pose16.ctypes.data, ptr(ip_pos), n, ptr(drag),
                                              ptr(self._drag_work), stream_ptr()), "sim_drag_unproject")

    def drag_pick(self, depth0, x, y, pose, intrinsics, ip_pos):
        """A ctrl-click at pixel (x, y) (gui.py:833-841): target = screen_to_world(x, y) against `depth0` ([H, W] fp32, the last frame's depth_0),
        the drag acts on the IP of `ip_pos` ([n_IP, 3] fp32, the IP positions that frame was rendered from) nearest to it.  Returns that IP's index:
        the drag's one read back to the host.  (x, y) are image pixels; a window's own offsets (dearpygui's +20 title bar, gui.py:809-812) are the
        caller's business."""
        self._unproject(depth0, x, y, pose, intrinsics, ip_pos)
        st = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            vid = self._drag[:1].view(torch.int32)[0].item()
        return int(vid)

    def drag_to(self, depth0, x, y, pose, intrinsics):
        """The cursor moved to pixel (x, y): target = screen_to_world(x, y) against `depth0` (gui.py:647-657).  No host read."""
        self._unproject(depth0, x, y, pose, intrinsics, None)

    def drag_scale(self, s):
        """Sets the GUI's force_scale (f = s 1e5 (target - p0))."""
        self.drag_force_scale = _check_scale(s)
        if self._drag is not None:
            with self._on_force_stream():
                check(lib().pn_sim_drag_set(ptr(self._drag), self.n_IP, -1, -1, float(self.drag_force_scale), None, stream_ptr()), "sim_drag_set")
        return self.drag_force_scale

    def drag_wheel(self, delta):
        """The mouse wheel's rule (gui.py:857-865) applied to the force scale; returns the new scale."""
        return self.drag_scale(wheel_force_scale(self.drag_force_scale, delta))

    def drag_hold(self, vid, target):
        """Drags IP `vid` toward the world point `target` (no unprojection): scripted drags and tests."""
        t = np.ascontiguousarray(np.asarray(target, np.float64).reshape(3))
        drag = self._drag_state()
        with self._on_force_stream():
            check(lib().pn_sim_drag_set(ptr(drag), self.n_IP, int(vid), 1, 0.0, t.ctypes.data, stream_ptr()), "sim_drag_set")

    def release(self):
        """Nothing picked (right click / Q, gui.py:821-826,843-849): every following substep gets dof_f = 0, as after clear_force()."""
        drag = self._drag_state()
        with self._on_force_stream():
            check(lib().pn_sim_drag_set(ptr(drag), self.n_IP, -1, 0, 0.0, None, stream_ptr()), "sim_drag_set")

    # ------------------------------------------------------------------ kinematic pins: the pinned points follow a scripted motion (csrc/pn_pins.hip)
    def enable_pin_motion(self):
        """From now on every stepforward() first writes rhs_gravity + stiff sum_p N_p^T u_p(t) (csrc/pn_pins.hip: k_pin_rhs) and runs the substep with
        it in the rhs_gravity slot: the pinned points follow u_p(t) (set_pin_motion, set_pin_offsets) through the reference's own penalty, the system
        matrix and Ainv unchanged.  t comes from a substep clock in device memory (substep k uses (k + 1) dt), so substeps captured into graphs after
        this call, or run frames ahead, move the pins at their own time.  No motion until set_pin_motion().  May be called before initialize();
        ValueError for a cloud without pinned points."""
        if not self.pin_enabled:
            if self.dof is not None:
                self._build_pins()   # raises for a cloud without pins, and pin motion then stays off
            self.pin_enabled = True
            if self.dof is not None and self.device.type == "cuda":
                self._alloc_pins()
        return self

    def _alloc_pins(self):
        nb = int(lib().pn_sim_pins_bytes())
        if nb != PIN_STATE_DOUBLES * 8:
            raise RuntimeError(f"libpienerf_hip.so's pn_pin_motion has {nb} bytes, solver.py allocates {PIN_STATE_DOUBLES * 8}")
        self._pin_state = torch.zeros(PIN_STATE_DOUBLES, dtype=torchfloat, device=self.device)    # clock 0, active 0, no motion
        self._rhs_ext = self.rhs_gravity.clone()
        # offset_p, zeros until set_pin_offsets(): allocated here and always passed, so that a substep captured into a graph holds its address
        self._pin_offsets = torch.zeros((self.n_pin, 3), dtype=torchfloat, device=self.device)

    def _enqueue_pin_rhs(self):
        """_rhs_ext = rhs_gravity + the pins' term at the clock's substep, then the clock + 1: two launches on the current stream.  Returns _rhs_ext."""
        check(lib().pn_sim_pins_rhs(self.n_k, self.n_pin, ptr(self._pins()), float(self.dt), float(self.stiff), ptr(self.rhs_gravity), ptr(self.pin_bg),
                                    ptr(self.pin_of), ptr(self.pin_N_csr), ptr(self.pin_rest), ptr(self._pin_offsets), ptr(self._rhs_ext), stream_ptr()),
              "sim_pins_rhs")
        return self._rhs_ext

    def _pins(self):
        if not self.pin_enabled:
            raise RuntimeError("Simulator: pin motion is not enabled (call enable_pin_motion() first)")
        if self._pin_state is None:
            raise RuntimeError("Simulator: the pin motion's state lives on a GPU: initialize the simulator on a cuda device first")
        return self._pin_state

    def set_pin_motion(self, translate=None, rotate=None):
        """The motion of the pinned points from the next substep on: u_p(t) = offset_p + T(t) + R(t)(X_p - c) - (X_p - c).
        translate = (A, hz, phase): T(t) = A sin(2 pi hz t + phase), A a 3-vector.  rotate = (axis, degrees, hz, phase, centre): R(t) the rotation about
        `axis` (normalised here) through `centre` (None: the centroid of the pinned rest points) by degrees sin(2 pi hz t + phase).  phase and centre may
        be left out; a part left out (None) is no motion of that kind.  Written on force_stream, between two substeps; the clock is left alone
        (reset_pin_clock)."""
        st = self._pins()
        T, R = pin_motion_params(translate, rotate, lambda: self.pin_rest.mean(dim=0).cpu().numpy())
        with self._on_force_stream():
            check(lib().pn_sim_pins_set(ptr(st), self.n_pin, 1, T.ctypes.data, R.ctypes.data, stream_ptr()), "sim_pins_set")

    def set_pin_offsets(self, u):
        """offset_p: a displacement per pinned point ([n_pin, 3], in the order of pin_ids), added to the scripted motion: host-scripted handles.  None
        zeroes it.  Copied into the simulator's own buffer on force_stream, between two substeps; offsets alone move the pins only once the motion is
        active (set_pin_motion(), with no arguments for offsets only)."""
        self._pins()
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
        st = self._pins()
        with self._on_force_stream():
            check(lib().pn_sim_pins_set(ptr(st), self.n_pin, 0, None, None, stream_ptr()), "sim_pins_set")

    def reset_pin_clock(self, k=0):
        """The next substep is substep `k` of the motion (t = (k + 1) dt)."""
        st = self._pins()
        if int(k) < 0:
            raise ValueError("reset_pin_clock: k >= 0")
        with self._on_force_stream():
            check(lib().pn_sim_pins_clock(ptr(st), int(k), stream_ptr()), "sim_pins_clock")

    def pin_clock(self):
        """Substeps since the last reset: the pin motion's one read back to the host.  It waits for force_stream (or the current stream) only: where
        the substeps run on other streams (the pipelined harness, a caller's own side stream) the value is defined after those have been waited for —
        drain_pipeline() / synchronize()."""
        st = self._pins()
        s = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            return int(st[:1].view(torch.int64)[0].item())

    def _pin_clock_keep(self):
        """The clock as a device copy (None without pin motion) for whoever warms the substep up and restores the state: _pin_clock_restore()."""
        return self._pin_state[:1].clone() if self._pin_state is not None else None

    def _pin_clock_restore(self, keep):
        if keep is not None:
            self._pin_state[:1].copy_(keep)

    # ------------------------------------------------------------------ contact with planes and spheres (csrc/pn_contact.hip)
    def enable_contact(self, stiffness=0.5, damping=0.5, friction=0.5, thickness=None):
        """From now on every stepforward() first writes rhs + the contact term (csrc/pn_contact.hip: k_contact_points, k_contact_rhs; include/pienerf_hip.h has the law) and
        runs the substep with it in the rhs_gravity slot: an explicit penalty against the colliders added with add_plane / add_sphere, evaluated at the
        integration points from the dof / dof_vel that substep starts from; the system matrix and Ainv unchanged.  thickness None: dx / 2 (integration
        points are cell centres, the visible surface lies about half a cell outside them).  The state lives in device memory, so substeps captured into
        graphs after this call follow set_collider / set_contact_params without a recapture.  May be called before initialize(); ValueError for
        parameters out of range (contact_params)."""
        p = contact_params(stiffness, damping, friction, 0.5 * float(self.dx) if thickness is None else thickness)
        self._contact_params = p
        if not self.contact_enabled:
            if self.dof is not None and self.Nx_csr is None:
                self._build_contact()
            self.contact_enabled = True
            if self.dof is not None and self.device.type == "cuda":
                self._alloc_contact()
        elif self._contact_state is not None:
            self._upload_contact_params()
        return self

    def _alloc_contact(self):
        nb = int(lib().pn_sim_contact_bytes())
        if nb != CONTACT_STATE_DOUBLES * 8:
            raise RuntimeError(f"libpienerf_hip.so's pn_contact_state has {nb} bytes, solver.py allocates {CONTACT_STATE_DOUBLES * 8}")
        self._contact_state = torch.zeros(CONTACT_STATE_DOUBLES, dtype=torchfloat, device=self.device)
        self._rhs_contact = self.rhs_gravity.clone()
        self._contact_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        self._upload_contact_params()
        for i, c in enumerate(self._colliders):
            if c is not None:
                self._upload_collider(i)

    def _contact(self):
        if not self.contact_enabled:
            raise RuntimeError("Simulator: contact is not enabled (call enable_contact() first)")
        return self._contact_state

    def _contact_on_gpu(self):
        st = self._contact()
        if st is None:
            raise RuntimeError("Simulator: the contact state lives on a GPU: initialize the simulator on a cuda device first")
        return st

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
        self._contact()
        old = self._contact_params
        new = [o if v is None else v for o, v in zip(old, (stiffness, damping, friction, thickness))]
        self._contact_params = contact_params(*new)
        if self._contact_state is not None:
            self._upload_contact_params()

    def add_plane(self, point, normal, velocity=None):
        """A half-space: the solid lies behind the plane through `point`, `normal` (normalised here) points out of it.  `velocity` (None: at rest) is the
        collider's own, for the relative velocity of damping and friction; the plane itself moves only when set_collider moves it.  Returns the
        collider's index; ValueError for a zero normal or a ninth collider."""
        self._contact()
        c = contact_plane(point, normal, velocity)
        return self._put_collider(self._free_slot(), c)

    def add_sphere(self, centre, radius, inside=False, velocity=None):
        """A solid sphere, or with inside=True a container the object lives in.  Returns the collider's index; ValueError for radius <= 0 or a ninth
        collider."""
        self._contact()
        c = contact_sphere(centre, radius, inside, velocity)
        return self._put_collider(self._free_slot(), c)

    def _slot(self, index):
        self._contact()
        i = int(index)
        if not 0 <= i < CONTACT_SLOTS or self._colliders[i] is None:
            raise ValueError(f"contact: there is no collider {index!r}")
        return i

    def set_collider(self, index, point=None, normal=None, centre=None, radius=None, inside=None, velocity=None):
        """Changes collider `index` from the next substep on; what is left None keeps its value.  A plane takes point / normal, a sphere centre / radius /
        inside, both velocity.  A moving collider is scripted from the host with this, per frame, with `velocity` given for the relative velocity.
        ValueError for an index without a collider, an argument of the other kind, or a value add_plane / add_sphere would refuse."""
        i = self._slot(index)
        t, g = self._colliders[i]
        vel = g[7:10] if velocity is None else velocity
        if t == CONTACT_PLANE:
            if centre is not None or radius is not None or inside is not None:
                raise ValueError(f"contact: collider {i} is a plane: it takes point, normal and velocity")
            c = contact_plane(g[0:3] if point is None else point, g[3:6] if normal is None else normal, vel)
        else:
            if point is not None or normal is not None:
                raise ValueError(f"contact: collider {i} is a sphere: it takes centre, radius, inside and velocity")
            c = contact_sphere(g[0:3] if centre is None else centre, g[6] if radius is None else radius, (t == CONTACT_CONTAINER) if inside is None else inside, vel)
        self._put_collider(i, c)

    def remove_collider(self, index):
        """Empties the slot: the collider acts on no further substep, its index may be handed out again."""
        self._put_collider(self._slot(index), None)

    def clear_colliders(self):
        self._contact()
        for i, c in enumerate(self._colliders):
            if c is not None:
                self._put_collider(i, None)

    def contact_state_bytes(self):
        """What the device state holds, packed from the mirror kept here (pack_contact_state): tests compare the device's bytes with it."""
        self._contact()
        return pack_contact_state(1, self._contact_params, self._colliders)

    def collider_state(self):
        """The pn_contact_state on the device (93 doubles), the simulator's own buffer: what the renderer's collider overlay reads
        (NeRFRenderer.set_collider_overlay; SimRenderHarness.draw_colliders), so a drawn collider is where set_collider last put it.  ValueError before
        enable_contact()."""
        if not self.contact_enabled:
            raise ValueError("collider_state: contact is not enabled (call enable_contact() first)")
        return self._contact_on_gpu()

    def collider_types(self):
        """The type of every collider slot (CONTACT_EMPTY / _PLANE / _SPHERE / _CONTAINER), from the host mirror."""
        return [CONTACT_EMPTY if c is None else int(c[0]) for c in self._colliders]

    def _enqueue_contact_rhs(self, rhs_in, one_launch=False):
        """_rhs_contact = rhs_in + the contact term of the current dof / dof_vel, on the current stream.  Returns _rhs_contact.  Two launches: the law at
        every point into _contact_accel, then the per-kernel sums (the measured faster form).  one_launch=True (tools/time_contact.py, tests):
        the form in which every entry evaluates its point itself — the same bits in _rhs_contact, _contact_accel left as it is."""
        check(lib().pn_sim_contact_rhs(self.n_k, self.n_IP, ptr(self._contact_on_gpu()), float(self.dt), float(self.dx), ptr(self.dof), ptr(self.dof_vel),
                                       ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer),
                                       ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_contact), None if one_launch else ptr(self._contact_accel), stream_ptr()),
              "sim_contact_rhs")
        return self._rhs_contact

    def contact_accel(self):
        """[n_IP, 3]: the contact acceleration a_i of every integration point in the last substep enqueued (zeros for a point not in contact).  The
        simulator's own buffer, overwritten by the next substep."""
        self._contact_on_gpu()
        return self._contact_accel

    def contact_count(self):
        """Integration points in contact in the last substep (a_i != 0: a penetrated collider always pushes, a_n > 0): contact's one read back to the
        host.  Like pin_clock() it waits for force_stream (or the current stream) only."""
        self._contact_on_gpu()
        s = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            return int((self._contact_accel != 0.0).any(dim=1).sum().item())

    # ------------------------------------------------------------------ force fields: wind, vortex, blast, air drag (csrc/pn_fields.hip)
    def enable_fields(self):
        """From now on every stepforward() first writes rhs + the field term (csrc/pn_fields.hip: k_field_points, k_field_rhs; include/pienerf_hip.h
        has the law) and runs the substep with it in the rhs_gravity slot, last in the chain rhs_gravity -> pins -> contact -> fields: body forces from
        the fields added with add_wind / add_air_drag / add_vortex / add_radial, evaluated at the integration points from the dof / dof_vel that
        substep starts from, at t = k dt of a substep clock in device memory; the system matrix and Ainv unchanged.  The state lives in device memory,
        so substeps captured into graphs after this call, or run frames ahead, follow set_field / reset_field_clock without a recapture.  After
        stop_fields() it switches the stage on again.  May be called before initialize()."""
        self._fields_active = True
        if not self.fields_enabled:
            if self.dof is not None and self.Nx_csr is None:
                self._build_contact()   # the stage reads contact's tables (Nx_csr)
            self.fields_enabled = True
            if self.dof is not None and self.device.type == "cuda":
                self._alloc_fields()
        elif self._field_state is not None:
            self._upload_fields_active()
        return self

    def stop_fields(self):
        """active = 0: every following substep gets its right-hand side without the field term, bit for bit; the fields stay in their slots and the
        clock keeps counting.  enable_fields() switches the stage on again."""
        self._fields_on()
        self._fields_active = False
        if self._field_state is not None:
            self._upload_fields_active()

    def _alloc_fields(self):
        nb = int(lib().pn_sim_fields_bytes())
        if nb != FIELD_STATE_DOUBLES * 8 or FIELD_DTYPE.itemsize != 144:
            raise RuntimeError(f"libpienerf_hip.so's pn_field_state has {nb} bytes, solver.py's FIELD_STATE_DTYPE {FIELD_STATE_DOUBLES * 8}")
        self._field_state = torch.zeros(FIELD_STATE_DOUBLES, dtype=torchfloat, device=self.device)   # clock 0, inactive, every slot empty
        self._rhs_fields = self.rhs_gravity.clone()
        self._field_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        for i, f in enumerate(self._fields):
            if f is not None:
                self._upload_field(i)
        self._upload_fields_active()

    def _fields_on(self):
        if not self.fields_enabled:
            raise RuntimeError("Simulator: force fields are not enabled (call enable_fields() first)")
        return self._field_state

    def _fields_on_gpu(self):
        st = self._fields_on()
        if st is None:
            raise RuntimeError("Simulator: the field state lives on a GPU: initialize the simulator on a cuda device first")
        return st

    def _upload_fields_active(self):
        with self._on_force_stream():
            check(lib().pn_sim_fields_set_active(ptr(self._field_state), int(self._fields_active), stream_ptr()), "sim_fields_set_active")

    def _upload_field(self, i):
        f = self._fields[i]
        t, g = (FIELD_EMPTY, None) if f is None else (f[0], np.ascontiguousarray(f[1]))
        with self._on_force_stream():
            check(lib().pn_sim_fields_set_field(ptr(self._field_state), int(i), int(t), g.ctypes.data if g is not None else None, stream_ptr()),
                  "sim_fields_set_field")

    def _put_field(self, i, t, args):
        """Slot i = the field of kind t built from `args` (None: empty), in the mirror and, once allocated, on the device through force_stream: the
        change lands between two substeps."""
        self._fields[i] = None if t is None else FIELD_BUILDERS[t](**args)
        self._field_args[i] = None if t is None else (t, dict(args))
        if self._field_state is not None:
            self._upload_field(i)
        return i

    def _free_field_slot(self):
        self._fields_on()
        for i, f in enumerate(self._fields):
            if f is None:
                return i
        raise ValueError(f"fields: all {FIELD_SLOTS} field slots are in use (remove_field frees one)")

    def add_wind(self, velocity, drag=2.0, gust=0.0, hz=0.0, phase=0.0, wave=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), start=0.0, stop=None):
        """A wind: a_i += min(drag, 1/dt) (u - v_i), u = velocity (1 + gust sin(2 pi (hz t - wave.(x_i - origin)) + phase)), while start <= t < stop
        (stop None: for ever).  Returns the field's index; ValueError for drag < 0, gust outside [0, 1], a non-finite value, stop < start or a ninth field."""
        i = self._free_field_slot()
        return self._put_field(i, FIELD_WIND, dict(velocity=velocity, drag=drag, gust=gust, hz=hz, phase=phase, wave=wave, origin=origin, start=start, stop=stop))

    def add_air_drag(self, drag):
        """Still air: a wind of zero velocity, that is, mass-proportional damping a_i -= min(drag, 1/dt) v_i.  Returns the field's index."""
        return self.add_wind((0.0, 0.0, 0.0), drag=drag)

    def add_vortex(self, point, axis, omega, radius, drag=2.0, start=0.0, stop=None):
        """A vortex about the line through `point` along `axis` (normalised here): a_i += min(drag, 1/dt) fall(rho) (omega axis x r - v_i), rho the
        distance from the axis, fall(q) = max(1 - q / radius, 0)^2.  Returns the field's index; ValueError for a zero axis, radius <= 0 or a ninth field."""
        i = self._free_field_slot()
        return self._put_field(i, FIELD_VORTEX, dict(point=point, axis=axis, omega=omega, radius=radius, drag=drag, start=start, stop=stop))

    def add_radial(self, centre, strength, radius, start=0.0, stop=None):
        """A radial field, with a short window a blast: a_i += s fall(|x_i - centre|) (x_i - centre) / |x_i - centre|, away from the centre for
        strength > 0, |s| = min(|strength|, radius / (2 dt^2)).  Returns the field's index; ValueError for radius <= 0 or a ninth field."""
        i = self._free_field_slot()
        return self._put_field(i, FIELD_RADIAL, dict(centre=centre, strength=strength, radius=radius, start=start, stop=stop))

    def _field_slot(self, index):
        self._fields_on()
        try:
            i = int(index)
        except (TypeError, ValueError):
            i = -1
        if not 0 <= i < FIELD_SLOTS or self._fields[i] is None:
            raise ValueError(f"fields: there is no field {index!r}")
        return i

    def set_field(self, index, **changed):
        """Changes field `index` from the next substep on: the arguments of its add_wind / add_vortex / add_radial call, what is left out keeps its
        value.  ValueError for an index without a field, an argument of another kind of field, or a value the add_ call would refuse; the field then
        stays as it was."""
        i = self._field_slot(index)
        t, args = self._field_args[i]
        other = sorted(set(changed) - set(FIELD_ARGS[t]))
        if other:
            raise ValueError(f"fields: field {i} is {FIELD_KINDS[t]}: it takes {', '.join(FIELD_ARGS[t])}, not {', '.join(other)}")
        new = dict(args, **changed)
        FIELD_BUILDERS[t](**new)   # raises before anything changes
        self._put_field(i, t, new)

    def remove_field(self, index):
        """Empties the slot: the field acts on no further substep, its index may be handed out again."""
        self._put_field(self._field_slot(index), None, None)

    def clear_fields(self):
        self._fields_on()
        for i, f in enumerate(self._fields):
            if f is not None:
                self._put_field(i, None, None)

    def field_types(self):
        """The type of every field slot (FIELD_EMPTY / _WIND / _VORTEX / _RADIAL), from the host mirror."""
        return [FIELD_EMPTY if f is None else int(f[0]) for f in self._fields]

    def reset_field_clock(self, k=0):
        """The next substep is substep `k` of the fields' clock (t = k dt)."""
        st = self._fields_on_gpu()
        if int(k) < 0:
            raise ValueError("reset_field_clock: k >= 0")
        with self._on_force_stream():
            check(lib().pn_sim_fields_clock(ptr(st), int(k), stream_ptr()), "sim_fields_clock")

    def field_clock(self):
        """Substeps since the last reset: the fields' one read back to the host.  Like pin_clock() it waits for force_stream (or the current stream)
        only."""
        st = self._fields_on_gpu()
        s = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            return int(st[:1].view(torch.int64)[0].item())

    def _field_clock_keep(self):
        """The clock as a device copy (None without fields) for whoever warms the substep up and restores the state: _field_clock_restore()."""
        return self._field_state[:1].clone() if self._field_state is not None else None

    def _field_clock_restore(self, keep):
        if keep is not None:
            self._field_state[:1].copy_(keep)

    def field_state_bytes(self, k=0):
        """What the device state holds when its clock reads `k`, packed from the mirror kept here (pack_field_state): tests compare the device's bytes
        with it."""
        self._fields_on()
        return pack_field_state(int(self._fields_active), self._fields, k)

    def _enqueue_fields_rhs(self, rhs_in):
        """_rhs_fields = rhs_in + the field term of the current dof / dof_vel at the clock's substep, then the clock + 1: three launches on the current
        stream.  Returns _rhs_fields."""
        check(lib().pn_sim_fields_rhs(self.n_k, self.n_IP, ptr(self._fields_on_gpu()), float(self.dt), float(self.dx), ptr(self.dof), ptr(self.dof_vel),
                                      ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer),
                                      ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_fields), ptr(self._field_accel), stream_ptr()), "sim_fields_rhs")
        return self._rhs_fields

    def field_accel(self):
        """[n_IP, 3]: the fields' acceleration a_i of every integration point in the last substep enqueued.  The simulator's own buffer, overwritten
        by the next substep."""
        self._fields_on_gpu()
        return self._field_accel

    # ------------------------------------------------------------------ self-contact (csrc/pn_selfcontact.hip)
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
        if not self.self_contact_enabled:
            if self.dof is not None and self.Nx_csr is None:
                self._build_contact()   # the stage reads contact's tables (Nx_csr)
            self.self_contact_enabled = True
            if self.dof is not None and self.device.type == "cuda":
                self._alloc_self_contact()
        elif self._self_state is not None:
            self._upload_self_params()
        return self

    def _alloc_self_contact(self):
        nb = int(lib().pn_sim_self_bytes())
        if nb != SELF_STATE_DOUBLES * 8:
            raise RuntimeError(f"libpienerf_hip.so's pn_selfcontact_state has {nb} bytes, solver.py's SELF_STATE_DTYPE {SELF_STATE_DOUBLES * 8}")
        self._self_state = torch.zeros(SELF_STATE_DOUBLES, dtype=torchfloat, device=self.device)   # inactive, nothing overflowed
        self._self_work = torch.zeros(int(lib().pn_sim_self_work_bytes(self.n_IP)) // 8, dtype=torchfloat, device=self.device)
        self._rhs_self = self.rhs_gravity.clone()
        self._self_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        self._self_X = self.IP_pos.to(dtype=torchfloat).contiguous()
        self._upload_self_params()

    def _self_contact(self):
        if not self.self_contact_enabled:
            raise RuntimeError("Simulator: self-contact is not enabled (call enable_self_contact() first)")
        return self._self_state

    def _self_contact_on_gpu(self):
        st = self._self_contact()
        if st is None:
            raise RuntimeError("Simulator: the self-contact state lives on a GPU: initialize the simulator on a cuda device first")
        return st

    def _upload_self_params(self):
        p = np.ascontiguousarray(self._self_params)
        with self._on_force_stream():
            check(lib().pn_sim_self_set_params(ptr(self._self_state), int(self._self_active), p.ctypes.data, stream_ptr()), "sim_self_set_params")

    def set_self_contact_params(self, stiffness=None, damping=None, friction=None, thickness=None, exclusion=None):
        """New values for the parameters given (None keeps one), from the next substep on.  ValueError for a value out of range."""
        self._self_contact()
        new = [o if v is None else v for o, v in zip(self._self_params, (stiffness, damping, friction, thickness, exclusion))]
        self._self_params = self_contact_params(*new)
        if self._self_state is not None:
            self._upload_self_params()

    def stop_self_contact(self):
        """active = 0: every following substep gets its right-hand side without the self-contact term, bit for bit; the parameters stay.
        enable_self_contact() switches the stage on again."""
        self._self_contact()
        self._self_active = False
        if self._self_state is not None:
            self._upload_self_params()

    def self_contact_state_bytes(self, overflowed=0):
        """What the device state holds after `overflowed` overflowed substeps, packed from the mirror kept here (pack_self_contact_state): tests
        compare the device's bytes with it."""
        self._self_contact()
        return pack_self_contact_state(int(self._self_active), self._self_params, overflowed)

    def _enqueue_self_rhs(self, rhs_in):
        """_rhs_self = rhs_in + the self-contact term of the current dof / dof_vel: eight launches on the current stream.  Returns _rhs_self."""
        check(lib().pn_sim_self_rhs(self.n_k, self.n_IP, ptr(self._self_contact_on_gpu()), ptr(self._self_work), float(self.dt), float(self.dx),
                                    ptr(self.dof), ptr(self.dof_vel), ptr(self._self_X), ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx),
                                    ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer), ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_self),
                                    ptr(self._self_accel), stream_ptr()), "sim_self_rhs")
        return self._rhs_self

    def self_contact_accel(self):
        """[n_IP, 3]: the self-contact acceleration a_i of every integration point in the last substep enqueued (zeros for a point without a partner).
        The simulator's own buffer, overwritten by the next substep."""
        self._self_contact_on_gpu()
        return self._self_accel

    def _self_read(self, f):
        s = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            return f()

    def self_contact_count(self):
        """Integration points with a_i != 0 in the last substep.  Like contact_count() it waits for force_stream (or the current stream) only."""
        self._self_contact_on_gpu()
        return self._self_read(lambda: int((self._self_accel != 0.0).any(dim=1).sum().item()))

    def self_contact_overflows(self):
        """Substeps whose stage was switched off because a bucket of the hashed grid held more than 64 points (the body has collapsed): the state's
        counter read back to the host."""
        st = self._self_contact_on_gpu()
        return self._self_read(lambda: int(st[1:2].view(torch.int64).item()))

    def bind_points(self, points, normals=None):
        """Binds arbitrary rest-space points [V,3] (the space of IP_pos and of extract_geometry's mesh; taken in fp64) to this simulator: a
        PointBinding (simulator/binding.py) whose warp() gives their positions — and, with rest `normals` [V,3], their normals — under the current or a
        snapshot dof in one HIP launch.  Initialisation-time torch; needs only what precompute() builds.  A point takes the 8 kernels of its own
        kernel-grid cell when all are active, else those of its nearest integration point; ValueError when a point's binding does not reproduce it
        at the rest state to 1e-9."""
        from .binding import bind_points
        return bind_points(self, points, normals)

    def update_pos(self):  # solver.py:604-617 (update_pos_kernel) — only used by OutputToPly
        d = self.dof.view(self.n_k, 10, 3)[self.pts_kernel.long()]
        self.pos = torch.einsum("nic,nicr->nr", self.pts_Nx, d)
        return self.pos
