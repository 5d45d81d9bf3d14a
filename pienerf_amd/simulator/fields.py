"""Force fields: wind, vortex, blast, air drag (csrc/pn_fields.hip).  A pn_field_state in device memory with its own substep clock, read
by three launches in front of every substep (k_field_points, k_field_rhs, k_field_tick) that write _rhs_fields = (the chain so far) + the field term of
the state and the time the substep starts from.  The slots are mirrored on the host, so they may be set before initialize() and are uploaded when the
state is allocated."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, _vec3, torchfloat

__all__ = ["FIELD_SLOTS", "FIELD_EMPTY", "FIELD_WIND", "FIELD_VORTEX", "FIELD_RADIAL", "FIELD_DTYPE", "FIELD_STATE_DTYPE", "FIELD_STATE_DOUBLES", "FIELD_ARGS",
           "FIELD_KINDS", "FIELD_BUILDERS", "field_wind", "field_vortex", "field_radial", "pack_field_state", "FieldsMixin"]   # what solver.py re-exports

FIELD_SLOTS = 8            # pn_field_state's field slots (include/pienerf_hip.h: PN_FIELD_SLOTS)
FIELD_EMPTY, FIELD_WIND, FIELD_VORTEX, FIELD_RADIAL = 0, 1, 2, 3
# pn_force_field / pn_field_state (include/pienerf_hip.h) as numpy records: 144 and 1168 bytes = pn_sim_fields_bytes(), checked in _alloc_fields
FIELD_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("c", "<f8"), ("s", "<f8"), ("R", "<f8"),
                        ("g", "<f8"), ("f", "<f8"), ("phi", "<f8"), ("kv", "<f8", (3,)), ("t0", "<f8"), ("t1", "<f8")])
FIELD_STATE_DTYPE = np.dtype([("k", "<i8"), ("active", "<i4"), ("n", "<i4"), ("f", FIELD_DTYPE, (FIELD_SLOTS,))])
FIELD_STATE_DOUBLES = FIELD_STATE_DTYPE.itemsize // 8
assert FIELD_DTYPE.itemsize == 144
# the arguments each kind of field takes, with the defaults of add_wind / add_vortex / add_radial: what set_field(index, **changed) may change
FIELD_ARGS = {
    FIELD_WIND: dict(velocity=None, drag=2.0, gust=0.0, hz=0.0, phase=0.0, wave=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), start=0.0, stop=None),
    FIELD_VORTEX: dict(point=None, axis=None, omega=None, radius=None, drag=2.0, start=0.0, stop=None),
    FIELD_RADIAL: dict(centre=None, strength=None, radius=None, start=0.0, stop=None),
}
FIELD_KINDS = {FIELD_WIND: "a wind", FIELD_VORTEX: "a vortex", FIELD_RADIAL: "a radial field"}

STAGE = Stage(name="fields", flag="fields_enabled", state="_field_state", subject="force fields are", owner="the field state", enable="enable_fields",
              struct="pn_field_state", nbytes=FIELD_STATE_DOUBLES * 8, sized_by="solver.py's FIELD_STATE_DTYPE", init="_init_fields", alloc="_alloc_fields",
              enqueue="_enqueue_fields_rhs", tables="_need_Nx_csr", writes="rhs", clock=True)


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


class FieldsMixin:
    def _init_fields(self):
        self.fields_enabled = False
        self._fields_active = False
        self._field_state = self._rhs_fields = self._field_accel = None
        self._fields = [None] * FIELD_SLOTS        # (type, geom17) per slot
        self._field_args = [None] * FIELD_SLOTS    # the arguments each was built from: what set_field() changes

    def enable_fields(self):
        """From now on every stepforward() first writes rhs + the field term (csrc/pn_fields.hip: k_field_points, k_field_rhs; include/pienerf_hip.h
        has the law) and runs the substep with it in the rhs_gravity slot, behind contact in the chain rhs_gravity -> pins -> contact -> fields: body
        forces from the fields added with add_wind / add_air_drag / add_vortex / add_radial, evaluated at the integration points from the dof / dof_vel that
        substep starts from, at t = k dt of a substep clock in device memory; the system matrix and Ainv unchanged.  The state lives in device memory,
        so substeps captured into graphs after this call, or run frames ahead, follow set_field / reset_field_clock without a recapture.  After
        stop_fields() it switches the stage on again.  May be called before initialize()."""
        self._fields_active = True
        if not self._switch_on(STAGE) and self._field_state is not None:
            self._upload_fields_active()
        return self

    def stop_fields(self):
        """active = 0: every following substep gets its right-hand side without the field term, bit for bit; the fields stay in their slots and the
        clock keeps counting.  enable_fields() switches the stage on again."""
        self._stage_state(STAGE, gpu=False)
        self._fields_active = False
        if self._field_state is not None:
            self._upload_fields_active()

    def _alloc_fields(self):
        self._new_state(STAGE)   # clock 0, inactive, every slot empty
        self._rhs_fields = self.rhs_gravity.clone()
        self._field_accel = torch.zeros((self.n_IP, 3), dtype=torchfloat, device=self.device)
        for i, f in enumerate(self._fields):
            if f is not None:
                self._upload_field(i)
        self._upload_fields_active()

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
        self._stage_state(STAGE, gpu=False)
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
        self._stage_state(STAGE, gpu=False)
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
        self._stage_state(STAGE, gpu=False)
        for i, f in enumerate(self._fields):
            if f is not None:
                self._put_field(i, None, None)

    def field_types(self):
        """The type of every field slot (FIELD_EMPTY / _WIND / _VORTEX / _RADIAL), from the host mirror."""
        return [FIELD_EMPTY if f is None else int(f[0]) for f in self._fields]

    def reset_field_clock(self, k=0):
        """The next substep is substep `k` of the fields' clock (t = k dt)."""
        st = self._stage_state(STAGE)
        if int(k) < 0:
            raise ValueError("reset_field_clock: k >= 0")
        with self._on_force_stream():
            check(lib().pn_sim_fields_clock(ptr(st), int(k), stream_ptr()), "sim_fields_clock")

    def field_clock(self):
        """Substeps since the last reset: the fields' one read back to the host.  Like pin_clock() it waits for force_stream (or the current stream)
        only."""
        return self._read_clock(STAGE)

    def _field_clock_keep(self):
        """The clock as a device copy (None without fields); keep_state() / restore_state() are the whole state's."""
        return self._clock_keep(STAGE)

    def _field_clock_restore(self, keep):
        self._clock_restore(STAGE, keep)

    def field_state_bytes(self, k=0):
        """What the device state holds when its clock reads `k`, packed from the mirror kept here (pack_field_state): tests compare the device's bytes
        with it."""
        self._stage_state(STAGE, gpu=False)
        return pack_field_state(int(self._fields_active), self._fields, k)

    def _enqueue_fields_rhs(self, rhs_in):
        """_rhs_fields = rhs_in + the field term of the current dof / dof_vel at the clock's substep, then the clock + 1: three launches on the current
        stream.  Returns _rhs_fields."""
        check(lib().pn_sim_fields_rhs(self.n_k, self.n_IP, ptr(self._stage_state(STAGE)), float(self.dt), float(self.dx), ptr(self.dof), ptr(self.dof_vel),
                                      ptr(self.IP_kernel), ptr(self.IP_rho), ptr(self.IP_Nx), ptr(self.kernel_bg), ptr(self.kernel_cnt), ptr(self.buffer),
                                      ptr(self.Nx_csr), ptr(rhs_in), ptr(self._rhs_fields), ptr(self._field_accel), stream_ptr()), "sim_fields_rhs")
        return self._rhs_fields

    def field_accel(self):
        """[n_IP, 3]: the fields' acceleration a_i of every integration point in the last substep enqueued.  The simulator's own buffer, overwritten
        by the next substep."""
        self._stage_state(STAGE)
        return self._field_accel
