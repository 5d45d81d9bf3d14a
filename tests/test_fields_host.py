"""Force fields, host side, on CPU (no kernel is launched): the law's properties on its numpy restatement (tests/fields_reference.py), the restatement
against physics on the CPU oracle (the cases of DESIGN.md 4.15, directions only), the C ABI and its argument checks, the packed state against the
header's layout, the Simulator's setters and main_render's arguments."""
import ctypes
import re
import struct

import numpy as np
import pytest

from conftest import make_oracle_sim
from fields_reference import OracleFields, air_drag, field_accel, kernel_order_walk, radial, vortex, wind
from test_contact_host import _c_layout, _cpu_sim, _header

FIELD_SYMBOLS = ("pn_sim_fields_bytes", "pn_sim_fields_set_active", "pn_sim_fields_set_field", "pn_sim_fields_clock", "pn_sim_fields_rhs")
PN_ERR_ARG = 1
DT = 1e-2


# ---------------------------------------------------------------- the law's properties
def _cloud(n=4000, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(n, 3)), rng.normal(scale=2.0, size=(n, 3))


GUSTY = dict(velocity=(5.0, 1.0, -2.0), drag=3.0, gust=0.6, hz=2.0, phase=0.4, wave=(0.5, 0.0, 0.25), origin=(0.1, 0.0, -0.2))
SWIRL = dict(point=(0.1, 0.0, -0.1), axis=(0.2, 1.0, -0.1), omega=6.0, radius=0.8, drag=4.0)
BLAST = dict(centre=(0.2, -0.3, 0.1), strength=400.0, radius=0.9)
KINDS = {"wind": (wind, GUSTY), "vortex": (vortex, SWIRL), "radial": (radial, BLAST)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_nothing_is_added_outside_the_window(kind):
    make, kw = KINDS[kind]
    x, v = _cloud()
    k0, k1 = 5, 9
    f = make(**kw, start=k0 * DT, stop=k1 * DT)
    always = field_accel([make(**kw)], x, v, 0.0, DT)
    assert np.abs(always).max() > 1.0
    for k, inside in ((0, False), (k0 - 1, False), (k0, True), (k1 - 1, True), (k1, False), (k1 + 1, False), (1000, False)):   # t = t0 is inside, t = t1 is not
        a = field_accel([f], x, v, k * DT, DT)
        assert bool(a.any()) == inside, (kind, k)
        if not inside:
            assert np.array_equal(a, np.zeros_like(a))
    # an open end: t1 = +inf
    assert field_accel([make(**kw, start=k0 * DT)], x, v, 1e9, DT).any()
    # an empty window acts never
    assert not field_accel([make(**kw, start=k0 * DT, stop=k0 * DT)], x, v, k0 * DT, DT).any()


def test_vortex_and_radial_are_exactly_zero_at_and_beyond_R():
    R = 0.5
    n = np.array([0.0, 1.0, 0.0])
    rho = np.array([0.0, 0.25, R * (1 - 1e-12), R, R * (1 + 1e-12), 0.75, 10.0])
    x = np.stack([rho, np.linspace(-1, 1, len(rho)), np.zeros(len(rho))], axis=1)     # distance rho from the y axis, any height
    v = np.full_like(x, 3.0)
    a = field_accel([vortex((0, 0, 0), n, 6.0, R, drag=4.0)], x, v, 0.0, DT)
    assert a[:3].any(axis=1).all() and np.array_equal(a[3:], np.zeros((4, 3)))
    assert np.abs(a[2]).max() < 1e-20                                                 # continuous at R: fall ~ (1e-12)^2
    y = np.stack([rho, np.zeros(len(rho)), np.zeros(len(rho))], axis=1)
    b = field_accel([radial((0, 0, 0), 400.0, R)], y, v, 0.0, DT)
    assert b[1:3].any(axis=1).all() and np.array_equal(b[3:], np.zeros((4, 3)))
    assert np.array_equal(b[0], np.zeros(3))                                          # at the centre: nothing (no direction to push in)
    assert b[1, 0] > 0 and field_accel([radial((0, 0, 0), -400.0, R)], y, v, 0.0, DT)[1, 0] < 0   # away for s > 0, toward for s < 0
    # the vortex drags toward the rigid rotation omega n x r: a point moving with it feels nothing
    r = np.array([[0.2, 0.3, 0.1]])
    assert np.array_equal(field_accel([vortex((0, 0, 0), n, 6.0, R, drag=4.0)], r, 6.0 * np.cross(n, r), 0.0, DT), np.zeros((1, 3)))


def test_fields_add_in_index_order_and_empty_slots_add_nothing():
    x, v = _cloud()
    fs = [wind(**GUSTY), vortex(**SWIRL), radial(**BLAST), air_drag(1.5)]
    dense = field_accel(fs, x, v, 0.07, DT)
    gaps = field_accel([None, fs[0], None, None, fs[1], fs[2], None, fs[3]], x, v, 0.07, DT)
    assert np.array_equal(dense, gaps)
    one_by_one = np.zeros_like(x)
    for f in fs:
        one_by_one = one_by_one + field_accel([f], x, v, 0.07, DT)
    assert np.array_equal(dense, one_by_one)
    assert not np.array_equal(dense, field_accel(fs[::-1], x, v, 0.07, DT)) and np.allclose(dense, field_accel(fs[::-1], x, v, 0.07, DT), rtol=1e-12, atol=1e-9)


def test_the_clamps():
    x, v = _cloud()
    for make, kw in ((wind, GUSTY), (vortex, SWIRL)):
        huge, edge = make(**dict(kw, drag=1e9)), make(**dict(kw, drag=1.0 / DT))
        assert np.array_equal(field_accel([huge], x, v, 0.03, DT), field_accel([edge], x, v, 0.03, DT))
    # still air: a point's own response per step, dt c_eff |v|, is at most |v|
    a = field_accel([air_drag(1e9)], x, v, 0.0, DT)
    assert np.array_equal(a, (1.0 / DT) * (0.0 - v))
    # the blast: dt^2 |a| <= R / 2, and the sign is kept
    for s in (1e12, -1e12):
        b = field_accel([radial(BLAST["centre"], s, BLAST["radius"])], x, v, 0.0, DT)
        assert np.array_equal(b, field_accel([radial(BLAST["centre"], np.sign(s) * BLAST["radius"] / (2 * DT * DT), BLAST["radius"])], x, v, 0.0, DT))
        assert (DT * DT * np.linalg.norm(b, axis=1) <= 0.5 * BLAST["radius"] * (1 + 1e-12)).all() and b.any()


# ---------------------------------------------------------------- the restatement against physics (oracle only, directions only)
N_PHYS, N_TAIL, N_HELD = 120, 40, 20
FORCE = np.array([300.0, 100.0, -200.0])


@pytest.fixture(scope="module")
def physics(small_cloud, small_opt):
    """Computed once: the small pinned chair dragged by the pick force for 20 substeps and released, 120 substeps in all, without a field, in still air
    with c = 5 and c = 1e9, and in a wind (5, 0, 0) with c = 2: (mean kinetic energy over the last 40 steps, peak point displacement, mean
    x-displacement at the end)."""
    out = {}
    for name, fs in (("none", []), ("air5", [air_drag(5.0)]), ("air1e9", [air_drag(1e9)]), ("wind", [wind((5.0, 0.0, 0.0), drag=2.0)])):
        o = OracleFields(make_oracle_sim(small_cloud, small_opt), fs)
        assert o.ref.n_IP == 432 and o.ref.n_k == 139
        x0 = o.ip_positions().copy()
        o.ref.update_force(o.ref.n_IP // 2, FORCE)
        ke, peak = [], 0.0
        for k in range(N_PHYS):
            if k == N_HELD:
                o.ref.clear_force()
            o.step()
            ke.append(o.kinetic_energy())
            peak = max(peak, float(np.linalg.norm(o.ip_positions() - x0, axis=1).max()))
        out[name] = (float(np.mean(ke[-N_TAIL:])), peak, float((o.ip_positions() - x0)[:, 0].mean()))
        print(f"{name}: mean kinetic energy over the last {N_TAIL} of {N_PHYS} substeps {out[name][0]:.4g}, peak point displacement {out[name][1]:.4g}, "
              f"mean x-displacement at the end {out[name][2]:+.4g}")
    return out


def test_still_air_damps_the_released_chair(physics):
    assert physics["air5"][0] < physics["none"][0]


def test_clamped_drag_stays_bounded(physics):
    assert np.isfinite(physics["air1e9"]).all() and physics["air1e9"][1] < physics["none"][1]


def test_wind_pushes_the_chair_downwind(physics):
    assert np.isfinite(physics["wind"]).all() and physics["wind"][2] > physics["none"][2]


# ---------------------------------------------------------------- the C ABI
def test_field_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    from pienerf_amd.simulator import solver
    text = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in FIELD_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    assert _lib.lib().pn_sim_fields_bytes() == solver.FIELD_STATE_DOUBLES * 8 == solver.FIELD_STATE_DTYPE.itemsize == 1168
    assert solver.FIELD_DTYPE.itemsize == 144
    assert len(_lib.SIGNATURES["pn_sim_fields_rhs"][1]) == 18 and _lib.SIGNATURES["pn_sim_fields_rhs"][1] == _lib.SIGNATURES["pn_sim_contact_rhs"][1]


def test_packed_state_has_the_headers_layout():
    from pienerf_amd.simulator import solver
    text = _header().replace("int64_t", "double")          # 8 bytes, 8-aligned: what the layout walk needs to know of it
    fld, fld_size, fld_al = _c_layout(text, "pn_force_field", {})
    st, st_size, _ = _c_layout(text, "pn_field_state", {"pn_force_field": (fld_size, fld_al)})
    for members, size, dt in ((fld, fld_size, solver.FIELD_DTYPE), (st, st_size, solver.FIELD_STATE_DTYPE)):
        assert size == dt.itemsize
        assert [(n, o) for n, o in members] == [(n, dt.fields[n][1]) for n in dt.names]
    assert (fld_size, st_size) == (144, 1168) and solver.FIELD_SLOTS == 8 and "#define PN_FIELD_SLOTS 8" in text
    for i, n in enumerate(("PN_FIELD_EMPTY", "PN_FIELD_WIND", "PN_FIELD_VORTEX", "PN_FIELD_RADIAL")):
        assert re.search(n + r"\s*=\s*%d\b" % i, text), n
    assert (solver.FIELD_EMPTY, solver.FIELD_WIND, solver.FIELD_VORTEX, solver.FIELD_RADIAL) == (0, 1, 2, 3)
    # the bytes, read back with struct at the header's offsets
    fs = [None] * 8
    fs[1] = solver.field_wind((5.0, 0.0, 1.0), drag=3.0, gust=0.5, hz=2.0, phase=0.25, wave=(0.5, 0.0, 0.25), origin=(0.1, 0.2, 0.3), start=0.5, stop=2.0)
    fs[4] = solver.field_vortex((0.1, 0.2, 0.3), (0.0, 2.0, 0.0), 6.0, 0.8, drag=4.0)
    fs[6] = solver.field_radial((1.0, 2.0, 3.0), -400.0, 0.9, start=0.05, stop=0.08)
    b = solver.pack_field_state(1, fs, k=7)
    assert len(b) == 1168
    assert struct.unpack_from("<qii", b, 0) == (7, 1, 7)                                   # the clock, active, n = 1 + the highest slot in use
    #                                                        type    p              n (W)          c    s    R    g    f    phi   kv              t0   t1
    assert struct.unpack_from("<ii17d", b, 16 + 144) == (1, 0, 0.1, 0.2, 0.3, 5.0, 0.0, 1.0, 3.0, 0.0, 0.0, 0.5, 2.0, 0.25, 0.5, 0.0, 0.25, 0.5, 2.0)
    assert struct.unpack_from("<ii17d", b, 16 + 4 * 144) == (2, 0, 0.1, 0.2, 0.3, 0.0, 1.0, 0.0, 4.0, 6.0, 0.8, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, np.inf)
    assert struct.unpack_from("<ii17d", b, 16 + 6 * 144) == (3, 0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, -400.0, 0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.05, 0.08)
    for i in (0, 2, 3, 5, 7):
        assert not any(b[16 + i * 144:16 + (i + 1) * 144])
    assert struct.unpack_from("<qii", solver.pack_field_state(0, [None] * 8), 0) == (0, 0, 0)


WIND_G = (0, 0, 0, 5, 0, 0, 2.0, 0, 0, 0.5, 2.0, 0.1, 0, 0, 0, 0.0, 1.0)       # p, W, c, s, R, g, f, phi, kv, t0, t1
VORTEX_G = (0, 0, 0, 0, 1, 0, 2.0, 6.0, 0.8, 0, 0, 0, 0, 0, 0, 0.0, float("inf"))
RADIAL_G = (0, 0, 0, 0, 0, 0, 0.0, 400.0, 0.9, 0, 0, 0, 0, 0, 0, 0.05, 0.08)


def _with(g, i, v):
    g = list(g)
    g[i] = v
    return tuple(g)


def test_setters_refuse_bad_arguments():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)
    assert h.pn_sim_fields_set_active(None, 1, None) == PN_ERR_ARG
    assert h.pn_sim_fields_set_active(d, 2, None) == PN_ERR_ARG and h.pn_sim_fields_set_active(d, -1, None) == PN_ERR_ARG
    assert h.pn_sim_fields_clock(None, 0, None) == PN_ERR_ARG and h.pn_sim_fields_clock(d, -1, None) == PN_ERR_ARG

    def field(state=d, index=0, type=1, g=WIND_G):
        a = np.array(g, np.float64) if g is not None else None
        return h.pn_sim_fields_set_field(state, index, type, a.ctypes.data if a is not None else None, None)
    assert field(state=None) == PN_ERR_ARG
    assert field(index=-1) == PN_ERR_ARG and field(index=8) == PN_ERR_ARG                        # an index outside 0..7
    assert field(type=4) == PN_ERR_ARG and field(type=-1) == PN_ERR_ARG                          # an unknown type
    assert field(g=None) == PN_ERR_ARG                                                           # a field needs its geometry
    for t, g in ((1, WIND_G), (2, VORTEX_G), (3, RADIAL_G)):
        for i in range(17):
            for bad in (float("nan"), float("-inf")) + (() if i == 16 else (float("inf"),)):     # only t1 may be +inf
                assert field(type=t, g=_with(g, i, bad)) == PN_ERR_ARG, (t, i, bad)
        assert field(type=t, g=_with(g, 6, -0.5)) == PN_ERR_ARG                                  # c < 0
        assert field(type=t, g=_with(g, 9, -0.1)) == PN_ERR_ARG and field(type=t, g=_with(g, 9, 1.1)) == PN_ERR_ARG   # g outside [0, 1]
        assert field(type=t, g=_with(_with(g, 15, 2.0), 16, 1.0)) == PN_ERR_ARG                  # t1 < t0
    for t, g in ((2, VORTEX_G), (3, RADIAL_G)):
        assert field(type=t, g=_with(g, 8, 0.0)) == PN_ERR_ARG and field(type=t, g=_with(g, 8, -1.0)) == PN_ERR_ARG   # R <= 0
    assert field(type=2, g=_with(VORTEX_G, 4, 2.0)) == PN_ERR_ARG and field(type=2, g=_with(VORTEX_G, 4, 0.0)) == PN_ERR_ARG   # not a unit axis
    assert field(type=2, g=_with(VORTEX_G, 4, 1.0 + 1e-8)) == PN_ERR_ARG
    assert b"argument check failed" in h.pn_last_error()
    out = ctypes.c_void_p(32)

    def rhs(n_k=4, n_IP=3, dt=1e-2, dx=0.1, null=None, rin=d, rout=out):
        p = [d] * 10 + [rin, rout, d]      # state, dof, dof_vel, topo, rho, Nx, kernel_bg, kernel_cnt, buffer, Nx_csr | rhs_in, rhs_out, accel_out
        if null is not None:
            p[null] = None
        return h.pn_sim_fields_rhs(n_k, n_IP, p[0], dt, dx, *p[1:], None)
    for i in range(13):
        assert rhs(null=i) == PN_ERR_ARG, i                                                      # a NULL pointer, whichever
    assert rhs(rout=d) == PN_ERR_ARG                                                             # rhs_out is another buffer than rhs_in
    assert rhs(dt=0.0) == PN_ERR_ARG and rhs(dt=-1.0) == PN_ERR_ARG and rhs(dt=float("nan")) == PN_ERR_ARG
    assert rhs(dx=0.0) == PN_ERR_ARG and rhs(dx=-1.0) == PN_ERR_ARG
    assert rhs(n_k=0) == PN_ERR_ARG and rhs(n_IP=0) == PN_ERR_ARG


# ---------------------------------------------------------------- the Simulator's side
def test_field_state_machine_on_cpu():
    from pienerf_amd.simulator import solver
    s = _cpu_sim()
    assert not s.fields_enabled
    for call in (lambda: s.add_wind((1, 0, 0)), lambda: s.add_air_drag(1.0), lambda: s.add_vortex((0, 0, 0), (0, 1, 0), 1.0, 1.0), lambda: s.add_radial((0, 0, 0), 1.0, 1.0),
                 lambda: s.set_field(0, drag=1.0), lambda: s.remove_field(0), s.clear_fields, s.stop_fields, s.field_state_bytes, s.field_clock, s.reset_field_clock):
        with pytest.raises(RuntimeError, match="enable_fields"):   # setters before enabling
            call()
    assert s.enable_fields() is s and s.fields_enabled and s._field_state is None   # before initialize(): allocated by initialize() on a GPU
    assert s._field_clock_keep() is None
    s._field_clock_restore(None)
    for call in (s.field_clock, s.reset_field_clock, s.field_accel):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    # fields may be described before the cloud arrives: kept here, uploaded with the state
    assert s.add_wind((5.0, 0.0, 0.0)) == 0
    assert s.add_air_drag(1.5) == 1
    assert s.add_vortex((0.1, 0.0, 0.0), (0.0, 3.0, 0.0), 6.0, 0.8) == 2
    assert s.add_radial((0.0, -1.0, 0.0), 400.0, 0.9, start=0.05, stop=0.08) == 3
    want = [solver.field_wind((5.0, 0.0, 0.0)), solver.field_wind((0.0, 0.0, 0.0), drag=1.5), solver.field_vortex((0.1, 0.0, 0.0), (0.0, 1.0, 0.0), 6.0, 0.8),
            solver.field_radial((0.0, -1.0, 0.0), 400.0, 0.9, 0.05, 0.08)] + [None] * 4
    assert s.field_state_bytes() == solver.pack_field_state(1, want)
    assert s.field_types() == [1, 1, 2, 3, 0, 0, 0, 0]
    assert want[0][1][6] == 2.0 and want[2][1][6] == 2.0 and want[0][1][16] == np.inf      # the default drag, the open end
    s.set_field(0, velocity=(0.0, 0.0, 4.0), gust=0.5, hz=2.0)                            # the drag is kept
    s.set_field(2, omega=-3.0, stop=1.0)
    s.set_field(3, strength=-50.0)
    want[0] = solver.field_wind((0.0, 0.0, 4.0), gust=0.5, hz=2.0)
    want[2] = solver.field_vortex((0.1, 0.0, 0.0), (0.0, 1.0, 0.0), -3.0, 0.8, stop=1.0)
    want[3] = solver.field_radial((0.0, -1.0, 0.0), -50.0, 0.9, 0.05, 0.08)
    assert s.field_state_bytes() == solver.pack_field_state(1, want)
    s.remove_field(1)
    assert struct.unpack_from("<qii", s.field_state_bytes(), 0) == (0, 1, 4)               # slot 3 is still in use
    assert s.add_radial((1.0, 0.0, 0.0), 10.0, 0.2) == 1                                   # a freed index is handed out again
    s.stop_fields()
    assert struct.unpack_from("<qii", s.field_state_bytes(k=3), 0) == (3, 0, 4)            # inactive; the fields stay
    s.enable_fields()
    assert struct.unpack_from("<qii", s.field_state_bytes(), 0) == (0, 1, 4)
    s.clear_fields()
    assert s._fields == [None] * 8 and struct.unpack_from("<qii", s.field_state_bytes(), 0) == (0, 1, 0)


def test_every_setter_validates():
    s = _cpu_sim().enable_fields()
    for bad in (dict(velocity=(1, 0)), dict(velocity=(1, float("nan"), 0)), dict(velocity=(1, 0, 0), drag=-0.1), dict(velocity=(1, 0, 0), drag=float("inf")),
                dict(velocity=(1, 0, 0), gust=1.5), dict(velocity=(1, 0, 0), gust=-0.1), dict(velocity=(1, 0, 0), hz=float("nan")), dict(velocity=(1, 0, 0), wave=(0, 1)),
                dict(velocity=(1, 0, 0), origin=(0, float("inf"), 0)), dict(velocity=(1, 0, 0), start=1.0, stop=0.5), dict(velocity=(1, 0, 0), start=float("inf")),
                dict(velocity=(1, 0, 0), stop=float("nan")), dict(velocity=(1, 0, 0), drag="strong")):
        with pytest.raises(ValueError):
            s.add_wind(**bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            s.add_air_drag(bad)
    for bad in (dict(axis=(0, 0, 0)), dict(axis=(0, 1)), dict(radius=0.0), dict(radius=-1.0), dict(omega=float("inf")), dict(drag=-1.0), dict(point=(0, 0))):
        with pytest.raises(ValueError):
            s.add_vortex(**dict(dict(point=(0, 0, 0), axis=(0, 1, 0), omega=1.0, radius=1.0), **bad))
    for bad in (dict(radius=0.0), dict(strength=float("nan")), dict(centre=(0, 0, 0, 0)), dict(start=2.0, stop=1.0)):
        with pytest.raises(ValueError):
            s.add_radial(**dict(dict(centre=(0, 0, 0), strength=1.0, radius=1.0), **bad))
    assert s._fields == [None] * 8                                                        # a refused field takes no slot
    w, q, r = s.add_wind((1, 0, 0)), s.add_vortex((0, 0, 0), (0, 1, 0), 1.0, 1.0), s.add_radial((0, 0, 0), 1.0, 1.0)
    before = s.field_state_bytes()
    # an argument of the wrong kind, a value out of range, an index without a field
    for i, kw in ((w, dict(radius=1.0)), (w, dict(omega=1.0)), (w, dict(centre=(0, 0, 0))), (w, dict(gust=2.0)), (w, dict(drag=-1.0)), (q, dict(velocity=(1, 0, 0))),
                  (q, dict(gust=0.5)), (q, dict(axis=(0, 0, 0))), (q, dict(radius=0.0)), (r, dict(drag=1.0)), (r, dict(point=(0, 0, 0))), (r, dict(radius=-1.0)),
                  (r, dict(stop=-1.0)), (5, dict(start=0.0)), (8, dict(start=0.0)), (-1, dict(start=0.0)), ("wind", dict(start=0.0))):
        with pytest.raises(ValueError):
            s.set_field(i, **kw)
    assert s.field_state_bytes() == before                                                # a refused change changes nothing
    for i in (3, 8, -1):
        with pytest.raises(ValueError):
            s.remove_field(i)
    for _ in range(5):
        s.add_air_drag(0.5)
    for call in (lambda: s.add_wind((1, 0, 0)), lambda: s.add_air_drag(1.0), lambda: s.add_vortex((0, 0, 0), (0, 1, 0), 1.0, 1.0), lambda: s.add_radial((0, 0, 0), 1.0, 1.0)):
        with pytest.raises(ValueError, match="8 field slots"):                            # a ninth field
            call()
    s.remove_field(q)
    assert s.add_radial((0, 0, 0), 2.0, 1.0) == q                                         # ... until one is removed


def test_fields_configured_before_initialize_build_the_tables(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud

    def sim():
        s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                      base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
        s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
        return s
    early = sim().enable_fields()
    early.add_wind((5.0, 0.0, 0.0), gust=0.3, hz=1.0)
    early.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    late = sim()
    late.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert late.Nx_csr is None and not late.fields_enabled
    late.enable_fields()                                                                  # builds contact's tables when they are not there
    late.add_wind((5.0, 0.0, 0.0), gust=0.3, hz=1.0)
    for s in (early, late):
        assert tuple(s.Nx_csr.shape) == (8 * s.n_IP, 10) and not s.contact_enabled
        assert np.array_equal(s.Nx_csr.numpy(), s.IP_Nx.numpy().reshape(-1, 10)[s.buffer.numpy().astype(np.int64)])
    assert early.field_state_bytes() == late.field_state_bytes()
    keep = late.Nx_csr
    late.enable_contact()
    assert late.Nx_csr is keep                                                            # one table serves both stages


def test_the_kernels_order_of_summation_walked_in_numpy(small_opt):
    """csrc/pn_fields.hip's k_field_rhs walked in numpy (fields_reference.kernel_order_walk) over the simulator's own tables on a 4 080-point chair at
    dx 0.05: the longest run (770 entries: four passes of the 256-thread workgroup, a ragged last one), a run shorter than a wave and a run between one
    and four waves equal the np.add.at restatement to round-off."""
    import torch
    from contact_reference import contact_term, ip_state
    from pienerf_amd import scene
    from pienerf_amd.simulator.solver import Simulator
    o = small_opt
    c = scene.make_chair_points(sub_res=45, hgs=o["hash_grid_size"])
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=0.05, stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
    s.initialize = s.precompute
    s.enable_fields()
    s.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    bg, cnt, buf, N = s.kernel_bg.numpy(), s.kernel_cnt.numpy(), s.buffer.numpy(), s.Nx_csr.numpy()
    assert s.n_k == 139 and cnt.max() == 770
    rng = np.random.default_rng(11)
    dof = s.dof.numpy() + rng.normal(scale=0.01, size=s.dof.numel())
    vel = rng.normal(scale=0.5, size=s.dof.numel())
    topo, Nx = s.IP_kernel.numpy(), s.IP_Nx.numpy()
    x, v = ip_state(topo, Nx, dof, vel)
    a = field_accel([wind(**GUSTY), vortex(**SWIRL), radial(**BLAST)], x, v, 0.07, s.dt)
    m = (s.IP_rho * s.dx ** 3).numpy()
    want = contact_term(s.n_k, topo, Nx, m, a).reshape(s.n_k, 30)
    kids = [int(np.argmax(cnt)), int(np.argmin(cnt)), int(np.argmin(np.abs(cnt - 150)))]
    assert cnt[kids[1]] < 64 < cnt[kids[2]] < 256
    for kid in kids:
        got = kernel_order_walk(bg, cnt, buf, N, m, a, kid)
        err = float(np.abs(got - want[kid]).max() / np.abs(want).max())
        print(f"kernel {kid}, run of {cnt[kid]} entries: kernel-order walk vs np.add.at restatement, rel err {err:.2e}")
        assert err < 1e-13   # fp64 sums of at most 770 terms: a few hundred ulps at the very most


# ---------------------------------------------------------------- main_render's arguments
def test_main_render_arguments_become_the_same_calls():
    from pienerf_amd import main_render
    ap = main_render.parser()
    a = ap.parse_args(["--wind", "5", "0", "1", "--wind_drag", "3", "--gust", "0.5", "2", "--gust_wave", "0.5", "0", "0.25", "--air_drag", "1.5",
                       "--vortex", "0.1", "0", "0", "0", "2", "0", "6", "0.8", "--vortex", "0", "0", "0", "1", "0", "0", "-3", "0.5",
                       "--blast", "0", "-1", "0", "400", "0.9", "0.05", "0.08", "--blast", "1", "0", "0", "10", "0.2", "0", "1"])
    assert a.wind == [5.0, 0.0, 1.0] and a.gust == [0.5, 2.0] and len(a.vortex) == 2 and len(a.blast) == 2 and main_render.wants_fields(a)
    s = _cpu_sim()
    assert main_render.configure_fields(s, a) == [0, 1, 2, 3, 4, 5]
    t = _cpu_sim().enable_fields()
    t.add_wind((5.0, 0.0, 1.0), drag=3.0, gust=0.5, hz=2.0, wave=(0.5, 0.0, 0.25))
    t.add_air_drag(1.5)
    t.add_vortex((0.1, 0.0, 0.0), (0.0, 2.0, 0.0), 6.0, 0.8)
    t.add_vortex((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), -3.0, 0.5)
    t.add_radial((0.0, -1.0, 0.0), 400.0, 0.9, start=0.05, stop=0.08)
    t.add_radial((1.0, 0.0, 0.0), 10.0, 0.2, start=0.0, stop=1.0)
    assert s.field_state_bytes() == t.field_state_bytes()
    # the defaults: drag 2, no gust
    s = _cpu_sim()
    main_render.configure_fields(s, ap.parse_args(["--wind", "5", "0", "0"]))
    t = _cpu_sim().enable_fields()
    t.add_wind((5.0, 0.0, 0.0))
    assert s.field_state_bytes() == t.field_state_bytes() and s._fields[0][1][6] == 2.0 and s._fields[0][1][9] == 0.0
    # nothing asked for: nothing enabled
    s = _cpu_sim()
    d = ap.parse_args([])
    assert main_render.configure_fields(s, d) == [] and not s.fields_enabled and not main_render.wants_fields(d)
    for argv, what in ((["--gust", "0.5", "1"], "belong to --wind"), (["--air_drag", "1", "--wind_drag", "3"], "belong to --wind"), (["--wind", "1", "0", "0", "--gust", "2", "1"], "gust"),
                       (["--air_drag", "-1"], "drag"), (["--vortex", "0", "0", "0", "0", "0", "0", "1", "1"], "axis"), (["--blast", "0", "0", "0", "1", "0", "0", "1"], "radius"),
                       (["--blast", "0", "0", "0", "1", "1", "2", "1"], "stop"), (["--air_drag", "1"] + ["--vortex", "0", "0", "0", "0", "1", "0", "1", "1"] * 8, "8 field slots")):
        with pytest.raises(SystemExit, match="fields: .*" + what):       # a usage error, not a traceback
            main_render.configure_fields(_cpu_sim(), ap.parse_args(argv))
    # they compose with the other scripted inputs
    a = ap.parse_args(["--wind", "5", "0", "0", "--floor", "-0.9", "--force", "300", "100", "-200", "--pin_shake", "0.05", "0", "0", "4", "--save_ply", "--video"])
    assert a.force == [300.0, 100.0, -200.0] and a.pin_shake is not None and a.floor == -0.9 and main_render.wants_fields(a) and main_render.wants_contact(a)
