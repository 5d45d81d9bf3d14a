"""Contact with planes and spheres, host side, on CPU (no kernel is launched): the law's properties on its numpy restatement (tests/contact_reference.py),
the restatement against physics on the CPU oracle (the scenes of DESIGN.md 4.10, with wide bars), the C ABI and its argument checks, the packed state
against the header's layout, the Simulator's setters and main_render's arguments."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, make_oracle_sim
from contact_reference import OracleContact, contact_accel, contact_parts, distance_normal, plane, sphere

CONTACT_SYMBOLS = ("pn_sim_contact_bytes", "pn_sim_contact_set_params", "pn_sim_contact_set_collider", "pn_sim_contact_rhs")
PN_ERR_ARG = 1
DT, H = 1e-2, 0.05


# ---------------------------------------------------------------- the law's properties
def _cloud(n=4000, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(n, 3)), rng.normal(scale=2.0, size=(n, 3))


COLLIDERS = {"plane": plane((0.1, -0.3, 0.0), (0.2, 1.0, -0.1), (0.0, 0.5, 0.0)), "sphere": sphere((0.0, 0.0, 0.4), 0.6, velocity=(0.3, 0.0, 0.0)),
             "container": sphere((0.1, 0.0, 0.0), 0.9, inside=True)}


@pytest.mark.parametrize("kind", list(COLLIDERS))
@pytest.mark.parametrize("par", [(0.5, 0.5, 0.5), (1.0, 1.0, 2.0), (1.0, 0.0, 0.0), (0.1, 1.0, 0.3)])
def test_law_bounds(kind, par):
    kappa, beta, mu = par
    x, v = _cloud()
    col = COLLIDERS[kind]
    delta, an, at, nh, wt = contact_parts(col, x, v, DT, kappa, beta, mu, H)
    a, hit = contact_accel([col], x, v, DT, kappa, beta, mu, H)
    out = delta == 0.0
    assert 100 < out.sum() < len(x) - 100                                   # both sides of the threshold are populated
    assert np.array_equal(hit, ~out)
    assert not a[out].any() and not an[out].any() and not at[out].any()     # delta = 0: exact zeros
    assert (an >= 0.0).all() and (an[~out] > 0.0).all()
    assert (DT * DT * an <= (kappa + beta) * delta * (1 + 1e-15)).all()     # no step pushes a point further out than it was in
    L = np.sqrt((wt * wt).sum(axis=1))
    assert (at <= np.minimum(mu * an, L / DT) * (1 + 1e-15)).all()
    assert np.allclose(np.sqrt((nh * nh).sum(axis=1)), 1.0, rtol=0, atol=1e-14)
    # the normal part of a is a_n, the tangential part has length a_t and opposes w_t
    a_n = (a * nh).sum(axis=1)
    a_t = a - a_n[:, None] * nh
    assert np.allclose(a_n, an, rtol=1e-12, atol=1e-9)
    assert np.allclose(np.sqrt((a_t * a_t).sum(axis=1)), at, rtol=1e-9, atol=1e-6 * max(an.max(), 1.0))
    assert ((a_t * wt).sum(axis=1) <= 1e-9 * max(an.max(), 1.0)).all()
    if mu == 0.0:
        assert np.abs(a_t).max() <= 1e-12 * an.max()
    if beta == 0.0:
        assert np.allclose(an, kappa * delta / DT ** 2, rtol=1e-15, atol=0)


def test_normals_point_out_of_the_solid():
    x, _ = _cloud(500)
    d, nh = distance_normal(COLLIDERS["container"], x)
    c = COLLIDERS["container"]["p"]
    assert ((nh * (x - c)).sum(axis=1) < 0.0).all()                          # the container's normal points inward, to its centre
    assert np.allclose(d, 0.9 - np.linalg.norm(x - c, axis=1), rtol=0, atol=1e-15)
    d, nh = distance_normal(COLLIDERS["sphere"], x)
    assert ((nh * (x - COLLIDERS["sphere"]["p"])).sum(axis=1) > 0.0).all()
    d, nh = distance_normal(COLLIDERS["plane"], x)
    assert np.allclose(d, (x - COLLIDERS["plane"]["p"]) @ COLLIDERS["plane"]["n"]) and abs(np.linalg.norm(COLLIDERS["plane"]["n"]) - 1.0) < 1e-15


def test_degenerate_centre():
    c = np.array([[0.2, -0.1, 0.3]])
    d, nh = distance_normal(sphere(c[0], 0.5), c)
    assert d[0] == -0.5 and np.array_equal(nh[0], [0.0, 1.0, 0.0])
    a, hit = contact_accel([sphere(c[0], 0.5)], c, np.zeros((1, 3)), DT, 0.5, 0.5, 0.5, H)
    assert hit[0] and a[0, 0] == 0.0 and a[0, 2] == 0.0 and abs(a[0, 1] - 0.5 * 0.55 / DT ** 2) < 1e-9   # pushed up, finite
    d, nh = distance_normal(sphere(c[0], 0.5, inside=True), c)
    assert d[0] == 0.5 and np.array_equal(nh[0], [-0.0, -1.0, -0.0]) and np.isfinite(nh).all()


def test_continuity_at_the_threshold():
    """The damping term is capped by delta and friction by mu a_n: a point a rounding error inside the threshold gets a force of rounding size, whatever
    its velocity — the device and the restatement cannot disagree by more than that over which side of delta = 0 a point is on."""
    col = plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    v = np.array([[3.0, -50.0, 1.0]])
    for eps in (1e-15, 1e-12, 1e-9):
        y = H - eps
        delta = H - y
        a, hit = contact_accel([col], np.array([[0.0, y, 0.0]]), v, DT, 1.0, 1.0, 2.0, H)
        assert hit[0] and 0.0 < delta < 1.1 * eps
        assert np.abs(a).max() <= (1.0 + 1.0) * delta / DT ** 2 * (1.0 + 2.0) * (1 + 1e-12)   # (kappa + beta) delta / dt^2, times (1 + mu) for friction
    a, hit = contact_accel([col], np.array([[0.0, H, 0.0]]), v, DT, 1.0, 1.0, 2.0, H)
    assert not hit[0] and not a.any()


def test_colliders_add_in_index_order_and_empty_slots_add_nothing():
    x, v = _cloud(600, seed=4)
    cols = list(COLLIDERS.values())
    a_all, _ = contact_accel(cols, x, v, DT, 0.5, 0.5, 0.5, H)
    parts = [contact_accel([c], x, v, DT, 0.5, 0.5, 0.5, H)[0] for c in cols]
    assert np.allclose(a_all, parts[0] + parts[1] + parts[2], rtol=1e-14, atol=1e-9)
    a_gap, _ = contact_accel([cols[0], None, cols[1], None, cols[2]], x, v, DT, 0.5, 0.5, 0.5, H)
    assert np.array_equal(a_gap, a_all)


# ---------------------------------------------------------------- the restatement against physics (oracle only)
def _unpinned(cloud):
    return dict(cloud, pin=np.zeros_like(np.asarray(cloud["pin"])))


def _max_point_disp(o, x0):
    """The largest displacement of an integration point (the points the contact law acts on and counts)."""
    return float(np.linalg.norm(o.ip_positions() - x0, axis=1).max())


def test_dropped_chair_lands_on_the_floor(small_cloud, small_opt):
    o = OracleContact(make_oracle_sim(_unpinned(small_cloud), small_opt), [plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0))])
    assert o.ref.n_IP == 432 and o.ref.n_k == 139 and o.par["h"] == 0.05
    low = []
    for _ in range(100):
        o.step()
        low.append(float(o.ip_positions()[:, 1].min()))
    print(f"dropped chair, floor y = -0.95: lowest integration point {min(low):.3f} over 100 substeps, {low[-1]:.3f} at the end, {o.hits} points in contact")
    assert min(low) > -1.2
    assert o.hits > 0
    free = OracleContact(make_oracle_sim(_unpinned(small_cloud), small_opt), [])
    for _ in range(100):
        free.step()
    y = float(free.ip_positions()[:, 1].min())
    print(f"same without the floor: lowest integration point {y:.2f}")
    assert y < -3.0


def test_friction_holds_the_chair_on_a_tilted_floor(small_cloud, small_opt):
    disp = {}
    for mu in (0.0, 1.0):
        o = OracleContact(make_oracle_sim(_unpinned(small_cloud), small_opt), [plane((0.0, -0.95, 0.0), (0.2, 1.0, 0.0))], mu=mu)
        x0 = o.ip_positions().copy()
        for _ in range(100):
            o.step()
        disp[mu] = _max_point_disp(o, x0)
    print(f"tilted floor, 100 substeps: max point displacement {disp[0.0]:.2f} without friction, {disp[1.0]:.2f} with mu = 1")
    assert disp[1.0] < disp[0.0]


def test_pinned_chair_among_three_colliders_stays_bounded(small_cloud, small_opt):
    cols = [plane((0.0, -0.83, 0.0), (0.0, 1.0, 0.0)), sphere((0.0, 0.0, 0.9), 0.5), sphere((0.0, 0.0, 0.0), 0.98, inside=True)]
    o = OracleContact(make_oracle_sim(small_cloud, small_opt), cols, kappa=1.0, beta=1.0, mu=2.0)
    x0 = o.ip_positions().copy()
    worst, hits = 0.0, []
    for _ in range(60):
        o.step()
        worst = max(worst, _max_point_disp(o, x0))
        hits.append(o.hits)
    print(f"pinned chair, floor + sphere + container at (1, 1, 2): max point displacement {worst:.3f} over 60 substeps, {min(hits)}..{max(hits)} points in contact")
    assert worst < 0.6 and max(hits) > 0


# ---------------------------------------------------------------- the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)


def test_contact_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in CONTACT_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    from pienerf_amd.simulator import solver
    assert _lib.lib().pn_sim_contact_bytes() == solver.CONTACT_STATE_DOUBLES * 8 == solver.CONTACT_STATE_DTYPE.itemsize == 744


def _c_layout(text, name, known):
    """Offsets of a plain C struct's members (int, double, arrays, structs already laid out) under natural alignment: [(member, offset)], size, align."""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(\w+)\s+(\d+)", text)}
    off, align, out = 0, 1, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ty, rest = decl.split(None, 1)
        size, al = {"int": (4, 4), "double": (8, 8)}.get(ty) or known[ty]
        for m in rest.split(","):
            mm = re.match(r"\s*(\w+)\s*(?:\[(\w+)\])?\s*$", m)
            cnt = 1 if mm.group(2) is None else (int(mm.group(2)) if mm.group(2).isdigit() else macros[mm.group(2)])
            off = (off + al - 1) // al * al
            out.append((mm.group(1), off))
            off += size * cnt
            align = max(align, al)
    return out, (off + align - 1) // align * align, align


def test_packed_state_has_the_headers_layout():
    from pienerf_amd.simulator import solver
    text = _header()
    col, col_size, col_al = _c_layout(text, "pn_contact_collider", {})
    st, st_size, _ = _c_layout(text, "pn_contact_state", {"pn_contact_collider": (col_size, col_al)})
    for members, size, dt in ((col, col_size, solver.CONTACT_COLLIDER_DTYPE), (st, st_size, solver.CONTACT_STATE_DTYPE)):
        assert size == dt.itemsize
        assert [(n, o) for n, o in members] == [(n, dt.fields[n][1]) for n in dt.names]
    assert (col_size, st_size) == (88, 744) and solver.CONTACT_SLOTS == 8 and "#define PN_CONTACT_SLOTS 8" in text
    for i, n in enumerate(("PN_CONTACT_EMPTY", "PN_CONTACT_PLANE", "PN_CONTACT_SPHERE", "PN_CONTACT_CONTAINER")):
        assert re.search(n + r"\s*=\s*%d\b" % i, text), n
    assert (solver.CONTACT_EMPTY, solver.CONTACT_PLANE, solver.CONTACT_SPHERE, solver.CONTACT_CONTAINER) == (0, 1, 2, 3)
    # the bytes, read back with struct at the header's offsets
    cols = [None] * 8
    cols[1] = solver.contact_plane((0.0, -0.95, 0.0), (0.0, 2.0, 0.0), (0.0, 0.25, 0.0))
    cols[4] = solver.contact_sphere((0.1, 0.2, 0.3), 0.5, inside=True)
    b = solver.pack_contact_state(1, (0.5, 0.25, 0.75, 0.05), cols)
    assert len(b) == 744
    assert struct.unpack_from("<ii4d", b, 0) == (1, 5, 0.5, 0.25, 0.75, 0.05)                       # active, n = 1 + highest slot in use, kappa, beta, mu, h
    assert struct.unpack_from("<ii10d", b, 40 + 88) == (1, 0, 0.0, -0.95, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.0)   # slot 1: a plane, unit normal
    assert struct.unpack_from("<ii10d", b, 40 + 4 * 88) == (3, 0, 0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0)
    for i in (0, 2, 3, 5, 6, 7):
        assert not any(b[40 + i * 88:40 + (i + 1) * 88])
    assert struct.unpack_from("<ii", solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.0), [None] * 8), 0) == (1, 0)


def test_setters_refuse_bad_arguments():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)

    def params(state=d, active=1, p=(0.5, 0.5, 0.5, 0.05)):
        a = np.array(p, np.float64)
        return h.pn_sim_contact_set_params(state, active, a.ctypes.data, None)
    assert params(state=None) == PN_ERR_ARG
    assert params(active=2) == PN_ERR_ARG and params(active=-2) == PN_ERR_ARG
    for bad in ((0.0, 0.5, 0.5, 0.05), (1.5, 0.5, 0.5, 0.05), (-0.1, 0.5, 0.5, 0.05), (0.5, -0.1, 0.5, 0.05), (0.5, 1.1, 0.5, 0.05), (0.5, 0.5, -1.0, 0.05),
                (0.5, 0.5, 0.5, -0.01), (float("nan"), 0.5, 0.5, 0.05), (0.5, 0.5, float("inf"), 0.05), (0.5, 0.5, 0.5, float("nan"))):
        assert params(p=bad) == PN_ERR_ARG, bad
    assert b"argument check failed" in h.pn_last_error()

    def coll(state=d, index=0, type=1, g=(0, 0, 0, 0, 1, 0, 0, 0, 0, 0)):
        a = np.array(g, np.float64) if g is not None else None
        return h.pn_sim_contact_set_collider(state, index, type, a.ctypes.data if a is not None else None, None)
    assert coll(state=None) == PN_ERR_ARG
    assert coll(index=-1) == PN_ERR_ARG and coll(index=8) == PN_ERR_ARG                         # a ninth collider
    assert coll(type=4) == PN_ERR_ARG and coll(type=-1) == PN_ERR_ARG
    assert coll(g=None) == PN_ERR_ARG                                                           # a collider needs its geometry
    assert coll(g=(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)) == PN_ERR_ARG                                  # zero normal
    assert coll(g=(0, 0, 0, 0, 2, 0, 0, 0, 0, 0)) == PN_ERR_ARG                                  # not a unit normal
    assert coll(type=2, g=(0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)) == PN_ERR_ARG                        # R = 0
    assert coll(type=3, g=(0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0)) == PN_ERR_ARG
    assert coll(g=(float("nan"), 0, 0, 0, 1, 0, 0, 0, 0, 0)) == PN_ERR_ARG
    assert coll(type=2, g=(0, 0, 0, 0, 0, 0, 0.5, 0, float("inf"), 0)) == PN_ERR_ARG
    rhs = lambda n_k=4, n_IP=3, state=d, dt=1e-2, dx=0.1, rin=d, out=ctypes.c_void_p(32): h.pn_sim_contact_rhs(n_k, n_IP, state, dt, dx, d, d, d, d, d, d, d, d, d,
                                                                                                               rin, out, None, None)
    assert rhs(state=None) == PN_ERR_ARG
    assert rhs(n_k=0) == PN_ERR_ARG and rhs(n_IP=0) == PN_ERR_ARG
    assert rhs(dt=float("nan")) == PN_ERR_ARG and rhs(dt=0.0) == PN_ERR_ARG and rhs(dx=-1.0) == PN_ERR_ARG
    assert rhs(out=None) == PN_ERR_ARG and rhs(rin=None) == PN_ERR_ARG
    assert rhs(out=d) == PN_ERR_ARG                                                             # rhs_out is another buffer than rhs_in


def test_the_shared_sum_is_in_library_header_and_signatures_and_refuses_bad_arguments():
    """pn_sim_accel_rhs: the per-kernel sum of contact, fields and self-contact on its own (csrc/pn_sim_rhs.h; tests/test_gpu_rhs_term.py runs it)."""
    from pienerf_amd import _lib
    n = "pn_sim_accel_rhs"
    assert re.search(r"\b" + n + r"\s*\(", _header()) and hasattr(ctypes.CDLL(_lib.LIB_PATH), n)
    i32, f64, P = _lib.SIGNATURES["pn_sim_contact_rhs"][1][0], _lib.SIGNATURES["pn_sim_contact_rhs"][1][3], _lib.SIGNATURES["pn_sim_contact_rhs"][1][2]
    assert _lib.SIGNATURES[n] == (i32, [i32, i32, f64] + [P] * 9)
    h, d, out = _lib.lib(), ctypes.c_void_p(16), ctypes.c_void_p(32)

    def rhs(n_k=4, n_IP=3, dx=0.1, null=None, rin=d, rout=out):
        p = [d] * 6 + [rin, rout]          # rho, kernel_bg, kernel_cnt, buffer, Nx_csr, accel | rhs_in, rhs_out
        if null is not None:
            p[null] = None
        return h.pn_sim_accel_rhs(n_k, n_IP, dx, *p, None)
    for i in range(8):
        assert rhs(null=i) == PN_ERR_ARG, i                                                      # a NULL pointer, whichever
    assert rhs(rout=d) == PN_ERR_ARG                                                             # rhs_out is another buffer than rhs_in
    assert rhs(dx=0.0) == PN_ERR_ARG and rhs(dx=-1.0) == PN_ERR_ARG and rhs(dx=float("nan")) == PN_ERR_ARG and rhs(dx=float("inf")) == PN_ERR_ARG
    assert rhs(n_k=0) == PN_ERR_ARG and rhs(n_IP=0) == PN_ERR_ARG and rhs(n_IP=(1 << 27) + 1) == PN_ERR_ARG
    assert b"argument check failed" in h.pn_last_error()


# ---------------------------------------------------------------- the Simulator's side
def _cpu_sim(dx=0.1):
    from pienerf_amd.simulator.solver import Simulator
    return Simulator(device="cpu", persistent=False, dx=dx)


def test_contact_state_machine_on_cpu():
    from pienerf_amd.simulator import solver
    s = _cpu_sim()
    assert not s.contact_enabled
    for call in (lambda: s.add_plane((0, 0, 0), (0, 1, 0)), lambda: s.add_sphere((0, 0, 0), 1.0), lambda: s.set_collider(0, radius=1.0), lambda: s.remove_collider(0),
                 s.clear_colliders, lambda: s.set_contact_params(stiffness=1.0), s.contact_accel, s.contact_count):
        with pytest.raises(RuntimeError, match="enable_contact"):   # setters before enabling
            call()
    assert s.enable_contact() is s and s.contact_enabled and s._contact_state is None   # before initialize(): allocated by initialize() on a GPU
    assert np.array_equal(s._contact_params, [0.5, 0.5, 0.5, 0.05])                      # the defaults, thickness dx / 2
    for call in (s.contact_accel, s.contact_count):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    # colliders may be described before the cloud arrives: kept here, uploaded with the state
    assert s.add_plane((0.0, -0.95, 0.0), (0.0, 3.0, 0.0)) == 0
    assert s.add_sphere((0.0, 0.0, 0.9), 0.5) == 1
    assert s.add_sphere((0.0, 0.0, 0.0), 0.98, inside=True, velocity=(0.0, 0.1, 0.0)) == 2
    want = [solver.contact_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0)), solver.contact_sphere((0.0, 0.0, 0.9), 0.5),
            solver.contact_sphere((0.0, 0.0, 0.0), 0.98, True, (0.0, 0.1, 0.0))] + [None] * 5
    assert s.contact_state_bytes() == solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.05), want)
    s.set_collider(0, point=(0.0, -0.9, 0.0), velocity=(0.0, 5.0, 0.0))                  # the normal is kept
    s.set_collider(1, radius=0.6)
    s.set_collider(2, inside=False)
    want[0] = solver.contact_plane((0.0, -0.9, 0.0), (0.0, 1.0, 0.0), (0.0, 5.0, 0.0))
    want[1] = solver.contact_sphere((0.0, 0.0, 0.9), 0.6)
    want[2] = solver.contact_sphere((0.0, 0.0, 0.0), 0.98, False, (0.0, 0.1, 0.0))
    assert s.contact_state_bytes() == solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.05), want)
    s.remove_collider(1)
    assert struct.unpack_from("<ii", s.contact_state_bytes(), 0) == (1, 3)               # slot 2 is still in use
    assert s.add_sphere((1.0, 0.0, 0.0), 0.2) == 1                                       # a freed index is handed out again
    s.set_contact_params(friction=2.0)
    s.set_contact_params(stiffness=1.0, damping=0.0, thickness=0.0)
    assert np.array_equal(s._contact_params, [1.0, 0.0, 2.0, 0.0])
    s.enable_contact(stiffness=0.25)                                                     # again: new parameters, the colliders stay
    assert np.array_equal(s._contact_params, [0.25, 0.5, 0.5, 0.05]) and s._colliders[0] is not None
    s.clear_colliders()
    assert s._colliders == [None] * 8 and struct.unpack_from("<ii", s.contact_state_bytes(), 0) == (1, 0)


def test_every_setter_validates():
    s = _cpu_sim()
    for kw in (dict(stiffness=0.0), dict(stiffness=1.01), dict(stiffness=-1.0), dict(damping=-0.1), dict(damping=1.5), dict(friction=-0.5), dict(thickness=-0.1),
               dict(stiffness=float("nan")), dict(friction=float("inf")), dict(thickness=float("nan"))):
        with pytest.raises(ValueError):
            _cpu_sim().enable_contact(**kw)
    assert not s.contact_enabled
    s.enable_contact(stiffness=1.0, damping=1.0, friction=2.0, thickness=0.0)            # the ends of the ranges are allowed
    for kw in (dict(stiffness=0.0), dict(stiffness=2.0), dict(damping=-1e-9), dict(damping=1.0 + 1e-9), dict(friction=-1.0), dict(thickness=-1.0),
               dict(damping=float("nan"))):
        with pytest.raises(ValueError):
            s.set_contact_params(**kw)
    assert np.array_equal(s._contact_params, [1.0, 1.0, 2.0, 0.0])                       # a refused change changes nothing
    for bad in (dict(point=(0, 0, 0), normal=(0, 0, 0)), dict(point=(0, 0), normal=(0, 1, 0)), dict(point=(0, 0, 0), normal=(0, float("nan"), 0)),
                dict(point=(0, 0, 0), normal=(0, 1, 0), velocity=(0, float("inf"), 0)), dict(point=(0, 0, 0), normal=(0, 1, 0), velocity=(0, 1))):
        with pytest.raises(ValueError):
            s.add_plane(**bad)
    for bad in (dict(centre=(0, 0, 0), radius=0.0), dict(centre=(0, 0, 0), radius=-1.0), dict(centre=(0, 0, 0), radius=float("nan")),
                dict(centre=(0, float("inf"), 0), radius=1.0), dict(centre=(0, 0, 0, 0), radius=1.0)):
        with pytest.raises(ValueError):
            s.add_sphere(**bad)
    assert s._colliders == [None] * 8
    p, q = s.add_plane((0, 0, 0), (0, 1, 0)), s.add_sphere((0, 0, 0), 1.0)
    for i, kw in ((p, dict(normal=(0, 0, 0))), (p, dict(radius=1.0)), (p, dict(centre=(0, 0, 0))), (p, dict(inside=True)), (q, dict(radius=0.0)),
                  (q, dict(point=(0, 0, 0))), (q, dict(normal=(0, 1, 0))), (5, dict(velocity=(0, 0, 0))), (8, dict(velocity=(0, 0, 0))), (-1, dict(velocity=(0, 0, 0)))):
        with pytest.raises(ValueError):
            s.set_collider(i, **kw)
    for i in (2, 8, -1):
        with pytest.raises(ValueError):
            s.remove_collider(i)
    for _ in range(6):
        s.add_sphere((0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="8 collider slots"):                            # a ninth collider
        s.add_plane((0, 0, 0), (0, 1, 0))
    with pytest.raises(ValueError, match="8 collider slots"):
        s.add_sphere((0, 0, 0), 1.0)


def test_contact_tables_belong_to_the_layout(small_cloud, small_opt):
    import torch
    from pienerf_amd.simulator.solver import Simulator
    o, c = small_opt, small_cloud

    def sim():
        s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                      base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
        s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
        return s
    plain = sim()
    plain.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert plain.Nx_csr is None                      # built only with the feature on
    plain.enable_contact()
    early = sim().enable_contact()
    early.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    for s in (plain, early):
        buf = s.buffer.numpy().astype(np.int64)
        assert tuple(s.Nx_csr.shape) == (8 * s.n_IP, 10)
        assert np.array_equal(s.Nx_csr.numpy(), s.IP_Nx.numpy().reshape(-1, 10)[buf])       # entry = point 8 + slot
        assert s._contact_params[3] == 0.5 * o["sim_dx"]
    # the runs the kernel walks: every (point, slot) pair once, ascending inside a kernel's run, slot 0 of every point exactly once
    bg, cnt = plain.kernel_bg.numpy(), plain.kernel_cnt.numpy()
    assert cnt.sum() == 8 * plain.n_IP and np.array_equal(np.sort(buf), np.arange(8 * plain.n_IP))
    topo = plain.IP_kernel.numpy()
    for k in range(plain.n_k):
        run = buf[bg[k]:bg[k] + cnt[k]]
        assert (np.diff(run) > 0).all() and (topo[run >> 3, run & 7] == k).all()


def test_the_kernels_order_of_summation_walked_in_numpy(small_opt):
    """csrc/pn_contact.hip's k_contact_rhs walked in numpy over the simulator's own tables (kernel_bg / kernel_cnt / buffer / Nx_csr): 256 threads striding
    each kernel's run in ascending order, the shuffle tree 32, 16 ... 1 inside each of the four waves, the waves added as ((w0 + w1) + w2) + w3.  On a
    4 080-point chair at dx 0.05 (runs of up to 770 entries, ragged last passes) it equals the np.add.at restatement to round-off: the tables and the
    order are the term."""
    import torch
    from contact_reference import contact_term, ip_state
    from pienerf_amd import scene
    from pienerf_amd.simulator.solver import Simulator
    o = small_opt
    c = scene.make_chair_points(sub_res=45, hgs=o["hash_grid_size"])
    s = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=0.05, stiff=o["sim_stiff"],
                  base=torch.tensor([-o["bound"]] * 3), device="cpu", persistent=False)
    s.initialize = s.precompute
    s.enable_contact()
    s.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    bg, cnt, buf, N = s.kernel_bg.numpy(), s.kernel_cnt.numpy(), s.buffer.numpy(), s.Nx_csr.numpy()
    assert s.n_k == 139 and cnt.max() == 770 and (cnt < 64).any()
    rng = np.random.default_rng(11)
    dof = s.dof.numpy() + rng.normal(scale=0.01, size=s.dof.numel())
    vel = rng.normal(scale=0.5, size=s.dof.numel())
    topo, Nx = s.IP_kernel.numpy(), s.IP_Nx.numpy()
    x, v = ip_state(topo, Nx, dof, vel)
    cols = [plane((0.0, -0.8, 0.0), (0.2, 1.0, -0.1), (0.0, 0.5, 0.1)), sphere((0.0, 0.0, 0.9), 0.5), sphere((0.0, 0.0, 0.0), 0.98, inside=True)]
    a, hit = contact_accel(cols, x, v, s.dt, 0.5, 0.5, 0.5, 0.025)
    m = (s.IP_rho * s.dx ** 3).numpy()
    assert 100 < hit.sum() < s.n_IP
    out = np.zeros((s.n_k, 30))
    for kid in range(s.n_k):
        lanes = np.zeros((256, 30))
        for e in range(bg[kid], bg[kid] + cnt[kid]):
            p = buf[e] >> 3
            if hit[p]:
                lanes[(e - bg[kid]) % 256] += np.outer(m[p] * N[e], a[p]).reshape(-1)
        w = 32
        waves = lanes.reshape(4, 64, 30).copy()
        while w:
            waves[:, :w] += waves[:, w:2 * w]
            w //= 2
        out[kid] = ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]
    want = contact_term(s.n_k, topo, Nx, m, a)
    err = float(np.abs(out.reshape(-1, 3) - want).max() / np.abs(want).max())
    print(f"kernel-order walk vs np.add.at restatement: rel err {err:.2e}")
    assert err < 1e-13   # fp64 sums of at most 770 terms: a few hundred ulps at the very most


# ---------------------------------------------------------------- main_render's arguments
def test_main_render_arguments_become_the_same_calls():
    from pienerf_amd import main_render
    from pienerf_amd.simulator import solver
    ap = main_render.parser()
    a = ap.parse_args(["--floor", "-0.95", "--collide_sphere", "0", "0", "0.9", "0.5", "--collide_sphere", "0.5", "0", "0", "0.2", "--collide_inside", "0", "0", "0",
                       "0.98", "--contact_stiffness", "1", "--contact_damping", "0.25", "--friction", "2", "--contact_thickness", "0.02", "--unpin"])
    assert a.unpin and a.floor == -0.95 and a.collide_sphere == [[0.0, 0.0, 0.9, 0.5], [0.5, 0.0, 0.0, 0.2]]
    s = _cpu_sim()
    assert main_render.configure_contact(s, a) == [0, 1, 2, 3]
    t = _cpu_sim().enable_contact(stiffness=1.0, damping=0.25, friction=2.0, thickness=0.02)
    t.add_plane((0.0, -0.95, 0.0), (0.0, 1.0, 0.0))
    t.add_sphere((0.0, 0.0, 0.9), 0.5)
    t.add_sphere((0.5, 0.0, 0.0), 0.2)
    t.add_sphere((0.0, 0.0, 0.0), 0.98, inside=True)
    assert s.contact_state_bytes() == t.contact_state_bytes()
    # the defaults: kappa = beta = mu = 0.5, h = dx / 2
    s = _cpu_sim(dx=0.05)
    main_render.configure_contact(s, ap.parse_args(["--floor", "-1"]))
    assert s.contact_state_bytes() == solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.025), [solver.contact_plane((0, -1, 0), (0, 1, 0))] + [None] * 7)
    # nothing asked for: nothing enabled
    s = _cpu_sim()
    d = ap.parse_args([])
    assert main_render.configure_contact(s, d) == [] and not s.contact_enabled and not d.unpin and not main_render.wants_contact(d)
    with pytest.raises(SystemExit, match="need --floor"):
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--friction", "1"]))
    with pytest.raises(SystemExit, match="stiffness"):     # a usage error, not a traceback
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--floor", "0", "--contact_stiffness", "3"]))
    with pytest.raises(SystemExit, match="radius"):
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--collide_sphere", "0", "0", "0", "-1"]))
    # they compose with the other scripted inputs
    a = ap.parse_args(["--floor", "-0.9", "--force", "300", "100", "-200", "--pin_shake", "0.05", "0", "0", "4", "--save_ply", "--save_mesh"])
    assert a.force == [300.0, 100.0, -200.0] and a.pin_shake is not None and a.save_ply and a.save_mesh and main_render.wants_contact(a)
