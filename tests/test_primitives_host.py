"""Box and capsule colliders without a GPU: the numpy law against brute-force geometry, the packed slots and their mirrors, the C setter's checks, the
draw restatement on exact cases, and main_render's flags (tests/primitives_reference.py; include/pienerf_hip.h: pn_contact_collider)."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import colliders_reference as cr
import contact_reference as cref
import primitives_reference as pr

PN_ERR_ARG = 1
F = np.float32


# ---------------------------------------------------------------- 1: the numpy law is the geometry
CASES = [pr.box((0.1, -0.2, 0.3), (0.5, 0.3, 0.4)), pr.box((-0.4, 0.0, 0.1), (0.15, 0.6, 0.35)),
         pr.capsule((-0.3, 0.1, 0.2), (0.4, 0.5, -0.1), 0.25), pr.capsule((0.2, -0.6, 0.0), (0.2, 0.5, 0.0), 0.4)]


@pytest.mark.parametrize("col", CASES, ids=["box", "flat_box", "capsule", "upright_capsule"])
def test_distance_is_the_distance_to_the_surface_and_the_normal_its_gradient(col):
    x = np.random.default_rng(5).uniform(-1.2, 1.2, (3000, 3))
    d, nh = pr.distance_normal(col, x)
    brute, res = pr.brute_distance(col, x)
    # a sample lies within res / sqrt(2) of every surface point, so the nearest sample is at most that much further than the surface (and never nearer)
    err = brute - np.abs(d)
    print(f"{col['kind']}: {int((d < 0).sum())} of {len(x)} points inside; brute - |d| in [{err.min():.2e}, {err.max():.2e}], resolution {res:.2e}")
    assert (d < 0).sum() > 20 and (d > 0).sum() > 1000      # the sample has points on both sides
    assert err.min() > -1e-12 and err.max() < res
    assert np.abs(np.sqrt((nh * nh).sum(axis=1)) - 1.0).max() < 1e-12
    # the gradient by central differences, away from the medial set (where d is not differentiable: the normal changes within the stencil)
    eps = 1e-6
    grad = np.stack([(pr.distance_normal(col, x + eps * e)[0] - pr.distance_normal(col, x - eps * e)[0]) / (2 * eps) for e in np.eye(3)], axis=1)
    smooth = np.ones(len(x), bool)
    for e in np.eye(3):
        for sgn in (-1.0, 1.0):
            smooth &= np.abs(pr.distance_normal(col, x + sgn * 1e-3 * e)[1] - nh).max(axis=1) < 0.05
    print(f"  {int(smooth.sum())} points away from the medial set, max |grad d - nh| {np.abs(grad - nh)[smooth].max():.2e}")
    assert smooth.sum() > 2000 and np.abs(grad - nh)[smooth].max() < 1e-5


def test_the_laws_conventions():
    b = pr.box((0.0, 0.0, 0.0), (0.5, 0.5, 0.5))
    # inside with ties: the lowest axis wins
    d, nh = pr.distance_normal(b, [(0.25, 0.25, 0.25), (0.0, 0.25, 0.25), (-0.25, 0.1, 0.25), (0.1, -0.3, -0.3)])
    assert d.tolist() == [-0.25, -0.25, -0.25, -0.2]
    assert nh.tolist() == [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]]
    # r_i = 0: the sign is +
    d, nh = pr.distance_normal(b, [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0)])
    assert d.tolist() == [-0.5, -0.5] and nh.tolist() == [[1, 0, 0], [1, 0, 0]]
    # on the surface counts as inside: d = 0 along the face's axis; outside: face, edge and corner regions
    d, nh = pr.distance_normal(b, [(0.5, 0.1, 0.0), (0.8, 0.0, 0.0), (0.8, -0.9, 0.0), (-0.8, 0.9, -0.6)])
    assert d[0] == 0.0 and nh[0].tolist() == [1, 0, 0]
    assert np.allclose(d[1:], [0.3, 0.5, np.sqrt(0.09 + 0.16 + 0.01)], rtol=0, atol=1e-15)
    assert nh[1].tolist() == [1, 0, 0] and np.allclose(nh[2], [0.6, -0.8, 0.0]) and (np.sign(nh[3]) == [-1, 1, -1]).all()
    assert pr.regions(b, [(0.8, 0.0, 0.0), (0.8, -0.9, 0.0), (-0.8, 0.9, -0.6), (0.0, 0.25, 0.25)]) == ["+00", "+-0", "-+-", "in1"]
    assert len(pr.BOX_REGIONS) == 26 + 3
    # a capsule point on the axis: the fallback normal
    c = pr.capsule((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.25)
    d, nh = pr.distance_normal(c, [(0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)])
    assert d.tolist() == [-0.25] * 3 and nh.tolist() == [[0, 1, 0]] * 3
    assert pr.regions(c, [(-0.5, 0.1, 0.0), (0.5, 0.1, 0.0), (1.5, 0.1, 0.0)]) == ["A", "body", "B"]


def test_a_capsule_point_clamped_to_its_first_end_takes_the_sphere_law_bit_for_bit():
    rng = np.random.default_rng(9)
    A, n, R, vel = np.array([0.1, -0.2, 0.3]), np.array([0.7, 0.2, -0.4]), 0.45, (0.3, -0.1, 0.2)
    x = A - 0.2 * n[None] / np.linalg.norm(n) + rng.normal(scale=0.25, size=(2000, 3))
    x = x[(x - A) @ n <= 0.0]
    v = rng.normal(size=x.shape)
    cap, sph = pr.capsule(A, A + n, R, vel), cref.sphere(A, R, velocity=vel)
    assert len(x) > 1000 and (pr.capsule_s(cap, x) == 0.0).all()
    a1, h1 = pr.contact_accel([cap], x, v, 1e-2, 0.5, 0.5, 0.5, 0.05)
    a2, h2 = cref.contact_accel([sph], x, v, 1e-2, 0.5, 0.5, 0.5, 0.05)
    assert 100 < h1.sum() < len(x) and np.array_equal(h1, h2) and np.array_equal(a1.view(np.uint64), a2.view(np.uint64))
    # old kinds pass through unchanged
    three = [cref.plane((0, -0.2, 0), (0.2, 1, -0.1)), cref.sphere((0, 0, 0), 0.5), cref.sphere((0, 0, 0), 0.6, inside=True)]
    b1, b2 = pr.contact_accel(three, x, v, 1e-2, 0.5, 0.5, 0.5, 0.05)[0], cref.contact_accel(three, x, v, 1e-2, 0.5, 0.5, 0.5, 0.05)[0]
    assert np.array_equal(b1.view(np.uint64), b2.view(np.uint64))


# ---------------------------------------------------------------- 2: packing and mirrors
def _cpu_sim(dx=0.1):
    from pienerf_amd.simulator.solver import Simulator
    return Simulator(device="cpu", persistent=False, dx=dx)


def test_packing_and_mirrors():
    from pienerf_amd.simulator import solver
    assert (solver.CONTACT_BOX, solver.CONTACT_CAPSULE) == (4, 5) == (pr.BOX, pr.CAPSULE)
    cols = [None] * 8
    cols[2] = solver.contact_box((0.1, 0.2, 0.3), (0.5, 0.25, 0.125), (0.0, 1.0, 0.0))
    cols[6] = solver.contact_capsule((0.0, -1.0, 0.5), (1.0, 1.0, 0.0), 0.75)
    b = solver.pack_contact_state(1, (0.5, 0.25, 0.75, 0.05), cols)
    assert len(b) == 744 and struct.unpack_from("<ii", b, 0) == (1, 7)                                 # n counts them
    assert struct.unpack_from("<ii10d", b, 40 + 2 * 88) == (4, 0, 0.1, 0.2, 0.3, 0.5, 0.25, 0.125, 0.0, 0.0, 1.0, 0.0)
    assert struct.unpack_from("<ii10d", b, 40 + 6 * 88) == (5, 0, 0.0, -1.0, 0.5, 1.0, 2.0, -0.5, 0.75, 0.0, 0.0, 0.0)   # p = A, n = B - A
    for t, g in (pr.slot_of(pr.box((0.1, 0.2, 0.3), (0.5, 0.25, 0.125), (0.0, 1.0, 0.0))), pr.slot_of(pr.capsule((0.0, -1.0, 0.5), (1.0, 1.0, 0.0), 0.75))):
        assert any(t == c[0] and np.array_equal(g, c[1]) for c in cols if c is not None)
    for bad in ((0.5, 0.0, 0.5), (0.5, -0.1, 0.5), (0.5, float("nan"), 0.5), (0.5, float("inf"), 0.5), (0.5, 0.5)):
        with pytest.raises(ValueError):
            solver.contact_box((0, 0, 0), bad)
    with pytest.raises(ValueError):
        solver.contact_box((0, float("nan"), 0), (1, 1, 1))
    for a, bb, R in (((0, 0, 0), (0, 0, 0), 0.5), ((0, 0, 0), (1, 0, 0), 0.0), ((0, 0, 0), (1, 0, 0), -1.0), ((0, 0, 0), (1, 0, 0), float("nan")),
                     ((0, 0, 0), (float("inf"), 0, 0), 0.5)):
        with pytest.raises(ValueError):
            solver.contact_capsule(a, bb, R)
    # the Simulator's mirror
    s = _cpu_sim().enable_contact()
    i = s.add_box((0.0, -1.0, 0.0), (1.0, 0.1, 1.0))
    j = s.add_capsule((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.2, velocity=(1.0, 0.0, 0.0))
    assert (i, j) == (0, 1) and s.collider_types() == [4, 5, 0, 0, 0, 0, 0, 0]
    want = [solver.contact_box((0.0, -1.0, 0.0), (1.0, 0.1, 1.0)), solver.contact_capsule((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.2, (1.0, 0.0, 0.0))] + [None] * 6
    assert s.contact_state_bytes() == solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.05), want)
    s.set_collider(i, half_extents=(2.0, 0.2, 2.0), centre=(0.0, -1.5, 0.0))
    s.set_collider(j, b=(0.0, 2.0, 0.0), radius=0.3)
    want = [solver.contact_box((0.0, -1.5, 0.0), (2.0, 0.2, 2.0)), solver.contact_capsule((0.0, 0.0, 0.0), (0.0, 2.0, 0.0), 0.3, (1.0, 0.0, 0.0))] + [None] * 6
    assert s.contact_state_bytes() == solver.pack_contact_state(1, (0.5, 0.5, 0.5, 0.05), want)
    s.set_collider(j, a=(0.0, 1.0, 0.0))              # b stays where it was
    assert np.array_equal(s._colliders[j][1][0:6], [0.0, 1.0, 0.0, 0.0, 1.0, 0.0])
    k = s.add_plane((0, -2, 0), (0, 1, 0))
    m = s.add_sphere((0, 0, 0), 0.5)
    for call in (lambda: s.set_collider(i, radius=1.0), lambda: s.set_collider(i, a=(0, 0, 0)), lambda: s.set_collider(i, normal=(0, 1, 0)),
                 lambda: s.set_collider(i, half_extents=(1.0, 0.0, 1.0)), lambda: s.set_collider(j, half_extents=(1, 1, 1)),
                 lambda: s.set_collider(j, centre=(0, 0, 0)), lambda: s.set_collider(j, b=(0.0, 1.0, 0.0)), lambda: s.set_collider(j, radius=0.0),
                 lambda: s.set_collider(k, half_extents=(1, 1, 1)), lambda: s.set_collider(k, a=(0, 0, 0)), lambda: s.set_collider(m, b=(0, 0, 0)),
                 lambda: s.set_collider(m, half_extents=(1, 1, 1))):
        with pytest.raises(ValueError):
            call()
    # the overlay's constants and default colours
    from pienerf_amd import colliders
    assert (colliders.BOX, colliders.CAPSULE) == (4, 5)
    st = colliders.collider_style(types=s.collider_types())
    assert [round(st.rgb[q][0], 6) for q in range(4)] == [colliders.OTHER_GREY, colliders.OTHER_GREY, colliders.PLANE_GREY, colliders.OTHER_GREY]


# ---------------------------------------------------------------- 3: ABI
def test_header_enum_and_the_setters_checks():
    text = (Path(__file__).resolve().parent.parent / "include" / "pienerf_hip.h").read_text()
    for i, n in ((4, "PN_CONTACT_BOX"), (5, "PN_CONTACT_CAPSULE")):
        assert re.search(n + r"\s*=\s*%d\b" % i, text), n
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(16)
    assert h.pn_sim_contact_bytes() == 744

    def coll(type, g, state=d, index=0):
        a = np.array(g, np.float64)
        return h.pn_sim_contact_set_collider(state, index, type, a.ctypes.data, None)
    nan, inf = float("nan"), float("inf")
    for g in ((0, 0, 0, 0.5, 0.0, 0.5, 0, 0, 0, 0), (0, 0, 0, 0.5, 0.5, -0.1, 0, 0, 0, 0), (0, 0, 0, -1, 0.5, 0.5, 0, 0, 0, 0),    # a half-extent <= 0
              (0, 0, 0, 0.5, 0.5, 0.5, 0.1, 0, 0, 0), (0, 0, 0, 0.5, 0.5, 0.5, -0.1, 0, 0, 0),                                      # R is reserved
              (0, 0, 0, 0.5, nan, 0.5, 0, 0, 0, 0), (inf, 0, 0, 0.5, 0.5, 0.5, 0, 0, 0, 0), (0, 0, 0, 0.5, 0.5, inf, 0, 0, 0, 0),
              (0, 0, 0, 0.5, 0.5, 0.5, 0, 0, nan, 0)):
        assert coll(4, g) == PN_ERR_ARG, g
    for g in ((0, 0, 0, 0, 0, 0, 0.5, 0, 0, 0),                                                    # n = 0
              (0, 0, 0, 1, 0, 0, 0.0, 0, 0, 0), (0, 0, 0, 1, 0, 0, -0.5, 0, 0, 0),               # R <= 0
              (0, 0, 0, nan, 0, 0, 0.5, 0, 0, 0), (0, 0, 0, 1, 0, 0, inf, 0, 0, 0), (0, nan, 0, 1, 0, 0, 0.5, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0.5, inf, 0, 0)):
        assert coll(5, g) == PN_ERR_ARG, g
    good_box, good_cap = (0, 0, 0, 0.5, 0.5, 0.5, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0.5, 0, 0, 0)
    assert coll(6, good_box) == PN_ERR_ARG and coll(-1, good_box) == PN_ERR_ARG and coll(6, good_cap) == PN_ERR_ARG
    assert coll(4, good_box, state=None) == PN_ERR_ARG and coll(5, good_cap, index=8) == PN_ERR_ARG
    assert b"argument check failed" in h.pn_last_error()


# ---------------------------------------------------------------- 4: the draw restatement on exact cases, fp32
def _one(o, d, cols, t_min=pr.T_MIN):
    o, d, z = np.array([o], F), np.array([d], F), np.zeros(1, F)
    return pr.draw(cols, cr.default_rgb(), 0.0, 0.5, 0.3, o, d, t_min, pr.T_MAX, 1.0, z, z, np.zeros((1, 3), F))


def test_draw_restatement_on_exact_cases():
    cols = cr.slots(pr.UNIT_BOX, pr.UNIT_CAPSULE)
    want = {"axial onto a face": (2.0, 0, 2), "from inside: the far face": (1.0, 0, 2), "parallel to a slab, inside it": (1.0, 0, 2),
            "parallel to a slab, outside it": (np.inf, -1, None), "grazing an edge": (np.inf, -1, None),
            "along the capsule's axis onto the cap": (1.5, 1, None), "onto the cylinder's middle": (2.5, 1, None), "eye inside the capsule": (0.5, 1, None)}
    rays = pr.hand_rays()
    assert [r[0] for r in rays] == list(want)
    for name, o, d in rays:
        r = _one(o, d, cols)
        t, k, face = want[name]
        assert (float(r.t[0]), int(r.slot[0])) == (t, k), (name, r.t, r.slot)
        if face is not None:
            assert int(r.face[0]) == face, name
    # the graze is a tie t_enter == t_exit: no hit, and flagged
    p, hx = np.asarray(pr.UNIT_BOX[1][0:3], F), np.asarray(pr.UNIT_BOX[1][3:6], F)
    hit, te, tx, fe, fx, near = pr.box_interval(p, hx, np.array([[2.0, 0.0, 0.0]], F), np.array([[-1.0, 0.0, 1.0]], F))
    assert not hit[0] and te[0] == tx[0] == 1.0 and near[0]
    # a ray into a corner's diagonal: all three entries tie, the lowest axis is the face; leaving through the opposite corner likewise
    cube = cr.slots((pr.BOX, np.array([0, 0, 0, 1.0, 1.0, 1.0, 0, 0, 0, 0.0])))
    hit, te, tx, fe, fx, near = pr.box_interval(np.zeros(3, F), np.ones(3, F), np.array([[3.0, 3.0, 3.0]], F), np.array([[-1.0, -1.0, -1.0]], F))
    assert hit[0] and (te[0], tx[0], fe[0], fx[0]) == (2.0, 4.0, 0, 0) and near[0]
    r = _one((0.0, 0.0, 0.0), (0.0, 2.0, 0.0), cube)        # t is in units of d as given
    assert (float(r.t[0]), int(r.face[0])) == (0.5, 1)
    # the colour: the face's normal shades a head-on hit fully, and the checker runs over the two other axes from the centre
    rgb = cr.default_rgb()
    r = _one((0.25, 0.1, 3.0), (0.0, 0.0, -1.0), cols)
    assert np.array_equal(r.image[0], rgb[0] * F(1) * (F(0.3) + (F(1) - F(0.3)) * F(1)))       # a = 1 at t = 2 of t_max = 12, over an empty frame
    o = np.array([[0.125, 0.125, 3.0], [0.375, 0.125, 3.0], [0.375, 0.375, 3.0], [-0.125, 0.125, 3.0]], F)
    d = np.broadcast_to(np.array([0.0, 0.0, -1.0], F), o.shape).copy()
    z = np.zeros(4, F)
    r = pr.draw(cols, rgb, 0.25, 0.5, 0.0, o, d, pr.T_MIN, pr.T_MAX, 0.0, z, z, np.zeros((4, 3), F))
    assert (r.image[:, 0] / rgb[0, 0]).tolist() == [1.0, 0.5, 1.0, 0.5]
    # the capsule's normal: head-on in the middle and on the cap
    for o, d in (((0.0, 2.0, 3.0), (0.0, 0.0, -1.0)), ((-3.0, 2.0, 0.0), (1.0, 0.0, 0.0))):
        r = _one(o, d, cols)
        assert np.array_equal(r.image[0], rgb[1] * F(1)), (o, r.image)
    # a state of planes, spheres and the container: colliders_reference's bits
    S = cr.STANDARD
    o, d = cr.get_rays_numpy(S["eye"], 64, 48, 0.9 * 64)
    acc, s, d0 = cr.standard_inputs(o.shape[0])
    args = (cr.standard_scene(), rgb, S["checker"], S["checker_dim"], S["ambient"], o, d, S["t_min"], S["t_max"], S["bg"], s, d0, acc)
    a, b = cr.draw(*args), pr.draw(*args)
    for x, y in ((a.image, b.image), (a.coverage, b.coverage), (a.t, b.t)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a.slot, b.slot) and not b.near.any()


@pytest.mark.parametrize("eye", list(pr.EYES))
def test_the_gpu_tests_ray_sets_flag_few_rays(eye):
    """The share of masked rays the GPU comparison allows is met by the reference alone."""
    o, d = cr.get_rays_numpy(pr.EYES[eye], 48, 48, 0.9 * 48)
    acc, s, d0 = cr.standard_inputs(o.shape[0])
    r = pr.draw(pr.mixed_scene(), cr.default_rgb(), 0.25, 0.5, 0.3, o, d, pr.T_MIN, pr.T_MAX, 1.0, s, d0, acc)
    hit = r.slot >= 0
    print(f"{eye}: hits per slot {np.bincount(r.slot[hit], minlength=8).tolist()}, box faces {np.bincount(r.face[r.slot == 3], minlength=3).tolist()}, "
          f"{int(r.near.sum())} rays flagged")
    assert r.near.sum() < 0.01 * hit.sum()
    if eye == "outside":
        assert (np.bincount(r.slot[hit], minlength=8)[[0, 1, 3, 4]] > 40).all() and (np.bincount(r.face[r.slot == 3], minlength=3) > 0).sum() >= 2
    if eye == "inside_box":
        assert (r.slot == 3).all() and (np.bincount(r.face, minlength=3) > 100).all()
    if eye == "inside_capsule":
        assert (r.slot[hit] == 4).sum() > 1000


# ---------------------------------------------------------------- 5: the command line
def test_main_render_flags():
    from pienerf_amd import main_render
    from pienerf_amd.simulator import solver
    ap = main_render.parser()
    a = ap.parse_args(["--collide_capsule", "0", "0", "0", "0", "1", "0", "0.2", "--collide_box", "0", "-1", "0", "1", "0.1", "1", "--floor", "-2",
                       "--collide_box", "1", "0", "0", "0.1", "0.1", "0.1", "--collide_sphere", "0", "0", "0.9", "0.5", "--collide_inside", "0", "0", "0", "3",
                       "--collide_capsule", "1", "0", "0", "1", "1", "0", "0.1", "--ball", "0", "2", "0", "0.2", "1"])
    assert a.collide_box == [[0, -1, 0, 1, 0.1, 1], [1, 0, 0, 0.1, 0.1, 0.1]] and len(a.collide_capsule) == 2 and main_render.wants_contact(a)
    s = _cpu_sim()
    assert main_render.configure_contact(s, a) == list(range(8))
    assert s.collider_types() == [1, 2, 3, 4, 4, 5, 5, 2]          # floor, spheres, container, boxes, capsules, then the balls
    assert np.array_equal(s._colliders[3][1], solver.contact_box((0, -1, 0), (1, 0.1, 1))[1])
    assert np.array_equal(s._colliders[6][1], solver.contact_capsule((1, 0, 0), (1, 1, 0), 0.1)[1])
    # a box alone is something to collide with, to draw and to cast shadows on
    a = ap.parse_args(["--collide_box", "0", "-1", "0", "1", "0.1", "1", "--draw_colliders", "--shadows", "--friction", "1"])
    assert main_render.wants_contact(a)
    s = _cpu_sim()
    assert main_render.configure_contact(s, a) == [0] and s.collider_types()[0] == 4 and s._contact_params[2] == 1.0
    a = ap.parse_args(["--collide_capsule", "0", "0", "0", "0", "1", "0", "0.2", "--draw_colliders"])
    assert main_render.wants_contact(a)
    with pytest.raises(SystemExit, match="need --floor"):
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--friction", "1"]))
    with pytest.raises(SystemExit, match="half-extents"):
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--collide_box", "0", "0", "0", "1", "0", "1"]))
    with pytest.raises(SystemExit, match="radius"):
        main_render.configure_contact(_cpu_sim(), ap.parse_args(["--collide_capsule", "0", "0", "0", "0", "1", "0", "0"]))
    for bad in (["--collide_box", "0", "0", "0", "1", "1"], ["--collide_capsule", "0", "0", "0", "0", "1", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_wrong_argument_counts_exit_with_a_message(capsys):
    from pienerf_amd import main_render
    with pytest.raises(SystemExit):
        main_render.parser().parse_args(["--collide_box", "0", "0", "0", "1", "1"])
    assert "--collide_box" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main_render.parser().parse_args(["--collide_capsule", "0", "0", "0", "0", "1", "0", "0.2", "7"])
    assert capsys.readouterr().err
