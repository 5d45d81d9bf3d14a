"""Mesh colliders on the host (pienerf_amd/sdf.py, simulator/contact.py, main_render --collide_mesh): the state's layout, the setters'
refusals, flag parsing, the mesh generators, read_mesh_ply, and the sanity of tests/sdf_reference.py itself.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

import sdf_reference as R
from pienerf_amd import _lib, main_render, scene, sdf
from pienerf_amd._captured import STAGE_NOT_CAPTURED, Captured
from pienerf_amd.sdf import SdfGrid, clean_triangles, mesh_box, mesh_icosphere, mesh_is_closed, mesh_terrain
from pienerf_amd.simulator import contact
from pienerf_amd.simulator.solver import Simulator


def _sphere_grid(n=9, s=0.25, R0=0.6):
    return SdfGrid.from_function(lambda p: np.sqrt((p * p).sum(axis=1)) - R0, (-1.0, -1.0, -1.0), s, (n, n, n))


# ---------------------------------------------------------------- layout
def test_struct_sizes_and_packed_bytes():
    h = _lib.lib()
    assert contact.SDF_SLOTS == 4 and contact.SDF_SLOT_DTYPE.itemsize == 80 and contact.SDF_STATE_DTYPE.itemsize == 328
    assert int(h.pn_sim_sdf_bytes()) == 328 and int(h.pn_sim_contact_bytes()) == 744      # the second state is beside the first, not in it
    from pienerf_amd.build import UNITS
    assert UNITS["pn_sdf.hip"] == ["-ffp-contract=fast"] == UNITS["pn_contact.hip"]
    i32, f64, P, u64 = _lib.i32, _lib.f64, _lib.P, _lib.u64
    assert _lib.SIGNATURES["pn_sdf_build"] == (i32, [P, i32, i32, i32, i32, P, f64, P, P, P])
    assert _lib.SIGNATURES["pn_sim_sdf_bytes"] == (u64, [])
    assert _lib.SIGNATURES["pn_sim_sdf_set_collider"] == (i32, [P, i32, P, i32, i32, i32, P, P])
    base = _lib.SIGNATURES["pn_sim_contact_rhs"][1]
    assert _lib.SIGNATURES["pn_sim_contact_sdf_rhs"] == (i32, base[:3] + [P] + base[3:])     # contact's arguments with the second state behind the first
    g = SdfGrid.from_function(lambda p: p[:, 1], (0.5, -1.0, 2.0), 0.25, (3, 4, 5))
    assert g.shape == (5, 4, 3) and g.res == (3, 4, 5) and np.array_equal(g.hi, [1.0, -0.25, 3.0])
    raw = contact.pack_sdf_state([None, (g, np.array([1.0, 2.0, 3.0]), np.array([0.0, -1.0, 0.5])), None, None])
    assert len(raw) == 328
    st = np.frombuffer(raw, contact.SDF_STATE_DTYPE)[0]
    assert st["n"] == 2 and st["reserved"] == 0 and st["c"][0]["grid"] == 0 and st["c"][0]["nx"] == 0
    c = st["c"][1]
    assert c["grid"] == g.values.data_ptr() and (c["nx"], c["ny"], c["nz"]) == (3, 4, 5)
    assert np.array_equal(c["lo"], [1.5, 1.0, 5.0]) and c["s"] == 0.25 and np.array_equal(c["v"], [0.0, -1.0, 0.5])
    # byte offsets, as the C struct has them
    assert np.frombuffer(raw[8 + 80:8 + 88], "<u8")[0] == g.values.data_ptr() and np.array_equal(np.frombuffer(raw[8 + 80 + 8:8 + 80 + 24], "<i4"), [3, 4, 5, 0])
    assert np.array_equal(np.frombuffer(raw[8 + 80 + 24:8 + 160], "<f8"), [1.5, 1.0, 5.0, 0.25, 0.0, -1.0, 0.5])


# ---------------------------------------------------------------- the setters
def test_setters_refuse_before_enable_contact_a_fifth_collider_and_bad_values():
    s = Simulator(device="cpu", persistent=False)
    g = _sphere_grid()
    for call in (lambda: s.add_mesh_collider(g), lambda: s.set_mesh_collider(0, offset=(0, 0, 0)), lambda: s.remove_mesh_collider(0),
                 lambda: s.mesh_collider_state(), lambda: s.mesh_collider_state_bytes()):
        with pytest.raises(RuntimeError, match=r"Simulator: contact is not enabled \(call enable_contact\(\) first\)"):
            call()
    assert "mesh_colliders" not in s.enabled_stage_names() and s._contact_capture_names() == ()
    s.enable_contact(thickness=0.05)
    assert s.mesh_collider_state() is None and "mesh_colliders" not in s.enabled_stage_names()
    with pytest.raises(ValueError, match="a mesh collider is an SdfGrid"):
        s.add_mesh_collider(g.values)
    for bad in ((0.0, np.nan, 0.0), (np.inf, 0.0, 0.0), (0.0, 0.0)):
        with pytest.raises(ValueError, match="a mesh collider's offset is a finite 3-vector"):
            s.add_mesh_collider(g, offset=bad)
    with pytest.raises(ValueError, match="a collider's velocity is a finite 3-vector"):
        s.add_mesh_collider(g, velocity=(0.0, np.nan, 0.0))
    assert all(c is None for c in s._mesh_colliders)
    ids = [s.add_mesh_collider(g, offset=(0.1 * k, 0.0, 0.0)) for k in range(4)]
    assert ids == [0, 1, 2, 3] and s.enabled_stage_names() == frozenset({"contact", "mesh_colliders"})
    with pytest.raises(ValueError, match="all 4 mesh collider slots are in use"):
        s.add_mesh_collider(g)
    s.remove_mesh_collider(1)
    with pytest.raises(ValueError, match="there is no mesh collider 1"):
        s.set_mesh_collider(1, offset=(0, 0, 0))
    with pytest.raises(ValueError, match="there is no mesh collider 4"):
        s.remove_mesh_collider(4)
    assert s.add_mesh_collider(g, velocity=(0.0, 1.0, 0.0)) == 1      # the freed index is handed out again
    s.set_mesh_collider(2, offset=(0.0, -0.5, 0.0))
    with pytest.raises(ValueError, match="finite 3-vector"):
        s.set_mesh_collider(2, offset=(0.0, np.inf, 0.0))
    st = np.frombuffer(s.mesh_collider_state_bytes(), contact.SDF_STATE_DTYPE)[0]
    assert st["n"] == 4 and np.array_equal(st["c"][2]["lo"], [-1.0, -1.5, -1.0]) and np.array_equal(st["c"][1]["v"], [0.0, 1.0, 0.0])
    assert np.array_equal(st["c"][2]["v"], [0.0, 0.0, 0.0])           # set_mesh_collider kept the velocity
    for i in range(4):
        s.remove_mesh_collider(i)
    assert s.enabled_stage_names() == frozenset({"contact"})
    # the analytic colliders are untouched by all of this, and the six stages are the six
    assert s.collider_types() == [0] * 8 and len(Simulator.STAGES) == 6 and "mesh_colliders" not in [st.name for st in Simulator.STAGES]


def test_grids_refuse_bad_resolutions_and_values():
    for res in ((1, 4, 4), (4, 4, 513), (4, 0, 4), (512, 512, 512 + 1), (4, 4)):
        with pytest.raises(ValueError, match="2 .. 512 nodes per axis"):
            SdfGrid.from_function(lambda p: p[:, 0], (0, 0, 0), 1.0, res)
    with pytest.raises(ValueError, match="2 .. 512 nodes per axis"):
        SdfGrid(torch.zeros((1, 2, 2)), (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="contiguous fp32 tensor"):
        SdfGrid(torch.zeros((2, 2, 2), dtype=torch.float64), (0, 0, 0), 1.0)
    for lo, s in (((0, np.nan, 0), 1.0), ((0, 0, 0), 0.0), ((0, 0, 0), -1.0), ((0, 0, 0), np.inf)):
        with pytest.raises(ValueError, match="finite 3-vector and `spacing` a finite number > 0"):
            SdfGrid(torch.zeros((2, 2, 2)), lo, s)
    with pytest.raises(ValueError, match="not finite"):
        SdfGrid.from_function(lambda p: np.full(len(p), np.nan), (1, 1, 1), 1.0, (2, 2, 2))
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        SdfGrid.from_mesh(*mesh_box(), device="cpu")
    with pytest.raises(ValueError, match="resolution is 6 .. 512"):
        SdfGrid.box_for(mesh_box()[0], resolution=5)
    # the library's own checks, before anything is enqueued (PN_ERR_ARG = 1)
    h, dummy = _lib.lib(), ctypes.c_void_p(16)
    geom = np.array([0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0])
    assert h.pn_sim_sdf_set_collider(dummy, 4, dummy, 4, 4, 4, geom.ctypes.data, None) == 1
    assert h.pn_sim_sdf_set_collider(dummy, -1, dummy, 4, 4, 4, geom.ctypes.data, None) == 1
    assert h.pn_sim_sdf_set_collider(None, 0, dummy, 4, 4, 4, geom.ctypes.data, None) == 1
    for res in ((1, 4, 4), (4, 513, 4), (512, 512, 513)):
        assert h.pn_sim_sdf_set_collider(dummy, 0, dummy, *res, geom.ctypes.data, None) == 1
    for k, bad in ((3, 0.0), (3, -1.0), (0, np.nan), (5, np.inf)):
        g2 = geom.copy()
        g2[k] = bad
        assert h.pn_sim_sdf_set_collider(dummy, 0, dummy, 4, 4, 4, g2.ctypes.data, None) == 1
    assert h.pn_sim_sdf_set_collider(dummy, 0, dummy, 4, 4, 4, None, None) == 1
    lo = np.zeros(3)
    assert h.pn_sdf_build(dummy, 0, 4, 4, 4, lo.ctypes.data, 0.5, dummy, None, None) == 1
    assert h.pn_sdf_build(dummy, 1, 4, 4, 1, lo.ctypes.data, 0.5, dummy, None, None) == 1
    assert h.pn_sdf_build(dummy, 1, 4, 4, 4, lo.ctypes.data, 0.0, dummy, None, None) == 1
    assert h.pn_sdf_build(None, 1, 4, 4, 4, lo.ctypes.data, 0.5, dummy, None, None) == 1
    assert sdf.SDF_MAX_PAIRS == 1 << 38
    assert h.pn_sdf_build(dummy, 2049, 512, 512, 512, lo.ctypes.data, 0.5, dummy, None, None) == 1     # 2^27 nodes x 2049 triangles: over the cap of one launch
    assert h.pn_sdf_build(dummy, (1 << 24) + 1, 4, 4, 4, lo.ctypes.data, 0.5, dummy, None, None) == 1
    assert h.pn_sim_contact_sdf_rhs(1, 1, dummy, None, 0.01, 0.1, *([dummy] * 12), None) == 1          # no second state
    assert h.pn_sim_contact_sdf_rhs(1, 1, dummy, dummy, 0.01, 0.1, *([dummy] * 11), None, None) == 1   # accel_out is required


def test_a_capture_without_the_mesh_launch_is_refused_in_the_stages_words():
    msg = STAGE_NOT_CAPTURED["mesh_colliders"]
    before, now = Captured(frozenset({"drag", "contact"}), None, None, 0), Captured(frozenset({"drag", "contact", "mesh_colliders"}), None, None, 0)
    with pytest.raises(RuntimeError) as e:
        before.check_substep(now, "graph")
    assert str(e.value) == msg.format(what="the step graph", again="capture()") and "captured before add_mesh_collider()" in str(e.value)
    with pytest.raises(RuntimeError, match=r"the pipeline was captured before add_mesh_collider\(\).*: capture_pipelined\(\) again"):
        before.check_substep(now, "pipe")
    now.check_substep(now, "graph")
    now.check_substep(before, "graph")     # captured with, none left now: no error


# ---------------------------------------------------------------- flags
def test_flag_parsing():
    p = main_render.parser()
    a = p.parse_args(["--collide_mesh", "a.ply", "--collide_mesh", "b.ply", "0", "-0.5", "1e-1", "--mesh_collider_res", "32"])
    assert a.collide_mesh == [["a.ply"], ["b.ply", "0", "-0.5", "1e-1"]] and a.mesh_collider_res == 32
    assert main_render.mesh_collider_specs(a) == [("a.ply", (0.0, 0.0, 0.0)), ("b.ply", (0.0, -0.5, 0.1))]
    assert main_render.wants_contact(a) and not main_render.wants_analytic_collider(a)
    main_render.check_overlay_args(a)
    d = p.parse_args([])
    assert d.collide_mesh is None and d.mesh_collider_res is None and main_render.mesh_collider_specs(d) == [] and not main_render.wants_contact(d)
    for argv, words in ((["--collide_mesh", "a.ply", "1", "2"], "1 or 4 values"), (["--collide_mesh", "a.ply", "x", "0", "0"], "must be numbers"),
                        (["--mesh_collider_res", "32"], "needs --collide_mesh"), (["--collide_mesh", "a.ply", "--mesh_collider_res", "5"], "6 .. 512"),
                        (["--collide_mesh", "a.ply"] * 5, "at most 4"),
                        (["--collide_mesh", "a.ply", "--draw_colliders"], "is not drawn")):
        with pytest.raises(SystemExit, match=words):
            main_render.check_overlay_args(p.parse_args(argv))
    main_render.check_overlay_args(p.parse_args(["--collide_mesh", "a.ply", "--floor", "-0.9", "--draw_colliders"]))   # the floor is drawn


# ---------------------------------------------------------------- meshes
def test_generators_make_closed_meshes():
    for name, (v, t), n_t in (("box", mesh_box((0.1, 0.2, 0.3), (0.5, 0.25, 1.0)), 12), ("ico0", mesh_icosphere(0), 20), ("ico2", mesh_icosphere(2, 0.6), 320),
                              ("terrain", mesh_terrain(res=7), 2 * 2 * 36 + 4 * 6 * 2)):
        assert v.dtype == np.float32 and t.dtype == np.int32 and t.shape == (n_t, 3) and t.min() == 0 and t.max() == len(v) - 1, name
        assert mesh_is_closed(t), name
        # consistently oriented: every directed edge appears once, its reverse once
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        assert len({tuple(x) for x in e}) == len(e) and {tuple(x) for x in e} == {tuple(x[::-1]) for x in e}, name
        # outward: the signed volume is positive
        a, b, c = (v[t[:, m]].astype(np.float64) for m in range(3))
        assert (a * np.cross(b, c)).sum() / 6.0 > 0.0, name
        assert clean_triangles(v, t)[1] == 0, name
    assert not mesh_is_closed(mesh_box()[1][:-1])
    v, _ = mesh_icosphere(2, 0.6, (1.0, 0.0, 0.0))
    assert np.abs(np.linalg.norm(v - np.array([1.0, 0.0, 0.0], np.float32), axis=1) - 0.6).max() < 1e-6
    v, t = mesh_box()
    assert abs((v[t[:, 0]] * np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0 - 1.0) < 1e-6     # the unit cube's volume
    with pytest.raises(ValueError, match="above `base`"):
        mesh_terrain(lambda x, z: x * 0.0 - 2.0)


def test_degenerate_triangles_are_dropped_before_upload():
    v, t = mesh_box()
    v = np.concatenate([v, v[:1], [[2.0, 0.0, 0.0], [3.0, 0.0, 0.0], [4.0, 0.0, 0.0]]]).astype(np.float32)
    extra = np.array([[0, 0, 1], [0, 8, 1], [9, 10, 11]], np.int32)     # a repeated index; two corners in one place; three corners on a line
    tri9, dropped = clean_triangles(v, np.concatenate([t, extra]))
    assert dropped == 3 and tri9.shape == (12, 9) and tri9.dtype == np.float32
    assert np.array_equal(tri9, np.concatenate([v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]], axis=1))
    with pytest.raises(ValueError, match="outside 0 .. 7"):
        clean_triangles(v[:8], np.array([[0, 1, 8]]))


def test_read_mesh_ply_round_trip(tmp_path):
    v, t = mesh_icosphere(1, 0.5)
    plain, rich = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    scene.write_mesh_ply(plain, v, t)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    scene.write_mesh_ply(rich, v, t, normals=n, colors=np.full((len(v), 3), 7, np.uint8))
    for path in (plain, rich):
        v2, t2 = scene.read_mesh_ply(path)
        assert v2.dtype == np.float32 and t2.dtype == np.int32 and np.array_equal(v2, v) and np.array_equal(t2, t), path
    assert np.array_equal(scene.read_ply(plain)["x"], v[:, 0])      # read_ply still reads the vertex element
    cloud = str(tmp_path / "cloud.ply")
    scene.write_ply(cloud, dict(pos=v.astype(np.float64)), props=("x", "y", "z"))
    with pytest.raises(ValueError, match="a vertex and a face element"):
        scene.read_mesh_ply(cloud)
    with open(plain, "rb") as f:
        raw = f.read()
    short = str(tmp_path / "short.ply")
    with open(short, "wb") as f:
        f.write(raw[:-5])
    with pytest.raises(ValueError, match="ends before"):
        scene.read_mesh_ply(short)


def test_terrain_tool_and_grid_files(tmp_path, capsys):
    out = sdf.main(["--terrain", str(tmp_path / "t.ply"), "--res", "9", "--size", "1.5"])
    v, t = scene.read_mesh_ply(out)
    assert mesh_is_closed(t) and len(v) == 2 * 81 and "closed: True" in capsys.readouterr().out
    assert np.isclose(v[:, 0].max() - v[:, 0].min(), 1.5) and v[:, 1].min() == -1.0
    g = _sphere_grid()
    g.save(str(tmp_path / "g.npz"))
    g2 = SdfGrid.load(str(tmp_path / "g.npz"))
    assert torch.equal(g.values, g2.values) and np.array_equal(g.lo, g2.lo) and g.spacing == g2.spacing and g2.values.dtype == torch.float32
    # from_function rounds the fp64 samples once
    q = g.node_positions().reshape(-1, 3)
    assert np.array_equal(g.values.numpy().reshape(-1), (np.sqrt((q * q).sum(axis=1)) - 0.6).astype(np.float32))
    # box_for: the bounds plus two voxels by default, `resolution` nodes along the longest axis
    lo, s, res = SdfGrid.box_for(mesh_box((0, 0, 0), (0.5, 0.25, 0.125))[0], resolution=24)
    assert res[0] == 24 and np.isclose(s, 1.0 / 19) and np.allclose(lo, [-0.5 - 2 * s, -0.25 - 2 * s, -0.125 - 2 * s])
    assert all(lo[a] + s * (res[a] - 1) >= h + 2 * s - 1e-9 for a, h in enumerate((0.5, 0.25, 0.125)))
    lo, s, res = SdfGrid.box_for(mesh_box()[0], spacing=0.125, margin=0.25)
    assert s == 0.125 and np.array_equal(lo, [-0.75] * 3) and res == (13, 13, 13)


# ---------------------------------------------------------------- the reference's own sanity
def test_reference_box_grid_is_the_analytic_box_distance():
    c, h = (0.05, -0.1, 0.0), (0.5, 0.375, 0.25)
    tri9, _ = clean_triangles(*mesh_box(c, h))
    lo, s, res = (-0.8, -0.8, -0.8), 0.107, (16, 14, 12)
    phi, w, dist = R.build(tri9, lo, s, res)
    q = R.node_positions(lo, s, res).reshape(-1, 3)
    c32, h32 = np.float32(c).astype(np.float64), np.float32(h).astype(np.float64)
    want = R.box_distance(q, c32, h32)     # the corners are fp32
    # the mesh's corners are fp32(c +- h), not c32 +- h32: one fp32 rounding of slack
    assert np.abs(phi.reshape(-1) - want).max() < 2e-7
    assert (phi < 0).sum() > 50 and (phi > 0).sum() > 1000 and np.array_equal(phi < 0, want.reshape(phi.shape) < 0)
    assert np.abs(np.abs(w) - np.round(np.abs(w))).max() < 1e-12 and set(np.round(w.reshape(-1)).astype(int)) == {0, 1}
    # the flipped orientation: w = -1 inside, the same grid
    v, t = mesh_box(c, h)
    phi2, w2, _ = R.build(clean_triangles(v, t[:, ::-1])[0], lo, s, res)
    assert np.array_equal(phi2, phi) and set(np.round(w2.reshape(-1)).astype(int)) == {0, -1}


def test_reference_trilinear_rule_reproduces_a_linear_field_exactly():
    nx, ny, nz = 5, 4, 6
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    V = (3.0 * i - 2.0 * j + 5.0 * k + 7.0).astype(np.float32)
    lo, s = np.array([-1.0, 0.5, 2.0]), 0.25
    rng = np.random.default_rng(5)
    u = rng.integers(0, 64, size=(200, 3)) / 64.0 * (np.array([nx, ny, nz]) - 1.0)      # dyadic coordinates: every step of the rule is exact
    u = u[(u < np.array([nx, ny, nz]) - 1.0).all(axis=1)]
    x = lo + s * u
    ok, d, g = R.sample(V, lo, s, x)
    assert ok.all() and len(x) > 150
    assert np.array_equal(d, 3.0 * u[:, 0] - 2.0 * u[:, 1] + 5.0 * u[:, 2] + 7.0)
    assert np.array_equal(g, np.broadcast_to([3.0, -2.0, 5.0], g.shape))
    # outside [0, n - 1) on any axis, or not finite: nothing
    out = np.array([[-1.0 - 1e-9, 0.6, 2.1], [0.0, 0.5 + 0.25 * 3, 2.1], [-0.9, 0.6, 2.0 + 0.25 * 5], [np.nan, 0.6, 2.1], [np.inf, 0.6, 2.1]])
    ok, d, g = R.sample(V, lo, s, out)
    assert not ok.any() and not d.any() and not g.any()
    ok, _, _ = R.sample(V, lo, s, np.array([[-1.0, 0.5, 2.0]]))      # the first node itself is inside
    assert ok.all()
    # the contact term of a grid whose field is a plane's is the plane's
    from contact_reference import contact_accel, plane
    floor = SdfGrid.from_function(lambda p: p[:, 1] + 0.8125, (-1.0, -1.0, -1.0), 0.125, (17, 17, 17))
    pts = rng.uniform(-0.95, 0.95, size=(300, 3))
    pts[:, 1] = rng.uniform(-0.9, -0.7, size=300)
    vel = rng.normal(size=(300, 3))
    par = (0.01, 0.5, 0.5, 0.5, 0.05)
    a_grid, hit_grid = R.sdf_accel([R.mesh_collider(floor.values.numpy(), floor.lo, floor.spacing)], pts, vel, *par)
    a_plane, hit_plane = contact_accel([plane((0.0, -0.8125, 0.0), (0.0, 1.0, 0.0))], pts, vel, *par)
    assert hit_plane.sum() > 50 and np.array_equal(hit_grid, hit_plane) and np.abs(a_grid - a_plane).max() <= 1e-12 * np.abs(a_plane).max()
