"""Marching cubes on CPU (no kernel is launched): the generated case table and its properties, the numpy reference's meshes (closed, oriented,
right topology and volume), the C ABI's argument checks and the PLY writers (tools/gen_mc_table.py, tests/mc_reference.py, csrc/pn_mesh.hip)."""
import ctypes
import os

import numpy as np
import pytest

import mc_reference as R
from conftest import ROOT
from gen_mc_table import CORNERS, EDGES, FACES, HEADER, case_table, header_text

PN_ERR_ARG = 1


def test_committed_header_is_the_generators_output_and_the_library_has_it():
    assert open(HEADER).read() == header_text(), "pienerf_amd/csrc/pn_mc_table.h is stale: python tools/gen_mc_table.py"
    from pienerf_amd import _lib
    count, edges = case_table()
    c = np.zeros(256, np.uint8)
    e = np.zeros((256, 15), np.int8)
    assert _lib.lib().pn_mc_case_table(c.ctypes.data, e.ctypes.data) == 0
    assert np.array_equal(c, count) and np.array_equal(e, edges)
    assert _lib.lib().pn_mc_case_table(None, e.ctypes.data) == PN_ERR_ARG


def _face_edge_ids():
    ids = []
    for corners, _ in FACES:
        fe = []
        for k in range(4):
            a, b = corners[k], corners[(k + 1) % 4]
            fe.append(next(i for i, (p, q) in enumerate(EDGES) if {p, q} == {a, b}))
        ids.append((corners, fe))
    return ids


@pytest.mark.parametrize("ci", range(256))
def test_case_uses_the_crossed_edges_and_cuts_ambiguous_faces_per_corner(ci):
    count, edges = case_table()
    above = [not (ci >> m) & 1 for m in range(8)]
    crossed = {e for e, (p, q) in enumerate(EDGES) if above[p] != above[q]}
    n = int(count[ci])
    assert n <= 5
    assert np.all(edges[ci, 3 * n:] == -1)
    tris = edges[ci, :3 * n].reshape(-1, 3).astype(int)
    assert set(tris.reshape(-1).tolist()) == crossed
    assert all(len(set(t)) == 3 for t in tris.tolist())
    und = {}
    for t in tris.tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            und[frozenset((a, b))] = und.get(frozenset((a, b)), 0) + 1
    faces = _face_edge_ids()
    boundary = {k for k, v in und.items() if v == 1}
    assert all(v in (1, 2) for v in und.values())
    for k in boundary:      # an edge no other triangle of the case shares lies on a cube face
        assert any(k <= set(fe) for _, fe in faces), (ci, tuple(k))
    for corners, fe in faces:
        ups = [above[m] for m in corners]
        if ups[0] == ups[2] and ups[1] == ups[3] and ups[0] != ups[1]:   # ambiguous face: each above corner is cut off on its own
            for k in range(4):
                if ups[k]:
                    assert frozenset((fe[(k - 1) % 4], fe[k])) in boundary, (ci, corners)


def _shell(f, value):
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (value,) * 6
    return f


def _grid(n):
    g = np.arange(n, dtype=np.float64)
    return np.meshgrid(g, g, g, indexing="ij")


def _sphere(n=28, r=9.1, c=(13.3, 13.6, 13.9)):
    X, Y, Z = _grid(n)
    return (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32)


def _closed(v, t):
    assert len(t) > 0 and R.directed_edges_paired(t, len(v)), "a directed edge is not met by its reverse exactly once"
    assert set(np.unique(t).tolist()) == set(range(len(v)))   # every vertex is used


def test_random_shell_field_covers_every_case_and_is_closed():
    rng = np.random.default_rng(7)
    f = _shell(rng.standard_normal((24, 25, 26)).astype(np.float32), -1.0)
    v, t = R.marching_cubes(f, 0.0)
    up = f.astype(np.float64) > 0.0
    case = np.zeros((23, 24, 25), np.int64)
    for m, (di, dj, dk) in enumerate(CORNERS):
        case |= (~up[di:23 + di, dj:24 + dj, dk:25 + dk]).astype(np.int64) << m
    assert len(np.unique(case)) == 256
    _closed(v, t)
    assert R.signed_volume(v, t) > 0


def test_sphere_is_a_closed_outward_sphere_with_the_analytic_volume():
    # the mesh is inscribed in the level set: on a signed distance it loses about 0.7 % of the volume at r = 9.1 cells, 0.3 % at r = 13.7
    r = 13.7
    v, t = R.marching_cubes(_sphere(n=34, r=r, c=(16.3, 16.6, 16.9)), 0.0)
    _closed(v, t)
    assert R.euler_characteristic(v, t) == 2
    vol = R.signed_volume(v, t)
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.005


def test_torus_has_euler_characteristic_zero():
    X, Y, Z = _grid(32)
    f = (3.6 - np.sqrt((np.sqrt((X - 15.7) ** 2 + (Y - 15.4) ** 2) - 9.2) ** 2 + (Z - 15.6) ** 2)).astype(np.float32)
    v, t = R.marching_cubes(f, 0.0)
    _closed(v, t)
    assert R.euler_characteristic(v, t) == 0
    assert R.signed_volume(v, t) > 0


def test_two_balls_have_euler_characteristic_four():
    X, Y, Z = _grid(30)
    f = np.maximum(5.2 - np.sqrt((X - 8.3) ** 2 + (Y - 9.1) ** 2 + (Z - 14.2) ** 2), 4.7 - np.sqrt((X - 20.6) ** 2 + (Y - 19.4) ** 2 + (Z - 15.1) ** 2))
    v, t = R.marching_cubes(f.astype(np.float32), 0.0)
    _closed(v, t)
    assert R.euler_characteristic(v, t) == 4
    assert R.signed_volume(v, t) > 0


def test_integer_field_with_exact_ties_is_closed():
    rng = np.random.default_rng(3)
    f = _shell(rng.integers(-2, 3, (20, 21, 22)).astype(np.float32), -3.0)
    assert np.any(f == 1.0)
    v, t = R.marching_cubes(f, 1.0)          # corners exactly at the threshold are not above
    _closed(v, t)
    assert R.signed_volume(v, t) > 0


def test_reference_crop_with_origin_matches_the_whole_lattice():
    f = np.full((40, 41, 42), -1.0, np.float32)
    f[10:38, 6:34, 12:40] = _sphere(28)
    v, t = R.marching_cubes(f, 0.0)
    vc, tc = R.marching_cubes(f[9:39, 5:35, 11:41], 0.0, origin=(9, 5, 11))
    assert np.array_equal(v, vc) and np.array_equal(t, tc)


# ------------------------------------------------------------------ C ABI argument checks (nothing is enqueued)
def test_mc_entries_refuse_bad_arguments_before_enqueueing():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(256)
    assert h.pn_mc_work_bytes(512, 512, 512) > 0                               # 512^3 is allowed
    assert h.pn_mc_work_bytes(755, 755, 755) > 0 and h.pn_mc_work_bytes(756, 756, 756) == 0     # 5 (n-1)^3 reaches 2^31
    assert h.pn_mc_work_bytes(2, 3, 119304647) > 0 and h.pn_mc_work_bytes(2, 3, 119304648) == 0  # 3 n reaches 2^31
    assert h.pn_mc_work_bytes(1 << 30, 1 << 30, 1 << 30) == 0
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (-2, 4, 4), (756, 756, 756), (2, 3, 119304648), (65536, 65536, 2)):
        assert h.pn_mc_work_bytes(*dims) == 0, dims
        assert h.pn_mc_count(d, *dims, 0.5, d, d, None) == PN_ERR_ARG, dims
        assert h.pn_mc_emit(d, *dims, 0.5, d, d, d, None) == PN_ERR_ARG, dims
    assert h.pn_mc_count(None, 4, 4, 4, 0.5, d, d, None) == PN_ERR_ARG         # no field
    assert h.pn_mc_count(d, 4, 4, 4, 0.5, None, d, None) == PN_ERR_ARG         # no work
    assert h.pn_mc_count(d, 4, 4, 4, 0.5, d, None, None) == PN_ERR_ARG         # no totals
    assert h.pn_mc_emit(None, 4, 4, 4, 0.5, d, d, d, None) == PN_ERR_ARG
    assert h.pn_mc_emit(d, 4, 4, 4, 0.5, d, None, d, None) == PN_ERR_ARG
    assert h.pn_mc_emit(d, 4, 4, 4, 0.5, d, d, None, None) == PN_ERR_ARG


def test_marching_cubes_refuses_a_cpu_field():
    import torch
    from pienerf_amd.mesh import marching_cubes
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros(4, 4, 4), 0.5)


# ------------------------------------------------------------------ PLY writers
def _read_faces(path):
    with open(path, "rb") as f:
        hdr = []
        while True:
            line = f.readline().decode().strip()
            hdr.append(line)
            if line == "end_header":
                break
        nv = int(next(h for h in hdr if h.startswith("element vertex")).split()[2])
        nf = int(next(h for h in hdr if h.startswith("element face")).split()[2])
        f.read(12 * nv)
        rec = np.frombuffer(f.read(), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert len(rec) == nf
    return hdr, rec


@pytest.mark.parametrize("n", [0, 1, 37])
def test_write_mesh_ply_round_trips(tmp_path, n):
    from pienerf_amd import scene
    rng = np.random.default_rng(n)
    v = rng.standard_normal((n + 2 if n else 0, 3))
    t = rng.integers(0, max(len(v), 1), (n, 3)).astype(np.int64)
    p = str(tmp_path / "m.ply")
    scene.write_mesh_ply(p, v, t)
    hdr, rec = _read_faces(p)
    assert hdr == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
                   f"element face {n}", "property list uchar int vertex_indices", "end_header"]
    c = scene.read_ply(p)
    assert np.array_equal(np.stack([c["x"], c["y"], c["z"]], 1), v.astype(np.float32).reshape(-1, 3))
    assert np.all(rec["n"] == 3) and np.array_equal(rec["i"], t)


def test_write_to_ply_writes_the_reference_ascii_layout(tmp_path):
    from pienerf_amd.nerf.utils import write_to_ply
    pts = np.array([[0.1, -2.0, 1e-17], [1.0 / 3.0, 5e20, -0.0], [np.pi, 2.5, 7.0]], np.float64)
    p = str(tmp_path / "p.ply")
    write_to_ply(pts, p)
    want = ["ply", "format ascii 1.0", "element vertex 3", "property float x", "property float y", "property float z", "end_header"]
    want += [" ".join(str(float(x)) for x in row) for row in pts]
    assert open(p).read() == "\n".join(want) + "\n"
    write_to_ply(np.zeros((0, 3)), p)
    assert open(p).read() == "\n".join(want[:2] + ["element vertex 0"] + want[3:7]) + "\n"


def test_mesh_module_does_not_reach_outside_the_package():
    for rel in ("pienerf_amd/mesh.py", "pienerf_amd/csrc/pn_mesh.hip", "pienerf_amd/csrc/pn_mc_table.h"):
        assert "oracle" not in open(os.path.join(ROOT, rel)).read(), rel
