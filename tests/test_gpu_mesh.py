"""Marching cubes on the GPU against the numpy reference (tests/mc_reference.py), bit for bit: lattices of every shape class, ties, NaN / inf,
empty results, both sides of every tile and level boundary of the scan, determinism, stream order, a 512^3 lattice, the chair's density field
through lattice_field / extract_geometry / Trainer.save_mesh / save_point_cloud, and the CLI."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# csrc/pn_mesh.hip: PN_MC_TILE = 256 nodes per tile, PN_MC_SCAN = 256 tile sums per workgroup and scan level, so the scan changes shape at
# 256 nodes (one tile), 256^2 = 65536 nodes (a second level) and 256^3 = 16777216 nodes (a third).
TILE, SCAN = 256, 256


def _gpu(field, thr):
    from pienerf_amd.mesh import marching_cubes
    v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(field, np.float32)).to(DEV), thr)
    return v.cpu().numpy(), t.cpu().numpy()


def _same(got, want):
    (gv, gt), (wv, wt) = got, want
    assert gv.dtype == np.float64 and gt.dtype == np.int32
    assert gv.shape == wv.shape and gt.shape == wt.shape, (gv.shape, wv.shape, gt.shape, wt.shape)
    assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)), "vertices differ (bitwise)"
    assert np.array_equal(gt, wt), "triangles differ"


def _check(field, thr):
    got = _gpu(field, thr)
    _same(got, R.marching_cubes(field, thr))
    return got


def _shell(f, value):
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (value,) * 6
    return f


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 3, 5), (33, 47, 29), (130, 7, 257)])
def test_random_fields_equal_the_reference(dims):
    rng = np.random.default_rng(sum(dims))
    f = rng.standard_normal(dims).astype(np.float32)
    _check(f, 0.0)
    _check(f, 0.7)
    v, t = _check(_shell(f.copy(), -1.0), 0.0)
    if min(dims) > 2:
        assert len(t) > 0 and R.directed_edges_paired(t, len(v))


@pytest.mark.parametrize("dims", [(2, 2, 2), (9, 10, 11), (33, 47, 29)])
def test_ties_equal_the_reference(dims):
    rng = np.random.default_rng(1 + sum(dims))
    f = rng.integers(-2, 3, dims).astype(np.float32)
    _check(f, 0.0)
    _check(f, 1.0)
    v, t = _check(_shell(f.copy(), -3.0), 1.0)
    assert R.directed_edges_paired(t, len(v))


def test_nan_and_inf_corners_follow_the_formula():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((17, 19, 23)).astype(np.float32)
    flat = f.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:300]] = np.nan
    flat[idx[300:600]] = np.inf
    flat[idx[600:900]] = -np.inf
    v, _ = _check(f, 0.0)
    assert np.isnan(v).any()
    _check(f, -1e30)


@pytest.mark.parametrize("value,thr", [(1.0, 0.5), (0.0, 0.5), (0.5, 0.5), (np.nan, 0.0)])
def test_uniform_fields_have_no_surface(value, thr):
    v, t = _check(np.full((5, 6, 7), value, np.float32), thr)
    assert v.shape == (0, 3) and t.shape == (0, 3)


# nodes on both sides of every tile / level boundary (257 and 65537 are prime: the next composite stands in)
BOUNDARY_DIMS = [(3, 5, 17), (4, 8, 8), (2, 3, 43), (15, 17, 257), (16, 64, 64), (2, 3, 10923), (3, 5, 1118481), (256, 256, 256), (97, 257, 673)]


@pytest.mark.parametrize("dims", BOUNDARY_DIMS)
def test_scan_tile_and_level_boundaries(dims):
    n = int(np.prod(dims))
    assert any(abs(n - b) <= 2 for b in (TILE, TILE * SCAN, TILE * SCAN * SCAN))
    rng = np.random.default_rng(n)
    f = np.where(rng.random(dims) < 0.03, 1.0, -1.0).astype(np.float32) * rng.random(dims).astype(np.float32)
    v, t = _check(f, 0.0)
    assert len(t) > 0


def test_repeated_calls_are_byte_identical_and_follow_the_side_stream():
    from pienerf_amd.mesh import marching_cubes
    rng = np.random.default_rng(11)
    src = torch.from_numpy(rng.standard_normal((64, 65, 66)).astype(np.float32)).to(DEV)
    a = marching_cubes(src, 0.1)
    b = marching_cubes(src, 0.1)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big = torch.full((64, 65, 66), -1.0, device=DEV)
        for _ in range(20):                          # a queue of work on the side stream ahead of the field's last write
            big.mul_(1.0000001)
        field = torch.empty_like(src)
        field.copy_(src)                             # produced on s
        c = marching_cubes(field, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int64), c[0].view(torch.int64)) and torch.equal(a[1], c[1])


def test_512_cubed_lattice_with_one_sphere_equals_the_reference_on_a_crop():
    from pienerf_amd.mesh import marching_cubes
    n = 512
    c = torch.tensor([300.3, 211.6, 77.2], dtype=torch.float64)
    g = torch.arange(n, dtype=torch.float64, device=DEV)
    field = torch.empty(n, n, n, dtype=torch.float32, device=DEV)
    for i in range(n):   # slab by slab: the fp64 distance of one 512^3 lattice would need 1 GB at once
        d = ((g[i] - c[0]) ** 2 + (g[:, None] - c[1]) ** 2 + (g[None, :] - c[2]) ** 2).sqrt()
        field[i] = (6.3 - d).to(torch.float32)
    v, t = (x.cpu().numpy() for x in marching_cubes(field, 0.0))
    lo = [int(np.floor(float(c[a]) - 9)) for a in range(3)]
    crop = field[lo[0]:lo[0] + 19, lo[1]:lo[1] + 19, lo[2]:lo[2] + 19].cpu().numpy()
    for face in (crop[0], crop[-1], crop[:, 0], crop[:, -1], crop[:, :, 0], crop[:, :, -1]):
        assert np.all(face < 0)
    _same((v, t), R.marching_cubes(crop, 0.0, origin=lo))
    assert R.directed_edges_paired(t, len(v)) and R.euler_characteristic(v, t) == 2


# ------------------------------------------------------------------ the chair's density field
def _model(ck=None):
    from pienerf_amd import scene
    from pienerf_amd.nerf.network import NeRFNetwork
    ck = ck or scene.make_checkpoint(shaped=True)
    return NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10,
                       bg_radius=-1).to(DEV).load_checkpoint_dict(ck)


@pytest.fixture(scope="module")
def chair():
    return _model()


def _reference_fields(bound_min, bound_max, resolution, query_func, S=128):
    """extract_fields' behaviour, restated on the host: per axis a CPU linspace cut into runs of S coordinates; for every (x run, y run, z run),
    x outermost, the run's points in 'ij' meshgrid order go to query_func (on the device) and its values come back into a host array."""
    runs = [list(torch.linspace(float(bound_min[a]), float(bound_max[a]), resolution).split(S)) for a in range(3)]
    host = np.zeros((resolution,) * 3, dtype=np.float32)
    with torch.no_grad():
        for (a, rx), (b, ry), (c, rz) in itertools.product(*(list(enumerate(r)) for r in runs)):
            gx, gy, gz = torch.meshgrid(rx, ry, rz, indexing="ij")
            pts = torch.stack([gx.flatten(), gy.flatten(), gz.flatten()], 1)
            block = query_func(pts).cpu().numpy().reshape(len(rx), len(ry), len(rz))
            host[a * S:a * S + len(rx), b * S:b * S + len(ry), c * S:c * S + len(rz)] = block
    return host


def _reference_geometry(u, bound_min, bound_max, resolution, threshold):
    """The numpy reference's mesh mapped to world space axis by axis: index / (resolution - 1), times the float32 extent of the box, plus its
    lower corner, each step in float64."""
    v, t = R.marching_cubes(u, threshold)
    lo = np.array(bound_min.tolist(), np.float32)
    ext = np.array(bound_max.tolist(), np.float32) - lo
    assert ext.dtype == np.float32
    cols = [v[:, a] / (resolution - 1.0) * float(ext[a]) + float(lo[a]) for a in range(3)]
    return np.stack(cols, 1).reshape(-1, 3), t.astype(np.int64)


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("res", [128, 256])
def test_chair_field_and_geometry_equal_the_reference_pipeline(chair, res, fp16):
    from pienerf_amd.mesh import density_query, lattice_field
    from pienerf_amd.nerf.utils import extract_fields, extract_geometry
    q = density_query(chair, fp16)
    bmin, bmax = chair.aabb_infer[:3], chair.aabb_infer[3:]
    want_u = _reference_fields(bmin, bmax, res, q)
    u = lattice_field(bmin, bmax, res, q)
    assert u.is_cuda and u.dtype == torch.float32
    assert np.array_equal(u.cpu().numpy().view(np.uint32), want_u.view(np.uint32))
    assert np.array_equal(extract_fields(bmin, bmax, res, q).view(np.uint32), want_u.view(np.uint32))
    v, t = extract_geometry(bmin, bmax, res, 10, q)
    wv, wt = _reference_geometry(want_u, bmin, bmax, res, 10)
    assert v.dtype == np.float64 and t.dtype == np.int64
    assert np.array_equal(v.view(np.uint64), wv.view(np.uint64)) and np.array_equal(t, wt)
    assert len(t) > 1000 and R.directed_edges_paired(t, len(v))
    assert R.signed_volume(v, t) > 0
    assert np.all(v >= -1.0) and np.all(v <= 1.0)


@pytest.mark.parametrize("fp16", [False, True])
def test_trainer_writes_the_mesh_and_the_point_cloud(chair, tmp_path, fp16):
    from pienerf_amd import scene
    from pienerf_amd.mesh import density_query
    from pienerf_amd.nerf.utils import extract_geometry
    from pienerf_amd.training import Trainer
    tr = Trainer(chair, scene.default_opt(), fp16=fp16)
    mp, pp = str(tmp_path / "meshes" / "m.ply"), str(tmp_path / "points" / "p.ply")
    tr.save_mesh(mp, resolution=96, threshold=10)
    tr.save_point_cloud(pp, resolution=96, threshold=10)
    v, t = extract_geometry(chair.aabb_infer[:3], chair.aabb_infer[3:], 96, 10, density_query(chair, fp16))
    c = scene.read_ply(mp)
    assert np.array_equal(np.stack([c["x"], c["y"], c["z"]], 1), v.astype(np.float32))
    with open(mp, "rb") as f:
        head = f.read(400).split(b"end_header\n")[0].decode()
    assert f"element face {len(t)}" in head
    lines = open(pp).read().splitlines()
    assert lines[2] == f"element vertex {len(v)}" and len(lines) == 7 + len(v)
    assert lines[7:] == [f"{p[0]} {p[1]} {p[2]}" for p in v]


def test_fp16_trainer_field_is_the_half_density_kernel():
    from pienerf_amd._lib import check, lib, ptr, stream_ptr
    from pienerf_amd.mesh import density_query, lattice_field
    m = _model()
    u = lattice_field(m.aabb_infer[:3], m.aabb_infer[3:], 64, density_query(m, True))
    g = torch.linspace(-1.0, 1.0, 64)
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    pts = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], -1).to(DEV).contiguous()
    sigma = torch.empty(pts.shape[0], dtype=torch.float32, device=DEV)
    geo = torch.empty(pts.shape[0], 15, dtype=torch.float32, device=DEV)
    check(lib().pn_nerf_density_half(m._net_handle(half=True), ptr(pts), pts.shape[0], ptr(sigma), ptr(geo), stream_ptr()), "density_half")
    assert torch.equal(u.reshape(-1).view(torch.int32), sigma.view(torch.int32))


def test_cli_writes_both_files(tmp_path):
    out = str(tmp_path / "mesh_out")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "pienerf_amd.mesh", "--out", out, "--resolution", "64"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "V " in r.stdout and "T " in r.stdout
    from pienerf_amd import scene
    c = scene.read_ply(os.path.join(out, "mesh.ply"))
    lines = open(os.path.join(out, "points.ply")).read().splitlines()
    assert len(c["x"]) > 100 and lines[2] == f"element vertex {len(c['x'])}"
