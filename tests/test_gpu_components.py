"""Connected-component labelling on the GPU (csrc/pn_components.hip) against scipy.ndimage.label, exactly: random occupancy on lattices of every
shape class, empty / full / checkerboard lattices, long thin components, pairs straddling every power-of-two boundary in every direction, a 256^3
lattice, determinism (repeat, stream, graph replay), and the two users: extract_geometry(components=) and AdaptiveUniformSampling(con=).
There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import mc_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRUCT = {6: ndimage.generate_binary_structure(3, 1), 26: np.ones((3, 3, 3), bool)}
# the 13 neighbour offsets of one half-space
HALF = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]


def _scipy(occ, conn):
    """scipy's labels, canonicalised: every voxel carries the smallest flat index of its component, background -1."""
    lab, n = ndimage.label(occ, structure=STRUCT[conn])
    flat = lab.ravel()
    first = np.zeros(n + 1, np.int64)
    idx = np.arange(flat.size, dtype=np.int64)
    first[flat[::-1]] = idx[::-1]          # a repeated index keeps the last value assigned: reversed, that is the first occurrence
    out = first[flat].astype(np.int32)
    out[flat == 0] = -1
    return out.reshape(occ.shape), n


def _gpu(occ, conn):
    from pienerf_amd.components import label_components
    lab = label_components(torch.from_numpy(np.ascontiguousarray(occ)).to(DEV), conn)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == occ.shape
    return lab.cpu().numpy()


def _check(occ, conn):
    want, n = _scipy(occ, conn)
    got = _gpu(occ, conn)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {occ.size} labels differ from scipy"
    return got, n


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 70), (5, 1, 9), (8, 8, 8), (9, 17, 33), (40, 37, 23), (130, 7, 65)])
def test_random_occupancy_equals_scipy(dims, conn):
    rng = np.random.default_rng(sum(dims) + conn)
    for p in (0.2, 0.3, 0.5):
        _check(rng.random(dims) < p, conn)
    _check((rng.random(dims) < 0.3).astype(np.uint8) * 7, conn)       # uint8 input, any non-zero value is occupied


@pytest.mark.parametrize("conn", [6, 26])
def test_empty_and_full_lattices(conn):
    for dims in ((1, 1, 1), (9, 17, 33), (40, 37, 23)):
        got, n = _check(np.zeros(dims, bool), conn)
        assert n == 0 and np.all(got == -1)
        got, n = _check(np.ones(dims, bool), conn)
        assert n == 1 and np.all(got == 0)


def test_checkerboard():
    i, j, k = np.indices((16, 16, 16))
    occ = (i + j + k) % 2 == 0
    got, n = _check(occ, 6)
    assert n == occ.sum() and np.array_equal(got[occ], np.flatnonzero(occ.ravel()))    # every voxel is its own component
    got, n = _check(occ, 26)
    assert n == 1 and np.all(got[occ] == 0)


def _snake(shape, z, x0, ylo, yhi):
    """Rows along y at x = x0, x0 + 2, ... in layer z, joined at alternating ends by one voxel at the odd x between: a one-voxel-wide path."""
    occ = np.zeros(shape, bool)
    rows = list(range(x0, shape[0], 2))
    for n, x in enumerate(rows):
        occ[x, ylo:yhi + 1, z] = True
        if n + 1 < len(rows):
            occ[x + 1, yhi if n % 2 == 0 else ylo, z] = True
    return occ


def test_long_thin_components():
    """One-voxel-wide paths through 48 x 48 x 4 that cross every tile boundary many times.  A path that no voxel of which touches a non-consecutive
    one by a face can use every second row of every second layer at most, so the longest has 2 351 voxels (the issue's "about 4.6 k" is what two
    such paths hold together); with a partner that is corner- but never face-adjacent the first keeps one layer and the partner bridges over z."""
    shape = (48, 48, 4)
    a = _snake(shape, 0, 0, 0, 47)
    long = a | _snake(shape, 2, 0, 0, 47)
    long[46, 47, 1] = True                                           # both layers end at (46, 47): joined there through layer 1
    assert long.sum() == 2351
    for conn in (6, 26):
        got, n = _check(long, conn)
        assert n == 1 and np.all(got[long] == 0)
    # the partner: rows at odd x in layer 1 (edge-adjacent to a's rows), U-turns lifted into layer 2 so that they never sit on top of a
    b = np.zeros(shape, bool)
    rows = list(range(1, 48, 2))
    for n, x in enumerate(rows):
        b[x, 1:47, 1] = True
        if n + 1 < len(rows):
            y = 46 if n % 2 == 0 else 1
            b[x:x + 3, y, 2] = True
    assert not (a & b).any() and b.sum() == 24 * 46 + 23 * 3
    faces = ndimage.binary_dilation(a, structure=STRUCT[6])
    assert not (faces & b).any() and (ndimage.binary_dilation(a, structure=STRUCT[26]) & b).any()
    got, n = _check(a | b, 6)
    assert n == 2 and np.all(got[a] == 0) and np.all(got[b] == np.flatnonzero(b.ravel())[0])
    got, n = _check(a | b, 26)
    assert n == 1 and np.all(got[a | b] == 0)


@pytest.mark.parametrize("conn", [6, 26])
def test_pairs_straddling_every_boundary_in_every_direction(conn):
    """For each of the 13 half-space offsets a lattice of its own (the four corner offsets would otherwise all sit at (s, s, s)): one pair per
    s in {4, 8, 16, 32, 64}, the pair's voxels on either side of index s on every axis the offset moves along, at staggered places on the others."""
    from pienerf_amd.components import label_components
    n = 80
    occs, pairs = [], []
    for d in HALF:
        occ = np.zeros((n, n, n), bool)
        for m, s in enumerate((4, 8, 16, 32, 64)):
            free = (11 + 13 * m, 7 + 14 * m, 5 + 15 * m)
            p = tuple(free[a] if d[a] == 0 else (s - 1 if d[a] > 0 else s) for a in range(3))
            q = tuple(p[a] + d[a] for a in range(3))
            assert all((min(p[a], q[a]), max(p[a], q[a])) == (s - 1, s) for a in range(3) if d[a] != 0)
            occ[p] = occ[q] = True
            pairs.append((len(occs), p, q, sum(c != 0 for c in d) == 1))
        assert occ.sum() == 10
        occs.append(occ)
    labs = [label_components(torch.from_numpy(o).to(DEV), conn).cpu().numpy() for o in occs]
    for o, lab in zip(occs, labs):
        assert np.array_equal(lab, _scipy(o, conn)[0])
    for which, p, q, face in pairs:
        joined = labs[which][p] == labs[which][q]
        assert joined == (face or conn == 26), (HALF[which], p, q)


@pytest.fixture(scope="module")
def big():
    occ = np.random.default_rng(256).random((256, 256, 256)) < 0.3
    return occ, torch.from_numpy(occ).to(DEV)


def test_256_cubed_equals_scipy(big):
    from pienerf_amd.components import label_components
    occ, dev = big
    want, n = _scipy(occ, 26)
    got = label_components(dev, 26).cpu().numpy()
    assert n > 100 and np.array_equal(got, want)


def test_labels_are_a_pure_function_of_the_input(big):
    """Two runs, a run on another stream and two replays of a captured graph give the same bytes."""
    from pienerf_amd.components import label_components
    rng = np.random.default_rng(5)
    for occ in (torch.from_numpy(rng.random((40, 37, 23)) < 0.3).to(DEV), big[1]):
        for conn in (6, 26):
            first = label_components(occ, conn)
            assert torch.equal(label_components(occ, conn), first)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                other = label_components(occ, conn)
            torch.cuda.current_stream().wait_stream(side)
            assert torch.equal(other, first)
    occ = torch.from_numpy(rng.random((40, 37, 23)) < 0.3).to(DEV)
    static = occ.clone()
    eager = label_components(static, 26)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = label_components(static, 26)
    for _ in range(2):
        captured.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    other = torch.from_numpy(rng.random((40, 37, 23)) < 0.5).to(DEV)     # the same launches serve another input
    static.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, label_components(other, 26))


# ------------------------------------------------------------------ meshing
RES, LO, HI = 40, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BOX_C, BOX_H = (-0.25, -0.2, -0.1), (0.45, 0.4, 0.5)
BALLS = [((0.62, 0.6, 0.55), 0.2), ((0.6, -0.62, 0.5), 0.12)]           # the larger sphere first


def _solid_query(pts):
    """> 0 inside a large box or one of two small spheres, < 0 outside (fp32, on the device)."""
    c = torch.tensor(BOX_C, dtype=torch.float32, device=pts.device)
    h = torch.tensor(BOX_H, dtype=torch.float32, device=pts.device)
    f = (h - (pts - c).abs()).min(dim=1).values
    for centre, r in BALLS:
        f = torch.maximum(f, r - (pts - torch.tensor(centre, dtype=torch.float32, device=pts.device)).norm(dim=1))
    return f


@pytest.fixture(scope="module")
def solid():
    from pienerf_amd.mesh import lattice_field
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    field = lattice_field(lo, hi, RES, _solid_query, device=torch.device(DEV)).cpu().numpy()
    lab, n = ndimage.label(field.astype(np.float64) > 0.0, structure=STRUCT[26])
    assert n == 3
    sizes = ndimage.sum_labels(np.ones_like(lab), lab, index=[1, 2, 3])
    order = [int(i) + 1 for i in np.argsort(-sizes, kind="stable")]
    assert sizes[order[0] - 1] > sizes[order[1] - 1] > sizes[order[2] - 1] > 0
    return dict(lo=lo, hi=hi, field=field, lab=lab, order=order)


def _world(idx):
    """extract_geometry's index -> world mapping, restated."""
    origin = np.asarray(LO, np.float32)
    extent = np.asarray(HI, np.float32) - origin
    return idx / (RES - 1.0) * extent.astype(np.float64) + origin.astype(np.float64)


def _reference_mesh(s, keep):
    f = s["field"].copy()
    if keep:
        f[(s["lab"] > 0) & ~np.isin(s["lab"], s["order"][:keep])] = -np.inf
    v, t = R.marching_cubes(f, 0.0)
    return _world(v), t.astype(np.int64)


def _geometry(s, **kw):
    from pienerf_amd.nerf.utils import extract_geometry
    return extract_geometry(s["lo"], s["hi"], RES, 0.0, _solid_query, **kw)


def _triangle_set(v, t):
    return {tuple(v[t_].view(np.uint64).reshape(-1).tolist()) for t_ in t}


def test_extract_geometry_keeps_the_largest_components(solid):
    full = _geometry(solid)
    zero = _geometry(solid, components=0)
    want = _reference_mesh(solid, 0)
    for got in (full, zero):                                          # components=0 is today's output
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])
    all_tris = _triangle_set(*full)
    counts = []
    for keep in (1, 2, 3, 9):
        v, t = _geometry(solid, components=keep)
        wv, wt = _reference_mesh(solid, min(keep, 3))
        assert v.dtype == np.float64 and t.dtype == np.int64
        assert np.array_equal(v.view(np.uint64), wv.view(np.uint64)) and np.array_equal(t, wt), keep      # bitwise
        tris = _triangle_set(v, t)
        assert len(tris) == len(t) and tris <= all_tris               # a sub-mesh of the unfiltered surface
        counts.append(len(t))
        assert R.directed_edges_paired(t.astype(np.int32), len(v))    # still closed
    assert 0 < counts[0] < counts[1] < counts[2] == counts[3] == len(full[1])
    # components=2 keeps the box and the LARGER sphere: no vertex near the small one, some near the large one
    v, _ = _geometry(solid, components=2)
    near = lambda c, r: np.linalg.norm(v - np.asarray(c), axis=1) < r + 0.08
    assert near(*BALLS[0]).any() and not near(*BALLS[1]).any()
    v, _ = _geometry(solid, components=1)
    assert not near(*BALLS[0]).any() and not near(*BALLS[1]).any()


# ------------------------------------------------------------------ sampling
BLOB_BIG, BLOB_SMALL = ((-0.2, 0.0, 0.05), 0.45), ((0.75, 0.7, 0.7), 0.13)     # cubes: (centre, half side)
SIGMA_IN = 400.0


def _in_blob(p, blob, xp):
    c, h = blob
    d = xp.abs(p - (torch.tensor(c, dtype=torch.float32, device=p.device) if xp is torch else np.asarray(c, np.float32)))
    return (d < np.float32(h)).all(1) if xp is np else (d < h).all(dim=1)


def _sigma_np(p):
    p = np.asarray(p, np.float32)
    return np.where(_in_blob(p, BLOB_BIG, np) | _in_blob(p, BLOB_SMALL, np), np.float32(SIGMA_IN), np.float32(0.0)).astype(np.float32)


def _sampler(opt):
    from pienerf_amd.sampling import AdaptiveUniformSampling

    class Analytic(AdaptiveUniformSampling):
        def get_density(self, x):                                     # two-valued, so host and device agree bit for bit
            x = x.to(self.device)
            inside = _in_blob(x, BLOB_BIG, torch) | _in_blob(x, BLOB_SMALL, torch)
            d_in = float(np.float32(1) - np.exp(-np.float32(SIGMA_IN) / np.float32(128.0)))
            return torch.where(inside, torch.full((), d_in, device=self.device), torch.zeros((), device=self.device))
    return Analytic(opt, torch.nn.Identity(), device=DEV)


@pytest.mark.parametrize("vres", [12, 40])                            # below and above sub_res
def test_sampler_keeps_the_points_of_the_largest_component(vres):
    from oracle import sampling as osamp
    from pienerf_amd import scene
    base = scene.default_opt(sub_res=20, sub_coeff=0.55, density_threshold=0.05, sim_dx=0.1)
    rand = torch.from_numpy(np.random.default_rng(11).random((4096, 3)).astype(np.float32))
    plain = _sampler(base)
    p0, v0 = plain.sample(rand=rand)
    off = _sampler(dict(base, con=0, vres=vres))

    def never(pts):
        raise AssertionError("con = 0 entered the component filter")
    off.component_filter = never                                      # con = 0 runs the code without the option and nothing else
    p0b, v0b = off.sample(rand=rand)
    assert torch.equal(p0, p0b) and torch.equal(v0, v0b) and off.last == plain.last and "components" not in off.last
    # the points of that code path, restated on the CPU.  (Its volumes are get_point_volumes', which this feature does not touch; the restatement
    # divides hgs^3 by the count once where torch multiplies by the count's reciprocal, so its volumes are not compared here.)
    rp, _, info = osamp.sample(base, _sigma_np, rand.numpy())
    assert np.array_equal(p0.cpu().numpy(), rp) and info["kept"] == plain.last["kept"]
    big = _in_blob(p0, BLOB_BIG, torch)
    small = _in_blob(p0, BLOB_SMALL, torch)
    assert int(big.sum()) > 500 and int(small.sum()) > 8 and bool((big ^ small).all())
    for conn in (26, 6):
        s = _sampler(dict(base, con=1, vres=vres, con_connectivity=conn))
        p1, v1 = s.sample(rand=rand)
        assert torch.equal(p1, p0[big])                               # the same points in the same order
        assert torch.equal(v1, s.get_point_volumes(p0[big]))
        assert s.last["components"] == 2 and s.last["dropped_points"] == int(small.sum()) and s.last["kept"] == int(big.sum())
        assert len(s.last["kept_components"]) == 1 and s.last["kept_components"][0][1] > 1
    s = _sampler(dict(base, con=2, vres=vres))
    p2, v2 = s.sample(rand=rand)
    assert torch.equal(p2, p0) and torch.equal(v2, v0) and s.last["components"] == 2 and s.last["dropped_points"] == 0
