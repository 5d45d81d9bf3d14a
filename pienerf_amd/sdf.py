"""Signed-distance grids: what a mesh collider is made of (csrc/pn_sdf.hip; include/pienerf_hip.h: pn_sdf_build has the law).

``SdfGrid`` holds fp32 values [nz, ny, nx] on a device, node (i, j, k) at ``lo + spacing * (i, j, k)``, cubic voxels, 2 .. 512 nodes per axis and at most
2^27 nodes; ``lo`` and ``spacing`` are fp64.  ``SdfGrid.from_mesh`` builds one from a closed triangle mesh in one HIP launch — exact point-to-triangle
distances, signs by the generalised winding number, so either orientation works and a marching-cubes mesh (pienerf_amd.mesh, main_render --save_mesh)
needs no adjacency tables.  The build costs nodes x triangles: 64^3 nodes against 20 000 triangles are 5e9 pairs.  There is no acceleration structure.
``SdfGrid.from_function`` samples a host callable instead (analytic shapes, tests).  ``Simulator.add_mesh_collider`` places a grid as a collider.

Mesh generators for machines without data: ``mesh_box``, ``mesh_icosphere``, ``mesh_terrain`` (a closed solid under a height function), and

    python -m pienerf_amd.sdf --terrain OUT.ply [--size 2.0] [--res 24] [--height 0.15] [--base -1.0]

writes such a terrain in write_mesh_ply's layout (main_render --collide_mesh reads it).

Out of scope: rotation and scaling of a placed grid (rotate the mesh before building), any acceleration of the O(nodes x triangles) build.
"""
import argparse
import warnings

import numpy as np
import torch

SDF_MAX_AXIS = 512
SDF_MAX_NODES = 1 << 27
SDF_MAX_PAIRS = 1 << 38   # PN_SDF_MAX_PAIRS: nodes x triangles of one build, so that the one launch stays a matter of seconds

__all__ = ["SdfGrid", "clean_triangles", "mesh_box", "mesh_icosphere", "mesh_terrain", "mesh_is_closed", "SDF_MAX_AXIS", "SDF_MAX_NODES", "SDF_MAX_PAIRS"]


def _check_res(res):
    r = tuple(int(v) for v in res)
    if len(r) != 3 or any(v < 2 or v > SDF_MAX_AXIS for v in r) or r[0] * r[1] * r[2] > SDF_MAX_NODES:
        raise ValueError(f"SdfGrid: a grid has 2 .. {SDF_MAX_AXIS} nodes per axis and at most 2^27 nodes, got {tuple(res)!r}")
    return r


def clean_triangles(vertices, triangles):
    """(tri9 [T', 9] float32, dropped): the corners of every triangle that is one — those with a repeated index or zero area (the cross product of two
    edges, in fp32, has squared length 0 or is not finite) are dropped, in the builder's arithmetic.  ValueError for an index out of range."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"SdfGrid: a triangle's vertex index lies outside 0 .. {len(v) - 1}")
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.cross(b - a, c - a).astype(np.float32)
        area2 = (x * x).sum(axis=1, dtype=np.float32)
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0]) & np.isfinite(area2) & (area2 > 0.0)
    tri9 = np.ascontiguousarray(np.concatenate([a, b, c], axis=1)[keep], dtype=np.float32)
    return tri9, int((~keep).sum())


class SdfGrid:
    """values: torch fp32 [nz, ny, nx] (x fastest); lo: numpy fp64 [3], the position of node (0, 0, 0); spacing: float.  After from_mesh also
    `dropped` (triangles the wrapper removed), `triangles` (those built from) and `closedness` (max over the nodes off the surface — distance above 1e-5 spacing — of | |w| - round(|w|) |,
    0 for a closed mesh)."""

    def __init__(self, values, lo, spacing):
        if not (isinstance(values, torch.Tensor) and values.dtype == torch.float32 and values.dim() == 3 and values.is_contiguous()):
            raise ValueError("SdfGrid: `values` is a contiguous fp32 tensor [nz, ny, nx]")
        nz, ny, nx = values.shape
        _check_res((nx, ny, nz))
        lo = np.asarray(lo, np.float64).reshape(-1)
        s = float(spacing)
        if lo.size != 3 or not np.isfinite(lo).all() or not (np.isfinite(s) and s > 0.0):
            raise ValueError(f"SdfGrid: `lo` is a finite 3-vector and `spacing` a finite number > 0, got {lo.tolist()!r}, {spacing!r}")
        self.values, self.lo, self.spacing = values, lo.copy(), s
        self.dropped, self.triangles, self.closedness = 0, 0, None

    @property
    def shape(self):
        """(nz, ny, nx)"""
        return tuple(int(v) for v in self.values.shape)

    @property
    def res(self):
        """(nx, ny, nz)"""
        nz, ny, nx = self.shape
        return nx, ny, nz

    @property
    def hi(self):
        return self.lo + self.spacing * (np.array(self.res, np.float64) - 1.0)

    # ------------------------------------------------------------------ builders
    @staticmethod
    def box_for(vertices, resolution=64, spacing=None, margin=None):
        """(lo [3], spacing, res (nx, ny, nz)) of the grid from_mesh lays around a mesh: its bounds plus `margin` on every side (None: two voxels),
        with `resolution` nodes along the longest axis, or with the `spacing` given."""
        v = np.asarray(vertices, np.float64).reshape(-1, 3)
        if len(v) == 0 or not np.isfinite(v).all():
            raise ValueError("SdfGrid: the mesh needs finite vertices")
        vmin, vmax = v.min(axis=0), v.max(axis=0)
        ext = float((vmax - vmin).max())
        if spacing is None:
            n = int(resolution)
            if not 6 <= n <= SDF_MAX_AXIS:
                raise ValueError(f"SdfGrid: resolution is 6 .. {SDF_MAX_AXIS} nodes along the longest axis, got {resolution!r}")
            # (n - 1) s = ext + 2 margin
            s = ext / (n - 1 - 4) if margin is None else (ext + 2.0 * float(margin)) / (n - 1)
        else:
            s = float(spacing)
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError(f"SdfGrid: the spacing must be a finite number > 0, got {s!r} (a mesh without extent needs `spacing`)")
        m = 2.0 * s if margin is None else float(margin)
        if not (np.isfinite(m) and m >= 0.0):
            raise ValueError(f"SdfGrid: margin must be a finite number >= 0, got {margin!r}")
        lo = vmin - m
        res = tuple(int(max(2, np.ceil((vmax[a] + m - lo[a]) / s - 1e-9) + 1)) for a in range(3))
        return lo, s, _check_res(res)

    @classmethod
    def from_mesh(cls, vertices, triangles, resolution=64, spacing=None, margin=None, device="cuda", lo=None, res=None):
        """The signed distance to the closed mesh (vertices [V, 3], triangles [T, 3]), negative inside, built in one launch (pn_sdf_build).  The box:
        box_for(vertices, resolution | spacing, margin), or `lo`, `spacing` and `res` = (nx, ny, nz) given outright.  Warns when the mesh is open
        (closedness > 0.1: signs are not defined).  The cost is nodes x triangles.  RuntimeError without a GPU device: there is no CPU builder."""
        from ._lib import check, lib, ptr, stream_ptr
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("SdfGrid.from_mesh runs on the GPU only (a HIP kernel builds the grid; there is no CPU fallback)")
        if lo is not None or res is not None:
            if lo is None or res is None or spacing is None:
                raise ValueError("SdfGrid.from_mesh: an explicit box needs lo, spacing and res together")
            lo, s, res = np.asarray(lo, np.float64).reshape(3), float(spacing), _check_res(res)
        else:
            lo, s, res = cls.box_for(vertices, resolution, spacing, margin)
        tri9, dropped = clean_triangles(vertices, triangles)
        if len(tri9) == 0:
            raise ValueError(f"SdfGrid.from_mesh: the mesh has no triangle with an area ({dropped} dropped)")
        if len(tri9) > 1 << 24:
            raise ValueError(f"SdfGrid.from_mesh: at most 2^24 triangles, got {len(tri9)}")
        nx, ny, nz = res
        if nx * ny * nz * len(tri9) > SDF_MAX_PAIRS:
            raise ValueError(f"SdfGrid.from_mesh: {nx} x {ny} x {nz} nodes x {len(tri9)} triangles exceed 2^38 node-triangle pairs, the cap of one build "
                             "(there is no acceleration structure): lower the resolution or simplify the mesh")
        with torch.cuda.device(dev):
            t = torch.from_numpy(tri9).to(dev)
            values = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
            wind = torch.empty((nz, ny, nx), dtype=torch.float64, device=dev)
            lo_c = np.ascontiguousarray(lo, dtype=np.float64)
            check(lib().pn_sdf_build(ptr(t), int(len(tri9)), nx, ny, nz, lo_c.ctypes.data, s, ptr(values), ptr(wind), stream_ptr()), "sdf_build")
            w = wind.abs()
            off = values.abs() > 1e-5 * s   # a node on the surface itself sees half the solid angle (w = 1/2 on a face): w jumps there, it says nothing about holes
            closedness = float(((w - torch.round(w)).abs() * off).max().item())
        g = cls(values, lo, s)
        g.dropped, g.triangles, g.closedness = dropped, int(len(tri9)), closedness
        if closedness > 0.1:
            warnings.warn(f"SdfGrid.from_mesh: the mesh is open (winding numbers up to {closedness:.2f} from an integer): inside and outside are not defined")
        return g

    @classmethod
    def from_function(cls, f, lo, spacing, res, device="cpu"):
        """`f` — a host callable taking points [n, 3] fp64 and returning [n] — sampled at the nodes in fp64 and rounded to fp32 once.  res = (nx, ny, nz)."""
        nx, ny, nz = _check_res(res)
        lo = np.asarray(lo, np.float64).reshape(3)
        s = float(spacing)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        pts = lo[None, :] + s * np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(np.float64)
        vals = np.asarray(f(pts), np.float64).reshape(nz, ny, nx)
        if not np.isfinite(vals).all():
            raise ValueError("SdfGrid.from_function: the function returned a value that is not finite")
        return cls(torch.from_numpy(vals.astype(np.float32)).contiguous().to(torch.device(device)), lo, s)

    def to(self, device):
        g = SdfGrid(self.values.to(torch.device(device)).contiguous(), self.lo, self.spacing)
        g.dropped, g.triangles, g.closedness = self.dropped, self.triangles, self.closedness
        return g

    def node_positions(self):
        """[nz, ny, nx, 3] fp64, on the host."""
        nz, ny, nx = self.shape
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return self.lo + self.spacing * np.stack([i, j, k], axis=-1).astype(np.float64)

    # ------------------------------------------------------------------ files
    def save(self, path):
        """.npz: values [nz, ny, nx] fp32, lo [3] fp64, spacing fp64."""
        with open(path, "wb") as f:
            np.savez(f, values=self.values.detach().cpu().numpy(), lo=self.lo, spacing=np.float64(self.spacing))

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as z:
            values, lo, s = np.ascontiguousarray(z["values"], dtype=np.float32), z["lo"], float(z["spacing"])
        if values.ndim != 3:
            raise ValueError(f"SdfGrid.load: {path}: values must be [nz, ny, nx]")
        return cls(torch.from_numpy(values).to(torch.device(device)), lo, s)


# ---------------------------------------------------------------------- mesh generators
def mesh_is_closed(triangles):
    """Whether every edge is shared by exactly two triangles."""
    t = np.asarray(triangles).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool(len(t) > 0 and (counts == 2).all())


def mesh_box(centre=(0.0, 0.0, 0.0), half_extents=(0.5, 0.5, 0.5)):
    """(vertices [8, 3] fp32, triangles [12, 3] int32) of an axis-aligned box, outward orientation."""
    c, h = np.asarray(centre, np.float64).reshape(3), np.asarray(half_extents, np.float64).reshape(3)
    sign = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)   # vertex v = x + 2 y + 4 z over bits
    v = c[None, :] + sign * h[None, :]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # -z, +z, -y, +y, -x, +x
    t = [tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v.astype(np.float32), np.array(t, np.int32)


def mesh_icosphere(subdivisions=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(vertices, triangles) of an icosahedron subdivided `subdivisions` times, every vertex on the sphere: 20 * 4^subdivisions triangles."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid, nt = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    verts = np.asarray(centre, np.float64).reshape(1, 3) + float(radius) * np.array(v)
    return verts.astype(np.float32), np.array(t, np.int32)


def mesh_terrain(height=None, size=2.0, res=24, base=-1.0, centre=(0.0, 0.0)):
    """(vertices, triangles) of a closed solid: the square of side `size` about `centre` (x, z), from y = `base` up to y = height(x, z) (a callable on
    arrays; None: gentle hills about y = base + 0.2), the top sampled on res x res nodes, with walls and a flat bottom.  height must stay above base."""
    n = int(res)
    if n < 2:
        raise ValueError("mesh_terrain: res >= 2")
    xs = centre[0] + np.linspace(-0.5 * size, 0.5 * size, n)
    zs = centre[1] + np.linspace(-0.5 * size, 0.5 * size, n)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    if height is None:
        def height(x, z):
            return base + 0.2 + 0.075 * (np.sin(3.0 * x) * np.cos(2.0 * z) + 0.5 * np.sin(5.0 * z + 1.0))
    Y = np.asarray(height(X, Z), np.float64)
    if Y.shape != X.shape or not np.isfinite(Y).all() or not (Y > base).all():
        raise ValueError("mesh_terrain: height(x, z) must be finite and above `base` everywhere")
    top = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    bot = np.stack([X, np.full_like(X, base), Z], axis=-1).reshape(-1, 3)
    v = np.concatenate([top, bot])

    def T(i, j):
        return i * n + j

    def B(i, j):
        return n * n + i * n + j
    t = []
    for i in range(n - 1):
        for j in range(n - 1):
            t += [(T(i, j), T(i, j + 1), T(i + 1, j + 1)), (T(i, j), T(i + 1, j + 1), T(i + 1, j))]       # top, normal +y
            t += [(B(i, j), B(i + 1, j + 1), B(i, j + 1)), (B(i, j), B(i + 1, j), B(i + 1, j + 1))]       # bottom, normal -y
    for k in range(n - 1):
        for (a0, a1, b0, b1) in ((T(0, k), T(0, k + 1), B(0, k), B(0, k + 1)),                  # x = min, normal -x
                                 (T(n - 1, k + 1), T(n - 1, k), B(n - 1, k + 1), B(n - 1, k)),  # x = max
                                 (T(k + 1, 0), T(k, 0), B(k + 1, 0), B(k, 0)),                  # z = min
                                 (T(k, n - 1), T(k + 1, n - 1), B(k, n - 1), B(k + 1, n - 1))):  # z = max
            t += [(a0, b0, b1), (a0, b1, a1)]
    return v.astype(np.float32), np.array(t, np.int32)


def parser():
    ap = argparse.ArgumentParser(prog="python -m pienerf_amd.sdf", description="write a closed terrain mesh for main_render --collide_mesh")
    ap.add_argument("--terrain", required=True, metavar="OUT.ply", help="the mesh file to write (write_mesh_ply's layout)")
    ap.add_argument("--size", type=float, default=2.0)
    ap.add_argument("--res", type=int, default=24)
    ap.add_argument("--height", type=float, default=0.15, help="the hills' amplitude")
    ap.add_argument("--base", type=float, default=-1.0, help="y of the flat bottom; the hills undulate about base + 0.2")
    return ap


def main(argv=None):
    from . import scene
    a = parser().parse_args(argv)
    amp = 0.5 * a.height

    def height(x, z):
        return a.base + 0.2 + amp * (np.sin(3.0 * x) * np.cos(2.0 * z) + 0.5 * np.sin(5.0 * z + 1.0))
    if not 0.0 <= 1.5 * amp < 0.2:
        raise SystemExit("--height must be in [0, 0.26): the hills stay above the bottom")
    v, t = mesh_terrain(height, size=a.size, res=a.res, base=a.base)
    scene.write_mesh_ply(a.terrain, v, t)
    print(f"{a.terrain}: {len(v)} vertices, {len(t)} triangles, closed: {mesh_is_closed(t)}")
    return a.terrain


if __name__ == "__main__":
    main()
