#!/usr/bin/env python
"""Generates the marching-cubes case table (pienerf_amd/csrc/pn_mc_table.h) from a rule, not from a typed-in table.

    python tools/gen_mc_table.py            # rewrites the header
    python tools/gen_mc_table.py --check    # exit 1 when the committed header differs

The rule ("Meshing"):
  * corners m = 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1), axes x, y, z = field axes 0, 1, 2; Bourke's edges 0..11;
  * bit m of the case index is set when corner m is NOT above the threshold;
  * on each cube face, segments join the crossed edges; a face with four crossed edges cuts off its two above-threshold corners separately
    (decided by the face's own corners, so two cubes sharing the face agree: no cracks);
  * every face segment is directed so that, seen from outside the cube, the above-threshold side lies on the segment's left hand ((b - a) x n_face
    points to it): the segments then chain into directed loops whose right-hand normal points out of the above-threshold region;
  * each loop is fan-triangulated from its smallest edge id whose fan puts no diagonal between two edges of one cube face; loops are taken in
    order of their smallest edge id.  (A fan from the plain smallest edge id lays such a chord across an ambiguous face in 20 loops; when the cube
    on the other side of that face does the same, one edge carries four triangles and the mesh is not a manifold.  Segments on a face are shared
    with the neighbour, diagonals that stay off the faces are shared only inside the loop, so without chords every directed edge meets its
    reverse exactly once.  A chord-free start exists for every loop.)
"""
import os
import sys

import numpy as np

CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))   # Bourke's numbering
# faces: corners in cyclic order and the outward normal
FACES = (((0, 1, 2, 3), (0, 0, -1)), ((4, 5, 6, 7), (0, 0, 1)), ((0, 1, 5, 4), (0, -1, 0)), ((3, 2, 6, 7), (0, 1, 0)), ((0, 3, 7, 4), (-1, 0, 0)),
         ((1, 2, 6, 5), (1, 0, 0)))
MAX_TRIS = 5
SLOTS = 3 * MAX_TRIS
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pienerf_amd", "csrc", "pn_mc_table.h")


def _edge_id(a, b):
    for e, (p, q) in enumerate(EDGES):
        if {p, q} == {a, b}:
            return e
    raise KeyError((a, b))


def _mid(e):
    p, q = EDGES[e]
    return (CORNERS[p] + CORNERS[q]) / 2.0


def _face_segments(above, corners, normal):
    """Directed segments (edge a, edge b) of one face."""
    c = corners
    crossed = [k for k in range(4) if above[c[k]] != above[c[(k + 1) % 4]]]   # face edge k joins c[k], c[k+1]
    pairs = []                                                                  # (edge, edge, an above-threshold corner on the segment's side)
    if len(crossed) == 2:
        k0, k1 = crossed
        up = next(m for m in c if above[m])
        pairs.append((_edge_id(c[k0], c[(k0 + 1) % 4]), _edge_id(c[k1], c[(k1 + 1) % 4]), up))
    elif len(crossed) == 4:
        for k in range(4):                      # cut off each above-threshold corner on its own: join its two face edges
            if above[c[k]]:
                pairs.append((_edge_id(c[(k - 1) % 4], c[k]), _edge_id(c[k], c[(k + 1) % 4]), c[k]))
    segs = []
    n = np.array(normal, np.float64)
    for a, b, up in pairs:
        pa, pb = _mid(a), _mid(b)
        side = float(np.dot(np.cross(pb - pa, n), CORNERS[up] - pa))
        assert side != 0.0
        segs.append((a, b) if side > 0 else (b, a))
    return segs


FACE_EDGES = tuple(frozenset(_edge_id(c[k], c[(k + 1) % 4]) for k in range(4)) for c, _ in FACES)


def _chord_free(loop):
    """The fan from loop[0] has no diagonal joining two edges of one face."""
    return not any(frozenset((loop[0], loop[i])) <= f for i in range(2, len(loop) - 1) for f in FACE_EDGES)


def _case(ci):
    above = [not (ci >> m) & 1 for m in range(8)]
    nxt = {}
    for corners, normal in FACES:
        for a, b in _face_segments(above, corners, normal):
            assert a not in nxt, (ci, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())   # every crossed edge: one segment in, one out
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start                      # start is the loop's smallest edge id (loops are visited in that order)
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    tris = []
    for loop in loops:
        start = min(v for r, v in enumerate(loop) if _chord_free(loop[r:] + loop[:r]))
        r = loop.index(start)
        loop = loop[r:] + loop[:r]
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    assert len(tris) <= MAX_TRIS, (ci, tris)
    return tris


def case_table():
    """(tri_count uint8 [256], tri_edges int8 [256, 15], -1 padded)."""
    count = np.zeros(256, np.uint8)
    edges = np.full((256, SLOTS), -1, np.int8)
    for ci in range(256):
        t = _case(ci)
        count[ci] = len(t)
        if t:
            edges[ci, :3 * len(t)] = np.array(t, np.int8).reshape(-1)
    return count, edges


def header_text():
    count, edges = case_table()
    lines = ["// Generated by tools/gen_mc_table.py: do not edit (python tools/gen_mc_table.py rewrites it; tests/test_mesh_host.py checks it).",
             "// Marching-cubes case table.  Case index: bit m set when corner m is NOT above the threshold; corners m = 0..7 at (0,0,0) (1,0,0)",
             "// (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1) in (axis 0, axis 1, axis 2); Bourke's edge numbering.  Triangles point out of the",
             "// above-threshold region.",
             "#pragma once",
             "",
             f"#define PN_MC_MAX_TRIS {MAX_TRIS}",
             f"#define PN_MC_SLOTS {SLOTS}",
             "",
             "// Initializers: the device's __constant__ copy and the host copy (pn_mc_case_table) are both defined from them.",
             "#define PN_MC_TRI_COUNT_INIT { \\"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(v)) for v in count[r:r + 32]) + ", \\")
    lines += ["}", "", "#define PN_MC_TRI_EDGES_INIT { \\"]
    for ci in range(256):
        lines.append("    {" + ", ".join(f"{int(v):2d}" for v in edges[ci]) + "}, /* " + f"{ci:3d}" + " */ \\")
    lines += ["}", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("up to date" if same else f"{HEADER} differs from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
