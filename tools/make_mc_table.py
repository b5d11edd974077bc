#!/usr/bin/env python3
"""Derive the marching-cubes triangle table of csrc/marching_cubes.hip and write it as a C header (dreg_nerf_amd/csrc/mc_table.h).

    python tools/make_mc_table.py [--out PATH]        (no --out: the committed header's path; tests/test_mc_host.py pins header == generator)

Nothing is transcribed: the 256 rows follow from one rule that reads only corner signs.

* Cube corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1); bit c of a configuration is set when that corner is inside (value > level).
* Cube edge e = 4 * axis + k runs along `axis` (0 x, 1 y, 2 z) from its low corner; k = a + 2 b with (a, b) the low corner's offsets on the two
  other axes in ascending axis order (x edge: (y, z); y edge: (x, z); z edge: (x, y)).  The edge's vertex is owned by the lattice node of its low
  corner.
* On each of the six cube faces the crossing points of the face's four edges are joined: two crossings give one segment; four crossings (the
  ambiguous face, corners alternating) give two segments, each cutting off one INSIDE corner.  The rule reads the face's four corner signs only,
  so the two cells that share a face draw the same segments on it.
* A segment is directed so that, seen from outside the cube, the inside corners lie on its left.  Every crossing point then ends one segment
  and starts one (its two faces see the edge's inside end on opposite sides), so the segments chain into closed loops.
* Loops are taken in ascending order of their smallest edge id and listed from that edge.  Each loop v0 v1 ... v(n-1) is fan-triangulated from
  an apex va: (va, va+1, va+2), (va, va+2, va+3), ... (indices mod n).  The apex is the first vertex of the list whose fan has no diagonal
  INSIDE A CUBE FACE (both ends on edges of one face).  Such a diagonal can only lie on an ambiguous face, and the neighbouring cell may draw
  the same one: the edge would then carry four triangles.  Fanning from v0 blindly does produce such edges on random lattices; an apex without
  them exists for every loop of every configuration (the generator asserts it).  With the direction above the right-hand normal of every
  triangle points to the outside (lower values).

Every mesh edge is then either a fan diagonal strictly inside its cell (used twice there, once per direction) or a face segment (used once by
each of the two cells that share the face, in opposite directions): the mesh is closed and every edge carries two triangles.
tests/test_mc_host.py checks it configuration by configuration and on random lattices."""
import argparse
import os

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_OUT = os.path.join(HERE, "..", "dreg_nerf_amd", "csrc", "mc_table.h")


def corner(x, y, z):
    return x + 2 * y + 4 * z


def edge_between(c0, c1):
    """Edge id of the cube edge joining two corners that differ in one coordinate."""
    d = c0 ^ c1
    axis = {1: 0, 2: 1, 4: 2}[d]
    lo = min(c0, c1)
    p = [lo & 1, lo >> 1 & 1, lo >> 2 & 1]
    a, b = [p[i] for i in range(3) if i != axis]
    return 4 * axis + a + 2 * b


def faces():
    """The six faces as corner 4-cycles, counter-clockwise when seen from OUTSIDE the cube (right-handed axes)."""
    out = []
    for axis in range(3):
        u, v = [(1, 2), (2, 0), (0, 1)][axis]                # (axis, u, v) is a cyclic permutation of (x, y, z): u x v = +axis
        for side in (0, 1):
            cyc = []
            for (a, b) in ((0, 0), (1, 0), (1, 1), (0, 1)):   # counter-clockwise about +axis
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, a, b
                cyc.append(corner(*p))
            if side == 0:                                     # the outward normal is -axis: reverse
                cyc = [cyc[0], cyc[3], cyc[2], cyc[1]]
            out.append(cyc)
    return out


FACES = faces()
FACE_EDGES = [frozenset(edge_between(c[i - 1], c[i]) for i in range(4)) for c in FACES]


def in_a_face(a, b):
    return any(a in f and b in f for f in FACE_EDGES)


def segments(cfg):
    """Directed segments (edge id -> edge id) of one configuration."""
    segs = []
    for cyc in FACES:
        ins = [cfg >> c & 1 for c in cyc]
        for i in range(4):
            # walking the face counter-clockwise (seen from outside) through corners i-1 -> i -> i+1: a run of inside corners STARTS after the
            # crossing on edge (i-1, i) and ENDS before the crossing on some edge (j, j+1).  The segment goes from the run's start crossing to its
            # end crossing: the walk keeps the face's interior on its left, so the run (the inside corners) is cut off on the segment's left.
            if ins[i] and not ins[i - 1]:
                j = i
                while ins[(j + 1) % 4]:
                    j = (j + 1) % 4
                start = edge_between(cyc[i - 1], cyc[i])
                end = edge_between(cyc[j], cyc[(j + 1) % 4])
                segs.append((start, end))
    return segs


def triangles(cfg):
    segs = segments(cfg)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (cfg, segs)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), (cfg, segs)
    tris, seen = [], set()
    for e0 in sorted(nxt):
        if e0 in seen:
            continue
        loop, e = [], e0
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == e0 and len(loop) >= 3, (cfg, loop)
        n = len(loop)
        apex = [a for a in range(n) if not any(in_a_face(loop[a], loop[(a + k) % n]) for k in range(2, n - 1))]
        assert apex, (cfg, loop)
        a = apex[0]
        for i in range(1, n - 1):
            tris.append((loop[a], loop[(a + i) % n], loop[(a + i + 1) % n]))
    return tris


def table():
    rows = [triangles(cfg) for cfg in range(256)]
    width = max(len(r) for r in rows)
    return rows, width


def header_text():
    rows, width = table()
    out = ["// Generated by tools/make_mc_table.py -- do not edit; tests/test_mc_host.py compares this file with the generator's output.",
           "// Row c: the triangles of cube configuration c (bit k set = corner k inside, corner k at (k & 1, k >> 1 & 1, k >> 2 & 1)) as triples of",
           "// cube edge ids 4 * axis + k, -1 after the last one; DREG_MC_NTRI[c] triangles.  Derivation: the generator's docstring.",
           "#pragma once",
           f"#define DREG_MC_WIDTH {width}",
           "static constexpr signed char DREG_MC_TRI[256][3 * DREG_MC_WIDTH] = {"]
    for cfg, r in enumerate(rows):
        flat = [e for t in r for e in t] + [-1] * (3 * (width - len(r)))
        out.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "}," + f"   // {cfg:3d}")
    out.append("};")
    out.append("static constexpr unsigned char DREG_MC_NTRI[256] = {")
    for a in range(0, 256, 32):
        out.append("    " + ", ".join(str(len(r)) for r in rows[a:a + 32]) + ",")
    out.append("};")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    with open(args.out, "w") as f:
        f.write(header_text())
    rows, width = table()
    print(f"{os.path.normpath(args.out)}: 256 configurations, width {width}, {sum(len(r) for r in rows)} triangles")
