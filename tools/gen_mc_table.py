"""Generates nmf_amd/csrc/mc_table.hpp, the 256-case triangle table of the marching-cubes kernels (csrc/mesh.hip):

    python tools/gen_mc_table.py            (rewrites the header; the header is committed)
    python tools/gen_mc_table.py --check    (exit status 1 if the committed header differs from what this script generates)

Numbering (restated in the header and in include/nmf_hip.h):
  corner c = dx + 2 dy + 4 dz of the cell's lower corner; bit c of the case index is set when that corner is inside (> level)
  edge e = 4 axis + k runs along `axis` (0 x, 1 y, 2 z) from the corner whose other two coordinates are (k & 1, k >> 1), taken in
  the order of the remaining axes (x: (dy, dz), y: (dx, dz), z: (dx, dy))

Construction (no table is copied from anywhere):
  1. on each of the six cube faces the sign-changing edges of that face are joined into segments.  Two crossings: one segment.
     Four crossings (the two inside corners are diagonal): one segment around EACH INSIDE corner, a rule that depends on the face's
     four corner signs only, so the two cells that share the face cut it by the same segments.
  2. every segment is directed so that, seen from outside the cube, the inside corners it cuts off lie to its right.  The neighbour
     sees the face from the other side: the same segment with the opposite direction (watertight by construction).
  3. every sign-changing edge then has one segment arriving and one leaving; following them gives closed loops.
  4. each loop is fan-triangulated from the first start (in edge order) whose diagonals do not lie in a cube face.
With 2. the triangle normals point from inside to outside: a closed blob has a positive signed volume sum(det[p0, p1, p2]) / 6.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "nmf_amd", "csrc", "mc_table.hpp")


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_corners(e):
    axis, k = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    c0 = ((k & 1) << others[0]) | ((k >> 1) << others[1])
    return c0, c0 | (1 << axis)


EDGES = [edge_corners(e) for e in range(12)]
MID = [(corner_xyz(a) + corner_xyz(b)) / 2.0 for a, b in EDGES]
# a face: (axis, side) -> its four corners, its four edges, its outward normal
FACES = []
for axis, side in itertools.product(range(3), range(2)):
    corners = [c for c in range(8) if ((c >> axis) & 1) == side]
    edges = [e for e, (a, b) in enumerate(EDGES) if a in corners and b in corners]
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    FACES.append((corners, edges, n))


def face_of(e0, e1):
    """index of a cube face both edges lie in, or None"""
    for i, (_, edges, _) in enumerate(FACES):
        if e0 in edges and e1 in edges:
            return i
    return None


def directed(e0, e1, n, right_of):
    """the segment between the two edges, directed so that the corners `right_of` are to its right seen against the normal n"""
    d = MID[e1] - MID[e0]
    left = np.cross(n, d)
    s = sum(float(np.dot(left, corner_xyz(c) - MID[e0])) for c in right_of)
    assert abs(s) > 1e-9
    return (e0, e1) if s < 0 else (e1, e0)


def segments(case):
    inside = lambda c: (case >> c) & 1                                              # noqa: E731
    segs = []
    for corners, edges, n in FACES:
        cross = [e for e in edges if inside(EDGES[e][0]) != inside(EDGES[e][1])]
        ins = [c for c in corners if inside(c)]
        if len(cross) == 2:
            if len(ins) <= 2:
                segs.append(directed(cross[0], cross[1], n, ins))
            else:                                                                  # three inside: the outside corner is to the LEFT
                a, b = directed(cross[0], cross[1], n, [c for c in corners if not inside(c)])
                segs.append((b, a))
        elif len(cross) == 4:
            for q in ins:                                                          # one segment around each inside corner
                e0, e1 = [e for e in cross if q in EDGES[e]]
                segs.append(directed(e0, e1, n, [q]))
        else:
            assert not cross
    return segs


def triangles(case):
    segs = segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (case, segs)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        for rot in range(len(loop)):
            lp = loop[rot:] + loop[:rot]
            diagonals = [(lp[0], lp[i]) for i in range(2, len(lp) - 1)]
            if all(face_of(a, b) is None for a, b in diagonals):
                break
        else:
            raise AssertionError(f"case {case}: no fan without a diagonal in a cube face for loop {loop}")
        tris += [(lp[0], lp[i], lp[i + 1]) for i in range(1, len(lp) - 1)]
    return tris


def render():
    table = [triangles(c) for c in range(256)]
    assert max(len(t) for t in table) <= 5
    lines = [
        "// GENERATED by tools/gen_mc_table.py -- do not edit; regenerate and commit.",
        "// The 256 marching-cubes cases of csrc/mesh.hip.  Corner c = dx + 2 dy + 4 dz; bit c of the case index = corner c is inside.",
        "// Edge e = 4 axis + k runs along axis (0 x, 1 y, 2 z) from the corner whose two other coordinates are (k & 1, k >> 1) in the",
        "// order of the remaining axes.  Triangles are edge triples whose normal points from inside to outside; on a face with four",
        "// crossings every inside corner is cut off by its own segment (a rule of the face's four signs only: neighbours agree).",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "namespace nmf_mc {",
        "",
        "// number of triangles of each case (0..5)",
        "static constexpr uint8_t kNumTri[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in table[r:r + 32]) + ",")
    lines += ["};", "", "// the edge triples of each case, -1 padded", "static constexpr int8_t kTri[256][16] = {"]
    for c, t in enumerate(table):
        flat = [e for tri in t for e in tri]
        flat += [-1] * (16 - len(flat))
        lines.append("    {" + ", ".join(f"{v:2d}" for v in flat) + "},   // " + format(c, "08b"))
    lines += ["};", "", "}  // namespace nmf_mc", ""]
    return "\n".join(lines)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    text = render()
    if "--check" in argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("mc_table.hpp is up to date" if same else "mc_table.hpp differs from the generator's output")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
