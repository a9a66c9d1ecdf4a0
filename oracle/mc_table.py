"""TEST INFRASTRUCTURE ONLY -- the marching-cubes case table restated for the oracle.

The reference meshes with skimage.measure.marching_cubes_lewiner (grid_fusion.py:327,348), which
is not installed here, so its triangles cannot be reproduced; PARITY UNPINNED for triangles (see
DESIGN.md).  The MI355X build derives its case table from one rule, restated here independently
of the library's C++ generator (csrc/tsdf_mesh.hip) so that tests can compare them:

  cube corners c = (x, y, z) bits (c & 1, c >> 1 & 1, c >> 2 & 1); a corner is INSIDE when its
  tsdf < 0; the 12 edges join corners differing in one bit; on each of the 6 faces, walked
  counter-clockwise as seen from outside the cube, every maximal run of inside corners gives
  one surface segment from the crossing where the walk leaves the run to the crossing where it
  entered it (so an ambiguous face keeps its two inside corners apart); segments chain into
  closed loops (each crossed edge starts one segment and ends one), and each loop is fanned
  into triangles.  The loops are taken in order of their smallest starting edge and walked
  from that edge; the fan starts at the first position of the walk from which no diagonal
  joins two crossings that lie in one cube face (such a position exists for every loop of
  every case; tests/test_mesh_cpu.py).

Why the fan start matters.  A diagonal between two crossings of one cube face lies in that
face's plane, and the cell across the face can emit the same directed edge, so four triangles
meet in one edge.  Fanning every loop from its smallest edge did that in 18 of the 256 cases,
all with a loop of 6 or 7 crossings: 91, 94, 111, 118, 123, 159, 167, 173, 183, 185, 217, 218,
222, 229, 230, 237, 246, 249.  Measured with mc_oracle.extract: 8-52 directed edges used twice
per mesh of a uniform random 13 x 9 x 17 field (seeds 0-7, about 4 900 triangles each); on
tests/golden/dense_c1.npz after its three frames (128^3), 111 of 16 969 surface cells were in
those cases and 8 directed edges were used twice among 34 632 triangles.  The rule above changes
the triangles of exactly those 18 cases, no case's triangle count, and brings both counts to 0.
What it guarantees, case by case: the triangles of a case tile its loops (their boundary is the
face segments, once each), no other triangle edge lies in a cube face, and the segments of two
cells on their shared face are each other's reverses -- so every directed edge of a mesh occurs
once, and an edge lacks its reverse only in a border face of the volume.
"""
from __future__ import annotations

CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
# edges sorted by (axis, lower corner): index = axis * 4 + (the two other coordinate bits)
EDGES = []
for axis in range(3):
    for c in range(8):
        if not (c >> axis) & 1:
            EDGES.append((c, c | (1 << axis)))
EDGE_ID = {}
for i, (a, b) in enumerate(EDGES):
    EDGE_ID[(a, b)] = EDGE_ID[(b, a)] = i


def _faces():
    """6 faces as corner cycles, counter-clockwise seen from outside (outward normal)."""
    faces = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3  # (u, v, axis) right-handed
        for side in (0, 1):
            base = side << axis
            cyc = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            if side == 0:  # outward normal is -axis: reverse to stay counter-clockwise
                cyc = cyc[::-1]
            faces.append(cyc)
    return faces


FACES = _faces()


def case_loops(cfg: int):
    inside = [(cfg >> c) & 1 for c in range(8)]
    seg = {}  # start edge -> end edge
    for cyc in FACES:
        n = 4
        if all(inside[c] for c in cyc) or not any(inside[c] for c in cyc):
            continue
        for i in range(n):
            a, b = cyc[i], cyc[(i + 1) % n]
            if inside[a] and not inside[b]:  # leaving a run at edge (a, b)
                # walk back to where the run was entered
                j = i
                while inside[cyc[(j - 1) % n]]:
                    j -= 1
                p, q = cyc[(j - 1) % n], cyc[j % n]  # entering edge (p outside, q inside)
                seg[EDGE_ID[(a, b)]] = EDGE_ID[(p, q)]
    loops = []
    left = dict(seg)
    while left:
        start = min(left)
        loop = [start]
        e = left.pop(start)
        while e != start:
            loop.append(e)
            e = left.pop(e)
        loops.append(loop)
    return loops


def _edge_faces(e: int):
    """The two cube faces (axis, side) that hold edge e."""
    a, b = EDGES[e]
    return {(ax, (a >> ax) & 1) for ax in range(3) if (a >> ax) & 1 == (b >> ax) & 1}


EDGE_FACES = [_edge_faces(e) for e in range(12)]


def fan_start(loop):
    """First position of the loop (walked from its smallest edge) whose fan has no diagonal
    between two crossings of one cube face."""
    n = len(loop)
    for s in range(n):
        if not any(EDGE_FACES[loop[s]] & EDGE_FACES[loop[(s + i) % n]] for i in range(2, n - 1)):
            return s
    raise AssertionError(("no admissible fan start", loop))


def triangles(cfg: int):
    tris = []
    for loop in case_loops(cfg):
        n, s = len(loop), fan_start(loop)
        for i in range(1, n - 1):
            tris.append((loop[s], loop[(s + i) % n], loop[(s + i + 1) % n]))
    return tris


def table():
    """256 x 16 list of edge ids, -1 padded (at most 5 triangles per case)."""
    out = []
    for cfg in range(256):
        t = [e for tri in triangles(cfg) for e in tri]
        assert len(t) <= 15, (cfg, len(t))
        out.append(t + [-1] * (16 - len(t)))
    return out
