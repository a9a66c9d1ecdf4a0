"""Checks shared by the mesh tests (CPU and GPU): the properties of a marching-cubes case table
that make meshes watertight and manifold, and the manifold check of an extracted mesh.

A case table is 256 rows of 16 cube-edge ids, -1 padded (tsdf_mc_table / mc_table.table()).  The
geometry of the cube (corners, edges, which faces hold an edge) is restated here from the edge
numbering alone (include/tsdf_hip.h: edge e runs along axis e // 4 from the corner whose other two
coordinate bits are e % 4 in increasing bit order), not taken from either generator."""
from collections import Counter

import numpy as np


def _edge_corners(e):
    axis, r = e // 4, e % 4
    u, v = [a for a in range(3) if a != axis]
    lo = ((r & 1) << u) | (((r >> 1) & 1) << v)
    return lo, lo | (1 << axis)


EDGE_CORNERS = [_edge_corners(e) for e in range(12)]
# the two cube faces (axis, side) that hold each edge
EDGE_FACES = [frozenset((ax, (a >> ax) & 1) for ax in range(3) if (a >> ax) & 1 == (b >> ax) & 1)
              for a, b in EDGE_CORNERS]
EDGE_OF = {}
for _e, (_a, _b) in enumerate(EDGE_CORNERS):
    EDGE_OF[(_a, _b)] = EDGE_OF[(_b, _a)] = _e

# triangles per case of the parent's table (a loop of n crossings gives n - 2 triangles however
# it is fanned, so no change of the fan rule may move these)
NTRI = [
    0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 2, 1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 2, 3, 4, 4, 3, 3, 4, 4, 3, 4, 5, 5, 2,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 2, 4, 3, 3, 4, 4, 5, 4, 3, 5, 2,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4, 3, 4, 4, 3, 4, 3, 5, 2, 4, 5, 5, 4, 5, 4, 2, 1,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 2, 3, 4, 5, 3, 2, 3, 4, 4, 3, 4, 5, 5, 4, 4, 5, 3, 2, 5, 2, 4, 1,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 2, 3, 3, 2, 3, 4, 4, 5, 4, 3, 5, 4, 4, 5, 5, 2, 3, 2, 4, 1,
    3, 4, 4, 5, 4, 5, 5, 2, 4, 5, 3, 4, 3, 4, 2, 1, 2, 3, 3, 2, 3, 2, 4, 1, 3, 4, 2, 1, 2, 1, 1, 0,
]


def case_triangles(table, cfg):
    row = [int(e) for e in table[cfg]]
    n = row.index(-1) if -1 in row else len(row)
    assert n % 3 == 0 and all(0 <= e < 12 for e in row[:n]) and all(e == -1 for e in row[n:]), (cfg, row)
    return [tuple(row[k:k + 3]) for k in range(0, n, 3)]


def triangle_edges(tris):
    return [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]


def case_boundary(table, cfg):
    """Directed triangle edges of the case (in the table's winding) left after each is cancelled
    against its reverse, as a Counter."""
    cnt = Counter(triangle_edges(case_triangles(table, cfg)))
    out = Counter()
    for (a, b), k in cnt.items():
        left = k - cnt.get((b, a), 0)
        if left > 0:
            out[(a, b)] = left
    return out


def face_segments(boundary, face):
    """The boundary's directed edges whose two crossings both lie in cube face (axis, side)."""
    return {s for s in boundary if face in EDGE_FACES[s[0]] and face in EDGE_FACES[s[1]]}


RANDOM_SHAPE = (17, 13, 21)  # no multiples of 8: 3 x 2 x 3 bricks, ragged in every axis


def random_field(seed, shape=RANDOM_SHAPE):
    """Uniform(-1, 1) float32 field; at RANDOM_SHAPE, seeds 0-3, its cells show all 256 cases."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def edge_keys(tsdf):
    """Global identity of every mesh vertex, in mesh order: ((x*Y + y)*Z + z)*3 + axis of each
    grid edge with exactly one end below 0."""
    t = np.asarray(tsdf)
    inside = t < 0
    flags = np.zeros(t.shape + (3,), bool)
    flags[:-1, :, :, 0] = inside[:-1] != inside[1:]
    flags[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    flags[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return np.flatnonzero(flags.reshape(-1))


def cell_cases(tsdf):
    """The marching-cubes case of every cell, shape (X-1, Y-1, Z-1)."""
    inside = np.asarray(tsdf) < 0
    X, Y, Z = inside.shape
    cube = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cube |= inside[ox:X - 1 + ox, oy:Y - 1 + oy, oz:Z - 1 + oz].astype(np.int64) << c
    return cube


def _border_faces(keys, shape):
    """Per vertex, a 6-bit mask of the volume's border faces that hold its grid edge."""
    vox, axis = np.divmod(np.asarray(keys, np.int64), 3)
    idx = np.stack(np.unravel_index(vox, shape), 1)
    mask = np.zeros(len(keys), np.int64)
    for a in range(3):
        lies = axis != a
        mask |= (lies & (idx[:, a] == 0)).astype(np.int64) << (2 * a)
        mask |= (lies & (idx[:, a] == shape[a] - 1)).astype(np.int64) << (2 * a + 1)
    return mask


def check_manifold(faces, keys, shape, all_referenced=True):
    """An oriented manifold mesh with boundary only on the volume's border: every directed edge
    occurs once; a directed edge without its reverse joins two vertices of one border face of the
    volume; no face repeats a vertex; every vertex is used.  Returns the number of open edges."""
    f = np.asarray(faces, np.int64)
    n = len(keys)
    if len(f) == 0:
        assert not all_referenced or n == 0
        return 0
    assert f.min() >= 0 and f.max() < n
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all(), \
        "a face repeats a vertex"
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = e[:, 0] * n + e[:, 1]
    u, cnt = np.unique(code, return_counts=True)
    twice = u[cnt > 1]
    assert len(twice) == 0, f"{len(twice)} directed edges used more than once, e.g. {divmod(int(twice[0]), n)}"
    rev = e[:, 1] * n + e[:, 0]
    open_ = e[~np.isin(rev, code)]
    border = _border_faces(keys, shape)
    stray = open_[(border[open_[:, 0]] & border[open_[:, 1]]) == 0]
    assert len(stray) == 0, f"{len(stray)} open edges off the volume's border, e.g. {stray[0]}"
    if all_referenced:
        assert len(np.unique(f)) == n, "a vertex is not referenced by any face"
    return len(open_)


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return n_verts - len(np.unique(e, axis=0)) + len(f)


def ulp_diff(a, b):
    """Largest distance between two float32 arrays in units in the last place (0 == bit-equal up to
    the sign of zero); NaN anywhere gives a huge number."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    if np.size(a) == 0:
        return 0
    return int(np.abs(key(a) - key(b)).max())
