"""Mesh extraction on the CPU: the library's case table equals the oracle's restatement of the
rule; both tables, case by case, have the properties that make meshes watertight and manifold
(tests/mesh_checks.py); the oracle's meshes are manifold, closed and consistently oriented, with
the right Euler characteristic; and the PLY writers keep the reference's format
(grid_fusion.py:386-446).  No GPU needed."""
import os

import numpy as np
import pytest

import mc_oracle
import mc_table
import mesh_checks as M


def _library_table():
    from tsdf_amd import _ffi
    tri = np.zeros(256 * 16, np.int8)
    ntri = np.zeros(256, np.uint8)
    _ffi.call("tsdf_mc_table", _ffi.ptr(tri), _ffi.ptr(ntri))
    return tri.reshape(256, 16), ntri


@pytest.fixture(scope="module", params=["library", "oracle"])
def table(request):
    """The case table of csrc/tsdf_mesh.hip (tsdf_mc_table) or of oracle/mc_table.py, as lists."""
    if request.param == "library":
        return _library_table()[0].astype(int).tolist()
    return mc_table.table()


def test_library_case_table_equals_oracle_rule():
    from tsdf_amd import _ffi
    tri = np.zeros(256 * 16, np.int8)
    ntri = np.zeros(256, np.uint8)
    _ffi.call("tsdf_mc_table", _ffi.ptr(tri), _ffi.ptr(ntri))
    ref = np.array(mc_table.table(), np.int8)
    assert np.array_equal(tri.reshape(256, 16), ref)
    assert np.array_equal(ntri, (ref >= 0).sum(axis=1) // 3)
    assert ntri.max() == 5 and ntri[0] == ntri[255] == 0


def test_checker_restates_the_cube_of_the_table():
    """tests/mesh_checks.py derives the cube's edges from the numbering the header documents; it
    must be the numbering both generators use."""
    assert [tuple(e) for e in mc_table.EDGES] == M.EDGE_CORNERS
    assert all(len(f) == 2 for f in M.EDGE_FACES)


def test_triangle_counts_are_the_parents(table):
    """The fan rule may move diagonals, never the number of triangles (bench.py's mesh figures)."""
    assert [len(M.case_triangles(table, c)) for c in range(256)] == M.NTRI
    assert np.array_equal(_library_table()[1], M.NTRI)


def test_triangle_boundary_of_every_case_is_its_face_segments(table):
    """Per case, the triangles' directed edges (table winding, before the (0, 2, 1) flip of the
    emit), each cancelled against its reverse, leave exactly the case's face segments, once each:
    the triangles of a case tile its loops and nothing else."""
    for cfg in range(256):
        edges = M.triangle_edges(M.case_triangles(table, cfg))
        assert len(set(edges)) == len(edges), f"case {cfg}: a directed edge twice"
        want = {}
        for loop in mc_table.case_loops(cfg):
            for i, e in enumerate(loop):
                want[(e, loop[(i + 1) % len(loop)])] = 1
        assert dict(M.case_boundary(table, cfg)) == want, f"case {cfg}"


def test_no_stray_triangle_edge_in_a_cube_face(table):
    """A triangle edge between two crossings of one cube face lies in that face's plane, where
    the neighbouring cell can emit it too (four triangles on one edge), unless it is one of the
    face's own segments, which the neighbour emits reversed.  The smallest-edge fan broke this in
    18 cases (91, 94, 111, 118, 123, 159, 167, 173, ...)."""
    bad = []
    for cfg in range(256):
        segs = M.case_boundary(table, cfg)
        for a, b in M.triangle_edges(M.case_triangles(table, cfg)):
            if M.EDGE_FACES[a] & M.EDGE_FACES[b] and (a, b) not in segs and (b, a) not in segs:
                bad.append(cfg)
                break
    assert not bad, f"{len(bad)} cases with a fan diagonal inside a cube face: {bad}"


def test_cases_agree_across_every_shared_face(table):
    """For every axis, every case A and every case B that can sit at A's +axis side (B's low-face
    corners are A's high-face corners; B's other four corners free: 256 x 3 x 16 pairs), A's
    segments on the shared face are B's reversed.  This keeps ambiguous faces watertight."""
    bnd = [M.case_boundary(table, c) for c in range(256)]
    pairs = 0
    for axis in range(3):
        bit = 1 << axis
        shift = {}  # A's edge on its high face -> the same grid edge as B's edge on its low face
        for e, (a, b) in enumerate(M.EDGE_CORNERS):
            if a & bit and b & bit:
                shift[e] = M.EDGE_OF[(a ^ bit, b ^ bit)]
        assert len(shift) == 4
        free = [c for c in range(8) if c & bit]
        for A in range(256):
            low = sum(((A >> (c | bit)) & 1) << c for c in range(8) if not c & bit)
            mine = {(shift[p], shift[q]) for p, q in M.face_segments(bnd[A], (axis, 1))}
            for k in range(16):
                B = low | sum(((k >> i) & 1) << c for i, c in enumerate(free))
                theirs = {(q, p) for p, q in M.face_segments(bnd[B], (axis, 0))}
                assert mine == theirs, (axis, A, B)
                pairs += 1
    assert pairs == 256 * 3 * 16


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_field_mesh_is_manifold(table, seed):
    """A uniform random field reaches all 256 cases, the 18 with 6- and 7-edge loops among them
    (8-52 directed edges were used twice per such mesh under the smallest-edge fan)."""
    t = M.random_field(seed)
    assert len(np.unique(M.cell_cases(t))) == 256
    color = np.zeros(t.shape, np.float32)
    v, n, col, f = mc_oracle.extract(t, color, np.zeros(3, np.float32), 1.0, table=table)
    keys = M.edge_keys(t)
    assert len(keys) == len(v) and len(f) > 4000
    opened = M.check_manifold(f, keys, t.shape)
    assert opened > 0  # the surface does reach the volume's border


def _grid(shape):
    return np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1).astype(np.float64)


def _sphere(n=24, r=7.3, c=(11.2, 12.1, 10.7)):
    x, y, z = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
    return np.clip(d / 3.0, -1, 1).astype(np.float32), np.array(c), r


class _Scene:
    """A solid by its signed distance `dist(points)` and the direction `outward(points)` from the
    solid's core to each point; tsdf = clip(dist / 3, -1, 1) on a grid of `shape`."""

    def __init__(self, shape, dist, outward, euler):
        self.shape, self.dist, self.outward, self.euler = shape, dist, outward, euler
        self.tsdf = np.clip(dist(_grid(shape)) / 3.0, -1, 1).astype(np.float32)


def _sphere_scene():
    t, c, r = _sphere()
    s = _Scene(t.shape, lambda p: np.linalg.norm(p - c, axis=-1) - r, lambda p: p - c, 2)
    assert np.array_equal(s.tsdf, t)
    return s


def _two_spheres_scene():
    cs = np.array([[6.2, 7.1, 6.7], [16.3, 15.2, 16.4]])
    rs = np.array([4.3, 5.1])

    def both(p):
        return np.stack([np.linalg.norm(p - c, axis=-1) - r for c, r in zip(cs, rs)], -1)

    def outward(p):
        return p - cs[np.argmin(both(p), axis=-1)]
    return _Scene((24, 24, 24), lambda p: both(p).min(-1), outward, 4)


def _torus_scene(c=(11.6, 11.4, 7.7), R=8.0, r=3.0):
    c = np.array(c)

    def ring(p):  # the nearest point of the torus' centre circle
        q = (p - c)[..., :2]
        q = q / np.linalg.norm(q, axis=-1, keepdims=True) * R
        return np.concatenate([q, np.zeros(q.shape[:-1] + (1,))], -1) + c
    return _Scene((24, 24, 16), lambda p: np.linalg.norm(p - ring(p), axis=-1) - r, lambda p: p - ring(p), 0)


def _check_closed_and_outward(scene, table=None):
    t = scene.tsdf
    color = np.full(t.shape, 3 * 65536 + 2 * 256 + 1, np.float32)
    v, n, col, f = mc_oracle.extract(t, color, np.zeros(3, np.float32), 1.0, table=table)
    assert len(f) > 100
    # every directed edge once, its reverse once: closed and consistently oriented
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    s = set(map(tuple, e))
    assert len(s) == len(e) and all((b, a) in s for a, b in s)
    vd = v.astype(np.float64)
    assert np.abs(scene.dist(vd)).max() < 0.2
    assert (np.einsum("ij,ij->i", n, scene.outward(vd)) > 0).all()
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", fn, scene.outward(vd[f].mean(axis=1))) > 0).mean() > 0.99
    assert (col == [1, 2, 3]).all()
    return v, f


def test_oracle_mesh_is_closed_and_outward():
    _check_closed_and_outward(_sphere_scene())


@pytest.mark.parametrize("scene", [_sphere_scene, _two_spheres_scene, _torus_scene])
def test_euler_characteristic_of_closed_meshes(table, scene):
    """V - E + F: 2 per sphere, 0 for a torus (wholly inside a 24 x 24 x 16 grid, radii 8 and 3
    voxels); each scene closed and outward as the sphere of the test above."""
    sc = scene()
    t = sc.tsdf  # the solid stays off the grid's border: the mesh has no boundary
    assert min(t[[0, -1]].min(), t[:, [0, -1]].min(), t[:, :, [0, -1]].min()) > 0
    v, f = _check_closed_and_outward(sc, table)
    assert M.check_manifold(f, M.edge_keys(sc.tsdf), sc.shape) == 0
    assert M.euler_characteristic(len(v), f) == sc.euler


def test_ply_writers_match_reference_format(tmp_path):
    from tsdf_amd import grid_fusion
    v = np.array([[0.5, 1.25, -2.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    n = np.eye(3, dtype=np.float32)
    c = np.array([[255, 0, 7], [1, 2, 3], [9, 8, 7]], np.uint8)
    f = np.array([[0, 1, 2]], np.int32)
    p = os.path.join(tmp_path, "m.ply")
    grid_fusion.meshwrite(p, v, f, n, c)
    lines = open(p).read().splitlines()
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex 3"]
    assert lines[12:15] == ["element face 1", "property list uchar int vertex_index", "end_header"]
    assert lines[15] == "0.500000 1.250000 -2.000000 1.000000 0.000000 0.000000 255 0 7"
    assert lines[-1] == "3 0 1 2"
    q = os.path.join(tmp_path, "p.ply")
    grid_fusion.pcwrite(q, np.hstack([v, c]))
    lines = open(q).read().splitlines()
    assert lines[2] == "element vertex 3" and lines[9] == "end_header"
    assert lines[10] == "0.500000 1.250000 -2.000000 255 0 7"
