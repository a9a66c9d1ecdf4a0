"""GPU marching cubes (tsdf_dense_extract_mesh) against the oracle's
restatement (oracle/mc_oracle.py): vertices, colours and faces bit-exact, normals within 1e-6
(measured: at most 2 ulp, see _check_exact).
Triangulation parity with the reference's skimage.marching_cubes_lewiner is UNPINNED (skimage is
not installed); the vertex rule (linear zero crossings on grid edges, colours of the voxels at
round(vertex), grid_fusion.py:336-346) is the reference's."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import mc_oracle
import mesh_checks as M

pytestmark = pytest.mark.gpu
C1 = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]


@pytest.fixture(scope="module")
def gf():
    from tsdf_amd import grid_fusion
    return grid_fusion


def _check(vol, t, c):
    v, n, col, f = vol.extract_mesh()
    rv, rn, rc, rf = mc_oracle.extract(t, c, vol._vol_origin, vol._voxel_size)
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(col, rc) and np.array_equal(f, rf)
    assert np.abs(n - rn).max() <= 1e-6
    return v, n, col, f


def test_mesh_of_lounge_c1_equals_oracle(gf):
    K = lounge_intrinsics()
    vol = gf.TSDFVolume(np.array(C1), 0.04)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, K, pose)
    t, _, c = vol.get_state()
    v, n, col, f = _check(vol, t, c)
    assert len(f) > 10000
    # (111 of this state's surface cells are in the 18 cases whose fan start moved)
    M.check_manifold(f, M.edge_keys(t), t.shape)
    verts, faces, norms, colors = vol.get_mesh()  # the reference's return order
    assert np.array_equal(verts, v) and np.array_equal(faces, f) and np.array_equal(colors, col)
    pc = vol.get_point_cloud()
    assert pc.shape == (len(v), 6) and np.array_equal(pc[:, :3], v) and np.array_equal(pc[:, 3:], col)


def test_mesh_of_ragged_set_state_volume(gf):
    """A state written with set_state into a volume whose dims are not multiples of 8, with
    exact zeros and both signs at the borders."""
    rng = np.random.default_rng(5)
    bnds = np.array([[0.0, 0.63], [0.0, 0.45], [0.0, 0.37]])
    vol = gf.TSDFVolume(bnds.copy(), 0.01)
    shape = tuple(int(d) for d in vol._vol_dim)
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    t = np.clip((np.sqrt((x - 30.3) ** 2 + (y - 20.2) ** 2 + (z - 18.9) ** 2) - 14.0) / 4.0, -1, 1).astype(np.float32)
    t[::7, ::5, ::3] = 0.0
    c = rng.integers(0, 1 << 24, size=shape).astype(np.float32)
    vol.set_state(t, np.ones(shape, np.float32), c)
    _check(vol, t, c)


def test_hash_mesh_equals_dense_mesh(gf):
    from tsdf_amd import hash_fusion
    K = lounge_intrinsics()
    vol = gf.TSDFVolume(np.array(C1), 0.04)
    ht = hash_fusion.HashTable(np.array(C1), 0.04, 1 << 16)
    for i in range(2):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, K, pose)
        ht.integrate(rgb, depth, K, pose)
    a, b = vol.get_mesh(), ht.get_mesh()
    t_h = ht.get_state()[0]
    # each mesh is the oracle's mesh of its own state, whichever branch below is taken
    for src, (v, f, n, col) in ((vol, a), (ht, b)):
        t, _, c = src.get_state()
        rv, rn, rc, rf = mc_oracle.extract(t, c, src._vol_origin, src._voxel_size)
        assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)) and np.array_equal(f, rf)
        assert np.array_equal(col, rc) and np.abs(n - rn).max() <= 1e-6
    if np.array_equal(vol.get_state()[0], t_h):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    else:  # f32 hash state may differ from the grid's by rounding; meshes agree in topology
        assert abs(len(a[0]) - len(b[0])) <= 0.001 * len(a[0])


def test_hash_densifies_on_the_device_like_the_host_export(gf):
    """tsdf_hash_to_dense (get_mesh / get_point_cloud of the hash without a host round trip)
    writes exactly get_state()'s volume into a dense handle: integrated blocks, an entry of
    weight 0 set by add_entries, a removed entry, and a ragged extent (dims not multiples of 8)."""
    from tsdf_amd import _ffi, hash_fusion
    bnds = np.array([[-2.56, 1.48], [-2.52, 2.56], [0.0, 5.00]])
    K = lounge_intrinsics()
    ht = hash_fusion.HashTable(bnds.copy(), 0.04, 1 << 12)
    for i in range(2):
        _, depth, rgb, pose = load_lounge(i)
        ht.integrate(rgb, depth, K, pose)
    ht.add_entries([[1, 2, 3], [100, 126, 124]], tsdf=[0.5, -0.25], weight=[0.0, 3.0], color=[7.0, 65793.0])
    ht.remove_entries([[1, 2, 4]])
    grid = ht._as_grid()
    for a, b in zip(grid.get_state(), ht.get_state()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    other = gf.TSDFVolume(np.array(C1), 0.04)
    with pytest.raises(_ffi.TSDFError):
        _ffi.call("tsdf_hash_to_dense", ht._h, other._h)  # dims differ


# ---- synthetic states: every case, the normal's zero branch, rounding ties, extreme ratios --------
ORIGIN = (-0.37, 0.21, 1.03)
VS = 0.01


def _bounds(shape, origin=ORIGIN, vs=VS):
    lo = np.array(origin, float)
    return np.stack([lo, lo + (np.array(shape) - 0.5) * vs], axis=1)  # ceil(extent / vs) == shape


def _volume(gf, shape):
    vol = gf.TSDFVolume(_bounds(shape), VS)
    assert tuple(int(d) for d in vol._vol_dim) == tuple(shape)
    assert np.all(vol._vol_origin != 0)
    return vol


def _colors(shape, seed=11):
    return np.random.default_rng(seed).integers(0, 1 << 24, size=shape).astype(np.float32)


def _loaded(gf, t, c=None):
    t = np.ascontiguousarray(t, np.float32)
    c = _colors(t.shape) if c is None else c
    vol = _volume(gf, t.shape)
    vol.set_state(t, np.ones(t.shape, np.float32), c)
    return vol, t, c


def _check_exact(vol, t, c, manifold=True):
    """The GPU mesh of a state equals the oracle's -- vertices, colours, faces and keys to the bit,
    normals within 1e-6 -- and is manifold by itself.  Normals, measured on the MI355X as the largest
    difference from the oracle: 2 ulp on the all-cases field (6496 vertices), on the volumes one
    voxel thick and on the single cells; 0 ulp on the checkerboard, the half-way ties and the
    extreme ratios.  Not 0 everywhere, so they stay at 1e-6 (the cause, the native square root
    behind __fsqrt_rn, is in DESIGN.md §7c); the figure is printed on every run."""
    v, n, col, f, k = vol.extract_mesh(keys=True)
    rv, rn, rc, rf = mc_oracle.extract(t, c, vol._vol_origin, vol._voxel_size)
    assert v.shape == rv.shape == n.shape == col.shape and f.shape == rf.shape
    assert v.dtype == n.dtype == np.float32 and col.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(k, M.edge_keys(t))
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(col, rc) and np.array_equal(f, rf)
    print("normals: max |gpu - oracle| = %d ulp over %d vertices" % (M.ulp_diff(n, rn), len(n)))
    assert not np.isnan(n).any()
    assert np.abs(n - rn).max(initial=0) <= 1e-6
    assert np.array_equal(n == 0, rn == 0)  # the len == 0 branch is taken for the same vertices
    if manifold:
        M.check_manifold(f, k, t.shape, all_referenced=min(t.shape) > 1)
    return v, n, col, f, k


@pytest.fixture(scope="module")
def all_cases(gf):
    """(volume, tsdf, colour) of the random field whose cells show all 256 cases; the tests that
    share it leave its state alone."""
    vol, t, c = _loaded(gf, M.random_field(0))
    assert len(np.unique(M.cell_cases(t))) == 256
    return vol, t, c


def test_mesh_of_all_256_cases_equals_oracle(all_cases):
    """(17, 13, 21): 3 x 2 x 3 bricks, no dimension a multiple of 8, every case present."""
    v, n, col, f, k = _check_exact(*all_cases)
    assert len(f) > 4000


def test_checkerboard_normals_are_exact_zeros(gf):
    """t = +-1 by the parity of x + y + z: only cases 105 and 150, and every central difference
    away from the border is 0, so the normal takes its len == 0 branch: +0.0, never NaN."""
    shape = (9, 6, 11)
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    vol, t, c = _loaded(gf, np.where((x + y + z) % 2 == 0, -1.0, 1.0))
    assert set(np.unique(M.cell_cases(t))) == {105, 150}
    v, n, col, f, k = _check_exact(vol, t, c)
    vox, axis = np.divmod(k, 3)
    idx = np.stack(np.unravel_index(vox, shape), 1)
    end = idx + np.eye(3, dtype=np.int64)[axis]
    inner = np.all((idx >= 1) & (end <= np.array(shape) - 2), axis=1)  # both ends off the border
    assert inner.sum() > 100
    assert np.all(n[inner].view(np.uint32) == 0)
    ln = np.linalg.norm(n.astype(np.float64), axis=1)  # (edges in a border face cancel to 0 too)
    assert np.all((ln == 0) | (np.abs(ln - 1) < 1e-6)) and (ln > 0).sum() > 100


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_way_vertices_take_the_colour_of_the_even_voxel(gf, axis):
    """Slabs of -0.5 / +0.5 alternating along one axis put every vertex exactly half-way along its
    edge; round-half-to-even (np.round, rintf) then picks the voxel with the even index."""
    shape = (7, 5, 6)
    i = np.arange(shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
    t = np.broadcast_to(np.where(i % 2 == 0, -0.5, 0.5), shape)
    vol, t, c = _loaded(gf, t)
    v, n, col, f, k = _check_exact(vol, t, c)
    vox, ax = np.divmod(k, 3)
    assert np.all(ax == axis) and len(k) == (shape[axis] - 1) * np.prod(shape) // shape[axis]
    idx = np.stack(np.unravel_index(vox, shape), 1)
    p = (v.astype(np.float64) - vol._vol_origin.astype(np.float64)) / VS
    assert np.abs(p[:, axis] - (idx[:, axis] + 0.5)).max() < 1e-3
    idx[:, axis] += idx[:, axis] % 2  # the even end of the edge
    cv = c[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.int64)
    assert np.array_equal(col, np.stack([cv & 255, (cv >> 8) & 255, cv >> 16], 1).astype(np.uint8))


@pytest.mark.parametrize("pair", [(-1.0, 2.0 ** -100), (-(2.0 ** -100), 1.0), (-1e-39, 3e-39)])
def test_extreme_edge_ratios_equal_oracle(gf, pair):
    """Slabs alternating between the pair's values along x, y, z in turn: t = v1 / (v1 - v2) rounds
    to 0.0 or 1.0, or its operands are f32 subnormals.  The library keeps f32 subnormals and its
    division is correctly rounded, so the mesh equals the oracle's to the bit here too."""
    shape = (6, 7, 5)
    pair = np.array(pair, np.float32)
    assert pair[0] < 0 < pair[1]  # neither flushed to zero on the host
    for axis in range(3):
        i = np.arange(shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
        vol, t, c = _loaded(gf, np.broadcast_to(pair[i % 2], shape))
        v, n, col, f, k = _check_exact(vol, t, c)
        assert len(v) == (shape[axis] - 1) * np.prod(shape) // shape[axis]


# ---- degenerate volumes ----------------------------------------------------------------------------
def _is_empty(mesh):
    v, n, col, f = mesh[:4]
    return v.shape == n.shape == col.shape == f.shape == (0, 3)


@pytest.mark.parametrize("bounds,vs", [
    ([[-1.3, 1.1], [-0.9, 1.7], [0.3, 4.0]], 0.05),      # the volumes of test_ragged_and_degenerate_volumes
    ([[-0.01, 0.01], [-0.01, 0.01], [2.0, 2.02]], 0.02),  # (dimensions of 1)
    ([[-6.0, -5.0], [-6.0, -5.0], [-3.0, -2.0]], 0.05),
])
def test_fresh_and_all_negative_volumes_give_an_empty_mesh(gf, bounds, vs):
    vol = gf.TSDFVolume(np.array(bounds, float), vs)
    assert _is_empty(vol.extract_mesh())
    assert vol.extract_mesh(keys=True)[4].shape == (0,)
    assert vol.get_point_cloud().shape == (0, 6)
    shape = tuple(int(d) for d in vol._vol_dim)
    vol.set_state(np.full(shape, -1.0, np.float32), np.ones(shape, np.float32), np.zeros(shape, np.float32))
    assert _is_empty(vol.extract_mesh())
    t, _, c = vol.get_state()
    assert _is_empty(mc_oracle.extract(t, c, vol._vol_origin, vol._voxel_size))


@pytest.mark.parametrize("shape", [(1, 5, 7), (5, 1, 7), (5, 7, 1), (1, 1, 9), (1, 1, 1)])
def test_volume_one_voxel_thick_gives_vertices_and_no_faces(gf, shape):
    vol, t, c = _loaded(gf, M.random_field(3, shape))
    v, n, col, f, k = _check_exact(vol, t, c)
    assert f.shape == (0, 3) and (len(v) > 0) == (max(shape) > 1)


@pytest.mark.parametrize("case", [1, 105, 254])
def test_single_cell_volume(gf, case):
    mag = np.array([0.3, 0.9, 0.5, 0.7, 0.2, 1.0, 0.6, 0.4], np.float32)
    t = np.zeros((2, 2, 2), np.float32)
    for corner in range(8):
        t[corner & 1, (corner >> 1) & 1, corner >> 2] = mag[corner] * (-1 if (case >> corner) & 1 else 1)
    vol, t, c = _loaded(gf, t)
    assert M.cell_cases(t).tolist() == [[[case]]]
    v, n, col, f, k = _check_exact(vol, t, c)
    assert len(f) == M.NTRI[case]


@pytest.mark.parametrize("corner", [(0, 0, 0), (4, 3, 5), (4, 0, 5)])
def test_single_negative_voxel_at_a_volume_corner(gf, corner):
    """The gradient's indices clamp on all three axes at the voxel itself."""
    t = np.full((5, 4, 6), 0.7, np.float32)
    t[corner] = -0.3
    vol, t, c = _loaded(gf, t)
    v, n, col, f, k = _check_exact(vol, t, c)
    assert len(v) == 3 and len(f) == 1


# ---- switches and repeats -------------------------------------------------------------------------
def test_extract_mesh_switches(all_cases):
    vol = all_cases[0]
    full = vol.extract_mesh(keys=True)
    assert np.all(np.diff(full[4]) > 0)
    for i, name in ((1, "normals"), (2, "colors"), (3, "faces")):
        got = vol.extract_mesh(keys=True, **{name: False})
        assert got[i] is None
        for j in range(5):
            assert j == i or np.array_equal(got[j], full[j]), (name, j)
    assert len(vol.extract_mesh()) == 4
    pc = vol.get_point_cloud()
    assert pc.dtype == np.float32 and np.array_equal(pc, np.hstack([full[0], full[2]]))
    verts, faces, norms, cols = vol.get_mesh()
    assert np.array_equal(verts, full[0]) and np.array_equal(faces, full[3])
    assert np.array_equal(norms, full[1]) and np.array_equal(cols, full[2])


def test_extract_again_after_the_state_shrank(gf):
    """A second extraction from the same handle holds nothing of the first (Mesh::release)."""
    vol, t, c = _loaded(gf, M.random_field(1))
    big = _check_exact(vol, t, c)
    t2 = np.full(t.shape, 0.5, np.float32)
    t2[7:10, 5:8, 9:12] = -0.25
    c2 = _colors(t.shape, seed=12)
    vol.set_state(t2, np.ones(t.shape, np.float32), c2)
    small = _check_exact(vol, t2, c2)
    assert 0 < len(small[0]) < len(big[0]) // 10 and 0 < len(small[3]) < len(big[3]) // 10
    vol.set_state(t, np.ones(t.shape, np.float32), c)
    again = _check_exact(vol, t, c)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)


def test_hash_mesh_of_all_256_cases_equals_oracle(gf):
    """A table filled voxel by voxel (add_entries, weight 1) with the all-cases field: get_mesh()
    is the oracle's mesh of the table's own get_state()."""
    from tsdf_amd import hash_fusion
    t0 = M.random_field(0)
    c0 = _colors(t0.shape)
    ht = hash_fusion.HashTable(_bounds(t0.shape), VS, 1 << 10)
    assert tuple(int(d) for d in ht._vol_dim) == t0.shape
    pos = np.stack(np.unravel_index(np.arange(t0.size), t0.shape), 1)
    ht.add_entries(pos, tsdf=t0.reshape(-1), weight=np.ones(t0.size, np.float32), color=c0.reshape(-1))
    t, w, c = ht.get_state()
    assert np.array_equal(w, np.ones_like(w)) and len(np.unique(M.cell_cases(t))) == 256
    assert np.array_equal(c, c0) and np.abs(t - t0).max() <= 1e-4
    v, f, n, col = ht.get_mesh()
    rv, rn, rc, rf = mc_oracle.extract(t, c, ht._vol_origin, ht._voxel_size)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)) and np.array_equal(f, rf)
    assert np.array_equal(col, rc) and np.abs(n - rn).max() <= 1e-6
    M.check_manifold(f, M.edge_keys(t), t.shape)
    pc = ht.get_point_cloud()
    assert np.array_equal(pc, np.hstack([v, col]))
