"""The voxel hash's own marching cubes (tsdf_hash_extract_mesh: over the table's live blocks, no
dense volume) against its two oracles: oracle/mc_oracle.py on the table's get_state() -- vertices,
colours, faces and keys to the bit, normals within 1e-6 as for the dense mesher -- and the dense
mesher on the densified table (_as_grid()), which it must equal byte for byte in all five arrays,
normals included, since both compile the same expressions."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import hash_mesh_cases as H
import mc_oracle
import mesh_checks as M

pytestmark = pytest.mark.gpu
ORIGIN = (-0.37, 0.21, 1.03)
VS = 0.01
C1 = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]


def _bounds(shape, origin=ORIGIN, vs=VS):
    lo = np.array(origin, float)
    return np.stack([lo, lo + (np.array(shape) - 0.5) * vs], axis=1)  # ceil(extent / vs) == shape


def _table(shape, map_size=1 << 10, **kw):
    from tsdf_amd import hash_fusion
    ht = hash_fusion.HashTable(_bounds(shape), VS, map_size, **kw)
    assert tuple(int(d) for d in ht._vol_dim) == tuple(shape)
    return ht


def _same_bytes(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, i
        assert x.tobytes() == y.tobytes(), "array %d differs" % i


def _check_both(ht, manifold=True):
    """extract_mesh(keys=True) of the table against the oracle's mesh of get_state() and against the
    dense mesher on the densified table."""
    got = ht.extract_mesh(keys=True)
    v, n, col, f, k = got
    t, _, c = ht.get_state()
    rv, rn, rc, rf = mc_oracle.extract(t, c, ht._vol_origin, ht._voxel_size)
    assert v.shape == rv.shape == n.shape == col.shape and f.shape == rf.shape
    assert v.dtype == n.dtype == np.float32 and col.dtype == np.uint8 and f.dtype == np.int32 and k.dtype == np.int64
    assert np.array_equal(k, M.edge_keys(t))
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(col, rc) and np.array_equal(f, rf)
    print("normals: max |gpu - oracle| = %d ulp over %d vertices" % (M.ulp_diff(n, rn), len(n)))
    assert not np.isnan(n).any()
    assert np.abs(n - rn).max(initial=0) <= 1e-6
    _same_bytes(got, ht._as_grid().extract_mesh(keys=True))
    if manifold:
        M.check_manifold(f, k, t.shape, all_referenced=min(t.shape) > 1)
    return got, t


def test_all_cases_full_table():
    t0 = M.random_field(0)
    c0 = np.random.default_rng(11).integers(0, 1 << 24, size=t0.shape).astype(np.float32)
    ht = _table(t0.shape)
    pos = np.stack(np.unravel_index(np.arange(t0.size), t0.shape), 1)
    ht.add_entries(pos, tsdf=t0.reshape(-1), weight=np.ones(t0.size, np.float32), color=c0.reshape(-1))
    (v, n, col, f, k), t = _check_both(ht)
    assert len(np.unique(M.cell_cases(t))) == 256 and len(f) > 4000
    info = ht.mesh_info()
    assert info["live_blocks"] == info["mesh_blocks"] == 3 * 2 * 3
    assert info["n_verts"] == len(v) and info["n_tris"] == len(f)


def test_holes():
    """Absent blocks, voxels without an entry in live blocks, removed entries, a live block emptied
    entry by entry and an entry of weight 0: cells and vertices anchored in absent blocks, gradients
    across them."""
    t0, c0, ent, live = H.holes_state(0)
    ht = _table(t0.shape)
    ht.add_entries(*H.entries(t0, c0, ent))
    some = np.stack(np.nonzero(ent), 1)[::97]
    assert ht.remove_entries(some).all()
    bx, by, bz = np.argwhere(live)[3]
    blk = np.stack(np.nonzero(ent[bx * 8:bx * 8 + 8, by * 8:by * 8 + 8, bz * 8:bz * 8 + 8]), 1) + 8 * np.array([bx, by, bz])
    ht.remove_entries(blk)
    free = np.argwhere(~ent & np.repeat(np.repeat(np.repeat(live, 8, 0), 8, 1), 8, 2)[:29, :19, :37])[5]
    ht.add_entries(free[None], tsdf=[-0.5], weight=[0.0], color=[258.0])
    (v, n, col, f, k), t = _check_both(ht)
    assert t[tuple(free)] == -0.5 and np.all(t[tuple(blk.T)] == 1.0)
    n_verts, n_cells = H.anchored_in_absent_blocks(t, live)
    assert n_verts >= 100 and n_cells >= 100
    info = ht.mesh_info()
    assert info["live_blocks"] <= info["mesh_blocks"] <= 8 * info["live_blocks"]


@pytest.mark.parametrize("corner", [(0, 0, 0), (4, 3, 5), (4, 0, 5)])
def test_single_negative_entry_at_a_ragged_corner(corner):
    ht = _table((5, 4, 6))
    ht.add_entries([corner], tsdf=[-0.3], weight=[1.0], color=[197121.0])
    (v, n, col, f, k), t = _check_both(ht)
    assert len(v) == 3 and len(f) == 1


def test_empty_table_and_switches():
    ht = _table(H.HOLES_SHAPE)
    v, n, col, f, k = ht.extract_mesh(keys=True)
    assert v.shape == n.shape == col.shape == f.shape == (0, 3) and k.shape == (0,)
    assert ht.get_point_cloud().shape == (0, 6)
    t0, c0, ent, _ = H.holes_state(1)
    ht.add_entries(*H.entries(t0, c0, ent))
    full = ht.extract_mesh(keys=True)
    assert len(full[0]) > 1000 and np.all(np.diff(full[4]) > 0)
    for i, name in ((1, "normals"), (2, "colors"), (3, "faces")):
        got = ht.extract_mesh(keys=True, **{name: False})
        assert got[i] is None
        for j in range(5):
            assert j == i or got[j].tobytes() == full[j].tobytes(), (name, j)
    assert len(ht.extract_mesh()) == 4
    pc = ht.get_point_cloud()
    assert pc.dtype == np.float32 and np.array_equal(pc, np.hstack([full[0], full[2]]))
    verts, faces, norms, cols = ht.get_mesh()  # the reference's order
    _same_bytes((verts, norms, cols, faces), full[:4])
    # a second extraction after the surface shrank holds nothing of the first
    keep = np.zeros_like(ent)
    keep[7:10, 5:8, 9:12] = True
    ht.remove_entries(np.stack(np.nonzero(ent & ~keep), 1))
    (v, n, col, f, k), t = _check_both(ht, manifold=False)
    assert len(v) < len(full[0]) // 10 and len(f) < len(full[3]) // 10
    ht.reset()
    assert ht.extract_mesh()[0].shape == (0, 3)


def test_after_integration():
    from tsdf_amd import hash_fusion
    K = lounge_intrinsics()
    ht = hash_fusion.HashTable(np.array(C1), 0.04, 1 << 16)
    for i in range(2):
        _, depth, rgb, pose = load_lounge(i)
        ht.integrate(rgb, depth, K, pose)
    got = ht.extract_mesh(keys=True)  # (runs the deferred frames first)
    _same_bytes(got, ht._as_grid().extract_mesh(keys=True))
    assert len(got[3]) > 10000


def test_extent_independence_at_1024_cubed():
    """The same blocks far inside a 1024^3 extent and in a table just larger than them: the same
    mesh up to the index offset, with scratch that follows the blocks, not the extent."""
    from tsdf_amd import hash_fusion
    t0, c0, ent, _ = H.holes_state(7, (32, 24, 40))
    bxyz, bt, bw, bc, occ = H.blocks_of(t0, c0, ent)
    far = hash_fusion.HashTable(np.array([[0.0, 10.24]] * 3), VS, 1 << 12, max_blocks=64)
    assert tuple(int(x) for x in far._vol_dim) == (1024, 1024, 1024)
    near = hash_fusion.HashTable(np.array([[0.0, 0.475], [0.0, 0.395], [0.0, 0.555]]), VS, 1 << 12, max_blocks=64)
    assert tuple(int(x) for x in near._vol_dim) == (48, 40, 56)
    far.import_blocks(bxyz + np.array([97, 61, 113], np.int32), bt, bw, bc, occ)
    near.import_blocks(bxyz + np.array([1, 1, 1], np.int32), bt, bw, bc, occ)
    fv, fn, fc, ff, fk = far.extract_mesh(keys=True)
    nv, nn, nc, nf, nk = near.extract_mesh(keys=True)
    info = far.mesh_info()
    assert len(fv) == len(nv) > 1000 and len(ff) == len(nf) > 1000
    _same_bytes((fn, fc, ff), (nn, nc, nf))
    off = np.array([768, 480, 896])
    vox, axis = np.divmod(nk, 3)
    idx = np.stack(np.unravel_index(vox, (48, 40, 56)), 1) + off
    assert np.array_equal(fk, np.ravel_multi_index(tuple(idx.T), (1024,) * 3) * 3 + axis)
    # the contract's vertex formula in float32, from the table's own entries
    end = idx.copy()
    end[np.arange(len(end)), axis] += 1
    f1, v1, _, _ = far.lookup(idx)
    f2, v2, _, _ = far.lookup(end)
    v1 = np.where(f1, v1, np.float32(1.0)).astype(np.float32)
    v2 = np.where(f2, v2, np.float32(1.0)).astype(np.float32)
    tt = (np.float32(0.0) - v1) / (v2 - v1)
    p = idx.astype(np.float32)
    p[np.arange(len(p)), axis] += tt
    want = p * np.float32(far._voxel_size) + np.asarray(far._vol_origin, np.float32)
    assert want.dtype == np.float32 and fv.tobytes() == want.tobytes()
    assert info["live_blocks"] == len(bxyz)
    assert info["live_blocks"] <= info["mesh_blocks"] <= 8 * info["live_blocks"]
    assert info["scratch_bytes"] <= (64 << 10) * info["mesh_blocks"] + (16 << 20)
