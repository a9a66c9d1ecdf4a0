"""CPU-side checks for the voxel hash's mesher: its C-ABI exists and is typed, and the "holes"
state its GPU test meshes really exercises what that test is for (every case, vertices and cells
anchored in absent blocks, a manifold oracle mesh), so the GPU test cannot lose its coverage
silently."""
import numpy as np

import hash_mesh_cases as H
import mc_oracle
import mesh_checks as M

SYMBOLS = ("tsdf_hash_extract_mesh", "tsdf_hash_get_mesh", "tsdf_hash_get_mesh_keys", "tsdf_hash_mesh_info")


def test_library_exports_and_types_the_hash_mesh_calls():
    from tsdf_amd import _ffi
    lib = _ffi.load()
    for name in SYMBOLS + ("tsdf_hash_extract_mesh_fields",):
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    assert len(_ffi.SIGNATURES["tsdf_hash_extract_mesh"]) == 3
    assert len(_ffi.SIGNATURES["tsdf_hash_get_mesh"]) == 5
    assert [k for k, _ in _ffi.HashMeshInfo._fields_][:3] == ["live_blocks", "mesh_blocks", "scratch_bytes"]


def test_holes_state_covers_what_the_gpu_test_is_for():
    t, c, ent, live = H.holes_state(0)
    assert t.shape == H.HOLES_SHAPE and live.shape == (4, 3, 5)
    assert live[0, 0, 0] and live[-1, -1, -1] and not live[1, 1, 1]
    assert np.all(t[~ent] == 1.0) and np.all(c[~ent] == 0.0)
    assert len(np.unique(M.cell_cases(t))) == 256
    n_verts, n_cells = H.anchored_in_absent_blocks(t, live)
    assert n_verts >= 100 and n_cells >= 100
    v, n, col, f = mc_oracle.extract(t, c, np.array([-0.37, 0.21, 1.03], np.float32), 0.01)
    assert not np.isnan(n).any()
    M.check_manifold(f, M.edge_keys(t), t.shape)


def test_blocks_of_restates_the_state():
    """The block form the extent test imports is the same state as the voxel form."""
    t, c, ent, _ = H.holes_state(5, (32, 24, 40))
    bxyz, bt, bw, bc, occ = H.blocks_of(t, c, ent)
    t2 = np.ones_like(t)
    c2 = np.zeros_like(c)
    for b, tt, cc, oo in zip(bxyz, bt, bc, occ):
        for z in range(8):
            for bit in range(64):
                if (int(oo[z]) >> bit) & 1:
                    x, y = bit >> 3, bit & 7
                    p = (b[0] * 8 + x, b[1] * 8 + y, b[2] * 8 + z)
                    t2[p] = tt[(x * 8 + y) * 8 + z]
                    c2[p] = cc[(x * 8 + y) * 8 + z]
    assert np.array_equal(t2, t) and np.array_equal(c2, c)
    assert int(sum(bin(int(w)).count("1") for w in occ.reshape(-1))) == int(ent.sum())
