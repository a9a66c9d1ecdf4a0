"""States for the voxel hash's mesher (tsdf_hash_extract_mesh) shared by its CPU and GPU tests: a
volume whose blocks are partly absent and whose live blocks have voxels without an entry, so that
vertices and cells are anchored in absent blocks and gradients reach across them."""
import numpy as np

import mesh_checks as M

HOLES_SHAPE = (29, 19, 37)  # 4 x 3 x 5 blocks, ragged on every axis


def holes_state(seed, shape=HOLES_SHAPE):
    """(tsdf, colour, entry mask, live-block mask): the volume a table holds after add_entries of
    the masked voxels -- tsdf 1 and colour 0 where there is no entry.  About 45 % of the blocks
    are live (the first and the last always, block (1, 1, 1) never), 85 % of their voxels have an
    entry."""
    rng = np.random.default_rng(seed)
    nb = tuple((s + 7) // 8 for s in shape)
    live = rng.random(nb) < 0.45
    live[0, 0, 0] = live[-1, -1, -1] = True
    live[1, 1, 1] = False
    f = rng.uniform(-1, 1, size=shape).astype(np.float32)
    col = rng.integers(0, 1 << 24, size=shape).astype(np.float32)
    lv = np.repeat(np.repeat(np.repeat(live, 8, 0), 8, 1), 8, 2)[:shape[0], :shape[1], :shape[2]]
    ent = lv & (rng.random(shape) < 0.85)
    t = np.where(ent, f, np.float32(1.0)).astype(np.float32)
    c = np.where(ent, col, np.float32(0.0)).astype(np.float32)
    return t, c, ent, live


def anchored_in_absent_blocks(t, live):
    """(vertices, surface cells) whose anchor voxel lies in a block that is not live."""
    shape = t.shape
    vox = M.edge_keys(t) // 3
    idx = np.stack(np.unravel_index(vox, shape), 1)
    n_verts = int((~live[idx[:, 0] >> 3, idx[:, 1] >> 3, idx[:, 2] >> 3]).sum())
    cases = M.cell_cases(t)
    cx, cy, cz = np.nonzero((cases != 0) & (cases != 255))
    n_cells = int((~live[cx >> 3, cy >> 3, cz >> 3]).sum())
    return n_verts, n_cells


def entries(t, c, ent):
    """(positions (n, 3), tsdf, weight, colour) of the entries, for add_entries."""
    pos = np.stack(np.nonzero(ent), 1)
    return pos, t[ent], np.ones(len(pos), np.float32), c[ent]


def blocks_of(t, c, ent):
    """The state's blocks that hold an entry, as import_blocks takes them: (bxyz (n, 3) int32, tsdf,
    weight, colour (n, 512) float32 in brick-local order, occ (n, 8) uint64: word z, bit x*8 + y).
    The shape must be whole blocks."""
    nb = tuple(s // 8 for s in t.shape)
    assert all(s % 8 == 0 for s in t.shape)

    def split(a):  # (nbx, nby, nbz, 8, 8, 8)
        return a.reshape(nb[0], 8, nb[1], 8, nb[2], 8).transpose(0, 2, 4, 1, 3, 5)
    T, C, E = split(t), split(c), split(ent)
    any_ = E.reshape(nb + (-1,)).any(-1)
    bxyz = np.stack(np.nonzero(any_), 1).astype(np.int32)
    sel = tuple(bxyz.T)
    bits = (np.uint64(1) << (np.arange(8, dtype=np.uint64)[:, None] * np.uint64(8) +
                             np.arange(8, dtype=np.uint64)[None, :]))  # [x][y]
    occ = (E[sel].astype(np.uint64) * bits[None, :, :, None]).sum(axis=(1, 2), dtype=np.uint64)  # (n, z)
    n = len(bxyz)
    return (bxyz, T[sel].reshape(n, 512).copy(), np.ones((n, 512), np.float32), C[sel].reshape(n, 512).copy(),
            np.ascontiguousarray(occ))
