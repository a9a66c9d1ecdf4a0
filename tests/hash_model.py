"""A voxel model of the hash's entry API and block transfer (test_hash_model_cpu.py,
test_hash_model_gpu.py): tsdf_hash_insert / remove / lookup / resize / export_blocks /
import_blocks / reset / trim restated on plain arrays, and the two scenes the tests run.  Plain
functions and one small class; everything here runs on the CPU.

The model of a table is an oracle.OracleTSDFVolume (f32 state, the state the pixel and update-path
tests already hold the hash to bit for bit) plus a boolean `entry` array of the same shape.  A
voxel without an entry holds (1, 0, 0): a removed voxel keeps no state, like the reference's table,
which finds no entry after a remove and starts from a fresh Voxel() (hash_fusion.py:138-143).

The model keeps no keys.  On the device a block is keyed while it holds an entry; a block imported
with no entry at all stays keyed too, until a remove names one of its voxels (the callers of
blocks() that import such blocks add them).
"""
import functools

import numpy as np

import oracle as O

DEFAULT = (1.0, 0.0, 0.0)  # (tsdf, weight, colour) of a voxel without an entry


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _ijk(p):
    return np.asarray(p, dtype=np.int64).reshape(-1, 3)


class HashModel:
    def __init__(self, bounds, voxel_size):
        self.vol = O.OracleTSDFVolume(np.array(bounds, dtype=np.float64), voxel_size)
        self.dims = tuple(int(d) for d in self.vol._vol_dim)
        assert all(d % 8 == 0 for d in self.dims)
        self.nb = tuple(d // 8 for d in self.dims)
        self.entry = np.zeros(self.dims, bool)

    @property
    def fields(self):
        return self.vol._tsdf_vol_cpu, self.vol._weight_vol_cpu, self.vol._color_vol_cpu

    def state(self):
        """What get_state() gives: the fields, (1, 0, 0) where there is no entry."""
        return tuple(np.where(self.entry, a, np.float32(d)) for a, d in zip(self.fields, DEFAULT))

    def copy(self):
        m = HashModel(self.vol._vol_bnds, self.vol._voxel_size)
        assert m.dims == self.dims
        m.vol._tsdf_vol_cpu[:], m.vol._weight_vol_cpu[:], m.vol._color_vol_cpu[:] = self.fields
        m.entry[:] = self.entry
        return m

    # -------------------------------------------------------------------------------- entries
    def insert(self, ijk, tsdf=None, weight=None, color=None):
        """The entry is set; a given field is written; a field not given stays for an existing
        entry and is the default for a new one (which it already holds)."""
        i = tuple(_ijk(ijk).T)
        self.entry[i] = True
        for a, val in zip(self.fields, (tsdf, weight, color)):
            if val is not None:
                a[i] = np.asarray(val, np.float32).reshape(-1)

    def remove(self, ijk):
        """The entry bit from before the call per voxel (of a voxel listed twice, the first
        reports it); the voxel goes back to (1, 0, 0)."""
        p = _ijk(ijk)
        i = tuple(p.T)
        lin = np.ravel_multi_index(i, self.dims)
        first = np.zeros(len(p), bool)
        first[np.unique(lin, return_index=True)[1]] = True
        removed = self.entry[i] & first
        self.entry[i] = False
        for a, d in zip(self.fields, DEFAULT):
            a[i] = d
        return removed

    def lookup(self, ijk):
        i = tuple(_ijk(ijk).T)
        f = self.entry[i]
        return (f,) + tuple(np.where(f, a[i], np.float32(d)) for a, d in zip(self.fields, DEFAULT))

    def integrate(self, rgb, depth_m, K, pose):
        """One frame through the oracle; the voxels it updates get entries.  Returns their number."""
        n = self.vol.integrate(rgb, depth_m, K, pose, want_mask=True)
        self.entry |= self.vol.last_updated.reshape(self.dims).astype(bool)
        return n

    def entries(self):
        return int(self.entry.sum())

    # -------------------------------------------------------------------------------- blocks
    def _by_block(self, a):
        """(X, Y, Z) as (nbx, nby, nbz, 8, 8, 8): block coordinates, then x, y, z inside the block."""
        nx, ny, nz = self.nb
        return a.reshape(nx, 8, ny, 8, nz, 8).transpose(0, 2, 4, 1, 3, 5)

    def blocks(self):
        """(n, 3) int32 coordinates of the 8^3 blocks with at least one entry, in C order."""
        return np.argwhere(self._by_block(self.entry).any((-1, -2, -3))).astype(np.int32)

    def export(self):
        """(bxyz, tsdf, weight, colour, occ) of blocks(): 512 values per field in the order
        (x*8 + y)*8 + z and 8 entry words per block (word z, bit x*8 + y)."""
        b = self.blocks()
        i = tuple(b.T.astype(np.int64))
        out = [np.ascontiguousarray(self._by_block(a)[i]).reshape(len(b), 512) for a in self.state()]
        bits = self._by_block(self.entry)[i].reshape(len(b), 64, 8)  # [block, x*8+y, z]
        occ = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :, None]).sum(1, dtype=np.uint64)
        return (b, *out, occ)

    def import_(self, bxyz, t, w, c, occ=None):
        """tsdf_hash_import_blocks: each block's entry words are replaced (None: every voxel has an
        entry); a given field is written, a field not given stays; a clear bit means absent, which
        is (1, 0, 0) in every field."""
        b = np.asarray(bxyz, np.int64).reshape(-1, 3)
        assert len(np.unique(b, axis=0)) == len(b)
        i = tuple(b.T)
        n = len(b)
        if occ is None:
            bits = np.ones((n, 8, 8, 8), bool)
        else:
            words = np.asarray(occ, np.uint64).reshape(n, 1, 8)  # [block, bit x*8+y, word z]
            bits = ((words >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)).astype(bool)
            bits = bits.reshape(n, 8, 8, 8)
        self._by_block(self.entry)[i] = bits
        for a, val, d in zip(self.fields, (t, w, c), DEFAULT):
            cur = self._by_block(a)[i] if val is None else np.asarray(val, np.float32).reshape(n, 8, 8, 8)
            self._by_block(a)[i] = np.where(bits, cur, np.float32(d))

    def reset(self):
        self.entry[:] = False
        for a, d in zip(self.fields, DEFAULT):
            a[:] = d

    def resize(self, new_capacity=None):
        """double_table_size changes no voxel."""

    def trim(self):
        """Handing pool memory back changes no voxel."""


def probe_slots(keys_home, S, occupied=None):
    """Sequential linear-probe insertion of keys with the given home slots into S slots: each takes
    the first free slot at or after its home (wrapping); `occupied` marks the slots that hold a
    live key, so a tombstone counts as free.  Returns the slot of each key in the order given; as
    a set, the slots filled do not depend on that order."""
    occ = np.zeros(S, bool) if occupied is None else np.array(occupied, bool)
    assert occ.shape == (S,)
    out = np.empty(len(keys_home), np.int64)
    for k, h in enumerate(np.asarray(keys_home, np.int64)):
        s = int(h)
        for _ in range(S):
            if not occ[s]:
                break
            s = s + 1 if s + 1 < S else 0
        else:
            raise ValueError("table full")
        occ[s] = True
        out[k] = s
    return out


def removal_rule(pos):
    """Indices into `pos` (entry voxels (n, 3) in C order) of the removal set: every third entry
    voxel, plus every entry of every fifth block that holds entries (blocks in C order)."""
    pos = np.asarray(pos, np.int64)
    blk, inv = np.unique(pos // 8, axis=0, return_inverse=True)  # (sorted rows = C order)
    take = np.zeros(len(pos), bool)
    take[::3] = True
    fifth = np.zeros(len(blk), bool)
    fifth[::5] = True
    take |= fifth[inv.reshape(-1)]
    return np.flatnonzero(take)


# ------------------------------------------------------------------------------------ scene A
A_VS, A_N = 0.04, 64
A_CASE = "camera-inside"
KINDS = ("canonical", "mixed")
N_HAND = 300   # voxels the `mixed` kind inserts by hand before frame 0


def a_bounds():
    return np.array([[0.0, A_N * A_VS]] * 3)


def a_frames():
    """(depth u16 mm (8, 480, 640), rgb, K, poses) of scene A."""
    import pixel_fixed_cases as P
    d, rgb, K, poses, inv = P.case(A_CASE)
    assert not inv and len(d) == 8
    return d, rgb, K, poses


def run_frames(m, frames):
    """Scene A's frames through the model; returns the voxel updates."""
    d, rgb, K, poses = a_frames()
    return sum(m.integrate(rgb[f], d[f].astype(float) / 1000.0, K, poses[f]) for f in frames)


@functools.lru_cache(maxsize=None)
def hand_voxels():
    """What the `mixed` kind inserts before frame 0: N_HAND voxels that the canonical run removes or
    keeps after frame 3 and that frames 4-7 update, with a non-integer weight, an odd colour
    (update_paths.ODD) and a tsdf of their own -- Vol::canon is off from the first launch on."""
    import update_paths as U
    a = scene_a("canonical")
    lin = np.flatnonzero(a["late_mask"].reshape(-1))
    lin = lin[:: max(1, len(lin) // N_HAND)][:N_HAND]
    ijk = np.stack(np.unravel_index(lin, (A_N,) * 3), 1)
    rng = np.random.default_rng(5)
    k = np.arange(len(ijk))
    return (ijk, rng.uniform(-1, 1, len(ijk)).astype(np.float32), (1.5 + (k % 3)).astype(np.float32),
            U.ODD[k % len(U.ODD)].astype(np.float32))


@functools.lru_cache(maxsize=None)
def scene_a(kind="canonical"):
    """Scene A on the model: frames 0-3, the removal, frames 4-7.  A dict of
      hand       (ijk, t, w, c) inserted before frame 0 (None for `canonical`)
      mid        the model after frame 3 (before the removal)
      removal    (n, 3) voxels removed, in C order, no duplicates
      after      the model after the removal
      final      the model after frames 4-7
      updates    (voxel updates of frames 0-3, of frames 4-7)
      late_mask  voxels frames 4-7 update
    and the counts the tests' conditions rest on (test_hash_model_cpu.py)."""
    m = HashModel(a_bounds(), A_VS)
    hand = None
    if kind == "mixed":
        hand = hand_voxels()
        m.insert(*hand)
    n0 = run_frames(m, range(4))
    mid = m.copy()
    pos = np.argwhere(m.entry)
    removal = pos[removal_rule(pos)]
    if hand is not None:  # the hand-inserted voxels leave the rule's set; every second one goes back in
        hl = set(map(tuple, hand[0]))
        removal = np.array([p for p in map(tuple, removal) if p not in hl] + [tuple(p) for p in hand[0][::2]])
        removal = removal[np.lexsort((removal[:, 2], removal[:, 1], removal[:, 0]))]
    blocks_before = mid.blocks()
    removed = m.remove(removal)
    assert removed.all()
    after = m.copy()
    late = np.zeros(m.dims, bool)
    d, rgb, K, poses = a_frames()
    n1 = 0
    for f in range(4, 8):
        n1 += m.integrate(rgb[f], d[f].astype(float) / 1000.0, K, poses[f])
        late |= m.vol.last_updated.reshape(m.dims).astype(bool)
    # the conditions
    blocks_after = after.blocks()
    alive = np.zeros(m.nb, bool)
    alive[tuple(blocks_after.T)] = True
    r = tuple(removal.T)
    again = late[r]                                   # removed voxels that frames 4-7 update again
    in_live = alive[tuple((removal // 8).T)]          # ... whose block stayed live
    third_only = pos[::3]
    left = mid.entry.copy()
    left[tuple(third_only.T)] = False
    by_third = mid._by_block(mid.entry).any((-1, -2, -3)) & ~mid._by_block(left).any((-1, -2, -3))
    nblk = len(blocks_before)
    whole = int((~alive[tuple(blocks_before[::5].T)]).sum())  # every fifth block, gone with all its entries
    return dict(hand=hand, mid=mid, removal=removal, after=after, final=m, updates=(n0, n1), late_mask=late,
                entries_mid=mid.entries(), blocks_mid=nblk, n_removed=len(removal),
                blocks_after=len(blocks_after), whole_blocks=whole,
                blocks_emptied_by_third=int(by_third.sum()), again=int(again.sum()),
                again_live=int((again & in_live).sum()),
                again_live_voxels=removal[again & in_live],
                old_weights=np.unique(mid.fields[1][r][again & in_live]))


# ------------------------------------------------------------------------------------ scene B
B_VS, B_N, B_MAP = 0.02, 512, 4096


def b_bounds():
    return np.array([[0.0, B_N * B_VS]] * 3)


@functools.lru_cache(maxsize=None)
def scene_b(int_bits=64):
    """The densest probe cluster of a 64^3-block volume in a 4096-slot table: the four adjacent
    home slots with the most block keys.  dict(start, homes (4,), blocks (n, 3) in C order, home
    (n,) of each, per_slot (4096,) keys per home slot, near_blocks / near_home: the blocks of the
    four home slots below and the four above the cluster)."""
    nb = B_N // 8
    b = np.indices((nb, nb, nb)).reshape(3, -1).T.astype(np.int64)
    h = O.hash_keys(b, B_MAP, int_bits)
    per = np.bincount(h, minlength=B_MAP)
    four = per + np.roll(per, -1) + np.roll(per, -2) + np.roll(per, -3)
    start = int(np.argmax(four))
    assert start + 3 < B_MAP
    sel = (h >= start) & (h < start + 4)
    near = ((h >= start - 4) & (h < start)) | ((h >= start + 4) & (h < start + 8))  # the neighbouring home slots
    return dict(start=start, homes=np.arange(start, start + 4), blocks=b[sel], home=h[sel], per_slot=per,
                near_blocks=b[near], near_home=h[near])


# ------------------------------------------------------------------------------------ C1 fixture
C1 = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]
C1_VS = 0.04


def c1_removal(gold_dir):
    """The removal set of tests/golden/hash_c1_remove.npz: removal_rule over hash_c1.npz's f0_pos."""
    import os
    pos = np.load(os.path.join(gold_dir, "hash_c1.npz"))["f0_pos"]
    idx = removal_rule(pos)
    return idx, pos[idx]
