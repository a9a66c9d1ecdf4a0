"""The voxel hash's entry API and block transfer on the GPU against the voxel model of
tests/hash_model.py: tsdf_hash_insert / remove / lookup / resize / export_blocks / import_blocks /
reset / trim and their kernels (k_insert_blocks, k_set_voxels, k_remove_voxels, k_free_empty,
k_rehash, k_export_blocks, k_write_blocks), in sequences with integrate, bit for bit.

What the sequences pin: a voxel without an entry holds (1, 0, 0) in the pool (Table::occ), because
integrate_brick and k_set_voxels read the pool without looking at the entry bit.  Before
k_remove_voxels and k_write_blocks restored the values under the bits they clear, a removed voxel
of a block that stayed live blended the next observation into its old weight, tsdf and colour, and
an insert without values brought the old values back.  Measured on the library from before that
fix: all 1 200 such voxels of scene A (1 761 in its `mixed` kind) ended with a wrong weight and
colour, 967 (1 460) with a wrong tsdf; 250 of 250 re-inserted voxels came back with old values; all
67 237 imported voxels under a clear bit kept the caller's garbage; 13 279 of the 22 621 voxels the
reference's run removes and sees again in lounge frame 1 had a weight other than the reference's 1.
test_one_probe_cluster failed there too: its second insert call ran out of probe steps in the run of
tombstones (TSDF_E_CAPACITY, see k_insert_blocks).

Every test here calls the HIP path through the C-ABI (tsdf_amd -> libtsdf_hip.so).
"""
import os

import numpy as np
import pytest

from conftest import GOLD, load_lounge, lounge_intrinsics
import oracle as O
import hash_model as M

pytestmark = pytest.mark.gpu

PATHS = ("fused", "inline", "deferred")  # k_fused_hash, TSDF_PIPELINE=0, per-frame ht.integrate
FIELDS = ("tsdf", "weight", "colour")


@pytest.fixture(scope="module")
def hf():
    from tsdf_amd import hash_fusion
    return hash_fusion


def table_a(hf, monkeypatch, path="fused"):
    for k in ("TSDF_PIPELINE", "TSDF_BATCH", "TSDF_TEXEL", "TSDF_DEFER_FRAMES", "TSDF_HASH_MAX_LOAD"):
        monkeypatch.delenv(k, raising=False)
    if path == "inline":
        monkeypatch.setenv("TSDF_PIPELINE", "0")
    return hf.HashTable(M.a_bounds(), M.A_VS, 1 << 14)


def feed(ht, path, lo, hi):
    """Frames lo .. hi-1 of scene A: one call, or one deferred call per frame (they stay pending
    until another call on the handle, 8 frames at the most)."""
    d, rgb, K, poses = M.a_frames()
    if path == "deferred":
        for f in range(lo, hi):
            ht.integrate(rgb[f], d[f], K, poses[f])
    else:
        ht.integrate_batch(d[lo:hi], rgb[lo:hi], K, np.linalg.inv(poses[lo:hi]))


def differing(got, exp):
    """Voxels per field whose bits differ."""
    return {n: int((np.asarray(g, np.float32).view(np.uint32) != np.asarray(e, np.float32).view(np.uint32)).sum())
            for n, g, e in zip(FIELDS, got, exp)}


NONE = dict.fromkeys(FIELDS, 0)


def check_table(ht, model, extra_blocks=None):
    """State, entries and live blocks of the table against the model."""
    assert differing(ht.get_state(), model.state()) == NONE
    info = ht.info()
    blocks = model.blocks()
    if extra_blocks is not None:
        blocks = np.unique(np.concatenate([blocks, np.asarray(extra_blocks, np.int32)]), axis=0)
    assert (info["entries"], info["used"]) == (model.entries(), len(blocks))


def sorted_export(ht):
    """export_blocks() in C order of the block coordinates (the device's order is its claim order)."""
    b, t, w, c, occ = ht.export_blocks()
    o = np.lexsort((b[:, 2], b[:, 1], b[:, 0]))
    return b[o], t[o], w[o], c[o], occ[o]


def present(occ):
    """(n, 8) entry words as (n, 512) booleans in the order (x*8 + y)*8 + z."""
    bits = (occ[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)
    return bits.astype(bool).reshape(len(occ), 512)


# ------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("path", PATHS)
def test_remove_then_integrate_matches_the_model(hf, monkeypatch, path, kind):
    """Scene A: frames 0-3, the removal, frames 4-7.  A removed voxel that frames 4-7 update again
    starts from a fresh voxel, as the reference's does (hash_fusion.py:138-143).  `mixed`: voxels
    inserted by hand with non-integer weights and odd colours keep Vol::canon off.  `deferred`: the
    removal is issued while frames 2-3 are still pending; they land before it."""
    a = M.scene_a(kind)
    ht = table_a(hf, monkeypatch, path)
    if a["hand"] is not None:
        ht.add_entries(*a["hand"])
    if path == "deferred":
        feed(ht, path, 0, 2)
        ht.sync()
        feed(ht, path, 2, 4)
    else:
        feed(ht, path, 0, 4)
    removed = ht.remove_entries(a["removal"])
    assert removed.all() and len(removed) == a["n_removed"]
    check_table(ht, a["after"])
    eb, et, ew, ec, eocc = sorted_export(ht)   # the pool itself: (1, 0, 0) under the cleared bits
    mb, mt, mw, mc, mocc = a["after"].export()
    assert np.array_equal(eb, mb) and np.array_equal(eocc, mocc) and differing((et, ew, ec), (mt, mw, mc)) == NONE
    before = ht.stats()
    assert before["voxel_updates"] == a["updates"][0]
    feed(ht, path, 4, 8)
    got = ht.get_state()
    stale = int((got[1][tuple(a["again_live_voxels"].T)] != a["final"].fields[1][tuple(a["again_live_voxels"].T)]).sum())
    print("removed voxels of live blocks that frames 4-7 update again: %d, with a wrong weight: %d; differing voxels %s"
          % (a["again_live"], stale, differing(got, a["final"].state())))
    assert stale == 0
    check_table(ht, a["final"])
    st = ht.stats()
    assert st["voxel_updates"] - before["voxel_updates"] == a["updates"][1]
    assert st["list_errors"] == 0 and st["bricks_skipped"] == 0
    ht.close()


# ------------------------------------------------------------------------------------ b
def test_readd_after_remove_starts_fresh(hf, monkeypatch):
    """After scene A's removal, 500 removed voxels of surviving blocks are inserted again: without
    values they are found as (1, 0, 0); with a tsdf only, weight and colour are 0; a voxel that
    still has its entry keeps its other fields.  Then frames 4-7, against the model."""
    a = M.scene_a("canonical")
    ht = table_a(hf, monkeypatch)
    feed(ht, "fused", 0, 4)
    assert ht.remove_entries(a["removal"]).all()
    m = a["after"].copy()
    v = a["again_live_voxels"][:500]
    assert len(v) == 500 and not m.entry[tuple(v.T)].any()
    rng = np.random.default_rng(3)
    bare, with_t = v[:250], v[250:]
    kept = np.argwhere(m.entry)[::97][:100]
    tv, tk = rng.uniform(-1, 1, 250).astype(np.float32), rng.uniform(-1, 1, len(kept)).astype(np.float32)
    kept_w, kept_c = m.fields[1][tuple(kept.T)].copy(), m.fields[2][tuple(kept.T)].copy()
    assert len(kept) == 100 and (kept_w >= 1).all()
    for ijk, t in ((bare, None), (with_t, tv), (kept, tk)):
        ht.add_entries(ijk, tsdf=t)
        m.insert(ijk, tsdf=t)
    f, t, w, c = ht.lookup(bare)
    stale = int(((t != 1) | (w != 0) | (c != 0)).sum())
    print("re-inserted without values: %d of %d voxels come back with old values" % (stale, len(bare)))
    assert f.all() and stale == 0
    f, t, w, c = ht.lookup(with_t)
    assert f.all() and M.same(t, tv) and not w.any() and not c.any()
    f, t, w, c = ht.lookup(kept)
    assert f.all() and M.same(t, tk) and M.same(w, kept_w) and M.same(c, kept_c)
    check_table(ht, m)
    feed(ht, "fused", 4, 8)
    M.run_frames(m, range(4, 8))
    check_table(ht, m)
    ht.close()


# ------------------------------------------------------------------------------------ c
def test_block_transfer_under_clear_bits(hf, monkeypatch):
    """Scene A's table after frame 3 is exported; the removal set's bits are cleared in the words on
    the host and garbage (tsdf -0.5, weight 7, colour 12345) is put under every clear bit; a fresh
    table imports that and integrates frames 4-7.  A clear bit means absent: the state equals the
    model's, and what the table exports again holds (1, 0, 0) under every clear bit.  Then an
    import over existing blocks with the weight not given: it stays."""
    a = M.scene_a("canonical")
    src = table_a(hf, monkeypatch)
    feed(src, "fused", 0, 4)
    b, t, w, c, occ = sorted_export(src)
    src.close()
    mb, mt, mw, mc, mocc = a["mid"].export()
    assert np.array_equal(b, mb) and np.array_equal(occ, mocc)
    assert differing((t, w, c), (mt, mw, mc)) == NONE
    # clear the removal set's bits
    r = a["removal"]
    nb = a["mid"].nb
    row = np.searchsorted(np.ravel_multi_index(tuple(b.T.astype(np.int64)), nb), np.ravel_multi_index(tuple((r // 8).T), nb))
    assert np.array_equal(b[row], r // 8)
    occ = occ.copy()
    np.bitwise_and.at(occ, (row, r[:, 2] & 7), ~(np.uint64(1) << ((r[:, 0] & 7) * 8 + (r[:, 1] & 7)).astype(np.uint64)))
    has = present(occ)
    assert int(has.sum()) == a["after"].entries()
    empty = ~has.any(1)   # blocks the removal emptied: imported all the same, they stay keyed
    assert empty.sum() == a["blocks_mid"] - a["blocks_after"]
    t, w, c = (np.where(has, x, np.float32(g)) for x, g in zip((t, w, c), (-0.5, 7.0, 12345.0)))
    dst = table_a(hf, monkeypatch)
    dst.import_blocks(b, t, w, c, occ)
    check_table(dst, a["after"], extra_blocks=b)
    eb, et, ew, ec, eocc = sorted_export(dst)
    ab, at, aw, ac, aocc = a["after"].export()
    assert np.array_equal(eb, b) and np.array_equal(eocc, occ)
    assert np.array_equal(eb[~empty], ab) and np.array_equal(eocc[~empty], aocc)
    at_entries = {n: int((has & (g.view(np.uint32) != x.view(np.uint32))).sum()) for n, g, x in zip(FIELDS, (et, ew, ec), (t, w, c))}
    assert at_entries == NONE
    under_clear = int((~has & ((et != 1) | (ew != 0) | (ec != 0))).sum())
    print("exported voxels under a clear bit that are not (1, 0, 0): %d of %d" % (under_clear, int((~has).sum())))
    assert under_clear == 0
    assert differing((et[~empty], ew[~empty], ec[~empty]), (at, aw, ac)) == NONE
    feed(dst, "fused", 4, 8)
    check_table(dst, a["final"], extra_blocks=b)
    assert dst.stats()["voxel_updates"] == a["updates"][1]
    # over existing blocks, weight not given
    m = a["final"].copy()
    sel = m.blocks()[::40][:3]
    rng = np.random.default_rng(4)
    nocc = rng.integers(0, 1 << 63, (len(sel), 8), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (len(sel), 8), dtype=np.uint64)
    nt = rng.uniform(-1, 1, (len(sel), 512)).astype(np.float32)
    nc = rng.integers(0, 1 << 24, (len(sel), 512)).astype(np.float32)
    dst.import_blocks(sel, nt, None, nc, nocc)
    m.import_(sel, nt, None, nc, nocc)
    assert m.entries() != a["final"].entries()
    check_table(dst, m, extra_blocks=b)
    eb, et, ew, ec, eocc = sorted_export(dst)
    rows = np.flatnonzero((eb[:, None, :] == sel[None, :, :]).all(2).any(1))
    assert np.array_equal(eb[rows], sel) and np.array_equal(eocc[rows], nocc)
    has = present(nocc)
    was = present(a["final"].export()[4][::40][:3])
    fw = a["final"].export()[2][::40][:3]
    assert (has & was).sum() > 100 and M.same(ew[rows][has & was], fw[has & was])        # the weight stayed
    assert not ew[rows][~(has & was)].any()                                              # no entry before or now: 0
    assert M.same(et[rows], np.where(has, nt, np.float32(1))) and M.same(ec[rows], np.where(has, nc, np.float32(0)))
    dst.close()


# ------------------------------------------------------------------------------------ d
class Book:
    """The voxels a table should hold, with their values."""

    def __init__(self):
        self.vox = np.zeros((0, 3), np.int64)
        self.val = np.zeros((0, 3), np.float32)

    def add(self, vox, val):
        self.vox, self.val = np.concatenate([self.vox, vox]), np.concatenate([self.val, val])

    def drop(self, mask):
        gone = self.vox[mask]
        self.vox, self.val = self.vox[~mask], self.val[~mask]
        return gone

    def blocks(self):
        return np.unique(self.vox // 8, axis=0)


def values(rng, n):
    return np.stack([rng.uniform(-1, 1, n), rng.integers(1, 50, n), rng.integers(0, 1 << 24, n)], 1).astype(np.float32)


def check_cluster(ht, book, S, int_bits, tombstones, gone=None):
    """Every voxel of the book is found with its values; voxels of one block share a slot, blocks
    have distinct slots, and the table's counts are what those slots imply.  Returns (blocks in C
    order, their slots).  (An insert of an existing voxel without values finds it: its slot.)"""
    slot, local = ht.add_entries(book.vox)
    v = book.vox
    assert np.array_equal(local, ((v[:, 0] & 7) * 8 + (v[:, 1] & 7)) * 8 + (v[:, 2] & 7))
    blocks, inv = np.unique(v // 8, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    bslot = np.full(len(blocks), -1, np.int64)
    bslot[inv] = slot
    assert np.array_equal(bslot[inv], slot)              # equal for the voxels of one block
    assert len(np.unique(bslot)) == len(blocks)          # distinct across blocks
    assert (bslot >= 0).all() and (bslot < S).all()
    home = O.hash_keys(blocks, S, int_bits)
    dist = (bslot - home) % S
    info = ht.info()
    assert (info["slots"], info["used"], info["entries"], info["tombstones"]) == (S, len(blocks), len(v), tombstones)
    assert (info["displaced"], info["max_probe"]) == (int((dist > 0).sum()), int(dist.max()))
    f, t, w, c = ht.lookup(v)
    assert f.all() and M.same(np.stack([t, w, c], 1), book.val)
    if gone is not None and len(gone):
        assert not ht.lookup(gone)[0].any()
    eb = ht.export_blocks()[0]
    assert len(eb) == len(blocks) and np.array_equal(np.unique(eb, axis=0), blocks.astype(np.int32))  # no duplicate key
    return blocks, bslot


@pytest.mark.parametrize("int_bits", [64, 32])
def test_one_probe_cluster(hf, int_bits):
    """Scene B: 311 block keys whose home slots are the four adjacent slots 2320-2323 of a 4096-slot
    table, inserted by one call: one contiguous run of slots, whatever order the threads won in.
    Then tombstones, their reuse by a second call, a rehash, trim and reset.  The table is never
    densified (512^3); lookup, info and export_blocks only."""
    s = M.scene_b(int_bits)
    S, start, n = M.B_MAP, s["start"], len(s["blocks"])
    ht = hf.HashTable(M.b_bounds(), M.B_VS, S, int_bits=int_bits, max_blocks=1024)
    rng = np.random.default_rng(int_bits)
    book = Book()
    # 1. one voxel of each block and a second one in 50 of them, shuffled, in one call
    at = rng.integers(0, 8, (n, 3))
    twice = np.sort(rng.choice(n, 50, replace=False))
    vox = np.concatenate([s["blocks"] * 8 + at, s["blocks"][twice] * 8 + (at[twice] + rng.integers(1, 4, (50, 3))) % 8])
    vox = vox[rng.permutation(len(vox))]
    val = values(rng, len(vox))
    slot, _ = ht.add_entries(vox, val[:, 0], val[:, 1], val[:, 2])
    book.add(vox, val)
    run = np.arange(start, start + n)
    assert np.array_equal(np.sort(M.probe_slots(s["home"], S)), run)
    assert np.array_equal(np.unique(slot), run)          # as a set, exactly the model's run
    blocks, bslot = check_cluster(ht, book, S, int_bits, 0)
    info = ht.info()
    assert np.array_equal(blocks, s["blocks"]) and info["used"] == n
    # the run implies: slot `start` holds a key at home, the last slot a key 307 to 310 from home
    assert n - 4 <= info["displaced"] <= n - 1 and n - 4 <= info["max_probe"] <= n - 1
    # 2. every voxel of every other block goes: one tombstone per block freed
    freed = s["blocks"][::2]
    in_freed = np.isin(np.ravel_multi_index(tuple((book.vox // 8).T), (64,) * 3), np.ravel_multi_index(tuple(freed.T), (64,) * 3))
    gone = book.vox[in_freed]
    assert ht.remove_entries(gone).all()
    book.drop(in_freed)
    blocks, bslot = check_cluster(ht, book, S, int_bits, len(freed), gone)
    # 3. one voxel three times in one call: one of the three reports it
    _, inv, count = np.unique(book.vox // 8, axis=0, return_inverse=True, return_counts=True)
    two = np.flatnonzero(count[inv.reshape(-1)] == 2)   # voxels of blocks that hold two: the block stays
    assert len(two) >= 2
    pick = np.arange(len(book.vox)) == two[0]
    rem = ht.remove_entries(np.repeat(book.vox[pick], 3, 0))
    assert rem.sum() == 1
    gone = np.concatenate([gone, book.drop(pick)])
    blocks, bslot = check_cluster(ht, book, S, int_bits, len(freed), gone)
    # 4. the freed blocks come back through other voxels, with 40 keys of the neighbouring home
    #    slots, in one call: each key takes the first free slot from its home, tombstones included
    pick = rng.choice(len(s["near_blocks"]), 40, replace=False)
    nvox = np.concatenate([freed * 8 + (at[::2] + 4) % 8, s["near_blocks"][pick] * 8 + rng.integers(0, 8, (40, 3))])
    nvox = nvox[rng.permutation(len(nvox))]
    nval = values(rng, len(nvox))
    live = np.zeros(S, bool)
    live[bslot] = True
    nblocks = np.unique(nvox // 8, axis=0)
    assert len(nblocks) == len(nvox)
    want = M.probe_slots(O.hash_keys(nblocks, S, int_bits), S, live)
    tomb = np.setdiff1d(run, bslot)
    assert len(tomb) == len(freed) and np.intersect1d(want, tomb).size > 0
    slot, _ = ht.add_entries(nvox, nval[:, 0], nval[:, 1], nval[:, 2])
    assert np.array_equal(np.unique(slot), np.sort(want))
    book.add(nvox, nval)
    blocks, bslot = check_cluster(ht, book, S, int_bits, len(np.setdiff1d(tomb, want)), gone)
    # 5. double_table_size: a rehash into an empty table
    ht.double_table_size()
    S *= 2
    assert ht.info()["capacity"] == S
    blocks, bslot = check_cluster(ht, book, S, int_bits, 0, gone)
    assert np.array_equal(np.sort(bslot), np.sort(M.probe_slots(O.hash_keys(blocks, S, int_bits), S)))
    # 6. trim changes nothing; reset empties the table
    info = ht.info()
    ht.trim()
    after = ht.info()
    assert {k: x for k, x in after.items() if k != "pool_capacity"} == {k: x for k, x in info.items() if k != "pool_capacity"}
    check_cluster(ht, book, S, int_bits, 0, gone)
    ht.reset()
    info = ht.info()
    assert (info["used"], info["entries"], info["tombstones"]) == (0, 0, 0)
    assert not ht.lookup(book.vox)[0].any() and len(ht.export_blocks()[0]) == 0
    ht.close()


# ------------------------------------------------------------------------------------ e
def test_removal_fixture_on_the_device(hf):
    """tests/golden/hash_c1_remove.npz, the reference's own run: lounge frame 0, remove_hash_entry
    over the rule's set, lounge frame 1.  Compared as test_lounge_c1_matches_reference_hash_path
    compares with hash_c1.npz: same positions, weights, colours and counts, tsdf within the f32
    state's 1e-4 (1e-6 in practice); the whole state against the oracle's restatement, which
    test_hash_model_cpu.py holds to the fixture's digest."""
    g = np.load(os.path.join(GOLD, "hash_c1_remove.npz"))
    idx, pos = M.c1_removal(GOLD)
    assert np.array_equal(idx, g["remove_idx"])
    K = lounge_intrinsics()
    ht = hf.HashTable(np.array(M.C1), M.C1_VS)
    hv = O.OracleHashVolume(np.array(M.C1), M.C1_VS)
    _, depth, rgb, pose = load_lounge(0)
    ht.integrate(rgb, depth, K, pose)
    hv.integrate(rgb, depth, K, pose)
    ret = ht.remove_entries(pos)
    assert np.array_equal(ret.astype(np.uint8), g["remove_ret"])
    assert ht.count_num_hash_entries() == int(g["entries_after_remove"])
    gone = tuple(pos[g["remove_ret"] == 1].T)
    hv.sdf[gone], hv.weight[gone], hv.color[gone] = M.DEFAULT
    _, depth, rgb, pose = load_lounge(1)
    ht.integrate(rgb, depth, K, pose)
    hv.integrate(rgb, depth, K, pose)
    assert ht.count_num_hash_entries() == int(g["entries_f1"])
    back = g["back_pos"].astype(np.int64)
    f, t, w, c = ht.lookup(back)
    wrong = int((w != g["back_weight"]).sum())
    print("removed voxels that frame 1 brings back: %d, with a weight other than the reference's: %d" % (len(back), wrong))
    assert f.all() and wrong == 0
    assert np.array_equal(c, g["back_color"])
    assert np.abs(t.astype(np.float64) - g["back_sdf"]).max() <= 1e-4  # f32 vs f64 state
    assert np.abs(t.astype(np.float64) - g["back_sdf"]).max() <= 1e-6  # in practice
    T, W, C = ht.get_state()
    lin, sdf, hw, hc = hv.entries()
    got = np.flatnonzero(W.reshape(-1) > 0)
    assert np.array_equal(got, lin)
    assert np.array_equal(W.reshape(-1)[lin].astype(np.float64), hw) and np.array_equal(C.reshape(-1)[lin].astype(np.float64), hc)
    assert np.abs(T.reshape(-1)[lin].astype(np.float64) - sdf).max() <= 1e-6
    assert (T.reshape(-1)[W.reshape(-1) == 0] == 1).all() and not C.reshape(-1)[W.reshape(-1) == 0].any()
    ht.close()
