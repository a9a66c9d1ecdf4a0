"""The conditions the hash model's GPU tests rest on (test_hash_model_gpu.py), the model's own
operations, and the model against the reference's removal fixture.  Everything here runs on the CPU.

The counts below are lower bounds; the values measured with the oracle when the tests were written
are the record: scene A holds 28 686 entries in 162 blocks after frame 3; the rule removes 12 979 of
them and 33 whole blocks, one more block loses its last entry through the every-third rule alone, so
128 blocks are left; frames 4-7 update 2 063 of the removed voxels again, 1 200 of them in blocks
that stayed live, over old weights 1 to 3.  Scene B's four home slots 2320-2323 take 311 block keys
(70, 76, 80 and 85), for int64 and for int32 keys.
"""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLD, load_lounge, lounge_intrinsics
import oracle as O
import hash_model as M
from bucket_table import BucketTable


@pytest.mark.parametrize("kind", M.KINDS)
def test_scene_a_puts_removed_voxels_under_later_frames(kind):
    a = M.scene_a(kind)
    assert a["again_live"] >= 1000          # removed voxels of surviving blocks that frames 4-7 update again
    assert a["whole_blocks"] >= 20          # blocks the rule removes whole ...
    assert a["blocks_mid"] - a["blocks_after"] >= a["whole_blocks"] >= 20  # ... and that are freed
    assert a["blocks_emptied_by_third"] >= 1
    assert (a["old_weights"] >= 1).all()    # state a stale voxel would blend into
    assert len(np.unique(a["removal"], axis=0)) == len(a["removal"]) == a["n_removed"]
    assert a["mid"].entry[tuple(a["removal"].T)].all() and not a["after"].entry[tuple(a["removal"].T)].any()
    # a removed voxel keeps no state: where frames 4-7 come back it holds one observation
    v = tuple(a["again_live_voxels"].T)
    assert (a["final"].fields[1][v] >= 1).all() and (a["final"].fields[1][v] <= 4).all()
    if kind == "canonical":
        assert (a["entries_mid"], a["blocks_mid"], a["n_removed"], a["whole_blocks"], a["blocks_after"],
                a["again"]) == (28686, 162, 12979, 33, 128, 2063)
    else:
        import update_paths as U
        ijk, t, w, c = a["hand"]
        assert len(ijk) >= 200 and not U.is_canonical(w, c)
        in_set = np.isin(np.ravel_multi_index(tuple(ijk.T), a["mid"].dims),
                         np.ravel_multi_index(tuple(a["removal"].T), a["mid"].dims))
        assert in_set.sum() == (len(ijk) + 1) // 2
        assert not U.is_canonical(*a["final"].state()[1:])  # some stay non-canonical to the end


@pytest.mark.parametrize("int_bits", [64, 32])
def test_scene_b_is_one_probe_cluster(int_bits):
    s = M.scene_b(int_bits)
    assert len(s["blocks"]) >= 300 and len(s["homes"]) == 4 and (np.diff(s["homes"]) == 1).all()
    assert (len(s["blocks"]), s["start"], int(s["per_slot"].max())) == (311, 2320, 85)
    n = len(s["blocks"])
    run = np.arange(s["start"], s["start"] + n)
    for order in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(0).permutation(n)):
        got = M.probe_slots(s["home"][order], M.B_MAP)
        assert np.array_equal(np.sort(got), run)       # one contiguous run from 2320, whatever the order
        assert (got >= s["home"][order]).all()
    # a tombstone counts as free: with every other slot of the run live, the rest fill the gaps first
    live = np.zeros(M.B_MAP, bool)
    live[run[::2]] = True
    got = M.probe_slots(s["home"][: n // 2], M.B_MAP, live)
    assert np.array_equal(np.sort(got), run[1::2][: n // 2])


def test_probe_slots_wraps_and_fills():
    assert M.probe_slots([6, 7, 7, 7], 8).tolist() == [6, 7, 0, 1]
    occ = np.array([1, 0, 1, 1, 0, 0, 0, 1], bool)
    assert M.probe_slots([7, 2, 2], 8, occ).tolist() == [1, 4, 5]
    with pytest.raises(ValueError):
        M.probe_slots([0, 0, 0], 2)


def test_model_operations():
    m = M.HashModel(M.a_bounds(), M.A_VS)
    p = np.array([[1, 2, 3], [9, 2, 3], [63, 63, 63]])
    m.insert(p[:2], tsdf=[0.25, -0.5], weight=[2.0, 3.5], color=[7.0, 9.0])
    m.insert(p[2:])                                       # a new entry without values: the default
    m.insert(p[:1], tsdf=[0.75])                          # an existing entry keeps its other fields
    f, t, w, c = m.lookup(np.vstack([p, [[0, 0, 0]]]))
    assert f.tolist() == [True, True, True, False]
    assert (t.tolist(), w.tolist(), c.tolist()) == ([0.75, -0.5, 1.0, 1.0], [2.0, 3.5, 0.0, 0.0], [7.0, 9.0, 0.0, 0.0])
    assert m.entries() == 3 and m.blocks().tolist() == [[0, 0, 0], [1, 0, 0], [7, 7, 7]]
    b, et, ew, ec, occ = m.export()
    local = (1 * 8 + 2) * 8 + 3
    assert et[0, local] == 0.75 and ew[0, local] == 2.0 and ec[0, local] == 7.0
    assert occ[0].tolist() == [0, 0, 0, 1 << (1 * 8 + 2), 0, 0, 0, 0] and occ[2, 7] == np.uint64(1) << np.uint64(63)
    # import: a clear bit is absent whatever the arrays hold; a field not given stays
    m2 = M.HashModel(M.a_bounds(), M.A_VS)
    has = m._by_block(m.entry)[tuple(b.T.astype(np.int64))].reshape(len(b), 512)
    m2.import_(b, np.where(has, et, np.float32(-0.5)), np.where(has, ew, np.float32(7.0)), ec, occ)
    assert m2.entries() == 3 and all(M.same(x, y) for x, y in zip(m2.state(), m.state()))
    assert all(M.same(x, np.where(m2.entry, x, np.float32(d))) for x, d in zip(m2.fields, M.DEFAULT))
    m2.import_(b[:1], et[:1], None, None, None)
    assert m2.entries() == 2 + 512 and [float(x[0]) for x in m2.lookup(p[:1])] == [1.0, 0.75, 2.0, 7.0]
    assert [float(x[0]) for x in m2.lookup([[0, 0, 0]])] == [1.0, 1.0, 0.0, 0.0]
    # remove: the bit from before the call, once per voxel; no state is kept
    r = m.remove(np.vstack([p[:1], p[:1], [[5, 5, 5]], p[:1]]))
    assert r.tolist() == [True, False, False, False]
    m.insert(p[:1])
    assert [x[0] for x in m.lookup(p[:1])] == [True, 1.0, 0.0, 0.0]
    m.resize(123), m.trim()
    assert m.entries() == 3
    m.reset()
    assert m.entries() == 0 and len(m.blocks()) == 0 and all(M.same(x, np.full(m.dims, d, np.float32))
                                                              for x, d in zip(m.fields, M.DEFAULT))


def test_model_matches_the_reference_removal_fixture():
    """tests/golden/hash_c1_remove.npz: the reference HashTable integrates lounge frame 0, removes the
    rule's set with remove_hash_entry and integrates frame 1.  The reference's chained-bucket table
    (oracle/bucket_table.py) predicts every remove's return; resetting the removed voxels to
    (1, 0, 0) -- the model's remove -- and integrating frame 1 gives the reference's f64 state
    exactly."""
    g = np.load(os.path.join(GOLD, "hash_c1_remove.npz"))
    g0 = np.load(os.path.join(GOLD, "hash_c1.npz"))
    idx, pos = M.c1_removal(GOLD)
    assert np.array_equal(idx, g["remove_idx"])
    hv = O.OracleHashVolume(np.array(M.C1), M.C1_VS)
    K = lounge_intrinsics()
    _, depth, rgb, pose = load_lounge(0)
    hv.integrate(rgb, depth, K, pose)
    dims = tuple(int(d) for d in hv._vol_dim)
    # the reference's table after frame 0 (insertion in C order), then its removes
    bt = BucketTable(1000000)
    for p in np.stack(np.unravel_index(hv.new_keys, dims), 1):
        bt.add(p)
    assert bt.count_entries() == int(g0["f0_entries"])
    ret = np.array([bt.remove(p) for p in pos], np.uint8)
    assert np.array_equal(ret, g["remove_ret"])
    assert bt.count_entries() == int(g["entries_after_remove"]) and bt.nonempty == int(g["nonempty_after_remove"])
    gone = tuple(pos[ret == 1].T)
    hv.sdf[gone], hv.weight[gone], hv.color[gone] = M.DEFAULT
    assert len(hv.entries()[0]) == int(g["entries_after_remove"])
    _, depth, rgb, pose = load_lounge(1)
    hv.integrate(rgb, depth, K, pose)
    lin, sdf, w, c = hv.entries()
    assert len(lin) == int(g["entries_f1"])
    p1 = np.stack(np.unravel_index(lin, dims), 1).astype(np.int64)
    h = hashlib.sha256()
    for a in (p1, sdf, w, c):
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == str(g["state_sha256"])
    back = np.isin(lin, np.ravel_multi_index(tuple(pos.T), dims))
    assert np.array_equal(p1[back], g["back_pos"].astype(np.int64))
    assert np.array_equal(sdf[back], g["back_sdf"])
    assert np.array_equal(w[back], g["back_weight"].astype(np.float64))
    assert np.array_equal(c[back], g["back_color"].astype(np.float64))
    assert len(g["back_pos"]) >= 1000 and (g["back_weight"] == 1).all()  # fresh voxels: one observation
