"""The proof, from the oracle alone, that the preloads of update_paths.py put every class of state
where test_update_paths_gpu.py claims it: enough updated items per class, T-class items with lanes
on both sides of the route change, and final weights at the deepest reciprocal-table entries."""
import numpy as np
import pytest

import update_paths as U

MIN_ITEMS = 16


@pytest.fixture(scope="module")
def finals():
    """The oracle's final weights per (scene, kind), computed once."""
    cache = {}

    def get(scene, kind):
        if (scene, kind) not in cache:
            d, c, poses = U.frames(scene)
            cache[scene, kind] = U.oracle_run(U.preload(scene, kind), d, c, poses)[1].copy()
        return cache[scene, kind]
    return get


def test_scenes_have_the_items_the_classes_need():
    st, mv = U.activity("static"), U.activity("moving")
    # static: every voxel frame 0 updates is updated by all 32 frames, and no lane comes late
    assert st["n"] > 100_000 and not st["late"].any()
    assert np.array_equal(st["count"][st["count"] > 0], np.full((st["count"] > 0).sum(), U.NF))
    both = (mv["early"].any((-1, -2)) & mv["late"].any((-1, -2))).sum()
    balanced = ((mv["early"].sum((-1, -2)) >= 8) & (mv["late"].sum((-1, -2)) >= 8)).sum()
    assert mv["active"].sum() > 1000 and both > 500 and balanced >= 150, (mv["active"].sum(), both, balanced)


@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("scene", U.SCENES)
def test_every_class_has_items_the_scene_updates(scene, kind):
    act, cls = U.activity(scene), U.deal(scene, kind)
    names = U.classes_of(scene, kind)
    assert set(np.unique(cls)) == {-1} | {U.CODE[c] for c in names}
    # every updated item has a class; an item without updates has none, or is the idle half of a U0 brick
    assert (cls[act["active"]] >= 0).all() and (cls[~act["active"]] <= U.CODE["U0"]).all()
    for name in names:
        sel = cls == U.CODE[name]
        assert (sel & act["active"]).sum() >= MIN_ITEMS, name
        if name.startswith("T"):  # a route change needs lanes on both sides of it
            assert act["early"][sel].any((-1, -2)).all() and act["late"][sel].any((-1, -2)).all(), name
        if name == "F":
            assert act["free"][sel].all()
    # U0 covers whole bricks, some of them: the hash's cull inserts those next to imported ones
    halves = cls.reshape(U.NB, U.NB, U.NB, 2)
    assert ((halves == U.CODE["U0"]).any(-1) == (halves == U.CODE["U0"]).all(-1)).all()
    assert (halves == U.CODE["U0"]).all(-1).sum() >= MIN_ITEMS


@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("scene", U.SCENES)
def test_preloads_hold_what_the_classes_say(scene, kind):
    act, cls = U.activity(scene), U.deal(scene, kind)
    t0, w0, c0 = U.preload(scene, kind)
    assert U.is_canonical(w0, c0) == (kind == "canonical")
    W, C, T = U.items(w0), U.items(c0), U.items(t0)
    lanes = lambda a, m: a[m]  # (n lanes, 4)
    checked = 0
    for i in map(tuple, np.argwhere(cls >= 0)):
        name = U.CLASSES[cls[i]]
        e, l = act["early"][i], act["late"][i]
        w, c = W[i], C[i]
        if name == "U0":
            assert (w == 0).all() and (c == 0).all() and (T[i] == 1).all()
        elif name == "U1":
            assert (w == U.L1 - 1).all()
        elif name == "U2":
            assert (lanes(w, e) == U.L1).sum() == 1 and w.max() == U.L1
        elif name == "U3":
            assert (w == U.L2 - 1).all()
        elif name == "U4":
            assert (lanes(w, e) == U.L2).sum() == 1 and w.max() == U.L2
        elif name == "U5":
            assert (lanes(w, e) == 4000.5).sum() == 1 and w.max() == 4000.5
        elif name == "U6":
            assert w.max() in (4000, 5000) and all((lanes(c, e) == o).any() for o in U.ODD)
        elif name == "T1":
            assert (lanes(w, e) == 4000).all() and (lanes(w, l) == 4070).all()
        elif name == "T2":
            assert (lanes(w, e) == 65000).all() and (lanes(w, l) == 65510).all()
        elif name == "T3":
            assert (lanes(w, e) == 4000).all() and (lanes(w, l) == 70000).all()
        elif name == "T4":
            assert (w == 100).all() and U.is_canonical(w, lanes(c, e)) and np.isin(lanes(c, l), U.ODD).all()
        elif name == "T5":
            assert (lanes(w, e) == 100).all() and (lanes(w, l) == 100.5).all()
        elif name == "F":
            assert (T[i] == 1).all() and w.min() >= 5 and w.max() <= 15 and U.is_canonical(w, c)
        checked += 1
    assert checked == (cls >= 0).sum() > 900


@pytest.mark.parametrize("kind", U.KINDS)
def test_static_scene_reaches_the_deepest_table_entries(kind, finals):
    """32 updates from L1 - 1 read LDS entry 4094, from L2 - 1 HBM entry 65534."""
    w = finals("static", kind)
    assert (w == U.L1 - 1 + U.NF).sum() >= 1000 and U.L1 - 1 + U.NF == 4094
    assert (w == U.L2 - 1 + U.NF).sum() >= 1000 and U.L2 - 1 + U.NF == 65534
    assert (w > U.L2).any()


@pytest.mark.parametrize("kind", U.KINDS)
def test_moving_scene_ends_on_both_sides_of_the_limits(kind, finals):
    w = finals("moving", kind)
    w0 = U.preload("moving", kind)[1]
    moved = w != w0
    for lim in (U.L1, U.L2):
        assert (moved & (w < lim)).any() and (moved & (w >= lim)).any(), lim
    assert (moved & (w >= U.L1) & (w < U.L2)).any()


def test_block_view_matches_the_local_order():
    a = np.arange(U.N ** 3, dtype=np.float32).reshape(U.N, U.N, U.N)
    b, xyz = U.blocks(a), U.block_coords()
    for j in (0, 777, 4095):
        bx, by, bz = xyz[j]
        for x, y, z in ((0, 0, 0), (3, 5, 7), (7, 7, 7)):
            assert b[j, (x * 8 + y) * 8 + z] == a[8 * bx + x, 8 * by + y, 8 * bz + z]
