"""Inputs of the update-path tests (test_update_paths_cpu.py, test_update_paths_gpu.py): two
32-frame scenes on a 128^3 @ 8 cm volume and preloaded states that pin every arithmetic route of
the integrate update (integrate_brick, csrc/tsdf_device.h) on chosen waves.  Plain functions only;
everything here runs on the CPU, from the synthetic scene and the C oracle.

A wave item is one brick times one z-half: item (bx, by, zq) holds x in 8*bx .. 8*bx+7, y in
8*by .. 8*by+7, z in 4*zq .. 4*zq+3; its lane (x & 7) * 8 + (y & 7) holds a column of 4 voxels.  A
wave picks its route from the state it has loaded so far, and a lane loads its column at the first
frame that updates it, so the items are classified with the oracle's per-frame update masks:

  early lanes  update at the item's first updating frame,
  late lanes   update only at a later frame,

and the preload deals these classes to the items the scene updates (L1 = 4063 and L2 = 65503 are
kRcpTab and kRcpBig less kMaxBatch + 1 of the default 32-frame build):

  U0  untouched (1, 0, 0), dealt per brick      new hash blocks next to imported ones
  U1  every weight L1 - 1                       LDS table up to its last entry (static: 4094)
  U2  weights 4000, one voxel L1                HBM table from the first frame
  U3  every weight L2 - 1                       HBM table up to its last entry (static: 65534)
  U4  weights 65000, one voxel L2               IEEE division
  U5  weights 4000, one voxel 4000.5       (m)  IEEE division through a non-integer weight
  U6  weights 4000 | 5000, four odd colours (m) exact colour route with a table tsdf quotient
  T1  early lanes 4000, late lanes 4070         LDS -> HBM inside the batch
  T2  early 65000, late 65510                   HBM -> IEEE inside the batch
  T3  early 4000, late 70000                    LDS -> IEEE inside the batch
  T4  late lanes hold odd colours          (m)  packed colours -> exact colours inside the batch
  T5  early 100, late 100.5                (m)  packed -> IEEE through a late non-integer weight
  F   tsdf 1, weights 5 .. 15, in free space    the free-space shortcut on preloaded weights

The `canonical` preload holds integer weights and canonical colours only (Vol::canon stays set, so
the u32-colour kernels run); `mixed` adds the classes marked (m).  The static scene has no late
lanes, so its preloads hold no T class.  The NZ = 8 kernels and the hash's in-line kernel give a
wave the whole brick: there the classes of both z-halves set the wave's route.
"""
import functools

import numpy as np

import oracle as O

ROOM = 10.24
VS = 0.08
N = 128            # voxels per axis
NB = N // 8        # bricks per axis
NF = 32            # frames per scene = frames per launch (TSDF_BATCH=32)
L1 = 4096 - 33     # kRcpTab - kMaxBatch - 1
L2 = 65536 - 33    # kRcpBig - kMaxBatch - 1
NEVER = 127
ODD = np.array([0.5, -3.0, 16777216.0 + 512.0, 123456.75], np.float32)

SCENES = ("static", "moving")
KINDS = ("canonical", "mixed")
CLASSES = ("U0", "U1", "U2", "U3", "U4", "U5", "U6", "T1", "T2", "T3", "T4", "T5", "F")
CODE = {name: i for i, name in enumerate(CLASSES)}  # (-1: an item the preload leaves alone)
MIXED_ONLY = ("U5", "U6", "T4", "T5")
T_PER_CLASS = 48   # items dealt to each T class (of ~185 well-balanced candidates)
OW_CYCLE = (1.0, 0.6, 2.0)


def bounds():
    return np.array([[0.0, ROOM]] * 3)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def classes_of(scene, kind):
    """The classes a preload of this scene and kind deals."""
    return tuple(c for c in CLASSES if (kind == "mixed" or c not in MIXED_ONLY)
                 and (scene == "moving" or not c.startswith("T")))


def ow_cycle(n):
    return np.array([OW_CYCLE[i % len(OW_CYCLE)] for i in range(n)])


# ------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def _rendered():
    from tsdf_amd import scene
    poses = scene.trajectory(NF, seed=0, start=120, radius_frac=0.34)
    d, c = scene.render(poses, scene.make_spheres(0, ring_frac=0.34), seed=0, start=120)
    d, c = np.ascontiguousarray(d.numpy()), np.ascontiguousarray(c.numpy())
    rng = np.random.default_rng(11)
    c[:, ::3] = rng.integers(0, 256, c[:, ::3].shape, dtype=np.uint8)  # averages are not trivial
    for a in (d, c, poses):
        a.setflags(write=False)
    return d, c, poses


@functools.lru_cache(maxsize=None)
def frames(scene):
    """(depth u16 mm (32, 480, 640), RGB8 (32, 480, 640, 3), poses (32, 4, 4)); `static` repeats
    frame 0's pose and depth under the 32 different colour images."""
    d, c, poses = _rendered()
    if scene == "moving":
        return d, c, poses
    ds, ps = np.repeat(d[:1], NF, axis=0), np.repeat(poses[:1], NF, axis=0)
    ds.setflags(write=False)
    ps.setflags(write=False)
    return ds, c, ps


def intrinsics():
    from tsdf_amd import scene
    return scene.intrinsics()


def fold(c):
    """RGB8 frames (F, H, W, 3) as folded float32 (F, H, W) (grid_fusion.py:228-232)."""
    return np.stack([O.fold_color(f) for f in c])


# ------------------------------------------------------------------------------------ oracle
def oracle_run(state, depth, rgb, poses, ow=None, *, voxel_size=VS, x_index=None, masks=False, into=None):
    """The oracle over the frames from `state` = (t0, w0, c0) (None: fresh): (tsdf, weight,
    colour, voxel updates[, per-voxel first updating frame, per-voxel update count]).  `into`: an
    OracleTSDFVolume to continue on."""
    orc = into or O.OracleTSDFVolume(bounds(), voxel_size, x_index=x_index)
    if state is not None:
        orc._tsdf_vol_cpu[:], orc._weight_vol_cpu[:], orc._color_vol_cpu[:] = state
    K = intrinsics()
    n = 0
    if masks:
        first = np.full(orc._tsdf_vol_cpu.size, NEVER, np.int8)
        count = np.zeros(orc._tsdf_vol_cpu.size, np.int8)
    for f in range(len(poses)):
        n += orc.integrate(rgb[f], depth[f].astype(float) / 1000.0, K, poses[f],
                           obs_weight=1.0 if ow is None else float(ow[f]), want_mask=masks)
        if masks:
            m = orc.last_updated.astype(bool)
            first[m & (first == NEVER)] = f
            count += m
    out = (orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu, n)
    if masks:
        shape = orc._tsdf_vol_cpu.shape
        out += (first.reshape(shape), count.reshape(shape))
    return out


def items(a):
    """A (128, 128, 128) array as a view (bx, by, zq, x & 7, y & 7, z & 3) of its wave items."""
    return a.reshape(NB, 8, NB, 8, N // 4, 4).transpose(0, 2, 4, 1, 3, 5)


@functools.lru_cache(maxsize=None)
def activity(scene):
    """What a fresh oracle run of the scene updates, per voxel, lane and item."""
    d, c, poses = frames(scene)
    t, _, _, n, first, count = oracle_run(None, d, c, poses, masks=True)
    lane_first = items(first).min(-1)                 # (bx, by, zq, 8, 8)
    item_first = lane_first.min((-1, -2))             # (bx, by, zq)
    active = item_first < NEVER
    early = (lane_first == item_first[..., None, None]) & active[..., None, None]
    late = (lane_first > item_first[..., None, None]) & (lane_first < NEVER)
    # free space: every update of the item's voxels left the fresh tsdf at exactly 1
    free = active & ~items((count > 0) & (t != 1.0)).any((-1, -2, -3))
    return dict(first=first, count=count, n=n, lane_first=lane_first, item_first=item_first, active=active,
                early=early, late=late, free=free)


# ------------------------------------------------------------------------------------ dealing
@functools.lru_cache(maxsize=None)
def deal(scene, kind):
    """Class code per item (bx, by, zq), -1 where the scene updates nothing.  Deterministic:
    every 6th active brick is U0 as a whole; the items with the best balance of early and late
    lanes go round-robin to the T classes; every 3rd free-space item of the rest is F; what is
    left goes round-robin to U1 .. U6."""
    act = activity(scene)
    names = classes_of(scene, kind)
    cls = np.full(act["active"].shape, -1, np.int8)
    brick_active = act["active"].reshape(NB, NB, NB, 2).any(-1)
    for j, (bx, by, bz) in enumerate(np.argwhere(brick_active)):
        if j % 6 == 0:
            cls[bx, by, 2 * bz:2 * bz + 2] = CODE["U0"]
    todo = act["active"] & (cls < 0)
    t_names = [c for c in names if c.startswith("T")]
    if t_names:
        balance = np.minimum(act["early"].sum((-1, -2)), act["late"].sum((-1, -2)))
        cand = np.argwhere(todo & (balance > 0))
        order = np.argsort(-balance[tuple(cand.T)], kind="stable")
        for j, (bx, by, zq) in enumerate(cand[order][:T_PER_CLASS * len(t_names)]):
            cls[bx, by, zq] = CODE[t_names[j % len(t_names)]]
    todo = act["active"] & (cls < 0)
    for j, (bx, by, zq) in enumerate(np.argwhere(todo & act["free"])):
        if j % 3 == 0:
            cls[bx, by, zq] = CODE["F"]
    todo = act["active"] & (cls < 0)
    u_names = [c for c in names if c.startswith("U") and c != "U0"]
    for j, (bx, by, zq) in enumerate(np.argwhere(todo)):
        cls[bx, by, zq] = CODE[u_names[j % len(u_names)]]
    cls.setflags(write=False)
    return cls


def _canon(rng, shape):
    return (rng.integers(0, 256, shape) * 65536 + rng.integers(0, 256, shape) * 256
            + rng.integers(0, 256, shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def preload(scene, kind):
    """(t0, w0, c0) float32 (128, 128, 128), read-only."""
    act, cls = activity(scene), deal(scene, kind)
    rng = np.random.default_rng([SCENES.index(scene), KINDS.index(kind), 7])
    t0, w0, c0 = np.ones((N, N, N), np.float32), np.zeros((N, N, N), np.float32), np.zeros((N, N, N), np.float32)
    T, W, C = items(t0), items(w0), items(c0)
    first = items(act["first"])
    S = (8, 8, 4)

    def background(w):  # about 30 % of the voxels the class does not pin start unseen
        a = np.full(S, w, np.float32)
        a[rng.random(S) < 0.3] = 0.0
        return a

    def by_lane(i, w_early, w_late):  # (lanes that never update: either value)
        pick = np.where(act["late"][i] | (~act["early"][i] & (rng.random((8, 8)) < 0.5)), w_late, w_early)
        return np.broadcast_to(pick[..., None], S).astype(np.float32)

    for ordinal, i in enumerate(map(tuple, np.argwhere(cls > CODE["U0"]))):
        name = CLASSES[cls[i]]
        # voxels of early lanes, those the item's first frame updates first: where the pins go
        at_first = first[i] == act["item_first"][i]
        pins = np.concatenate([np.argwhere(at_first), np.argwhere(act["early"][i][..., None] & ~at_first)])
        pin = tuple(pins[0])
        t, c = rng.uniform(-1, 1, S).astype(np.float32), _canon(rng, S)
        if name == "U1":
            w = np.full(S, L1 - 1, np.float32)
        elif name == "U2":
            w = background(4000)
            w[pin] = L1
        elif name == "U3":
            w = np.full(S, L2 - 1, np.float32)
        elif name == "U4":
            w = background(65000)
            w[pin] = L2
        elif name == "U5":
            w = background(4000)
            w[pin] = 4000.5
        elif name == "U6":
            w = background(4000 if ordinal % 2 else 5000)
            for k in range(4):
                c[tuple(pins[k])] = ODD[k]
        elif name == "T1":
            w = by_lane(i, 4000, 4070)
        elif name == "T2":
            w = by_lane(i, 65000, 65510)
        elif name == "T3":
            w = by_lane(i, 4000, 70000)
        elif name == "T4":
            w = np.full(S, 100, np.float32)
            odd_lane = by_lane(i, 0, 1) > 0
            c = np.where(odd_lane, rng.choice(ODD, S), c).astype(np.float32)
        elif name == "T5":
            w = by_lane(i, 100, 100.5)
        else:  # F
            t = np.ones(S, np.float32)
            w = rng.integers(5, 16, S).astype(np.float32)
        T[i], W[i], C[i] = t, w, c
    for a in (t0, w0, c0):
        a.setflags(write=False)
    return t0, w0, c0


def is_canonical(w, c):
    """Vol::canon's condition: weights integers >= 0, colours integers in [0, 2^24)."""
    return bool(((w >= 0) & (w == np.trunc(w))).all() and ((c >= 0) & (c < 2.0 ** 24) & (c == np.trunc(c))).all())


# ------------------------------------------------------------------------------------ hash blocks
def blocks(a):
    """A (128, 128, 128) array as (4096, 512) blocks in brick-local order (x * 8 + y) * 8 + z."""
    return np.ascontiguousarray(a.reshape(NB, 8, NB, 8, NB, 8).transpose(0, 2, 4, 1, 3, 5)).reshape(NB ** 3, 512)


def block_coords():
    return np.ascontiguousarray(np.indices((NB, NB, NB)).reshape(3, -1).T.astype(np.int32))


def preloaded_blocks(scene, kind):
    """(bxyz, t, w, c) of every brick with at least one preloaded (non-U0) half; wholly U0
    bricks are left for the cull to insert."""
    sel = (deal(scene, kind).reshape(NB, NB, NB, 2) > CODE["U0"]).any(-1).reshape(-1)
    t0, w0, c0 = preload(scene, kind)
    return (block_coords()[sel],) + tuple(np.ascontiguousarray(blocks(a)[sel]) for a in (t0, w0, c0))


# ------------------------------------------------------------------------------------ reporting
def mismatch_by_class(scene, kind, got, exp):
    """Differing voxels per class of their item, for the assertion message: the class names the
    route (the table in this module's docstring)."""
    cls = deal(scene, kind)
    out = {}
    for field, g, e in zip(("tsdf", "weight", "colour"), got, exp):
        bad = np.asarray(g, np.float32).view(np.uint32) != np.asarray(e, np.float32).view(np.uint32)
        per_item = items(bad).sum((-1, -2, -3))
        for code in np.unique(cls[per_item > 0]):
            name = CLASSES[code] if code >= 0 else "none"
            out[f"{field}/{name}"] = int(per_item[cls == code].sum())
    return out
