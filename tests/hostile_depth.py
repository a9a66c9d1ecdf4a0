"""Inputs shared by tests/test_hostile_depth_cpu.py, tests/test_hostile_depth_gpu.py and
tools/gen_golden.py (the "hostile" section): float64 depth frames holding what float-depth sources
really deliver -- NaN, infinities, negatives, -0.0, depths too small for f32, depths at and beyond
the u16 millimetre range, depths too large for f32 -- in a small ragged volume seen from three
poses, at an image width the vectorised prep takes (W % 4 == 0) and at one it does not.  Everything
here is NumPy; the counts the placement must reach are taken on the oracle alone and asserted by the
CPU module.  Callers must leave the returned arrays unchanged (they are cached).

The reference's rule (grid_fusion.py:278-286): `depth_val > 0` is false for NaN, -inf, negatives and
-0.0; +inf and every huge depth pass and carve free space with tsdf = min(1, diff / trunc) = 1; a
tiny positive depth updates the voxels with 0 < z <= trunc only."""
import functools
import struct

import numpy as np

import icp_ref as I

BOUNDS = [[-0.48, 0.48], [-0.40, 0.40], [0.0, 0.48]]  # 48 x 40 x 24 voxels at 2 cm: ragged, <= 64 per axis
VS = 0.02
DIMS = (48, 40, 24)
K = np.array([[100.0, 0.0, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]])
SIZES = {"vec": (96, 128), "scalar": (95, 126)}  # (H, W): k_prep_vec, and the scalar k_prep with partial tiles
PLANE_Z = 0.3

NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]  # a NaN with the sign bit set
# name -> (value, group)
CLASSES = {
    "nan": (float("nan"), "zero"), "nan_neg": (NAN_NEG, "zero"),
    "neg_inf": (-np.inf, "zero"), "neg_one": (-1.0, "zero"), "neg_zero": (-0.0, "zero"),
    "pos_inf": (np.inf, "carve"),
    "tiny_5e-324": (5e-324, "tiny"), "tiny_1e-46": (1e-46, "tiny"), "tiny_1e-40": (1e-40, "tiny"),
    "d_65.535": (65.535, "far"), "d_65.536": (65.536, "far"), "d_70": (70.0, "far"),
    "huge_3.5e38": (3.5e38, "carve"), "huge_1e300": (1e300, "carve"), "huge_1.7e308": (1.7e308, "carve"),
}
VALUES = np.array([v for v, _ in CLASSES.values()])
# What a class must change in a fresh volume, alone in its region of an otherwise zero frame, from
# pose 0: "zero" classes nothing, "tiny" at least MIN_TINY voxels (those with 0 < z <= trunc),
# "carve" and "far" at least MIN_CARVE (free space through the whole volume).
MIN_TINY, MIN_CARVE = 10, 1000


def track_hostile(values):
    """The tracking rule of icp_ref / sdf_ref / icp_color_ref: no depth unless f32(d) > 0 and finite."""
    with np.errstate(over="ignore"):
        f = np.asarray(values, dtype=np.float64).astype(np.float32)
    return ~((f > 0) & np.isfinite(f))


def region(size):
    """(rows, cols) of the class region: it holds one whole 64 x 64 prep tile -- tile (x 1, y 0) of the
    128-wide image, tile (0, 0) of the 126-wide one -- and the pixels around the principal point."""
    return (slice(0, 80), slice(32, 128)) if size == "vec" else (slice(0, 80), slice(0, 96))


def whole_tile(size):
    return (slice(0, 64), slice(64, 128)) if size == "vec" else (slice(0, 64), slice(0, 64))


def poses():
    """Camera at z = -0.05 looking along +z; the same turned 20 degrees about its x and about its y axis."""
    a = np.radians(20.0)
    c, s = np.cos(a), np.sin(a)
    out = []
    for R in (np.eye(3), np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])):
        P = np.eye(4)
        P[:3, :3] = R
        P[:3, 3] = [0.0, 0.0, -0.05]
        out.append(P)
    return out


def background(size):
    """A plane at 0.3 m whose depths are no whole millimetres (these frames must travel as f64); five
    distinct values, so that the fixture's copy of the frames compresses."""
    H, W = SIZES[size]
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return PLANE_Z + 3.1e-5 + 2e-5 * ((u + 3 * v) % 5)


def mm_exact(depth):
    """The frame rounded to whole millimetres, as RN(k / 1000): what the deferred path stages as u16."""
    return np.rint(np.asarray(depth) * 1000.0) / 1000.0


def rgb(size, seed=0):
    """A deterministic colour image (H, W, 3) u8: constant over 8 x 8 pixel blocks (the fixture's copy
    of the images and of the blended voxel colours compresses), with a seeded 1 % sprinkle of any byte."""
    H, W = SIZES[size]
    v, u = np.meshgrid(np.arange(H) // 8, np.arange(W) // 8, indexing="ij")
    c = np.stack([(37 * u + 11 * v + 17 * seed) % 256, (29 * v + 5 * seed + 40) % 256, (13 * u + 53 * v + 90) % 256], axis=-1).astype(np.uint8)
    rng = np.random.default_rng(100 + seed)
    m = rng.random((H, W)) < 0.01
    c[m] = rng.integers(0, 256, (int(m.sum()), 3), dtype=np.uint8)
    return np.ascontiguousarray(c)


def class_frame(size, name, alone=False):
    """The class in its region; elsewhere the background, or zeros with `alone` (the coverage frames)."""
    d = np.zeros(SIZES[size]) if alone else background(size).copy()
    d[region(size)] = CLASSES[name][0]
    return d


def scatter_frame(size):
    """The background with one hostile pixel in every 4 x 2 block a prep thread reads (a quarter of
    the blocks of the last, partial column / row have none): block b holds class b % 15 at position
    b % 8 of the block, so every class meets every position, on either side of each fmaxf."""
    d = background(size).copy()
    H, W = SIZES[size]
    by, bx = np.meshgrid(np.arange((H + 1) // 2), np.arange((W + 3) // 4), indexing="ij")
    b = (by * ((W + 3) // 4) + bx).ravel()
    y, x = 2 * by.ravel() + (b % 8) // 4, 4 * bx.ravel() + (b % 8) % 4
    ok = (y < H) & (x < W)
    d[y[ok], x[ok]] = VALUES[b[ok] % len(VALUES)]
    return d


@functools.lru_cache(maxsize=None)
def sequence(size):
    """The frames of one image size, in the order they are integrated into one volume:
    (names, depth (F,H,W) f64, rgb (F,H,W,3) u8, poses (F,4,4), obs_weight (F,)).  A benign frame, the
    15 class frames, the scatter frame, an all-NaN and an all-zero frame, a benign frame; the poses
    cycle, the weights alternate 1 and 0.5."""
    names = ["benign0"] + list(CLASSES) + ["scatter", "all_nan", "all_zero", "benign1"]
    H, W = SIZES[size]
    frames = {"benign0": background(size), "scatter": scatter_frame(size), "all_nan": np.full((H, W), np.nan),
              "all_zero": np.zeros((H, W)), "benign1": background(size) + 0.01}
    depth = np.stack([frames[n] if n in frames else class_frame(size, n) for n in names])
    P = poses()
    return (names, depth, np.stack([rgb(size, f % 3) for f in range(len(names))]),
            np.stack([P[f % 3] for f in range(len(names))]), np.array([1.0, 0.5] * len(names))[:len(names)])


def oracle_run(size, obs_weight=None, frames=None):
    """The oracle over sequence(size) (or its first `frames` frames): (volume, per-frame update counts)."""
    import oracle as O
    names, depth, col, P, ow = sequence(size)
    vol = O.OracleTSDFVolume(np.array(BOUNDS), VS)
    assert tuple(int(x) for x in vol._vol_dim) == DIMS
    n = [vol.integrate(col[f], depth[f], K, P[f], obs_weight=float(ow[f] if obs_weight is None else obs_weight))
         for f in range(len(names) if frames is None else frames)]
    return vol, n


@functools.lru_cache(maxsize=None)
def class_counts(size):
    """name -> voxels the class changes: the oracle's update count, in a fresh volume from pose 0, of
    a frame that is zero outside the class's region; and whether any NaN reached the state."""
    import oracle as O
    out, clean = {}, True
    for name in CLASSES:
        vol = O.OracleTSDFVolume(np.array(BOUNDS), VS)
        out[name] = vol.integrate(rgb(size), class_frame(size, name, alone=True), K, poses()[0])
        assert out[name] == int((vol._weight_vol_cpu > 0).sum())
        clean &= not (np.isnan(vol._tsdf_vol_cpu).any() or np.isnan(vol._weight_vol_cpu).any() or np.isnan(vol._color_vol_cpu).any())
    return out, clean


def assert_coverage(size):
    counts, clean = class_counts(size)
    assert clean
    for name, (_, group) in CLASSES.items():
        n = counts[name]
        assert (n == 0 if group == "zero" else n >= (MIN_TINY if group == "tiny" else MIN_CARVE)), (size, name, n)
    return counts


# ---- tracking: the corner scene at 64 x 48 with scattered hostile pixels -------------------------------
TRACK_HW = (48, 64)
TRACK_K = np.array(I.FRAME_K, dtype=np.float64)
TRACK_K[0] *= TRACK_HW[1] / I.FRAME_HW[1]
TRACK_K[1] *= TRACK_HW[0] / I.FRAME_HW[0]
HOSTILE_RATE = 0.05


@functools.lru_cache(maxsize=None)
def track_frame(pose_key="true"):
    """(depth (48,64) f64 metres, hostile (48,64) bool): the corner rendered from its true pose
    ("true") or the identity ("eye"), u16 / 1000, with about 5 % of the pixels replaced by the class
    values in turn (seeded).  `hostile` marks the replaced pixels that the tracking rule drops: 1e-40
    (an f32 subnormal) and the depths near 65.5 / 70 m stay depths there."""
    pose = I.TRUE_POSE if pose_key == "true" else np.eye(4)
    d = I.render(pose, TRACK_K, TRACK_HW).astype(np.float64) / 1000.0
    rng = np.random.default_rng(41)
    m = rng.random(TRACK_HW) < HOSTILE_RATE
    d[m] = VALUES[np.arange(int(m.sum())) % len(VALUES)]
    return d, m & track_hostile(d)


def track_rgb():
    """The grey image of the RGB-D entry points at the tracking size (the textured plane's)."""
    import icp_color_ref as C
    return C.plane_render(K=TRACK_K, hw=TRACK_HW)[1]


# ---- the deferred path: hostile f64 frames among millimetre-exact ones -------------------------------
@functools.lru_cache(maxsize=None)
def deferred_sequence(size):
    """(depth list, rgb, poses, obs_weight): before every frame of sequence(size) two benign frames
    whose depths are whole millimetres.  Per-frame deferred calls stage those as u16 millimetres; the
    frame that follows is no such frame (all but "all_zero"), has to travel as f64 and so to flush
    the pending batch first."""
    names, depth, col, P, ow = sequence(size)
    mm = [mm_exact(background(size)), mm_exact(background(size) + 0.004)]
    assert all(np.array_equal(m, np.rint(m * 1000.0) / 1000.0) and (m > 0).all() for m in mm)
    D, C, Q, Wt = [], [], [], []
    for f in range(len(names)):
        for k, g in ((0, (f + 1) % len(names)), (1, (f + 2) % len(names)), (None, f)):
            D.append(depth[f] if k is None else mm[k])
            C.append(col[g])
            Q.append(P[g])
            Wt.append(float(ow[f]) if k is None else 1.0)
    return D, C, Q, Wt


# ---- frustum bounds -------------------------------------------------------------------------------
def frustum_poses(n):
    """n camera poses whose translations are nonzero on every axis (no bound is decided between a
    +0.0 and a -0.0).  Even frames: the product of poses()'s rotations about x and y, which has a
    single zero entry, so that an infinite max depth gives infinite coordinates besides the NaN ones;
    odd frames: the three rotations of poses() in turn, whose zero entries all give 0 * inf."""
    P = poses()
    R = [q[:3, :3] for q in P] + [P[1][:3, :3] @ P[2][:3, :3]]
    out = []
    for f in range(n):
        Q = np.eye(4)
        Q[:3, :3] = R[3] if f % 2 == 0 else R[(f // 2) % 3]
        Q[:3, 3] = [0.11 + 0.01 * f, -0.23 + 0.02 * f, -0.05 - 0.01 * f]
        out.append(Q)
    return np.stack(out)


def frustum_frames(size="vec"):
    """name -> f64 frame.  "finite": the maximum over the non-NaN pixels is finite (and so are the
    frustum's coordinates); "contract": an infinite maximum, coordinates that overflow, or no
    non-NaN pixel at all."""
    H_, W = SIZES[size]
    nan_scatter = background(size).copy()
    nan_scatter[::3, ::5] = np.nan
    nan_scatter[1::7, 2::3] = NAN_NEG
    finite = {"neg_only": np.full((H_, W), -1.0), "tiny_only": np.full((H_, W), 5e-324), "huge_1e300": class_frame(size, "huge_1e300"),
              "nan_scatter": nan_scatter, "nan_region": class_frame(size, "nan"), "neg_and_nan": np.where(nan_scatter == nan_scatter, -2.5, np.nan),
              "far": class_frame(size, "d_70"), "benign": background(size)}
    contract = {"pos_inf": class_frame(size, "pos_inf"), "scatter": scatter_frame(size), "huge_1.7e308": class_frame(size, "huge_1.7e308"),
                "all_nan": np.full((H_, W), np.nan), "all_nan_neg": np.full((H_, W), NAN_NEG)}
    return finite, contract
