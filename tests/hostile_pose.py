"""Inputs shared by tests/test_hostile_pose_cpu.py, tests/test_hostile_pose_gpu.py and
tools/gen_golden.py (the "hostile_pose" section): the poses, intrinsics and query points a SLAM front
end hands over when it has lost tracking -- NaN, infinities, huge translations, singular and zero
matrices, a camera centre on a voxel centre, matrices that are no rigid motion (scaled, sheared,
mirrored), negative, zero, tiny, huge and non-finite focal lengths and principal points -- on a small
ragged volume (40 x 24 x 20 voxels, at 4 cm and at 0.0625 m) seen through 80 x 60 images.  Everything
here is NumPy and runs on the CPU; callers must leave the returned arrays unchanged (they are cached).

A pose case is given as the rows of inv(cam_pose) ("rows": what the C-ABI takes) and, where a camera
pose exists whose inverse the wrapper can form, as that pose ("pose": what the drop-in classes
take; the reference and the wrapper both call np.linalg.inv on it).  An intrinsics case is a K for
the good pose.  `expect` says what the case must do by itself on a preloaded volume, in the oracle:
"noop" changes no voxel, "active" at least MIN_ACTIVE, "any" is whatever the reference does.

The reference's rule for a pixel (grid_fusion.py:183-197, 273-277): np.rint(...).astype(int) of a NaN
or an out-of-range value is the most negative int64, which fails 0 <= u; so a voxel whose u, v or z
is NaN, or whose u or v is infinite, is never updated.

Why no gather or store of a kernel can leave its buffer on these inputs:
  integrate   a frame with a non-finite row or intrinsic, or with z the same non-positive number
              everywhere, is integrated as the zero matrix and culled outright (frame_is_dead,
              tsdf_pixel.h; prepare_batch); for the rest the fast pixel is taken only past zmin
              (pixel_fixed: the 16-bit fields cannot alias, 1 / z is finite) and tested against
              (W - 1, H - 1) as packed u16, the exact pixel is the saturating v_cvt_i32_f64 of rint(.)
              tested unsigned against W and H; the cull reads the pyramid at texels clamped to the image
              (fminf / fmaxf drop NaN) and rejects a brick otherwise;
  frustum     no gather depends on the pose or K;
  raycast, sample, SDF linearise, merge
              floor_i clamps to +-1e9 (NaN becomes -1e9) before the cast, the offset (<= 2^24) is
              subtracted in int without overflow, and sdf_cell / load_cell answer "outside" unless
              0 <= l <= dims - 2; the colour voxel is clamped into the volume; every march advances k
              by at least 1 up to (z_far - z_near) / z_step;
  ICP         the model pixel is cast only after 0 <= rint(x) <= W - 1 held in float (false for NaN).
The restatements assert the same on every gather (raycast_ref.assert_in_range, clamp_index)."""
import functools

import numpy as np

HW = (60, 80)  # (H, W)
K = np.array([[60.0, 0.0, 39.5], [0.0, 62.0, 29.5], [0.0, 0.0, 1.0]])
# name -> (bounds, voxel size); both give DIMS
VOLUMES = {"4cm": ([[-0.8, 0.8], [-0.48, 0.48], [0.0, 0.8]], 0.04),
           "p2": ([[-1.25, 1.25], [-0.75, 0.75], [0.0, 1.25]], 0.0625)}
DIMS = (40, 24, 20)
MIN_ACTIVE, MIN_GOOD = 100, 1000
NAN, INF = float("nan"), float("inf")


def volume_scale(vol):
    """Lengths of the 0.0625 m volume are those of the 4 cm one times this."""
    return VOLUMES[vol][1] / 0.04


# ---- good frames ------------------------------------------------------------------------------------
def good_rows(vol="4cm", f=0):
    """inv(cam_pose) of good frame f, written down exactly (no np.linalg.inv): a camera 0.6 m (times the
    volume's scale) in front of the z = 0 face, looking along +z, turned f-dependent small angles
    about y and x and shifted sideways."""
    s = volume_scale(vol)
    a, b = np.radians(3.0 * ((f % 5) - 2)), np.radians(2.0 * ((f % 3) - 1))
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1.0, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Rx @ Ry  # world -> camera rotation
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.array([0.03 * ((f % 4) - 1.5), 0.02 * ((f % 3) - 1), 0.6]) * s
    return T


def good_pose(vol="4cm", f=0):
    T = good_rows(vol, f)
    P = np.eye(4)
    P[:3, :3] = T[:3, :3].T
    P[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return P


@functools.lru_cache(maxsize=None)
def depth_mm(vol="4cm", f=0):
    """u16 millimetres: a wavy surface around 1.0 m (times the volume's scale) from the camera, inside
    the volume; a block of invalid (0) pixels; every value a whole millimetre, so that the u16 and the
    f64 form of the frame (mm / 1000.) carry the same metres."""
    H, W = HW
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 1000.0 + 150.0 * np.sin(0.11 * u + 0.3 * f) * np.cos(0.13 * v) + 40.0 * ((u // 8 + v // 8 + f) % 3)
    d = np.rint(d * volume_scale(vol)).astype(np.uint16)
    d[5:9, 60:70] = 0
    return d


def depth_m(vol="4cm", f=0):
    return depth_mm(vol, f).astype(np.float64) / 1000.0


@functools.lru_cache(maxsize=None)
def rgb(f=0):
    H, W = HW
    v, u = np.meshgrid(np.arange(H) // 4, np.arange(W) // 4, indexing="ij")
    return np.ascontiguousarray(np.stack([(37 * u + 11 * v + 17 * f) % 256, (29 * v + 5 * f + 40) % 256,
                                          (13 * u + 53 * v + 90) % 256], axis=-1).astype(np.uint8))


# ---- pose cases -------------------------------------------------------------------------------------
def _with(T, r, c, value):
    T = T.copy()
    T[r, c] = value
    return T


def _about_centre(A, vol):
    """A applied in camera space about the point the good camera sees the volume's middle at
    (0, 0, 1.0 m times the scale): rows [A R | A t + (I - A) c0]."""
    T = good_rows(vol)
    c0 = np.array([0.0, 0.0, 1.0]) * volume_scale(vol)
    out = np.eye(4)
    out[:3, :3] = A @ T[:3, :3]
    out[:3, 3] = A @ T[:3, 3] + (np.eye(3) - A) @ c0
    return out


def _centre_rows():
    """Axis-aligned, the camera centre on the centre of voxel (20, 12, 10) of the 0.0625 m volume:
    every voxel's camera coordinates are exact multiples of 2^-4."""
    T = np.eye(4)
    o, vs = np.array([b[0] for b in VOLUMES["p2"][0]]), VOLUMES["p2"][1]
    T[:3, 3] = -(o + vs * np.array([20, 12, 10]))
    return T


def _rigid_inverse(T):
    P = np.eye(4)
    P[:3, :3] = T[:3, :3].T
    P[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return P


@functools.lru_cache(maxsize=None)
def pose_cases():
    """name -> dict(vol, rows (4,4) inv(cam_pose), pose (4,4) or None, expect)."""
    g = good_rows("4cm")
    gp = good_pose("4cm")
    out = {}

    def add(name, rows, pose, expect, vol="4cm"):
        out[name] = dict(vol=vol, rows=np.ascontiguousarray(rows, dtype=np.float64),
                         pose=None if pose is None else np.ascontiguousarray(pose, dtype=np.float64), expect=expect)

    add("nan_all", np.full((4, 4), NAN), np.full((4, 4), NAN), "noop")
    for k, ax in enumerate("xyz"):
        add("nan_t" + ax, _with(g, k, 3, NAN), _with(gp, k, 3, NAN), "noop")
    add("inf_tz_pos", _with(g, 2, 3, INF), _with(gp, 2, 3, INF), "noop")
    add("inf_tz_neg", _with(g, 2, 3, -INF), _with(gp, 2, 3, -INF), "noop")
    for label, t in (("1e30", 1e30), ("1e39", 1e39), ("1e300", 1e300), ("1e307", 1e307)):
        # 1e30 is finite in f32; 1e39 is infinite in the cull's f32; at 1e307 the folded T * fx overflows
        rows = g.copy()
        rows[:3, 3] = [t, -t, t]
        add("huge_" + label, rows, _rigid_inverse(rows), "noop")
    rows = g.copy()
    rows[2, :] = 0.0
    add("zero_row3", rows, None, "noop")
    add("zero_all", np.zeros((4, 4)), np.zeros((4, 4)), "noop")
    c = _centre_rows()
    add("centre", c, _rigid_inverse(c), "active", vol="p2")
    shear = np.array([[1.0, 0.35, 0.0], [0.0, 1.0, 0.25], [0.2, 0.0, 1.0]])
    for name, A in (("scale_2", np.diag([2.0, 2.0, 2.0])), ("scale_half", np.diag([0.5, 0.5, 0.5])),
                    ("scale_1_2_half", np.diag([1.0, 2.0, 0.5])), ("shear", shear), ("mirror", np.diag([-1.0, 1.0, 1.0]))):
        rows = _about_centre(A, "4cm")
        add(name, rows, np.linalg.inv(rows), "active")
    assert np.linalg.det(out["mirror"]["rows"][:3, :3]) < 0
    return out


# ---- intrinsics cases -------------------------------------------------------------------------------
def _K(**kw):
    k = K.copy()
    idx = {"fx": (0, 0), "fy": (1, 1), "cx": (0, 2), "cy": (1, 2), "skew": (0, 1), "k22": (2, 2)}
    for name, v in kw.items():
        k[idx[name]] = v
    return k


@functools.lru_cache(maxsize=None)
def intrinsics_cases():
    """name -> dict(K, expect); the pose is the good one."""
    out = {"fx_neg": (_K(fx=-60.0), "active"), "fy_neg": (_K(fy=-62.0), "active"), "fxy_neg": (_K(fx=-60.0, fy=-62.0), "active"),
           "fx_zero": (_K(fx=0.0), "active"), "fx_1e-30": (_K(fx=1e-30), "active"), "fx_1e30": (_K(fx=1e30), "any"),
           "cx_70000": (_K(cx=70000.0), "noop"), "cx_1e30": (_K(cx=1e30), "noop"),
           "skew_k22": (_K(skew=7.5, k22=3.0), "active")}
    for what in ("fx", "cx", "cy"):
        for label, v in (("nan", NAN), ("inf", INF), ("ninf", -INF)):
            out["%s_%s" % (what, label)] = (_K(**{what: v}), "noop")
    return {k: dict(K=v[0], expect=v[1]) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def frame_cases():
    """Every integrate case as one table: name -> dict(vol, K, rows, pose, expect).  Pose cases keep K,
    intrinsics cases the good pose (whose rows and pose are exact inverses of each other)."""
    out = {}
    for name, c in pose_cases().items():
        out[name] = dict(c, K=K)
    for name, c in intrinsics_cases().items():
        out[name] = dict(vol="4cm", K=c["K"], rows=good_rows("4cm"), pose=good_pose("4cm"), expect=c["expect"])
    # the camera on a voxel centre with a focal length that turns the x == 0 plane's 0 * fx into NaN
    # (fx infinite) or leaves that plane alone in the image (fx = 1e30)
    centre = pose_cases()["centre"]
    out["centre_fx_inf"] = dict(centre, K=_K(fx=INF), expect="noop")
    out["centre_fx_1e30"] = dict(centre, K=_K(fx=1e30), expect="any")
    return out


def forms(case):
    """The forms a case is driven in: "rows" always, "pose" where a camera pose exists."""
    return ("rows", "pose") if case["pose"] is not None else ("rows",)


def case_rows(case, form):
    """inv(cam_pose) as the form delivers it: the rows themselves, or np.linalg.inv of the pose -- which
    raises numpy.linalg.LinAlgError for the zero matrix, as in the reference."""
    return case["rows"] if form == "rows" else np.linalg.inv(case["pose"])


# ---- sequences --------------------------------------------------------------------------------------
PRELOAD = 2  # good frames integrated before a single hostile frame


def batch_rows(vol, n, at, hostile_rows):
    """(n, 4, 4) rows of good frames PRELOAD .. with `hostile_rows` as frame `at`."""
    T = np.stack([good_rows(vol, PRELOAD + f) for f in range(n)])
    T[at] = hostile_rows
    return T


def batch_images(vol, n):
    """(depth u16 (n,H,W), rgb (n,H,W,3)) of the frames of batch_rows."""
    return (np.stack([depth_mm(vol, PRELOAD + f) for f in range(n)]), np.stack([rgb(PRELOAD + f) for f in range(n)]))


BATCHES = ((8, 3), (32, 17))  # (frames, index of the hostile frame)


# ---- the oracle over these inputs -------------------------------------------------------------------
def new_oracle(vol, kind="dense", **kw):
    import oracle as O
    b, vs = VOLUMES[vol]
    o = (O.OracleTSDFVolume if kind == "dense" else O.OracleHashVolume)(np.array(b), vs, **kw)
    assert tuple(int(x) for x in o._vol_dim) == DIMS
    return o


def preload(orc, vol):
    return sum(orc.integrate(rgb(f), depth_m(vol, f), K, None, rows=good_rows(vol, f)) for f in range(PRELOAD))


def oracle_single(name, form, kind="dense", **kw):
    """The preloaded oracle after the case's frame alone: (oracle, voxels the frame changed).  The
    hostile frame carries good frame PRELOAD's images."""
    c = frame_cases()[name]
    orc = new_oracle(c["vol"], kind, **kw)
    preload(orc, c["vol"])
    with np.errstate(all="ignore"):
        n = orc.integrate(rgb(PRELOAD), depth_m(c["vol"], PRELOAD), c["K"], None, rows=case_rows(c, form))
    return orc, n


def oracle_batch(name, form, n, at, kind="dense", **kw):
    """The preloaded oracle after a batch of n frames with the case as frame `at`: (oracle, per-frame
    update counts).  Every frame but `at` is good and uses K; the case's K applies to its frame alone,
    so intrinsics cases are batches of one K each: the GPU tests split them at the frame."""
    c = frame_cases()[name]
    orc = new_oracle(c["vol"], kind, **kw)
    preload(orc, c["vol"])
    T = batch_rows(c["vol"], n, at, case_rows(c, form))
    d, col = batch_images(c["vol"], n)
    counts = []
    with np.errstate(all="ignore"):
        for f in range(n):
            counts.append(orc.integrate(col[f], d[f].astype(np.float64) / 1000.0, c["K"] if f == at else K, None, rows=T[f]))
    return orc, counts


# ---- the same classes for raycast, track and merge, on any scene --------------------------------------
NONRIGID = {"scale_2": np.diag([2.0, 2.0, 2.0]), "scale_half": np.diag([0.5, 0.5, 0.5]), "scale_1_2_half": np.diag([1.0, 2.0, 0.5]),
            "shear": np.array([[1.0, 0.35, 0.0], [0.0, 1.0, 0.25], [0.2, 0.0, 1.0]]), "mirror": np.diag([-1.0, 1.0, 1.0])}


def scene_poses(base, origin, vs):
    """name -> camera pose (4, 4): the pose classes applied to the camera-to-world pose `base` of a
    scene whose volume has the given origin and voxel size (raycast poses, tracking guesses)."""
    base = np.asarray(base, dtype=np.float64)
    out = {"nan_all": np.full((4, 4), NAN)}
    for k, ax in enumerate("xyz"):
        out["nan_t" + ax] = _with(base, k, 3, NAN)
    out["inf_tz_pos"], out["inf_tz_neg"] = _with(base, 2, 3, INF), _with(base, 2, 3, -INF)
    for label, t in (("1e30", 1e30), ("1e39", 1e39), ("1e300", 1e300)):
        q = base.copy()
        q[:3, 3] = [t, -t, t]
        out["huge_" + label] = q
    q = base.copy()
    q[2, :] = 0.0
    out["zero_row3"] = q
    out["zero_all"] = np.zeros((4, 4))
    q = np.eye(4)  # axis-aligned, on the centre of the voxel nearest to the base camera
    q[:3, 3] = np.asarray(origin, dtype=np.float64) + vs * np.rint((base[:3, 3] - np.asarray(origin, dtype=np.float64)) / vs)
    out["centre"] = q
    for name, A in NONRIGID.items():
        q = base.copy()
        q[:3, :3] = base[:3, :3] @ A
        out[name] = q
    return out


def guess_is_rigid(pose, tol=1e-3):
    """The rule the track entry points refuse a guess by (include/tsdf_hip.h): the rotation block is
    orthonormal with determinant +1 within tol; the translation is not looked at."""
    R = np.asarray(pose, dtype=np.float64).reshape(4, 4)[:3, :3]
    with np.errstate(all="ignore"):
        return bool((np.abs(R.T @ R - np.eye(3)) <= tol).all() and abs(np.linalg.det(R) - 1.0) <= tol)


def scene_intrinsics(K0):
    """name -> K (3, 3): the intrinsics classes applied to a scene's K."""
    K0 = np.asarray(K0, dtype=np.float64)

    def mod(**kw):
        k = K0.copy()
        idx = {"fx": (0, 0), "fy": (1, 1), "cx": (0, 2), "cy": (1, 2), "skew": (0, 1), "k22": (2, 2)}
        for name, v in kw.items():
            k[idx[name]] = v
        return k

    out = {"fx_neg": mod(fx=-K0[0, 0]), "fy_neg": mod(fy=-K0[1, 1]), "fxy_neg": mod(fx=-K0[0, 0], fy=-K0[1, 1]), "fx_zero": mod(fx=0.0),
           "fx_1e-30": mod(fx=1e-30), "fx_1e30": mod(fx=1e30), "cx_70000": mod(cx=70000.0), "cx_1e30": mod(cx=1e30),
           "skew_k22": mod(skew=7.5, k22=3.0)}
    for what in ("fx", "cx", "cy"):
        for label, v in (("nan", NAN), ("inf", INF), ("ninf", -INF)):
            out["%s_%s" % (what, label)] = mod(**{what: v})
    return out


def merge_nonrigid(T):
    """name -> src_to_dst: the rigid T with its rotation scaled, sheared and mirrored."""
    out = {}
    for name, A in NONRIGID.items():
        b = np.array(T, dtype=np.float64)
        b[:3, :3] = b[:3, :3] @ A
        out[name] = b
    return out


def merge_far(T):
    b = np.array(T, dtype=np.float64)
    b[:3, 3] = [1e30, -1e30, 1e30]
    return b


# ---- points for sample() ----------------------------------------------------------------------------
POINT_VALUES = {"nan": NAN, "inf": INF, "ninf": -INF, "1e300": 1e300, "-1e300": -1e300, "3e9": 3e9, "-3e9": -3e9,
                "1e9": 1e9, "-1e9": -1e9}
MAX_OFFSET = (1 << 24)  # tsdf_dense_create accepts dims + index_offset <= 2^24 per axis


def sample_points(origin, vs, dims, off=(0, 0, 0)):
    """(names, points (N, 3) f64) for a handle of `dims` voxels at index offset `off`: every value of
    POINT_VALUES in each coordinate in turn -- in voxels of global index space, the world coordinate
    is origin + vs * value -- with the other two coordinates inside the handle; after each hostile point
    a finite neighbour inside the handle."""
    origin, off = np.asarray(origin, dtype=np.float64), np.asarray(off, dtype=np.float64)
    names, pts = [], []
    k = 0
    for label, v in POINT_VALUES.items():
        for a in range(3):
            idx = off + np.rint(np.array(dims) * (0.2 + 0.02 * (k % 30))) + 0.25
            p = origin + vs * idx
            h = p.copy()
            with np.errstate(all="ignore"):
                h[a] = origin[a] + vs * v
            names += ["%s_%s" % (label, "xyz"[a]), "neighbour"]
            pts += [h, p]
            k += 1
    return names, np.array(pts)
