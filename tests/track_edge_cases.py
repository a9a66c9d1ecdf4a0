"""Inputs shared by tests/test_track_edges_cpu.py and tests/test_track_edges_gpu.py: the corner state
(tests/icp_ref.py) cut into volumes whose last bricks are partly filled and into slabs with an index
offset, sample points on and around every face of such a handle, and frames with more pixels than
one grid of the linearise kernels has lanes.  Everything here is NumPy: the references are the
restatements (sdf_ref, icp_ref, icp_color_ref, raycast_ref), computed once per process and shared;
callers must leave the returned arrays unchanged.  The conditions on the inputs (which codes and
which faces the reference reaches) are counted here and asserted by both test modules."""
import functools

import numpy as np

import icp_color_ref as C
import icp_ref as I
import raycast_ref as R
import sdf_ref as S

# name -> (dims of the whole volume, slab (x0, x1) or None)
RAGGED = (61, 45, 37)
VOLUMES = {"ragged": (RAGGED, None), "ragged_holed": (RAGGED, None), "ragged_hash": (RAGGED, None),
           "slab": ((64, 45, 37), (19, 53)), "high_slab": (I.SHAPE, (32, 64))}
SAMPLED = ("ragged", "ragged_hash", "slab", "high_slab")  # the four handles of the sample and linearise tests
MIN_COUNT = 20


def bounds(dims):
    """vol_bnds whose ceil(extent / VS) is `dims`, from the corner scene's origin."""
    lo = I.ORIGIN.astype(np.float64)
    return np.stack([lo, lo + (np.asarray(dims, dtype=np.float64) - 0.5) * I.VS], axis=1)


def kept_voxels(dims):
    """(dims) bool: False in the whole 8^3 blocks the holed handles leave out (test_track_sdf_gpu's
    `holed` rate and seed)."""
    nb = [(s + 7) // 8 for s in dims]
    drop = np.random.default_rng(9).random(nb) < 0.25
    return ~np.repeat(np.repeat(np.repeat(drop, 8, 0), 8, 1), 8, 2)[:dims[0], :dims[1], :dims[2]]


@functools.lru_cache(maxsize=None)
def state(name):
    """((tsdf, weight, colour) of the handle's own extent, index offset): what get_state() must return.
    ragged_holed is the dense volume with weight 0 in the blocks left out; ragged_hash the table after
    add_entries of the voxels of the other blocks (no entry: tsdf 1, weight 0, colour 0)."""
    dims, slab = VOLUMES[name]
    x0, x1 = slab or (0, dims[0])
    t, w, c = (np.ascontiguousarray(a[x0:x1, :dims[1], :dims[2]]) for a in I.corner_state())
    if name in ("ragged_holed", "ragged_hash"):
        keep = kept_voxels(dims)
        w = w * keep
        if name == "ragged_hash":
            t, c = np.where(keep, t, np.float32(1)), np.where(keep, c, np.float32(0))
    return (t, w, c), (x0, 0, 0)


def holed_corner_state():
    """The whole corner volume with the same blocks never observed (dense: weight 0 there)."""
    t, w, c = I.corner_state()
    return t, w * kept_voxels(I.SHAPE), c


# ---- sample points on the faces ---------------------------------------------------------------------
def face_positions(n):
    """The local index positions of the sweep on an axis of n voxels: around cell -1 | 0, a brick
    boundary, the last valid cell n - 2 and the first invalid one n - 1."""
    return [-1.0, -2.0 ** -20, 0.0, 0.5, 6.999, 7.0, 7.5, 8.0, n - 2.0, n - 2 + 0.75, n - 1 - 2.0 ** -10, n - 1.0, n - 0.5]


def interior_positions(n):
    """About 30 positions inside an axis of n voxels, some in cells with (l & 7) == 7."""
    b = np.array([7.5, 15.25, 23.75, 31.5])
    return np.concatenate([np.linspace(0.3, n - 1.4, 26), b[b < n - 1.1]])


@functools.lru_cache(maxsize=None)
def sample_points(name):
    """World points (N, 3) f64 for the handle: per axis and face position a sweep of the other two
    axes, the eight corners, and 500 seeded random points in a box one voxel larger than the handle."""
    (t, _, _), off = state(name)
    dims = t.shape
    q = []
    for d in range(3):
        a, b = [interior_positions(dims[e]) for e in range(3) if e != d]
        A, B = (x.ravel() for x in np.meshgrid(a, b, indexing="ij"))
        for f in face_positions(dims[d]):
            cols = [A, B]
            cols.insert(d, np.full(A.shape, f))
            q.append(np.stack(cols, axis=1))
    q.append(np.array([[i, j, k] for i in (0, dims[0] - 1) for j in (0, dims[1] - 1) for k in (0, dims[2] - 1)], dtype=np.float64))
    q.append(-1.0 + np.random.default_rng(17).random((500, 3)) * (np.array(dims) + 1.0))
    q = np.concatenate(q)
    return I.ORIGIN.astype(np.float64) + (q + np.array(off, dtype=np.float64)) * I.VS


@functools.lru_cache(maxsize=None)
def sample_ref(name):
    """S.sample at sample_points(name) on state(name): (sdf, grad, code), and the local cell index
    l (N, 3) the restatement itself derives from the points rounded to f32."""
    (t, w, _), off = state(name)
    P = sample_points(name)
    out = S.sample(P, t, w, **S.CORNER_VOL, index_offset=off)
    q = ((P - I.ORIGIN.astype(np.float64)) / np.float64(I.VS)).astype(np.float32)
    code, _, _, i0 = S.cell(t, w, q, off)
    assert np.array_equal(code, out[2])
    return out, i0 - np.array(off)


def sample_counts(name):
    """The conditions on the sample points, counted on the reference: the four codes, and per axis the
    points of code >= 4 in the last cell (l = dims - 2), of code 2 at l = dims - 1 and at l = -1."""
    (_, _, code), l = sample_ref(name)
    dims = state(name)[0][0].shape
    n = {"codes": {k: int((code == k).sum()) for k in (2, 3, 4, 6)}}
    for d, ax in enumerate("xyz"):
        n[ax] = {"last cell, code >= 4": int(((code >= 4) & (l[:, d] == dims[d] - 2)).sum()),
                 "dims - 1, code 2": int(((code == 2) & (l[:, d] == dims[d] - 1)).sum()),
                 "-1, code 2": int(((code == 2) & (l[:, d] == -1)).sum())}
    return n


def assert_sample_conditions(name):
    n = sample_counts(name)
    assert set(np.unique(sample_ref(name)[0][2])) == {2, 3, 4, 6}
    assert min(n["codes"].values()) >= MIN_COUNT, (name, n)
    for ax in "xyz":
        assert min(n[ax].values()) >= MIN_COUNT, (name, ax, n)
    return n


# ---- the every-code frame on the edge volumes -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linearize_ref(name, stride):
    frame, K, M, G = S.every_code_case()
    (t, w, _), off = state(name)
    return S.linearize(frame, K, M, G, t, w, stride=stride, index_offset=off, **S.CORNER_VOL, **S.EVERY_CODE)


def face_counts(ref, dims, off, d):
    """Pixels of the linearisation on axis d: code >= 3 in the last cell, code 2 just past it, code
    >= 3 in the first cell, code 2 just before it."""
    code, l = ref["code"], ref["cell"][..., d] - off[d]
    return {"dims - 2": int(((code >= 3) & (l == dims[d] - 2)).sum()), "dims - 1": int(((code == 2) & (l == dims[d] - 1)).sum()),
            "0": int(((code >= 3) & (l == 0)).sum()), "-1": int(((code == 2) & (l == -1)).sum())}


def assert_linearize_conditions(name, stride):
    """Every code but 1 occurs (on the slab every third pixel shows no code 5: its 19 pixels of that
    code at stride 1 all fall between the samples); at stride 1 the faces the every-code frame
    reaches: both x faces of the slab, the +y face of the ragged volumes.  (The frame never reaches the
    z faces: sample_points do.)"""
    ref = linearize_ref(name, stride)
    counts = np.bincount(ref["code"].ravel(), minlength=7)
    absent = {1, 5} if (name, stride) == ("slab", 3) else {1}
    assert {k for k in range(7) if counts[k] == 0} == absent, (name, stride, counts)
    (t, _, _), off = state(name)
    faces = {ax: face_counts(ref, t.shape, off, d) for d, ax in enumerate("xyz")}
    if stride == 1:
        if name == "slab":
            assert min(faces["x"].values()) >= MIN_COUNT, faces
        if name in ("ragged", "ragged_holed", "ragged_hash"):
            assert min(faces["y"]["dims - 2"], faces["y"]["dims - 1"]) >= MIN_COUNT, faces
    return counts, faces


# The colour weight of the RGB-D tracks on the cut volumes: with it the combined systems stay well
# below the cond(A) of 5e2 the pose-step tolerance was derived for (test_track_edges_cpu.py measures it).
EDGE_COLOR_WEIGHT = 0.0005


def track_frame():
    """(frame, K, pose guess) of the SDF and ICP tracks on the edge volumes."""
    from test_track_cpu import corner_starts
    return I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW), I.FRAME_K, corner_starts()[0]


# ---- raycast poses for the corner volume and its cuts ---------------------------------------------------
def corner_poses():
    """In the manner of raycast_ref.ragged_poses: looking along +z from outside the volume (the
    near plane is outside, rays enter through the z = 0 face), and obliquely from beyond the low
    corner towards the corner of the three planes."""
    a = np.eye(4)
    a[:3, 3] = [0.05, -0.05, 0.1]
    return {"front": a, "oblique": R.look_at([-0.75, -0.6, 0.3], [0.25, 0.15, 1.05])}


K_FACE = np.array([[75.0, 0.0, 41.2], [0.0, 75.0, 29.7], [0.0, 0.0, 1.0]])  # test_raycast_gpu.py's, for the high-face poses
FACE_Z_FAR = 3.0


def box(name):
    """(lo, hi) in metres of the handle's own voxel centres."""
    (t, _, _), off = state(name)
    lo = I.ORIGIN.astype(np.float64) + np.array(off) * I.VS
    return lo, lo + (np.array(t.shape) - 1.0) * I.VS


@functools.lru_cache(maxsize=None)
def ellipsoid(name):
    """The handle's extent holding raycast_ref's ellipsoid instead of the corner (tsdf < 0 inside,
    the surface in the outermost bricks of every axis, holes, exact zeros): rays through the high
    faces hit it, which the corner, seen from behind its planes, does not allow.  The hash leaves
    out the same blocks as state('ragged_hash')."""
    (t0, _, _), off = state(name)
    t, w, c = R.ellipsoid_state(t0.shape)
    if name == "ragged_hash":
        keep = kept_voxels(t0.shape)
        t, w, c = np.where(keep, t, np.float32(1)), w * keep, np.where(keep, c, np.float32(0))
    return (t, w, c), off


# ---- more pixels than one grid of lanes -------------------------------------------------------------
LARGE_H = 416
N_CU_MI355X = 256


def grid_lanes(n_cu):
    """tsdf_track.hip's linearize_grid: at most 4 workgroups of 256 lanes per compute unit."""
    return 4 * 256 * n_cu


def large_hw(n_cu):
    w = -(-(grid_lanes(n_cu) + 4096) // LARGE_H)
    if w > 1024:
        raise AssertionError(f"{n_cu} compute units ask for a frame {w} pixels wide: these tests stop at 1024")
    return LARGE_H, w


def large_K(hw, scale=1):
    return np.array([[320.0 * scale, 0.0, hw[1] / 2.0], [0.0, 320.0 * scale, 208.0 * scale], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def large_sdf_case(n_cu, scale=1):
    """(frame u16, K, M, G): the corner from the identity without holes, sdf_ref's every-code M.
    scale 2: twice as wide and as high through twice the focal length, for stride 2."""
    h, w = large_hw(n_cu)
    hw = (h * scale, w * scale)
    K = large_K(hw, scale)
    return I.render(np.eye(4), K, hw, holes=False), K, I.perturbation(np.random.default_rng(5), 0.08, 3.0), np.eye(4)


@functools.lru_cache(maxsize=None)
def large_sdf_ref(n_cu, holed=False, scale=1):
    frame, K, M, G = large_sdf_case(n_cu, scale)
    t, w, _ = holed_corner_state() if holed else I.corner_state()
    return S.linearize(frame, K, M, G, t, w, stride=scale, **S.CORNER_VOL, **S.EVERY_CODE)


def large_track_case(n_cu):
    """(frame u16, K, pose guess): the corner from its true pose on the large frame, first seeded start."""
    from test_track_cpu import corner_starts
    hw = large_hw(n_cu)
    return I.render(I.TRUE_POSE, large_K(hw), hw, holes=False), large_K(hw), corner_starts()[0]


def second_trip(a, n_cu, stride=1):
    """The values of a per-pixel map at the sampled pixels a lane meets on its second trip round the
    grid-stride loop: lane index (v / stride) * su + u / stride >= grid_lanes."""
    s = np.asarray(a)[::stride, ::stride].reshape(-1)
    return s[grid_lanes(n_cu):]


def assert_second_trip(code, n_cu, inlier, others, stride=1):
    """At least 100 inliers and 20 of each other code among the second trip's pixels."""
    tail = np.bincount(second_trip(code, n_cu, stride), minlength=7)
    assert tail[inlier] >= 100 and all(tail[k] >= MIN_COUNT for k in others), tail
    return tail


def pitched_model_pose():
    """The model camera of the large ICP frames: at the origin, pitched 32 degrees down.  The second
    trip is the frame's last rows, which look at the floor plane 32 .. 33 degrees below the axis --
    outside the 61x83 model camera's +-16 degrees unless it looks there."""
    a = np.radians(32.0)
    P = np.eye(4)
    P[:3, :3] = [[1.0, 0.0, 0.0], [0.0, np.cos(a), np.sin(a)], [0.0, -np.sin(a), np.cos(a)]]
    return P


def large_rgb(hw):
    """A deterministic grey image (H, W, 3) u8 for the large frame."""
    v, u = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    g = np.rint(128 + 40 * np.sin(u / 7.0) * np.cos(v / 5.0) + 30 * np.sin((u + 2 * v) / 23.0)).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], axis=-1))


@functools.lru_cache(maxsize=None)
def large_icp_case(n_cu):
    """(frame u16, rgb, K, M, model pose): large_sdf_case's frame, seen from the identity, against
    model maps raycast from pitched_model_pose(); M is that pose's inverse after the 2 cm / 1 degree
    offset of the linearise tests."""
    frame, K, _, _ = large_sdf_case(n_cu)
    P = pitched_model_pose()
    return frame, large_rgb(frame.shape), K, np.linalg.inv(P) @ I.offset_2cm_1deg(), P


def large_icp_refs(n_cu, maps):
    """(geometric, colour) restatements of the large frame against maps = (depth, normals, colours)."""
    frame, rgb, K, M, P = large_icp_case(n_cu)
    d, n, c = maps
    return (I.linearize(frame, K, M, d, n, I.MODEL_K, P), C.linearize_color(frame, rgb, K, M, d, c, I.MODEL_K))


@functools.lru_cache(maxsize=None)
def pitched_model_maps():
    """The reference raycast of the corner state from pitched_model_pose(): 61x83 through MODEL_K."""
    t, w, c = I.corner_state()
    return R.raycast(t, w, c, I.ORIGIN, I.VS, I.MODEL_K, pitched_model_pose(), I.MODEL_HW, 0.0, I.Z_FAR, I.VS)
