"""The device's tracking, sampling and raycast where their code branches and the other tests do not
go (inputs and conditions: tests/track_edge_cases.py, checked on the CPU by
tests/test_track_edges_cpu.py): volumes whose last brick of every axis is partly filled, dense and in
the voxel hash with whole blocks absent; a slab whose index offset is no multiple of 8 and a slab
whose high face is the volume's; and frames with more pixels than one grid of the linearise kernels
has lanes, so that lanes go round the grid-stride loop twice and the finish adds 4 n_cu partial
records.  Every comparison is one the other tracking and raycast tests make, against the same NumPy
restatements on the handle's own state: codes, residuals, depth, colour and samples byte-identical,
counts equal, sums within inliers 2^-52 sum|term|, normals within 1e-6, pose steps within STEP_TOL.
Volumes <= 64x48x40, frames 71x53 but for the large ones (416 x 640 on an MI355X)."""
import numpy as np
import pytest

import icp_color_ref as C
import icp_ref as I
import raycast_ref as R
import sdf_ref as S
import track_edge_cases as E
from test_raycast_gpu import MIN_HITS, check, same
from test_track_color_gpu import follow as rgbd_follow
from test_track_gpu import follow as icp_follow
from test_track_sdf_gpu import STEP_TOL, check_linearize, follow as sdf_follow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gf():
    from tsdf_amd import grid_fusion
    return grid_fusion


@pytest.fixture(scope="module")
def hf():
    from tsdf_amd import hash_fusion
    return hash_fusion


@pytest.fixture(scope="module")
def tr():
    from tsdf_amd import tracking
    return tracking


def make(gf, hf, name, st=None):
    """A fresh handle of the named extent holding st (default: its cut of the corner state).  The
    table takes the voxels of the blocks that are kept through add_entries."""
    dims, slab = E.VOLUMES[name]
    (t, w, c), off = E.state(name) if st is None else st
    if name == "ragged_hash":
        ht = hf.HashTable(E.bounds(dims), I.VS, 1 << 12)
        assert tuple(ht._vol_dim) == dims and np.array_equal(ht._vol_origin, I.ORIGIN)
        keep = E.kept_voxels(dims)
        ht.add_entries(np.argwhere(keep), tsdf=t[keep], weight=w[keep], color=c[keep])
        return ht
    vol = gf.TSDFVolume(E.bounds(dims), I.VS, slab=slab)
    assert tuple(vol._vol_dim) == dims and np.array_equal(vol._vol_origin, I.ORIGIN)
    assert tuple(vol._local_dim) == t.shape and int(vol.x_index[0]) == off[0]
    vol.set_state(t, w, c)
    return vol


@pytest.fixture(scope="module")
def handles(gf, hf):
    """name -> handle holding track_edge_cases.state(name), built on first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make(gf, hf, name)
        return made[name]

    return get


@pytest.mark.parametrize("name", list(E.VOLUMES))
def test_handles_hold_the_intended_state(handles, name):
    """get_state() is the cut of the corner state; the table returns (1, 0, 0) where a block was left out."""
    want = {"ragged": (61, 45, 37), "ragged_holed": (61, 45, 37), "ragged_hash": (61, 45, 37), "slab": (34, 45, 37),
            "high_slab": (32, 48, 40)}[name]
    got = handles(name).get_state()
    (t, w, c), _ = E.state(name)
    assert got[0].shape == want
    for a, b in zip(got, (t, w, c)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if name == "ragged_hash":
        gone = ~E.kept_voxels(want)
        assert gone.sum() > 10000 and (got[0][gone] == 1).all() and not got[1][gone].any() and not got[2][gone].any()


# ---- sample at the faces ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.SAMPLED)
def test_sample_at_the_faces_equals_the_restatement(handles, name):
    n = E.assert_sample_conditions(name)
    print(name, n)
    want, _ = E.sample_ref(name)
    got = handles(name).sample(E.sample_points(name))
    for a, b, what in zip(got, want, ("sdf", "grad", "code")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def test_sample_of_the_ragged_hash_equals_the_dense_handles(handles):
    """The table against the dense volume with weight 0 in the absent blocks: the same codes
    everywhere, the same values wherever the dense code is not 3 (test_track_sdf_gpu.py's holed
    comparison); and against the dense volume without holes wherever the table's own code is not 3."""
    P = E.sample_points("ragged_hash")
    h, d, full = (handles(k).sample(P) for k in ("ragged_hash", "ragged_holed", "ragged"))
    assert np.array_equal(h[2], d[2])
    sel = d[2] != 3
    assert sel.sum() > 1000 and (~sel).sum() > 500
    for a, b in zip(h, d):
        assert np.array_equal(a[sel], b[sel])
    for a, b in zip(h, full):
        assert np.array_equal(a[h[2] != 3], b[h[2] != 3])
    assert ((h[2] == 3) & (full[2] != 3)).sum() > 1000


# ---- SDF linearise and track ------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", list(E.VOLUMES))
def test_sdf_linearize_on_the_edge_volumes(handles, tr, name, stride):
    """The every-code frame (71x53) on each handle against the restatement with the handle's index
    offset.  Conditions, on the reference: every code but 1; the slab's x faces with 140 (all
    inliers) / 208 / 35 / 58 pixels in cells dims - 2 / dims - 1 / 0 / -1, the ragged +y face with
    133 / 257."""
    counts, faces = E.assert_linearize_conditions(name, stride)
    print(name, "stride", stride, counts.tolist(), faces)
    frame, K, M, G = S.every_code_case()
    got = tr.sdf_linearize(handles(name), frame, K, M, G, stride=stride, **S.EVERY_CODE)
    check_linearize(got, E.linearize_ref(name, stride), f"{name} stride {stride}")


@pytest.mark.parametrize("name", ["ragged", "ragged_hash", "slab"])
def test_sdf_track_on_the_edge_volumes(handles, tr, name):
    """track(method="sdf") of the corner frame follows the restatement chain on the handle's own
    extent, is not lost and keeps >= 1000 inliers (the slab: 2320 with its 34 voxels)."""
    frame, K, g = E.track_frame()
    (t, w, _), off = E.state(name)
    obj = handles(name)
    pose, info = obj.track(frame, K, g, method="sdf", return_info=True)
    sdf_follow(obj, tr, frame, K, g, info, (t, w), index_offset=off)
    assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
    ref = S.linearize(frame, K, info["trajectory"][info["iterations"] - 1], g, t, w, index_offset=off, **S.CORNER_VOL)
    print(f"{name}: {info['status']} after {info['iterations']}, inliers {info['inliers']}")
    assert info["status"] != "lost" and ref["inliers"] >= 1000 and info["inliers"] == ref["inliers"]
    if name == "ragged_hash":
        _, dense = handles("ragged_holed").track(frame, K, g, method="sdf", return_info=True)
        assert dense["inliers"] == info["inliers"] and dense["status"] == info["status"]
        assert np.abs(dense["trajectory"] - info["trajectory"]).max() <= STEP_TOL


# ---- raycast and ICP --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_hash", "slab"])
def test_raycast_of_the_ragged_hash_and_the_unaligned_slab(gf, hf, handles, name, monkeypatch):
    """The corner state from two poses in the manner of raycast_ref.ragged_poses, and from one pose
    outside each high face; then the ellipsoid in the same extent from the high-face poses.  Each
    equals the reference with the handle's index offset and is byte-identical with TSDF_RAY_SKIP=0.
    At least MIN_HITS rays hit, except where the corner is seen through a high face: its planes are
    then seen from behind (0 .. 458 hits); the ellipsoid is what those poses hit."""
    (st, off), (est, _) = E.state(name), E.ellipsoid(name)
    corner, ball = handles(name), make(gf, hf, name, (est, off))
    monkeypatch.setenv("TSDF_RAY_SKIP", "0")
    brute_corner, brute_ball = make(gf, hf, name), make(gf, hf, name, (est, off))
    faces = R.high_face_poses(*E.box(name))
    cases = [(corner, brute_corner, st, I.MODEL_K, p, I.Z_FAR, MIN_HITS, k) for k, p in E.corner_poses().items()]
    cases += [(corner, brute_corner, st, E.K_FACE, p, E.FACE_Z_FAR, None, "corner " + k) for k, p in faces.items()]
    cases += [(ball, brute_ball, est, E.K_FACE, p, E.FACE_Z_FAR, MIN_HITS, "ellipsoid " + k) for k, p in faces.items()]
    for obj, brute, state, K, pose, z_far, min_hits, label in cases:
        got, ref = check(obj, K, pose, state=state, off=off, z_far=z_far, min_hits=min_hits)
        print(name, label, "hits", int((ref[0] != 0).sum()))
        every = brute.raycast(K, pose, I.MODEL_HW, z_far=z_far)
        for u, v in zip(got, every):
            assert u.tobytes() == v.tobytes(), label


@pytest.mark.parametrize("name", ["ragged_hash", "slab"])
def test_icp_and_rgbd_track_on_the_edge_volumes(handles, tr, name):
    """track() and track(color_im=...) follow test_track_gpu.py's and test_track_color_gpu.py's
    restatement chains.  The chains run on the handle's own model maps, as there -- and those maps
    equal raycast_ref's with the handle's index offset (depth and colour to the byte, normals within
    1e-6).  Neither track is lost.  The colour weight is the one test_track_edges_cpu.py found to keep
    cond(A) below the chain's 5e2 on both cuts."""
    frame, K, g = E.track_frame()
    rgb = C.plane_render()[1]
    (t, w, c), off = E.state(name)
    obj = handles(name)
    same(obj.raycast(K, g, frame.shape, z_far=I.Z_FAR),
         R.raycast(t, w, c, I.ORIGIN, I.VS, K, g, frame.shape, 0.0, I.Z_FAR, I.VS, index_offset=off))
    pose, info = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True)
    d, _ = icp_follow(obj, tr, frame, K, g, I.Z_FAR, info)
    assert (d > 0).sum() >= 2000 and info["status"] != "lost" and info["inliers"] >= 1000
    assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
    pose, cinfo = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True, color_im=rgb, color_weight=E.EDGE_COLOR_WEIGHT)
    rgbd_follow(obj, tr, frame, rgb, K, g, I.Z_FAR, cinfo, color_weight=E.EDGE_COLOR_WEIGHT)
    print(f"{name}: icp {info['status']} after {info['iterations']}, inliers {info['inliers']}; rgbd {cinfo['status']} after "
          f"{cinfo['iterations']}, inliers {cinfo['inliers']}, colour inliers {cinfo['color_inliers']}")
    assert cinfo["status"] != "lost" and cinfo["inliers"] >= 1000 and cinfo["color_inliers"] >= 100


# ---- more than one grid of lanes --------------------------------------------------------------------
@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def corner(gf):
    vol = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    assert tuple(vol._vol_dim) == I.SHAPE
    vol.set_state(*I.corner_state())
    return vol


@pytest.fixture(scope="module")
def holed_hash(hf):
    """The whole corner volume in a table with test_track_sdf_gpu.py's blocks left out."""
    t, w, c = E.holed_corner_state()
    keep = E.kept_voxels(I.SHAPE)
    ht = hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12)
    ht.add_entries(np.argwhere(keep), tsdf=t[keep], weight=w[keep], color=c[keep])
    return ht


def test_the_large_frame_is_more_than_one_grid(n_cu):
    h, w = E.large_hw(n_cu)  # (fails above 1024 pixels of width: these tests do not grow with the hardware)
    # tsdf_track.hip's linearize_grid launches min(ceil(su sv / 256), 4 n_cu) workgroups of 256 lanes
    assert h * w > 4 * 256 * n_cu and h == 416 and w <= 1024
    assert -(-(h * w) // 256) > 4 * n_cu


@pytest.mark.parametrize("kind", ["u16", "f64"])
@pytest.mark.parametrize("handle", ["dense", "holed hash"])
def test_large_sdf_linearize_equals_the_restatement(corner, holed_hash, tr, n_cu, handle, kind):
    """416 x W (640 on 256 compute units) at stride 1: the lanes' second trip holds >= 100 inliers and
    >= 20 of each of codes 2 .. 5 on the reference; two calls give the same bytes."""
    frame, K, M, G = E.large_sdf_case(n_cu)
    ref = E.large_sdf_ref(n_cu, handle != "dense")
    tail = E.assert_second_trip(ref["code"], n_cu, 6, (2, 3, 4, 5))
    print(f"{handle} {kind}: {frame.shape}, second trip codes 0..6 {tail.tolist()}")
    obj = corner if handle == "dense" else holed_hash
    f = frame if kind == "u16" else frame.astype(np.float64) / 1000.0
    got = tr.sdf_linearize(obj, f, K, M, G, **S.EVERY_CODE)
    check_linearize(got, ref, f"large {handle} {kind}")
    again = tr.sdf_linearize(obj, f, K, M, G, **S.EVERY_CODE)
    assert again["sums"].tobytes() == got["sums"].tobytes() and again["residual"].tobytes() == got["residual"].tobytes()


def test_large_sdf_linearize_at_stride_2(corner, tr, n_cu):
    """A frame twice as wide and as high at stride 2: as many lanes, u and v from the lane index
    through the stride."""
    frame, K, M, G = E.large_sdf_case(n_cu, 2)
    ref = E.large_sdf_ref(n_cu, False, 2)
    E.assert_second_trip(ref["code"], n_cu, 6, (2, 3, 4, 5), stride=2)
    assert frame.shape == (832, 2 * E.large_hw(n_cu)[1])
    check_linearize(tr.sdf_linearize(corner, frame, K, M, G, stride=2, **S.EVERY_CODE), ref, "large stride 2")


def test_large_icp_linearize_equals_the_restatement(corner, tr, n_cu):
    """tsdf_icp_linearize and tsdf_icp_linearize_rgbd on the large frame against the 61x83 maps of the
    device raycast from the pitched model pose, as test_linearize_131x97_second_trip_of_the_finish
    compares them; both halves have >= 100 inliers in the second trip, and two calls give the same
    bytes.  The restatements of this size take 0.12 s (geometry) and 0.10 s (colour) on the CPU."""
    frame, rgb, K, M, P = E.large_icp_case(n_cu)
    d, n, c = corner.raycast(I.MODEL_K, P, I.MODEL_HW, z_far=I.Z_FAR)
    same((d, n, c), E.pitched_model_maps())
    geo, col = E.large_icp_refs(n_cu, (d, n, c))
    gt = np.bincount(E.second_trip(geo["code"], n_cu), minlength=7)
    ct = np.bincount(E.second_trip(col["code"], n_cu), minlength=6)
    print(f"second trip: geometry codes 0..6 {gt.tolist()}, colour codes 0..5 {ct.tolist()}")
    assert gt[6] >= 100 and ct[5] >= 100
    old = tr.icp_linearize(frame, K, M, d, n, I.MODEL_K, P)
    got = tr.icp_linearize_rgbd(frame, rgb, K, M, d, n, c, I.MODEL_K, P)
    for res in (old, got):
        assert res["code"].tobytes() == geo["code"].tobytes()
        assert res["residual"].tobytes() == geo["resid"].tobytes()
        assert (res["inliers"], res["candidates"]) == (geo["inliers"], geo["candidates"])
    assert got["color_code"].tobytes() == col["code"].tobytes()
    assert got["color_residual"].tobytes() == col["resid"].tobytes()
    assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
    for label, sums, ref in (("icp_linearize", old["sums"], geo), ("rgbd geometry", got["sums"], geo),
                             ("rgbd colour", got["color_sums"], col)):
        bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
        err = np.abs(sums - ref["sums"])
        print(f"large {label}: inliers {ref['inliers']}, max |sum - fsum| / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()
    assert old["sums"].tobytes() == got["sums"].tobytes()
    old2 = tr.icp_linearize(frame, K, M, d, n, I.MODEL_K, P)
    got2 = tr.icp_linearize_rgbd(frame, rgb, K, M, d, n, c, I.MODEL_K, P)
    assert old2["sums"].tobytes() == old["sums"].tobytes()
    assert got2["sums"].tobytes() == got["sums"].tobytes() and got2["color_sums"].tobytes() == got["color_sums"].tobytes()


def test_large_sdf_track_follows_the_restatement(corner, tr, n_cu):
    """Two iterations on the large frame: the finish solves and updates from 4 n_cu partial records.
    About 1.7e5 inliers at cond(A) ~ 40: N 2^-52 ~ 4e-11 relative on the sums moves the step by
    ~ 1e-10, within STEP_TOL."""
    frame, K, g = E.large_track_case(n_cu)
    pose, info = corner.track(frame, K, g, method="sdf", max_iter=2, return_info=True)
    assert info["iterations"] == 2 and info["inliers"] >= 100000
    sdf_follow(corner, tr, frame, K, g, info, I.corner_state()[:2], device_counts=False, max_iter=2)
    assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
