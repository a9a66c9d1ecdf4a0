"""The hostile f64 depth frames of tests/hostile_depth.py on the device: NaN, infinities, negatives,
-0.0, depths too small or too large for f32 and depths at and beyond the u16 range, through every way
into the dense and the hash integrate (against the oracle, which tests/test_hostile_depth_cpu.py pins
to the reference), through the three linearisations and trackers (against their restatements) and
through the frustum bounds (against the oracle and the contract of include/tsdf_hip.h).  Volume
48 x 40 x 24, images 128 x 96 and 126 x 95; tracking on the corner scene's cuts at 64 x 48."""
import numpy as np
import pytest

import hostile_depth as H
import icp_color_ref as C
import icp_ref as I
import oracle as O
import sdf_ref as S
import track_edge_cases as E
from test_track_color_gpu import follow as rgbd_follow
from test_track_edges_gpu import make
from test_track_gpu import follow as icp_follow
from test_track_sdf_gpu import check_linearize, follow as sdf_follow

pytestmark = pytest.mark.gpu
WAYS = ("sync", "deferred", "batch_host", "batch_device")
WEIGHTS = {"one": 1.0, "half": 0.5, "mixed": None}  # mixed: the sequence's own 1, 0.5, 1, ...


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


@pytest.fixture
def knobs(monkeypatch):
    def set_(pipe):
        monkeypatch.setenv("TSDF_BATCH", "8")
        monkeypatch.setenv("TSDF_PIPELINE", pipe)
    return set_


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_state(got, orc, label):
    for a, b, what in zip(got, (orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu), ("tsdf", "weight", "colour")):
        assert not np.isnan(a).any(), (label, what)
        diff = bits(a) != bits(b)
        assert not diff.any(), (label, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def oracle_over(depth, rgb, poses, ow):
    orc = O.OracleTSDFVolume(np.array(H.BOUNDS), H.VS)
    return orc, sum(orc.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f])) for f in range(len(depth)))


def feed(gf, way, depth, rgb, poses, ow, invalid_65535=False):
    """One dense handle given the frames through `way`; returns it synchronised."""
    from tsdf_amd import _ffi
    vol = gf.TSDFVolume(np.array(H.BOUNDS), H.VS, defer=way != "sync")
    assert tuple(int(x) for x in vol._vol_dim) == H.DIMS
    if way in ("sync", "deferred"):
        for f in range(len(depth)):
            vol.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f]))
    elif way == "batch_host":
        vol.integrate_batch(np.stack(depth), np.stack(rgb), H.K, np.linalg.inv(np.stack(poses)), list(ow), invalid_65535=invalid_65535)
    else:
        import torch
        d, c = torch.from_numpy(np.stack(depth)).cuda(), torch.from_numpy(np.stack(rgb)).cuda()
        torch.cuda.synchronize()
        vol.integrate_batch(d.data_ptr(), c.data_ptr(), H.K, np.linalg.inv(np.stack(poses)), list(ow), depth_kind=_ffi.DEPTH_F64_M,
                            hw=depth[0].shape, device_ptrs=True, invalid_65535=invalid_65535)
    vol.sync()
    return vol


# ---- dense integrate --------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("size", list(H.SIZES))
@pytest.mark.parametrize("way", WAYS)
def test_dense_integrate_equals_the_oracle(gf, knobs, way, size, pipe):
    """The 20 frames of the sequence (benign, the 15 classes each over a whole prep tile, the scatter
    frame, all-NaN, all-zero, benign; three poses) with obs_weight 1, 0.5 and alternating: tsdf, weight
    and colour bit for bit, the update count, no list error, no NaN in the state.  The deferred way
    puts two millimetre-exact frames before each: the f64 frame flushes their staged batch."""
    knobs(pipe)
    for wname, ow in WEIGHTS.items():
        if way == "deferred":
            depth, rgb, poses, w = H.deferred_sequence(size)
            w = list(w) if ow is None else [ow] * len(depth)
        else:
            _, depth, rgb, poses, w = H.sequence(size)
            w = list(w) if ow is None else [ow] * len(depth)
        orc, n = oracle_over(depth, rgb, poses, w)
        vol = feed(gf, way, depth, rgb, poses, w)
        st = vol.stats()
        print(way, size, "pipeline", pipe, wname, "updates", st["voxel_updates"], "oracle", n)
        same_state(vol.get_state(), orc, (way, size, pipe, wname))
        assert st["voxel_updates"] == n and st["list_errors"] == 0 and st["frames"] == len(depth)
        vol.close()


@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("size", list(H.SIZES))
def test_each_class_alone_changes_what_the_oracle_says(gf, knobs, size, pipe):
    """A fresh volume per class, the class alone in its region of an otherwise zero frame (the
    coverage frames: every pyramid level of the region's whole tile carries the class and nothing
    else): the update count is the oracle's -- 0 for NaN, -inf, negatives and -0.0, the 28 voxels with
    0 < z <= trunc for the tiny depths whether or not they survive a conversion to f32, 4097 for +inf
    and the far and huge depths -- and so is the state."""
    knobs(pipe)
    counts = H.assert_coverage(size)
    for name in H.CLASSES:
        d, c, P = H.class_frame(size, name, alone=True), H.rgb(size), H.poses()[0]
        orc, n = oracle_over([d], [c], [P], [1.0])
        assert n == counts[name]
        for way in ("sync", "batch_host"):
            vol = feed(gf, way, [d], [c], [P], [1.0])
            st = vol.stats()
            assert st["voxel_updates"] == n, (name, way, st["voxel_updates"], n)
            same_state(vol.get_state(), orc, (name, way))
            assert st["list_errors"] == 0
            vol.close()


@pytest.mark.parametrize("way", ["batch_host", "batch_device"])
def test_invalid_65535_is_a_u16_flag(gf, knobs, way):
    """invalid_65535 with f64 depth masks nothing: 65.535 m stays a depth, as in the oracle without
    any masking."""
    knobs("1")
    for size in H.SIZES:
        _, depth, rgb, poses, w = H.sequence(size)
        orc, n = oracle_over(depth, rgb, poses, w)
        vol = feed(gf, way, depth, rgb, poses, w, invalid_65535=True)
        same_state(vol.get_state(), orc, (way, size))
        assert vol.stats()["voxel_updates"] == n
        masked = np.where(depth == 65.535, 0.0, depth)
        assert oracle_over(masked, rgb, poses, w)[1] < n  # (the mask would have shown)


# ---- hash integrate ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("size", list(H.SIZES))
@pytest.mark.parametrize("way", ["batch", "per_frame"])
def test_hash_integrate_equals_the_dense_handle(gf, hf, knobs, way, size, pipe):
    """The same frames into a table (the fused launch and, with TSDF_PIPELINE=0, the in-line one; one
    batch call, or deferred per-frame calls): the dense handle's state bit for bit (weights 1: the hash
    ignores obs_weight), the oracle's number of observed voxels as entries, the oracle's update count."""
    knobs(pipe)
    _, depth, rgb, poses, _ = H.sequence(size)
    ones = [1.0] * len(depth)
    orc, n = oracle_over(depth, rgb, poses, ones)
    dense = feed(gf, "batch_host", depth, rgb, poses, ones)
    same_state(dense.get_state(), orc, ("dense", size, pipe))
    ht = hf.HashTable(np.array(H.BOUNDS), H.VS, 1 << 12)
    if way == "batch":
        ht.integrate_batch(depth, rgb, H.K, np.linalg.inv(poses))
    else:
        for f in range(len(depth)):
            ht.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=0.5)
    ht.sync()
    for a, b, what in zip(ht.get_state(), dense.get_state(), ("tsdf", "weight", "colour")):
        assert np.array_equal(bits(a), bits(b)), (what, way, size, pipe)
    assert ht.count_num_hash_entries() == int((orc._weight_vol_cpu > 0).sum())
    st = ht.stats()
    assert st["voxel_updates"] == n and st["list_errors"] == 0 and st["bricks_skipped"] == 0


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_hash_keeps_no_block_for_frames_without_a_depth(hf, knobs, pipe):
    """NaN-only, negative-only (and -inf, -0.0) frames on a fresh table: no entry, no block left."""
    knobs(pipe)
    for size, (Hh, W) in H.SIZES.items():
        ht = hf.HashTable(np.array(H.BOUNDS), H.VS, 1 << 12)
        frames = np.stack([np.full((Hh, W), v) for v in (np.nan, H.NAN_NEG, -1.0, -np.inf, -0.0)])
        P = np.stack([H.poses()[f % 3] for f in range(len(frames))])
        ht.integrate_batch(frames, np.stack([H.rgb(size)] * len(frames)), H.K, np.linalg.inv(P))
        assert ht.info()["used"] == 0 and ht.count_num_hash_entries() == 0
        for f in range(len(frames)):
            ht.integrate(H.rgb(size), frames[f], H.K, P[f])
        ht.sync()
        info = ht.info()
        assert info["used"] == 0 and info["entries"] == 0 and ht.stats()["voxel_updates"] == 0
        assert not ht.get_state()[1].any()


# ---- tracking ---------------------------------------------------------------------------------------
HANDLES = ("ragged", "ragged_hash")


@pytest.fixture(scope="module")
def handles(gf, hf):
    made = {}

    def get(name):
        if name not in made:
            made[name] = make(gf, hf, name)
        return made[name]

    return get


def close_sums(got, ref, label):
    """Every sum within N 2^-52 sum|term| of the exact sum: the terms are exact products, only the
    order of the N - 1 additions differs from the restatement's fsum."""
    bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
    err = np.abs(got - ref["sums"])
    assert np.isfinite(got).all() and (err <= bound).all(), (label, float(np.max(err / np.maximum(bound, 1e-300))))


@pytest.mark.parametrize("name", HANDLES)
def test_icp_and_rgbd_linearize_drop_hostile_pixels(handles, tr, name):
    """The 64 x 48 corner frame with ~5 % hostile pixels against the handle's own 83 x 61 model maps:
    both entry points give the restatement's code and residual maps to the byte and its counts; a
    hostile pixel has code 0 in both halves, its left and upper neighbours code 1 in the geometric
    one.  The sums are within the order-of-addition bound of the exact ones, and byte-identical to
    those of the frame with 0 in place of every hostile pixel: such a pixel adds exactly nothing."""
    frame, hostile = H.track_frame("eye")
    rgb, M = H.track_rgb(), I.offset_2cm_1deg()
    d, n, c = handles(name).raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    geo = I.linearize(frame, H.TRACK_K, M, d, n, I.MODEL_K, np.eye(4))
    col = C.linearize_color(frame, rgb, H.TRACK_K, M, d, c, I.MODEL_K)
    assert geo["inliers"] >= 300 and (geo["code"][hostile] == 0).all() and (col["code"][hostile] == 0).all()
    old = tr.icp_linearize(frame, H.TRACK_K, M, d, n, I.MODEL_K, np.eye(4))
    got = tr.icp_linearize_rgbd(frame, rgb, H.TRACK_K, M, d, n, c, I.MODEL_K, np.eye(4))
    zeroed = np.where(hostile, 0.0, frame)
    clean = tr.icp_linearize_rgbd(zeroed, rgb, H.TRACK_K, M, d, n, c, I.MODEL_K, np.eye(4))
    for res in (old, got):
        assert res["code"].tobytes() == geo["code"].tobytes()
        assert res["residual"].tobytes() == geo["resid"].tobytes()
        assert (res["inliers"], res["candidates"]) == (geo["inliers"], geo["candidates"])
        close_sums(res["sums"], geo, name)
    assert got["color_code"].tobytes() == col["code"].tobytes()
    assert got["color_residual"].tobytes() == col["resid"].tobytes()
    assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
    close_sums(got["color_sums"], col, name + " colour")
    assert old["sums"].tobytes() == got["sums"].tobytes() == clean["sums"].tobytes()
    assert got["color_sums"].tobytes() == clean["color_sums"].tobytes()
    for k in ("code", "residual", "color_code", "color_residual"):
        assert got[k].tobytes() == clean[k].tobytes(), k


@pytest.mark.parametrize("name", HANDLES)
def test_sdf_linearize_drops_hostile_pixels(handles, tr, name):
    frame, hostile = H.track_frame("eye")
    (t, w, _), off = E.state(name)
    M = I.offset_2cm_1deg()
    ref = S.linearize(frame, H.TRACK_K, M, np.eye(4), t, w, index_offset=off, **S.CORNER_VOL)
    assert ref["inliers"] >= 300 and (ref["code"][hostile] == 0).all()
    got = tr.sdf_linearize(handles(name), frame, H.TRACK_K, M, np.eye(4))
    check_linearize(got, ref, f"{name} hostile")
    clean = tr.sdf_linearize(handles(name), np.where(hostile, 0.0, frame), H.TRACK_K, M, np.eye(4))
    assert got["sums"].tobytes() == clean["sums"].tobytes() and got["code"].tobytes() == clean["code"].tobytes()
    assert got["residual"].tobytes() == clean["residual"].tobytes()


@pytest.mark.parametrize("method", ["icp", "rgbd", "sdf"])
@pytest.mark.parametrize("name", HANDLES)
def test_track_follows_the_restatement_on_a_hostile_frame(handles, tr, name, method):
    """One track per method on the hostile frame: the restatement chain of the method's own test
    module (every pose step, the counts, status, rms and norms), not lost, a finite pose."""
    from test_track_cpu import corner_starts
    frame, _ = H.track_frame("true")
    (t, w, _), off = E.state(name)
    obj, g, K = handles(name), corner_starts()[0], H.TRACK_K
    if method == "icp":
        pose, info = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True)
        icp_follow(obj, tr, frame, K, g, I.Z_FAR, info)
    elif method == "rgbd":
        rgb = H.track_rgb()
        pose, info = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True, color_im=rgb, color_weight=E.EDGE_COLOR_WEIGHT)
        rgbd_follow(obj, tr, frame, rgb, K, g, I.Z_FAR, info, color_weight=E.EDGE_COLOR_WEIGHT)
        assert info["color_inliers"] >= 100
    else:
        pose, info = obj.track(frame, K, g, method="sdf", return_info=True)
        sdf_follow(obj, tr, frame, K, g, info, (t, w), index_offset=off)
    print(f"{name} {method}: {info['status']} after {info['iterations']}, inliers {info['inliers']}")
    assert info["status"] != "lost" and info["inliers"] >= 1000 and np.isfinite(pose).all()
    assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
    if method != "rgbd":
        et, ea = I.pose_error(pose, I.TRUE_POSE)
        assert et < 5e-3 and ea < 0.5


# ---- frustum bounds ---------------------------------------------------------------------------------
def frustum_call(gf, frames, poses, device):
    if not device:
        return gf.view_frustum_bounds(frames, H.K, poses, return_max_depth=True, return_points=True)
    import torch
    from tsdf_amd import _ffi
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    return gf.view_frustum_bounds(d.data_ptr(), H.K, poses, device_ptrs=True, hw=frames.shape[1:], depth_kind=_ffi.DEPTH_F64_M,
                                  n_frames=len(frames), return_max_depth=True, return_points=True)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("size", list(H.SIZES))
def test_frustum_bounds_with_a_finite_maximum(gf, size, device):
    """Negative-only, tiny-only, 1e300, NaN scattered among valid pixels: the maximum is np.fmax over
    the frame (np.max but for the NaNs), and points and bounds are the oracle's bit for bit."""
    finite, _ = H.frustum_frames(size)
    frames = np.stack(list(finite.values()))
    Hh, W = H.SIZES[size]
    poses = H.frustum_poses(len(frames))
    want_md = np.array([np.fmax.reduce(f, axis=None) for f in frames])
    assert np.isfinite(want_md).all() and want_md[0] == -1.0 and want_md[1] == 5e-324 and want_md[2] == 1e300
    assert all(O.frame_max_depth(f) == m for f, m in zip(frames, want_md))
    b, md, pts = frustum_call(gf, frames, poses, device)
    assert np.array_equal(bits(md), bits(want_md))
    want_pts = np.stack([O.view_frustum(m, Hh, W, H.K, p) for m, p in zip(want_md, poses)])
    assert np.isfinite(want_pts).all()
    assert np.array_equal(bits(pts), bits(want_pts))
    assert np.array_equal(bits(b), bits(O.frustum_bounds(want_md, Hh, W, H.K, poses)))
    # one frame at a time, from the running bounds: the same union
    run = np.zeros((3, 2))
    for f in range(len(frames)):
        run = gf.view_frustum_bounds(frames[f:f + 1], H.K, poses[f:f + 1], init=run)
    assert np.array_equal(bits(run), bits(b))


@pytest.mark.parametrize("device", [False, True])
def test_frustum_bounds_contract_for_nan_frames_and_infinite_maxima(gf, device):
    """include/tsdf_hip.h: a NaN pixel is ignored; a frame without a non-NaN pixel has max depth 0.0
    (its frustum is the camera centre, like an all-invalid u16 frame's); NaN coordinates (0 * inf,
    inf - inf) are reported in frustum_pts and not folded into the bounds; infinite ones are folded."""
    _, contract = H.frustum_frames("vec")
    names, frames = list(contract), np.stack(list(contract.values()))
    Hh, W = H.SIZES["vec"]
    poses = H.frustum_poses(len(frames))
    want_md = np.array([O.frame_max_depth(f) for f in frames])
    assert [want_md[names.index(k)] for k in names] == [np.inf, np.inf, 1.7e308, 0.0, 0.0]
    for sel in (slice(None), slice(3, 5), slice(2, 3), slice(0, 1)):  # all; the NaN frames alone; overflow alone; +inf alone
        b, md, pts = frustum_call(gf, frames[sel], poses[sel], device)
        assert np.array_equal(bits(md), bits(want_md[sel]))
        want_pts = np.stack([O.view_frustum(m, Hh, W, H.K, p) for m, p in zip(want_md[sel], poses[sel])])
        assert np.array_equal(np.isnan(pts), np.isnan(want_pts))
        ok = ~np.isnan(want_pts)
        assert np.array_equal(bits(pts)[ok], bits(want_pts)[ok])
        want_b = O.frustum_bounds(want_md[sel], Hh, W, H.K, poses[sel])
        assert not np.isnan(b).any() and np.array_equal(bits(b), bits(want_b))
    b, _, pts = frustum_call(gf, frames, poses, device)
    # (the case shows all of it: test_hostile_depth_cpu.py checks the same on the oracle alone)
    assert np.isnan(pts[0]).any() and np.isinf(pts[0]).any() and np.isinf(pts[2]).any() and np.isinf(b).any()
    for f in (3, 4):  # the all-NaN frames: five times the camera centre
        assert np.array_equal(pts[f], np.repeat(poses[f][:3, 3:4], 5, axis=1))


def test_frustum_bounds_u16_contrast(gf):
    """The u16 kind beside it: an all-invalid frame (65535 everywhere, masked) has max depth 0.0 and the
    camera centre as its frustum -- what the all-NaN f64 frame gives -- and 65535 unmasked is 65.535 m."""
    Hh, W = H.SIZES["vec"]
    frames = np.zeros((3, Hh, W), np.uint16)
    frames[0] = 65535
    frames[1, 5, 7] = 1234
    frames[2, 9, 3] = 65535
    frames[2, 9, 4] = 65534
    poses = H.frustum_poses(3)
    for inval, want_md in ((True, [0.0, 1.234, 65.534]), (False, [65.535, 1.234, 65.535])):
        b, md, pts = gf.view_frustum_bounds(frames, H.K, poses, invalid_65535=inval, return_max_depth=True, return_points=True)
        assert np.array_equal(bits(md), bits(np.array(want_md)))
        want_pts = np.stack([O.view_frustum(m, Hh, W, H.K, p) for m, p in zip(want_md, poses)])
        assert np.array_equal(bits(pts), bits(want_pts))
        assert np.array_equal(bits(b), bits(O.frustum_bounds(want_md, Hh, W, H.K, poses)))
    nan = np.full((1, Hh, W), np.nan)
    _, md, pts = gf.view_frustum_bounds(nan, H.K, poses[:1], return_max_depth=True, return_points=True)
    _, md16, pts16 = gf.view_frustum_bounds(frames[:1], H.K, poses[:1], invalid_65535=True, return_max_depth=True, return_points=True)
    assert np.array_equal(bits(md), bits(md16)) and np.array_equal(bits(pts), bits(pts16))
