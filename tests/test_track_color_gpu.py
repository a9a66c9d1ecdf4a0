"""The device's RGB-D tracker (tsdf_icp_linearize_rgbd, tsdf_dense_track_rgbd / tsdf_hash_track_rgbd,
DESIGN.md §7f) against its NumPy restatement (tests/icp_color_ref.py on top of tests/icp_ref.py):
both code maps and both residual maps byte-identical, all 56 sums within what the order of addition
can change, the geometric half byte-identical to tsdf_icp_linearize, every pose update reproduced
step by step, and the final poses within the bounds tests/test_track_color_cpu.py measured -- on a
single plane, where the geometric track alone is lost.  Volumes <= 128^3, images <= 83 x 61 but
for one frame of 131 x 97."""
import ctypes

import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_color_ref as C
import icp_ref as I
from test_track_color_cpu import LOUNGE_RGBD_MEASURED, PLANE_MEASURED, lounge_rgb
from test_track_cpu import C1, LOUNGE_MEASURED, LOUNGE_Z_FAR, lounge_case

pytestmark = pytest.mark.gpu
# The combined systems here have cond(A) 1e2 .. 3e2 (asserted below 5e2 in follow) over ~6e3 exact
# terms, like the geometric systems of tests/test_track_gpu.py (2e2 .. 5e2, ~3e3 terms): the f64
# Cholesky solve's forward error is ~cond * 6 * 2^-53 * |xi| ~ 1e-13 * 1e-2, the sums differ from
# fsum by ~N * 2^-52 relative, i.e. ~1e-12 * cond on xi: ~1e-10.  The same 1e-9 holds.
STEP_TOL = 1e-9
MODELS = {"model": (I.MODEL_K, I.MODEL_HW), "frame": (I.FRAME_K, I.FRAME_HW)}


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
    assert hasattr(tracking, "icp_linearize_rgbd")
    return tracking


@pytest.fixture(scope="module")
def plane(gf):
    vol = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    assert tuple(vol._vol_dim) == I.SHAPE and np.array_equal(vol._vol_origin, I.ORIGIN)
    vol.set_state(*C.plane_state())
    return vol


@pytest.fixture(scope="module")
def corner(gf):
    vol = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    vol.set_state(*I.corner_state())
    return vol


@pytest.fixture(scope="module")
def plane_maps(plane):
    """The model maps of the linearise tests: the device raycasts of the plane volume from the
    identity, 83x61 through MODEL_K and 71x53 through FRAME_K."""
    out = {}
    for name, (K, hw) in MODELS.items():
        d, n, c = plane.raycast(K, np.eye(4), hw, z_far=I.Z_FAR)
        assert (d > 0).sum() > 2500 and (d == 0).sum() > 200 and c.dtype == np.uint8
        out[name] = (d, n, c)
    return out


@pytest.fixture(scope="module")
def lin_refs(plane_maps):
    """The restatement's two halves on the linearise scene, computed once: (model, stride) -> (geo, col)."""
    frame, rgb = C.plane_render(extras=True)
    M = I.offset_2cm_1deg()
    refs = {}
    for name, (K, _) in MODELS.items():
        d, n, c = plane_maps[name]
        for s in (1, 3):
            refs[name, s] = (I.linearize(frame, I.FRAME_K, M, d, n, K, np.eye(4), stride=s),
                             C.linearize_color(frame, rgb, I.FRAME_K, M, d, c, K, stride=s))
    return frame, rgb, refs


def dev_linearize(tr, frame, rgb, maps, name="model", stride=1, **kw):
    return tr.icp_linearize_rgbd(frame, rgb, I.FRAME_K, I.offset_2cm_1deg(), *maps, MODELS[name][0], np.eye(4),
                                 stride=stride, **kw)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["u16", "f64"])
@pytest.mark.parametrize("name", ["model", "frame"])
def test_linearize_rgbd_equals_the_restatement(tr, plane_maps, lin_refs, name, kind, stride):
    """Both code maps and both residual maps are byte-identical to the restatement, the four counts
    equal, each of the 56 sums within N 2^-52 sum|term| of its exact sum (N that half's inliers), and
    the geometric half is tsdf_icp_linearize's to the byte."""
    frame, rgb, refs = lin_refs
    geo, col = refs[name, stride]
    counts = np.bincount(col["code"].ravel(), minlength=6)
    assert len(counts) == 6 and counts.min() >= (20 if stride == 1 else 1), counts  # the reference shows every code
    f = frame if kind == "u16" else frame.astype(np.float64) / 1000.0
    got = dev_linearize(tr, f, rgb, plane_maps[name], name, stride)
    assert got["color_code"].tobytes() == col["code"].tobytes()
    assert got["color_residual"].tobytes() == col["resid"].tobytes()
    assert got["code"].tobytes() == geo["code"].tobytes()
    assert got["residual"].tobytes() == geo["resid"].tobytes()
    assert (got["inliers"], got["candidates"]) == (geo["inliers"], geo["candidates"])
    assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
    for half, ref, key in (("geometry", geo, "sums"), ("colour", col, "color_sums")):
        bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
        err = np.abs(got[key] - ref["sums"])
        print(f"{name} {kind} stride {stride} {half}: inliers {ref['inliers']}, max |sum - fsum| / bound "
              f"{np.max(err / bound):.3f}")
        assert (err <= bound).all()
    d, n, _ = plane_maps[name]
    old = tr.icp_linearize(f, I.FRAME_K, I.offset_2cm_1deg(), d, n, MODELS[name][0], np.eye(4), stride=stride)
    assert old["sums"].tobytes() == got["sums"].tobytes()
    assert old["code"].tobytes() == got["code"].tobytes() and old["residual"].tobytes() == got["residual"].tobytes()
    assert (old["inliers"], old["candidates"]) == (got["inliers"], got["candidates"])
    assert np.array_equal(got["color_A"], got["color_A"].T) and np.array_equal(got["color_b"], got["color_sums"][21:27])


def test_linearize_131x97_second_trip_of_the_finish(tr, plane_maps):
    """The other frames of the suite give at most 20 partial records, so the finish's lanes add one
    record each.  The plane's analytic frame through a 131x97 frame camera (FRAME_K scaled; the model
    maps are the 83x61 ones) gives 50: slices 0..17 add two records, slices 18..31 one.  Both entry
    points, u16, stride 1: codes and residuals byte-identical to the restatement, counts equal, sums
    within N 2^-52 sum|term|."""
    hw = (97, 131)
    K = I.FRAME_K.copy()
    K[0] *= hw[1] / I.FRAME_HW[1]
    K[1] *= hw[0] / I.FRAME_HW[0]
    frame, rgb = C.plane_render(K=K, hw=hw, extras=True)
    assert -(-frame.size // 256) == 50  # one partial record per workgroup of 256 pixels
    d, n, c = plane_maps["model"]
    M = I.offset_2cm_1deg()
    geo = I.linearize(frame, K, M, d, n, I.MODEL_K, np.eye(4))
    col = C.linearize_color(frame, rgb, K, M, d, c, I.MODEL_K)
    assert geo["inliers"] >= 20 and col["inliers"] >= 20  # (about 10^4 each: the bound below is not vacuous)
    old = tr.icp_linearize(frame, K, M, d, n, I.MODEL_K, np.eye(4))
    got = tr.icp_linearize_rgbd(frame, rgb, K, M, d, n, c, I.MODEL_K, np.eye(4))
    for res in (old, got):
        assert res["code"].tobytes() == geo["code"].tobytes()
        assert res["residual"].tobytes() == geo["resid"].tobytes()
        assert (res["inliers"], res["candidates"]) == (geo["inliers"], geo["candidates"])
    assert got["color_code"].tobytes() == col["code"].tobytes()
    assert got["color_residual"].tobytes() == col["resid"].tobytes()
    assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
    for name, sums, ref in (("icp_linearize", old["sums"], geo), ("rgbd geometry", got["sums"], geo),
                            ("rgbd colour", got["color_sums"], col)):
        bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
        err = np.abs(sums - ref["sums"])
        print(f"131x97 {name}: inliers {ref['inliers']}, max |sum - fsum| / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()
    assert old["sums"].tobytes() == got["sums"].tobytes()


def test_optional_maps_and_invalid_65535(tr, plane_maps, lin_refs):
    frame, rgb, refs = lin_refs
    full = dev_linearize(tr, frame, rgb, plane_maps["model"])
    bare = dev_linearize(tr, frame, rgb, plane_maps["model"], codes=False, residuals=False)
    assert all(bare[k] is None for k in ("code", "residual", "color_code", "color_residual"))
    assert bare["sums"].tobytes() == full["sums"].tobytes() and bare["color_sums"].tobytes() == full["color_sums"].tobytes()
    f2 = frame.copy()
    f2[20:30, 10:20] = 65535
    d, _, c = plane_maps["model"]
    ref = C.linearize_color(f2, rgb, I.FRAME_K, I.offset_2cm_1deg(), d, c, I.MODEL_K, invalid_65535=True)
    got = dev_linearize(tr, f2, rgb, plane_maps["model"], invalid_65535=True)
    assert got["color_code"].tobytes() == ref["code"].tobytes() and (got["color_code"][20:30, 10:20] == 0).all()


def track_kw(obj, frame, rgb, K, g, z_far, **kw):
    return obj.track(frame, K, g, z_far=z_far, return_info=True, color_im=rgb, **kw)


def follow(obj, tr, frame, rgb, K, g, z_far, info, device_counts=True, **color_kw):
    """The restatement chain, handle-agnostic: for each relative pose M_i the device produced, both
    halves of the restatement at M_i, combined and stepped, reproduce M_{i+1} within STEP_TOL, with
    the same counts, status and iteration count.  The model maps are the handle's own device raycast
    at g, the ones the track itself used."""
    d, n, c = obj.raycast(K, g, frame.shape, z_far=z_far)
    w = color_kw.get("color_weight", C.COLOR_DEFAULTS["color_weight"])
    cmax = color_kw.get("color_max_diff", C.COLOR_DEFAULTS["color_max_diff"])
    traj = info["trajectory"]
    assert len(traj) == info["iterations"] + 1 and np.array_equal(traj[0], np.eye(4))
    status = None
    for i in range(info["iterations"]):
        assert status is None
        lin = I.linearize(frame, K, traj[i], d, n, K, g)
        col = C.linearize_color(frame, rgb, K, traj[i], d, c, K, color_max_diff=cmax)
        if device_counts:
            got = tr.icp_linearize_rgbd(frame, rgb, K, traj[i], d, n, c, K, g, color_max_diff=cmax, codes=False, residuals=False)
            assert (got["inliers"], got["candidates"]) == (lin["inliers"], lin["candidates"])
            assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
        sums = C.combine(lin["sums"], col["sums"], w)
        cond = np.linalg.cond(I.system(sums)[0])
        assert cond < 5e2, cond  # what STEP_TOL was derived for
        M2, status, wn, tn = I.step(traj[i], sums, lin["inliers"])
        err = np.abs(M2 - traj[i + 1]).max()
        assert err <= STEP_TOL, (i, err)
    if status is None:
        status = I.MAX_ITER
        assert info["iterations"] == 10
    assert info["status"] == status
    assert info["inliers"] == lin["inliers"] and info["candidates"] == lin["candidates"]
    assert info["color_inliers"] == col["inliers"] and info["color_candidates"] == col["candidates"]
    assert abs(info["rms"] - np.sqrt(lin["sums"][27] / lin["inliers"])) <= 1e-12
    assert abs(info["color_rms"] - np.sqrt(col["sums"][27] / col["inliers"])) <= 1e-9
    assert abs(info["w_norm"] - wn) <= 1e-9 and abs(info["t_norm"] - tn) <= 1e-9


def test_plane_track_needs_the_colour_and_follows_the_restatement(plane, tr):
    """On the plane the geometric track does not come within 10 mm of the truth from any start; with
    color_im it follows the restatement step by step and ends within the CPU test's bounds."""
    frame, rgb = C.plane_render()
    for k, (g, (mt, ma)) in enumerate(zip(C.plane_starts(), PLANE_MEASURED)):
        geo_pose, geo = plane.track(frame, I.FRAME_K, g, z_far=I.Z_FAR, return_info=True)
        gt, _ = I.pose_error(geo_pose, C.TRUE_POSE)
        assert gt > 0.010 and "color_inliers" not in geo
        pose, info = track_kw(plane, frame, rgb, I.FRAME_K, g, I.Z_FAR)
        follow(plane, tr, frame, rgb, I.FRAME_K, g, I.Z_FAR, info, device_counts=k == 0)
        assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
        et, ea = I.pose_error(pose, C.TRUE_POSE)
        print(f"plane: geometry {geo['status']} at {1e3 * gt:.0f} mm; RGB-D {info['status']} after {info['iterations']}, "
              f"{1e3 * et:.4f} mm / {ea:.5f} deg, colour inliers {info['color_inliers']} of {info['color_candidates']}")
        assert info["status"] in ("converged", "max_iter")
        assert et <= 2 * mt and ea <= 2 * ma


def test_hash_track_on_an_integrated_plane(hf, tr):
    """The model fused by the ordinary integrate from four rendered RGB-D frames of the plane
    (142x106), tracked on the table: the chain holds against the table's own raycast, the colour
    term has its inliers and the track is not lost."""
    ht = hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 14)
    rng = np.random.default_rng(9)
    K2 = I.FRAME_K.copy()
    K2[:2] *= 2
    for i in range(4):
        P = np.eye(4) if i == 0 else I.perturbation(rng, 0.03, 2.0)
        mm, rgb = C.plane_render(P, K2, (106, 142))
        ht.integrate(rgb, mm.astype(np.float64) / 1000.0, K2, P)
    frame, rgb = C.plane_render()
    for k, g in enumerate(C.plane_starts()[:2]):
        pose, info = track_kw(ht, frame, rgb, I.FRAME_K, g, I.Z_FAR)  # (first: the frames are still pending)
        follow(ht, tr, frame, rgb, I.FRAME_K, g, I.Z_FAR, info, device_counts=k == 0)
        et, ea = I.pose_error(pose, C.TRUE_POSE)
        print(f"hash plane: {info['status']} after {info['iterations']}, {1e3 * et:.4f} mm / {ea:.5f} deg, colour inliers "
              f"{info['color_inliers']}")
        assert info["status"] != "lost" and info["color_inliers"] > 2000 and et < 0.010
    ht.close()


@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_lounge_rgbd_track(gf, hf, tr, kind):
    """The three lounge frames through integrate(), frame 2 (depth and RGB decimated by 8) tracked
    with the colour term: the chain holds on the handle's own maps, and the final errors are within
    the CPU test's bounds -- twice its measurements, and 1.5x the geometric track's."""
    obj = gf.TSDFVolume(np.array(C1), 0.04) if kind == "dense" else hf.HashTable(np.array(C1), 0.04, 1 << 16)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        obj.integrate(rgb, depth, lounge_intrinsics(), pose)
    frame, K, true, starts = lounge_case()
    rgb = lounge_rgb()
    for k, (g, (mt, ma), (gt, ga)) in enumerate(zip(starts, LOUNGE_RGBD_MEASURED, LOUNGE_MEASURED)):
        pose, info = track_kw(obj, frame, rgb, K, g, LOUNGE_Z_FAR)
        follow(obj, tr, frame, rgb, K, g, LOUNGE_Z_FAR, info, device_counts=k == 0)
        et, ea = I.pose_error(pose, true)
        print(f"lounge {kind}: {info['status']} after {info['iterations']}, inliers {info['inliers']}, colour inliers "
              f"{info['color_inliers']}, {1e3 * et:.3f} mm / {ea:.4f} deg")
        assert info["status"] != "lost" and info["inliers"] >= 1000
        assert et <= 2 * mt and ea <= 2 * ma
        assert et <= 1.5 * gt and ea <= 1.5 * ga
    obj.close()


def test_zero_weight_is_the_geometric_track_to_the_byte(corner, plane):
    """color_weight = 0: the colour sums are formed (the counts show it) and contribute exactly
    nothing -- on the corner, where the geometric track runs several iterations, and on the plane."""
    rgb = C.plane_render()[1]
    rng = np.random.default_rng(11)
    g = I.TRUE_POSE @ I.perturbation(rng, 0.04, 2.0)
    for vol, frame, start in ((corner, I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW), g),
                              (plane, C.plane_render()[0], C.plane_starts()[0])):
        p0, i0 = vol.track(frame, I.FRAME_K, start, z_far=I.Z_FAR, return_info=True)
        p1, i1 = track_kw(vol, frame, rgb, I.FRAME_K, start, I.Z_FAR, color_weight=0.0)
        assert p0.tobytes() == p1.tobytes() and i0["trajectory"].tobytes() == i1["trajectory"].tobytes()
        assert all(i0[k] == i1[k] for k in i0 if k != "trajectory")
        if vol is corner:  # (the plane's geometric track ends hundreds of metres away, where nothing projects)
            assert i1["iterations"] >= 3 and i1["color_candidates"] > 1000
    p3, i3 = track_kw(corner, I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW), rgb, I.FRAME_K, g, I.Z_FAR, color_weight=0.0,
                      stride=3)
    p2, i2 = corner.track(I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW), I.FRAME_K, g, z_far=I.Z_FAR, return_info=True, stride=3)
    assert p2.tobytes() == p3.tobytes() and i2["iterations"] >= 3


def test_two_calls_give_identical_bytes(plane, tr, plane_maps, lin_refs):
    frame, rgb, _ = lin_refs
    a, b = (dev_linearize(tr, frame, rgb, plane_maps["model"]) for _ in range(2))
    for k in ("sums", "color_sums", "residual", "color_residual", "code", "color_code"):
        assert a[k].tobytes() == b[k].tobytes()
    seen, srgb = C.plane_render()
    g = C.plane_starts()[0]
    (p1, i1), (p2, i2) = (track_kw(plane, seen, srgb, I.FRAME_K, g, I.Z_FAR) for _ in range(2))
    assert i1["iterations"] >= 3
    assert p1.tobytes() == p2.tobytes() and i1["trajectory"].tobytes() == i2["trajectory"].tobytes()
    s3, s3b = (track_kw(plane, seen, srgb, I.FRAME_K, g, I.Z_FAR, stride=3) for _ in range(2))
    assert s3[0].tobytes() == s3b[0].tobytes() and s3[1]["color_inliers"] < i1["color_inliers"] / 4


def test_device_tensors_equal_host_arrays(plane, tr, plane_maps, lin_refs):
    import torch
    frame, rgb, _ = lin_refs
    dev = torch.device("cuda", 0)
    host = dev_linearize(tr, frame, rgb, plane_maps["model"])
    maps = [torch.from_numpy(m).to(dev) for m in plane_maps["model"]]
    for f in (frame.view(np.int16), frame.astype(np.float64) / 1000.0):
        got = dev_linearize(tr, torch.from_numpy(f).to(dev), torch.from_numpy(rgb).to(dev), maps)
        assert got["sums"].tobytes() == host["sums"].tobytes() and got["color_sums"].tobytes() == host["color_sums"].tobytes()
        assert got["color_inliers"] == host["color_inliers"]
        assert np.array_equal(got["color_code"].cpu().numpy(), host["color_code"])
        assert got["color_residual"].cpu().numpy().tobytes() == host["color_residual"].tobytes()
        assert got["residual"].cpu().numpy().tobytes() == host["residual"].tobytes()
    seen, srgb = C.plane_render()
    g = C.plane_starts()[1]
    p_host, i_host = track_kw(plane, seen, srgb, I.FRAME_K, g, I.Z_FAR)
    p_dev, i_dev = track_kw(plane, torch.from_numpy(seen.view(np.int16)).to(dev), torch.from_numpy(srgb).to(dev), I.FRAME_K, g,
                            I.Z_FAR)
    assert p_host.tobytes() == p_dev.tobytes() and i_host["trajectory"].tobytes() == i_dev["trajectory"].tobytes()
    assert i_host["color_inliers"] == i_dev["color_inliers"]


def raw_track(vol, frame, rgb, g, *, fn="tsdf_dense_track_rgbd", cprm=None, H=None, W=None, color=True):
    from tsdf_amd import _ffi, tracking
    prm = tracking.icp_params()
    cprm = tracking.color_params() if cprm is None else cprm
    o, info, cinfo = np.full(16, np.nan), _ffi.TrackInfo(), _ffi.TrackColorInfo()
    H, W = frame.shape[0] if H is None else H, frame.shape[1] if W is None else W
    rc = getattr(_ffi.load(), fn)(vol._h, _ffi.ptr(frame), _ffi.DEPTH_U16_MM, _ffi.ptr(rgb) if color else None, H, W,
                                  _ffi.ptr(_ffi.f64(I.FRAME_K, 9)), _ffi.ptr(_ffi.f64(g, 16)), ctypes.byref(prm),
                                  ctypes.byref(cprm) if cprm is not False else None, 0.0, I.Z_FAR, I.VS, _ffi.ptr(o),
                                  ctypes.byref(info), ctypes.byref(cinfo), None, 0)
    return rc, o, _ffi.load().tsdf_last_error().decode()


def test_bad_arguments_are_refused_with_a_message(plane, hf, tr, plane_maps, lin_refs):
    """Every refusal is TSDF_E_ARG with a message and comes before any launch: out_pose is untouched."""
    from tsdf_amd import _ffi
    seen, srgb = C.plane_render()
    g = C.plane_starts()[0]
    rc, o, _ = raw_track(plane, seen, srgb, g)
    assert rc == 0 and np.isfinite(o).all()
    cases = [(dict(color=False), "color"), (dict(cprm=False), "color params"),
             (dict(cprm=tr.color_params(color_weight=-1e-3)), "color_weight"),
             (dict(cprm=tr.color_params(color_weight=float("nan"))), "color_weight"),
             (dict(cprm=tr.color_params(color_weight=float("inf"))), "color_weight"),
             (dict(cprm=tr.color_params(color_max_diff=0.0)), "color_max_diff"),
             (dict(cprm=tr.color_params(color_max_diff=-5.0)), "color_max_diff"),
             (dict(cprm=tr.color_params(color_max_diff=float("nan"))), "color_max_diff"),
             (dict(H=3, W=71), "4x4"), (dict(H=53, W=3), "4x4"), (dict(H=0, W=71), "image size")]
    for kw, word in cases:
        rc, o, msg = raw_track(plane, seen, srgb, g, **kw)
        assert rc == _ffi.E_ARG and word in msg and np.isnan(o).all(), (kw, msg)
    ht = hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12)
    rc, o, msg = raw_track(ht, seen, srgb, g, fn="tsdf_hash_track_rgbd", cprm=tr.color_params(color_weight=-1.0))
    assert rc == _ffi.E_ARG and "color_weight" in msg
    assert _ffi.load().tsdf_hash_track_rgbd(None, None, 0, None, 1, 1, None, None, None, None, 0.0, 1.0, 0.1, None, None, None,
                                            None, 0) == _ffi.E_ARG
    ht.close()

    def refused(fn, *a, **kw):
        with pytest.raises(_ffi.TSDFError) as e:
            fn(*a, **kw)
        assert e.value.code == _ffi.E_ARG and len(str(e.value)) > 12
        return str(e.value)

    # the existing refusals also apply
    assert "stride" in refused(track_kw, plane, seen, srgb, I.FRAME_K, g, I.Z_FAR, stride=0)
    assert "dist_max" in refused(track_kw, plane, seen, srgb, I.FRAME_K, g, I.Z_FAR, dist_max=0.0)
    assert "color_weight" in refused(track_kw, plane, seen, srgb, I.FRAME_K, g, I.Z_FAR, color_weight=-0.5)
    assert "color_max_diff" in refused(track_kw, plane, seen, srgb, I.FRAME_K, g, I.Z_FAR, color_max_diff=0)
    # the handle-less call
    frame, rgb, _ = lin_refs
    maps = plane_maps["model"]
    assert "color_weight" in refused(dev_linearize, tr, frame, rgb, maps, color_weight=-1.0)
    assert "color_max_diff" in refused(dev_linearize, tr, frame, rgb, maps, color_max_diff=-1.0)
    assert "stride" in refused(dev_linearize, tr, frame, rgb, maps, stride=0)
    assert "4x4" in refused(tr.icp_linearize_rgbd, frame, rgb, I.FRAME_K, np.eye(4), maps[0][:3], maps[1][:3], maps[2][:3],
                            I.MODEL_K, np.eye(4))
    assert "4x4" in refused(tr.icp_linearize_rgbd, frame, rgb, I.FRAME_K, np.eye(4), *(np.ascontiguousarray(m[:, :3]) for m in maps),
                            I.MODEL_K, np.eye(4))
    prm, cprm = tr.icp_params(), tr.color_params()
    K, E = _ffi.ptr(_ffi.f64(I.FRAME_K, 9)), _ffi.ptr(_ffi.f64(np.eye(4), 16))
    sums, counts = np.zeros(56), np.zeros(4, np.int64)
    lin = _ffi.load().tsdf_icp_linearize_rgbd
    args = lambda **o: [o.get(k, v) for k, v in dict(  # noqa: E731
        device=0, depth=_ffi.ptr(frame), dk=0, color=_ffi.ptr(rgb), Hf=53, Wf=71, Kf=K, M=E, md=_ffi.ptr(maps[0]),
        mn=_ffi.ptr(maps[1]), mc=_ffi.ptr(maps[2]), Hm=61, Wm=83, Km=K, P=E, prm=ctypes.byref(prm), cprm=ctypes.byref(cprm),
        sums=_ffi.ptr(sums), counts=_ffi.ptr(counts), code=None, res=None, ccode=None, cres=None, flags=0).items()]
    assert lin(*args()) == 0 and counts[2] > 1000
    for o, word in (({"color": None}, "color"), ({"mc": None}, "model"), ({"cprm": None}, "color params"),
                    ({"Hm": 3}, "4x4"), ({"Wm": 1 << 24}, "image size"), ({"depth": None}, "depth"),
                    ({"sums": None}, "sums"), ({"prm": None}, "params"), ({"dk": 7}, "depth_kind"), ({"device": 99}, "device")):
        assert lin(*args(**o)) == _ffi.E_ARG and word in _ffi.load().tsdf_last_error().decode(), o


def test_bad_colour_images_raise_value_error(plane, tr, plane_maps, lin_refs):
    import torch
    frame, rgb, _ = lin_refs
    dev = torch.device("cuda", 0)
    seen, srgb = C.plane_render()
    g = C.plane_starts()[0]
    d_t, c_t = torch.from_numpy(seen.view(np.int16)).to(dev), torch.from_numpy(srgb).to(dev)
    bad = [(seen, srgb.astype(np.float32)),            # wrong dtype
           (seen, srgb[:, :, :2]),                     # wrong shape
           (seen, srgb[:-1]),                          # not the depth frame's size
           (seen, c_t),                                # a tensor alongside an array
           (d_t, srgb),                                # an array alongside a tensor
           (d_t, c_t.cpu()),                           # host tensor
           (d_t, c_t.to(torch.float32)),               # wrong tensor dtype
           (d_t, torch.zeros((53, 71, 6), dtype=torch.uint8, device=dev)[:, :, ::2])]  # strided view
    for d, c in bad:
        with pytest.raises(ValueError):
            track_kw(plane, d, c, I.FRAME_K, g, I.Z_FAR)
    maps = plane_maps["model"]
    t_maps = [torch.from_numpy(m).to(dev) for m in maps]
    f_t, r_t = torch.from_numpy(frame.view(np.int16)).to(dev), torch.from_numpy(rgb).to(dev)
    dev_linearize(tr, f_t, r_t, t_maps)
    for f, c, m in ((f_t, rgb, t_maps), (f_t, r_t, [t_maps[0], t_maps[1], maps[2]]), (frame, rgb[:, :, :1], maps),
                    (f_t, r_t, [t_maps[0], t_maps[1], t_maps[2].to(torch.float32)]),
                    (frame, rgb, [maps[0], maps[1], maps[2][:-1]])):
        with pytest.raises(ValueError):
            dev_linearize(tr, f, c, m)
