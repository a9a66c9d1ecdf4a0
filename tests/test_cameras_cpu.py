"""Conditions on the inputs of tests/test_cameras_gpu.py, checked with the restatements alone: the
cameras of tests/camera_cases.py (fx != fy; the principal point outside the image) keep the scenes in
view, reach every code, let the reference trackers converge -- and tell fx from fy: the same
restatement with the two exchanged gives results the device tests' assertions would reject, so a
kernel that exchanged them could not pass.  Every test prints the counts and errors that
camera_cases.py records."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import camera_cases as X
import icp_color_ref as C
import icp_ref as I
import raycast_ref as R
import sdf_ref as S
import test_raycast_cpu as RC
from test_track_cpu import C1, LOUNGE_SEED, LOUNGE_Z_FAR
from track_edge_cases import MIN_COUNT

SWAP_FLOOR = 500  # codes a swap of fx and fy must change: a floor under the measured 970 .. 2745, not a measurement


@pytest.fixture(scope="module")
def corner():
    return I.corner_state()


@pytest.fixture(scope="module")
def plane():
    return C.plane_state()


@pytest.mark.parametrize("name", ["aniso", "off"])
def test_plane_raycast_equals_the_analytic_depth(name):
    """test_raycast_cpu's oblique plane through A_MODEL from the origin and through OFF_MODEL from its
    pose: every ray whose analytic hit lies two voxels inside the volume (so that the samples before
    and after it have their cells) is a hit, within 4 x PLANE_ERR_F32 of the analytic depth."""
    K, pose = (X.A_MODEL, np.eye(4)) if name == "aniso" else (X.OFF_MODEL, X.OFF_MODEL_POSE)
    state = RC.plane_state()
    v, u = np.meshgrid(np.arange(RC.HW[0], dtype=np.float64), np.arange(RC.HW[1], dtype=np.float64), indexing="ij")
    dirs = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ pose[:3, :3].T
    za = ((RC.P0 - pose[:3, 3]) @ RC.N) / (dirs @ RC.N)
    q = (pose[:3, 3] + dirs * za[..., None] - RC.ORIGIN.astype(np.float64)) / RC.VS
    inside = (za > 0) & np.all((q >= 2) & (q <= np.array(RC.SHAPE) - 3), axis=-1)
    d, n, _ = R.raycast(*state, RC.ORIGIN, RC.VS, K, pose, RC.HW, 0.0, 2.0, RC.VS)
    err = np.abs(d.astype(np.float64) - za)[inside].max()
    other = R.raycast(*state, RC.ORIGIN, RC.VS, X.swapped(K), pose, RC.HW, 0.0, 2.0, RC.VS)[0]
    differ = int((other.view(np.uint32) != d.view(np.uint32)).sum())
    print(f"plane {name}: {int(inside.sum())} of {inside.size} rays meet the plane inside, hits {int((d > 0).sum())}, max |depth - "
          f"analytic| {err:.3e} m, depth {za[inside].min():.3f} .. {za[inside].max():.3f}; fx <-> fy changes {differ} depths")
    assert inside.sum() >= 0.9 * inside.size
    assert (d[inside] > 0).all()
    assert err <= 4 * RC.PLANE_ERR_F32
    assert np.abs(n[inside] - RC.N).max() <= 1e-4
    assert differ >= 0.9 * inside.size


def corner_inputs(corner, pair, pitched):
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    return I.render(Pf, Kf, I.FRAME_HW), I.corner_model(corner, Pm, Km, I.MODEL_HW)


@pytest.mark.parametrize("pair,pitched", X.lin_cases())
def test_corner_linearisation_reaches_every_code_and_tells_fx_from_fy(corner, pair, pitched):
    """Every code 0 .. 6 at least 20 times (stride 3: the stride-1 map masked); exchanging fx and fy of
    the model camera, or of the frame camera, changes at least 500 codes."""
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    frame, (dm, nm) = corner_inputs(corner, pair, pitched)
    lin = I.linearize(frame, Kf, M, dm, nm, Km, Pm, **I.CORNER_GATES)
    counts = np.bincount(lin["code"].ravel(), minlength=7)
    by_m = I.linearize(frame, Kf, M, dm, nm, X.swapped(Km), Pm, **I.CORNER_GATES)
    by_f = I.linearize(frame, X.swapped(Kf), M, dm, nm, Km, Pm, **I.CORNER_GATES)
    dm_, df_ = int((by_m["code"] != lin["code"]).sum()), int((by_f["code"] != lin["code"]).sum())
    third = I.linearize(frame, Kf, M, dm, nm, Km, Pm, stride=3, **I.CORNER_GATES)
    print(f"corner {pair} pitched {pitched}: codes 0..6 {counts.tolist()}, fx <-> fy of Km changes {dm_}, of Kf {df_}; stride 3 "
          f"{np.bincount(third['code'].ravel(), minlength=7).tolist()}")
    assert len(counts) == 7 and counts.min() >= 20
    assert dm_ >= SWAP_FLOOR and df_ >= SWAP_FLOOR
    keep = np.zeros_like(lin["code"], bool)
    keep[::3, ::3] = True
    assert np.array_equal(third["code"], np.where(keep, lin["code"], 0)) and third["inliers"] >= 100


def plane_inputs(plane, pair, pitched):
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    return C.plane_render(Pf, Kf, I.FRAME_HW, extras=True), C.plane_model(plane, Pm, Km, I.MODEL_HW)


@pytest.mark.parametrize("pair,pitched", X.lin_cases())
def test_colour_linearisation_reaches_every_code_and_tells_fx_from_fy(plane, pair, pitched):
    """Every colour code the isotropic plane case (test_track_color_cpu) yields at least 20 times is
    yielded at least 20 times with the model camera level, and at least 10 times with it pitched (one
    code falls to 17 there); exchanging fx and fy of the model camera changes at least 500 codes."""
    iso_frame, iso_rgb = C.plane_render(extras=True)
    idm, _, icm = C.plane_model(plane)
    iso = np.bincount(C.linearize_color(iso_frame, iso_rgb, I.FRAME_K, I.offset_2cm_1deg(), idm, icm, I.MODEL_K)["code"].ravel(),
                      minlength=6)
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    (frame, rgb), (dm, nm, cm) = plane_inputs(plane, pair, pitched)
    col = C.linearize_color(frame, rgb, Kf, M, dm, cm, Km)
    counts = np.bincount(col["code"].ravel(), minlength=6)
    changed = int((C.linearize_color(frame, rgb, Kf, M, dm, cm, X.swapped(Km))["code"] != col["code"]).sum())
    print(f"plane {pair} pitched {pitched}: colour codes 0..5 {counts.tolist()} (isotropic {iso.tolist()}), fx <-> fy of Km "
          f"changes {changed}")
    assert (iso >= 20).all()
    assert (counts[iso >= 20] >= (10 if pitched else 20)).all()
    assert changed >= SWAP_FLOOR


@pytest.mark.parametrize("pair,pitched", X.lin_cases())
def test_gradient_scaling_alone_moves_the_colour_sums_past_the_bound(plane, pair, pitched):
    """The Jacobian line scales the image gradient by (fxm, fym).  With that line alone exchanged --
    codes and residuals identical -- the colour sums differ from the restatement's by more than 100
    times the bound the device test allows (inliers 2^-52 sum|term|)."""
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    (frame, rgb), (dm, nm, cm) = plane_inputs(plane, pair, pitched)
    col = C.linearize_color(frame, rgb, Kf, M, dm, cm, Km)
    bad = C.linearize_color(frame, rgb, Kf, M, dm, cm, Km, swap_gradient_focals=True)
    assert np.array_equal(bad["code"], col["code"]) and bad["resid"].tobytes() == col["resid"].tobytes()
    bound = col["inliers"] * 2.0 ** -52 * col["abs_sums"]
    ratio = np.abs(bad["sums"] - col["sums"])[:27] / bound[:27]  # (sum r r has no Jacobian in it)
    print(f"plane {pair} pitched {pitched}: |sums with Gx fym, Gy fxm - sums| / bound: least {ratio.min():.3e} over the 27 sums "
          f"with a row in them")
    assert bad["sums"][27] == col["sums"][27]
    assert (ratio > 100).all()


@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_sdf_linearisation_reaches_every_code(corner, pair):
    """Every code sdf_ref.every_code_case() yields at least MIN_COUNT times is yielded at least
    MIN_COUNT times through A_FRAME and OFF_FRAME; exchanging fx and fy changes at least 500 codes."""
    t, w, _ = corner
    f0, K0, M0, G0 = S.every_code_case()
    iso = np.bincount(S.linearize(f0, K0, M0, G0, t, w, **S.CORNER_VOL, **S.EVERY_CODE)["code"].ravel(), minlength=7)
    frame, K, M, G = X.sdf_code_case(pair)
    lin = S.linearize(frame, K, M, G, t, w, **S.CORNER_VOL, **S.EVERY_CODE)
    counts = np.bincount(lin["code"].ravel(), minlength=7)
    changed = int((S.linearize(frame, X.swapped(K), M, G, t, w, **S.CORNER_VOL, **S.EVERY_CODE)["code"] != lin["code"]).sum())
    third = S.linearize(frame, K, M, G, t, w, stride=3, **S.CORNER_VOL, **S.EVERY_CODE)
    print(f"sdf {pair}: codes 0..6 {counts.tolist()} (isotropic {iso.tolist()}), fx <-> fy changes {changed}; stride 3 "
          f"{np.bincount(third['code'].ravel(), minlength=7).tolist()}")
    assert (iso[[0, 2, 3, 4, 5, 6]] >= MIN_COUNT).all() and iso[1] == 0
    assert (counts[iso >= MIN_COUNT] >= MIN_COUNT).all()
    assert changed >= SWAP_FLOOR and third["inliers"] >= MIN_COUNT


def report(label, out, true, g):
    et, ea = I.pose_error(out["pose"], true)
    st, sa = I.pose_error(g, true)
    print(f"{label}: start {1e3 * st:.1f} mm / {sa:.2f} deg -> {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after "
          f"{out['iterations']} iterations, inliers {out['inliers'][-1]}, cond(A) {out['cond']:.0f}")
    return et, ea


@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_reference_trackers_converge(corner, plane, pair):
    """icp_ref.track and sdf_ref.track on the corner, icp_color_ref.track on the plane, each from its
    two seeded starts: converged, cond(A) below 5e2 (what the device tests' step tolerance was derived
    for), and the final error within twice the value measured here (camera_cases.MEASURED)."""
    K, true, starts = X.track_case(pair)
    assert I.pose_error(*starts)[0] > 0.01  # two starts, not one twice
    frame = I.render(true, K, I.FRAME_HW)
    for k, g in enumerate(starts):
        dm, nm = I.corner_model(corner, g, K, I.FRAME_HW)
        for kind, out in (("icp", I.track(frame, K, dm, nm, g)), ("sdf", S.track(frame, K, g, corner[0], corner[1], **S.CORNER_VOL))):
            et, ea = report(f"{pair} {kind} start {k}", out, true, g)
            mt, ma = X.MEASURED[pair][kind][k]
            assert out["status"] == I.CONVERGED and out["cond"] < 5e2
            assert et <= 2 * mt and ea <= 2 * ma
    K, true, starts = X.plane_track_case(pair)
    frame, rgb = C.plane_render(true, K, I.FRAME_HW)
    for k, g in enumerate(starts):
        dm, nm, cm = C.plane_model(plane, g, K, I.FRAME_HW)
        out = C.track(frame, rgb, K, dm, nm, cm, g)
        et, ea = report(f"{pair} rgbd start {k}", out, true, g)
        mt, ma = X.MEASURED[pair]["rgbd"][k]
        assert out["status"] == I.CONVERGED and out["cond"] < 5e2
        assert et <= 2 * mt and ea <= 2 * ma


def lounge_aniso_case():
    """test_track_cpu.lounge_case() with unequal factors: columns decimated by 8, rows by 7.5 -- row v
    of the 64 x 80 frame is the source row nearest 7.5 v (half-way rows take the next one), so odd rows
    sit half a source pixel, 0.07 of theirs, below where K puts them -- and K's rows divided by 8 and
    7.5: fx 65.6, fy 70.0."""
    K = lounge_intrinsics().copy()
    K[0] /= 8.0
    K[1] /= 7.5
    _, depth, _, pose = load_lounge(2, color=False)
    rows = np.floor(7.5 * np.arange(64) + 0.5).astype(int)
    rng = np.random.default_rng(LOUNGE_SEED)
    return (np.ascontiguousarray(depth[rows][:, ::8]), K, pose,
            [pose @ I.perturbation(rng, 0.03, 1.5) for _ in X.LOUNGE_MEASURED])


def test_reference_tracks_the_lounge_through_unequal_factors():
    """test_track_cpu's lounge case (C1 at 4 cm, 3 frames fused by the oracle) with frame 2 decimated
    by 8 and 7.5: not lost, at least 1000 inliers, within twice camera_cases.LOUNGE_MEASURED."""
    import oracle as O
    vol = O.OracleTSDFVolume(np.array(C1), 0.04)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, lounge_intrinsics(), pose)
    state = (vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu)
    frame, K, true, starts = lounge_aniso_case()
    assert frame.shape == (64, 80) and K[0, 0] != K[1, 1]
    for k, (g, (mt, ma)) in enumerate(zip(starts, X.LOUNGE_MEASURED)):
        dm, nm, _ = R.raycast(*state, vol._vol_origin, 0.04, K, g, frame.shape, 0.0, LOUNGE_Z_FAR, 0.04)
        out = I.track(frame, K, dm, nm, g)
        et, ea = report(f"lounge 8 x 7.5 start {k}", out, true, g)
        assert out["status"] != I.LOST and out["inliers"][-1] >= 1000
        assert et <= 2 * mt and ea <= 2 * ma


@pytest.mark.parametrize("name", ["aniso", "off"])
def test_tiny_raycasts_of_the_corner_hit(corner, name):
    """The corner state cast at the TINY sizes (an image smaller than a wave's 8 x 8 tile, exactly one
    tile, strips 3 wide and 3 high), the camera scaled per axis to each size: at least one hit each,
    and at least half the rays for the four larger sizes."""
    K, pose = (X.A_MODEL, np.eye(4)) if name == "aniso" else (X.OFF_MODEL, X.OFF_MODEL_POSE)
    hits = []
    for hw in X.TINY:
        d, _, _ = R.raycast(*corner, I.ORIGIN, I.VS, X.scaled(K, I.MODEL_HW, hw), pose, hw, 0.0, I.Z_FAR, I.VS)
        hits.append(int((d > 0).sum()))
        assert hits[-1] >= 1 and (hw == (1, 1) or 2 * hits[-1] >= d.size)
    print(f"tiny {name}: hits {hits} of {[h * w for h, w in X.TINY]}")
    assert hits == X.TINY_HITS[name]


def test_frustum_points_tell_fx_from_fy():
    """oracle.view_frustum with the two frustum cameras of the device test: exchanging fx and fy moves
    the far corners by more than a centimetre (the device test compares bits)."""
    import oracle as O
    pose = load_lounge(0, color=False)[3]
    for K in X.frustum_cameras(lounge_intrinsics()):
        assert K[0, 0] != K[1, 1]
        a, b = O.view_frustum(3.0, 480, 640, K, pose), O.view_frustum(3.0, 480, 640, X.swapped(K), pose)
        print(f"frustum fx {K[0, 0]:.1f} fy {K[1, 1]:.1f} c ({K[0, 2]:.1f}, {K[1, 2]:.1f}): fx <-> fy moves a corner by "
              f"{np.abs(a - b).max():.3f} m")
        assert np.abs(a - b).max() > 0.01
