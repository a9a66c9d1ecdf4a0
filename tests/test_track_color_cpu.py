"""The photometric term's NumPy restatement (tests/icp_color_ref.py) checked on the
CPU: the colour row against a finite motion, the plane scene's coverage of every colour code, the
point of the feature -- a single plane, on which the geometric track is lost and the RGB-D track
converges -- and that the term does not hurt the well-constrained lounge.  The final errors measured
here are the bounds (at 2x) of these tests and of the device's (tests/test_track_color_gpu.py)."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_color_ref as C
import icp_ref as I
import raycast_ref as R
from test_track_cpu import C1, LOUNGE_MEASURED, LOUNGE_Z_FAR, lounge_case

# Final pose errors of the RGB-D restatement at the default weight (0.001 m per level), measured here
# (metres, degrees), per seeded start.  Plane: true pose the identity, starts 2 cm / 1 degree off
# (rng 5); converged in 5, 4 and 4 iterations, cond(A) 171 .. 184, 2803 .. 2967 colour inliers of
# 3319 .. 3497 candidates.  The geometric track from the same starts takes one step of 134 .. 1239 m
# (cond(A) 7e16 .. 9e16) and is lost at its second iteration.
PLANE_MEASURED = [(3.769e-4, 0.04628), (0.847e-4, 0.07204), (7.904e-4, 0.07380)]
# Lounge (test_track_cpu's case with frame 2's RGB decimated by 8): all three end max_iter, 1568 ..
# 1611 colour inliers of 3933 .. 4079 candidates, cond(A) 116 .. 118; the errors are 0.37 .. 0.95 of
# the geometric track's LOUNGE_MEASURED.  This case chose the default weight: at 0.002 the errors are
# 0.75 .. 1.49 of the geometric ones, at 0.003 up to 1.9, at 0.0005 0.63 .. 0.89; the plane behaves
# alike from 0.001 to 0.003.
LOUNGE_RGBD_MEASURED = [(5.053e-3, 0.1818), (2.731e-3, 0.0982), (1.403e-3, 0.0796)]


@pytest.fixture(scope="module")
def plane():
    return C.plane_state()


def test_colour_row_is_the_derivative_of_the_residual(plane):
    """With the model image held fixed and I_b taken as the bilinear function it is, the residual at
    E(delta) M is r - J delta up to second order.  The residual is I_f - I_b(pi(p')), p' = E p;
    inside one bilinear cell I_b(x, y) has the gradient (Gx', Gy') the lerp of the texels'
    *intensities* gives, while the row uses the lerp of the texels' *central differences*: a
    different, smoother estimate of the same derivative.  So the check is made where the two agree
    by construction: on a model image whose intensity is a linear ramp (both gradients exact and
    constant), which isolates the projection's derivative -- the part the row computes."""
    dm, nm, cm = C.plane_model(plane)
    Hm, Wm = dm.shape
    v, u = np.meshgrid(np.arange(Hm), np.arange(Wm), indexing="ij")
    ramp = (20 + 2 * u + v).astype(np.uint8)          # I = 20 + 2 u + v <= 20 + 164 + 60: no wrap
    ramp_map = np.stack([ramp, ramp, ramp], axis=-1)
    frame, rgb = C.plane_render()
    M = I.offset_2cm_1deg()
    lin = C.linearize_color(frame, rgb, I.FRAME_K, M, dm, ramp_map, I.MODEL_K, color_max_diff=1e9)
    assert lin["inliers"] > 2000
    p, g, r, J, If = (lin[k].astype(np.float64) for k in ("p", "g", "r", "J", "If"))
    fx, fy, cx, cy = I.MODEL_K[0, 0], I.MODEL_K[1, 1], I.MODEL_K[0, 2], I.MODEL_K[1, 2]
    # the texels' gradients are the ramp's: Gx = 2, Gy = 1
    assert np.allclose(g[:, 0] * p[:, 2], 2 * fx, rtol=1e-5) and np.allclose(g[:, 1] * p[:, 2], fy, rtol=1e-5)
    rng = np.random.default_rng(1)
    for scale in (1e-3, 1e-4):
        delta = rng.standard_normal(6)
        delta *= scale / np.linalg.norm(delta)
        E = I.se3(delta)
        p2 = p @ E[:3, :3].T + E[:3, 3]
        Ib2 = 20 + 2 * (fx * p2[:, 0] / p2[:, 2] + cx) + (fy * p2[:, 1] / p2[:, 2] + cy)
        r2 = If - Ib2
        lin_err = np.abs(r2 - (r - J @ delta)).max()
        first = np.abs(J @ delta).max()
        # What the first order leaves out, with I = 20 + 2 x + y, |dI/dp| <= 3 f / z and |d2I/dp2| <=
        # 3 * 2 f / z^2 (|p_x|, |p_y| < z here):
        #   E(delta) p = p + w x p + t + O(|w|^2 |p| / 2): 3 f / z * scale^2 |p| / 2;
        #   the projection's curvature over dp, |dp| <= scale (|p| + 1): 3 * 2 f / z^2 * dp^2 / 2.
        # And f32 rounding, independent of the scale: x and y take three operations each at magnitude
        # <= 83 (half an ulp 3.8e-6), times the gradient (2, 1): 3.6e-5; the bilinear I_b is three
        # lerps of three operations at magnitude <= 265 (half an ulp 1.5e-5): 1.4e-4; r one more:
        # 2e-4 levels in all; the row's own rounding is 1e-5 relative to the first-order term.
        pn, z = np.linalg.norm(p, axis=1).max(), p[:, 2].min()
        dp = scale * (pn + 1)
        bound = 3 * fx / z * scale ** 2 * pn / 2 + 3 * 2 * fx / z ** 2 * dp ** 2 / 2 + 2e-4 + 1e-5 * first
        print(f"delta {scale:g}: max |r' - (r - J delta)| {lin_err:.3e}, bound {bound:.3e}, first-order term {first:.3e}")
        assert lin_err <= bound
        assert first > 10 * bound  # a wrong row (a sign, a missing term) would show


def test_plane_scene_yields_every_colour_code(plane):
    """A condition on the inputs: on the linearise scene (plane frame with a hole, an occluder and a
    brightened rectangle; model map 83x61, M a 2 cm / 1 degree offset) every colour code 0 .. 5 occurs
    at least 20 times at stride 1 and at least once at stride 3, whose map is the stride-1 map masked."""
    dm, nm, cm = C.plane_model(plane)
    frame, rgb = C.plane_render(extras=True)
    M = I.offset_2cm_1deg()
    lin = C.linearize_color(frame, rgb, I.FRAME_K, M, dm, cm, I.MODEL_K)
    counts = np.bincount(lin["code"].ravel(), minlength=6)
    print("colour codes 0..5:", counts.tolist())
    assert len(counts) == 6 and counts.min() >= 20
    assert lin["inliers"] == counts[5] and lin["candidates"] == counts[2:].sum()
    assert (lin["resid"][lin["code"] != 5] == 0).all() and lin["resid"][lin["code"] == 5].any()
    assert (lin["code"][-1, :] != 0).any() and (lin["code"][:, -1] != 0).any()  # the last row and column take part
    as_m = C.linearize_color(frame.astype(np.float64) / 1000.0, rgb, I.FRAME_K, M, dm, cm, I.MODEL_K)
    assert np.array_equal(as_m["code"], lin["code"]) and np.array_equal(as_m["sums"], lin["sums"])
    third = C.linearize_color(frame, rgb, I.FRAME_K, M, dm, cm, I.MODEL_K, stride=3)
    c3 = np.bincount(third["code"].ravel(), minlength=6)
    print("stride 3:", c3.tolist())
    assert c3.min() >= 1
    keep = np.zeros_like(lin["code"], bool)
    keep[::3, ::3] = True
    assert np.array_equal(third["code"], np.where(keep, lin["code"], 0))
    # the geometric half sees the same scene: its codes all occur too
    geo = I.linearize(frame, I.FRAME_K, M, dm, nm, I.MODEL_K, np.eye(4))
    assert np.bincount(geo["code"].ravel(), minlength=7).min() >= 20


def test_photo_texels_and_intensity():
    rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], np.uint8)
    assert C.intensity(rgb).tolist() == [[255.0, 0.0, 76.0, 149.0, 28.0, (770 + 30000 + 870) >> 8]]
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    dm = np.ones((6, 7), np.float32)
    dm[2, 3] = 0.0
    T = C.photo_texels(col, dm)
    Im = C.intensity(col)
    valid = T[..., 3] > 0
    want = np.zeros((6, 7), bool)
    want[1:-1, 1:-1] = True
    want[2, 3] = want[1, 3] = want[3, 3] = want[2, 2] = want[2, 4] = False
    assert np.array_equal(valid, want) and (T[~valid] == 0).all()
    assert T[4, 2].tolist() == [Im[4, 2], (Im[4, 3] - Im[4, 1]) / 2, (Im[5, 2] - Im[3, 2]) / 2, 1.0]


def test_geometry_is_lost_on_the_plane_and_colour_converges(plane):
    """The point of the feature.  From each seeded start 2 cm / 1 degree off, the geometric
    restatement does not end within 10 mm of the truth (a condition on the starts: measured lost at
    iteration 2, decimetres away), and the RGB-D restatement ends converged or max_iter within twice
    PLANE_MEASURED."""
    frame, rgb = C.plane_render()
    starts = C.plane_starts()
    assert len(starts) == len(PLANE_MEASURED)
    for g, (mt, ma) in zip(starts, PLANE_MEASURED):
        st, sa = I.pose_error(g, C.TRUE_POSE)
        assert abs(st - 0.02) < 1e-9 and abs(sa - 1.0) < 1e-6
        dm, nm, cm = C.plane_model(plane, g, I.FRAME_K, I.FRAME_HW)
        geo = I.track(frame, I.FRAME_K, dm, nm, g)
        gt, ga = I.pose_error(geo["pose"], C.TRUE_POSE)
        print(f"plane, geometry only: {geo['status']} after {geo['iterations']}, {1e3 * gt:.1f} mm / {ga:.2f} deg, "
              f"cond(A) {geo['cond']:.1e}")
        assert gt > 0.010
        out = C.track(frame, rgb, I.FRAME_K, dm, nm, cm, g)
        et, ea = I.pose_error(out["pose"], C.TRUE_POSE)
        print(f"plane, RGB-D: {out['status']} after {out['iterations']}, {1e3 * et:.4f} mm / {ea:.5f} deg, cond(A) "
              f"{out['cond']:.0f}, colour inliers {out['color_inliers'][-1]} of {out['color_candidates'][-1]}")
        assert out["status"] in (I.CONVERGED, I.MAX_ITER)
        assert et <= 2 * mt and ea <= 2 * ma


def lounge_rgb():
    """Frame 2's RGB decimated by 8 (60,80,3), the image lounge_case's depth frame goes with."""
    _, _, rgb, _ = load_lounge(2)
    return np.ascontiguousarray(rgb[::8, ::8])


def test_rgbd_tracks_the_lounge():
    """test_track_cpu's lounge case with the colour term at the default weight: final errors within
    twice LOUNGE_RGBD_MEASURED, and each no more than 1.5x the geometric track's LOUNGE_MEASURED:
    the colour term must not hurt a well-constrained scene."""
    import oracle as O
    Kl = lounge_intrinsics()
    vol = O.OracleTSDFVolume(np.array(C1), 0.04)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, Kl, pose)
    state = (vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu)
    frame, K, true, starts = lounge_case()
    rgb = lounge_rgb()
    assert frame.shape == (60, 80) and rgb.shape == (60, 80, 3)
    for g, (mt, ma), (gt, ga) in zip(starts, LOUNGE_RGBD_MEASURED, LOUNGE_MEASURED):
        dm, nm, cm = R.raycast(*state, vol._vol_origin, 0.04, K, g, frame.shape, 0.0, LOUNGE_Z_FAR, 0.04)
        out = C.track(frame, rgb, K, dm, nm, cm, g)
        et, ea = I.pose_error(out["pose"], true)
        print(f"lounge RGB-D: {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after {out['iterations']}, inliers "
              f"{out['inliers'][-1]}, colour inliers {out['color_inliers'][-1]} of {out['color_candidates'][-1]}, "
              f"cond(A) {out['cond']:.0f}")
        assert out["status"] != I.LOST and out["inliers"][-1] >= 1000
        assert et <= 2 * mt and ea <= 2 * ma
        assert et <= 1.5 * gt and ea <= 1.5 * ga


def test_zero_weight_reproduces_the_geometric_track(plane):
    """color_weight = 0: A_g + 0 * A_c is A_g to the bit, so the trajectory is icp_ref.track's."""
    frame, rgb = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW), C.plane_render()[1]
    rng = np.random.default_rng(11)
    g = I.TRUE_POSE @ I.perturbation(rng, 0.04, 2.0)
    state = I.corner_state()
    dm, nm, cm = R.raycast(*state, I.ORIGIN, I.VS, I.FRAME_K, g, I.FRAME_HW, 0.0, I.Z_FAR, I.VS)
    a = I.track(frame, I.FRAME_K, dm, nm, g)
    b = C.track(frame, rgb, I.FRAME_K, dm, nm, cm, g, color_weight=0.0)
    assert a["iterations"] == b["iterations"] >= 3 and a["status"] == b["status"]
    assert np.array(a["trajectory"]).tobytes() == np.array(b["trajectory"]).tobytes()
    assert b["color_inliers"][0] > 100  # the colour sums were formed
