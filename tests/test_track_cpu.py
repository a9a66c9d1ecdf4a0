"""The tracking contract's NumPy restatement (tests/icp_ref.py) checked on the CPU:
the linearisation against a finite motion, the corner scene's coverage of every pixel code, and
what the method itself reaches -- on the analytic corner and on the lounge fixture fused by the
oracle.  The final errors measured here are the bounds (at 2x) of these tests and of the device's
tests (tests/test_track_gpu.py imports them)."""
import math

import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_ref as I
import raycast_ref as R

# Final pose errors of the reference, measured here (metres, degrees), per seeded start.
# Corner: true pose translation (0.01, -0.02, 0.03), starts 4 cm / 2 degrees off (rng 11); the first
# start ends as max_iter (the inlier set flips between 2707 and 2708 pixels), the second converges
# in 5 iterations; cond(A) 199 and 284.
CORNER_SEED = 11
CORNER_MEASURED = [(1.853e-3, 0.0676), (1.014e-3, 0.0255)]
# Lounge: 3 frames fused at 4 cm, frame 2 decimated by 8, starts 3 cm / 1.5 degrees off (rng 23):
# 2238 .. 2277 inliers, cond(A) 125 .. 135.
LOUNGE_SEED = 23
LOUNGE_MEASURED = [(5.656e-3, 0.1923), (3.762e-3, 0.1127), (3.836e-3, 0.1289)]
C1 = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]
LOUNGE_Z_FAR = 6.0


def corner_starts():
    rng = np.random.default_rng(CORNER_SEED)
    return [I.TRUE_POSE @ I.perturbation(rng, 0.04, 2.0) for _ in CORNER_MEASURED]


def lounge_case():
    """(depth frame (60,80) f64 metres, K / 8, true pose, the seeded starts)."""
    K = lounge_intrinsics().copy()
    K[:2] /= 8.0
    _, depth, _, pose = load_lounge(2, color=False)
    rng = np.random.default_rng(LOUNGE_SEED)
    return np.ascontiguousarray(depth[::8, ::8]), K, pose, [pose @ I.perturbation(rng, 0.03, 1.5) for _ in LOUNGE_MEASURED]


@pytest.fixture(scope="module")
def corner():
    return I.corner_state()


def test_row_is_the_derivative_of_the_residual(corner):
    """With the pairs held fixed, the residuals at E(delta) M are r - J delta up to second order:
    E(delta) p = p + w x p + t + O(|w|^2 |p| / 2), and n (w x p) = (p x n) w."""
    dm, nm = I.corner_model(corner)
    frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    lin = I.linearize(frame, I.FRAME_K, I.offset_2cm_1deg(), dm, nm, I.MODEL_K, np.eye(4))
    assert lin["inliers"] > 2000
    p, n, r, J = (lin[k].astype(np.float64) for k in ("p", "n", "r", "J"))
    rng = np.random.default_rng(1)
    for scale in (1e-3, 1e-4):
        delta = rng.standard_normal(6)
        delta *= scale / np.linalg.norm(delta)
        E = I.se3(delta)
        p2 = p @ E[:3, :3].T + E[:3, 3]
        r2 = r - np.einsum("ij,ij->i", n, p2 - p)  # n (q - p2), q fixed: r = n (q - p)
        lin_err = np.abs(r2 - (r - J @ delta)).max()
        first = np.abs(J @ delta).max()
        w2 = float(delta[:3] @ delta[:3])
        bound = 0.5 * w2 * np.linalg.norm(p, axis=1).max() * 1.01 + 1e-6 * scale  # (+ the f32 rounding of J, n)
        print(f"delta {scale:g}: max |r' - (r - J delta)| {lin_err:.3e}, bound {bound:.3e}, first-order term {first:.3e}")
        assert lin_err <= bound
        assert first > 50 * bound


def test_corner_scene_yields_every_code(corner):
    """A condition on the inputs: the restatement on the corner scene (model map 83x61, frame 71x53,
    M a 2 cm / 1 degree offset) gives every code 0 .. 6 at least 20 times; so do the u16 frame's
    values as f64 metres; every third pixel still shows every code."""
    dm, nm = I.corner_model(corner)
    frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    M = I.offset_2cm_1deg()
    t, a = I.pose_error(np.eye(4), M)
    assert abs(t - 0.02) < 1e-9 and abs(a - 1.0) < 1e-6
    lin = I.linearize(frame, I.FRAME_K, M, dm, nm, I.MODEL_K, np.eye(4), **I.CORNER_GATES)
    counts = np.bincount(lin["code"].ravel(), minlength=7)
    print("codes 0..6:", counts.tolist())
    assert len(counts) == 7 and counts.min() >= 20
    assert lin["inliers"] == counts[6] and lin["candidates"] == counts[2:].sum()
    assert (lin["resid"][lin["code"] != 6] == 0).all() and lin["resid"][lin["code"] == 6].any()
    as_m = I.linearize(frame.astype(np.float64) / 1000.0, I.FRAME_K, M, dm, nm, I.MODEL_K, np.eye(4), **I.CORNER_GATES)
    assert np.array_equal(as_m["code"], lin["code"]) and np.array_equal(as_m["sums"], lin["sums"])
    third = I.linearize(frame, I.FRAME_K, M, dm, nm, I.MODEL_K, np.eye(4), stride=3, **I.CORNER_GATES)
    c3 = np.bincount(third["code"].ravel(), minlength=7)
    print("stride 3:", c3.tolist())
    assert c3.min() >= 1
    keep = np.zeros_like(lin["code"], bool)
    keep[::3, ::3] = True
    assert np.array_equal(third["code"], np.where(keep, lin["code"], 0))


def test_reference_converges_on_the_corner(corner):
    """From two seeded starts 4 cm / 2 degrees off, one track each against the reference raycast at
    the start: the final error is asserted at twice the value measured here (CORNER_MEASURED)."""
    frame = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    for g, (mt, ma) in zip(corner_starts(), CORNER_MEASURED):
        dm, nm = I.corner_model(corner, g, I.FRAME_K, I.FRAME_HW)
        out = I.track(frame, I.FRAME_K, dm, nm, g)
        et, ea = I.pose_error(out["pose"], I.TRUE_POSE)
        st, sa = I.pose_error(g, I.TRUE_POSE)
        print(f"corner: start {1e3 * st:.1f} mm / {sa:.2f} deg -> {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after "
              f"{out['iterations']} iterations, inliers {out['inliers'][-1]}, cond(A) {out['cond']:.0f}")
        assert out["status"] != I.LOST
        assert out["cond"] < 1e3  # a well-conditioned start
        assert et <= 2 * mt and ea <= 2 * ma


def test_reference_tracks_the_lounge():
    """Lounge C1 at 4 cm, 3 frames fused by the oracle; frame 2's depth decimated by 8 (80x60, K / 8)
    tracked from three seeded starts 3 cm / 1.5 degrees off its pose (the fixture poses differ frame
    to frame by 1 - 2 mm, less than 4 cm voxels resolve: a perturbed start is the test).  Final error
    against the fixture pose asserted at twice the value measured here (LOUNGE_MEASURED)."""
    import oracle as O
    Kl = lounge_intrinsics()
    vol = O.OracleTSDFVolume(np.array(C1), 0.04)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, Kl, pose)
    state = (vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu)
    frame, K, true, starts = lounge_case()
    assert frame.shape == (60, 80)
    for g, (mt, ma) in zip(starts, LOUNGE_MEASURED):
        dm, nm, _ = R.raycast(*state, vol._vol_origin, 0.04, K, g, frame.shape, 0.0, LOUNGE_Z_FAR, 0.04)
        out = I.track(frame, K, dm, nm, g)
        et, ea = I.pose_error(out["pose"], true)
        st, sa = I.pose_error(g, true)
        print(f"lounge: start {1e3 * st:.1f} mm / {sa:.2f} deg -> {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after "
              f"{out['iterations']} iterations, inliers {out['inliers'][-1]}, cond(A) {out['cond']:.0f}")
        assert out["status"] != I.LOST and out["inliers"][-1] >= 1000
        assert et <= 2 * mt and ea <= 2 * ma


def test_step_declares_lost_without_moving():
    M = I.offset_2cm_1deg()
    sums = np.zeros(28)
    M2, status, _, _ = I.step(M, sums, 500)          # A = 0: no positive pivot
    assert status == I.LOST and np.array_equal(M2, M)
    sums[[0, 6, 11, 15, 18, 20]] = 1.0               # A = I, b = 0
    M3, status, wn, tn = I.step(M, sums, 99)         # too few inliers
    assert status == I.LOST and np.array_equal(M3, M)
    M4, status, wn, tn = I.step(M, sums, 100)
    assert status == I.CONVERGED and wn == 0 and tn == 0 and np.array_equal(M4, M)
    assert math.isclose(I.COS30, math.sqrt(3) / 2)
