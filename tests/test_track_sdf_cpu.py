"""The point-to-SDF contract's NumPy restatement (tests/sdf_ref.py) checked on the CPU:
the row against a finite motion, the every-code inputs, the cell against raycast_ref's, and what the
method itself reaches on the analytic corner and on the lounge fixture fused by the oracle.  The
final errors measured here are the bounds (at 2x) of these tests and of the device's tests
(tests/test_track_sdf_gpu.py imports them)."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_ref as I
import raycast_ref as R
import sdf_ref as S
from test_track_cpu import C1, LOUNGE_Z_FAR, corner_starts, lounge_case

# What the restatement reaches, measured here, per seeded start of test_track_cpu.py: (final
# translation error in metres, rotation error in degrees, iterations, inliers of the last
# linearisation, cond(A)).  Corner: both 4 cm / 2 degree starts converge to the same minimum.
CORNER_SDF_MEASURED = [(1.057e-3, 0.02472, 4, 2975, 151), (1.057e-3, 0.02472, 4, 2975, 150)]
# Lounge: 3 frames fused at 4 cm by the oracle, frame 2 decimated by 8 (80 x 60), starts 3 cm / 1.5
# degrees off; all three converge.  The ICP restatement on the same starts (test_track_cpu.py): 5.656 /
# 3.762 / 3.836 mm, 0.192 / 0.113 / 0.129 degrees with 2238 .. 2277 inliers.
LOUNGE_SDF_MEASURED = [(2.254e-3, 0.04505, 7, 2893, 131), (1.529e-3, 0.04218, 6, 2894, 128),
                       (1.529e-3, 0.04218, 5, 2894, 127)]


@pytest.fixture(scope="module")
def corner():
    return I.corner_state()


def test_row_is_the_derivative_of_the_residual(corner):
    """With each point's cell held fixed, F(p) = -trunc tri(c, Qr p + Qo - i0) is a cubic polynomial
    of p, and r - J delta is F(E(delta) p) to first order.  What remains is bounded per point by the
    rotation's second order, |w|^2 |p| |n| / 2, and the interpolant's: with dq the motion in voxels
    and h the largest mixed second differences of the corner values, trunc (sum h) |dq|^2 +
    trunc |h_xyz| |dq|^3 (a trilinear function has no pure second derivatives).  And it is second
    order: a tenth of the motion leaves less than a fiftieth of the remainder."""
    t, w, _ = corner
    frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    G = np.eye(4)
    lin = S.linearize(frame, I.FRAME_K, I.offset_2cm_1deg(), G, t, w, **S.CORNER_VOL)
    assert lin["inliers"] > 2000
    p, n, J = (lin[k].astype(np.float64) for k in ("p", "n", "J"))
    Qr, Qo, _, sc, tr = (np.float64(x) for x in S.geometry(S.CORNER_VOL["origin"], I.VS, 5 * I.VS, G))
    i0 = lin["cell"][lin["code"] == 6]
    c = [t[i0[:, 0] + (s >> 2), i0[:, 1] + ((s >> 1) & 1), i0[:, 2] + (s & 1)].astype(np.float64) for s in range(8)]

    def F(pts):
        return -tr * R._trilinear(c, pts @ Qr.T + Qo - i0)

    r0 = F(p)
    assert np.abs(r0 - lin["r"]).max() <= 2e-6  # (the f32 rounding of q, f and r)
    hxy = np.maximum(abs(c[6] - c[4] - c[2] + c[0]), abs(c[7] - c[5] - c[3] + c[1]))
    hxz = np.maximum(abs(c[5] - c[4] - c[1] + c[0]), abs(c[7] - c[6] - c[3] + c[2]))
    hyz = np.maximum(abs(c[3] - c[2] - c[1] + c[0]), abs(c[7] - c[6] - c[5] + c[4]))
    hxyz = abs(c[7] - c[6] - c[5] + c[4] - c[3] + c[2] + c[1] - c[0])
    rng = np.random.default_rng(1)
    worst = {}
    direction = rng.standard_normal(6)
    for scale in (1e-3, 1e-4):
        delta = direction * (scale / np.linalg.norm(direction))
        E = I.se3(delta)
        p2 = p @ E[:3, :3].T + E[:3, 3]
        lin_err = np.abs(F(p2) - (r0 - J @ delta))
        dq = np.linalg.norm((p2 - p) @ Qr.T, axis=1)
        w2 = float(delta[:3] @ delta[:3])
        bound = (0.5 * w2 * np.linalg.norm(p, axis=1) * np.linalg.norm(n, axis=1) * 1.01 + tr * (hxy + hxz + hyz) * dq ** 2
                 + tr * hxyz * dq ** 3 + 1e-6 * scale)  # (+ the f32 rounding of J, n)
        first = np.abs(J @ delta).max()
        print(f"delta {scale:g}: max |F(E p) - (r - J delta)| {lin_err.max():.3e}, max bound {bound.max():.3e}, "
              f"first-order term {first:.3e}")
        assert (lin_err <= bound).all()
        worst[scale] = lin_err.max() / first
    assert worst[1e-4] <= worst[1e-3] / 5 and worst[1e-4] < 0.02


def test_every_code_occurs(corner):
    """A condition on the inputs: the corner through a wide camera (K 40 px), M 8 cm / 3 degrees off,
    dist_max 6 cm, gives every code 0, 2 .. 6 at least 20 times (1 never occurs: no frame normal is
    needed); so do the u16 frame's values as f64 metres; every third pixel still shows every code."""
    t, w, _ = corner
    frame, K, M, G = S.every_code_case()
    lin = S.linearize(frame, K, M, G, t, w, **S.CORNER_VOL, **S.EVERY_CODE)
    counts = np.bincount(lin["code"].ravel(), minlength=7)
    print("codes 0..6:", counts.tolist())
    assert len(counts) == 7 and counts[1] == 0 and np.delete(counts, 1).min() >= 20
    assert lin["inliers"] == counts[6] and lin["candidates"] == counts[2:].sum()
    assert (lin["resid"][lin["code"] != 6] == 0).all() and lin["resid"][lin["code"] == 6].any()
    assert lin["code"][-1].any() and lin["code"][:, -1].any()  # the last row and column take part
    as_m = S.linearize(frame.astype(np.float64) / 1000.0, K, M, G, t, w, **S.CORNER_VOL, **S.EVERY_CODE)
    assert np.array_equal(as_m["code"], lin["code"]) and np.array_equal(as_m["sums"], lin["sums"])
    third = S.linearize(frame, K, M, G, t, w, stride=3, **S.CORNER_VOL, **S.EVERY_CODE)
    c3 = np.bincount(third["code"].ravel(), minlength=7)
    print("stride 3:", c3.tolist())
    assert np.delete(c3, 1).min() >= 1
    keep = np.zeros_like(lin["code"], bool)
    keep[::3, ::3] = True
    assert np.array_equal(third["code"], np.where(keep, lin["code"], 0))


def test_restatement_converges_on_the_corner(corner):
    """The seeded starts of test_track_cpu.py, 4 cm / 2 degrees off: final error, iterations and
    cond(A) asserted at twice the values measured here (CORNER_SDF_MEASURED)."""
    t, w, _ = corner
    frame = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    for g, (mt, ma, mi, mn, mc) in zip(corner_starts(), CORNER_SDF_MEASURED):
        out = S.track(frame, I.FRAME_K, g, t, w, **S.CORNER_VOL)
        et, ea = I.pose_error(out["pose"], I.TRUE_POSE)
        print(f"corner: {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after {out['iterations']} iterations, "
              f"inliers {out['inliers'][-1]}, cond(A) {out['cond']:.0f}")
        assert out["status"] == I.CONVERGED and out["iterations"] <= 2 * mi
        assert out["inliers"][-1] >= mn // 2 and out["cond"] <= 2 * mc
        assert et <= 2 * mt and ea <= 2 * ma


def test_restatement_tracks_the_lounge():
    """test_track_cpu.py's lounge case (80 x 60, 4 cm, 3 frames fused by the oracle), with the ICP
    restatement's figures for the same starts printed beside it; no ordering of the two is asserted."""
    import oracle as O
    vol = O.OracleTSDFVolume(np.array(C1), 0.04)
    for i in range(3):
        _, depth, rgb, pose = load_lounge(i)
        vol.integrate(rgb, depth, lounge_intrinsics(), pose)
    t, w, c = vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu
    frame, K, true, starts = lounge_case()
    for g, (mt, ma, mi, mn, mc) in zip(starts, LOUNGE_SDF_MEASURED):
        out = S.track(frame, K, g, t, w, vol._vol_origin, 0.04, 5 * 0.04)
        et, ea = I.pose_error(out["pose"], true)
        dm, nm, _ = R.raycast(t, w, c, vol._vol_origin, 0.04, K, g, frame.shape, 0.0, LOUNGE_Z_FAR, 0.04)
        icp = I.track(frame, K, dm, nm, g)
        it, ia = I.pose_error(icp["pose"], true)
        print(f"lounge sdf: {1e3 * et:.3f} mm / {ea:.4f} deg, {out['status']} after {out['iterations']}, inliers "
              f"{out['inliers'][-1]}, cond(A) {out['cond']:.0f} | icp: {1e3 * it:.3f} mm / {ia:.4f} deg, {icp['status']} "
              f"after {icp['iterations']}, inliers {icp['inliers'][-1]}, cond(A) {icp['cond']:.0f}")
        assert out["status"] != I.LOST and out["iterations"] <= 2 * mi
        assert out["inliers"][-1] >= mn // 2 and out["cond"] <= 2 * mc
        assert et <= 2 * mt and ea <= 2 * ma


def sample_points(rng, n=4000):
    """World points across the corner volume and a margin around it."""
    lo, hi = I.BOUNDS[:, 0] - 0.1, I.BOUNDS[:, 1] + 0.1
    return lo + rng.random((n, 3)) * (hi - lo)


def test_sample_equals_the_raycast_cell(corner):
    """The restated sample on points across the volume and around it: all four codes occur; where
    raycast_ref's cell is valid (inside, weights > 0) the code is 4 or 6 and value and gradient are
    raycast_ref's trilinear value and gradient, scaled; elsewhere zeros.  And at the hit points of a
    reference raycast the sampled distance is near 0 and the gradient's direction is the normal map's."""
    t, w, col = corner
    P = sample_points(np.random.default_rng(2))
    sdf, grad, code = S.sample(P, t, w, **S.CORNER_VOL)
    counts = np.bincount(code, minlength=7)
    print("sample codes:", counts.tolist())
    assert set(np.flatnonzero(counts)) == {2, 3, 4, 6} and counts[[2, 3, 4, 6]].min() >= 20
    q = ((P - I.ORIGIN.astype(np.float64)) / I.VS).astype(np.float32)
    i0 = np.floor(q).astype(np.int64)
    cs, valid = R._cell(t, w, i0, np.array(t.shape), np.float32)
    assert np.array_equal(valid, code >= 4)
    f = R._trilinear(cs, q - i0.astype(np.float32))
    g = np.stack(R._gradient(cs, q - i0.astype(np.float32)), axis=1)
    assert np.array_equal(sdf[valid], (np.float32(0.1) * f)[valid])
    assert np.array_equal(grad[valid], (np.float32(np.float64(0.1) / I.VS) * g)[valid])
    assert not sdf[~valid].any() and not grad[~valid].any()
    flat = np.any([np.abs(x) >= 1 for x in cs], axis=0)
    assert np.array_equal(code[valid] == 4, flat[valid])
    # the raycast's hits
    d, nm, _ = R.raycast(t, w, col, I.ORIGIN, I.VS, I.MODEL_K, np.eye(4), I.MODEL_HW, 0.0, I.Z_FAR, I.VS)
    v, u = np.nonzero((d > 0) & (np.abs(nm).sum(axis=-1) > 0))
    z = d[v, u].astype(np.float64)
    hits = np.stack([(u - I.MODEL_K[0, 2]) / I.MODEL_K[0, 0] * z, (v - I.MODEL_K[1, 2]) / I.MODEL_K[1, 1] * z, z], axis=1)
    hs, hg, hc = S.sample(hits, t, w, **S.CORNER_VOL)
    ok = hc == 6
    assert ok.sum() > 3000
    # between two samples one voxel apart the interpolant leaves its chord by at most the mixed
    # second differences: a fraction of a voxel's tsdf step (vs / trunc = 0.2), here under 0.05 = 5 mm
    assert np.abs(hs[ok]).max() <= 5e-3
    unit = hg[ok] / np.linalg.norm(hg[ok], axis=1, keepdims=True)
    cos = np.einsum("ij,ij->i", unit, nm[v, u][ok])
    print(f"hits: {ok.sum()}, max |sdf| {np.abs(hs[ok]).max():.2e} m, min cos {cos.min():.6f}")
    assert np.median(cos) > 1 - 1e-6 and (cos > 1 - 1e-3).mean() > 0.99
