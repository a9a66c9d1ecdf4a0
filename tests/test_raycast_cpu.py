"""The raycast contract's NumPy restatement (tests/raycast_ref.py) checked on the CPU: against an
analytic plane, on the contract's miss cases, the live-brick rule behind the kernels' skipping,
and the fused lounge model against the depth image it was fused from."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import raycast_ref as R

VS = 0.02
SHAPE = (64, 48, 40)
ORIGIN = np.array([-0.625, -0.5, 0.5], np.float32)  # (exact in f32)
HW = (61, 83)
K = np.array([[101.3, 0.0, 41.2], [0.0, 101.3, 29.7], [0.0, 0.0, 1.0]])
N = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])  # oblique, facing the camera
P0 = np.array([0.0, 0.0, 0.907])  # (no ray meets the plane exactly at a sample: f = 0 there is a miss)
# Largest |f32 reference depth - analytic depth| over the 83x61 rays, measured here: 1.26e-7 m
# (depths 0.77 .. 1.11 m: f32 ulp there is 6e-8 .. 1.2e-7; f64 mode: 2.4e-10 m, the f32 rounding of
# the stored tsdf).  The test asserts four times the f32 figure.
PLANE_ERR_F32 = 1.26e-7


def plane_state():
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in SHAPE), indexing="ij")
    p = np.stack([x, y, z], axis=-1) * VS + ORIGIN.astype(np.float64)
    sdf = (p - P0) @ N
    t = np.clip(sdf / (5 * VS), -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 1 << 24, size=SHAPE).astype(np.float32)
    return t, np.ones(SHAPE, np.float32), c


def analytic_depth():
    v, u = np.meshgrid(np.arange(HW[0], dtype=np.float64), np.arange(HW[1], dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    return (P0 @ N) / (d @ N)


def cast(state, pose=np.eye(4), z_far=2.0, dtype=np.float32, **kw):
    return R.raycast(*state, ORIGIN, VS, K, pose, HW, 0.0, z_far, VS, dtype=dtype, **kw)


@pytest.fixture(scope="module")
def plane():
    return plane_state()


def test_plane_depth_equals_the_analytic_depth(plane):
    """Trilinear interpolation is exact on a linear field and the last positive sample's cell lies in
    the unclipped band, so the reference's depth is the ray-plane depth up to rounding: measured
    1.26e-7 m in f32 (2.4e-10 m in f64) over depths of 0.77 .. 1.11 m; asserted at 4x the f32 figure.
    The normal is the plane's, the colour that of the voxel nearest the hit."""
    za = analytic_depth()
    d64, n64, _, i64 = cast(plane, dtype=np.float64, info=True)
    d32, n32, c32, i32 = cast(plane, info=True)
    assert i32["hit"].all() and i64["hit"].all()
    e32, e64 = np.abs(d32.astype(np.float64) - za).max(), np.abs(d64 - za).max()
    print(f"plane: max |depth - analytic| f32 {e32:.3e} m, f64 {e64:.3e} m; depth {za.min():.3f} .. {za.max():.3f}")
    assert e32 <= 4 * PLANE_ERR_F32
    assert e64 <= 4 * PLANE_ERR_F32
    assert np.abs(n32 - N).max() <= 1e-4 and np.abs(n64 - N).max() <= 1e-6
    # colour: the voxel at round(q(z*))
    qo, qd = R.ray_setup(ORIGIN, VS, K, np.eye(4), HW)
    q = qo + qd * d32.reshape(-1, 1)
    rv = np.rint(q).astype(int)
    assert np.array_equal(c32.reshape(-1, 3), R.decode_color(plane[2][rv[:, 0], rv[:, 1], rv[:, 2]]))


def test_ray_from_behind_the_plane_misses(plane):
    pose = np.diag([-1.0, 1.0, -1.0, 1.0])  # turned about y, looking back along -z
    pose[:3, 3] = [0.0, 0.0, 1.25]          # inside the volume, behind the plane
    d, n, c, info = cast(plane, pose=pose, info=True)
    assert info["decided"].any() and not info["hit"].any()
    assert not d.any() and not n.any() and not c.any()


def test_weight_zero_corner_of_the_last_positive_sample_turns_a_hit_into_a_miss(plane):
    t, w, c = plane
    d, _, _, info = cast(plane, info=True)
    ray = (HW[0] // 2) * HW[1] + HW[1] // 2
    assert info["hit"][ray]
    qo, qd = R.ray_setup(ORIGIN, VS, K, np.eye(4), HW)
    zk = np.float32(info["k"][ray] - 1) * np.float32(VS)
    cell = np.floor(qo[ray] + qd[ray] * zk).astype(int)
    w2 = w.copy()
    w2[cell[0] + 1, cell[1], cell[2] + 1] = 0.0
    d2, n2, c2, info2 = cast((t, w2, c), info=True)
    assert not info2["hit"][ray] and d2.reshape(-1)[ray] == 0 and not n2.reshape(-1, 3)[ray].any()
    assert info2["hit"].sum() >= info["hit"].sum() - 64  # only the rays through that voxel change


def test_z_far_in_front_of_the_surface_misses(plane):
    d, _, _, info = cast(plane, z_far=0.6, info=True)
    assert not info["decided"].any() and not d.any()


def test_every_deciding_sample_lies_in_a_live_brick():
    """The skip argument: a sample can decide a ray only if its cell's brick is live."""
    t, w, c = R.ragged_state()
    live = R.live_bricks(t, w)
    assert live.shape == (8, 6, 5) and live.any() and not live.all()
    n = 0
    for pose in R.ragged_poses():
        *_, info = R.raycast(t, w, c, np.zeros(3, np.float32), 0.01, K, pose, HW, 0.0, 1.2, 0.01, info=True)
        cell = info["cell"][info["decided"]]
        b = cell >> 3
        assert live[b[:, 0], b[:, 1], b[:, 2]].all()
        assert info["hit"].sum() > 500
        n += len(cell)
    assert n > 2000


def test_reference_raycast_of_the_fused_lounge_model_matches_the_input_depth():
    """Model against input: lounge C1 at 0.04 m, 3 frames fused (CPU oracle), raycast from frame 0's
    pose on every 4th pixel; the median |raycast - input depth| over the pixels valid in both is
    below one voxel."""
    import oracle as O
    Kl = lounge_intrinsics()
    vol = O.OracleTSDFVolume(np.array([[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]), 0.04)
    frames = [load_lounge(i) for i in range(3)]
    for _, depth, rgb, pose in frames:
        vol.integrate(rgb, depth, Kl, pose)
    depth0, pose0 = frames[0][1], frames[0][3]
    s = 4
    Ks = Kl.copy()
    Ks[:2] /= s  # pixel u of the small image is pixel s*u of the frame
    hw = (depth0.shape[0] // s, depth0.shape[1] // s)
    d, _, _ = R.raycast(vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu, vol._vol_origin, 0.04,
                        Ks, pose0, hw, 0.0, 6.0, 0.04)
    ref = depth0[::s, ::s][:hw[0], :hw[1]]
    both = (d > 0) & (ref > 0)
    med = float(np.median(np.abs(d[both] - ref[both])))
    print(f"lounge: {both.sum()} of {both.size} pixels valid in both, median |raycast - input| {med:.4f} m")
    assert both.sum() > 0.3 * both.size
    assert med < 0.04
