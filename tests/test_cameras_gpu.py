"""Every entry point that takes a camera matrix after the integrate, run with fx != fy and with the
principal point outside the image (tests/camera_cases.py), through the C-ABI and against the NumPy
restatements with the assertions of the existing device tests: raycast bit for bit (normals within
1e-6), linearisation maps byte-identical and sums within inliers 2^-52 sum|term|, every track step
reproduced and the final pose within twice the reference's own error, frustum bounds bit for bit.
tests/test_cameras_cpu.py shows, on the restatements alone, that these inputs reach every code and
that exchanging fx and fy changes what is compared here.  Volumes <= 128^3, images <= 83 x 61 but for
the 200-pixel strips.

    entry point                          fx != fy                              principal point outside
    tsdf_dense_raycast                   test_lounge_raycast[dense], _ragged,  test_lounge_raycast[dense] (off-right, off-left),
                                         _slab, test_tiny_raycasts[dense-*]    test_tiny_raycasts[dense-off], model_maps
    tsdf_hash_raycast                    test_lounge_raycast[hash],            test_lounge_raycast[hash], test_tiny_raycasts[hash-off]
                                         test_tiny_raycasts[hash-*]
    tsdf_icp_linearize                   test_icp_linearize[aniso-*]           test_icp_linearize[off-*]
    tsdf_icp_linearize_rgbd              test_icp_linearize_rgbd[aniso-*]      test_icp_linearize_rgbd[off-*]
    tsdf_{dense,hash}_track              test_icp_track[aniso-*]               test_icp_track[off-*]
    tsdf_{dense,hash}_track_rgbd         test_rgbd_track[aniso-*]              test_rgbd_track[off-*]
    tsdf_{dense,hash}_track_sdf          test_sdf_track[aniso-*]               test_sdf_track[off-*]
    tsdf_{dense,hash}_sdf_linearize      test_sdf_linearize[aniso-*]           test_sdf_linearize[off-*]
    tsdf_frustum_bounds                  test_frustum_bounds (first camera)    test_frustum_bounds (second camera)
(the integrate's companion cases are parameters of tests/test_pixel_fixed_gpu.py).
"""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import camera_cases as X
import icp_color_ref as C
import icp_ref as I
import oracle as O
import raycast_ref as R
import sdf_ref as S
from test_raycast_gpu import C1, HW, MIN_HITS, Z_FAR, blocks_of, check, make_dense, make_hash, poses, same
from test_track_color_gpu import follow as follow_rgbd
from test_track_gpu import follow as follow_icp
from test_track_sdf_gpu import check_linearize, follow as follow_sdf

pytestmark = pytest.mark.gpu
KINDS = ("dense", "hash")


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


@pytest.fixture(scope="module")
def frames():
    return [load_lounge(i) for i in range(3)]


def brute_twin(monkeypatch, make):
    """A second handle made by `make` that marches every sample (TSDF_RAY_SKIP=0 is read at create)."""
    monkeypatch.setenv("TSDF_RAY_SKIP", "0")
    try:
        return make()
    finally:
        monkeypatch.delenv("TSDF_RAY_SKIP")


def check_both(obj, brute, K, pose, **kw):
    """test_raycast_gpu.check against the reference, and the brute-force twin's bytes.  The skip's
    exit distances divide by the ray direction, whose x and y now scale differently."""
    got, ref = check(obj, K, pose, min_hits=MIN_HITS, **kw)
    every = brute.raycast(K, pose, HW, z_far=kw.get("z_far", Z_FAR))
    for a, b in zip(got, every):
        assert a.tobytes() == b.tobytes()
    return int((ref[0] != 0).sum())


# ---- raycast ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lounge_raycast(kind, gf, hf, frames, monkeypatch):
    """The lounge fusion (3 frames) from "frame0" and "outside" through the anisotropic camera and
    through cameras whose principal point is off the image."""
    make = (lambda: make_dense(gf, frames)) if kind == "dense" else (lambda: make_hash(hf, frames))
    obj = make()
    state = obj.get_state()
    brute = brute_twin(monkeypatch, make)
    P = poses(frames)
    for name, (K, where) in X.lounge_raycast_cameras(lounge_intrinsics()).items():
        assert K[0, 0] != K[1, 1]
        for w in where:
            print(f"lounge {kind} {name} {w}: {check_both(obj, brute, K, P[w], state=state)} hits")


def test_ragged_raycast(gf, monkeypatch):
    """The ragged sphere with holes and exact zeros in the 63 x 45 x 37 volume, through A_MODEL."""
    state = R.ragged_state()

    def make():
        vol = gf.TSDFVolume(np.array([[0.0, 0.63], [0.0, 0.45], [0.0, 0.37]]), 0.01)
        assert tuple(vol._vol_dim) == state[0].shape
        vol.set_state(*state)
        return vol

    vol, brute = make(), brute_twin(monkeypatch, make)
    for pose in R.ragged_poses():
        check_both(vol, brute, X.A_MODEL, pose, state=state, z_far=1.2)


def test_slab_raycast(gf, frames, monkeypatch):
    """The slab handle (rows 40 .. 104, index offset 40) of the lounge fusion, through A_MODEL."""
    vol = make_dense(gf, frames, slab=(40, 104))
    state = vol.get_state()
    assert state[0].shape == (64, 128, 128)

    def make():
        twin = gf.TSDFVolume(np.array(C1), 0.04, slab=(40, 104))
        twin.set_state(*state)
        return twin

    brute = brute_twin(monkeypatch, make)
    P = poses(frames)
    for w in ("frame0", "outside"):
        check_both(vol, brute, X.A_MODEL, P[w], state=state, off=(40, 0, 0))


def hash_of(hf, state):
    """A table holding `state` (the corner scene's extent), every block imported."""
    ht = hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12)
    assert tuple(ht._vol_dim) == I.SHAPE and np.array_equal(ht._vol_origin, I.ORIGIN)
    nb = [s // 8 for s in I.SHAPE]
    bxyz = np.stack(np.meshgrid(*(np.arange(n) for n in nb), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    ht.import_blocks(bxyz, *(blocks_of(a) for a in state))
    return ht


def handle_of(gf, hf, kind, state):
    if kind == "hash":
        return hash_of(hf, state)
    vol = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    assert tuple(vol._vol_dim) == I.SHAPE and np.array_equal(vol._vol_origin, I.ORIGIN)
    vol.set_state(*state)
    return vol


@pytest.fixture(scope="module")
def corner(gf, hf):
    return {kind: handle_of(gf, hf, kind, I.corner_state()) for kind in KINDS}


@pytest.fixture(scope="module")
def plane(gf, hf):
    return {kind: handle_of(gf, hf, kind, C.plane_state()) for kind in KINDS}


@pytest.mark.parametrize("name", ["aniso", "off"])
@pytest.mark.parametrize("kind", KINDS)
def test_tiny_raycasts(kind, name, corner):
    """Images smaller than a wave's 8 x 8 tile, exactly one tile, and strips 3 wide and 3 high, with
    host outputs and with device out= tensors (prefilled: every pixel is written, a miss with zeros)."""
    import torch
    obj = corner[kind]
    state = obj.get_state()
    K0, pose = (X.A_MODEL, np.eye(4)) if name == "aniso" else (X.OFF_MODEL, X.OFF_MODEL_POSE)
    dev = torch.device("cuda", 0)
    for hw, hits in zip(X.TINY, X.TINY_HITS[name]):
        K = X.scaled(K0, I.MODEL_HW, hw)
        ref = R.raycast(*state, I.ORIGIN, I.VS, K, pose, hw, 0.0, I.Z_FAR, I.VS)
        assert (ref[0] != 0).sum() == hits
        got = obj.raycast(K, pose, hw, z_far=I.Z_FAR)
        same(got, ref)
        out = (torch.full(hw, 7.0, dtype=torch.float32, device=dev), torch.full(hw + (3,), 7.0, dtype=torch.float32, device=dev),
               torch.full(hw + (3,), 7, dtype=torch.uint8, device=dev))
        assert obj.raycast(K, pose, hw, z_far=I.Z_FAR, out=out) is out
        for a, b in zip(got, out):
            assert a.tobytes() == b.cpu().numpy().tobytes()


# ---- the ICP linearisations ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_maps(corner, plane):
    """(scene, pair, pitched) -> the dense handle's raycast from the case's model pose through its model
    camera, 83 x 61: the maps the linearise tests read.  Each equals the reference raycast."""
    out = {}
    for scene, handle, state in (("corner", corner["dense"], I.corner_state()), ("plane", plane["dense"], C.plane_state())):
        for pair, pitched in X.lin_cases():
            _, Km, _, Pm, _ = X.lin_case(pair, pitched)
            got = handle.raycast(Km, Pm, I.MODEL_HW, z_far=I.Z_FAR)
            same(got, R.raycast(*state, I.ORIGIN, I.VS, Km, Pm, I.MODEL_HW, 0.0, I.Z_FAR, I.VS))
            assert (got[0] > 0).sum() > 2500 and (got[0] == 0).sum() > 200
            out[scene, pair, pitched] = got
    return out


def as_kind(frame, kind):
    return frame if kind == "u16" else frame.astype(np.float64) / 1000.0


def assert_sums(got, ref, label):
    bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
    err = np.abs(got - ref["sums"])
    print(f"{label}: inliers {ref['inliers']}, max |sum - fsum| / bound {np.max(err / bound):.3f}")
    assert ref["inliers"] >= 100 and (err <= bound).all()


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["u16", "f64"])
@pytest.mark.parametrize("pair,pitched", X.lin_cases())
def test_icp_linearize(tr, model_maps, pair, pitched, kind, stride):
    """tsdf_icp_linearize on the corner, frame 71 x 53 against model maps 83 x 61: code and residual
    maps byte-identical to the restatement, counts equal, sums within N 2^-52 sum|term|."""
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    d, n, _ = model_maps["corner", pair, pitched]
    frame = I.render(Pf, Kf, I.FRAME_HW)
    ref = I.linearize(frame, Kf, M, d, n, Km, Pm, stride=stride, **I.CORNER_GATES)
    counts = np.bincount(ref["code"].ravel(), minlength=7)
    assert stride != 1 or counts.min() >= 20, counts  # the reference shows every code
    got = tr.icp_linearize(as_kind(frame, kind), Kf, M, d, n, Km, Pm, stride=stride, dist_max=I.CORNER_GATES["dist_max"],
                           cos_min=I.CORNER_GATES["cos_min"])
    assert got["code"].tobytes() == ref["code"].tobytes()
    assert got["residual"].tobytes() == ref["resid"].tobytes()
    assert (got["inliers"], got["candidates"]) == (ref["inliers"], ref["candidates"])
    assert_sums(got["sums"], ref, f"corner {pair} pitched {pitched} {kind} stride {stride}")


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["u16", "f64"])
@pytest.mark.parametrize("pair,pitched", X.lin_cases())
def test_icp_linearize_rgbd(tr, model_maps, pair, pitched, kind, stride):
    """tsdf_icp_linearize_rgbd on the textured plane: both code maps and both residual maps
    byte-identical to the restatement, the four counts equal, the 56 sums within N 2^-52 sum|term|,
    and the geometric half tsdf_icp_linearize's to the byte."""
    Kf, Km, Pf, Pm, M = X.lin_case(pair, pitched)
    d, n, c = model_maps["plane", pair, pitched]
    frame, rgb = C.plane_render(Pf, Kf, I.FRAME_HW, extras=True)
    geo = I.linearize(frame, Kf, M, d, n, Km, Pm, stride=stride)
    col = C.linearize_color(frame, rgb, Kf, M, d, c, Km, stride=stride)
    counts = np.bincount(col["code"].ravel(), minlength=6)
    assert stride != 1 or counts.min() >= 10, counts  # the reference shows every colour code
    f = as_kind(frame, kind)
    got = tr.icp_linearize_rgbd(f, rgb, Kf, M, d, n, c, Km, Pm, stride=stride)
    assert got["color_code"].tobytes() == col["code"].tobytes()
    assert got["color_residual"].tobytes() == col["resid"].tobytes()
    assert got["code"].tobytes() == geo["code"].tobytes()
    assert got["residual"].tobytes() == geo["resid"].tobytes()
    assert (got["inliers"], got["candidates"]) == (geo["inliers"], geo["candidates"])
    assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"])
    label = f"plane {pair} pitched {pitched} {kind} stride {stride}"
    assert_sums(got["sums"], geo, label + " geometry")
    assert_sums(got["color_sums"], col, label + " colour")
    old = tr.icp_linearize(f, Kf, M, d, n, Km, Pm, stride=stride)
    assert old["sums"].tobytes() == got["sums"].tobytes()
    assert old["code"].tobytes() == got["code"].tobytes() and old["residual"].tobytes() == got["residual"].tobytes()
    assert (old["inliers"], old["candidates"]) == (got["inliers"], got["candidates"])


# ---- the trackers -------------------------------------------------------------------------------------
def assert_reaches(label, pose, info, g, true, measured):
    """The pose is the guess times the last relative pose, and within twice the reference's own error."""
    assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
    et, ea = I.pose_error(pose, true)
    print(f"{label}: {info['status']} after {info['iterations']}, inliers {info['inliers']}, {1e3 * et:.3f} mm / {ea:.4f} deg")
    assert info["status"] == "converged"
    assert et <= 2 * measured[0] and ea <= 2 * measured[1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_icp_track(pair, kind, corner, tr):
    obj = corner[kind]
    K, true, starts = X.track_case(pair)
    frame = I.render(true, K, I.FRAME_HW)
    for k, g in enumerate(starts):
        pose, info = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True)
        follow_icp(obj, tr, frame, K, g, I.Z_FAR, info)
        assert_reaches(f"icp {pair} {kind} start {k}", pose, info, g, true, X.MEASURED[pair]["icp"][k])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_rgbd_track(pair, kind, plane, tr):
    obj = plane[kind]
    K, true, starts = X.plane_track_case(pair)
    frame, rgb = C.plane_render(true, K, I.FRAME_HW)
    for k, g in enumerate(starts):
        pose, info = obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True, color_im=rgb)
        follow_rgbd(obj, tr, frame, rgb, K, g, I.Z_FAR, info)
        assert info["color_inliers"] > 2000
        assert_reaches(f"rgbd {pair} {kind} start {k}", pose, info, g, true, X.MEASURED[pair]["rgbd"][k])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_sdf_track(pair, kind, corner, tr):
    obj = corner[kind]
    tw = obj.get_state()[:2]
    K, true, starts = X.track_case(pair)
    frame = I.render(true, K, I.FRAME_HW)
    for k, g in enumerate(starts):
        pose, info = obj.track(frame, K, g, return_info=True, method="sdf")
        follow_sdf(obj, tr, frame, K, g, info, tw)
        assert_reaches(f"sdf {pair} {kind} start {k}", pose, info, g, true, X.MEASURED[pair]["sdf"][k])


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", list(X.PAIRS))
def test_sdf_linearize(pair, kind, stride, corner, tr):
    """The every-code inputs through A_FRAME / OFF_FRAME, as u16 millimetres and as f64 metres."""
    obj = corner[kind]
    t, w, _ = obj.get_state()
    frame, K, M, G = X.sdf_code_case(pair)
    ref = S.linearize(frame, K, M, G, t, w, stride=stride, **S.CORNER_VOL, **S.EVERY_CODE)
    counts = np.bincount(ref["code"].ravel(), minlength=7)
    assert np.delete(counts, 1).min() >= (20 if stride == 1 else 1), counts  # the reference shows every code
    for depth_kind in ("u16", "f64"):
        got = tr.sdf_linearize(obj, as_kind(frame, depth_kind), K, M, G, stride=stride, **S.EVERY_CODE)
        check_linearize(got, ref, f"sdf {pair} {kind} {depth_kind} stride {stride}")


# ---- frustum bounds -----------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_frustum_bounds(gf):
    """10 lounge depth frames from host memory, as raw u16 with the 65535 mask and as f64 metres,
    through fx != fy and through a principal point left of and above the image: per-frame maxima,
    frustum points and bounds equal the oracle's bit for bit."""
    fr = [load_lounge(i, color=False) for i in range(10)]
    raw = np.stack([f[0] for f in fr]).astype(np.uint16)
    metres = np.stack([f[1] for f in fr])
    P = np.stack([f[3] for f in fr])
    H, W = raw.shape[1:]
    ref_md = metres.reshape(10, -1).max(axis=1)
    for K in X.frustum_cameras(lounge_intrinsics()):
        ref_b = O.frustum_bounds(ref_md, H, W, K, P)
        ref_pts = np.stack([O.view_frustum(ref_md[i], H, W, K, P[i]) for i in range(10)])
        for depth, inval in ((raw, True), (metres, False)):
            b, md, pts = gf.view_frustum_bounds(depth, K, P, invalid_65535=inval, return_max_depth=True, return_points=True)
            assert np.array_equal(_bits(md), _bits(ref_md))
            assert np.array_equal(_bits(pts), _bits(ref_pts))
            assert np.array_equal(_bits(b), _bits(ref_b))
