"""The conditions on the inputs of tests/test_track_edges_gpu.py, checked on the restatements alone
(tests/track_edge_cases.py): the edge volumes are what they are meant to be, the sample points reach
every face of every handle with every code, the every-code frame reaches the faces it can, the
tracks on the cut volumes keep their inliers, and the large frames put inliers and every refusal
into a lane's second trip round the grid-stride loop of an MI355X (256 compute units).  The figures
printed here are the ones the GPU tests assert again on their own references."""
import time

import numpy as np
import pytest

import icp_color_ref as C
import icp_ref as I
import raycast_ref as R
import sdf_ref as S
import track_edge_cases as E

N_CU = E.N_CU_MI355X
MIN_HITS = 250  # test_raycast_gpu.py's


def test_edge_volumes_are_cut_from_the_corner():
    full = I.corner_state()
    want = {"ragged": ((61, 45, 37), (0, 0, 0)), "ragged_hash": ((61, 45, 37), (0, 0, 0)), "slab": ((34, 45, 37), (19, 0, 0)),
            "high_slab": ((32, 48, 40), (32, 0, 0))}
    for name, (dims, off) in want.items():
        (t, w, c), o = E.state(name)
        assert t.shape == w.shape == c.shape == dims and o == off
        assert tuple(np.ceil((E.bounds(E.VOLUMES[name][0])[:, 1] - E.bounds(E.VOLUMES[name][0])[:, 0]) / I.VS).astype(int)) \
            == E.VOLUMES[name][0]
        sl = (slice(off[0], off[0] + dims[0]), slice(0, dims[1]), slice(0, dims[2]))
        if name != "ragged_hash":
            assert all(np.array_equal(a, b[sl]) for a, b in zip((t, w, c), full))
    keep = E.kept_voxels(E.RAGGED)
    (t, w, c), _ = E.state("ragged_hash")
    assert 0.6 < keep.mean() < 0.9
    assert np.array_equal(t[keep], full[0][:61, :45, :37][keep]) and (t[~keep] == 1).all()
    assert not w[~keep].any() and not c[~keep].any() and np.array_equal(w[keep], full[1][:61, :45, :37][keep])
    # blocks are left out at a partly filled last brick of every axis, and kept there too
    nb_keep = keep[::8, ::8, ::8]
    for d in range(3):
        last = np.take(nb_keep, -1, axis=d)
        assert last.any() and not last.all(), d


@pytest.mark.parametrize("name", E.SAMPLED)
def test_sample_points_reach_every_face_with_every_code(name):
    n = E.assert_sample_conditions(name)
    print(name, len(E.sample_points(name)), "points:", n)
    (sdf, grad, code), l = E.sample_ref(name)
    assert not sdf[code < 4].any() and not grad[code < 4].any()
    dims = np.array(E.state(name)[0][0].shape)
    assert np.array_equal(code == 2, ((l < 0) | (l > dims - 2)).any(axis=1))
    assert (((l & 7) == 7).any(axis=1) & (code >= 4)).sum() >= E.MIN_COUNT  # cells across a brick boundary


def test_the_ragged_hash_differs_from_the_dense_volume_only_by_its_holes():
    (_, _, cd), _ = E.sample_ref("ragged")
    (sh, gh, ch), _ = E.sample_ref("ragged_hash")
    (sd, gd, _), _ = E.sample_ref("ragged")
    sel = ch != 3
    assert np.array_equal(ch[sel], cd[sel]) and np.array_equal(sh[sel], sd[sel]) and np.array_equal(gh[sel], gd[sel])
    assert ((ch == 3) & (cd != 3)).sum() >= 1000  # the blocks left out are met


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", list(E.VOLUMES))
def test_every_code_frame_on_the_edge_volumes(name, stride):
    counts, faces = E.assert_linearize_conditions(name, stride)
    print(name, "stride", stride, "codes 0..6:", counts.tolist(), faces)
    if stride == 3:
        keep = np.zeros_like(E.linearize_ref(name, 1)["code"], bool)
        keep[::3, ::3] = True
        assert np.array_equal(E.linearize_ref(name, 3)["code"], np.where(keep, E.linearize_ref(name, 1)["code"], 0))


def test_the_face_counts_are_the_measured_ones():
    """The figures measured when these inputs were chosen: slab (19, 53) x faces 140 / 208 / 35 / 58,
    ragged +y 133 / 257."""
    _, f = E.assert_linearize_conditions("slab", 1)
    assert f["x"] == {"dims - 2": 140, "dims - 1": 208, "0": 35, "-1": 58}
    inl = (E.linearize_ref("slab", 1)["code"] == 6) & (E.linearize_ref("slab", 1)["cell"][..., 0] - 19 == 32)
    assert inl.sum() == 140  # all inliers
    _, f = E.assert_linearize_conditions("ragged", 1)
    assert (f["y"]["dims - 2"], f["y"]["dims - 1"]) == (133, 257)


@pytest.mark.parametrize("name", ["ragged", "ragged_holed", "ragged_hash", "slab"])
def test_restatement_tracks_on_the_edge_volumes(name):
    """The SDF track of the corner frame is not lost and keeps >= 1000 inliers in every iteration on
    each cut (the slab's 34 voxels are wide enough: no wider range is needed)."""
    frame, K, g = E.track_frame()
    (t, w, _), off = E.state(name)
    M, status, inl = np.eye(4), None, []
    while status is None and len(inl) < 10:
        lin = S.linearize(frame, K, M, g, t, w, index_offset=off, **S.CORNER_VOL)
        inl.append(lin["inliers"])
        M, status, _, _ = I.step(M, lin["sums"], lin["inliers"])
    print(name, status, inl)
    assert status != I.LOST and min(inl) >= 1000


@pytest.mark.parametrize("name", ["ragged_hash", "slab"])
def test_restatement_icp_and_rgbd_track_on_the_edge_volumes(name):
    """The ICP and the RGB-D track (the plane scene's grey image as the frame's colours) against the
    reference raycast of each cut: not lost, >= 1000 geometric and >= 100 colour inliers, and cond(A)
    below the 5e2 STEP_TOL was derived for in every iteration.  The colour weight is
    E.EDGE_COLOR_WEIGHT = 0.0005: measured here, the combined systems then have cond(A) <= 113 on the
    table and <= 195 on the slab, where the default 0.001 gives 546 in the slab's first iteration."""
    frame, K, g = E.track_frame()
    rgb = C.plane_render()[1]
    (t, w, c), off = E.state(name)
    d, n, col = R.raycast(t, w, c, I.ORIGIN, I.VS, K, g, frame.shape, 0.0, I.Z_FAR, I.VS, index_offset=off)
    out = I.track(frame, K, d, n, g)
    assert out["status"] != I.LOST and min(out["inliers"]) >= 1000 and out["cond"] < 5e2
    M, status, conds, inl, cin = np.eye(4), None, [], [], []
    while status is None and len(inl) < 10:
        lin = I.linearize(frame, K, M, d, n, K, g)
        cl = C.linearize_color(frame, rgb, K, M, d, col, K)
        sums = C.combine(lin["sums"], cl["sums"], E.EDGE_COLOR_WEIGHT)
        conds.append(float(np.linalg.cond(I.system(sums)[0])))
        inl.append(lin["inliers"])
        cin.append(cl["inliers"])
        M, status, _, _ = I.step(M, sums, lin["inliers"])
    print(name, "icp", out["status"], out["inliers"], f"cond {out['cond']:.0f}; rgbd", status, inl, cin, [round(x) for x in conds])
    assert status != I.LOST and min(inl) >= 1000 and min(cin) >= 100 and max(conds) < 2.5e2


@pytest.mark.parametrize("name", ["ragged_hash", "slab"])
def test_raycast_poses_hit(name):
    """The two corner poses hit the corner state of each handle; the high-face poses, which see the
    corner's planes from behind, hit the ellipsoid held by the same extent."""
    (t, w, c), off = E.state(name)
    for label, pose in E.corner_poses().items():
        d = R.raycast(t, w, c, I.ORIGIN, I.VS, I.MODEL_K, pose, I.MODEL_HW, 0.0, I.Z_FAR, I.VS, index_offset=off)[0]
        print(name, label, int((d > 0).sum()))
        assert (d > 0).sum() >= MIN_HITS
    (t, w, c), off = E.ellipsoid(name)
    for face, pose in R.high_face_poses(*E.box(name)).items():
        d = R.raycast(t, w, c, I.ORIGIN, I.VS, E.K_FACE, pose, I.MODEL_HW, 0.0, E.FACE_Z_FAR, I.VS, index_offset=off)[0]
        print(name, face, int((d > 0).sum()))
        assert (d > 0).sum() >= MIN_HITS


def test_large_frame_is_more_than_one_grid():
    hw = E.large_hw(N_CU)
    assert hw == (416, 640) and hw[0] * hw[1] > E.grid_lanes(N_CU) == 262144
    assert E.large_hw(304) == (416, 759)
    with pytest.raises(AssertionError, match="1024"):
        E.large_hw(512)


@pytest.mark.parametrize("holed", [False, True])
def test_large_sdf_frame_second_trip(holed):
    """416x640 at stride 1: the restatement takes 0.5 .. 0.9 s and finds 135 360 inliers on the whole
    volume; the second trip (45 056 pixels) holds codes 2: 2371, 3: 135, 4: 526, 5: 830, 6: 234."""
    t0 = time.perf_counter()
    ref = E.large_sdf_ref(N_CU, holed)
    dt = time.perf_counter() - t0
    tail = E.assert_second_trip(ref["code"], N_CU, 6, (2, 3, 4, 5))
    print(f"holed {holed}: {dt:.2f} s, inliers {ref['inliers']}, second trip codes 0..6 {tail.tolist()}")
    if not holed:
        assert ref["inliers"] == 135360 and tail.tolist() == [0, 0, 2371, 135, 526, 830, 234]


def test_large_sdf_frame_at_stride_2():
    """832x1280 through twice the focal length at stride 2: the same rays as 416x640 at stride 1, so
    the same codes at the sampled pixels; the restatement takes about 1 s."""
    t0 = time.perf_counter()
    ref = E.large_sdf_ref(N_CU, False, 2)
    dt = time.perf_counter() - t0
    tail = E.assert_second_trip(ref["code"], N_CU, 6, (2, 3, 4, 5), stride=2)
    print(f"stride 2: {dt:.2f} s, inliers {ref['inliers']}, second trip {tail.tolist()}")
    assert np.array_equal(ref["code"][::2, ::2], E.large_sdf_ref(N_CU)["code"]) and not ref["code"][1::2].any()


def test_large_icp_frame_second_trip():
    """The large frame against the 61x83 maps raycast from the pitched model pose: both halves have
    >= 100 inliers in the second trip (measured: 1214 geometric, 485 colour; the restatements take
    0.12 s and 0.10 s)."""
    maps = E.pitched_model_maps()
    assert (maps[0] > 0).sum() >= 2000
    t0 = time.perf_counter()
    geo, col = E.large_icp_refs(N_CU, maps)
    dt = time.perf_counter() - t0
    gt = np.bincount(E.second_trip(geo["code"], N_CU), minlength=7)
    ct = np.bincount(E.second_trip(col["code"], N_CU), minlength=6)
    print(f"both restatements {dt:.2f} s; geometry inliers {geo['inliers']}, second trip {gt.tolist()}; colour inliers "
          f"{col['inliers']}, second trip {ct.tolist()}")
    assert gt[6] >= 100 and ct[5] >= 100


def test_large_track_keeps_its_inliers():
    """Two iterations of the SDF track on the large frame of the true pose: about 1.7e5 inliers and
    cond(A) ~ 40, so with N 2^-52 ~ 4e-11 relative on the sums the pose step moves by ~ 1e-10 (< STEP_TOL)."""
    frame, K, g = E.large_track_case(N_CU)
    t, w, _ = I.corner_state()
    out = S.track(frame, K, g, t, w, **S.CORNER_VOL, max_iter=2)
    print(out["status"], out["inliers"], f"cond {out['cond']:.0f}")
    assert out["status"] == I.MAX_ITER and min(out["inliers"]) >= 100000 and out["cond"] < 1e2
