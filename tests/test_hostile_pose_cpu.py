"""The hostile poses, intrinsics and points of tests/hostile_pose.py on the CPU alone: the oracle against
the fixture the reference itself produced (tools/gen_golden.py, "hostile_pose"), the conditions that
keep the device tests from passing vacuously, the restatements of raycast, tracking, sampling and
merge on every case (they assert every gather index themselves), and the stand-alone sanitizer run
of tools/check_pixel_fixed.c with the hostile rows and intrinsics."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, REPO
import hostile_pose as P
import icp_color_ref as C
import icp_ref as I
import merge_ref as M
import oracle as O
import raycast_ref as R
import sdf_ref as S

CASES = P.frame_cases()
CASE_FORMS = [(n, f) for n, c in CASES.items() for f in P.forms(c)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "hostile_pose.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_fixture_holds_the_shared_inputs(gold):
    assert list(gold["names"]) == list(CASES) and np.array_equal(gold["K_good"], P.K) and tuple(gold["hw"]) == P.HW
    for name, c in CASES.items():
        assert np.array_equal(bits(gold[name + "/rows"]), bits(c["rows"])), name
        assert np.array_equal(bits(gold[name + "/K"]), bits(c["K"])), name
        assert (name + "/pose" in gold.files) == (c["pose"] is not None)
        if c["pose"] is not None:
            assert np.array_equal(bits(gold[name + "/pose"]), bits(c["pose"])), name
    for vol in P.VOLUMES:
        orc = P.new_oracle(vol)
        assert P.preload(orc, vol) >= MIN_PRELOAD
        assert digest(orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu) == str(gold["preload_sha_" + vol])
        assert int((orc._weight_vol_cpu > 0).sum()) == int(gold["preload_n_" + vol])
    assert os.path.getsize(os.path.join(GOLD, "hostile_pose.npz")) < 512 * 1024


MIN_PRELOAD = 10000


def test_the_case_table_holds_what_it_names():
    """Every class of the issue is in the table, with the property its name claims."""
    pc, ic = P.pose_cases(), P.intrinsics_cases()
    assert np.isnan(pc["nan_all"]["rows"]).all()
    g = P.good_rows()
    for k, ax in enumerate("xyz"):
        r = pc["nan_t" + ax]["rows"]
        assert np.isnan(r[k, 3]) and np.isnan(r).sum() == 1 and np.isnan(pc["nan_t" + ax]["pose"]).sum() == 1
    assert pc["inf_tz_pos"]["rows"][2, 3] == np.inf and pc["inf_tz_neg"]["rows"][2, 3] == -np.inf
    with np.errstate(over="ignore"):
        f32 = {k: np.float32(pc["huge_" + k]["rows"][2, 3]) for k in ("1e30", "1e39", "1e300", "1e307")}
        assert np.isfinite(f32["1e30"]) and all(np.isinf(f32[k]) for k in ("1e39", "1e300", "1e307"))
        assert np.isfinite(pc["huge_1e300"]["rows"][:3] * 60.0).all() and np.isinf(pc["huge_1e307"]["rows"][0, 3] * 60.0)
    assert not pc["zero_row3"]["rows"][2].any() and pc["zero_row3"]["rows"][:2].any() and pc["zero_row3"]["pose"] is None
    assert not pc["zero_all"]["rows"].any() and not pc["zero_all"]["pose"].any()
    # the camera centre is a voxel centre, the voxel size a power of two, the pose axis-aligned
    c = pc["centre"]
    b, vs = P.VOLUMES[c["vol"]]
    assert np.log2(vs) == int(np.log2(vs)) and np.array_equal(c["rows"][:3, :3], np.eye(3))
    idx = (-c["rows"][:3, 3] - np.array([x[0] for x in b])) / vs
    assert np.array_equal(idx, np.rint(idx)) and (idx > 0).all() and (idx < np.array(P.DIMS) - 1).all()
    for name, det in (("scale_2", 8.0), ("scale_half", 0.125), ("scale_1_2_half", 1.0), ("shear", None), ("mirror", -1.0)):
        A = pc[name]["rows"][:3, :3]
        assert not np.allclose(A.T @ A, np.eye(3)) or det == -1.0
        if det is not None:
            assert np.isclose(np.linalg.det(A), det)
    for n in ("fx_neg", "fy_neg", "fxy_neg", "fx_zero", "fx_1e-30", "fx_1e30", "fx_nan", "fx_inf", "fx_ninf", "cx_nan", "cx_inf", "cx_ninf",
              "cy_nan", "cy_inf", "cy_ninf", "cx_70000", "cx_1e30", "skew_k22"):
        assert n in ic
    assert ic["skew_k22"]["K"][0, 1] != 0 and ic["skew_k22"]["K"][2, 2] != 1


@pytest.mark.parametrize("name,form", CASE_FORMS)
def test_oracle_equals_the_reference_bit_for_bit(gold, name, form):
    """Dense (tsdf, weight, colour) after the case's frame on the preloaded volume, the voxels it
    changed, and the hash path's key set and entries on a fresh table: the reference's, through the
    fixture.  Where the reference raised, the oracle's front end raises the same type."""
    p = "%s/%s/" % (name, form)
    raised = str(gold[p + "raised"])
    c = CASES[name]
    if raised:
        assert raised == "LinAlgError" and name == "zero_all" and form == "pose"
        with pytest.raises(np.linalg.LinAlgError):
            P.oracle_single(name, form)
        return
    orc, n = P.oracle_single(name, form)
    pre = P.new_oracle(c["vol"])
    P.preload(pre, c["vol"])
    changed = orc._weight_vol_cpu.reshape(-1) != pre._weight_vol_cpu.reshape(-1)
    assert n == int(gold[p + "nupd"]) == int(changed.sum())
    assert np.array_equal(np.packbits(changed), gold[p + "mask"])
    assert digest(orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu) == str(gold[p + "sha"])
    assert not np.isnan(orc._tsdf_vol_cpu).any() and not np.isnan(orc._color_vol_cpu).any()
    hv = P.new_oracle(c["vol"], "hash")
    with np.errstate(all="ignore"):
        hv.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], None, rows=P.case_rows(c, form))
    has = hv.weight > 0
    assert np.array_equal(np.packbits(has.reshape(-1)), gold[p + "hash_mask"])
    assert digest(hv.sdf[has], hv.weight[has], hv.color[has]) == str(gold[p + "hash_sha"])


def same_or_nan(got, want):
    """Bit for bit where the reference holds a number, NaN where it holds a NaN."""
    ok = ~np.isnan(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[ok], bits(want)[ok])


def test_frustum_oracle_equals_the_reference(gold):
    """get_view_frustum of every case that has a pose, and the demo's bounds (np.minimum / np.amin: a
    NaN stays) over each case alone and over all of them in the fixture's order: the oracle's points
    and bounds are the reference's.  The NaN coordinates here are the pose's or K's (the max depth is
    finite), which tsdf_frustum_bounds keeps as the reference does (include/tsdf_hip.h)."""
    Hh, W = P.HW
    order = list(gold["frustum_order"])
    assert sorted(order) == sorted(n for n, c in CASES.items() if c["pose"] is not None)
    run = np.zeros((3, 2))
    n_nan = 0
    for k, name in enumerate(order):
        c = CASES[name]
        md = float(P.depth_m(c["vol"], P.PRELOAD).max())
        with np.errstate(all="ignore"):
            assert same_or_nan(O.view_frustum(md, Hh, W, c["K"], c["pose"]), gold[name + "/pose/frustum"]), name
            alone = O.frustum_bounds([md], Hh, W, c["K"], [c["pose"]])
            run = O.frustum_bounds([md], Hh, W, c["K"], [c["pose"]], init=run)
        assert same_or_nan(alone, gold[name + "/pose/frustum_bounds"]), name
        assert same_or_nan(run, gold["frustum_running"][k]), name
        n_nan += bool(np.isnan(alone).any())
    # both kinds are there: the finite ones come first and fold to finite and infinite bounds
    first_nan = next(k for k, n in enumerate(order) if np.isnan(gold[n + "/pose/frustum_bounds"]).any())
    assert first_nan >= 15 and n_nan >= 10 and not np.isnan(gold["frustum_running"][first_nan - 1]).any()
    assert np.isnan(gold["nan_all/pose/frustum_bounds"]).all() and np.isnan(gold["fx_zero/pose/frustum_bounds"][0]).all()
    assert np.isinf(gold["inf_tz_pos/pose/frustum_bounds"]).any()


# ---- the conditions that keep the device tests from passing vacuously ---------------------------------
def test_every_case_does_what_its_class_says_on_the_oracle():
    counts = {}
    for name, form in CASE_FORMS:
        if (name, form) == ("zero_all", "pose"):
            continue
        counts[name, form] = n = P.oracle_single(name, form)[1]
        exp = CASES[name]["expect"]
        assert (n == 0) if exp == "noop" else (n >= P.MIN_ACTIVE if exp == "active" else True), (name, form, n)
    print(counts)
    for name in ("scale_2", "scale_half", "scale_1_2_half", "shear", "mirror", "fx_neg", "fy_neg", "fxy_neg", "fx_zero", "centre"):
        assert CASES[name]["expect"] == "active"
    # the camera on a voxel centre: one voxel at the origin of the camera frame, a plane with z == 0,
    # half of the volume behind it
    c = CASES["centre"]
    b, vs = P.VOLUMES[c["vol"]]
    g = [np.float32(b[a][0]) + vs * np.arange(P.DIMS[a]) + c["rows"][a, 3] for a in range(3)]
    x, y, z = np.meshgrid(*g, indexing="ij")
    assert int(((x == 0) & (y == 0) & (z == 0)).sum()) == 1 and int((z == 0).sum()) == P.DIMS[0] * P.DIMS[1]
    assert int((z < 0).sum()) == P.DIMS[0] * P.DIMS[1] * 10 and int((x == 0).sum()) == P.DIMS[1] * P.DIMS[2]


@pytest.mark.parametrize("n,at", P.BATCHES)
def test_the_good_frames_of_a_mixed_batch_change_enough(n, at):
    """Per batch size: the good frames change >= 1000 voxels each, and a batch with a no-op case in it
    ends in the state of the batch without that frame."""
    for name in ("nan_all", "mirror", "fx_zero"):
        orc, counts = P.oracle_batch(name, "rows", n, at)
        assert len(counts) == n and all(c >= P.MIN_GOOD for f, c in enumerate(counts) if f != at), (name, counts)
        exp = CASES[name]["expect"]
        assert counts[at] == 0 if exp == "noop" else counts[at] >= P.MIN_ACTIVE
    c = CASES["nan_all"]
    without = P.new_oracle("4cm")
    P.preload(without, "4cm")
    T = P.batch_rows("4cm", n, at, c["rows"])
    d, col = P.batch_images("4cm", n)
    for f in range(n):
        if f != at:
            without.integrate(col[f], d[f].astype(np.float64) / 1000.0, P.K, None, rows=T[f])
    orc, _ = P.oracle_batch("nan_all", "rows", n, at)
    assert np.array_equal(orc._tsdf_vol_cpu, without._tsdf_vol_cpu) and np.array_equal(orc._weight_vol_cpu, without._weight_vol_cpu)


def test_u16_and_f64_frames_carry_the_same_metres():
    for vol in P.VOLUMES:
        mm = P.depth_mm(vol, P.PRELOAD)
        assert mm.dtype == np.uint16 and (mm == 0).sum() == 40 and mm.max() < 65535
        k = mm.astype(np.float64)
        assert np.array_equal(np.rint(P.depth_m(vol, P.PRELOAD) * 1000.0), k)


# ---- the restatements are defined on every case ----------------------------------------------------
@pytest.fixture(scope="module")
def corner():
    return I.corner_state()


@pytest.mark.parametrize("name", list(P.scene_poses(np.eye(4), I.ORIGIN, I.VS)))
def test_raycast_restatement_is_defined_on_every_pose(corner, name):
    """raycast_ref on the corner scene from every hostile pose: it returns (its own asserts check every
    gather index and every float -> int conversion), deterministic, and a pose that holds a NaN or
    an infinity sees nothing."""
    pose = P.scene_poses(np.eye(4), I.ORIGIN, I.VS)[name]
    with np.errstate(all="ignore"):
        d, n, c = R.raycast(*corner, I.ORIGIN, I.VS, I.MODEL_K, pose, I.MODEL_HW, 0.0, I.Z_FAR, I.VS)
        d2, _, _ = R.raycast(*corner, I.ORIGIN, I.VS, I.MODEL_K, pose, I.MODEL_HW, 0.0, I.Z_FAR, I.VS)
    assert d.tobytes() == d2.tobytes() and not np.isnan(d).any() and not np.isnan(n).any()
    if not np.isfinite(pose[:3]).all():
        assert not d.any() and not n.any() and not c.any()
    print(name, int((d != 0).sum()), "hits")


@pytest.mark.parametrize("name", list(P.scene_intrinsics(I.MODEL_K)))
def test_raycast_restatement_is_defined_on_every_intrinsics(corner, name):
    K = P.scene_intrinsics(I.MODEL_K)[name]
    with np.errstate(all="ignore"):
        d, n, c = R.raycast(*corner, I.ORIGIN, I.VS, K, np.eye(4), I.MODEL_HW, 0.0, I.Z_FAR, I.VS)
    assert not np.isnan(d).any() and not np.isnan(n).any()
    if np.isnan(K[:2]).any():
        assert not d.any()
    print(name, int((d != 0).sum()), "hits")


@pytest.fixture(scope="module")
def corner_maps(corner):
    return R.raycast(*corner, I.ORIGIN, I.VS, I.MODEL_K, np.eye(4), I.MODEL_HW, 0.0, I.Z_FAR, I.VS)


def test_linearize_restatements_are_defined_on_every_guess_and_K(corner, corner_maps):
    """icp_ref, icp_color_ref and sdf_ref with every hostile pose as the relative pose / the guess and
    every hostile K as the frame's intrinsics: codes in range, finite sums (an inlier's row is made of
    finite numbers), no inlier where the pose or K holds a NaN."""
    md, mn, mc = corner_maps
    frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    rgb = np.repeat(frame[..., None] >> 4, 3, axis=-1).astype(np.uint8)
    t, w, _ = corner
    poses = P.scene_poses(np.eye(4), I.ORIGIN, I.VS)
    Ks = P.scene_intrinsics(I.FRAME_K)
    runs = [(n, I.FRAME_K, p) for n, p in poses.items()] + [(n, k, np.eye(4)) for n, k in Ks.items()]
    for name, K, pose in runs:
        with np.errstate(all="ignore"):
            geo = I.linearize(frame, K, pose, md, mn, I.MODEL_K, np.eye(4))
            col = C.linearize_color(frame, rgb, K, pose, md, mc, I.MODEL_K)
            sdf = S.linearize(frame, K, np.eye(4), pose, t, w, **S.CORNER_VOL)
        for ref, top in ((geo, 6), (col, 5), (sdf, 6)):
            assert ref["code"].max() <= top and np.isfinite(ref["sums"]).all(), name
            if np.isnan(pose).any() or np.isnan(K[:2]).any():
                assert ref["inliers"] == 0, name


def test_the_rigid_guess_rule_admits_poses_read_from_text():
    """The rule the track entry points refuse a guess by, at its tolerance of 1e-3: the lounge poses
    (eight printed digits, R^T R off by up to 1.5e-4) and every seeded start pass, as do the guesses
    whose translation alone is hostile; the scaled, sheared, mirrored, zero and NaN rotations do not,
    by a margin: the nearest of them is off by more than 0.1."""
    from conftest import load_lounge
    from test_track_cpu import corner_starts
    worst = max(np.abs(p[:3, :3].T @ p[:3, :3] - np.eye(3)).max() for p in (load_lounge(i, color=False)[3] for i in range(10)))
    assert 1e-5 < worst < 2e-4 and all(P.guess_is_rigid(load_lounge(i, color=False)[3]) for i in range(10))
    assert all(P.guess_is_rigid(g) for g in corner_starts())
    poses = P.scene_poses(corner_starts()[0], I.ORIGIN, I.VS)
    bad = {n for n, p in poses.items() if not P.guess_is_rigid(p)}
    assert bad == {"nan_all", "zero_row3", "zero_all", "scale_2", "scale_half", "scale_1_2_half", "shear", "mirror"}
    for n in bad - {"nan_all"}:
        R = poses[n][:3, :3]
        assert max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0)) > 0.1, n


def test_sample_restatement_on_the_hostile_points(corner):
    """sdf_ref.sample at every hostile point, on the corner volume and with the largest and the smallest
    index offset tsdf_dense_create accepts: a hostile point has code 2 and zeros, its finite neighbour a
    code >= 3; the cell index of a clamped coordinate minus the offset stays inside an int32."""
    t, w, _ = corner
    dims = np.array(t.shape)
    for off in ((0, 0, 0), tuple(int(x) for x in P.MAX_OFFSET - dims)):
        names, pts = P.sample_points(I.ORIGIN, I.VS, t.shape, off)
        with np.errstate(all="ignore"):
            sdf, grad, code = S.sample(pts, t, w, **S.CORNER_VOL, index_offset=off)
            q = ((pts - I.ORIGIN.astype(np.float64)) / np.float64(I.VS)).astype(np.float32)
        l = np.floor(R.clamp_index(q)).astype(np.int64) - np.array(off)
        assert l.min() >= -(1 << 31) and l.max() < (1 << 31)
        hostile = np.array([n != "neighbour" for n in names])
        assert (code[hostile] == 2).all() and not sdf[hostile].any() and not grad[hostile].any()
        assert (code[~hostile] >= 3).all() and (code[~hostile] >= 4).sum() >= 20, (off, np.bincount(code[~hostile]))
        assert not np.isnan(sdf).any() and not np.isnan(grad).any()
    assert {n.rsplit("_", 1)[0] for n in names if n != "neighbour"} == set(P.POINT_VALUES)


def test_merge_restatement_refuses_what_the_device_refuses():
    """merge_ref.check_transform: NaN or an infinity in any of the 12 entries, scales, a shear and a
    mirror are no rigid transform; a translation of 1e30 is one, and merges nothing."""
    T = M.CASES["rot"][1]
    for r in range(3):
        for c in range(4):
            for v in (np.nan, np.inf, -np.inf):
                b = np.array(T)
                b[r, c] = v
                assert not M.check_transform(b)
    for name, b in P.merge_nonrigid(T).items():
        assert not M.check_transform(b), name
    far = P.merge_far(T)
    assert M.check_transform(far)
    dst = M.CASES["rot"][0]
    code, _, _ = M.sample(dst, M.SRC, *M.source_state(), far)
    assert (code == M.OUTSIDE).all()


# ---- the fast pixel path's host side, under the sanitizers --------------------------------------------
def test_pixel_fixed_checker_runs_clean_under_the_sanitizers(tmp_path):
    """tools/check_pixel_fixed.c, a plain C program with its own main that links only host code, built
    with -fsanitize=undefined,address: its case "hostile" holds the hostile rows and intrinsics."""
    exe = os.path.join(tmp_path, "chk")
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "check_pixel_fixed.c"), "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    m = re.search(r"pixel_fixed hostile checked (\d+) fine (\d+) bad (\d+)", out.stdout)
    assert m and int(m.group(1)) > 500000 and int(m.group(2)) > 100000 and int(m.group(3)) == 0, out.stdout
