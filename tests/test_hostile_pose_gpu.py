"""The hostile poses, intrinsics and points of tests/hostile_pose.py on the device: NaN, infinite, huge,
singular, zero and non-rigid inv(cam_pose) rows and camera poses, negative, zero, tiny, huge and
non-finite focal lengths and principal points, through every way into the dense and the hash
integrate (against the oracle, which tests/test_hostile_pose_cpu.py pins to the reference), the
frustum bounds (against the reference's own points and bounds, through the fixture), the raycast, the
trackers and their linearisations (against the restatements), sample() at NaN, infinite and huge
points on handles with the smallest and the largest index offset, and the merge's refusals.  Volume
40 x 24 x 20 at 4 cm and 0.0625 m, images 80 x 60; raycast and tracking on the corner scene's cuts."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLD
import hostile_pose as P
import icp_color_ref as C
import icp_ref as I
import oracle as O
import raycast_ref as R
import sdf_ref as S
import track_edge_cases as E
from test_raycast_gpu import same as same_maps
from test_track_edges_gpu import make
from test_track_sdf_gpu import STEP_TOL, check_linearize

pytestmark = pytest.mark.gpu
CASES = P.frame_cases()
CASE_FORMS = [(n, f) for n, c in CASES.items() for f in P.forms(c)]


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
def gold():
    return np.load(os.path.join(GOLD, "hostile_pose.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_or_nan(got, want):
    """Bit for bit where the reference holds a number, NaN where it holds a NaN."""
    ok = ~np.isnan(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[ok], bits(want)[ok])


# ---- the oracle's results, computed once ------------------------------------------------------------
def fields(orc):
    return orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu


@functools.lru_cache(maxsize=None)
def preload_state(vol):
    orc = P.new_oracle(vol)
    P.preload(orc, vol)
    return tuple(a.copy() for a in fields(orc))


@functools.lru_cache(maxsize=None)
def want_single(name, form):
    orc, n = P.oracle_single(name, form)
    return tuple(a.copy() for a in fields(orc)), n


@functools.lru_cache(maxsize=None)
def want_batch(name, form, n, at):
    """A case that changes nothing shares the result of the good frames alone."""
    if CASES[name]["expect"] == "noop" and name != "nan_all":
        assert want_single(name, form)[1] == 0
        return want_batch("nan_all", "rows", n, at)
    orc, counts = P.oracle_batch(name, form, n, at)
    return tuple(a.copy() for a in fields(orc)), sum(counts)


def same_state(got, want, rows, label):
    for a, b, what in zip(got, want, ("tsdf", "weight", "colour")):
        b = b[rows]
        assert not np.isnan(a).any(), (label, what)
        diff = bits(a) != bits(b)
        assert not diff.any(), (label, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ---- dense integrate ----------------------------------------------------------------------------------
# depth kind, where the frames live, texel route (u16 + RGB8 only) or in place, prep / cull pipeline, shard
DENSE = {
    "u16-host-texel-pipe": dict(depth="u16", device=False, texel="1", pipe="1", shard=None),
    "u16-device-inplace-pipe": dict(depth="u16", device=True, texel="0", pipe="1", shard=None),
    "u16-host-texel-nopipe": dict(depth="u16", device=False, texel="1", pipe="0", shard=None),
    "f64-host-nopipe": dict(depth="f64", device=False, texel="1", pipe="0", shard=None),
    "f64-device-pipe": dict(depth="f64", device=True, texel="0", pipe="1", shard=None),
    "u16-host-inplace-nopipe-slab": dict(depth="u16", device=False, texel="0", pipe="0", shard=("slab", (13, 31))),
    "u16-host-texel-pipe-cyclic": dict(depth="u16", device=False, texel="1", pipe="1", shard=("cyclic", (1, 3))),
    "f64-host-pipe-cyclic": dict(depth="f64", device=False, texel="0", pipe="1", shard=("cyclic", (0, 3))),
}


def set_env(monkeypatch, cfg, batch):
    for k in ("TSDF_TEXEL", "TSDF_PIPELINE", "TSDF_DENSE_NZ", "TSDF_BATCH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSDF_BATCH", str(batch))
    monkeypatch.setenv("TSDF_PIPELINE", cfg["pipe"])
    if "texel" in cfg:
        monkeypatch.setenv("TSDF_TEXEL", cfg["texel"])


def dense_handle(gf, vol, cfg):
    b, vs = P.VOLUMES[vol]
    kw = {} if cfg["shard"] is None else ({"slab": cfg["shard"][1]} if cfg["shard"][0] == "slab" else {"shard": cfg["shard"][1]})
    h = gf.TSDFVolume(np.array(b), vs, **kw)
    assert tuple(int(x) for x in h._vol_dim) == P.DIMS
    return h


def frames_of(cfg, depth_mm, rgb):
    """(depth argument, colour argument, extra keywords, what to keep alive) for integrate_batch."""
    from tsdf_amd import _ffi
    d = depth_mm if cfg["depth"] == "u16" else depth_mm.astype(np.float64) / 1000.0
    if not cfg["device"]:
        return d, rgb, {}, None
    import torch
    td = torch.from_numpy(d.view(np.int16) if cfg["depth"] == "u16" else d).cuda()
    tc = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()  # the handle's stream does not follow torch's
    kind = _ffi.DEPTH_U16_MM if cfg["depth"] == "u16" else _ffi.DEPTH_F64_M
    return td.data_ptr(), tc.data_ptr(), dict(depth_kind=kind, hw=P.HW, device_ptrs=True), (td, tc)


def run_frames(h, cfg, case, rows, depth_mm, rgb, at):
    """The frames through integrate_batch: one call, or -- the case's K differs from the good one, and
    a call takes one K -- the frames before `at`, the case's and those after it in three calls."""
    cuts = [(0, len(rows), P.K)] if case["K"] is P.K else [(0, at, P.K), (at, at + 1, case["K"]), (at + 1, len(rows), P.K)]
    for a, b, K in cuts:
        if a == b:
            continue
        d, c, kw, keep = frames_of(cfg, depth_mm[a:b], rgb[a:b])
        h.integrate_batch(d, c, K, rows[a:b], **kw)
        del keep


@pytest.mark.parametrize("cfg", list(DENSE))
def test_dense_single_hostile_frame_on_a_preloaded_volume(gf, monkeypatch, cfg):
    """Every case, as rows and as a pose, alone on the preloaded volume: tsdf, weight and colour equal the
    oracle's bit for bit, the update count is its count; a case that is a no-op leaves the preload."""
    cfg = DENSE[cfg]
    set_env(monkeypatch, cfg, 8)
    hs = {vol: dense_handle(gf, vol, cfg) for vol in P.VOLUMES}
    for name, form in CASE_FORMS:
        if (name, form) == ("zero_all", "pose"):
            continue
        c = CASES[name]
        h = hs[c["vol"]]
        rows_x = h.x_index
        pre = preload_state(c["vol"])
        h.reset()
        h.set_state(*(a[rows_x] for a in pre))
        h.stats(reset=True)
        run_frames(h, cfg, c, P.case_rows(c, form)[None], P.depth_mm(c["vol"], P.PRELOAD)[None], P.rgb(P.PRELOAD)[None], 0)
        want, n = want_single(name, form)
        same_state(h.get_state(), want, rows_x, (name, form))
        st = h.stats()
        assert st["list_errors"] == 0
        if cfg["shard"] is None:
            assert st["voxel_updates"] == n, (name, form, st["voxel_updates"], n)
        if c["expect"] == "noop":
            same_state(h.get_state(), pre, rows_x, (name, form, "preload"))
            assert st["voxel_updates"] == 0
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("n,at", P.BATCHES)
@pytest.mark.parametrize("cfg", list(DENSE))
def test_dense_hostile_frame_inside_a_batch(gf, monkeypatch, cfg, n, at):
    """Frame 3 of 8 and frame 17 of 32 among good frames: the oracle over the same frames, bit for bit.
    The pose cases run inside one launch with the good frames.  A call takes one K, so an intrinsics case
    is three calls -- the frames before it, the hostile frame as a launch of its own, the frames after
    it -- and is never inside a launch with good frames."""
    cfg = DENSE[cfg]
    set_env(monkeypatch, cfg, n)
    hs = {vol: dense_handle(gf, vol, cfg) for vol in P.VOLUMES}
    for name, form in CASE_FORMS:
        if (name, form) == ("zero_all", "pose"):
            continue
        c = CASES[name]
        h = hs[c["vol"]]
        h.reset()
        h.set_state(*(a[h.x_index] for a in preload_state(c["vol"])))
        h.stats(reset=True)
        d, col = P.batch_images(c["vol"], n)
        run_frames(h, cfg, c, P.batch_rows(c["vol"], n, at, P.case_rows(c, form)), d, col, at)
        want, total = want_batch(name, form, n, at) if c["vol"] == "4cm" else want_batch_of(name, form, n, at)
        same_state(h.get_state(), want, h.x_index, (name, form, n))
        st = h.stats()
        assert st["list_errors"] == 0
        if cfg["shard"] is None:
            assert st["voxel_updates"] == total, (name, form, st["voxel_updates"], total)
    for h in hs.values():
        h.close()


@functools.lru_cache(maxsize=None)
def want_batch_of(name, form, n, at):
    orc, counts = P.oracle_batch(name, form, n, at)
    return tuple(a.copy() for a in fields(orc)), sum(counts)


def test_dense_drop_in_integrate_takes_the_pose(gf, monkeypatch):
    """TSDFVolume.integrate(cam_pose), synchronous and deferred: the wrapper forms inv(cam_pose) as the
    reference does -- the oracle's state -- and raises numpy's LinAlgError for the zero matrix, as the
    reference did when the fixture was made."""
    set_env(monkeypatch, DENSE["u16-host-texel-pipe"], 8)
    for defer in (False, True):
        for name, c in CASES.items():
            if c["pose"] is None:
                continue
            b, vs = P.VOLUMES[c["vol"]]
            h = gf.TSDFVolume(np.array(b), vs, defer=defer)
            pre = preload_state(c["vol"])
            h.set_state(*pre)
            if name == "zero_all":
                with pytest.raises(np.linalg.LinAlgError):
                    h.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], c["pose"])
                same_state(h.get_state(), pre, slice(None), (name, "raised"))
            else:
                h.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], c["pose"])
                same_state(h.get_state(), want_single(name, "pose")[0], slice(None), (name, defer))
            h.close()


# ---- hash integrate -----------------------------------------------------------------------------------
HASH = {
    "u16-host-pipe": dict(depth="u16", device=False, pipe="1"),
    "u16-device-nopipe": dict(depth="u16", device=True, pipe="0"),
    "f64-host-nopipe": dict(depth="f64", device=False, pipe="0"),
    "f64-device-pipe": dict(depth="f64", device=True, pipe="1"),
}


def blocks_of(weight):
    """The number of 8^3 blocks that hold a voxel with an entry: the pool's live blocks."""
    idx = np.argwhere(weight > 0) // 8
    return len(np.unique(idx, axis=0))


def check_table(ht, want, label):
    """State, entry count and live pool blocks against the oracle's volume (weights 1: the voxels with
    weight > 0 are the reference's keys)."""
    same_state(ht.get_state(), want, slice(None), label)
    info = ht.info()
    assert (info["entries"], info["used"]) == (int((want[1] > 0).sum()), blocks_of(want[1])), (label, info)
    st = ht.stats()
    assert st["list_errors"] == 0 and st["bricks_skipped"] == 0, (label, st)


def hash_frames(ht, cfg, K, rows, depth_mm, rgb):
    d, c, kw, keep = frames_of(cfg, depth_mm, rgb)
    ht.integrate_batch(d, c, K, rows, **kw)
    del keep


@pytest.mark.parametrize("cfg", list(HASH))
def test_hash_single_hostile_frame(hf, monkeypatch, cfg):
    """Every case alone on a fresh table and on a preloaded one: the oracle's state, its keys as the
    entry count, the blocks that hold them as the pool's live blocks.  A no-op frame leaves the fresh
    table without an entry and without a block, and the preloaded one as it was."""
    cfg = HASH[cfg]
    set_env(monkeypatch, cfg, 8)
    tables = {}
    for name, form in CASE_FORMS:
        if (name, form) == ("zero_all", "pose"):
            continue
        c = CASES[name]
        vol = c["vol"]
        if vol not in tables:
            b, vs = P.VOLUMES[vol]
            tables[vol] = hf.HashTable(np.array(b), vs, 1 << 12)
        ht = tables[vol]
        rows = P.case_rows(c, form)[None]
        img = (P.depth_mm(vol, P.PRELOAD)[None], P.rgb(P.PRELOAD)[None])
        # fresh
        ht.reset()
        hash_frames(ht, cfg, c["K"], rows, *img)
        fresh = P.new_oracle(vol)
        with np.errstate(all="ignore"):
            n = fresh.integrate(img[1][0], P.depth_m(vol, P.PRELOAD), c["K"], None, rows=rows[0])
        check_table(ht, fields(fresh), (name, form, "fresh"))
        if c["expect"] == "noop":
            info = ht.info()
            assert n == 0 and (info["entries"], info["used"]) == (0, 0), (name, form, info)
        # preloaded
        ht.reset()
        pre_rows = np.stack([P.good_rows(vol, f) for f in range(P.PRELOAD)])
        hash_frames(ht, cfg, P.K, pre_rows, np.stack([P.depth_mm(vol, f) for f in range(P.PRELOAD)]),
                    np.stack([P.rgb(f) for f in range(P.PRELOAD)]))
        hash_frames(ht, cfg, c["K"], rows, *img)
        check_table(ht, want_single(name, form)[0], (name, form, "preloaded"))
    for ht in tables.values():
        ht.close()


@pytest.mark.parametrize("n,at", P.BATCHES)
@pytest.mark.parametrize("cfg", ["u16-host-pipe", "f64-device-pipe", "u16-device-nopipe"])
def test_hash_hostile_frame_inside_a_batch(hf, monkeypatch, cfg, n, at):
    cfg = HASH[cfg]
    set_env(monkeypatch, cfg, n)
    tables = {}
    for name, form in CASE_FORMS:
        if (name, form) == ("zero_all", "pose"):
            continue
        c = CASES[name]
        vol = c["vol"]
        if vol not in tables:
            b, vs = P.VOLUMES[vol]
            tables[vol] = hf.HashTable(np.array(b), vs, 1 << 12)
        ht = tables[vol]
        ht.reset()
        pre_rows = np.stack([P.good_rows(vol, f) for f in range(P.PRELOAD)])
        hash_frames(ht, cfg, P.K, pre_rows, np.stack([P.depth_mm(vol, f) for f in range(P.PRELOAD)]),
                    np.stack([P.rgb(f) for f in range(P.PRELOAD)]))
        d, col = P.batch_images(vol, n)
        rows = P.batch_rows(vol, n, at, P.case_rows(c, form))
        cuts = [(0, n, P.K)] if c["K"] is P.K else [(0, at, P.K), (at, at + 1, c["K"]), (at + 1, n, P.K)]
        for a, b_, K in cuts:
            hash_frames(ht, cfg, K, rows[a:b_], d[a:b_], col[a:b_])
        want, _ = want_batch(name, form, n, at) if vol == "4cm" else want_batch_of(name, form, n, at)
        check_table(ht, want, (name, form, n))
    for ht in tables.values():
        ht.close()


def test_hash_drop_in_integrate_takes_the_pose(hf, monkeypatch):
    set_env(monkeypatch, HASH["u16-host-pipe"], 8)
    for name, c in CASES.items():
        if c["pose"] is None:
            continue
        b, vs = P.VOLUMES[c["vol"]]
        ht = hf.HashTable(np.array(b), vs, 1 << 12)
        if name == "zero_all":
            with pytest.raises(np.linalg.LinAlgError):
                ht.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], c["pose"])
            ht.sync()
            assert (ht.info()["entries"], ht.info()["used"]) == (0, 0)
        else:
            ht.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], c["pose"])
            ht.sync()
            fresh = P.new_oracle(c["vol"])
            with np.errstate(all="ignore"):
                fresh.integrate(P.rgb(P.PRELOAD), P.depth_m(c["vol"], P.PRELOAD), c["K"], c["pose"])
            check_table(ht, fields(fresh), (name, "drop-in"))
        ht.close()


# ---- frustum bounds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u16", "f64", "device"])
def test_frustum_points_and_bounds_equal_the_reference(gf, gold, kind):
    """Every case that has a pose, in the fixture's order (the cases whose own bounds hold no NaN first):
    get_view_frustum's points, the demo's bounds of each frame alone and its running union -- in one
    call and frame by frame from the running bounds -- bit for bit, NaN where the reference's
    np.minimum / np.amin leave a NaN."""
    from tsdf_amd import _ffi
    order = list(gold["frustum_order"])
    for K_id in sorted({id(CASES[n]["K"]) for n in order}):  # (a call takes one K)
        names = [n for n in order if id(CASES[n]["K"]) == K_id]
        for vol in P.VOLUMES:
            sel = [n for n in names if CASES[n]["vol"] == vol]
            if not sel:
                continue
            K = CASES[sel[0]]["K"]
            poses = np.stack([CASES[n]["pose"] for n in sel])
            mm = np.stack([P.depth_mm(vol, P.PRELOAD)] * len(sel))
            kw, keep = {}, None
            frames = mm if kind == "u16" else mm.astype(np.float64) / 1000.0
            if kind == "device":
                import torch
                keep = torch.from_numpy(frames).cuda()
                torch.cuda.synchronize()
                frames, kw = keep.data_ptr(), dict(device_ptrs=True, hw=P.HW, depth_kind=_ffi.DEPTH_F64_M, n_frames=len(sel))
            b, md, pts = gf.view_frustum_bounds(frames, K, poses, return_max_depth=True, return_points=True, **kw)
            assert (md == float(P.depth_m(vol, P.PRELOAD).max())).all()
            want = np.zeros((3, 2))
            with np.errstate(all="ignore"):
                for k, n in enumerate(sel):
                    assert same_or_nan(pts[k], gold[n + "/pose/frustum"]), (n, pts[k], gold[n + "/pose/frustum"])
                    one = gold[n + "/pose/frustum_bounds"]
                    want[:, 0], want[:, 1] = np.minimum(want[:, 0], one[:, 0]), np.maximum(want[:, 1], one[:, 1])
                    if kind != "device":
                        alone = gf.view_frustum_bounds(frames[k:k + 1], K, poses[k:k + 1])
                        assert same_or_nan(alone, one), (n, alone, one)
            assert same_or_nan(b, want), (sel, b, want)
            del keep
    # the running union over all cases, frame by frame from the bounds so far
    run = np.zeros((3, 2))
    for k, n in enumerate(order):
        c = CASES[n]
        mm = P.depth_mm(c["vol"], P.PRELOAD)[None]
        run = gf.view_frustum_bounds(mm if kind == "u16" else mm.astype(np.float64) / 1000.0, c["K"], c["pose"][None], init=run)
        assert same_or_nan(run, gold["frustum_running"][k]), (n, run, gold["frustum_running"][k])


# ---- raycast ------------------------------------------------------------------------------------------
HANDLES = ("ragged", "ragged_hash")


@pytest.fixture(scope="module")
def handles(gf, hf):
    made = {}

    def get(name):
        if name not in made:
            made[name] = make(gf, hf, name)
        return made[name]

    return get


def raycast_cases():
    base = E.corner_poses()["front"]
    out = [("pose:" + n, I.MODEL_K, p) for n, p in P.scene_poses(np.asarray(base, dtype=np.float64), I.ORIGIN, I.VS).items()]
    out += [("K:" + n, k, np.asarray(base, dtype=np.float64)) for n, k in P.scene_intrinsics(I.MODEL_K).items()]
    return out


def test_raycast_from_hostile_poses_and_intrinsics(handles):
    """Every pose and intrinsics case on the corner scene, dense and hash: the depth and colour maps equal
    raycast_ref bit for bit, a second call returns the same bytes, no NaN leaves the kernel, and a pose
    or K that holds a NaN sees nothing.  The normal map cannot be restated to the bit: the kernel's
    length is __fsqrt_rn, which compiles to the hardware square root, accurate to one ulp but not
    correctly rounded, where NumPy's is; measured on the axis-aligned "centre" case, 29 of the hit rays
    have a length one ulp below the correctly rounded one and so 83 components one ulp (1.2e-7) off, and
    every one of them equals gradient / nextafter(length, 0).  So the normals are held to what is exact
    -- the same rays have a normal, the same components are zero, none is NaN -- and to the suite's own
    1e-6 (test_raycast_gpu.same, raycast_ref's docstring); the table against the dense handle is byte for
    byte in the next test."""
    hits = {}
    for label, K, pose in raycast_cases():
        for name in HANDLES:
            obj = handles(name)
            (t, w, c), off = E.state(name)
            g = obj.raycast(K, pose, I.MODEL_HW, z_far=I.Z_FAR)
            g2 = obj.raycast(K, pose, I.MODEL_HW, z_far=I.Z_FAR)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g, g2)), (label, name)
            with np.errstate(all="ignore"):
                ref = R.raycast(t, w, c, I.ORIGIN, I.VS, K, pose, I.MODEL_HW, 0.0, I.Z_FAR, I.VS, index_offset=off)
            assert not np.isnan(g[0]).any() and not np.isnan(g[1]).any(), (label, name)
            assert np.array_equal(bits(g[0]), bits(ref[0])) and np.array_equal(g[2], ref[2]), (label, name)
            assert np.array_equal(g[1] == 0, ref[1] == 0) and np.array_equal(np.signbit(g[1]), np.signbit(ref[1])), (label, name)
            same_maps(g, ref)
            if name == "ragged":
                hits[label] = int((g[0] != 0).sum())
        if np.isnan(pose[:3]).any() or np.isnan(np.asarray(K)[:2]).any():
            assert hits[label] == 0, label
    print(hits)
    assert sum(v > 250 for v in hits.values()) >= 8  # the non-rigid and negative-focal cases see the scene


def test_raycast_of_the_table_equals_the_holed_dense_volume(gf, hf, handles):
    """dense == hash: the table against the dense handle that has weight 0 in the table's absent blocks,
    byte for byte, on every case."""
    holed = make(gf, hf, "ragged_holed")
    for label, K, pose in raycast_cases():
        a = handles("ragged_hash").raycast(K, pose, I.MODEL_HW, z_far=I.Z_FAR)
        b = holed.raycast(K, pose, I.MODEL_HW, z_far=I.Z_FAR)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), label
    holed.close()


# ---- track --------------------------------------------------------------------------------------------
def track_cases():
    from test_track_cpu import corner_starts
    g = corner_starts()[0]
    out = [("pose:" + n, I.FRAME_K, p) for n, p in P.scene_poses(g, I.ORIGIN, I.VS).items()]
    out += [("K:" + n, k, g) for n, k in P.scene_intrinsics(I.FRAME_K).items()]
    return out


def chain(info, linearize_at, label):
    """The restatement chain without conditions on the system: for each relative pose M_i the device
    produced, the restatement's linearisation at M_i and icp_ref.step give M_{i+1} within STEP_TOL, the
    same status, iteration and inlier counts."""
    traj = info["trajectory"]
    assert len(traj) == info["iterations"] + 1 and np.array_equal(traj[0], np.eye(4)), label
    status, lin, worst = None, None, 0.0
    for i in range(info["iterations"]):
        assert status is None, label
        with np.errstate(all="ignore"):
            lin = linearize_at(traj[i])
        M2, status, _, _ = I.step(traj[i], lin["sums"], lin["inliers"])
        worst = max(worst, float(np.abs(M2 - traj[i + 1]).max()))
    print(label, info["status"], info["iterations"], info["inliers"], "max step error %.3g" % worst)
    assert worst <= STEP_TOL, (label, worst)
    assert info["status"] == (status or I.MAX_ITER), (label, info["status"], status)
    assert (info["inliers"], info["candidates"]) == (lin["inliers"], lin["candidates"]), label


def track_one(obj, method, frame, rgb, K, g):
    if method == "sdf":
        return obj.track(frame, K, g, method="sdf", return_info=True)
    kw = {} if method == "icp" else dict(color_im=rgb, color_weight=E.EDGE_COLOR_WEIGHT)
    return obj.track(frame, K, g, z_far=I.Z_FAR, return_info=True, **kw)


@pytest.mark.parametrize("method", ["icp", "rgbd", "sdf"])
def test_track_with_hostile_guesses_and_intrinsics(gf, hf, handles, tr, method):
    """Every pose case as the guess and every intrinsics case as K.  A guess whose rotation is no rotation
    (scaled, sheared, mirrored, zero, NaN: hostile_pose.guess_is_rigid) is refused with TSDF_E_ARG by
    every handle.  For the rest: the trajectory of the dense handle and of the table follows the
    restatement on the handle's own state within STEP_TOL with its status and counts; the table and the
    dense handle that has weight 0 in the table's absent blocks agree in status, iterations and inliers
    and in the trajectory within STEP_TOL; the returned pose is guess @ M_last, NaN exactly where that
    product is, and finite unless the track is lost."""
    from tsdf_amd import _ffi
    frame = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    rgb = C.plane_render(K=I.FRAME_K, hw=I.FRAME_HW)[1] if method == "rgbd" else None
    holed = make(gf, hf, "ragged_holed")
    refused = 0
    for label, K, g in track_cases():
        objs = {"ragged": handles("ragged"), "ragged_hash": handles("ragged_hash"), "ragged_holed": holed}
        if not P.guess_is_rigid(g):
            for name, obj in objs.items():
                with pytest.raises(_ffi.TSDFError) as e:
                    track_one(obj, method, frame, rgb, K, g)
                assert e.value.code == _ffi.E_ARG and "pose_guess" in str(e.value), (label, name, str(e.value))
            refused += 1
            continue
        infos = {}
        for name, obj in objs.items():
            pose, info = track_one(obj, method, frame, rgb, K, g)
            infos[name] = info
            with np.errstate(all="ignore"):
                want = np.asarray(g, dtype=np.float64) @ info["trajectory"][-1]
            assert np.array_equal(np.isnan(pose), np.isnan(want)), (label, name)
            assert same_or_nan(pose, want) or np.nanmax(np.abs(pose - want)) <= 1e-12, (label, name)
            if info["status"] != "lost":
                assert np.isfinite(pose).all(), (label, name, info["status"])
            if name == "ragged_holed":
                continue
            (t, w, _), off = E.state(name)
            if method == "sdf":
                chain(info, lambda M: S.linearize(frame, K, M, g, t, w, index_offset=off, **S.CORNER_VOL), (label, name, method))
            else:
                d, n, c = obj.raycast(K, g, frame.shape, z_far=I.Z_FAR)
                if method == "icp":
                    chain(info, lambda M: I.linearize(frame, K, M, d, n, K, g), (label, name, method))
                else:
                    def lin_rgbd(M):
                        geo = I.linearize(frame, K, M, d, n, K, g)
                        col = C.linearize_color(frame, rgb, K, M, d, c, K)
                        return dict(geo, sums=C.combine(geo["sums"], col["sums"], E.EDGE_COLOR_WEIGHT))
                    chain(info, lin_rgbd, (label, name, method))
        a, b = infos["ragged_hash"], infos["ragged_holed"]
        assert (a["status"], a["iterations"], a["inliers"], a["candidates"]) == (b["status"], b["iterations"], b["inliers"], b["candidates"]), label
        assert np.abs(a["trajectory"] - b["trajectory"]).max() <= STEP_TOL, label
    holed.close()
    assert refused == 8  # nan_all, zero_row3, zero_all, three scales, the shear, the mirror


@pytest.mark.parametrize("fn", ["tsdf_dense_track", "tsdf_hash_track", "tsdf_dense_track_sdf", "tsdf_hash_track_sdf"])
def test_a_refused_guess_writes_to_no_output(handles, tr, fn):
    """The C-ABI with a mirrored guess: TSDF_E_ARG, and out_pose, info and the trajectory keep their bytes."""
    from tsdf_amd import _ffi
    from test_track_cpu import corner_starts
    obj = handles("ragged_hash" if "hash" in fn else "ragged")
    g = P.scene_poses(corner_starts()[0], I.ORIGIN, I.VS)["mirror"]
    frame = np.ascontiguousarray(I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW))
    H, W = frame.shape
    out, traj = np.full(16, 7.25), np.full((11, 4, 4), 7.25)
    info = _ffi.TrackInfo()
    ctypes.memset(ctypes.byref(info), 0x5A, ctypes.sizeof(info))
    before = bytes(info)
    prm = tr.icp_params()
    args = [obj._h, _ffi.ptr(frame), _ffi.DEPTH_U16_MM, H, W, _ffi.ptr(_ffi.f64(I.FRAME_K, 9)), _ffi.ptr(_ffi.f64(g, 16)), ctypes.byref(prm)]
    if not fn.endswith("_sdf"):
        args += [0.0, float(I.Z_FAR), float(I.VS)]
    with pytest.raises(_ffi.TSDFError) as e:
        _ffi.call(fn, *args, _ffi.ptr(out), ctypes.byref(info), _ffi.ptr(traj), 0)
    assert e.value.code == _ffi.E_ARG
    assert (out == 7.25).all() and (traj == 7.25).all() and bytes(info) == before


def test_linearizations_with_hostile_poses_and_intrinsics(handles, tr):
    """icp_linearize, icp_linearize_rgbd and sdf_linearize with every pose case as the relative pose (and,
    for the SDF, as the guess) and every intrinsics case as the frame's K: codes and residuals byte for
    byte, counts equal.  The sums cannot be equal to the bit: the restatement's are the exact sums
    (math.fsum of exact products), the device adds the same products in the order its launch shape fixes,
    so each is held to the suite's order-of-addition bound, inliers * 2^-52 * sum|term|, which is exactly 0
    -- sums equal to the bit -- wherever a case leaves no inlier; the sums are finite everywhere."""
    frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    rgb = C.plane_render(K=I.FRAME_K, hw=I.FRAME_HW)[1]
    obj = handles("ragged")
    d, n, c = obj.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    poses = P.scene_poses(I.offset_2cm_1deg(), I.ORIGIN, I.VS)
    runs = [("pose:" + k, I.FRAME_K, p) for k, p in poses.items()] + [("K:" + k, v, I.offset_2cm_1deg()) for k, v in P.scene_intrinsics(I.FRAME_K).items()]
    for label, K, M in runs:
        with np.errstate(all="ignore"):
            geo = I.linearize(frame, K, M, d, n, I.MODEL_K, np.eye(4))
            col = C.linearize_color(frame, rgb, K, M, d, c, I.MODEL_K)
        old = tr.icp_linearize(frame, K, M, d, n, I.MODEL_K, np.eye(4))
        got = tr.icp_linearize_rgbd(frame, rgb, K, M, d, n, c, I.MODEL_K, np.eye(4))
        for res in (old, got):
            assert res["code"].tobytes() == geo["code"].tobytes() and res["residual"].tobytes() == geo["resid"].tobytes(), label
            assert (res["inliers"], res["candidates"]) == (geo["inliers"], geo["candidates"]), label
            err = np.abs(res["sums"] - geo["sums"])
            assert np.isfinite(res["sums"]).all() and (err <= geo["inliers"] * 2.0 ** -52 * geo["abs_sums"]).all(), label
        assert got["color_code"].tobytes() == col["code"].tobytes() and got["color_residual"].tobytes() == col["resid"].tobytes(), label
        assert (got["color_inliers"], got["color_candidates"]) == (col["inliers"], col["candidates"]), label
        err = np.abs(got["color_sums"] - col["sums"])
        assert np.isfinite(got["color_sums"]).all() and (err <= col["inliers"] * 2.0 ** -52 * col["abs_sums"]).all(), label
        for name in HANDLES:
            (t, w, _), off = E.state(name)
            for Mi, G in ((M, np.eye(4)), (np.eye(4), M)):
                with np.errstate(all="ignore"):
                    ref = S.linearize(frame, K, Mi, G, t, w, index_offset=off, **S.CORNER_VOL)
                check_linearize(tr.sdf_linearize(handles(name), frame, K, Mi, G), ref, f"{label} {name}")


# ---- sample -------------------------------------------------------------------------------------------
def check_sample(got, pts, names, t, w, off, label):
    with np.errstate(all="ignore"):
        want = S.sample(pts, t, w, **S.CORNER_VOL, index_offset=off)
    for a, b, what in zip(got, want, ("sdf", "grad", "code")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (label, what)
    sdf, grad, code = got
    hostile = np.array([n != "neighbour" for n in names])
    assert (code[hostile] == 2).all() and (code[~hostile] >= 3).all() and (code[~hostile] >= 4).sum() >= 10, label
    low = code < 4
    assert not sdf[low].any() and not grad[low].any() and sdf.tobytes().count(b"\x00") >= 4 * int(low.sum())
    assert (bits(sdf[low]) == 0).all() and (bits(np.ascontiguousarray(grad[low])) == 0).all(), label  # exactly +0.0


@pytest.mark.parametrize("name", ["ragged", "ragged_hash", "slab"])
def test_sample_at_hostile_points(handles, name):
    """NaN, +-inf, +-1e300, +-3e9 and +-1e9 (in voxels) in one coordinate: code 2 and exact zeros, bit-equal
    to sdf_ref; the finite neighbour beside each keeps its value."""
    (t, w, _), off = E.state(name)
    names, pts = P.sample_points(I.ORIGIN, I.VS, t.shape, off)
    check_sample(handles(name).sample(pts), pts, names, t, w, off, name)


@pytest.mark.parametrize("which", ["largest", "smallest"])
def test_sample_with_the_extreme_index_offsets(tr, which):
    """A 40 x 24 x 20 handle created through the C-ABI with the largest index_offset tsdf_dense_create
    accepts on every axis (dims + offset == 2^24) and with the smallest (0): floor_i's clamp to +-1e9
    minus the offset stays inside an int, and sdf_cell answers 2."""
    from tsdf_amd import _ffi
    dims = np.array(P.DIMS, np.int64)
    off = (P.MAX_OFFSET - dims) if which == "largest" else np.zeros(3, np.int64)
    t, w, c = (np.ascontiguousarray(a[:dims[0], :dims[1], :dims[2]]) for a in I.corner_state())
    h = ctypes.c_void_p()
    origin = np.ascontiguousarray(I.ORIGIN, dtype=np.float32)
    _ffi.call("tsdf_dense_create", _ffi.ptr(dims), _ffi.ptr(np.ascontiguousarray(off)), _ffi.ptr(origin), float(I.VS), float(5 * I.VS), 0,
              ctypes.byref(h))
    try:
        with pytest.raises(_ffi.TSDFError):  # one more voxel of offset is refused
            h2 = ctypes.c_void_p()
            _ffi.call("tsdf_dense_create", _ffi.ptr(dims), _ffi.ptr(np.ascontiguousarray(P.MAX_OFFSET - dims + 1)), _ffi.ptr(origin),
                      float(I.VS), float(5 * I.VS), 0, ctypes.byref(h2))
        _ffi.call("tsdf_dense_set", h, _ffi.ptr(t), _ffi.ptr(w), _ffi.ptr(c))
        names, pts = P.sample_points(I.ORIGIN, I.VS, tuple(dims), tuple(int(x) for x in off))
        got = tr.sample_call("tsdf_dense_sample", h, 0, pts)
        check_sample(got, pts, names, t, w, tuple(int(x) for x in off), which)
    finally:
        _ffi.call("tsdf_dense_destroy", h)
