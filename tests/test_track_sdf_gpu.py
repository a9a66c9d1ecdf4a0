"""The device's point-to-SDF alignment (tsdf_*_track_sdf, tsdf_*_sdf_linearize, tsdf_*_sample, DESIGN.md
§7g) against its NumPy restatement (tests/sdf_ref.py): codes and residuals byte-identical, sums
within what the order of addition can change, every pose update reproduced step by step, and the
final poses within the bounds tests/test_track_sdf_cpu.py measured for the method.  Volumes <= 128^3,
images <= 83 x 61."""
import ctypes

import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_ref as I
import sdf_ref as S
from test_track_cpu import C1, corner_starts, lounge_case
from test_track_sdf_cpu import CORNER_SDF_MEASURED, LOUNGE_SDF_MEASURED, sample_points

pytestmark = pytest.mark.gpu
STEP_TOL = 1e-9  # cond(A) ~ 1.5e2 with ~3e3 terms: the f64 solve's forward error is ~1e-10


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
def corner(gf):
    vol = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    assert tuple(vol._vol_dim) == I.SHAPE and np.array_equal(vol._vol_origin, I.ORIGIN)
    vol.set_state(*I.corner_state())
    return vol


@pytest.fixture(scope="module")
def corner_tw():
    t, w, _ = I.corner_state()
    return t, w


@pytest.fixture(scope="module")
def code_refs(corner_tw):
    """The restatement's linearisations of the every-code inputs, computed once: stride -> dict."""
    frame, K, M, G = S.every_code_case()
    return {s: S.linearize(frame, K, M, G, *corner_tw, stride=s, **S.CORNER_VOL, **S.EVERY_CODE) for s in (1, 3)}


def volume_of(obj):
    return dict(origin=obj._vol_origin, voxel_size=obj._voxel_size, trunc=obj._trunc_margin)


def check_linearize(got, ref, label):
    """Maps byte-identical, counts equal, every sum within N 2^-52 sum|term| of the exact sum (the
    terms are exact products; only the order of the N - 1 additions differs)."""
    assert got["code"].tobytes() == ref["code"].tobytes()
    assert got["residual"].tobytes() == ref["resid"].tobytes()
    assert (got["inliers"], got["candidates"]) == (ref["inliers"], ref["candidates"])
    bound = ref["inliers"] * 2.0 ** -52 * ref["abs_sums"]
    err = np.abs(got["sums"] - ref["sums"])
    print(f"{label}: inliers {got['inliers']}, candidates {got['candidates']}, max |sum - fsum| / bound "
          f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got["A"], got["A"].T) and np.array_equal(got["b"], got["sums"][21:27])


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["u16", "f64"])
def test_sdf_linearize_equals_the_restatement(corner, tr, code_refs, kind, stride):
    frame, K, M, G = S.every_code_case()
    ref = code_refs[stride]
    counts = np.bincount(ref["code"].ravel(), minlength=7)
    assert np.delete(counts, 1).min() >= (20 if stride == 1 else 1), counts  # the reference shows every code
    got = tr.sdf_linearize(corner, frame if kind == "u16" else frame.astype(np.float64) / 1000.0, K, M, G, stride=stride,
                           **S.EVERY_CODE)
    check_linearize(got, ref, f"{kind} stride {stride}")


def test_invalid_65535_and_null_maps(corner, tr, corner_tw):
    frame, K, M, G = S.every_code_case()
    f2 = frame.copy()
    f2[20:30, 10:20] = 65535
    ref = S.linearize(f2, K, M, G, *corner_tw, invalid_65535=True, **S.CORNER_VOL, **S.EVERY_CODE)
    got = tr.sdf_linearize(corner, f2, K, M, G, invalid_65535=True, **S.EVERY_CODE)
    assert got["code"].tobytes() == ref["code"].tobytes() and (got["code"][20:30, 10:20] == 0).all()
    kept = tr.sdf_linearize(corner, f2, K, M, G, **S.EVERY_CODE)  # 65.535 m is a depth like any other without the flag
    assert kept["code"][25, 15] != 0
    bare = tr.sdf_linearize(corner, frame, K, M, G, codes=False, residuals=False, **S.EVERY_CODE)
    assert bare["code"] is None and bare["residual"] is None
    assert bare["sums"].tobytes() == tr.sdf_linearize(corner, frame, K, M, G, **S.EVERY_CODE)["sums"].tobytes()


@pytest.fixture(scope="module")
def lounge_frames():
    return [load_lounge(i) for i in range(3)]


def fused(gf, hf, kind, frames):
    obj = gf.TSDFVolume(np.array(C1), 0.04) if kind == "dense" else hf.HashTable(np.array(C1), 0.04, 1 << 16)
    for _, depth, rgb, pose in frames:
        obj.integrate(rgb, depth, lounge_intrinsics(), pose)  # (deferred: the next call on the handle runs them)
    return obj


def entry_mask(ht):
    """(X, Y, Z) bool: the voxels with an entry, from the table's exported entry words."""
    bxyz, _, _, _, occ = ht.export_blocks()
    m = np.zeros(tuple(int(x) for x in ht._vol_dim), bool)
    bits = ((occ[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)  # [block, z, x*8 + y]
    for b, (bx, by, bz) in enumerate(bxyz):
        blk = bits[b].reshape(8, 8, 8).transpose(1, 2, 0)  # [x, y, z]
        x0, y0, z0 = 8 * int(bx), 8 * int(by), 8 * int(bz)
        sub = m[x0:x0 + 8, y0:y0 + 8, z0:z0 + 8]
        sub[...] = blk[:sub.shape[0], :sub.shape[1], :sub.shape[2]]
    return m


@pytest.mark.parametrize("stride", [1, 3])
def test_sdf_linearize_on_a_hash_after_deferred_integrates(hf, gf, tr, lounge_frames, stride):
    """Three deferred integrate() calls, then one linearisation (it runs the pending frames),
    restated from the handle's own get_state().  Conditions on the inputs: at least 20 pixels with a
    code >= 3 whose cell straddles a block boundary, and at least 20 with code 3 through a voxel
    without an entry."""
    ht = fused(gf, hf, "hash", lounge_frames)
    frame, K, _, starts = lounge_case()
    got = tr.sdf_linearize(ht, frame, K, np.eye(4), starts[0], stride=stride)
    t, w, _ = ht.get_state()
    ref = S.linearize(frame, K, np.eye(4), starts[0], t, w, stride=stride, **volume_of(ht))
    check_linearize(got, ref, f"hash stride {stride}")
    if stride == 1:
        assert ref["inliers"] > 2000
        code, i0 = ref["code"], ref["cell"]
        straddle = (code >= 3) & ((i0 & 7) == 7).any(axis=-1)
        has = entry_mask(ht)
        assert not (w[~has] > 0).any()
        c3 = np.argwhere(code == 3)
        cells = i0[c3[:, 0], c3[:, 1]]
        no_entry = np.zeros(len(cells), bool)
        for s in range(8):
            no_entry |= ~has[cells[:, 0] + (s >> 2), cells[:, 1] + ((s >> 1) & 1), cells[:, 2] + (s & 1)]
        print(f"straddling cells {int(straddle.sum())}, code 3 through a voxel without an entry {int(no_entry.sum())}")
        assert straddle.sum() >= 20 and no_entry.sum() >= 20


def follow(obj, tr, frame, K, g, info, tw, device_counts=True, index_offset=(0, 0, 0), max_iter=10, **prm):
    """The restatement chain: for each relative pose M_i the device produced, sdf_ref.linearize(M_i)
    and icp_ref.step reproduce M_{i+1} within STEP_TOL, with the same counts (the device's own
    linearisation at M_i), status, iteration count, rms and norms.  tw is the handle's own extent
    (a slab's starts at index_offset); max_iter is the call's."""
    traj = info["trajectory"]
    assert len(traj) == info["iterations"] + 1 and np.array_equal(traj[0], np.eye(4))
    status = None
    for i in range(info["iterations"]):
        assert status is None
        lin = S.linearize(frame, K, traj[i], g, *tw, index_offset=index_offset, **volume_of(obj), **prm)
        if device_counts:
            got = tr.sdf_linearize(obj, frame, K, traj[i], g, codes=False, residuals=False, **prm)
            assert (got["inliers"], got["candidates"]) == (lin["inliers"], lin["candidates"])
        M2, status, wn, tn = I.step(traj[i], lin["sums"], lin["inliers"])
        err = np.abs(M2 - traj[i + 1]).max()
        assert err <= STEP_TOL, (i, err)
    if status is None:
        status = I.MAX_ITER
        assert info["iterations"] == max_iter
    assert info["status"] == status
    assert info["inliers"] == lin["inliers"] and info["candidates"] == lin["candidates"]
    assert abs(info["rms"] - np.sqrt(lin["sums"][27] / lin["inliers"])) <= 1e-12
    assert abs(info["w_norm"] - wn) <= 1e-9 and abs(info["t_norm"] - tn) <= 1e-9


def test_corner_track_follows_the_restatement_and_reaches_its_accuracy(corner, tr, corner_tw):
    frame = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    for g, (mt, ma, *_) in zip(corner_starts(), CORNER_SDF_MEASURED):
        pose, info = corner.track(frame, I.FRAME_K, g, return_info=True, method="sdf")
        follow(corner, tr, frame, I.FRAME_K, g, info, corner_tw)
        assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
        et, ea = I.pose_error(pose, I.TRUE_POSE)
        print(f"corner: {info['status']} after {info['iterations']}, inliers {info['inliers']}, {1e3 * et:.3f} mm / {ea:.4f} deg")
        assert et <= 2 * mt and ea <= 2 * ma


@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_lounge_track_after_deferred_integrates(gf, hf, tr, lounge_frames, kind):
    """Three per-frame integrate() calls (deferred), then track: it must run the pending frames
    itself.  Each handle follows the restatement chain on its own get_state() and ends within the
    CPU test's lounge bound."""
    obj = fused(gf, hf, kind, lounge_frames)
    frame, K, true, starts = lounge_case()
    tw, first = None, True
    for g, (mt, ma, *_) in zip(starts, LOUNGE_SDF_MEASURED):
        pose, info = obj.track(frame, K, g, return_info=True, method="sdf")  # (first: the frames are still pending)
        if tw is None:
            tw = obj.get_state()[:2]
            assert (tw[1] > 0).sum() > 10000
        follow(obj, tr, frame, K, g, info, tw, device_counts=first)
        first = False
        assert np.abs(pose - g @ info["trajectory"][-1]).max() <= 1e-12
        et, ea = I.pose_error(pose, true)
        print(f"lounge {kind}: {info['status']} after {info['iterations']}, inliers {info['inliers']}, "
              f"{1e3 * et:.3f} mm / {ea:.4f} deg")
        assert info["status"] != "lost" and info["inliers"] >= 1000
        assert et <= 2 * mt and ea <= 2 * ma


def test_two_calls_give_identical_bytes(corner, tr):
    frame, K, M, G = S.every_code_case()
    a, b = (tr.sdf_linearize(corner, frame, K, M, G, **S.EVERY_CODE) for _ in range(2))
    assert a["sums"].tobytes() == b["sums"].tobytes() and a["residual"].tobytes() == b["residual"].tobytes()
    seen = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    g = corner_starts()[0]
    (p1, i1), (p2, i2) = (corner.track(seen, I.FRAME_K, g, return_info=True, method="sdf") for _ in range(2))
    assert i1["iterations"] >= 3
    assert p1.tobytes() == p2.tobytes() and i1["trajectory"].tobytes() == i2["trajectory"].tobytes()
    s3, s3b = (corner.track(seen, I.FRAME_K, g, return_info=True, method="sdf", stride=3) for _ in range(2))
    assert s3[0].tobytes() == s3b[0].tobytes() and s3[1]["status"] != "lost" and s3[1]["inliers"] < i1["inliers"] / 4


def last_ms():
    from tsdf_amd import _ffi
    ms, it = (ctypes.c_double * 5)(), ctypes.c_int()
    _ffi.call("tsdf_track_last_ms", ms, ctypes.byref(it))
    return list(ms), it.value


def test_device_tensors_and_the_fast_path(gf, tr, lounge_frames):
    """Device tensors give the bytes host arrays give.  With profiling on an SDF track reports no
    raycast time, and leaves the raycast's live bits alone: a raycast after it spends on its live-bit
    pass what a raycast with current bits spends, not what recomputing them (TSDF_RAY_REFLAG) costs
    (medians of 5; the pass reads the 128^3 volume, an empty event pair reads nothing)."""
    import torch
    from tsdf_amd import _ffi
    dev = torch.device("cuda", 0)
    obj = fused(gf, None, "dense", lounge_frames)
    frame, K, _, starts = lounge_case()
    g = starts[1]
    mm = np.rint(frame * 1000.0).astype(np.uint16)
    for f, t in ((mm, torch.from_numpy(mm.view(np.int16)).to(dev)), (frame, torch.from_numpy(frame).to(dev))):
        host = tr.sdf_linearize(obj, f, K, np.eye(4), g)
        got = tr.sdf_linearize(obj, t, K, np.eye(4), g)
        assert got["sums"].tobytes() == host["sums"].tobytes() and got["inliers"] == host["inliers"] > 2000
        assert np.array_equal(got["code"].cpu().numpy(), host["code"])
        assert got["residual"].cpu().numpy().tobytes() == host["residual"].tobytes()
        p_host, i_host = obj.track(f, K, g, return_info=True, method="sdf")
        p_dev, i_dev = obj.track(t, K, g, return_info=True, method="sdf")
        assert p_host.tobytes() == p_dev.tobytes() and i_host["trajectory"].tobytes() == i_dev["trajectory"].tobytes()
    obj.set_profiling(True)

    def live_ms(flags):
        d = np.empty(frame.shape, np.float32)
        _ffi.call("tsdf_dense_raycast", obj._h, frame.shape[0], frame.shape[1], _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(g, 16)),
                  0.0, 6.0, 0.04, _ffi.ptr(d), None, None, flags)
        a, b = ctypes.c_double(), ctypes.c_double()
        _ffi.call("tsdf_raycast_last_ms", ctypes.byref(a), ctypes.byref(b))
        assert (d > 0).sum() > 2000
        return a.value

    live_ms(0)  # the bits are current from here on
    current, after, reflag = [], [], []
    for _ in range(5):
        current.append(live_ms(0))
        _, info = obj.track(frame, K, g, return_info=True, method="sdf")
        ms, it = last_ms()
        assert ms[0] == 0.0 and it == info["iterations"] >= 3 and ms[2] > 0.0 and ms[3] > 0.0
        after.append(live_ms(0))
        reflag.append(live_ms(_ffi.RAY_REFLAG))
    _, info = obj.track(frame, K, g, return_info=True)  # the ICP still reports its raycast
    assert last_ms()[0][0] > 0.0
    print(f"live-bit pass, ms: current bits {np.median(current):.4f}, after an SDF track {np.median(after):.4f}, "
          f"recomputed {np.median(reflag):.4f}")
    assert np.median(after) < 0.5 * (np.median(current) + np.median(reflag))  # nearer to current bits than to recomputed ones


@pytest.fixture(scope="module")
def holed(gf, hf):
    """The corner state with whole 8^3 blocks never observed, in a dense handle and in a hash built by
    import_blocks from the blocks that are left."""
    t, w, c = I.corner_state()
    nb = [(s + 7) // 8 for s in I.SHAPE]
    drop = np.random.default_rng(9).random(nb) < 0.25
    w = w * ~np.repeat(np.repeat(np.repeat(drop, 8, 0), 8, 1), 8, 2)[:I.SHAPE[0], :I.SHAPE[1], :I.SHAPE[2]]
    dense = gf.TSDFVolume(I.BOUNDS.copy(), I.VS)
    dense.set_state(t, w, c)
    ht = hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12)
    assert tuple(ht._vol_dim) == I.SHAPE and np.array_equal(ht._vol_origin, I.ORIGIN)
    keep = np.argwhere(~drop).astype(np.int32)
    blocks = [np.stack([a[8 * x:8 * x + 8, 8 * y:8 * y + 8, 8 * z:8 * z + 8].reshape(512) for x, y, z in keep]) for a in (t, w, c)]
    ht.import_blocks(keep, *blocks)
    return dense, ht, (t, w)


def test_sample_equals_the_restatement_and_the_hash_the_dense_handle(corner, corner_tw, holed):
    P = sample_points(np.random.default_rng(2))
    want = S.sample(P, *corner_tw, **S.CORNER_VOL)
    counts = np.bincount(want[2], minlength=7)
    assert set(np.flatnonzero(counts)) == {2, 3, 4, 6} and counts[[2, 3, 4, 6]].min() >= 20
    got = corner.sample(P)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    dense, ht, tw = holed
    d, h, ref = dense.sample(P), ht.sample(P), S.sample(P, *tw, **S.CORNER_VOL)
    for a, b in zip(d, ref):
        assert a.tobytes() == b.tobytes()
    sel = d[2] != 3
    assert sel.sum() > 1000 and (d[2] == 3).sum() > 500
    for a, b in zip(h, d):
        assert np.array_equal(a[sel], b[sel])
    assert np.array_equal(h[2], d[2])  # (a voxel without an entry has weight 0: the same code 3)
    import torch
    t = ht.sample(torch.from_numpy(P).to("cuda:0"))
    for a, b in zip(t, h):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    from tsdf_amd import _ffi
    only = np.zeros(len(P), np.uint8)
    _ffi.call("tsdf_dense_sample", corner._h, _ffi.ptr(P), len(P), None, None, _ffi.ptr(only), 0)  # any output may be NULL
    assert np.array_equal(only, want[2])
    assert all(len(x) == 0 for x in corner.sample(np.zeros((0, 3))))


def test_hash_linearize_and_track_equal_the_dense_handle_across_missing_blocks(tr, holed):
    """The every-code inputs on the holed corner: the hash (blocks left out) gives the dense handle's
    bytes, which are the restatement's; cells straddling block boundaries and voxels without an entry
    both occur among the refused pixels."""
    dense, ht, tw = holed
    frame, K, M, G = S.every_code_case()
    ref = S.linearize(frame, K, M, G, *tw, **S.CORNER_VOL, **S.EVERY_CODE)
    counts = np.bincount(ref["code"].ravel(), minlength=7)
    assert np.delete(counts, 1).min() >= 20, counts
    assert ((ref["code"] >= 3) & ((ref["cell"] & 7) == 7).any(axis=-1)).sum() >= 20
    for obj, label in ((dense, "holed dense"), (ht, "holed hash")):
        check_linearize(tr.sdf_linearize(obj, frame, K, M, G, **S.EVERY_CODE), ref, label)
    seen = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    g = corner_starts()[0]
    (pd, idn), (ph, ih) = (o.track(seen, I.FRAME_K, g, return_info=True, method="sdf") for o in (dense, ht))
    assert idn["status"] != "lost" and idn["inliers"] == ih["inliers"] > 1000
    assert np.abs(idn["trajectory"] - ih["trajectory"]).max() <= STEP_TOL  # (the same terms; the grid is the frame's)


def raw_track(fn, handle, frame, g, *, flags=0, prm=None, dk=0, H=None, W=None, depth=True, K=True, pose=True, out=True):
    from tsdf_amd import _ffi, tracking
    prm = tracking.icp_params() if prm is None else prm
    o, info = np.full(16, np.nan), _ffi.TrackInfo()
    traj = np.zeros((_ffi.ICP_MAX_ITER + 1, 16))
    H, W = frame.shape[0] if H is None else H, frame.shape[1] if W is None else W
    rc = getattr(_ffi.load(), fn)(handle, _ffi.ptr(frame) if depth else None, dk, H, W,
                                  _ffi.ptr(_ffi.f64(I.FRAME_K, 9)) if K else None, _ffi.ptr(_ffi.f64(g, 16)) if pose else None,
                                  ctypes.byref(prm) if prm is not False else None, _ffi.ptr(o) if out else None,
                                  ctypes.byref(info), _ffi.ptr(traj), flags)
    return rc, o.reshape(4, 4), info, _ffi.load().tsdf_last_error().decode()


def test_lost_is_not_an_error(gf, hf):
    seen = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    g = corner_starts()[0]
    for obj, fn in ((gf.TSDFVolume(I.BOUNDS.copy(), I.VS), "tsdf_dense_track_sdf"),
                    (hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12), "tsdf_hash_track_sdf")):  # empty volumes
        rc, pose, info, _ = raw_track(fn, obj._h, seen, g)
        assert rc == 0 and info.status == 3 and info.iterations == 1 and info.inliers == 0 and info.candidates > 1000
        assert np.array_equal(pose, g)
        pose, inf = obj.track(seen, I.FRAME_K, g, return_info=True, method="sdf")
        assert inf["status"] == "lost" and np.array_equal(pose, g) and len(inf["trajectory"]) == 2
        assert np.array_equal(inf["trajectory"][1], np.eye(4))


def test_bad_arguments_are_refused_with_a_message(corner, gf, hf, tr):
    from tsdf_amd import _ffi
    seen = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    g = corner_starts()[0]

    def refused(fn, *a, **kw):
        with pytest.raises(_ffi.TSDFError) as e:
            fn(*a, **kw)
        assert e.value.code == _ffi.E_ARG and len(str(e.value)) > 12
        return str(e.value)

    sdf = dict(method="sdf")
    assert "stride" in refused(corner.track, seen, I.FRAME_K, g, stride=0, **sdf)
    assert "max_iter" in refused(corner.track, seen, I.FRAME_K, g, max_iter=0, **sdf)
    assert "dist_max" in refused(corner.track, seen, I.FRAME_K, g, dist_max=0.0, **sdf)
    assert "dist_max" in refused(tr.sdf_linearize, corner, seen, I.FRAME_K, np.eye(4), g, dist_max=-1.0)
    assert "stride" in refused(tr.sdf_linearize, corner, seen, I.FRAME_K, np.eye(4), g, stride=0)
    with pytest.raises(ValueError, match="color_im"):
        corner.track(seen, I.FRAME_K, g, color_im=np.zeros(seen.shape + (3,), np.uint8), **sdf)
    for obj in (corner, hf.HashTable(I.BOUNDS.copy(), I.VS, 1 << 12)):
        with pytest.raises(ValueError, match="method"):
            obj.track(seen, I.FRAME_K, g, method="gicp")
    with pytest.raises(ValueError):
        corner.sample(np.zeros((4, 2)))
    for kw, word in (({"depth": False}, "depth"), ({"K": False}, "camera"), ({"pose": False}, "camera"),
                     ({"out": False}, "out_pose"), ({"prm": False}, "params"), ({"dk": 7}, "depth_kind"),
                     ({"H": 0}, "image size"), ({"W": 1 << 24}, "image size")):
        rc, _, _, msg = raw_track("tsdf_dense_track_sdf", corner._h, seen, g, **kw)
        assert rc == _ffi.E_ARG and word in msg, (kw, msg)
    lib = _ffi.load()
    assert lib.tsdf_hash_track_sdf(None, None, 0, 1, 1, None, None, None, None, None, None, 0) == _ffi.E_ARG
    assert "handle" in lib.tsdf_last_error().decode()
    assert lib.tsdf_dense_sample(None, None, 0, None, None, None, 0) == _ffi.E_ARG
    assert lib.tsdf_dense_sample(corner._h, None, 5, None, None, None, 0) == _ffi.E_ARG
    assert "points" in lib.tsdf_last_error().decode()
    assert lib.tsdf_dense_sample(corner._h, None, -1, None, None, None, 0) == _ffi.E_ARG
    # the linearise call's pointers and kinds
    prm, K, E = tr.icp_params(), _ffi.ptr(_ffi.f64(I.FRAME_K, 9)), _ffi.ptr(_ffi.f64(np.eye(4), 16))
    sums, counts = np.zeros(28), np.zeros(2, np.int64)
    args = lambda **o: [o.get(k, v) for k, v in dict(  # noqa: E731
        h=corner._h, depth=_ffi.ptr(seen), dk=0, H=53, W=71, K=K, M=E, G=E, prm=ctypes.byref(prm), sums=_ffi.ptr(sums),
        counts=_ffi.ptr(counts), code=None, res=None, flags=0).items()]
    assert lib.tsdf_dense_sdf_linearize(*args()) == 0
    for o, word in (({"H": 0}, "image size"), ({"depth": None}, "depth"), ({"K": None}, "camera"), ({"G": None}, "camera"),
                    ({"M": None}, "camera"), ({"sums": None}, "sums"), ({"counts": None}, "sums"), ({"prm": None}, "params"),
                    ({"dk": 7}, "depth_kind"), ({"h": None}, "handle")):
        assert lib.tsdf_dense_sdf_linearize(*args(**o)) == _ffi.E_ARG and word in lib.tsdf_last_error().decode(), o
    # shards: what the raycast refuses
    shard = gf.TSDFVolume(np.array(C1), 0.04, shard=(0, 2))
    hs = hf.HashTable(np.array(C1), 0.04, 1 << 16, shard=0, n_shards=2)
    for obj in (shard, hs):
        assert "shard" in refused(obj.track, seen, I.FRAME_K, g, **sdf)
        assert "shard" in refused(tr.sdf_linearize, obj, seen, I.FRAME_K, np.eye(4), g)
        assert "shard" in refused(obj.sample, np.zeros((3, 3)))
