"""The device raycast (tsdf_dense_raycast / tsdf_hash_raycast) against its NumPy
restatement (tests/raycast_ref.py) run on get_state(): hit mask, depth and colour bit-identical,
normals within 1e-6 (the mesh test's bound).  Volumes <= 128^3, images 83 x 61 (no multiple of the
8 x 8 tile of a wave)."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import raycast_ref as R

pytestmark = pytest.mark.gpu
C1 = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]
HW = (61, 83)
Z_FAR = 6.0
MIN_HITS = 250  # ~5 % of the 5063 rays: a case whose rays mostly miss would check little


@pytest.fixture(scope="module")
def gf():
    from tsdf_amd import grid_fusion
    return grid_fusion


@pytest.fixture(scope="module")
def hf():
    from tsdf_amd import hash_fusion
    return hash_fusion


@pytest.fixture(scope="module")
def frames():
    return [load_lounge(i) for i in range(3)]


def small_K():
    """The lounge intrinsics for an 83-pixel-wide image."""
    K = lounge_intrinsics().copy()
    K[:2] *= 83.0 / 640.0
    return K


def poses(frames):
    """Fused frame 0's pose; outside the volume looking in (the near plane is outside, rays enter
    through the z = 0 face); behind the surfaces looking back (mostly misses)."""
    p0 = frames[0][3]
    outside = np.eye(4)
    outside[:3, 3] = [0.1, -0.2, -1.0]
    behind = np.diag([-1.0, 1.0, -1.0, 1.0])
    behind[:3, 3] = [0.0, 0.0, 4.9]
    return {"frame0": p0, "outside": outside, "behind": behind}


def make_dense(gf, frames, n=3, **kw):
    vol = gf.TSDFVolume(np.array(C1), 0.04, **kw)
    for _, depth, rgb, pose in frames[:n]:
        vol.integrate(rgb, depth, lounge_intrinsics(), pose)
    return vol


def make_hash(hf, frames, n=3):
    ht = hf.HashTable(np.array(C1), 0.04, 1 << 16)
    for _, depth, rgb, pose in frames[:n]:
        ht.integrate(rgb, depth, lounge_intrinsics(), pose)
    # as test_hash_densifies_on_the_device_like_the_host_export: an entry of weight 0, one with
    # values, a removed entry -- and entries removed out of the fused surface
    ht.add_entries([[1, 2, 3], [100, 126, 124]], tsdf=[0.5, -0.25], weight=[0.0, 3.0], color=[7.0, 65793.0])
    ht.remove_entries([[1, 2, 4]])
    t, w, _ = ht.get_state()
    ht.remove_entries(np.argwhere((w > 0) & (np.abs(t) < 0.5))[::97])
    return ht


def same(got, ref):
    d, n, c = got
    rd, rn, rc = ref
    assert np.array_equal(d != 0, rd != 0)
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(c, rc)
    assert np.abs(n - rn).max() <= 1e-6


def check(obj, K, pose, *, state=None, off=(0, 0, 0), z_far=Z_FAR, z_near=0.0, z_step=None, min_hits=None):
    """Raycast first (it must run the deferred frames itself), then the reference on the state."""
    got = obj.raycast(K, pose, HW, z_near=z_near, z_far=z_far, z_step=z_step)
    st = obj.get_state() if state is None else state
    zs = obj._voxel_size if z_step is None else z_step
    ref = R.raycast(*st, obj._vol_origin, obj._voxel_size, K, pose, HW, z_near, z_far, zs, index_offset=off)
    same(got, ref)
    if min_hits is not None:
        assert (ref[0] != 0).sum() >= min_hits
    return got, ref


@pytest.fixture(scope="module")
def dense(gf, frames):
    return make_dense(gf, frames)


def test_dense_raycast_of_the_lounge_fusion_equals_the_reference(dense, frames):
    K = small_K()
    state = dense.get_state()
    P = poses(frames)
    check(dense, K, P["frame0"], state=state, min_hits=MIN_HITS)
    check(dense, K, P["outside"], state=state, min_hits=MIN_HITS)
    _, ref = check(dense, K, P["behind"], state=state)
    assert (ref[0] != 0).sum() < 0.5 * ref[0].size  # mostly misses
    # axis-aligned: the central ray (pixel 41, 30) has two direction components of exactly 0
    Ka = np.array([[75.0, 0.0, 41.0], [0.0, 75.0, 30.0], [0.0, 0.0, 1.0]])
    pa = np.eye(4)
    pa[:3, 3] = [0.02, 0.02, 0.1]
    qo, qd = R.ray_setup(dense._vol_origin, 0.04, Ka, pa, HW)
    assert np.array_equal(qd[30 * 83 + 41, :2], [0.0, 0.0])
    check(dense, Ka, pa, state=state, min_hits=MIN_HITS)
    # a finer and a coarser march, and a near plane inside the scene
    check(dense, K, P["frame0"], state=state, z_step=0.013, z_near=0.5, z_far=4.0, min_hits=MIN_HITS)
    check(dense, K, P["frame0"], state=state, z_step=0.1, min_hits=MIN_HITS)


def test_default_z_far_and_z_step(dense, frames):
    """z_step defaults to the voxel size, z_far to the largest camera z of the volume's corners."""
    K, pose = small_K(), frames[0][3]
    b = np.asarray(dense._vol_bnds, dtype=np.float64)
    corners = np.array([[b[0, i], b[1, j], b[2, k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    z_far = float((np.linalg.inv(pose) @ corners.T)[2].max())
    got = dense.raycast(K, pose, HW)
    ref = R.raycast(*dense.get_state(), dense._vol_origin, 0.04, K, pose, HW, 0.0, z_far, 0.04)
    same(got, ref)


def test_ragged_set_state_volume_with_holes_and_exact_zeros(gf):
    vol = gf.TSDFVolume(np.array([[0.0, 0.63], [0.0, 0.45], [0.0, 0.37]]), 0.01)
    state = R.ragged_state()
    assert tuple(vol._vol_dim) == state[0].shape
    vol.set_state(*state)
    K = np.array([[101.3, 0.0, 41.2], [0.0, 101.3, 29.7], [0.0, 0.0, 1.0]])
    for pose in R.ragged_poses():
        check(vol, K, pose, state=state, z_far=1.2, min_hits=MIN_HITS)


def test_slab_handle_with_an_index_offset(gf, frames):
    vol = make_dense(gf, frames, slab=(40, 104))
    K = small_K()
    P = poses(frames)
    state = vol.get_state()
    assert state[0].shape == (64, 128, 128)
    check(vol, K, P["frame0"], state=state, off=(40, 0, 0), min_hits=MIN_HITS)
    check(vol, K, P["outside"], state=state, off=(40, 0, 0), min_hits=MIN_HITS)


def test_hash_raycast_equals_the_reference_on_its_densified_state(hf, frames):
    ht = make_hash(hf, frames)
    K = small_K()
    P = poses(frames)
    state = ht.get_state()
    check(ht, K, P["frame0"], state=state, min_hits=MIN_HITS)
    check(ht, K, P["outside"], state=state, min_hits=MIN_HITS)
    check(ht, K, P["behind"], state=state)


def test_flags_follow_the_state(gf, hf, frames):
    """Raycast, integrate through the deferred path, raycast, set_state, raycast, reset, raycast:
    each equals the reference on the state of that moment (the live bits are never stale)."""
    K, pose = small_K(), frames[0][3]
    Kl = lounge_intrinsics()
    vol = make_dense(gf, frames, n=2)
    (d0, _, _), _ = check(vol, K, pose, min_hits=MIN_HITS)
    far = frames[2]
    vol.integrate(far[2], far[1], Kl, far[3])  # deferred: the raycast must run it first
    (d1, _, _), _ = check(vol, K, pose, min_hits=MIN_HITS)
    assert not np.array_equal(d0, d1)
    t, w, c = vol.get_state()
    vol.set_state(np.roll(t, 9, axis=2), np.roll(w, 9, axis=2), np.roll(c, 9, axis=2))
    (d2, _, _), _ = check(vol, K, pose, min_hits=MIN_HITS)
    assert not np.array_equal(d1, d2)
    vol.reset()
    (d3, n3, c3), _ = check(vol, K, pose)
    assert not d3.any() and not n3.any() and not c3.any()
    # the hash: integrate, entries added and removed, reset
    ht = hf.HashTable(np.array(C1), 0.04, 1 << 16)
    ht.integrate(frames[0][2], frames[0][1], Kl, frames[0][3])
    (h0, _, _), _ = check(ht, K, pose, min_hits=MIN_HITS)
    ht.integrate(far[2], far[1], Kl, far[3])
    (h1, _, _), _ = check(ht, K, pose, min_hits=MIN_HITS)
    assert not np.array_equal(h0, h1)
    t, w, _ = ht.get_state()
    ht.remove_entries(np.argwhere((w > 0) & (t < 0))[::3])
    (h2, _, _), _ = check(ht, K, pose)
    assert not np.array_equal(h1, h2)
    ht.reset()
    (h3, _, _), _ = check(ht, K, pose)
    assert not h3.any()


def test_skipping_changes_nothing(gf, hf, frames, dense, monkeypatch):
    """TSDF_RAY_SKIP=0 evaluates every sample: byte-identical outputs, dense and hash."""
    K = small_K()
    P = poses(frames)
    ht = make_hash(hf, frames)
    monkeypatch.setenv("TSDF_RAY_SKIP", "0")
    brute = gf.TSDFVolume(np.array(C1), 0.04)
    brute.set_state(*dense.get_state())
    brute_h = make_hash(hf, frames)
    for name in ("frame0", "outside"):
        for a, b in ((dense, brute), (ht, brute_h)):
            x, y = a.raycast(K, P[name], HW, z_far=Z_FAR), b.raycast(K, P[name], HW, z_far=Z_FAR)
            assert (x[0] != 0).sum() > MIN_HITS
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()


K_FACE = np.array([[75.0, 0.0, 41.2], [0.0, 75.0, 29.7], [0.0, 0.0, 1.0]])


def blocks_of(a):
    """(X, Y, Z) with dims multiples of 8 -> (n_blocks, 512) in brick-local order (x*8 + y)*8 + z."""
    nb = [d // 8 for d in a.shape]
    return np.ascontiguousarray(a.reshape(nb[0], 8, nb[1], 8, nb[2], 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 512))


def high_face_case(name, gf, hf):
    """(handle, state, index offset, poses, z_far): a surface in the outermost bricks of every axis."""
    if name == "ragged":  # 63 x 45 x 37: the last brick of every axis is partly outside the volume
        vol = gf.TSDFVolume(np.array([[0.0, 0.63], [0.0, 0.45], [0.0, 0.37]]), 0.01)
        state = R.ellipsoid_state((63, 45, 37))
        vol.set_state(*state)
        return vol, state, (0, 0, 0), R.high_face_poses([0, 0, 0], [0.63, 0.45, 0.37]), 1.6
    state = R.ellipsoid_state((128, 128, 128))
    lo, hi = np.array(C1)[:, 0], np.array(C1)[:, 1]
    P = R.high_face_poses(lo, hi)
    if name == "dense":
        vol = gf.TSDFVolume(np.array(C1), 0.04)
        vol.set_state(*state)
        return vol, state, (0, 0, 0), P, 10.0
    if name == "slab":  # the high half: index offset 64, its high x end is the volume's
        vol = gf.TSDFVolume(np.array(C1), 0.04, slab=(64, 128))
        state = tuple(np.ascontiguousarray(a[64:]) for a in state)
        vol.set_state(*state)
        return vol, state, (64, 0, 0), P, 10.0
    ht = hf.HashTable(np.array(C1), 0.04, 1 << 16)
    t, w, c = (blocks_of(a) for a in state)
    bxyz = np.stack(np.meshgrid(*(np.arange(16),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    keep = (t != 1.0).any(axis=1)  # (blocks wholly in free space stay absent)
    ht.import_blocks(bxyz[keep], t[keep], w[keep], c[keep])
    return ht, ht.get_state(), (0, 0, 0), P, 10.0


@pytest.mark.parametrize("name", ["dense", "ragged", "slab", "hash"])
def test_rays_entering_through_the_high_faces(name, gf, hf, monkeypatch):
    """Rays that enter through the +x, +y and +z faces and move towards lower indices: the outermost
    brick on the high side holds cells inside the volume next to cells outside it, so the space a ray
    may skip there ends at the volume's face, not at the brick's.  Equal to the reference, and
    byte-identical with TSDF_RAY_SKIP=0."""
    obj, state, off, P, z_far = high_face_case(name, gf, hf)
    monkeypatch.setenv("TSDF_RAY_SKIP", "0")
    brute = high_face_case(name, gf, hf)[0]
    for face, pose in P.items():
        got, ref = check(obj, K_FACE, pose, state=state, off=off, z_far=z_far, min_hits=MIN_HITS)
        every = brute.raycast(K_FACE, pose, HW, z_far=z_far)
        for u, v in zip(got, every):
            assert u.tobytes() == v.tobytes(), face


def test_reflag_and_event_times(dense, frames):
    """TSDF_RAY_REFLAG recomputes the live bits of an unchanged state (same images); with profiling
    on, tsdf_raycast_last_ms reports the live-bit pass and the march of the thread's last raycast."""
    import ctypes
    from tsdf_amd import _ffi
    K, pose = small_K(), frames[0][3]
    want = dense.raycast(K, pose, HW, z_far=Z_FAR, normals=False, colors=False)[0]

    def cast(flags):
        d = np.zeros(HW, np.float32)
        _ffi.call("tsdf_dense_raycast", dense._h, HW[0], HW[1], _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(pose, 16)),
                  0.0, Z_FAR, 0.04, _ffi.ptr(d), None, None, flags)
        a, b = ctypes.c_double(), ctypes.c_double()
        _ffi.call("tsdf_raycast_last_ms", ctypes.byref(a), ctypes.byref(b))
        return d, a.value, b.value

    dense.set_profiling(True)
    try:
        d0, live0, march0 = cast(0)                 # the bits are current: no pass
        d1, live1, march1 = cast(_ffi.RAY_REFLAG)   # recomputed
    finally:
        dense.set_profiling(False)
    assert np.array_equal(d0, want) and np.array_equal(d1, want)
    assert march0 > 0 and march1 > 0 and live0 >= 0 and live1 > 0
    d2, live2, march2 = cast(_ffi.RAY_REFLAG)       # profiling off: the times stay those of the last profiled call
    assert np.array_equal(d2, want) and (live2, march2) == (live1, march1)


def test_out_tensors_are_validated(dense, frames):
    """A tensor the kernel would write out of bounds or to the wrong memory is a ValueError."""
    import torch
    K, pose = small_K(), frames[0][3]
    dev = torch.device("cuda", 0)
    good = torch.zeros(HW, dtype=torch.float32, device=dev)
    bad = [torch.zeros(HW, dtype=torch.float32),                          # host memory
           torch.zeros((HW[0] - 1, HW[1]), dtype=torch.float32, device=dev),  # too small
           torch.zeros(HW, dtype=torch.float64, device=dev),                # wrong dtype
           torch.zeros((HW[0], 2 * HW[1]), dtype=torch.float32, device=dev)[:, ::2],  # strided view
           np.zeros(HW, np.float32)]
    for b in bad:
        with pytest.raises(ValueError):
            dense.raycast(K, pose, HW, z_far=Z_FAR, out=(b, None, None))
    with pytest.raises(ValueError):
        dense.raycast(K, pose, HW, z_far=Z_FAR, out=(good, good, None))  # normals are (H, W, 3)
    with pytest.raises(ValueError):
        dense.raycast(K, pose, HW, z_far=Z_FAR, out=(good, None))
    dense.raycast(K, pose, HW, z_far=Z_FAR, out=(good, None, None))
    assert np.array_equal(good.cpu().numpy(), dense.raycast(K, pose, HW, z_far=Z_FAR)[0])


def test_device_outputs_null_fields_and_async(dense, frames):
    import torch
    from tsdf_amd import _ffi
    K, pose = small_K(), frames[0][3]
    d, n, c = dense.raycast(K, pose, HW, z_far=Z_FAR)
    dev = torch.device("cuda", 0)
    out = (torch.zeros(HW, dtype=torch.float32, device=dev), torch.zeros(HW + (3,), dtype=torch.float32, device=dev),
           torch.zeros(HW + (3,), dtype=torch.uint8, device=dev))
    assert dense.raycast(K, pose, HW, z_far=Z_FAR, out=out) is out
    for a, b in zip((d, n, c), out):
        assert np.array_equal(a, b.cpu().numpy())
    # fields not asked for
    d2, n2, c2 = dense.raycast(K, pose, HW, z_far=Z_FAR, normals=False, colors=False)
    assert n2 is None and c2 is None and np.array_equal(d, d2)
    only_n = (None, torch.zeros(HW + (3,), dtype=torch.float32, device=dev), None)
    dense.raycast(K, pose, HW, z_far=Z_FAR, out=only_n)
    assert np.array_equal(n, only_n[1].cpu().numpy())
    # TSDF_ASYNC: the result is complete after the handle's sync
    late = torch.zeros(HW, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _ffi.call("tsdf_dense_raycast", dense._h, HW[0], HW[1], _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(pose, 16)),
              0.0, Z_FAR, 0.04, late.data_ptr(), None, None, _ffi.DEVICE_PTRS | _ffi.ASYNC)
    dense.sync()
    assert np.array_equal(d, late.cpu().numpy())


def test_bad_arguments_are_refused_with_a_message(gf, hf, dense, frames):
    from tsdf_amd import _ffi
    K, pose = small_K(), frames[0][3]

    def refused(fn, *a, **kw):
        with pytest.raises(_ffi.TSDFError) as e:
            fn(*a, **kw)
        assert e.value.code == _ffi.E_ARG and len(str(e.value)) > 12
        return str(e.value)

    assert "z_step" in refused(dense.raycast, K, pose, HW, z_far=Z_FAR, z_step=0.0)
    refused(dense.raycast, K, pose, HW, z_far=Z_FAR, z_step=-0.04)
    assert "z_far" in refused(dense.raycast, K, pose, HW, z_near=2.0, z_far=1.0)
    assert "z_near" in refused(dense.raycast, K, pose, HW, z_near=-0.1, z_far=Z_FAR)
    d = np.zeros(4, np.float32)
    for h, w in ((0, 83), (61, 0), (1 << 24, 1), (1, 1 << 24), (1 << 14, 1 << 14)):
        with pytest.raises(_ffi.TSDFError) as e:
            _ffi.call("tsdf_dense_raycast", dense._h, h, w, _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(pose, 16)),
                      0.0, Z_FAR, 0.04, _ffi.ptr(d), None, None, 0)
        assert e.value.code == _ffi.E_ARG and "image size" in str(e.value)
    shard = gf.TSDFVolume(np.array(C1), 0.04, shard=(0, 2))
    assert "shard" in refused(shard.raycast, K, pose, HW, z_far=Z_FAR)
    hs = hf.HashTable(np.array(C1), 0.04, 1 << 16, shard=0, n_shards=2)
    assert "shard" in refused(hs.raycast, K, pose, HW, z_far=Z_FAR)
    refused(hs.raycast, K, pose, HW, z_far=Z_FAR, z_step=0.0)
    with pytest.raises(_ffi.TSDFError):
        _ffi.call("tsdf_hash_raycast", None, 61, 83, _ffi.ptr(_ffi.f64(K, 9)), _ffi.ptr(_ffi.f64(pose, 16)),
                  0.0, Z_FAR, 0.04, _ffi.ptr(d), None, None, 0)


def test_raycast_of_the_model_matches_the_depth_it_was_fused_from(dense, frames):
    """From fused pose 0 at the frame's own resolution: over the pixels valid in both, the median
    |raycast - input depth| is below one voxel (the reference alone: 0.0047 m on every 4th pixel,
    tests/test_raycast_cpu.py)."""
    _, depth, _, pose = frames[0]
    d, _, _ = dense.raycast(lounge_intrinsics(), pose, depth.shape, z_far=Z_FAR, normals=False, colors=False)
    both = (d > 0) & (depth > 0)
    med = float(np.median(np.abs(d[both] - depth[both])))
    print(f"lounge: {both.sum()} of {both.size} pixels valid in both, median |raycast - input| {med:.4f} m")
    assert both.sum() > 0.3 * both.size
    assert med < 0.04
