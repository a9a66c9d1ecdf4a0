"""The device's merge (tsdf_dense_merge / tsdf_hash_merge) against its NumPy restatement
(tests/merge_ref.py): the destination byte for byte and the info counts, for dense and hash on either
side; then what a merge must leave right for the calls that follow it -- the canonical flag (an
integrate afterwards), the raycast's live bits -- and the deferred frames, slab shards, repeatability
and refusals.  Volumes <= 96 x 72 x 64."""
import ctypes

import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import icp_ref as I
import merge_ref as M
from test_track_cpu import C1

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = ["dense", "hash"]


@pytest.fixture(scope="module")
def gf():
    from tsdf_amd import grid_fusion
    return grid_fusion


@pytest.fixture(scope="module")
def hf():
    from tsdf_amd import hash_fusion
    return hash_fusion


def blocks_of(t, w, c, mask):
    """Dense arrays and an entry mask as import_blocks takes them: the bricks with an entry."""
    dims = t.shape
    nbk = tuple((d + 7) // 8 for d in dims)
    out = []
    for a, fill in ((t, 1.0), (w, 0.0), (c, 0.0), (mask, False)):
        p = np.full(tuple(8 * k for k in nbk), fill, a.dtype)
        p[:dims[0], :dims[1], :dims[2]] = a
        out.append(p.reshape(nbk[0], 8, nbk[1], 8, nbk[2], 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 8, 8, 8))
    bt, bw, bc, bm = out
    live = np.nonzero(bm.any(axis=(1, 2, 3)))[0]
    bxyz = np.stack(np.unravel_index(live, nbk), axis=1).astype(np.int32)
    # entry words: word z, bit x*8 + y
    bits = (bm[live].astype(np.uint64) << (np.arange(8, dtype=np.uint64)[:, None, None] * np.uint64(8)
                                          + np.arange(8, dtype=np.uint64)[None, :, None])).sum(axis=(1, 2), dtype=np.uint64)
    return bxyz, bt[live].reshape(-1, 512), bw[live].reshape(-1, 512), bc[live].reshape(-1, 512), bits


def make(gf, hf, kind, geo, state=None, mask=None, slab=None, small=False):
    """A handle of `kind` on geo's lattice holding `state` (tsdf, weight, colour); a hash holds the
    entries of `mask` (default: the observed voxels).  small: a table and a pool that must grow."""
    if kind == "dense":
        h = gf.TSDFVolume(geo.bounds(), geo.vs, slab=slab)
        assert np.array_equal(h._vol_origin, geo.origin) and h._trunc_margin == geo.trunc
        if state is not None:
            h.set_state(*state)
        return h
    h = hf.HashTable(geo.bounds(), geo.vs, 64 if small else 1 << 12, max_blocks=16 if small else None)
    assert tuple(h._vol_dim) == geo.dims and np.array_equal(h._vol_origin, geo.origin) and h._trunc_margin == geo.trunc
    if state is not None:
        m = state[1] > 0 if mask is None else mask
        h.import_blocks(*blocks_of(*state, m))
    return h


def entry_mask(h):
    """A hash's entry mask from its exported blocks."""
    bxyz, _, _, _, occ = h.export_blocks()
    dims = tuple(int(d) for d in h._vol_dim)
    nbk = tuple((d + 7) // 8 for d in dims)
    m = np.zeros(tuple(8 * k for k in nbk), bool)
    for (bx, by, bz), words in zip(bxyz, occ):
        for z in range(8):
            bits = np.array([(int(words[z]) >> b) & 1 for b in range(64)], bool)  # bit x*8 + y
            m[bx * 8:bx * 8 + 8, by * 8:by * 8 + 8, bz * 8 + z] = bits.reshape(8, 8)
    return m[:dims[0], :dims[1], :dims[2]]


def same_state(got, want, label=""):
    for g, w, name in zip(got, want, ("tsdf", "weight", "colour")):
        assert g.dtype == F32 and g.tobytes() == np.asarray(w, F32).tobytes(), (label, name, int((g != w).sum()))


def check_against(h, kind, r, info, label):
    same_state(h.get_state(), (r["tsdf"], r["weight"], r["color"]), label)
    want = dict(r["info"])
    if kind == "dense":
        want["blocks_allocated"] = 0
    assert info == want, label
    if kind == "hash":
        hi = h.info()
        # (nothing was freed in these tables: blocks_in_pool is the live blocks)
        assert (hi["used"], hi["entries"], hi["blocks_in_pool"]) == (r["used"], r["entries"], r["used"]), (label, hi)


@pytest.fixture(scope="module")
def sources(gf, hf):
    """The corner source as a dense volume and as a table holding its observed voxels."""
    st = M.source_state()
    return {k: make(gf, hf, k, M.SRC, st) for k in KINDS}


@pytest.mark.parametrize("sk", KINDS)
@pytest.mark.parametrize("dk", KINDS)
@pytest.mark.parametrize("name", list(M.CASES))
def test_case_into_empty(gf, hf, sources, name, dk, sk):
    dst, T, _ = M.CASES[name]
    _, r = M.case_result(name)
    h = make(gf, hf, dk, dst, small=True)
    info = h.merge(sources[sk], T, return_info=True)
    check_against(h, dk, r, info, (name, dk, sk))
    if dk == "hash":
        assert np.array_equal(entry_mask(h), r["mask"])
        assert r["used"] > 64  # (more blocks than the smallest pool and table hold: both had to grow)
        assert h.info()["capacity"] > 64 and h.info()["pool_capacity"] > 64
    h.close()


@pytest.mark.parametrize("sk", KINDS)
@pytest.mark.parametrize("dk", KINDS)
@pytest.mark.parametrize("name", ["rot", "big", "fine", "odd"])
def test_case_into_prefilled(gf, hf, sources, name, dk, sk):
    dst, T, _ = M.CASES[name]
    (t0, w0, c0, m0), r = M.case_result(name, filled=True)
    h = make(gf, hf, dk, dst, (t0, w0, c0), mask=m0, small=True)
    info = h.merge(sources[sk], T, return_info=True)
    check_against(h, dk, r, info, (name, dk, sk))
    assert h.merge(sources[sk], T) == r["info"]["samples"]  # (the plain return value, on a second merge)
    h.close()


def test_big_allocates_360_blocks(gf, hf, sources):
    dst, T, _ = M.CASES["big"]
    h = make(gf, hf, "hash", dst, small=True)
    info = h.merge(sources["dense"], T, return_info=True)
    assert info == {"samples": 104583, "bricks_updated": 360, "blocks_allocated": 360}
    hi = h.info()
    assert (hi["used"], hi["blocks_in_pool"]) == (360, 360) and hi["capacity"] > 360
    h.close()


# ---- the canonical flag: an integrate after the merge --------------------------------------------
LOUNGE = M.Geo((64, 64, 64), (-2.56, -2.56, 0.0), 0.08)  # C1 at 8 cm
PATCH = M.Geo((40, 32, 24), (-1.5, -1.2, 0.8), 0.08)       # a source inside the lounge frames' view


def patch_state(canonical):
    rng = np.random.default_rng(4)
    t = rng.uniform(-1.0, 1.0, PATCH.dims).astype(F32)
    w = rng.integers(0, 7, PATCH.dims).astype(F32)
    c = rng.integers(0, 1 << 24, PATCH.dims).astype(F32)
    if not canonical:
        w = w * F32(0.5)
        c = c * F32(0.25) + F32(0.125)
        assert (w != np.trunc(w)).sum() > 100 and (c != np.trunc(c)).sum() > 100
    return t, w, c


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("sk", KINDS)
@pytest.mark.parametrize("dk", KINDS)
def test_integrate_after_merge(gf, hf, dk, sk, canonical):
    """The merged bytes are the restatement's also for weights in halves and colours that are no
    integers; and a frame integrated into the merged handle gives what it gives a fresh handle set to
    the merged state -- the canonical flag (the integrate's fast paths) is right either way."""
    assert tuple(gf.volume_geometry(np.array(C1), 0.08)[1]) == LOUNGE.dims
    st = patch_state(canonical)
    T = M.rigid(9, 0.07, 6.0)
    src = make(gf, hf, sk, PATCH, st)
    d0 = M.prefilled(LOUNGE, seed=3)
    r = M.merge(LOUNGE, *d0[:3], PATCH, *st, T, d_mask=d0[3])
    assert r["info"]["samples"] > 5000
    h = make(gf, hf, dk, LOUNGE, d0[:3], mask=d0[3])
    info = h.merge(src, T, return_info=True)
    check_against(h, dk, r, info, (dk, sk, canonical))
    fresh = make(gf, hf, dk, LOUNGE, (r["tsdf"], r["weight"], r["color"]), mask=r["mask"])
    _, depth, rgb, pose = load_lounge(1)
    for v in (h, fresh):
        v.integrate(rgb, depth, lounge_intrinsics(), pose)
    a, b = h.get_state(), fresh.get_state()
    assert (a[1] != r["weight"]).sum() > 1000  # (the frame reached the merged voxels)
    same_state(a, b, (dk, sk, canonical))
    if dk == "hash":
        assert h.info()["entries"] == fresh.info()["entries"]
    for v in (h, fresh, src):
        v.close()


# ---- the raycast's live bits ----------------------------------------------------------------------
@pytest.mark.parametrize("dk", KINDS)
def test_raycast_after_merge(gf, hf, sources, dk):
    """A raycast before the merge computes the live bits of the empty volume; the raycast after it
    must see the merged model: that of a fresh handle set to the merged state."""
    _, r = M.case_result("ident")
    h = make(gf, hf, dk, M.SRC)
    before = h.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    assert not before[0].any()
    h.merge(sources["hash" if dk == "dense" else "dense"])
    after = h.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    fresh = make(gf, hf, dk, M.SRC, (r["tsdf"], r["weight"], r["color"]), mask=r["mask"])
    want = fresh.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    assert (want[0] > 0).sum() > 1000
    for a, b in zip(after, want):
        assert a.tobytes() == b.tobytes()
    h.close()
    fresh.close()


# ---- deferred frames ------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", KINDS)
@pytest.mark.parametrize("dk", KINDS)
def test_deferred_frames_run_first(gf, hf, dk, sk):
    """integrate() per frame (deferred batches) on the source and on the destination, then the merge
    with no sync in between: the result of the same calls with explicit syncs."""
    K = lounge_intrinsics()
    frames = [load_lounge(i) for i in range(3)]
    T = M.rigid(2, 0.1, 4.0)
    out = []
    for sync in (False, True):
        src, dst = make(gf, hf, sk, LOUNGE), make(gf, hf, dk, LOUNGE)
        for _, depth, rgb, pose in frames[:2]:
            src.integrate(rgb, depth, K, pose)
        dst.integrate(frames[2][2], frames[2][1], K, frames[2][3])
        if sync:
            src.sync()
            dst.sync()
        n = dst.merge(src, T)
        assert n > 1000
        out.append((n,) + tuple(dst.get_state()))
        src.close()
        dst.close()
    assert out[0][0] == out[1][0]
    same_state(out[0][1:], out[1][1:], (dk, sk))


# ---- slab shards ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", KINDS)
def test_slab_destination(gf, hf, sources, sk):
    """Two slabs of the destination (index_offset), merged separately, hold the unsharded merge."""
    dst, T, _ = M.CASES["rot"]
    (t0, w0, c0, _), r = M.case_result("rot", filled=True)
    n = 0
    for x0, x1 in ((0, 24), (24, 48)):
        h = gf.TSDFVolume(dst.bounds(), dst.vs, slab=(x0, x1))
        h.set_state(t0[x0:x1], w0[x0:x1], c0[x0:x1])
        n += h.merge(sources[sk], T)
        same_state(h.get_state(), (r["tsdf"][x0:x1], r["weight"][x0:x1], r["color"][x0:x1]), (sk, x0))
        h.close()
    assert n == r["info"]["samples"]


@pytest.mark.parametrize("dk", KINDS)
def test_slab_source(gf, hf, dk):
    """A slab of the source is a source with a global index offset: the restatement on that slab."""
    dst, T, _ = M.CASES["rot"]
    st = M.source_state()
    x0, x1 = 16, 48
    geo = M.SRC.slab(x0, x1)
    src = gf.TSDFVolume(M.SRC.bounds(), M.SRC.vs, slab=(x0, x1))
    src.set_state(*(a[x0:x1] for a in st))
    d0 = M.prefilled(dst)
    r = M.merge(dst, *d0[:3], geo, *(a[x0:x1] for a in st), T, d_mask=d0[3])
    whole = M.case_result("rot", filled=True)[1]
    assert 1000 < r["info"]["samples"] < whole["info"]["samples"]
    h = make(gf, hf, dk, dst, d0[:3], mask=d0[3])
    info = h.merge(src, T, return_info=True)
    check_against(h, dk, r, info, dk)
    h.close()
    src.close()


# ---- repeatability --------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", KINDS)
@pytest.mark.parametrize("dk", KINDS)
def test_two_calls_give_identical_bytes(gf, hf, sources, dk, sk):
    dst, T, _ = M.CASES["big"]
    d0 = M.case_result("big", filled=True)[0]
    out = []
    for _ in range(2):
        h = make(gf, hf, dk, dst, d0[:3], mask=d0[3])
        h.merge(sources[sk], T)
        out.append(h.get_state() + ((entry_mask(h),) if dk == "hash" else ()))
        h.close()
    same_state(out[0][:3], out[1][:3], (dk, sk))
    if dk == "hash":
        assert np.array_equal(out[0][3], out[1][3])


# ---- refusals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dk", KINDS)
def test_refusals(gf, hf, sources, dk):
    from tsdf_amd import _ffi
    dst, T, _ = M.CASES["rot"]
    d0 = M.case_result("rot", filled=True)[0]
    h = make(gf, hf, dk, dst, d0[:3], mask=d0[3])
    before = h.get_state()
    fn = "tsdf_dense_merge" if dk == "dense" else "tsdf_hash_merge"
    sd, sh = sources["dense"]._h, sources["hash"]._h
    Tp = _ffi.ptr(_ffi.f64(T, 16))
    info = _ffi.MergeInfo()

    def refused(*args):
        with pytest.raises(_ffi.TSDFError) as e:
            _ffi.call(fn, *args)
        assert e.value.code == _ffi.E_ARG and len(str(e.value)) > 20, str(e.value)

    refused(None, sd, None, Tp, ctypes.byref(info), 0)            # NULL destination
    refused(h._h, sd, None, None, ctypes.byref(info), 0)          # NULL matrix
    refused(h._h, None, None, Tp, ctypes.byref(info), 0)          # no source
    refused(h._h, sd, sh, Tp, ctypes.byref(info), 0)              # two sources
    refused(h._h, sd, None, Tp, ctypes.byref(info), 1)            # flags
    refused(h._h, *((h._h, None) if dk == "dense" else (None, h._h)), Tp, None, 0)  # the same handle
    bad = [np.array(T) for _ in range(5)]
    bad[0][:3, :3] *= 1.0 + 1e-5   # not orthonormal
    bad[1][:3, 0] *= -1.0          # determinant -1
    bad[2][3, 0] = 1e-3            # last row
    bad[3][0, 3] = np.inf
    bad[4][1, 1] = np.nan
    for r in range(3):             # NaN, +inf and -inf in each of the 12 entries
        for c in range(4):
            for v in (np.nan, np.inf, -np.inf):
                bad.append(np.array(T))
                bad[-1][r, c] = v
    import hostile_pose
    bad += list(hostile_pose.merge_nonrigid(T).values())  # scales, a shear, a mirror: no rigid motion (include/tsdf_hip.h)
    for b in bad:
        assert not M.check_transform(b)
        refused(h._h, sd, None, _ffi.ptr(_ffi.f64(b, 16)), None, 0)
        same_state(h.get_state(), before, dk)
    # a rigid transform 1e30 m away is accepted and, as in merge_ref, finds every voxel outside the source
    far = hostile_pose.merge_far(T)
    assert M.check_transform(far) and (M.sample(dst, M.SRC, *M.source_state(), far)[0] == M.OUTSIDE).all()
    for src in sources.values():
        info_far = h.merge(src, far, return_info=True)
        assert info_far["samples"] == 0 and info_far["bricks_updated"] == 0, info_far
        same_state(h.get_state(), before, dk)
    cyc = gf.TSDFVolume(M.SRC.bounds(), M.SRC.vs, shard=(0, 2))
    refused(h._h, cyc._h, None, Tp, None, 0)                      # a cyclic column shard as the source
    hs = hf.HashTable(M.SRC.bounds(), M.SRC.vs, 1 << 10, shard=0, n_shards=2)
    refused(h._h, None, hs._h, Tp, None, 0)                       # a hash shard as the source
    refused(cyc._h if dk == "dense" else hs._h, sd, None, Tp, None, 0)  # ... and as the destination
    fine = make(gf, hf, "dense", M.CASES["fine"][0])
    refused(h._h, fine._h, None, Tp, None, 0)                     # trunc_S < trunc_D: no downsampling
    with pytest.raises(TypeError):
        h.merge(np.zeros(3))
    same_state(h.get_state(), before, dk)
    for v in (h, cyc, hs, fine):
        v.close()
