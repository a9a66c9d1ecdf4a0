"""Every integrate variant's slow update paths against the oracle, bit for bit.

The update (integrate_brick, csrc/tsdf_device.h) picks per wave, from the state it loads, between
RN(1/n) from the LDS table (integer weights below L1 = 4063), from the HBM table (below L2 =
65503), IEEE division, packed or exact colours and the free-space shortcut, and may change its
choice whenever a lane first loads its column.  update_paths.py preloads 128^3 volumes so that
chosen waves take each route and each route change (test_update_paths_cpu.py proves that from the
oracle alone); this file runs those volumes through every kernel instantiation the dispatches of
csrc/tsdf_dense.hip and csrc/tsdf_hash.hip can pick, plus the Vol::canon hand-over between calls
and the smallest volumes whose default dispatch takes the texel kernels.  DESIGN.md §2 maps the
instantiations to the cases.

Every test here calls the HIP path through the C-ABI (tsdf_amd -> libtsdf_hip.so).
"""
import numpy as np
import pytest

import update_paths as U

pytestmark = pytest.mark.gpu

ENV_KNOBS = ("TSDF_TEXEL", "TSDF_PIPELINE", "TSDF_DENSE_NZ")


def path(hash=False, pipeline=1, texel=0, nz=4, depth="u16", colour="rgb8"):
    return dict(hash=hash, pipeline=pipeline, texel=texel, nz=nz, depth=depth, colour=colour)


# the issue's matrix: name -> how the path is reached
PATHS = {
    "dense-fused-2g": path(),                                   # k_fused<1,4,0> / CU
    "dense-fused-texel": path(texel=1),                         # k_fused<1,4,2> / CU
    "dense-fused-f64": path(depth="f64"),                       # k_fused<1,4,1> / CU
    "dense-inline": path(pipeline=0),                           # k_integrate<false,0,0,true,4>
    "dense-inline-folded": path(colour="f32"),                  # k_integrate<false,0,1,true,4> (in-line by rule)
    "dense-nz8-fused": path(nz=8),                              # k_fused<1,8,0>
    "dense-nz8-inline": path(nz=8, pipeline=0),                 # k_integrate<false,0,0,true,8>
    "hash-fused-2g": path(hash=True),                           # k_fused_hash<0> / CU
    "hash-fused-texel": path(hash=True, texel=1),               # k_fused_hash<2> / CU
    "hash-fused-f64": path(hash=True, depth="f64"),             # k_fused_hash<1> / CU
    "hash-inline": path(hash=True, pipeline=0),                 # k_integrate<true,0,0,true>
}
OW_PATHS = ("dense-fused-2g", "dense-fused-texel", "dense-fused-f64", "dense-inline")
# the instantiations of the dispatch switches that the matrix and the obs_weight cases leave:
# (path, per-frame obs_weight cycle)
REST = {
    "dense-nz8-fused-ow": (path(nz=8), True),                                  # k_fused<0,8,0>
    "dense-nz8-fused-f64": (path(nz=8, depth="f64"), False),                   # k_fused<1,8,1>
    "dense-nz8-fused-f64-ow": (path(nz=8, depth="f64"), True),                 # k_fused<0,8,1>
    "dense-inline-folded-ow": (path(colour="f32"), True),                      # k_integrate<false,0,1,false,4>
    "dense-inline-f64": (path(pipeline=0, depth="f64"), False),                # <false,1,0,true,4>
    "dense-inline-f64-ow": (path(pipeline=0, depth="f64"), True),              # <false,1,0,false,4>
    "dense-inline-f64-folded": (path(depth="f64", colour="f32"), False),       # <false,1,1,true,4>
    "dense-inline-f64-folded-ow": (path(depth="f64", colour="f32"), True),     # <false,1,1,false,4>
    "dense-nz8-inline-ow": (path(nz=8, pipeline=0), True),                     # <false,0,0,false,8>
    "dense-nz8-inline-folded": (path(nz=8, colour="f32"), False),              # <false,0,1,true,8>
    "dense-nz8-inline-folded-ow": (path(nz=8, colour="f32"), True),            # <false,0,1,false,8>
    "dense-nz8-inline-f64": (path(nz=8, pipeline=0, depth="f64"), False),      # <false,1,0,true,8>
    "dense-nz8-inline-f64-ow": (path(nz=8, pipeline=0, depth="f64"), True),    # <false,1,0,false,8>
    "dense-nz8-inline-f64-folded": (path(nz=8, depth="f64", colour="f32"), False),     # <false,1,1,true,8>
    "dense-nz8-inline-f64-folded-ow": (path(nz=8, depth="f64", colour="f32"), True),   # <false,1,1,false,8>
    "hash-inline-folded": (path(hash=True, colour="f32"), False),              # k_integrate<true,0,1,true>
    "hash-inline-f64": (path(hash=True, pipeline=0, depth="f64"), False),      # k_integrate<true,1,0,true>
    "hash-inline-f64-folded": (path(hash=True, depth="f64", colour="f32"), False),     # k_integrate<true,1,1,true>
}


@pytest.fixture(scope="module")
def expected():
    """The oracle's (tsdf, weight, colour, voxel updates) per (preload kind, scene, obs_weight
    pattern), computed once and left unchanged."""
    cache = {}

    def get(kind, scene, ow=False):
        key = (kind, scene, ow)
        if key not in cache:
            d, c, poses = U.frames(scene)
            t, w, c_, n = U.oracle_run(U.preload(scene, kind), d, c, poses, U.ow_cycle(U.NF) if ow else None)
            for a in (t, w, c_):
                a.setflags(write=False)
            cache[key] = (t, w, c_, n)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def inputs():
    """The scenes' frames in the formats the paths take: same values, so the same oracle result."""
    cache = {}

    def get(scene, depth="u16", colour="rgb8"):
        d, c, poses = U.frames(scene)
        if ("d", scene, depth) not in cache:
            cache["d", scene, depth] = d if depth == "u16" else d.astype(float) / 1000.0
        if ("c", colour) not in cache:
            cache["c", colour] = c if colour == "rgb8" else U.fold(c)
        return cache["d", scene, depth], cache["c", colour], np.linalg.inv(poses)
    return get


def make(p, monkeypatch, voxel_size=U.VS, map_size=8192, knobs=True):
    """A fresh handle on the path's dispatch (the library reads the environment at create)."""
    from tsdf_amd import grid_fusion, hash_fusion
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSDF_BATCH", str(U.NF))
    if knobs:
        monkeypatch.setenv("TSDF_TEXEL", str(p["texel"]))
        monkeypatch.setenv("TSDF_PIPELINE", str(p["pipeline"]))
        if p["nz"] != 4:
            monkeypatch.setenv("TSDF_DENSE_NZ", str(p["nz"]))
    if p["hash"]:
        vol = hash_fusion.HashTable(U.bounds(), voxel_size, map_size)
    else:
        vol = grid_fusion.TSDFVolume(U.bounds(), voxel_size)
    assert vol.frames_per_launch() == U.NF  # one launch holds a whole scene
    return vol


def load(vol, p, scene, kind):
    if p["hash"]:
        vol.import_blocks(*U.preloaded_blocks(scene, kind))
    else:
        vol.set_state(*U.preload(scene, kind))


def run(vol, p, frames, ow=None, lo=0, hi=U.NF):
    d, c, Tinv = frames
    if p["hash"]:
        vol.integrate_batch(d[lo:hi], c[lo:hi], U.intrinsics(), Tinv[lo:hi])
    else:
        vol.integrate_batch(d[lo:hi], c[lo:hi], U.intrinsics(), Tinv[lo:hi], None if ow is None else ow[lo:hi])


def check(vol, p, exp, n_updates, where=None):
    """State equal to the oracle's bit for bit, the oracle's update count, no list errors and (hash)
    no brick skipped.  `where` = (scene, kind) names the classes of differing voxels."""
    got = vol.get_state()
    st = vol.stats()
    vol.close()
    ok = [U.same(g, e) for g, e in zip(got, exp)]
    assert all(ok), U.mismatch_by_class(*where, got, exp) if where else ok
    assert st["voxel_updates"] == n_updates
    assert st["list_errors"] == 0
    if p["hash"]:
        assert st["bricks_skipped"] == 0


@pytest.mark.parametrize("name", PATHS)
@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("scene", U.SCENES)
def test_preloaded_routes(scene, kind, name, expected, inputs, monkeypatch):
    """One 32-frame launch into the preloaded volume: every class of item (LDS, HBM and IEEE
    quotients, exact colours, free space, and the route changes inside the batch) equals the
    oracle.  The canonical preload keeps Vol::canon, so the fused launches run their u32-colour
    (CU) instantiations; the mixed one clears it."""
    p = PATHS[name]
    t, w, c, n = expected(kind, scene)
    vol = make(p, monkeypatch)
    load(vol, p, scene, kind)
    run(vol, p, inputs(scene, p["depth"], p["colour"]))
    check(vol, p, (t, w, c), n, (scene, kind))


@pytest.mark.parametrize("name", OW_PATHS)
def test_preloaded_routes_with_obs_weights(name, expected, inputs, monkeypatch):
    """Per-frame obs_weight 1.0, 0.6, 2.0, ... (OW1 = false kernels) on the mixed preload."""
    p = PATHS[name]
    t, w, c, n = expected("mixed", "moving", True)
    vol = make(p, monkeypatch)
    load(vol, p, "moving", "mixed")
    run(vol, p, inputs("moving", p["depth"], p["colour"]), U.ow_cycle(U.NF))
    check(vol, p, (t, w, c), n, ("moving", "mixed"))


@pytest.mark.parametrize("name", REST)
def test_remaining_instantiations(name, expected, inputs, monkeypatch):
    """The kernels of the dispatch switches that the matrix above does not reach (f64 depth and
    folded colour in-line, NZ = 8 with each input kind, obs_weight != 1 beside them), on the
    mixed preload and the moving scene."""
    p, ow = REST[name]
    t, w, c, n = expected("mixed", "moving", ow)
    vol = make(p, monkeypatch)
    load(vol, p, "moving", "mixed")
    run(vol, p, inputs("moving", p["depth"], p["colour"]), U.ow_cycle(U.NF) if ow else None)
    check(vol, p, (t, w, c), n, ("moving", "mixed"))


# ------------------------------------------------------------------------------ canon hand-over
def _then(first, d, c, poses, ow=None, state=None):
    """The oracle over `first` = (depth, rgb, poses, ow) and then the frames given."""
    import oracle as O
    orc = O.OracleTSDFVolume(U.bounds(), U.VS)
    n1 = U.oracle_run(state, *first, into=orc)[3]
    t, w, c_, n2 = U.oracle_run(None, d, c, poses, ow, into=orc)
    return t, w, c_, n1 + n2


@pytest.fixture(scope="module")
def handed_over():
    cache = {}

    def get(which):
        if which not in cache:
            d, c, poses = U.frames("moving")
            first = {"ow": (d[:8], c[:8], poses[:8], np.full(8, 0.6)),
                     "float": (d[:8], c[:8], poses[:8], None)}[which]
            cache[which] = _then(first, d, c, poses)
        return cache[which]
    return get


@pytest.mark.parametrize("texel", [0, 1])
def test_canon_handover_after_obs_weight(texel, handed_over, inputs, monkeypatch):
    """8 frames with obs_weight 0.6 leave non-integer weights; the next call's obs_weight-1 RGB8
    launches on the same handle must not take the canonical (range-test only) kernels."""
    p = path(texel=texel)
    d, c, Tinv = inputs("moving")
    vol = make(p, monkeypatch)
    vol.integrate_batch(d[:8], c[:8], U.intrinsics(), Tinv[:8], np.full(8, 0.6))
    run(vol, p, (d, c, Tinv))
    t, w, c_, n = handed_over("ow")
    assert (w != np.trunc(w)).any()
    check(vol, p, (t, w, c_), n)


@pytest.mark.parametrize("texel", [0, 1])
def test_canon_handover_after_float_colour(texel, handed_over, inputs, monkeypatch):
    """8 frames of folded float colour (in-line kernels), then 32 RGB8 frames (fused)."""
    p = path(texel=texel)
    d, c, Tinv = inputs("moving")
    vol = make(p, monkeypatch)
    vol.integrate_batch(d[:8], inputs("moving", "u16", "f32")[1][:8], U.intrinsics(), Tinv[:8])
    run(vol, p, (d, c, Tinv))
    t, w, c_, n = handed_over("float")
    check(vol, p, (t, w, c_), n)


@pytest.mark.parametrize("texel", [0, 1])
def test_canon_handover_set_state(texel, expected, handed_over, inputs, monkeypatch):
    """set_state(mixed) clears the flag, 8 frames run, set_state(canonical) sets it again: the 32
    frames that follow equal the oracle from the canonical preload."""
    p = path(texel=texel)
    frames = inputs("moving")
    vol = make(p, monkeypatch)
    load(vol, p, "moving", "mixed")
    run(vol, p, frames, hi=8)
    # (which voxels a frame updates does not depend on the state: the first 8 frames' count from
    # the fresh hand-over run)
    n8 = handed_over("float")[3] - U.activity("moving")["n"]
    assert vol.stats()["voxel_updates"] == n8 > 0
    load(vol, p, "moving", "canonical")
    run(vol, p, frames)
    t, w, c, n = expected("canonical", "moving")
    check(vol, p, (t, w, c), n8 + n, ("moving", "canonical"))


@pytest.mark.parametrize("texel", [0, 1])
def test_hash_add_entries_then_integrate(texel, inputs, monkeypatch):
    """add_entries on a fresh table: about 100 voxels the scene updates, with weights 4070 and
    0.5 and one odd colour, clear the table's flag; the 32 frames then equal the oracle."""
    p = path(hash=True, texel=texel)
    d, c, poses = U.frames("moving")
    upd = np.flatnonzero(U.activity("moving")["count"].reshape(-1) > 0)
    idx = upd[::len(upd) // 100][:100]
    ijk = np.stack(np.unravel_index(idx, (U.N,) * 3), 1)
    rng = np.random.default_rng(5)
    tv = rng.uniform(-1, 1, len(idx)).astype(np.float32)
    wv = np.where(np.arange(len(idx)) % 2 == 0, 4070.0, 0.5).astype(np.float32)
    cv = U._canon(rng, len(idx))
    cv[7] = U.ODD[3]
    state = [np.ones((U.N,) * 3, np.float32), np.zeros((U.N,) * 3, np.float32), np.zeros((U.N,) * 3, np.float32)]
    for a, v in zip(state, (tv, wv, cv)):
        a.reshape(-1)[idx] = v
    t, w, c_, n = U.oracle_run(state, d, c, poses)
    vol = make(p, monkeypatch)
    vol.add_entries(ijk, tv, wv, cv)
    run(vol, p, inputs("moving"))
    check(vol, p, (t, w, c_), n)


@pytest.mark.parametrize("texel", [0, 1])
def test_hash_import_blocks_handover(texel, inputs, monkeypatch):
    """import_blocks(canonical) and 8 frames on the u32-colour kernels, then an import of a few
    blocks of odd colours and the other 24 frames."""
    import oracle as O
    p = path(hash=True, texel=texel)
    d, c, poses = U.frames("moving")
    bxyz, bt, bw, bc = U.preloaded_blocks("moving", "canonical")
    rng = np.random.default_rng(6)
    pick = np.arange(0, len(bxyz), len(bxyz) // 6)[:6]
    ot = rng.uniform(-1, 1, (len(pick), 512)).astype(np.float32)
    ow_ = np.full((len(pick), 512), 50, np.float32)
    oc = rng.choice(U.ODD, (len(pick), 512)).astype(np.float32)
    orc = O.OracleTSDFVolume(U.bounds(), U.VS)
    n = U.oracle_run(U.preload("moving", "canonical"), d[:8], c[:8], poses[:8], into=orc)[3]
    for j, (bx, by, bz) in enumerate(bxyz[pick]):
        s = (slice(8 * bx, 8 * bx + 8), slice(8 * by, 8 * by + 8), slice(8 * bz, 8 * bz + 8))
        orc._tsdf_vol_cpu[s], orc._weight_vol_cpu[s], orc._color_vol_cpu[s] = (
            a[j].reshape(8, 8, 8) for a in (ot, ow_, oc))
    t, w, c_, n2 = U.oracle_run(None, d[8:], c[8:], poses[8:], into=orc)
    frames = inputs("moving")
    vol = make(p, monkeypatch)
    vol.import_blocks(bxyz, bt, bw, bc)
    run(vol, p, frames, hi=8)
    vol.import_blocks(bxyz[pick], ot, ow_, oc)
    run(vol, p, frames, lo=8)
    check(vol, p, (t, w, c_), n + n2)


# ------------------------------------------------------------------------------ rule-selected texels
def _layer_preload(rng, ny, nz):
    """8 x rows of random weights in [4040, 4100) with 30 % zeros and 25 % odd colours."""
    shape = (8, ny, nz)
    w0 = rng.integers(4040, 4100, shape).astype(np.float32)
    w0[rng.random(shape) < 0.3] = 0.0
    t0 = rng.uniform(-1, 1, shape).astype(np.float32)
    c0 = np.where(rng.random(shape) < 0.25, rng.choice(U.ODD, shape), U._canon(rng, shape)).astype(np.float32)
    return t0, w0, c0


def test_dense_texels_by_rule(inputs, monkeypatch):
    """No TSDF_TEXEL in the environment: a 320^3 volume (64,000 bricks >= 3 * 2^14) takes the texel
    kernels by Base::texel_for.  Weights around L1 and odd colours everywhere (the 8-row layer
    below repeated along x); the rows of brick layer 20 equal the oracle restricted to them."""
    vs, layer = 0.032, 20
    vol = make(path(), monkeypatch, voxel_size=vs, knobs=False)
    dims = [int(x) for x in vol._vol_dim]
    assert int(np.prod([(x + 7) // 8 for x in dims])) >= 3 << 14
    t0, w0, c0 = _layer_preload(np.random.default_rng(12), dims[1], dims[2])
    vol.set_state(*(np.tile(a, ((dims[0] + 7) // 8, 1, 1))[:dims[0]] for a in (t0, w0, c0)))
    frames = inputs("moving")
    run(vol, path(), frames)
    rows = np.arange(8 * layer, 8 * layer + 8)
    d, c, poses = U.frames("moving")
    t, w, c_, n = U.oracle_run((t0, w0, c0), d, c, poses, voxel_size=vs, x_index=rows)
    assert n > 100_000 and (w > U.L1 + 16).any() and ((w > 0) & (w < U.L1)).any()
    got = vol.get_rows(rows)
    assert vol.stats()["list_errors"] == 0
    vol.close()
    assert [U.same(g, e) for g, e in zip(got, (t, w, c_))] == [True] * 3


def test_hash_texels_by_rule(inputs, monkeypatch):
    """No TSDF_TEXEL in the environment: a table over 410^3 voxels (140,608 bricks >= 3 * 2^15) takes
    the texel kernels by the rule.  Every other block of brick layer 26 is imported with weights
    around L1 and odd colours; the layer's rows, read back through lookup, hold an entry where a
    block was imported or the oracle updated, and the oracle's values everywhere."""
    vs, layer = 0.025, 26
    p = path(hash=True)
    vol = make(p, monkeypatch, voxel_size=vs, map_size=1 << 16, knobs=False)
    dims = [int(x) for x in vol._vol_dim]
    nb = [(x + 7) // 8 for x in dims]
    assert int(np.prod(nb)) >= 3 << 15
    t0, w0, c0 = _layer_preload(np.random.default_rng(13), 8 * nb[1], 8 * nb[2])
    by, bz = (a.reshape(-1) for a in np.meshgrid(np.arange(nb[1]), np.arange(nb[2]), indexing="ij"))
    keep = (by + bz) % 2 == 0
    bxyz = np.stack([np.full(keep.sum(), layer), by[keep], bz[keep]], 1).astype(np.int32)

    def as_blocks(a):
        return np.ascontiguousarray(a.reshape(8, nb[1], 8, nb[2], 8).transpose(1, 3, 0, 2, 4)).reshape(-1, 512)[keep]
    vol.import_blocks(bxyz, as_blocks(t0), as_blocks(w0), as_blocks(c0))
    run(vol, p, inputs("moving"))
    # the oracle's start: the preload inside imported blocks, (1, 0, 0) elsewhere
    imported = np.repeat(np.repeat(keep.reshape(nb[1], nb[2]), 8, 0), 8, 1)[None, :dims[1], :dims[2]]
    imported = np.broadcast_to(imported, (8, dims[1], dims[2]))
    start = [np.where(imported, a[:, :dims[1], :dims[2]], fill).astype(np.float32)
             for a, fill in zip((t0, w0, c0), (1.0, 0.0, 0.0))]
    rows = np.arange(8 * layer, 8 * layer + 8)
    d, c, poses = U.frames("moving")
    t, w, c_, n, _, count = U.oracle_run(start, d, c, poses, voxel_size=vs, x_index=rows, masks=True)
    assert n > 100_000 and (w > U.L1 + 16).any() and ((count > 0) & ~imported).any()
    ijk = np.stack(np.meshgrid(rows, np.arange(dims[1]), np.arange(dims[2]), indexing="ij"), -1).reshape(-1, 3)
    found, gt, gw, gc = vol.lookup(ijk)
    st = vol.stats()
    vol.close()
    assert np.array_equal(found.reshape(t.shape), imported | (count > 0))
    assert [U.same(g.reshape(t.shape), e) for g, e in zip((gt, gw, gc), (t, w, c_))] == [True] * 3
    assert st["list_errors"] == 0 and st["bricks_skipped"] == 0
