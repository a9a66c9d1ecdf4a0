"""The dense cull in service waves of the integrate workgroups (k_fused, Stage::cw): a launch with
both an integrate and a cull stage dispatches no cull workgroups; the last cw waves of every
integrate workgroup take (superbrick x all frames) units from one launch-wide cursor before they
join their workgroup's item loop, and every wave drains the cursor once more at its end.
TSDF_CULL_WAVES=n forces cw = n on any unsharded dense handle (0: the cull workgroups), so these
tests run both paths on small volumes and require the same bits and the same statistics.

Every test here calls the HIP path through the C-ABI (tsdf_amd -> libtsdf_hip.so).
"""
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

K = np.array([[585.0, 0, 320], [0, 585.0, 240], [0, 0, 1]])
STATS = ("voxel_updates", "batch_voxels", "bricks_visited", "bricks_touched")


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _frames(n, start):
    from tsdf_amd import scene
    poses = scene.trajectory(n, seed=0, start=start)
    d, c = scene.render(poses, scene.make_spheres(0), seed=0, start=start)
    d, c = np.ascontiguousarray(d.numpy()), np.ascontiguousarray(c.numpy())
    rng = np.random.default_rng(11)
    c[:, ::5, ::3] = rng.integers(0, 256, c[:, ::5, ::3].shape, dtype=np.uint8)  # every byte value
    d[:, 40:60, 100:180] = 65535  # invalid under the demos' mask (grid_demo1.py:82)
    return d, c, poses


@functools.lru_cache(maxsize=None)
def _oracle(bnds, vs, n, start):
    """The oracle's state after the frames (computed once per geometry, never written to)."""
    d, c, poses = _frames(n, start)
    orc = O.OracleTSDFVolume(np.array(bnds), vs)
    upd = 0
    for f in range(len(d)):
        m = d[f].astype(float) / 1000.0
        m[m == 65.535] = 0
        upd += orc.integrate(c[f], m, K, poses[f])
    return orc, upd


def _run(vol, d, c, poses, ingest):
    import torch
    Tinv = np.linalg.inv(poses)
    if ingest == "host":
        vol.integrate_batch(d, c, K, Tinv, sync=False, invalid_65535=True)
    else:
        dd, cc = torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(c).cuda()
        torch.cuda.synchronize()
        vol.integrate_batch(dd.data_ptr(), cc.data_ptr(), K, Tinv, hw=d.shape[1:], device_ptrs=True,
                            sync=False, invalid_65535=True)
    vol.sync()
    st = vol.stats()
    return vol.get_state(), {k: st[k] for k in STATS}


def _against_oracle(bnds, n, start, ingest, monkeypatch):
    from tsdf_amd import grid_fusion
    monkeypatch.setenv("TSDF_BATCH", "8")
    d, c, poses = _frames(n, start)
    orc, upd = _oracle(bnds, 0.08, n, start)
    assert upd > 10_000
    for tex in ("0", "1"):
        monkeypatch.setenv("TSDF_TEXEL", tex)
        base = None
        for cw in ("0", "1", "2", "12"):
            monkeypatch.setenv("TSDF_CULL_WAVES", cw)
            vol = grid_fusion.TSDFVolume(np.array(bnds), 0.08)
            (T, W, C), st = _run(vol, d, c, poses, ingest)
            vol.close()
            assert _same(T, orc._tsdf_vol_cpu) and _same(W, orc._weight_vol_cpu) and _same(C, orc._color_vol_cpu), (tex, cw)
            assert st["voxel_updates"] == upd and st["bricks_visited"] > 0, (tex, cw, st)
            if base is None:
                base = st
            assert st == base, (tex, cw)


@pytest.mark.parametrize("ingest", ["device", "host"])
def test_service_waves_equal_cull_workgroups_and_oracle(ingest, monkeypatch):
    """128^3 @ 8 cm (64 superbricks: most service waves find the cursor empty), 21 frames in batches
    of 8 -- two full launches, a ragged one and the fill launches without an integrate stage --
    with 0 (cull workgroups), 1, 2 and 12 service waves, on texels and on two gathers: the
    oracle's bits every time, and the same four statistics as the cull workgroups."""
    _against_oracle(((0.0, 10.24),) * 3, 21, 260, ingest, monkeypatch)


@pytest.mark.parametrize("ingest", ["device", "host"])
def test_ragged_volume_partial_bricks_and_superbricks(ingest, monkeypatch):
    """100 x 61 x 45 voxels @ 8 cm: 13 x 8 x 6 bricks, so a partial brick and a partial superbrick
    (4 x 4 x 4 bricks) on every axis; 9 frames (a full and a one-frame launch)."""
    from tsdf_amd import grid_fusion
    bnds = ((1.0, 8.97), (2.5, 7.35), (3.0, 6.58))
    dims = grid_fusion.volume_geometry(np.array(bnds), 0.08)[1]
    assert tuple(int(x) for x in dims) == (100, 61, 45)
    _against_oracle(bnds, 9, 260, ingest, monkeypatch)


def test_one_service_wave_takes_several_units(monkeypatch):
    """256^3 @ 4 cm (512 superbricks) with one integrate workgroup per CU and one service wave
    each: fewer service waves than units, so a wave takes several.  State and statistics as with
    the cull workgroups on the same geometry (which the other dense tests pin to the oracle)."""
    from tsdf_amd import grid_fusion
    monkeypatch.setenv("TSDF_BATCH", "8")
    monkeypatch.setenv("TSDF_FUSED_GI_PER_CU", "1")
    d, c, poses = _frames(9, 260)
    bnds = np.array([[0.0, 10.24]] * 3)
    out = {}
    for cw in ("0", "1"):
        monkeypatch.setenv("TSDF_CULL_WAVES", cw)
        vol = grid_fusion.TSDFVolume(bnds.copy(), 0.04)
        out[cw] = _run(vol, d, c, poses, "device")
        vol.close()
    (s0, st0), (s1, st1) = out["0"], out["1"]
    assert st0["bricks_visited"] > 0 and st0["voxel_updates"] > 0
    assert st1 == st0
    for a, b in zip(s0, s1):
        assert _same(a, b)


def test_shards_ignore_the_knob(monkeypatch):
    """A 2-shard handle (tsdf_dense_create_shard) keeps its cull workgroups whatever
    TSDF_CULL_WAVES says: the same rows and statistics with 2 as with 0."""
    from tsdf_amd import grid_fusion
    monkeypatch.setenv("TSDF_BATCH", "8")
    d, c, poses = _frames(9, 260)
    bnds = np.array([[0.0, 10.24]] * 3)
    out = {}
    for cw in ("0", "2"):
        monkeypatch.setenv("TSDF_CULL_WAVES", cw)
        for rank in range(2):
            vol = grid_fusion.TSDFVolume(bnds.copy(), 0.08, shard=(rank, 2))
            out[cw, rank] = _run(vol, d, c, poses, "device")
            vol.close()
    for rank in range(2):
        (s0, st0), (s2, st2) = out["0", rank], out["2", rank]
        assert st0["bricks_visited"] > 0 and st0["voxel_updates"] > 0
        assert st2 == st0
        for a, b in zip(s0, s2):
            assert _same(a, b)
