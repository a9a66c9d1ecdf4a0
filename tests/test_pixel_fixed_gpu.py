"""The integrate's 16.16 fixed-point pixel path and the texels' invalid-depth sentinel on the GPU,
bit for bit against the oracle in tsdf, weight and colour: 64^3 volumes at 4 cm, at most 8 frames,
each case on the dense handle with TSDF_TEXEL 0 and 1 and on the hash.  (The library picks the
kernel: frames whose width is no multiple of 4 go through the in-line kernels, the others through
the fused launch.)

Every test here calls the HIP path through the C-ABI (tsdf_amd -> libtsdf_hip.so).
"""
import numpy as np
import pytest

import pixel_fixed_cases as P

pytestmark = pytest.mark.gpu

MODES = ("dense-texel0", "dense-texel1", "hash")


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def run(name, mode, monkeypatch):
    from tsdf_amd import grid_fusion, hash_fusion
    for k in ("TSDF_TEXEL", "TSDF_PIPELINE", "TSDF_DENSE_NZ", "TSDF_BATCH"):
        monkeypatch.delenv(k, raising=False)
    if mode != "hash":
        monkeypatch.setenv("TSDF_TEXEL", mode[-1])
    d, rgb, K, poses, inv = P.case(name)
    vol = hash_fusion.HashTable(P.bounds(), P.VS, 1 << 14) if mode == "hash" else grid_fusion.TSDFVolume(P.bounds(), P.VS)
    vol.integrate_batch(d, rgb, K, np.linalg.inv(poses), invalid_65535=inv)
    got = vol.get_state()
    st = vol.stats()
    vol.close()
    t, w, c, n = P.expected(name)
    assert n > 0 and int((w > 0).sum()) > 0
    assert [same(g, e) for g, e in zip(got, (t, w, c))] == [True] * 3
    assert st["voxel_updates"] == n and st["list_errors"] == 0
    if mode == "hash":
        assert st["bricks_skipped"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", P.CASES)
def test_bit_exact_against_the_oracle(name, mode, monkeypatch):
    run(name, mode, monkeypatch)
