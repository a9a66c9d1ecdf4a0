"""The integrate's 16.16 fixed-point pixel path and the texels' invalid-depth sentinel on the GPU,
bit for bit against the oracle in tsdf, weight and colour: 64^3 volumes at 4 cm, at most 8 frames,
each case on the dense handle with TSDF_TEXEL 0 and 1 and on the hash.  (The library picks the
kernel: frames whose width is no multiple of 4 go through the in-line kernels, the others through
the fused launch.)  The two cases with fx != fy and the principal point off the image also arrive as
device-resident tensors, as f64 metres and frame by frame through the deferred integrate().

Every test here calls the HIP path through the C-ABI (tsdf_amd -> libtsdf_hip.so).
"""
import numpy as np
import pytest

import pixel_fixed_cases as P

pytestmark = pytest.mark.gpu

MODES = ("dense-texel0", "dense-texel1", "hash")


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


HOWS = ("host", "device", "f64", "deferred")


def run(name, mode, monkeypatch, how="host"):
    """how: the u16 frames as host arrays in one batch; as device-resident tensors (device_ptrs); as
    f64 metres; or frame by frame through the deferred integrate() (get_state runs the pending ones)."""
    from tsdf_amd import grid_fusion, hash_fusion
    for k in ("TSDF_TEXEL", "TSDF_PIPELINE", "TSDF_DENSE_NZ", "TSDF_BATCH"):
        monkeypatch.delenv(k, raising=False)
    if mode != "hash":
        monkeypatch.setenv("TSDF_TEXEL", mode[-1])
    d, rgb, K, poses, inv = P.case(name)
    vol = hash_fusion.HashTable(P.bounds(), P.VS, 1 << 14) if mode == "hash" else grid_fusion.TSDFVolume(P.bounds(), P.VS)
    if how == "host":
        vol.integrate_batch(d, rgb, K, np.linalg.inv(poses), invalid_65535=inv)
    elif how == "device":
        import torch
        dd, cc = torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
        torch.cuda.synchronize()  # the handle's stream does not follow torch's
        vol.integrate_batch(dd.data_ptr(), cc.data_ptr(), K, np.linalg.inv(poses), hw=d.shape[1:], device_ptrs=True,
                            invalid_65535=inv)
    elif how == "f64":
        assert not inv  # (the 65535 mask is a u16 convention)
        vol.integrate_batch(d.astype(np.float64) / 1000.0, rgb, K, np.linalg.inv(poses))
    else:
        assert how == "deferred" and not inv and vol.defer
        for f in range(len(d)):
            vol.integrate(rgb[f], d[f], K, poses[f])
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


@pytest.mark.parametrize("how", HOWS[1:])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["small-97x61", "small-100x61"])
def test_anisotropic_off_image_camera_by_every_way_in(name, mode, how, monkeypatch):
    """The two cases with fx 90 / fy 110 and the principal point off the image, by the other ways a
    frame reaches the kernels: device-resident tensors (97 wide: the in-line kernels read the device
    pointers; 100 wide: the fused launch with a partial prep tile in x), f64 metres, and one deferred
    integrate() per frame.  The same bits, voxel updates and list errors as from host u16 arrays."""
    run(name, mode, monkeypatch, how)
