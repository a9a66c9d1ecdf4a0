"""The integrate's 16.16 fixed-point pixel path and the texels' invalid-depth sentinel, on the
CPU: tools/check_pixel_fixed.c runs the host functions the library itself uses (csrc/tsdf_pixel.h)
against the reference's rint((x*fx)/z + cx)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
import pixel_fixed_cases as P


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("pixel_fixed"), "chk")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tools", "check_pixel_fixed.c"), "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    rows = {}
    for m in re.finditer(r"pixel_fixed (\w) checked (\d+)(?: fine (\d+))? bad (\d+)", out.stdout):
        rows[m.group(1)] = (int(m.group(2)), int(m.group(3) or 0), int(m.group(4)))
    assert set(rows) == set("abcde"), out.stdout + out.stderr
    rows["rc"] = out.returncode
    return rows


def test_fine_pixels_equal_the_reference_on_random_steps(report):
    """(a) 1e7 random (numerator, z, principal point): image sides 1..16384, principal points on and
    off the 2^-16 grid, negative and large; the reciprocal off by up to 2^-24.4."""
    n, fine, bad = report["a"]
    assert n >= 10_000_000 and fine > 0.9 * n and bad == 0


def test_fine_pixels_equal_the_reference_next_to_every_boundary(report):
    """(b) values within 3e-4 px of every half-integer: some are kept, none of those is wrong."""
    n, fine, bad = report["b"]
    assert n > 1_000_000 and 0 < fine < n and bad == 0


def test_no_step_past_zmin_aliases_into_the_image(report):
    n, fine, bad = report["c"]
    assert n > 1_000_000 and fine > 0 and bad == 0


def test_non_finite_and_oversized_frames_take_no_fast_path(report):
    n, _, bad = report["d"]
    assert n >= 50 and bad == 0


def test_invalid_texel_depth_fails_the_truncation_test(report):
    n, _, bad = report["e"]
    assert n > 65535 and bad == 0
    assert report["rc"] == 0


def test_the_boundary_case_lands_on_boundaries():
    """On the CPU: the oracle's own pixel lies within 2e-4 of a rounding boundary for at least 1 %
    of the boundary case's steps in front of the camera and inside the image."""
    d = P.case("boundary-hits")[0]
    H, W = d.shape[1:]
    near = steps = 0
    for f in range(len(d)):
        u, v, z = P.projection("boundary-hits", f)
        ok = (z > 0) & (np.rint(u) >= 0) & (np.rint(u) < W) & (np.rint(v) >= 0) & (np.rint(v) < H)
        u, v = u[ok], v[ok]
        edge = (np.abs(u - np.rint(u)) > 0.5 - 2e-4) | (np.abs(v - np.rint(v)) > 0.5 - 2e-4)
        near += int(edge.sum())
        steps += int(ok.sum())
    print(f"boundary-hits: {near} of {steps} steps within 2e-4 px of a boundary")
    assert steps > 100000 and near >= 0.01 * steps


def test_the_inside_case_holds_near_and_behind_voxels():
    """On the CPU: the camera-inside case has voxels with 0 < z < 0.1 m that project into the image
    and voxels behind the camera plane; the invalid-depth cases put invalid pixels over voxels
    with 0 < z <= trunc."""
    d = P.case("camera-inside")[0]
    H, W = d.shape[1:]
    u, v, z = P.projection("camera-inside", 0)
    inside = (np.rint(u) >= 0) & (np.rint(u) < W) & (np.rint(v) >= 0) & (np.rint(v) < H)
    assert int(((z > 0) & (z < 0.1) & inside).sum()) > 0 and int((z < 0).sum()) > 1000
    for name in ("invalid-depth", "invalid-depth-65535"):
        d = P.case(name)[0]
        px = []
        for f in range(len(d)):
            u, v, z = P.projection(name, f)
            ok = (z > 0) & (z <= 5 * P.VS) & (np.rint(u) >= 0) & (np.rint(u) < W) & (np.rint(v) >= 0) & (np.rint(v) < H)
            px.append(d[f][np.rint(v[ok]).astype(int), np.rint(u[ok]).astype(int)])
        px = np.concatenate(px)
        assert int((px == 0).sum()) > 50
        if name.endswith("65535"):
            assert int((px == 65535).sum()) > 50
