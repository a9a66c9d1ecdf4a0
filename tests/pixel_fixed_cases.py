"""Inputs of the fixed-point pixel tests (test_pixel_fixed_cpu.py, test_pixel_fixed_gpu.py): small
frames and poses on a 64^3 @ 4 cm volume that put the integrate's pixel path (project_part,
csrc/tsdf_device.h) where it can go wrong, and the oracle's result for each.  Plain functions only;
everything here runs on the CPU."""
import functools

import numpy as np

import oracle as O

VS = 0.04
N = 64
MODES = ("dense-texel0", "dense-texel1", "hash")


def bounds():
    return np.array([[0.0, N * VS]] * 3)


def look(eye, yaw=0.0, pitch=0.0, roll=0.0):
    """Camera-to-world pose at `eye`, optical axis +z turned by yaw (about y), pitch (x), roll (z)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx @ Rz
    T[:3, 3] = eye
    return T


def intr(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def images(rng, F, H, W, lo_mm, hi_mm):
    """Smooth-ish depth in millimetres with per-pixel noise (so a wrong pixel shows) and random colour."""
    base = rng.integers(lo_mm, hi_mm, size=(F, 1 + H // 8, 1 + W // 8))
    d = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :H, :W] + rng.integers(0, 40, size=(F, H, W))
    return np.ascontiguousarray(d.astype(np.uint16)), rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """(depth u16 (F,H,W), rgb (F,H,W,3), K, poses (F,4,4), invalid_65535)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = N * VS / 2
    if name == "camera-inside":
        # the camera sits inside the volume: kept bricks hold voxels with 0 < z < the fast path's
        # depth limit (about 0.16 m with the aliasing term) and voxels behind the camera plane
        poses = np.stack([look([c + 0.013 * f, c - 0.021 * f, 0.9 + 0.017 * f], 0.3 * f - 1.0, 0.1 * f - 0.3, 0.05 * f)
                          for f in range(8)])
        d, rgb = images(rng, 8, 480, 640, 150, 1600)
        return d, rgb, intr(525.0, 525.0, 319.5, 239.5), poses, False
    if name in ("small-97x61", "small-100x61"):
        # an off-grid C, an off-centre principal point, most projections outside on both sides
        W = 97 if name == "small-97x61" else 100
        # (u in [0, W) needs x/z in [0.45, 1.5], v in [0, 61) needs y/z in [-1.8, -1.3])
        poses = np.stack([look([c - 2.0 + 0.05 * f, c + 3.0 - 0.04 * f, c - 2.0 - 0.03 * f], 0.02 * f - 0.06, 0.05 - 0.015 * f, 0.01 * f)
                          for f in range(8)])
        d, rgb = images(rng, 8, 61, W, 600, 3200)
        return d, rgb, intr(90.0, 110.0, np.float32(-40.3), np.float32(200.7)), poses, False
    if name == "oversized-40000x2":
        # an image side above 16384: every step takes the exact path
        poses = np.stack([look([c, c, -1.0 - 0.05 * f], 0.02 * f, 0.0, 0.0) for f in range(2)])
        d, rgb = images(rng, 2, 2, 40000, 900, 3400)
        return d, rgb, intr(18000.0, 40.0, 19999.5, 0.5), poses, False
    if name == "boundary-hits":
        # the voxel grid aligned with the optical axis at integer-pixel spacing: camera-space
        # x = (i + 0.5) * VS, z = n * VS, so u - cx = 240 (2i + 1) / n is an integer -- a rounding
        # boundary with cx = 319.5 -- on every plane whose n divides 240 and on many voxels elsewhere
        eye = np.array([32 * VS, 32 * VS, -20 * VS]) - 0.5 * VS * np.array([1, 1, 0])
        poses = np.stack([look(eye - np.array([0, 0, 4 * VS * f])) for f in range(4)])
        d, rgb = images(rng, 4, 480, 640, 1000, 4200)
        return d, rgb, intr(480.0, 480.0, 319.5, 239.5), poses, False
    if name in ("invalid-depth", "invalid-depth-65535"):
        # zero-depth (and, masked, 65535) pixels over voxels with 0 < z <= trunc = 0.2 m -- the
        # only place a depth > 0 test decides anything: depth 0 passes depth - z >= -trunc there
        poses = np.stack([look([c + 0.01 * f, c, 0.5 + 0.02 * f], 0.2 * f - 0.6, 0.1 * f, 0.0) for f in range(6)])
        d, rgb = images(rng, 6, 480, 640, 100, 1500)
        hole = rng.random(d.shape) < 0.35
        d[hole] = 0
        d[:, 200:280, 280:360] = 0  # a solid hole on the optical axis
        if name.endswith("65535"):
            d[rng.random(d.shape) < 0.2] = 65535
            d[:, 100:180, 280:360] = 65535
        return d, rgb, intr(525.0, 525.0, 319.5, 239.5), poses, name.endswith("65535")
    raise KeyError(name)


CASES = ("camera-inside", "small-97x61", "small-100x61", "oversized-40000x2", "boundary-hits", "invalid-depth",
         "invalid-depth-65535")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's (tsdf, weight, colour, voxel updates), computed once and left unchanged."""
    d, rgb, K, poses, inv = case(name)
    orc = O.OracleTSDFVolume(bounds(), VS)
    n = 0
    for f in range(len(d)):
        dm = d[f].astype(float) / 1000.0
        if inv:
            dm[dm == 65.535] = 0
        n += orc.integrate(rgb[f], dm, K, poses[f])
    out = (orc._tsdf_vol_cpu, orc._weight_vol_cpu, orc._color_vol_cpu)
    for a in out:
        a.setflags(write=False)
    return out + (n,)



def projection(name, f):
    """The reference's unrounded pixel (u, v) and depth z of every voxel for frame f (the NumPy
    port's arithmetic, oracle._numpy_project)."""
    d, rgb, K, poses, _ = case(name)
    idx = O.vox_coords_for((N, N, N))
    o = np.zeros(3, np.float32).astype(np.float64)
    pts = (o[None, :] + VS * idx.astype(np.float32).astype(np.float64)).astype(np.float32)
    cam = np.dot(np.linalg.inv(poses[f]), np.hstack([pts, np.ones((len(pts), 1), np.float32)]).T).T[:, :3]
    k = K.astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (cam[:, 0] * k[0, 0]) / cam[:, 2] + k[0, 2], (cam[:, 1] * k[1, 1]) / cam[:, 2] + k[1, 2], cam[:, 2]


