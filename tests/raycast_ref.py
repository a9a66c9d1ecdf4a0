"""NumPy restatement of the raycast contract (include/tsdf_hip.h), brute force over
every sample k and vectorised over the rays.  It follows the documented operation order, so in
float32 it equals the kernels bit for bit (hit mask, depth, colour; the normals' last steps are
compared within 1e-6); dtype=np.float64 runs the same march in f64 for the CPU checks.

Takes the (tsdf, weight, colour) arrays of get_state(): C-order (X, Y, Z) float32.
"""
import numpy as np


def _lerp(a, b, t):
    return a + t * (b - a)


def clamp_index(q):
    """q with the kernels' clamp before every float -> int conversion (floor_i, tsdf_cell.h):
    fminf(fmaxf(q, -1e9), 1e9), whose fmaxf drops a NaN -- so NaN becomes -1e9, far outside every
    volume -- and whose result always converts to an integer exactly."""
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(q), -1.0e9, np.clip(q, -1.0e9, 1.0e9))
    assert np.isfinite(c).all() and (np.abs(c) <= 1.0e9).all()
    return c


def assert_in_range(index, shape):
    """Every gather of the restatements goes through here: an index outside the array is what the
    kernel must not form either."""
    for i, n in zip(index, shape):
        assert ((i >= 0) & (i < n)).all(), (int(np.min(i)), int(np.max(i)), int(n))
    return index


def _cell(tsdf, weight, l, dims, dtype):
    """Corner values c[s] (s = dx*4 + dy*2 + dz) of the cells at local indices l (N, 3), and the
    cells' validity: 8 corners inside the volume, all with weight > 0."""
    inside = np.all((l >= 0) & (l <= dims - 2), axis=1)
    lc = np.clip(l, 0, np.maximum(dims - 2, 0))
    c, valid = [], inside.copy()
    for s in range(8):
        i = assert_in_range((lc[:, 0] + (s >> 2), lc[:, 1] + ((s >> 1) & 1), lc[:, 2] + (s & 1)), tsdf.shape)
        c.append(tsdf[i].astype(dtype))
        valid &= weight[i] > 0
    return c, valid


def _trilinear(c, t):
    c00, c01 = _lerp(c[0], c[1], t[:, 2]), _lerp(c[2], c[3], t[:, 2])
    c10, c11 = _lerp(c[4], c[5], t[:, 2]), _lerp(c[6], c[7], t[:, 2])
    return _lerp(_lerp(c00, c01, t[:, 1]), _lerp(c10, c11, t[:, 1]), t[:, 0])


def _gradient(c, t):
    gx = _lerp(_lerp(c[4] - c[0], c[5] - c[1], t[:, 2]), _lerp(c[6] - c[2], c[7] - c[3], t[:, 2]), t[:, 1])
    gy = _lerp(_lerp(c[2] - c[0], c[3] - c[1], t[:, 2]), _lerp(c[6] - c[4], c[7] - c[5], t[:, 2]), t[:, 0])
    gz = _lerp(_lerp(c[1] - c[0], c[3] - c[2], t[:, 1]), _lerp(c[5] - c[4], c[7] - c[6], t[:, 1]), t[:, 0])
    return gx, gy, gz


def decode_color(cv):
    """The fold B*65536 + G*256 + R back to (r, g, b) uint8, in float32 like the mesh's colours."""
    cv = cv.astype(np.float32)
    cb = np.floor(cv / np.float32(65536.0))
    cg = np.floor((cv - cb * np.float32(65536.0)) / np.float32(256.0))
    cr = cv - cb * np.float32(65536.0) - cg * np.float32(256.0)
    return np.stack([np.floor(x).astype(np.int32).astype(np.uint8) for x in (cr, cg, cb)], axis=-1)


def ray_setup(origin, voxel_size, cam_intr, cam_pose, hw, dtype=np.float32):
    """qo, qd (N, 3) of the H*W rays in index space: f64, rounded once to dtype."""
    H, W = hw
    K = np.asarray(cam_intr, dtype=np.float64).reshape(3, 3)
    P = np.asarray(cam_pose, dtype=np.float64).reshape(4, 4)
    vs = np.float64(voxel_size)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx = ((u - K[0, 2]) / K[0, 0]).reshape(-1)
    dy = ((v - K[1, 2]) / K[1, 1]).reshape(-1)
    org = np.asarray(origin, dtype=np.float32).astype(np.float64)
    qd = np.stack([((P[d, 0] * dx + P[d, 1] * dy) + P[d, 2]) / vs for d in range(3)], axis=1).astype(dtype)
    qo = np.stack([np.full(dx.shape, (P[d, 3] - org[d]) / vs) for d in range(3)], axis=1).astype(dtype)
    return qo, qd


def raycast(tsdf, weight, color, origin, voxel_size, cam_intr, cam_pose, hw, z_near, z_far, z_step, *,
            index_offset=(0, 0, 0), dtype=np.float32, info=False):
    """(depth (H,W) dtype, normals (H,W,3) dtype, colors (H,W,3) u8) [, info dict with the flat
    arrays hit, decided, k (the deciding sample) and cell (its local cell index)]."""
    H, W = hw
    N = H * W
    dims = np.array(tsdf.shape, dtype=np.int64)
    off = np.asarray(index_offset, dtype=np.int64)
    qo, qd = ray_setup(origin, voxel_size, cam_intr, cam_pose, hw, dtype)
    zn, zf, zs = dtype(z_near), dtype(z_far), dtype(z_step)

    def sample(idx, z):
        q = qo[idx] + qd[idx] * z[:, None] if np.ndim(z) else qo[idx] + qd[idx] * z
        i0 = np.floor(clamp_index(q)).astype(np.int64)
        t = q - i0.astype(dtype)
        return q, i0 - off, t

    depth = np.zeros(N, dtype)
    normals = np.zeros((N, 3), dtype)
    colors = np.zeros((N, 3), np.uint8)
    hit = np.zeros(N, bool)
    decided = np.zeros(N, bool)
    dec_k = np.full(N, -1, np.int64)
    dec_cell = np.zeros((N, 3), np.int64)
    prev_valid = np.zeros(N, bool)
    prev_f = np.zeros(N, dtype)
    k = 0
    while True:
        zk = zn + dtype(k) * zs
        if not zk <= zf:
            break
        idx = np.flatnonzero(~decided)
        if idx.size == 0:
            break
        _, l, t = sample(idx, zk)
        c, valid = _cell(tsdf, weight, l, dims, dtype)
        f = _trilinear(c, t)
        if k >= 1:
            dec = valid & (f < 0)
            di = idx[dec]
            decided[di] = True
            dec_k[di] = k
            dec_cell[di] = l[dec]
            h = dec & prev_valid[idx] & (prev_f[idx] > 0)
            hi = idx[h]
            if hi.size:
                hit[hi] = True
                f0, f1 = prev_f[hi], f[h]
                z0 = zn + dtype(k - 1) * zs
                zstar = z0 + zs * (f0 / (f0 - f1))
                depth[hi] = zstar
                q, ls, ts = sample(hi, zstar)
                rv = np.rint(clamp_index(q)).astype(np.int64) - off
                rv = np.clip(rv, 0, dims - 1)
                colors[hi] = decode_color(color[assert_in_range((rv[:, 0], rv[:, 1], rv[:, 2]), color.shape)])
                cs, vs_ = _cell(tsdf, weight, ls, dims, dtype)
                gx, gy, gz = _gradient(cs, ts)
                ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
                ok = vs_ & (ln > 0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    g = np.stack([gx / ln, gy / ln, gz / ln], axis=1)
                normals[hi[ok]] = g[ok]
        prev_valid[idx] = valid
        prev_f[idx] = f
        k += 1
    out = (depth.reshape(H, W), normals.reshape(H, W, 3), colors.reshape(H, W, 3))
    if info:
        return out + ({"hit": hit, "decided": decided, "k": dec_k, "cell": dec_cell},)
    return out


def live_bricks(tsdf, weight):
    """The live-brick rule: brick b (8^3 voxels) is live when some voxel of its 9^3 reach -- its
    own voxels plus the +1 layer the corners of its cells touch -- has weight > 0 and tsdf < 0."""
    neg = (weight > 0) & (tsdf < 0)
    for ax in range(3):
        n = neg.shape[ax]
        nb = (n + 7) // 8
        pad = [(0, 0)] * 3
        pad[ax] = (0, 8 * nb + 1 - n)
        p = np.moveaxis(np.pad(neg, pad), ax, 0)
        own = p[:8 * nb].reshape((nb, 8) + p.shape[1:]).any(axis=1)
        neg = np.moveaxis(own | p[8::8][:nb], 0, ax)
    return neg


# ---- states and poses shared by the CPU and GPU tests -------------------------------------------
def ragged_state(holes=True):
    """The ragged sphere of test_mesh_gpu.py::test_mesh_of_ragged_set_state_volume (63x45x37, exact
    zeros), with random weight-0 holes."""
    rng = np.random.default_rng(5)
    shape = (63, 45, 37)
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    t = np.clip((np.sqrt((x - 30.3) ** 2 + (y - 20.2) ** 2 + (z - 18.9) ** 2) - 14.0) / 4.0, -1, 1).astype(np.float32)
    t[::7, ::5, ::3] = 0.0
    c = rng.integers(0, 1 << 24, size=shape).astype(np.float32)
    w = np.ones(shape, np.float32)
    if holes:
        w[rng.random(shape) < 0.02] = 0.0
    return t, w, c


def ragged_poses():
    """Looking at the sphere along +z from outside the volume, and obliquely from a corner."""
    a = np.eye(4)
    a[:3, 3] = [0.3, 0.2, -0.35]
    f = np.array([0.3, 0.2, 0.19]) - np.array([-0.2, -0.15, -0.1])
    f /= np.linalg.norm(f)
    r = np.cross([0.0, 1.0, 0.0], f)
    r /= np.linalg.norm(r)
    b = np.eye(4)
    b[:3, 0], b[:3, 1], b[:3, 2], b[:3, 3] = r, np.cross(f, r), f, [-0.2, -0.15, -0.1]
    return [a, b]


def ellipsoid_state(shape, holes=True, seed=11):
    """An ellipsoid that nearly fills a volume of `shape` voxels, tsdf < 0 inside: its surface lies in
    the outermost brick of every axis, the partly filled last bricks of ragged dims included.  Exact
    zeros and (optionally) weight-0 holes as in ragged_state."""
    rng = np.random.default_rng(seed)
    c = (np.array(shape) - 1) / 2.0
    a = c - 2.0
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    rn = np.sqrt(((x - c[0]) / a[0]) ** 2 + ((y - c[1]) / a[1]) ** 2 + ((z - c[2]) / a[2]) ** 2)
    t = np.clip((rn - 1.0) * a.min() / 4.0, -1, 1).astype(np.float32)
    t[::7, ::5, ::3] = 0.0
    col = rng.integers(0, 1 << 24, size=shape).astype(np.float32)
    w = np.ones(shape, np.float32)
    if holes:
        w[rng.random(shape) < 0.02] = 0.0
    return t, w, col


def look_at(eye, target):
    """Camera-to-world pose at `eye` looking at `target` (camera z forward, x right, y down)."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    r = np.cross(up, f)
    r /= np.linalg.norm(r)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = r, np.cross(f, r), f, eye
    return p


def high_face_poses(lo, hi):
    """Poses outside the +x, +y and +z faces of the box [lo, hi] (metres), looking inward: the rays
    enter through a high face and move towards lower indices."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    out = {}
    for ax, name in enumerate("xyz"):
        eye = c + 0.013 * half.max() * np.array([1.0, -2.0, 1.5])
        eye[ax] = c[ax] + half[ax] + 0.75 * half.max()
        out["+" + name] = look_at(eye, c + 0.02 * half.max() * np.array([-1.0, 1.0, 2.0]))
    return out
