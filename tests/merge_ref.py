"""NumPy restatement of the volume merge: one fused volume sampled into another under a
rigid transform, operation by operation in float32 -- the kernel (csrc/tsdf_merge.hip) is matched
against it byte for byte.  Volumes are dense C-order arrays; a hash is its get_volume() plus the
entry mask (a voxel without an entry holds (1, 0, 0)).  Also the cases the tests share.
"""
import math

import numpy as np

import icp_ref

F32 = np.float32
OUTSIDE, UNSEEN, SAMPLE = 2, 3, 6


class Geo:
    """A volume's lattice: dims and global index offset of the (shard's) array, f32 origin, voxel
    size and truncation."""

    def __init__(self, dims, origin, vs, trunc=None, off=(0, 0, 0)):
        self.dims = tuple(int(d) for d in dims)
        self.origin = np.asarray(origin, F32)
        self.vs = float(vs)
        self.trunc = 5 * self.vs if trunc is None else float(trunc)
        self.off = tuple(int(o) for o in off)

    def bounds(self):
        """vol_bnds of the unsharded volume for the Python classes (dims = ceil(extent / vs))."""
        lo = self.origin.astype(np.float64)
        return np.stack([lo, lo + (np.asarray(self.dims) - 0.5) * self.vs], axis=1)

    def slab(self, x0, x1):
        return Geo((x1 - x0,) + self.dims[1:], self.origin, self.vs, self.trunc, (self.off[0] + x0,) + self.off[1:])


def constants(dst, src, T):
    """A (3x3), b (3), rho as f32, from f64 (each value rounded once); three-term sums (a + b) + c."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    s = dst.vs / src.vs
    d = dst.origin.astype(np.float64) - t
    A = np.empty((3, 3), F32)
    b = np.empty(3, F32)
    for k in range(3):
        for j in range(3):
            A[k, j] = F32(R[j, k] * s)
        b[k] = F32((((R[0, k] * d[0] + R[1, k] * d[1]) + R[2, k] * d[2]) - float(src.origin[k])) / src.vs)
    return A, b, F32(src.trunc / dst.trunc)


def lerp(a, b, t):
    return a + t * (b - a)


def trilinear(c, f):
    """tsdf_cell.h: lerp z, then y, then x; c[dx*4 + dy*2 + dz]."""
    c00, c01 = lerp(c[0], c[1], f[2]), lerp(c[2], c[3], f[2])
    c10, c11 = lerp(c[4], c[5], f[2]), lerp(c[6], c[7], f[2])
    return lerp(lerp(c00, c01, f[1]), lerp(c10, c11, f[1]), f[0])


def decode(c):
    """The exact update path's floor formulas (csrc/tsdf_device.h): b, g, r of a folded colour."""
    b = np.floor(c / F32(65536.0))
    g = np.floor((c - b * F32(65536.0)) / F32(256.0))
    r = c - b * F32(65536.0) - g * F32(256.0)
    return b, g, r


def sample(dst, src, s_t, s_w, s_c, T):
    """Rules 1-4 for every destination voxel: code map, n_degenerate map, and u, w_S, colour where
    the code is SAMPLE (elsewhere 0)."""
    A, b, rho = constants(dst, src, T)
    g = [np.arange(dst.off[k], dst.off[k] + dst.dims[k]).astype(F32) for k in range(3)]
    x, y, z = np.meshgrid(*g, indexing="ij")
    i0, f, n = [], [], []
    for k in range(3):
        q = ((A[k, 0] * x + A[k, 1] * y) + A[k, 2] * z) + b[k]
        assert q.dtype == F32
        fl = np.floor(np.clip(q, F32(-1.0e9), F32(1.0e9)))
        i0.append(fl.astype(np.int64) - src.off[k])  # S's local index
        f.append(q - fl)
        n.append((f[k] > 0).astype(np.int64))
    code = np.full(dst.dims, SAMPLE, np.uint8)
    inside = np.ones(dst.dims, bool)
    for k in range(3):
        inside &= (i0[k] >= 0) & (i0[k] + n[k] <= src.dims[k] - 1)
    code[~inside] = OUTSIDE
    ndeg = sum((f[k] == 0).astype(np.int64) for k in range(3))
    m = inside
    l = [i0[k][m] for k in range(3)]
    nn = [n[k][m] for k in range(3)]
    ff = [f[k][m] for k in range(3)]
    c, w = [], []
    for s in range(8):
        dx, dy, dz = s >> 2, (s >> 1) & 1, s & 1
        idx = (l[0] + dx * nn[0], l[1] + dy * nn[1], l[2] + dz * nn[2])
        assert all(((i >= 0) & (i < d)).all() for i, d in zip(idx, s_t.shape))  # (every gather index in range)
        c.append(s_t[idx])
        w.append(s_w[idx])
    seen = np.ones(len(l[0]), bool)
    for s in range(8):
        seen &= w[s] > 0
    v = trilinear(c, ff)
    u = np.minimum(F32(1.0), np.maximum(F32(-1.0), rho * v))
    assert u.dtype == F32
    w_s = w[0]
    for s in range(1, 8):
        w_s = np.minimum(w_s, w[s])
    col = s_c[tuple(l[k] + (ff[k] >= F32(0.5)).astype(np.int64) for k in range(3))]
    sub = code[m]
    sub[~seen] = UNSEEN
    code[m] = sub
    out = {}
    for name, val in (("u", u), ("w", w_s), ("c", col), ("rv", rho * v)):
        a = np.zeros(dst.dims, F32)
        a[m] = np.where(seen, val, F32(0.0))
        out[name] = a
    return code, ndeg, out


def merge(dst, d_t, d_w, d_c, src, s_t, s_w, s_c, T, d_mask=None):
    """The merged destination (tsdf, weight, colour[, entry mask]), the code map and the info counts.
    d_mask: a hash destination's entry mask (its unset voxels hold (1, 0, 0))."""
    d_t, d_w, d_c = (np.array(a, F32) for a in (d_t, d_w, d_c))
    s_t, s_w, s_c = (np.asarray(a, F32) for a in (s_t, s_w, s_c))
    code, ndeg, smp = sample(dst, src, s_t, s_w, s_c, T)
    m = code == SAMPLE
    wd, td, cd = d_w[m], d_t[m], d_c[m]
    ws, u, cs = smp["w"][m], smp["u"][m], smp["c"][m]
    wn = wd + ws
    tn = (((wd * td).astype(np.float64) + (ws * u).astype(np.float64)) / wn.astype(np.float64)).astype(F32)
    ob, og, orr = decode(cd)
    nb, ng, nr = decode(cs)
    cb = np.minimum(F32(255.0), np.rint((wd * ob + ws * nb) / wn))
    cg = np.minimum(F32(255.0), np.rint((wd * og + ws * ng) / wn))
    cr = np.minimum(F32(255.0), np.rint((wd * orr + ws * nr) / wn))
    cn = cb * F32(65536.0) + cg * F32(256.0) + cr
    assert tn.dtype == F32 and cn.dtype == F32 and wn.dtype == F32
    d_t[m], d_w[m], d_c[m] = tn, wn, cn
    nbk = tuple((d + 7) // 8 for d in dst.dims)
    pad = np.zeros(tuple(8 * k for k in nbk), bool)

    def bricks(mask):
        p = pad.copy()
        p[:dst.dims[0], :dst.dims[1], :dst.dims[2]] = mask
        return p.reshape(nbk[0], 8, nbk[1], 8, nbk[2], 8).any(axis=(1, 3, 5))

    upd = bricks(m)
    info = {"samples": int(m.sum()), "bricks_updated": int(upd.sum()), "blocks_allocated": 0}
    res = {"tsdf": d_t, "weight": d_w, "color": d_c, "code": code, "ndeg": ndeg, "info": info, "sample": smp}
    if d_mask is not None:
        had = bricks(d_mask)
        mask = d_mask | m
        info["blocks_allocated"] = int((upd & ~had).sum())
        res["mask"] = mask
        res["used"] = int(bricks(mask).sum())
        res["entries"] = int(mask.sum())
    return res


def empty(geo):
    return np.ones(geo.dims, F32), np.zeros(geo.dims, F32), np.zeros(geo.dims, F32)


def prefilled(geo, seed=11):
    """A seeded destination: half of the bricks hold integer weights 0..5, tsdf uniform in (-1, 1) and
    canonical colours; the rest (1, 0, 0).  Returns (tsdf, weight, colour, entry mask): within a
    filled brick about three quarters of the voxels have an entry (the hash's partial occupancy)."""
    rng = np.random.default_rng(seed)
    nbk = tuple((d + 7) // 8 for d in geo.dims)
    full = tuple(8 * k for k in nbk)
    bm = rng.random(nbk) < 0.5
    vox = np.repeat(np.repeat(np.repeat(bm, 8, 0), 8, 1), 8, 2)
    vox &= rng.random(full) < 0.75
    vox = vox[:geo.dims[0], :geo.dims[1], :geo.dims[2]]
    t = rng.uniform(-1.0, 1.0, geo.dims).astype(F32)
    t = np.clip(t, F32(-0.999), F32(0.999))
    w = rng.integers(0, 6, geo.dims).astype(F32)
    c = rng.integers(0, 1 << 24, geo.dims).astype(F32)
    t, w, c = np.where(vox, t, F32(1.0)), np.where(vox, w, F32(0.0)), np.where(vox, c, F32(0.0))
    return t, w, c, vox


# ---- the cases ------------------------------------------------------------------------------------
SRC = Geo(icp_ref.SHAPE, icp_ref.ORIGIN, icp_ref.VS)
E = icp_ref.se3([0.10, -0.17, 0.12, 0.05, -0.03, 0.04])


def translation(x, y, z):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def quarter_turn(x):
    """A 90 degree turn about z (exact entries) and a shift along x: the z axis stays on the lattice
    (degenerate), x and y land between the source's voxels -- exactly one degenerate axis."""
    T = translation(x, 0.0, 0.0)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    return T


# name -> (destination lattice, T, (outside, unseen, samples) of the CPU prototype or None)
CASES = {
    "ident": (SRC, np.eye(4), (0, 8200, 114680)),
    "shift": (SRC, translation(0.06, -0.04, 0.10), (24670, 6570, 91640)),
    "half": (SRC, translation(0.01, 0.0, 0.0), (1920, 10040, 110920)),
    "rot": (Geo((48, 40, 32), (-0.4, -0.35, 0.55), 0.02), E, (11342, 5602, 44496)),
    "big": (Geo((96, 72, 64), (-0.9, -0.7, 0.3), 0.02), E, (326915, 10870, 104583)),
    "fine": (Geo((56, 48, 40), (-0.3, -0.3, 0.6), 0.01, trunc=0.05), E, (12, 15154, 92354)),
    # beyond the prototype's six: one degenerate axis, and extents that are no multiple of the brick
    "turn": (SRC, quarter_turn(0.01), None),
    "odd": (Geo((45, 38, 29), (-0.4, -0.35, 0.55), 0.02), E, None),
}


def counts(code):
    return tuple(int((code == k).sum()) for k in (OUTSIDE, UNSEEN, SAMPLE))


_state = None


def source_state():
    """icp_ref.corner_state(), computed once and shared (read-only)."""
    global _state
    if _state is None:
        _state = icp_ref.corner_state()
        for a in _state:
            a.setflags(write=False)
    return _state


_results = {}


def case_result(name, filled=False):
    """merge() of a case into an empty (or the seeded pre-filled) destination, computed once."""
    key = (name, filled)
    if key not in _results:
        dst, T, _ = CASES[name]
        d = prefilled(dst) if filled else empty(dst) + (np.zeros(dst.dims, bool),)
        _results[key] = (d, merge(dst, d[0], d[1], d[2], SRC, *source_state(), T, d_mask=d[3]))
    return _results[key]


def rigid(seed, trans, deg):
    return icp_ref.perturbation(np.random.default_rng(seed), trans, deg)


def check_transform(T):
    """The refusal rule for T: finite, last row 0 0 0 1, R orthonormal with det +1 to 1e-6."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    if not np.isfinite(T).all() or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        return False
    R = T[:3, :3]
    return bool(np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6)


assert math.isclose(SRC.trunc, 0.1)


# ---- what the method reaches: two lounge submaps joined, against the map of all their frames ------
LOUNGE_VS = 0.04
LOUNGE_G_SEED = 5


def lounge_maps(G, bounds, load_lounge, intrinsics):
    """Oracle maps at 4 cm: A of frames 0-4, B of frames 5-9 in a world moved by G (poses G^-1 pose),
    C of all ten in A's lattice.  The fixture holds colour images of frames 0-2 only: frame i takes
    the image of frame i % 3 (the comparison is of tsdf and weight).  Returns (geo, A, B, C), each map
    (tsdf, weight, colour)."""
    import oracle as O
    K = intrinsics()
    vols = [O.OracleTSDFVolume(np.array(bounds, dtype=np.float64), LOUNGE_VS) for _ in range(3)]
    Ginv = np.linalg.inv(G)
    rgbs = [load_lounge(i)[2] for i in range(3)]
    for i in range(10):
        _, depth, _, pose = load_lounge(i, color=False)
        rgb = rgbs[i % 3]
        if i < 5:
            vols[0].integrate(rgb, depth, K, pose)
        else:
            vols[1].integrate(rgb, depth, K, Ginv @ pose)
        vols[2].integrate(rgb, depth, K, pose)
    geo = Geo(vols[0]._vol_dim, vols[0]._vol_origin, LOUNGE_VS)
    return (geo,) + tuple((v._tsdf_vol_cpu, v._weight_vol_cpu, v._color_vol_cpu) for v in vols)


def lounge_compare(geo, A, B, C, G):
    """Merge B into A under G and compare with C over the voxels observed in both with |tsdf_C| < 1:
    (n, weights equal, max |dtsdf|, mean, 95th percentile and max |dtsdf| * trunc in millimetres)."""
    r = merge(geo, *A, geo, *B, G)
    m = (r["weight"] > 0) & (C[1] > 0) & (np.abs(C[0]) < 1) & (r["code"] == SAMPLE)
    d = np.abs(r["tsdf"][m].astype(np.float64) - C[0][m].astype(np.float64))
    return {"n": int(m.sum()), "weights_equal": bool(np.array_equal(r["weight"][m], C[1][m])),
            "max_dt": float(d.max()), "mean_mm": float(d.mean() * geo.trunc * 1000.0),
            "p95_mm": float(np.percentile(d, 95) * geo.trunc * 1000.0), "max_mm": float(d.max() * geo.trunc * 1000.0)}
