"""NumPy restatement of the tracking contract (include/tsdf_hip.h): frame-to-model
point-to-plane ICP.  `linearize` follows the documented operation order in float32, so its codes
and residuals equal the kernel's bit for bit; its sums are the exact sums (math.fsum over the f64
terms, each an exact product of two f32 values), returned with the sum of the terms' magnitudes so
that a test can bound what a different order of addition may change.  `step` solves and updates,
`track` iterates.  Also the corner scene shared by the CPU and GPU tests.
"""
import math

import numpy as np

import raycast_ref as R

F32 = np.float32
COS30 = math.cos(math.radians(30.0))
CONVERGED, MAX_ITER, LOST = "converged", "max_iter", "lost"
DEFAULTS = dict(dist_max=0.1, cos_min=COS30, stride=1, max_iter=10, min_inliers=100, eps_rot=1e-5, eps_trans=1e-5)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]  # the order of the 21 upper-triangle sums


def depth_metres(depth, invalid_65535=False):
    """Step 1: the frame's depth in f32 metres."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        mm = depth.astype(np.float64)
        if invalid_65535:
            mm[depth == 65535] = 0.0
        return (mm / 1000.0).astype(F32)
    with np.errstate(over="ignore"):
        return depth.astype(np.float64).astype(F32)


def tables(K, hw):
    """x_u = f32((u - cx) / fx), y_v = f32((v - cy) / fy): f64, one rounding."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    return (((np.arange(hw[1], dtype=np.float64) - K[0, 2]) / K[0, 0]).astype(F32),
            ((np.arange(hw[0], dtype=np.float64) - K[1, 2]) / K[1, 1]).astype(F32))


def _cross(a, b):
    """a x b, each component as a_y*b_z - a_z*b_y."""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def linearize(depth, Kf, M, model_depth, model_normals, Km, model_pose, *, dist_max=0.1, cos_min=COS30, stride=1,
              invalid_65535=False, **_):
    """One linearisation.  Returns a dict: code (Hf,Wf) u8, resid (Hf,Wf) f32, sums (28,) f64 exact,
    abs_sums (28,) the sums of |term|, inliers, candidates, and J (N,6) f32 / r (N,) f32 / p (N,3) f32 /
    n (N,3) f32 of the inliers in row-major pixel order."""
    d = depth_metres(depth, invalid_65535)
    Hf, Wf = d.shape
    Dm = np.asarray(model_depth, dtype=F32)
    Nm = np.asarray(model_normals, dtype=F32)
    Hm, Wm = Dm.shape
    xf, yf = tables(Kf, (Hf, Wf))
    xm, ym = tables(Km, (Hm, Wm))
    M32 = np.asarray(M, dtype=np.float64).reshape(4, 4).astype(F32)
    Rm = np.asarray(model_pose, dtype=np.float64).reshape(4, 4)[:3, :3].astype(F32)
    Km = np.asarray(Km, dtype=np.float64).reshape(3, 3)
    fxm, fym, cxm, cym = F32(Km[0, 0]), F32(Km[1, 1]), F32(Km[0, 2]), F32(Km[1, 2])
    dist2 = F32(dist_max) * F32(dist_max)
    cmin = F32(cos_min)

    code = np.zeros((Hf, Wf), np.uint8)
    resid = np.zeros((Hf, Wf), F32)
    vv, uu = np.meshgrid(np.arange(Hf - 1), np.arange(Wf - 1), indexing="ij")
    sampled = (uu % stride == 0) & (vv % stride == 0)
    d0, dr, dd = d[:-1, :-1], d[:-1, 1:], d[1:, :-1]

    def good(x):
        return (x > 0) & np.isfinite(x)

    with np.errstate(all="ignore"):
        alive = sampled & good(d0)                       # else code 0
        c = np.zeros((Hf - 1, Wf - 1), np.uint8)
        ok = good(dr) & good(dd)
        xu, xr = xf[:-1][None, :], xf[1:][None, :]
        yv, yd = yf[:-1][:, None], yf[1:][:, None]
        V = (xu * d0, yv * d0, d0)
        A = (xr * dr - V[0], yv * dr - V[1], dr - V[2])
        B = (xu * dd - V[0], yd * dd - V[1], dd - V[2])
        cr = _cross(B, A)
        l = np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
        ok &= ~(l == 0)
        c[alive & ~ok] = 1
        alive &= ok
        nf = (cr[0] / l, cr[1] / l, cr[2] / l)
        p = [((M32[k, 0] * V[0] + M32[k, 1] * V[1]) + M32[k, 2] * V[2]) + M32[k, 3] for k in range(3)]
        m = [(M32[k, 0] * nf[0] + M32[k, 1] * nf[1]) + M32[k, 2] * nf[2] for k in range(3)]
        uf = np.rint(fxm * (p[0] / p[2]) + cxm)
        vf = np.rint(fym * (p[1] / p[2]) + cym)
        ok = ~(p[2] <= 0) & ((uf >= 0) & (uf <= F32(Wm - 1)) & (vf >= 0) & (vf <= F32(Hm - 1)))
        c[alive & ~ok] = 2
        alive &= ok
        um = np.where(alive, uf, 0).astype(np.int64)
        vm = np.where(alive, vf, 0).astype(np.int64)
        assert ((vm >= 0) & (vm < Hm) & (um >= 0) & (um < Wm)).all()  # (every gather index in range, whatever M and K)
        dm = Dm[vm, um]
        nw = [Nm[vm, um, k] for k in range(3)]
        ok = (dm > 0) & ~((nw[0] == 0) & (nw[1] == 0) & (nw[2] == 0))
        c[alive & ~ok] = 3
        alive &= ok
        q = (xm[um] * dm, ym[vm] * dm, dm)
        n = [(Rm[0, k] * nw[0] + Rm[1, k] * nw[1]) + Rm[2, k] * nw[2] for k in range(3)]
        e = [q[k] - p[k] for k in range(3)]
        ok = ~((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > dist2)
        c[alive & ~ok] = 4
        alive &= ok
        ok = ~((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2] < cmin)
        c[alive & ~ok] = 5
        alive &= ok
        c[alive] = 6
        r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        pxn = _cross(p, n)
    code[:-1, :-1] = c
    resid[:-1, :-1] = np.where(alive, r, F32(0))
    J = np.stack([pxn[0][alive], pxn[1][alive], pxn[2][alive], n[0][alive], n[1][alive], n[2][alive]], axis=1).astype(F32)
    ri = r[alive].astype(F32)
    J64, r64 = J.astype(np.float64), ri.astype(np.float64)
    terms = [J64[:, i] * J64[:, j] for i, j in TRI] + [J64[:, i] * r64 for i in range(6)] + [r64 * r64]
    return {"code": code, "resid": resid,
            "sums": np.array([math.fsum(t) for t in terms]), "abs_sums": np.array([math.fsum(np.abs(t)) for t in terms]),
            "inliers": int(alive.sum()), "candidates": int((code >= 2).sum()),
            "J": J, "r": ri, "p": np.stack([x[alive] for x in p], axis=1), "n": np.stack([x[alive] for x in n], axis=1)}


def system(sums):
    """(A (6,6), b (6,)) from the 28 sums."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRI):
        A[i, j] = A[j, i] = sums[k]
    return A, np.asarray(sums[21:27], dtype=np.float64)


def se3(xi):
    """E(xi): Rodrigues' rotation of w = xi[:3] with translation t = xi[3:]."""
    w = np.asarray(xi[:3], dtype=np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    a, b = (math.sin(th) / th, (1.0 - math.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * Kx + b * (Kx @ Kx)
    E[:3, 3] = xi[3:6]
    return E


def step(M, sums, inliers, *, min_inliers=100, eps_rot=1e-5, eps_trans=1e-5, **_):
    """Solve A xi = b by Cholesky and update: (M', status or None, |w|, |t|).  Lost (fewer than
    min_inliers inliers, or A not positive definite) leaves M unchanged."""
    M = np.asarray(M, dtype=np.float64).reshape(4, 4)
    if inliers < min_inliers:
        return M.copy(), LOST, 0.0, 0.0
    A, b = system(sums)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return M.copy(), LOST, 0.0, 0.0
    xi = np.linalg.solve(L.T, np.linalg.solve(L, b))
    if not np.isfinite(xi).all():
        return M.copy(), LOST, 0.0, 0.0
    wn, tn = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
    return se3(xi) @ M, (CONVERGED if wn <= eps_rot and tn <= eps_trans else None), wn, tn


def track(depth, K, model_depth, model_normals, pose_guess, *, invalid_65535=False, **params):
    """Iterate from M_0 = I against the model maps of a raycast at pose_guess (same K and size as
    the frame).  Returns a dict: pose, status, iterations, trajectory [M_0, ...], inliers [...],
    cond (of the last solved system)."""
    prm = dict(DEFAULTS, **params)
    M = np.eye(4)
    traj, inl, status, cond = [M.copy()], [], None, float("nan")
    for it in range(prm["max_iter"]):
        lin = linearize(depth, K, M, model_depth, model_normals, K, pose_guess, invalid_65535=invalid_65535, **prm)
        inl.append(lin["inliers"])
        M, status, _, _ = step(M, lin["sums"], lin["inliers"], **prm)
        traj.append(M.copy())
        if status is None or status == CONVERGED:
            cond = float(np.linalg.cond(system(lin["sums"])[0]))
        if status is not None:
            break
    return {"pose": np.asarray(pose_guess, dtype=np.float64).reshape(4, 4) @ M, "status": status or MAX_ITER,
            "iterations": len(inl), "trajectory": traj, "inliers": inl, "cond": cond}


def pose_error(a, b):
    """(translation distance in metres, rotation angle in degrees) between two poses."""
    a, b = np.asarray(a, dtype=np.float64).reshape(4, 4), np.asarray(b, dtype=np.float64).reshape(4, 4)
    Rr = a[:3, :3].T @ b[:3, :3]
    # from the antisymmetric part: a pose read from a text file is orthonormal to ~1e-5 only, and
    # acos of the trace turns that into degrees near 0
    sk = 0.5 * np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])
    ang = math.degrees(math.atan2(float(np.linalg.norm(sk)), (np.trace(Rr) - 1.0) / 2.0))
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), ang


def perturbation(rng, trans, deg):
    """A rigid motion of `trans` metres and `deg` degrees about seeded random directions."""
    ax, t = rng.standard_normal(3), rng.standard_normal(3)
    E = se3(np.concatenate([ax / np.linalg.norm(ax) * math.radians(deg), t / np.linalg.norm(t) * trans]))
    return E


# ---- the corner scene ---------------------------------------------------------------------------
VS = 0.02
SHAPE = (64, 48, 40)
ORIGIN = np.array([-0.625, -0.5, 0.5], np.float32)  # (exact in f32)
BOUNDS = np.array([[-0.625, -0.625 + 63.5 * VS], [-0.5, -0.5 + 47.5 * VS], [0.5, 0.5 + 39.5 * VS]])  # ceil -> SHAPE
PLANE_N = np.array([[-1.0, 0.1, -0.15], [0.08, -1.0, -0.1], [0.12, 0.05, -1.0]])
PLANE_N /= np.linalg.norm(PLANE_N, axis=1, keepdims=True)
PLANE_P = np.array([[0.4, 0.0, 0.9], [0.0, 0.3, 0.9], [0.0, 0.0, 1.1]])
MODEL_HW = (61, 83)
MODEL_K = np.array([[101.3, 0.0, 41.2], [0.0, 101.3, 29.7], [0.0, 0.0, 1.0]])  # test_raycast_cpu.py's K
FRAME_HW = (53, 71)
FRAME_K = np.array([[88.0, 0.0, 35.0], [0.0, 88.0, 26.0], [0.0, 0.0, 1.0]])
Z_FAR = 2.0
TRUE_POSE = np.eye(4)
TRUE_POSE[:3, 3] = [0.01, -0.02, 0.03]
# The gates of the linearise tests on this scene: in a convex corner a 2 cm / 1 degree offset never
# separates a pair by the default 0.1 m, so the distance gate is set where it cuts (a condition on
# the inputs, like the holes: every code must occur at least 20 times).
CORNER_GATES = dict(dist_max=0.022, cos_min=COS30)


def corner_state():
    """tsdf = the clipped minimum of the three planes' signed distances (truncation 5 voxels), all
    weights 1 but for a carved band of weight-0 voxels (some model rays miss), random colours."""
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in SHAPE), indexing="ij")
    p = np.stack([x, y, z], axis=-1) * VS + ORIGIN.astype(np.float64)
    sdf = np.min([(p - PLANE_P[i]) @ PLANE_N[i] for i in range(3)], axis=0)
    t = np.clip(sdf / (5 * VS), -1.0, 1.0).astype(np.float32)
    w = np.ones(SHAPE, np.float32)
    w[22:25, :, :] = 0.0
    w[:, 14:16, 20:] = 0.0
    c = np.random.default_rng(3).integers(0, 1 << 24, size=SHAPE).astype(np.float32)
    return t, w, c


def render(pose, K, hw, holes=True):
    """The analytic depth image of the three planes from `pose`, rounded to millimetres (u16), with
    a rectangle of zeros and a few isolated zero pixels."""
    pose = np.asarray(pose, dtype=np.float64)
    v, u = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    dirs = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ pose[:3, :3].T
    z = np.full(hw, np.inf)
    for i in range(3):
        den = dirs @ PLANE_N[i]
        zi = ((PLANE_P[i] - pose[:3, 3]) @ PLANE_N[i]) / np.where(den < 0, den, np.nan)
        z = np.fmin(z, np.where(zi > 0, zi, np.inf))
    mm = np.rint(np.where(np.isfinite(z), z, 0.0) * 1000.0).astype(np.uint16)
    if holes:
        mm[8:20, 40:52] = 0
        mm[30:50:4, 5:30:6] = 0
    return mm


def offset_2cm_1deg():
    """The relative pose of the linearise tests: 2 cm and 1 degree."""
    return perturbation(np.random.default_rng(7), 0.02, 1.0)


def corner_model(state=None, pose=np.eye(4), K=MODEL_K, hw=MODEL_HW):
    """(depth, normals) of the reference raycast of the corner state."""
    t, w, c = corner_state() if state is None else state
    d, n, _ = R.raycast(t, w, c, ORIGIN, VS, K, pose, hw, 0.0, Z_FAR, VS)
    return d, n
