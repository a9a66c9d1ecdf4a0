"""NumPy restatement of the photometric term of the tracker (include/tsdf_hip.h):
the colour half of the RGB-D linearisation, the combined step and the RGB-D track, on top of
icp_ref's geometric half.  `linearize_color` follows the documented operation order in float32, so
its codes and residuals equal the kernel's bit for bit; its sums are exact (math.fsum over exact
products), returned with the sums of the terms' magnitudes.  Also the textured plane scene, on which
point-to-plane ICP alone is degenerate, shared by the CPU and GPU tests.
"""
import math

import numpy as np

import icp_ref as I
import raycast_ref as R

F32 = np.float32
COLOR_DEFAULTS = dict(color_weight=0.001, color_max_diff=40.0)


def intensity(rgb):
    """I = (77 R + 150 G + 29 B) >> 8 of an (H,W,3) uint8 image: an integer 0 .. 255 held in f32."""
    c = np.asarray(rgb)
    assert c.dtype == np.uint8 and c.ndim == 3 and c.shape[2] == 3
    c = c.astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]) >> 8).astype(F32)


def photo_texels(model_colors, model_depth):
    """The model's photo texels (Hm,Wm,4) f32: (I, Gx, Gy, D), central differences halved; a pixel
    on the border, or with a pixel without depth among itself and its 4-neighbours, is all zeros."""
    Im = intensity(model_colors)
    Dm = np.asarray(model_depth, dtype=F32)
    Hm, Wm = Dm.shape
    t = np.zeros((Hm, Wm, 4), F32)
    if Hm < 3 or Wm < 3:
        return t
    c = (slice(1, -1), slice(1, -1))
    valid = (Dm[c] > 0) & (Dm[1:-1, :-2] > 0) & (Dm[1:-1, 2:] > 0) & (Dm[:-2, 1:-1] > 0) & (Dm[2:, 1:-1] > 0)
    gx = (Im[1:-1, 2:] - Im[1:-1, :-2]) * F32(0.5)
    gy = (Im[2:, 1:-1] - Im[:-2, 1:-1]) * F32(0.5)
    inner = np.stack([Im[c], gx, gy, Dm[c]], axis=-1)
    t[1:-1, 1:-1] = np.where(valid[..., None], inner, F32(0))
    return t


def _lerp(a, b, t):
    return a + t * (b - a)


def linearize_color(depth, rgb, Kf, M, model_depth, model_colors, Km, *, dist_max=0.1, color_max_diff=40.0, stride=1,
                    invalid_65535=False, swap_gradient_focals=False, **_):
    """The colour half of one linearisation.  Returns a dict like icp_ref.linearize's: code (Hf,Wf)
    u8 (0 .. 5), resid (Hf,Wf) f32 (intensity levels; 0 where the code is not 5), sums / abs_sums
    (28,), inliers, candidates (codes 2 .. 5), and J (N,6) f32 / r (N,) f32 / p (N,3) f32 /
    g (N,3) f32 / If (N,) f32 (the frame's intensity) of the inliers in row-major pixel order.
    swap_gradient_focals is a deliberate fault for tests/test_cameras_cpu.py: the Jacobian line alone
    scales Gx by fym and Gy by fxm; the codes and residuals stay what they are."""
    d = I.depth_metres(depth, invalid_65535)
    Hf, Wf = d.shape
    If = intensity(rgb)
    assert If.shape == d.shape
    T = photo_texels(model_colors, model_depth)
    Hm, Wm = T.shape[:2]
    xf, yf = I.tables(Kf, (Hf, Wf))
    M32 = np.asarray(M, dtype=np.float64).reshape(4, 4).astype(F32)
    Km = np.asarray(Km, dtype=np.float64).reshape(3, 3)
    fxm, fym, cxm, cym = F32(Km[0, 0]), F32(Km[1, 1]), F32(Km[0, 2]), F32(Km[1, 2])
    dmax, cmax = F32(dist_max), F32(color_max_diff)

    vv, uu = np.meshgrid(np.arange(Hf), np.arange(Wf), indexing="ij")
    sampled = (uu % stride == 0) & (vv % stride == 0)
    with np.errstate(all="ignore"):
        alive = sampled & (d > 0) & np.isfinite(d)            # else code 0
        code = np.zeros((Hf, Wf), np.uint8)
        V = (xf[None, :] * d, yf[:, None] * d, d)
        p = [((M32[k, 0] * V[0] + M32[k, 1] * V[1]) + M32[k, 2] * V[2]) + M32[k, 3] for k in range(3)]
        x = fxm * (p[0] / p[2]) + cxm
        y = fym * (p[1] / p[2]) + cym
        x0, y0 = np.floor(x), np.floor(y)
        ok = ~(p[2] <= 0) & ((x0 >= 1) & (x0 <= F32(Wm - 3)) & (y0 >= 1) & (y0 <= F32(Hm - 3)))
        code[alive & ~ok] = 1
        alive &= ok
        xi = np.where(alive, x0, 1).astype(np.int64)
        yi = np.where(alive, y0, 1).astype(np.int64)
        xi, yi = np.clip(xi, 0, max(Wm - 2, 0)), np.clip(yi, 0, max(Hm - 2, 0))  # (dead pixels only)
        assert ((yi >= 0) & (yi + 1 < T.shape[0]) & (xi >= 0) & (xi + 1 < T.shape[1])).all()
        t00, t01, t10, t11 = T[yi, xi], T[yi, xi + 1], T[yi + 1, xi], T[yi + 1, xi + 1]
        ok = (t00[..., 3] > 0) & (t01[..., 3] > 0) & (t10[..., 3] > 0) & (t11[..., 3] > 0)
        code[alive & ~ok] = 2
        alive &= ok
        tx, ty = x - x0, y - y0
        Ib, Gx, Gy, Db = (_lerp(_lerp(t00[..., k], t01[..., k], tx), _lerp(t10[..., k], t11[..., k], tx), ty)
                          for k in range(4))
        ok = ~(np.abs(Db - p[2]) > dmax)
        code[alive & ~ok] = 3
        alive &= ok
        r = If - Ib
        ok = ~(np.abs(r) > cmax)
        code[alive & ~ok] = 4
        alive &= ok
        code[alive] = 5
        sx, sy = (fym, fxm) if swap_gradient_focals else (fxm, fym)
        a, b, iz = Gx * sx, Gy * sy, F32(1) / p[2]
        gx, gy = a * iz, b * iz
        g = (gx, gy, -((gx * p[0] + gy * p[1]) * iz))
        pxg = I._cross(p, g)
    resid = np.where(alive, r, F32(0)).astype(F32)
    J = np.stack([pxg[0][alive], pxg[1][alive], pxg[2][alive], g[0][alive], g[1][alive], g[2][alive]], axis=1).astype(F32)
    ri = r[alive].astype(F32)
    J64, r64 = J.astype(np.float64), ri.astype(np.float64)
    terms = [J64[:, i] * J64[:, j] for i, j in I.TRI] + [J64[:, i] * r64 for i in range(6)] + [r64 * r64]
    return {"code": code, "resid": resid,
            "sums": np.array([math.fsum(t) for t in terms]), "abs_sums": np.array([math.fsum(np.abs(t)) for t in terms]),
            "inliers": int(alive.sum()), "candidates": int((code >= 2).sum()),
            "J": J, "r": ri, "p": np.stack([q[alive] for q in p], axis=1), "g": np.stack([q[alive] for q in g], axis=1),
            "If": If[alive]}


def combine(sums_g, sums_c, color_weight):
    """A = A_g + lambda^2 A_c, b = b_g + lambda^2 b_c (and the same for sum r r), f64, lambda^2 in f64."""
    l2 = float(color_weight) * float(color_weight)
    return np.asarray(sums_g, dtype=np.float64) + l2 * np.asarray(sums_c, dtype=np.float64)


def track(depth, rgb, K, model_depth, model_normals, model_colors, pose_guess, *, color_weight=0.001, color_max_diff=40.0,
          invalid_65535=False, **params):
    """icp_ref.track with the colour term: per iteration both halves at M_i, the combined system,
    icp_ref.step (lost looks at the geometric inliers and the combined system's pivots).  Returns
    icp_ref.track's dict plus color_inliers [...], color_candidates [...]."""
    prm = dict(I.DEFAULTS, **params)
    M = np.eye(4)
    traj, inl, cin, ccand, status, cond = [M.copy()], [], [], [], None, float("nan")
    for it in range(prm["max_iter"]):
        lin = I.linearize(depth, K, M, model_depth, model_normals, K, pose_guess, invalid_65535=invalid_65535, **prm)
        col = linearize_color(depth, rgb, K, M, model_depth, model_colors, K, color_max_diff=color_max_diff,
                              invalid_65535=invalid_65535, **prm)
        inl.append(lin["inliers"])
        cin.append(col["inliers"])
        ccand.append(col["candidates"])
        sums = combine(lin["sums"], col["sums"], color_weight)
        M, status, _, _ = I.step(M, sums, lin["inliers"], **prm)
        traj.append(M.copy())
        if status is None or status == I.CONVERGED:
            cond = float(np.linalg.cond(I.system(sums)[0]))
        if status is not None:
            break
    return {"pose": np.asarray(pose_guess, dtype=np.float64).reshape(4, 4) @ M, "status": status or I.MAX_ITER,
            "iterations": len(inl), "trajectory": traj, "inliers": inl, "color_inliers": cin, "color_candidates": ccand,
            "cond": cond}


# ---- the textured plane scene ---------------------------------------------------------------------
# One plane fills the view: point-to-plane ICP cannot see the two in-plane translations and the
# rotation about the normal; the texture can.  Volume, cameras and sizes are the corner scene's.
PLANE_P0 = np.array([0.0, 0.0, 1.0])
PLANE_NRM = np.array([0.1, -0.05, -1.0]) / np.linalg.norm([0.1, -0.05, -1.0])
PLANE_E1 = np.cross(PLANE_NRM, [0.0, 1.0, 0.0]) / np.linalg.norm(np.cross(PLANE_NRM, [0.0, 1.0, 0.0]))
PLANE_E2 = np.cross(PLANE_NRM, PLANE_E1)
TRUE_POSE = np.eye(4)
START_SEED = 5
N_STARTS = 3


def texture(pts):
    """The grey level (f64, an integer 0 .. 255) at the points (..., 3): a function of their
    coordinates a, b along the plane's axes e1, e2."""
    a, b = pts @ PLANE_E1, pts @ PLANE_E2
    g = 128 + 50 * np.sin(9 * a + 1) * np.cos(7 * b) + 40 * np.sin(4 * b + 2.4 * a) + 20 * np.cos(15 * a - 11 * b)
    return np.rint(np.clip(g, 0, 255))


def plane_state():
    """(tsdf, weight, colour) of the plane volume: truncation 5 voxels, all weights 1 but for a carved
    band of weight-0 voxels (some model rays miss), the texture at the voxel centres as grey."""
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in I.SHAPE), indexing="ij")
    p = np.stack([x, y, z], axis=-1) * I.VS + I.ORIGIN.astype(np.float64)
    sdf = (p - PLANE_P0) @ PLANE_NRM
    t = np.clip(sdf / (5 * I.VS), -1.0, 1.0).astype(np.float32)
    w = np.ones(I.SHAPE, np.float32)
    w[22:25, :, :] = 0.0
    g = texture(p)
    c = (g * 65536 + g * 256 + g).astype(np.float32)
    return t, w, c


def plane_render(pose=TRUE_POSE, K=I.FRAME_K, hw=I.FRAME_HW, extras=False):
    """(depth u16 mm, rgb (H,W,3) u8 grey) of the plane seen from `pose`, analytic.  extras (the
    linearise tests): a rectangle of depth 0, a nearer occluding rectangle, and a rectangle brightened
    by 80 levels."""
    pose = np.asarray(pose, dtype=np.float64)
    v, u = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    dirs = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ pose[:3, :3].T
    den = dirs @ PLANE_NRM
    z = ((PLANE_P0 - pose[:3, 3]) @ PLANE_NRM) / np.where(den < 0, den, np.nan)
    z = np.where(z > 0, z, 0.0)
    grey = texture(pose[:3, 3] + dirs * z[..., None])
    mm = np.rint(z * 1000.0).astype(np.uint16)
    if extras:
        mm[6:15, 38:50] = 0
        mm[36:47, 8:20] = 700
        grey[30:42, 44:56] = np.minimum(grey[30:42, 44:56] + 80, 255)
    g8 = grey.astype(np.uint8)
    return mm, np.ascontiguousarray(np.stack([g8, g8, g8], axis=-1))


def plane_starts():
    rng = np.random.default_rng(START_SEED)
    return [TRUE_POSE @ I.perturbation(rng, 0.02, 1.0) for _ in range(N_STARTS)]


def plane_model(state=None, pose=np.eye(4), K=I.MODEL_K, hw=I.MODEL_HW):
    """(depth, normals, colours) of the reference raycast of the plane state."""
    t, w, c = plane_state() if state is None else state
    return R.raycast(t, w, c, I.ORIGIN, I.VS, K, pose, hw, 0.0, I.Z_FAR, I.VS)
