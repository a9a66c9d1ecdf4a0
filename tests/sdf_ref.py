"""NumPy restatement of the point-to-SDF alignment (include/tsdf_hip.h): a depth frame
aligned to the volume's own signed distance field, without a raycast.  `linearize` follows the
documented operation order in float32, so its codes and residuals equal the kernel's bit for bit;
its sums are the exact sums (math.fsum over f64 terms that are exact products of two f32 values),
returned with the sums of the terms' magnitudes.  `sample` is the cell alone at world points;
`track` iterates with icp_ref's `step`.  The cell's arithmetic is raycast_ref's.

Takes the (tsdf, weight) arrays of get_state(): C-order (X, Y, Z) float32.
"""
import math

import numpy as np

import icp_ref as I
import raycast_ref as R
from icp_ref import F32, TRI, _cross, depth_metres, pose_error, se3, step, tables  # noqa: F401

DEFAULTS = dict(dist_max=0.1, stride=1, max_iter=10, min_inliers=100, eps_rot=1e-5, eps_trans=1e-5)


def cell(tsdf, weight, q, index_offset=(0, 0, 0)):
    """Steps 3 - 5 for index-space points q (N, 3) f32: (code (N,) u8 in {2, 3, 4, 6}, f (N,) f32,
    g 3 x (N,) f32, i0 (N, 3) global cell indices); f and g are meaningful for codes 4 and 6."""
    q = np.asarray(q, dtype=F32)
    dims = np.array(tsdf.shape, dtype=np.int64)
    i0 = np.floor(R.clamp_index(q)).astype(np.int64)
    t = q - i0.astype(F32)
    l = i0 - np.asarray(index_offset, dtype=np.int64)
    inside = np.all((l >= 0) & (l <= dims - 2), axis=1)
    lc = np.clip(l, 0, np.maximum(dims - 2, 0))
    c, seen, flat = [], np.ones(len(q), bool), np.zeros(len(q), bool)
    for s in range(8):
        i = R.assert_in_range((lc[:, 0] + (s >> 2), lc[:, 1] + ((s >> 1) & 1), lc[:, 2] + (s & 1)), tsdf.shape)
        c.append(tsdf[i].astype(F32))
        seen &= weight[i] > 0
        flat |= np.abs(c[-1]) >= 1
    code = np.where(~inside, 2, np.where(~seen, 3, np.where(flat, 4, 6))).astype(np.uint8)
    with np.errstate(all="ignore"):
        f = R._trilinear(c, t)
        g = R._gradient(c, t)
    return code, f, g, i0


def geometry(origin, voxel_size, trunc, pose_guess):
    """The host side: f64, each value rounded to f32 once."""
    G = np.asarray(pose_guess, dtype=np.float64).reshape(4, 4)
    vs = np.float64(voxel_size)
    org = np.asarray(origin, dtype=np.float32).astype(np.float64)
    return ((G[:3, :3] / vs).astype(F32), ((G[:3, 3] - org) / vs).astype(F32), G[:3, :3].astype(F32),
            F32(np.float64(trunc) / vs), F32(trunc))


def linearize(depth, K, M, pose_guess, tsdf, weight, origin, voxel_size, trunc, *, dist_max=0.1, stride=1,
              invalid_65535=False, index_offset=(0, 0, 0), **_):
    """One linearisation.  Returns a dict: code (H,W) u8, resid (H,W) f32, sums (28,) f64 exact,
    abs_sums (28,), inliers, candidates, cell (H,W,3) the global cell index i0 of every pixel with a
    depth, and J (N,6) / r (N,) / p (N,3) / n (N,3) f32 of the inliers in row-major pixel order."""
    d = depth_metres(depth, invalid_65535)
    H, W = d.shape
    xf, yf = tables(K, (H, W))
    M32 = np.asarray(M, dtype=np.float64).reshape(4, 4).astype(F32)
    Qr, Qo, Rg, sc, tr = geometry(origin, voxel_size, trunc, pose_guess)
    dmax = F32(dist_max)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    code = np.zeros((H, W), np.uint8)
    resid = np.zeros((H, W), F32)
    with np.errstate(all="ignore"):
        alive = (uu % stride == 0) & (vv % stride == 0) & (d > 0) & np.isfinite(d)
        V = (xf[None, :] * d, yf[:, None] * d, d)
        p = [((M32[k, 0] * V[0] + M32[k, 1] * V[1]) + M32[k, 2] * V[2]) + M32[k, 3] for k in range(3)]
        q = np.stack([(((Qr[a, 0] * p[0] + Qr[a, 1] * p[1]) + Qr[a, 2] * p[2]) + Qo[a]) for a in range(3)], axis=-1)
        cc, f, g, i0 = cell(tsdf, weight, q.reshape(-1, 3), index_offset)
        cc, f = cc.reshape(H, W), f.reshape(H, W)
        g = [x.reshape(H, W) for x in g]
        r = -(tr * f)
        gate = (np.abs(r) > dmax) | ((g[0] == 0) & (g[1] == 0) & (g[2] == 0))
        cc = np.where((cc == 6) & gate, 5, cc).astype(np.uint8)
        n = [sc * ((Rg[0, i] * g[0] + Rg[1, i] * g[1]) + Rg[2, i] * g[2]) for i in range(3)]
        pxn = _cross(p, n)
    code[alive] = cc[alive]
    inl = code == 6
    resid[inl] = r[inl]
    J = np.stack([pxn[0][inl], pxn[1][inl], pxn[2][inl], n[0][inl], n[1][inl], n[2][inl]], axis=1).astype(F32)
    ri = r[inl].astype(F32)
    J64, r64 = J.astype(np.float64), ri.astype(np.float64)
    terms = [J64[:, i] * J64[:, j] for i, j in TRI] + [J64[:, i] * r64 for i in range(6)] + [r64 * r64]
    return {"code": code, "resid": resid,
            "sums": np.array([math.fsum(t) for t in terms]), "abs_sums": np.array([math.fsum(np.abs(t)) for t in terms]),
            "inliers": int(inl.sum()), "candidates": int((code >= 2).sum()), "cell": i0.reshape(H, W, 3),
            "J": J, "r": ri, "p": np.stack([x[inl] for x in p], axis=1), "n": np.stack([x[inl] for x in n], axis=1)}


def sample(points, tsdf, weight, origin, voxel_size, trunc, index_offset=(0, 0, 0)):
    """(sdf (N,) f32 metres, grad (N,3) f32, code (N,) u8) at world points (N,3) f64: value and
    gradient for codes 4 and 6, zeros otherwise."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    org = np.asarray(origin, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = ((P - org) / np.float64(voxel_size)).astype(F32)
        code, f, g, _ = cell(tsdf, weight, q, index_offset)
        sc, tr = F32(np.float64(trunc) / np.float64(voxel_size)), F32(trunc)
        ok = code >= 4
        sdf = np.where(ok, tr * f, F32(0)).astype(F32)
        grad = np.stack([np.where(ok, sc * x, F32(0)) for x in g], axis=1).astype(F32)
    return sdf, grad, code


def track(depth, K, pose_guess, tsdf, weight, origin, voxel_size, trunc, *, invalid_65535=False, **params):
    """Iterate from M_0 = I.  Returns icp_ref.track's dict."""
    prm = dict(DEFAULTS, **params)
    M = np.eye(4)
    traj, inl, status, cond = [M.copy()], [], None, float("nan")
    for _ in range(prm["max_iter"]):
        lin = linearize(depth, K, M, pose_guess, tsdf, weight, origin, voxel_size, trunc, invalid_65535=invalid_65535, **prm)
        inl.append(lin["inliers"])
        M, status, _, _ = step(M, lin["sums"], lin["inliers"], **prm)
        traj.append(M.copy())
        if status is None or status == I.CONVERGED:
            cond = float(np.linalg.cond(I.system(lin["sums"])[0]))
        if status is not None:
            break
    return {"pose": np.asarray(pose_guess, dtype=np.float64).reshape(4, 4) @ M, "status": status or I.MAX_ITER,
            "iterations": len(inl), "trajectory": traj, "inliers": inl, "cond": cond}


# ---- the every-code inputs on the corner state (a condition on the inputs, checked by the CPU test)
WIDE_K = np.array([[40.0, 0.0, 35.0], [0.0, 40.0, 26.0], [0.0, 0.0, 1.0]])
EVERY_CODE = dict(dist_max=0.06)


def every_code_case():
    """(frame u16, K, M, G): the corner seen through a wide camera from the identity, 8 cm / 3 degrees off."""
    return I.render(np.eye(4), WIDE_K, I.FRAME_HW), WIDE_K, I.perturbation(np.random.default_rng(5), 0.08, 3.0), np.eye(4)


CORNER_VOL = dict(origin=I.ORIGIN, voxel_size=I.VS, trunc=5 * I.VS)
