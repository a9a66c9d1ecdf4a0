"""Camera tracking against the fused model (not in the reference, whose poses come
from files): frame-to-model point-to-plane ICP on the device.

  * `TSDFVolume.track` / `HashTable.track` (through `track_call`): the pose of a depth frame, given
    a guess -- the raycast at the guess, all iterations and the pose updates run on the handle's
    stream with one synchronisation at the end (tsdf_dense_track / tsdf_hash_track).
  * `icp_linearize`: one linearisation against model maps the caller holds (tsdf_icp_linearize),
    for tests and for trackers that keep their own loop.
  * With a colour image (`track(color_im=...)`, `icp_linearize_rgbd`) a photometric term joins the
    geometric one: it observes the motions a single plane leaves free.
  * `track(method="sdf")`, `sdf_linearize` and `TSDFVolume.sample` / `HashTable.sample` (through
    `sample_call`): point-to-SDF alignment on the volume itself -- no raycast, no
    model maps, no frame normals.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _ffi
from .grid_fusion import default_z_far, encode_depth


def icp_params(dist_max=0.1, angle_max_deg=30.0, stride=1, max_iter=10, min_inliers=100, eps_rot=1e-5, eps_trans=1e-5,
               cos_min=None):
    """tsdf_icp_params_t from the wrappers' keywords (cos_min, when given, replaces angle_max_deg)."""
    c = math.cos(math.radians(float(angle_max_deg))) if cos_min is None else float(cos_min)
    return _ffi.IcpParams(float(dist_max), c, int(stride), int(max_iter), int(min_inliers), float(eps_rot),
                          float(eps_trans))


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _device_image(x, name, shape, dtypes, device):
    """The address of a CUDA tensor the kernels may read or write as a (shape) image of one of
    `dtypes` on `device`; anything else is a ValueError (as raycast's out= tensors)."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in dtypes and tuple(x.shape) == tuple(shape)
            and x.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of shape {tuple(shape)} and dtype in {dtypes}")
    if x.device.index != device:
        raise ValueError(f"{name} lives on {x.device}, the call runs on device {device}")
    return x.data_ptr()


def _depth_tensor_kind(t):
    import torch
    kinds = {torch.int16: _ffi.DEPTH_U16_MM, torch.float64: _ffi.DEPTH_F64_M}
    if hasattr(torch, "uint16"):
        kinds[torch.uint16] = _ffi.DEPTH_U16_MM
    if not (isinstance(t, torch.Tensor) and t.dtype in kinds and t.dim() == 2):
        raise ValueError("a device depth frame must be a 2-d CUDA tensor of int16 / uint16 millimetres or float64 metres")
    return kinds[t.dtype], tuple(kinds)


COLOR_WEIGHT, COLOR_MAX_DIFF = 0.001, 40.0  # the wrappers' defaults of the photometric term


def color_params(color_weight=COLOR_WEIGHT, color_max_diff=COLOR_MAX_DIFF):
    """tsdf_icp_color_params_t from the wrappers' keywords."""
    return _ffi.IcpColorParams(float(color_weight), float(color_max_diff))


def _color_image(color_im, name, hw, like_tensor, device):
    """The address of an (H,W,3) uint8 image: a CUDA tensor read in place when the depth frame is
    one, else a NumPy array (returned as well, to keep it alive).  Anything else is a ValueError."""
    if like_tensor:
        import torch
        if not _is_tensor(color_im):
            raise ValueError(f"{name} must be a CUDA tensor when the depth frame is one")
        return _device_image(color_im, name, tuple(hw) + (3,), (torch.uint8,), device), color_im
    if _is_tensor(color_im):
        raise ValueError(f"{name} is a tensor but the depth frame is an array: pass both alike")
    c = np.asarray(color_im)
    if c.dtype != np.uint8 or c.shape != tuple(hw) + (3,):
        raise ValueError(f"{name} must be an (H,W,3) uint8 image of the depth frame's size {tuple(hw)}, "
                         f"got {c.dtype} {c.shape}")
    c = np.ascontiguousarray(c)
    return _ffi.ptr(c), c


def track_call(fn, handle, vol_bnds, voxel_size, depth_im, cam_intr, pose_guess, dist_max, angle_max_deg, stride,
               max_iter, min_inliers, eps_rot, eps_trans, z_near, z_far, z_step, return_info, invalid_65535=False,
               color_im=None, color_weight=COLOR_WEIGHT, color_max_diff=COLOR_MAX_DIFF, method="icp"):
    """The track entry points' host side (tsdf_dense_track / tsdf_hash_track, with color_im the
    _rgbd ones, with method="sdf" the _sdf ones, which take no z range): defaults, the depth frame
    through encode_depth (or a CUDA tensor read in place), the result as arrays."""
    if method not in ("icp", "sdf"):
        raise ValueError(f"method must be 'icp' or 'sdf', got {method!r}")
    sdf = method == "sdf"
    if sdf and color_im is not None:
        raise ValueError("method='sdf' takes no color_im: the photometric term belongs to the ICP")
    pose = _ffi.f64(pose_guess, 16)
    K = _ffi.f64(cam_intr, 9)
    if z_step is None:
        z_step = float(voxel_size)
    if z_far is None and not sdf:
        z_far = default_z_far(vol_bnds, pose, z_near)
    prm = icp_params(dist_max, angle_max_deg, stride, max_iter, min_inliers, eps_rot, eps_trans)
    flags = _ffi.DEPTH_INVALID_65535 if invalid_65535 else 0
    if _is_tensor(depth_im):
        dk, dtypes = _depth_tensor_kind(depth_im)
        H, W = depth_im.shape
        dptr = _device_image(depth_im, "depth_im", (H, W), dtypes, depth_im.device.index)
        flags |= _ffi.DEVICE_PTRS
        import torch
        torch.cuda.synchronize(depth_im.device)  # the handle's stream does not follow torch's
    else:
        dk, d = encode_depth(depth_im)
        if d.ndim != 2:
            raise ValueError("depth_im must be a 2-d image")
        H, W = d.shape
        dptr = _ffi.ptr(d)
    out = np.empty(16, np.float64)
    info = _ffi.TrackInfo()
    n_traj = max(int(max_iter), 0) + 1
    traj = np.zeros((n_traj, 4, 4), np.float64) if return_info else None
    cinfo = None
    if sdf:
        _ffi.call(fn + "_sdf", handle, dptr, dk, int(H), int(W), _ffi.ptr(K), _ffi.ptr(pose), ctypes.byref(prm),
                  _ffi.ptr(out), ctypes.byref(info), _ffi.ptr(traj), flags)
    elif color_im is None:
        _ffi.call(fn, handle, dptr, dk, int(H), int(W), _ffi.ptr(K), _ffi.ptr(pose), ctypes.byref(prm), float(z_near),
                  float(z_far), float(z_step), _ffi.ptr(out), ctypes.byref(info), _ffi.ptr(traj), flags)
    else:
        is_t = _is_tensor(depth_im)
        cptr, keep = _color_image(color_im, "color_im", (H, W), is_t, depth_im.device.index if is_t else None)
        cprm, cinfo = color_params(color_weight, color_max_diff), _ffi.TrackColorInfo()
        _ffi.call(fn + "_rgbd", handle, dptr, dk, cptr, int(H), int(W), _ffi.ptr(K), _ffi.ptr(pose), ctypes.byref(prm),
                  ctypes.byref(cprm), float(z_near), float(z_far), float(z_step), _ffi.ptr(out), ctypes.byref(info),
                  ctypes.byref(cinfo), _ffi.ptr(traj), flags)
        del keep
    out = out.reshape(4, 4)
    if not return_info:
        return out
    res = info.as_dict()
    if cinfo is not None:
        res.update(cinfo.as_dict())
    res["status"] = _ffi.TRACK_STATUS.get(info.status, str(info.status))
    res["trajectory"] = traj[:info.iterations + 1].copy()
    return out, res


def icp_linearize(depth, frame_intr, rel_pose, model_depth, model_normals, model_intr, model_pose, *, dist_max=0.1,
                  angle_max_deg=30.0, cos_min=None, stride=1, codes=True, residuals=True, invalid_65535=False,
                  device=0):
    """One linearisation of the point-to-plane ICP (tsdf_icp_linearize) of the depth
    frame (Hf,Wf; uint16 mm or metres) seen through frame_intr at rel_pose (frame camera to model
    camera) against model_depth (Hm,Wm) f32 / model_normals (Hm,Wm,3) f32, the maps of a raycast at
    model_pose through model_intr.  The images are NumPy arrays, or all contiguous CUDA tensors on
    `device` (then the code / residual maps come back as CUDA tensors too).  Returns a dict: sums
    (28,) f64 -- the 21 upper-triangle entries of sum J_i J_j, the 6 of sum J_i r, sum r^2 --,
    inliers, candidates, A (6,6), b (6,), code (Hf,Wf) u8 and residual (Hf,Wf) f32 (None when not
    asked for)."""
    Kf, Km = _ffi.f64(frame_intr, 9), _ffi.f64(model_intr, 9)
    M, P = _ffi.f64(rel_pose, 16), _ffi.f64(model_pose, 16)
    prm = icp_params(dist_max, angle_max_deg, stride, cos_min=cos_min)
    flags = _ffi.DEPTH_INVALID_65535 if invalid_65535 else 0
    tensors = [_is_tensor(x) for x in (depth, model_depth, model_normals)]
    if any(tensors):
        import torch
        if not all(tensors):
            raise ValueError("depth, model_depth and model_normals must be all CUDA tensors or all arrays")
        dk, dtypes = _depth_tensor_kind(depth)
        Hf, Wf = depth.shape
        if model_depth.dim() != 2:
            raise ValueError("model_depth must be a 2-d CUDA tensor")
        Hm, Wm = model_depth.shape
        dptr = _device_image(depth, "depth", (Hf, Wf), dtypes, device)
        mptr = _device_image(model_depth, "model_depth", (Hm, Wm), (torch.float32,), device)
        nptr = _device_image(model_normals, "model_normals", (Hm, Wm, 3), (torch.float32,), device)
        dev = torch.device("cuda", device)
        code = torch.zeros((Hf, Wf), dtype=torch.uint8, device=dev) if codes else None
        res = torch.zeros((Hf, Wf), dtype=torch.float32, device=dev) if residuals else None
        cptr = None if code is None else code.data_ptr()
        rptr = None if res is None else res.data_ptr()
        torch.cuda.synchronize(dev)  # the call runs on a stream of its own
        flags |= _ffi.DEVICE_PTRS
    else:
        dk, d = encode_depth(depth)
        md = np.ascontiguousarray(model_depth, dtype=np.float32)
        mn = np.ascontiguousarray(model_normals, dtype=np.float32)
        if d.ndim != 2 or md.ndim != 2 or mn.shape != md.shape + (3,):
            raise ValueError("depth (Hf,Wf), model_depth (Hm,Wm) and model_normals (Hm,Wm,3) expected")
        (Hf, Wf), (Hm, Wm) = d.shape, md.shape
        code = np.zeros((Hf, Wf), np.uint8) if codes else None
        res = np.zeros((Hf, Wf), np.float32) if residuals else None
        dptr, mptr, nptr, cptr, rptr = (_ffi.ptr(x) for x in (d, md, mn, code, res))
    sums = np.zeros(28, np.float64)
    counts = np.zeros(2, np.int64)
    _ffi.call("tsdf_icp_linearize", int(device), dptr, dk, int(Hf), int(Wf), _ffi.ptr(Kf), _ffi.ptr(M), mptr, nptr,
              int(Hm), int(Wm), _ffi.ptr(Km), _ffi.ptr(P), ctypes.byref(prm), _ffi.ptr(sums), _ffi.ptr(counts), cptr,
              rptr, flags)
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    return {"sums": sums, "inliers": int(counts[0]), "candidates": int(counts[1]), "A": A, "b": sums[21:27].copy(),
            "code": code, "residual": res}


def icp_linearize_rgbd(depth, color, frame_intr, rel_pose, model_depth, model_normals, model_colors, model_intr,
                       model_pose, *, dist_max=0.1, angle_max_deg=30.0, cos_min=None, stride=1,
                       color_weight=COLOR_WEIGHT, color_max_diff=COLOR_MAX_DIFF, codes=True, residuals=True,
                       invalid_65535=False, device=0):
    """One RGB-D linearisation (tsdf_icp_linearize_rgbd): icp_linearize's geometric
    half -- the same bytes -- and the photometric half in the same pass.  color (Hf,Wf,3) uint8 is
    the frame's image, model_colors (Hm,Wm,3) uint8 the raycast's colour map; all images are NumPy
    arrays or all contiguous CUDA tensors on `device`.  Returns icp_linearize's dict (sums (28,), A, b,
    inliers, candidates, code, residual: the geometry) plus color_sums (28,), color_A, color_b,
    color_inliers, color_candidates, color_code (Hf,Wf) u8 (0 .. 5) and color_residual (Hf,Wf) f32
    in intensity levels.  color_weight is validated and otherwise unused here: the sums are not
    scaled."""
    Kf, Km = _ffi.f64(frame_intr, 9), _ffi.f64(model_intr, 9)
    M, P = _ffi.f64(rel_pose, 16), _ffi.f64(model_pose, 16)
    prm = icp_params(dist_max, angle_max_deg, stride, cos_min=cos_min)
    cprm = color_params(color_weight, color_max_diff)
    flags = _ffi.DEPTH_INVALID_65535 if invalid_65535 else 0
    images = (depth, color, model_depth, model_normals, model_colors)
    tensors = [_is_tensor(x) for x in images]
    if any(tensors):
        import torch
        if not all(tensors):
            raise ValueError("depth, color and the three model maps must be all CUDA tensors or all arrays")
        dk, dtypes = _depth_tensor_kind(depth)
        Hf, Wf = depth.shape
        if model_depth.dim() != 2:
            raise ValueError("model_depth must be a 2-d CUDA tensor")
        Hm, Wm = model_depth.shape
        dptr = _device_image(depth, "depth", (Hf, Wf), dtypes, device)
        cptr = _device_image(color, "color", (Hf, Wf, 3), (torch.uint8,), device)
        mptr = _device_image(model_depth, "model_depth", (Hm, Wm), (torch.float32,), device)
        nptr = _device_image(model_normals, "model_normals", (Hm, Wm, 3), (torch.float32,), device)
        mcptr = _device_image(model_colors, "model_colors", (Hm, Wm, 3), (torch.uint8,), device)
        dev = torch.device("cuda", device)
        outs = [torch.zeros((Hf, Wf), dtype=t, device=dev) if on else None
                for t, on in ((torch.uint8, codes), (torch.float32, residuals)) * 2]
        optr = [None if o is None else o.data_ptr() for o in outs]
        torch.cuda.synchronize(dev)  # the call runs on a stream of its own
        flags |= _ffi.DEVICE_PTRS
    else:
        dk, d = encode_depth(depth)
        md = np.ascontiguousarray(model_depth, dtype=np.float32)
        mn = np.ascontiguousarray(model_normals, dtype=np.float32)
        if d.ndim != 2 or md.ndim != 2 or mn.shape != md.shape + (3,):
            raise ValueError("depth (Hf,Wf), model_depth (Hm,Wm) and model_normals (Hm,Wm,3) expected")
        (Hf, Wf), (Hm, Wm) = d.shape, md.shape
        cptr, c = _color_image(color, "color", (Hf, Wf), False, None)
        mcptr, mc = _color_image(model_colors, "model_colors", (Hm, Wm), False, None)
        outs = [np.zeros((Hf, Wf), t) if on else None for t, on in ((np.uint8, codes), (np.float32, residuals)) * 2]
        dptr, mptr, nptr = (_ffi.ptr(x) for x in (d, md, mn))
        optr = [_ffi.ptr(o) for o in outs]
    sums = np.zeros(56, np.float64)
    counts = np.zeros(4, np.int64)
    _ffi.call("tsdf_icp_linearize_rgbd", int(device), dptr, dk, cptr, int(Hf), int(Wf), _ffi.ptr(Kf), _ffi.ptr(M), mptr, nptr,
              mcptr, int(Hm), int(Wm), _ffi.ptr(Km), _ffi.ptr(P), ctypes.byref(prm), ctypes.byref(cprm), _ffi.ptr(sums),
              _ffi.ptr(counts), *optr, flags)

    def system(v):
        A = np.zeros((6, 6))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                A[i, j] = A[j, i] = v[k]
                k += 1
        return A, v[21:27].copy()

    (A, b), (Ac, bc) = system(sums[:28]), system(sums[28:])
    return {"sums": sums[:28].copy(), "inliers": int(counts[0]), "candidates": int(counts[1]), "A": A, "b": b,
            "code": outs[0], "residual": outs[1], "color_sums": sums[28:].copy(), "color_inliers": int(counts[2]),
            "color_candidates": int(counts[3]), "color_A": Ac, "color_b": bc, "color_code": outs[2],
            "color_residual": outs[3]}


def sdf_linearize(obj, depth, cam_intr, rel_pose, pose_guess, *, dist_max=0.1, stride=1, codes=True, residuals=True,
                  invalid_65535=False):
    """One linearisation of the point-to-SDF alignment (tsdf_dense_sdf_linearize /
    tsdf_hash_sdf_linearize) of the depth frame (H,W; uint16 mm or metres) seen through
    cam_intr at rel_pose (frame camera to the guess camera's frame) against the volume of obj (a
    TSDFVolume or a HashTable) at pose_guess (camera-to-world).  depth is a NumPy array, or a
    contiguous CUDA tensor on the handle's device (then the code / residual maps come back as CUDA
    tensors too).  Returns icp_linearize's dict; the codes are 0 not sampled or no depth, 2 cell
    outside the volume, 3 a corner never observed, 4 a corner on the truncated plateau, 5 further
    than dist_max or no gradient, 6 inlier."""
    K, M, G = _ffi.f64(cam_intr, 9), _ffi.f64(rel_pose, 16), _ffi.f64(pose_guess, 16)
    prm = icp_params(dist_max, stride=stride)
    flags = _ffi.DEPTH_INVALID_65535 if invalid_65535 else 0
    if _is_tensor(depth):
        import torch
        dk, dtypes = _depth_tensor_kind(depth)
        H, W = depth.shape
        dptr = _device_image(depth, "depth", (H, W), dtypes, obj.device)
        dev = torch.device("cuda", obj.device)
        code = torch.zeros((H, W), dtype=torch.uint8, device=dev) if codes else None
        res = torch.zeros((H, W), dtype=torch.float32, device=dev) if residuals else None
        cptr = None if code is None else code.data_ptr()
        rptr = None if res is None else res.data_ptr()
        torch.cuda.synchronize(dev)  # the handle's stream does not follow torch's
        flags |= _ffi.DEVICE_PTRS
    else:
        dk, d = encode_depth(depth)
        if d.ndim != 2:
            raise ValueError("depth must be a 2-d image")
        H, W = d.shape
        code = np.zeros((H, W), np.uint8) if codes else None
        res = np.zeros((H, W), np.float32) if residuals else None
        dptr, cptr, rptr = (_ffi.ptr(x) for x in (d, code, res))
    sums = np.zeros(28, np.float64)
    counts = np.zeros(2, np.int64)
    fn = "tsdf_hash_sdf_linearize" if type(obj).__name__ == "HashTable" else "tsdf_dense_sdf_linearize"
    _ffi.call(fn, obj._h, dptr, dk, int(H), int(W), _ffi.ptr(K), _ffi.ptr(M), _ffi.ptr(G), ctypes.byref(prm),
              _ffi.ptr(sums), _ffi.ptr(counts), cptr, rptr, flags)
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    return {"sums": sums, "inliers": int(counts[0]), "candidates": int(counts[1]), "A": A, "b": sums[21:27].copy(),
            "code": code, "residual": res}


def sample_call(fn, handle, device, points):
    """The sample entry points' host side (tsdf_dense_sample / tsdf_hash_sample): (sdf (N,) f32 metres,
    grad (N,3) f32, code (N,) u8) at world points (N,3) -- NumPy arrays for an array, CUDA tensors for a
    contiguous float64 CUDA tensor on the handle's device (anything else raises ValueError)."""
    if _is_tensor(points):
        import torch
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be (N, 3)")
        n = int(points.shape[0])
        pptr = _device_image(points, "points", (n, 3), (torch.float64,), device)
        dev = torch.device("cuda", device)
        out = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev),
               torch.zeros(n, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)  # the handle's stream does not follow torch's
        _ffi.call(fn, handle, pptr, n, *[o.data_ptr() for o in out], _ffi.DEVICE_PTRS)
        return out
    P = np.ascontiguousarray(points, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    n = P.shape[0]
    out = (np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8))
    _ffi.call(fn, handle, _ffi.ptr(P), n, *[_ffi.ptr(o) for o in out], 0)
    return out
