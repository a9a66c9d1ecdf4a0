#!/usr/bin/env python3
"""Tracking timing (tsdf_dense_track / tsdf_hash_track): 160 frames of the bench
trajectory fused into the bench's 512^3 @ 2 cm volume and its voxel hash (2^22 buckets), then 20
of the trajectory's 640 x 480 depth frames tracked, each from its predecessor's pose, with the depth
frame resident on the device.  Timed with the library's HIP events (tsdf_track_last_ms with
profiling on): the raycast at the guess, the setup, and the linearise and finish launches per
iteration run; the per-frame total is their sum plus the launches that fell through after a status
was set.  Dense and hash, stride 1 and 2.  The raycast alone (tsdf_*_raycast of depth and normals at
the same poses, the call a tracker built on the parent commit would make) is timed in the same run
with tsdf_raycast_last_ms: the march with current live bits, as inside a track here, and with
TSDF_RAY_REFLAG, as after every integrate of a track-and-fuse loop.

Method: the clock is warmed like bench.py's (300 ms of untimed tracks right before each
configuration's timed loop); every frame is tracked REPS times, a frame's figure is the median of
its repeats, and the report gives the median, minimum and maximum over the frames.  The poses found
are compared with the trajectory's own.  Prints one JSON object.
    PYTHONPATH=union-thesis-slam_amd python tools/gpu/track_time.py

--color measures the photometric term (tsdf_*_track_rgbd) instead of the strides: per
handle the geometric track and the RGB-D track at stride 1, alternately configured in the same run
on the same build, the frames' RGB images resident on the device; the RGB-D figures add the prep
launch (tsdf_track_last_prep_ms), which is part of the total.

--sdf measures the point-to-SDF alignment (tsdf_*_track_sdf) against the ICP: per handle
and stride the ICP track and the SDF track, alternately configured in the same run on the same build
(icp, sdf, icp_again, sdf_again at stride 1, then icp and sdf at stride 2).  An SDF track queues no
raycast, so its raycast figure is 0 and "raycast alone" does not apply to it."""
import argparse
import contextlib
import ctypes
import io
import json
import math
import sys
import time

import numpy as np
import torch

from tsdf_amd import _ffi, grid_fusion, hash_fusion, scene, tracking

FRAMES, TRACKED, FIRST, REPS, HW = 160, 20, 120, 3, (480, 640)
ROOM, VOXEL = 10.24, 0.02


def pose_error(a, b):
    r = a[:3, :3].T @ b[:3, :3]
    sk = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), math.degrees(math.atan2(np.linalg.norm(sk), (np.trace(r) - 1) / 2))


def summary(v, scale=1e3, digits=1):
    return {"median": round(scale * float(np.median(v)), digits), "min": round(scale * min(v), digits),
            "max": round(scale * max(v), digits)}


def time_config(obj, name, K, poses, depth, stride, z_far, maps, preheat_s=0.3, rgb=None, method="icp"):
    """rgb: the frames' RGB8 images on the device -- then the RGB-D track is timed (the prep launch
    as a sixth figure), else the geometric one (prep 0).  method "sdf": the SDF track."""
    Kp = _ffi.ptr(_ffi.f64(K, 9))
    prm = tracking.icp_params(stride=stride)
    cprm, cinfo = tracking.color_params(), _ffi.TrackColorInfo()
    out, info = np.zeros(16), _ffi.TrackInfo()

    def track(f):
        head = (obj._h, depth[f].data_ptr(), _ffi.DEPTH_U16_MM)
        cam = (HW[0], HW[1], Kp, _ffi.ptr(_ffi.f64(poses[f - 1], 16)), ctypes.byref(prm))
        prep = ctypes.c_double(0.0)
        if method == "sdf":
            _ffi.call(f"tsdf_{name}_track_sdf", *head, *cam, _ffi.ptr(out), ctypes.byref(info), None, _ffi.DEVICE_PTRS)
        elif rgb is None:
            _ffi.call(f"tsdf_{name}_track", *head, *cam, 0.0, z_far, VOXEL, _ffi.ptr(out), ctypes.byref(info), None,
                      _ffi.DEVICE_PTRS)
        else:
            _ffi.call(f"tsdf_{name}_track_rgbd", *head, rgb[f].data_ptr(), *cam, ctypes.byref(cprm), 0.0, z_far, VOXEL,
                      _ffi.ptr(out), ctypes.byref(info), ctypes.byref(cinfo), None, _ffi.DEVICE_PTRS)
            _ffi.call("tsdf_track_last_prep_ms", ctypes.byref(prep))
        ms, it = (ctypes.c_double * 5)(), ctypes.c_int()
        _ffi.call("tsdf_track_last_ms", ms, ctypes.byref(it))
        return list(ms) + [prep.value], it.value

    def cast(f, flags):
        _ffi.call(f"tsdf_{name}_raycast", obj._h, HW[0], HW[1], Kp, _ffi.ptr(_ffi.f64(poses[f - 1], 16)), 0.0, z_far,
                  VOXEL, maps[0].data_ptr(), maps[1].data_ptr(), None, _ffi.DEVICE_PTRS | flags)
        a, b = ctypes.c_double(), ctypes.c_double()
        _ffi.call("tsdf_raycast_last_ms", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    frames = range(FIRST, FIRST + TRACKED)
    t_end = time.perf_counter() + preheat_s
    i = 0
    while time.perf_counter() < t_end:
        track(FIRST + i % TRACKED)
        i += 1
    cols = {k: [] for k in ("raycast", "setup", "linearize_per_iter", "finish_per_iter", "fall_through", "total",
                            "raycast_share", "prep")}
    iters, status, inliers, c_inliers, err_t, err_r, start_t, start_r = [], [], [], [], [], [], [], []
    for f in frames:
        r = [track(f) for _ in range(REPS)]
        it = r[0][1]
        med = [float(np.median([x[0][k] for x in r])) for k in range(6)]
        total = sum(med)
        cols["prep"].append(med[5])
        c_inliers.append(cinfo.color_inliers)
        cols["raycast"].append(med[0])
        cols["setup"].append(med[1])
        cols["linearize_per_iter"].append(med[2] / max(it, 1))
        cols["finish_per_iter"].append(med[3] / max(it, 1))
        cols["fall_through"].append(med[4])
        cols["total"].append(total)
        cols["raycast_share"].append(med[0] / total)
        iters.append(it)
        status.append(_ffi.TRACK_STATUS.get(info.status, str(info.status)))
        inliers.append(info.inliers)
        e = pose_error(out.reshape(4, 4), poses[f])
        s = pose_error(poses[f - 1], poses[f])
        err_t.append(e[0]); err_r.append(e[1]); start_t.append(s[0]); start_r.append(s[1])  # noqa: E702
    alone, alone_live = [], []
    for f in frames if method != "sdf" else ():
        alone.append(float(np.median([cast(f, 0)[1] for _ in range(REPS)])))
        alone_live.append(float(np.median([sum(cast(f, _ffi.RAY_REFLAG)) for _ in range(REPS)])))
    res = {k + "_us": summary(v) for k, v in cols.items() if k != "raycast_share"}
    res["raycast_share_of_total"] = summary(cols["raycast_share"], 1.0, 3)
    if method != "sdf":
        res["raycast_alone_us"] = summary(alone)
        res["raycast_alone_with_live_pass_us"] = summary(alone_live)
    res["iterations"] = {"median": float(np.median(iters)), "min": min(iters), "max": max(iters)}
    res["status"] = {s: status.count(s) for s in sorted(set(status))}
    res["inliers"] = {"median": float(np.median(inliers)), "min": int(min(inliers)), "max": int(max(inliers))}
    if rgb is not None:
        res["color_inliers"] = {"median": float(np.median(c_inliers)), "min": int(min(c_inliers)), "max": int(max(c_inliers))}
    res["start_error"] = {"mm": summary(start_t, 1e3, 2), "deg": summary(start_r, 1.0, 3)}
    res["final_error"] = {"mm": summary(err_t, 1e3, 2), "deg": summary(err_r, 1.0, 3)}
    res["warmup_tracks"] = i
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--color", action="store_true", help="geometric against RGB-D track at stride 1 (see above)")
    ap.add_argument("--sdf", action="store_true", help="ICP against SDF track at stride 1 and 2 (see above)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    poses = scene.trajectory(FRAMES, seed=0, radius_frac=scene.BENCH_RING)
    sph = scene.make_spheres(0, ring_frac=scene.BENCH_RING)
    depth = torch.empty((FRAMES,) + HW, dtype=torch.int16, device=dev)
    rgb = torch.empty((FRAMES,) + HW + (3,), dtype=torch.uint8, device=dev)
    for s in range(0, FRAMES, 40):
        d, c = scene.render(poses[s:s + 40], sph, seed=0, start=s, device=dev, depth_dtype=torch.int16)
        depth[s:s + len(d)] = d
        rgb[s:s + len(c)] = c
    K = scene.intrinsics()
    Tinv = np.ascontiguousarray(np.linalg.inv(poses))
    maps = (torch.zeros(HW, dtype=torch.float32, device=dev), torch.zeros(HW + (3,), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    z_far = ROOM * 3 ** 0.5
    res = {"build_id": _ffi.build_id(), "frames_fused": FRAMES, "image": list(HW), "frames_tracked": TRACKED,
           "first_frame": FIRST, "reps": REPS, "z_step": VOXEL, "z_far": round(z_far, 3), "max_iter": 10,
           "units": "microseconds unless named"}
    for name in ("dense", "hash"):
        bnds = np.array([[0.0, ROOM]] * 3)
        with contextlib.redirect_stdout(io.StringIO()):
            obj = (grid_fusion.TSDFVolume(bnds, VOXEL) if name == "dense" else
                   hash_fusion.HashTable(bnds, VOXEL, 1 << 22, max_blocks=1 << 15))
        obj.integrate_batch(depth.data_ptr(), rgb.data_ptr(), K, Tinv, hw=HW, device_ptrs=True)
        obj.set_profiling(True)
        configs = ([("stride1", 1, None), ("stride2", 2, None)] if not args.color else
                   [("geometry", 1, None), ("rgbd", 1, rgb), ("geometry_again", 1, None), ("rgbd_again", 1, rgb)])
        if args.sdf:
            configs = [("icp_stride1", 1, None), ("sdf_stride1", 1, None), ("icp_stride1_again", 1, None),
                       ("sdf_stride1_again", 1, None), ("icp_stride2", 2, None), ("sdf_stride2", 2, None)]
        for label, stride, images in configs:
            r = time_config(obj, name, K, poses, depth, stride, z_far, maps, rgb=images,
                            method="sdf" if label.startswith("sdf") else "icp")
            res[f"{name}_{label}"] = r
            print(name, label, json.dumps(r), file=sys.stderr, flush=True)
        obj.close()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
