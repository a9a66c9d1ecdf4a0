#!/usr/bin/env python3
"""Raycast timing (tsdf_dense_raycast / tsdf_hash_raycast): 160 frames of the bench
trajectory fused into the bench's 512^3 @ 2 cm volume and its voxel hash (2^22 buckets), then
640 x 480 raycasts from 20 of the trajectory's poses into device buffers, timed with the library's
HIP events (tsdf_raycast_last_ms with profiling on): the live-bit pass and the march separately,
dense and hash, with the skip (TSDF_RAY_SKIP=1, the default) and without (0: every sample).

Method: the clock is warmed like bench.py's (300 ms of untimed raycasts right before each
configuration's timed loop); every pose is cast REPS times with TSDF_RAY_REFLAG, so each call runs
the live-bit pass too; a pose's figure is the median of its repeats, and the report gives the median,
minimum and maximum over the poses.  Prints one JSON object.
    PYTHONPATH=union-thesis-slam_amd python tools/gpu/raycast_time.py"""
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

from tsdf_amd import _ffi, grid_fusion, hash_fusion, scene

FRAMES, POSES, REPS, HW = 160, 20, 5, (480, 640)
ROOM, VOXEL = 10.24, 0.02


def last_ms():
    a, b = ctypes.c_double(), ctypes.c_double()
    _ffi.call("tsdf_raycast_last_ms", ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def time_config(obj, fn, K, poses, out, z_far, preheat_s=0.3):
    Kp = _ffi.ptr(_ffi.f64(K, 9))
    ptrs = [o.data_ptr() for o in out]

    def cast(pose, flags):
        _ffi.call(fn, obj._h, HW[0], HW[1], Kp, _ffi.ptr(_ffi.f64(pose, 16)), 0.0, z_far, VOXEL, *ptrs,
                  _ffi.DEVICE_PTRS | flags)

    t_end = time.perf_counter() + preheat_s
    i = 0
    while time.perf_counter() < t_end:
        cast(poses[i % len(poses)], 0)
        i += 1
    live, march, hits = [], [], []
    for pose in poses:
        r = []
        for _ in range(REPS):
            cast(pose, _ffi.RAY_REFLAG)
            r.append(last_ms())
        live.append(float(np.median([x[0] for x in r])))
        march.append(float(np.median([x[1] for x in r])))
        hits.append(int((out[0] != 0).sum().item()))

    def summary(v):
        return {"median_us": round(1e3 * float(np.median(v)), 1), "min_us": round(1e3 * min(v), 1),
                "max_us": round(1e3 * max(v), 1)}

    return {"live_pass": summary(live), "march": summary(march),
            "hit_fraction": round(float(np.mean(hits)) / (HW[0] * HW[1]), 3), "warmup_casts": i}


def main():
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
    out = (torch.zeros(HW, dtype=torch.float32, device=dev), torch.zeros(HW + (3,), dtype=torch.float32, device=dev),
           torch.zeros(HW + (3,), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    views = [poses[i] for i in range(0, FRAMES, FRAMES // POSES)]
    z_far = ROOM * 3 ** 0.5
    res = {"build_id": _ffi.build_id(), "frames_fused": FRAMES, "image": list(HW), "poses": len(views), "reps": REPS,
           "z_step": VOXEL, "z_far": round(z_far, 3)}
    for skip in ("1", "0"):
        os.environ["TSDF_RAY_SKIP"] = skip  # (read when a handle is created)
        for name in ("dense", "hash"):
            bnds = np.array([[0.0, ROOM]] * 3)
            with contextlib.redirect_stdout(io.StringIO()):
                obj = (grid_fusion.TSDFVolume(bnds, VOXEL) if name == "dense" else
                       hash_fusion.HashTable(bnds, VOXEL, 1 << 22, max_blocks=1 << 15))
            obj.integrate_batch(depth.data_ptr(), rgb.data_ptr(), K, Tinv, hw=HW, device_ptrs=True)
            obj.set_profiling(True)
            r = time_config(obj, f"tsdf_{name}_raycast", K, views, out, z_far)
            if name == "hash":
                r["blocks_live"] = obj.info()["used"]
            res[f"{name}_skip{skip}"] = r
            print(name, skip, json.dumps(r), file=sys.stderr, flush=True)
            obj.close()
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
