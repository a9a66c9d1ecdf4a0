#!/usr/bin/env python3
"""Merge timing (tsdf_dense_merge / tsdf_hash_merge): 160 frames of the bench trajectory
fused into the bench's 512^3 @ 2 cm volume and its voxel hash (2^22 buckets), then each merged into an
empty 512^3 handle -- dense and hash on either side, with the identity and with a 10 degree / 20 cm
transform.  Per configuration: the HIP-event time of the merge's launches (tsdf_merge_last_profile with
profiling on) and the wall time of the call, the median, minimum and maximum of REPS merges, each into
a freshly reset destination; the samples, the updated bricks, the bricks the cull let through, and the
lower bound on the bytes moved -- updated bricks x 512 voxels x 12 B read and written, plus the source's
observed bricks x 512 x 12 B read once -- over the 8 TB/s peak.  The yardstick in the same run:
tsdf_hash_to_dense of the same table, a pass that moves the same state with no arithmetic.  The clock
is warmed by an untimed merge of each configuration.  Prints one JSON object.
    PYTHONPATH=union-thesis-slam_amd timeout -k 10 300 python tools/gpu/time_merge.py
"""
import contextlib
import io
import json
import sys
import time

import numpy as np
import torch

from tsdf_amd import _ffi, grid_fusion, hash_fusion, scene

FRAMES, REPS, HW = 160, 5, (480, 640)
ROOM, VOXEL = 10.24, 0.02
PEAK_BPS = 8.0e12


def summary(v, digits=3):
    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def rigid(deg, trans):
    """deg about a fixed oblique axis through the room's centre, then trans along another direction."""
    ax = np.array([0.3, 1.0, 0.2])
    ax = ax / np.linalg.norm(ax) * np.radians(deg)
    th = np.linalg.norm(ax)
    Kx = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    T = np.eye(4)
    if th > 0:
        T[:3, :3] = np.eye(3) + np.sin(th) / th * Kx + (1.0 - np.cos(th)) / th ** 2 * (Kx @ Kx)
    c = np.full(3, ROOM / 2)
    d = np.array([1.0, -0.5, 0.25])
    T[:3, 3] = c - T[:3, :3] @ c + d / np.linalg.norm(d) * trans
    return T


def make(kind):
    bnds = np.array([[0.0, ROOM]] * 3)
    with contextlib.redirect_stdout(io.StringIO()):
        return (grid_fusion.TSDFVolume(bnds, VOXEL) if kind == "dense" else
                hash_fusion.HashTable(bnds, VOXEL, 1 << 22, max_blocks=1 << 15))


def observed_bricks(src):
    """Source bricks with an observed voxel (weight > 0)."""
    if isinstance(src, hash_fusion.HashTable):
        w = src.export_blocks()[2]
        return int((w > 0).any(axis=1).sum())
    w = src.get_state()[1]
    n = w.shape[0] // 8
    return int((w.reshape(n, 8, n, 8, n, 8) > 0).any(axis=(1, 3, 5)).sum())


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
    torch.cuda.synchronize()
    res = {"build_id": _ffi.build_id(), "frames_fused": FRAMES, "reps": REPS, "units": "milliseconds unless named",
           "peak_bytes_per_s": PEAK_BPS}
    sources = {}
    for kind in ("dense", "hash"):
        sources[kind] = make(kind)
        sources[kind].integrate_batch(depth.data_ptr(), rgb.data_ptr(), K, Tinv, hw=HW, device_ptrs=True)
        res[f"{kind}_source_observed_bricks"] = observed_bricks(sources[kind])
    del depth, rgb
    torch.cuda.empty_cache()

    # the yardstick: the table densified into a dense handle
    yard = make("dense")
    ys = []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        _ffi.call("tsdf_hash_to_dense", sources["hash"]._h, yard._h)
        ys.append(1e3 * (time.perf_counter() - t0))
    res["yardstick_hash_to_dense_wall"] = summary(ys[1:])
    res["yardstick_note"] = "wall time of the call: a reset of the dense handle (a fill of 512^3 x 12 B) and the copy of the live blocks"
    yard.close()

    for dk in ("dense", "hash"):
        for sk in ("dense", "hash"):
            for label, T in (("identity", np.eye(4)), ("10deg_20cm", rigid(10.0, 0.2))):
                dst = make(dk)
                dst.set_profiling(True)
                ev, wall, info, cand = [], [], None, -1
                for i in range(REPS + 1):  # (the first is the warm-up)
                    dst.reset()
                    t0 = time.perf_counter()
                    info = dst.merge(sources[sk], T, return_info=True)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    ms, cand = grid_fusion.merge_last_profile()
                    ev.append(ms)
                nb = (512 // 8) ** 3
                bound_bytes = info["bricks_updated"] * 512 * 12 * 2 + res[f"{sk}_source_observed_bricks"] * 512 * 12
                bound_ms = 1e3 * bound_bytes / PEAK_BPS
                r = {"event": summary(ev[1:]), "wall": summary(wall[1:]), **info, "destination_bricks": nb,
                     "candidate_bricks": cand, "bound_bytes": bound_bytes, "bound_ms": round(bound_ms, 4),
                     "bound_over_event": round(bound_ms / float(np.median(ev[1:])), 4)}
                res[f"{sk}_to_{dk}_{label}"] = r
                print(sk, "->", dk, label, json.dumps(r), file=sys.stderr, flush=True)
                dst.close()
                torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
