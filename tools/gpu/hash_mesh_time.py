#!/usr/bin/env python3
"""Mesh extraction of the voxel hash (tsdf_hash_extract_mesh) against the path it
replaces: densify into a dense handle of the whole extent (HashTable._as_grid) and run the dense
marching cubes there.  Two workloads:
  a  the bench's 512^3 @ 2 cm hash (2^22 buckets) after 160 frames of the bench trajectory;
  b  a 1024^3 @ 1 cm table holding the same blocks (exported from a, imported at the same block
     coordinates): eight times the extent, the same live blocks.
Both paths are timed in the same process, alternating, with a host clock around the synchronising
calls, after a warm-up: the new path is one tsdf_hash_extract_mesh; the old path is the creation of
the dense handle, tsdf_hash_to_dense and tsdf_dense_extract_mesh (what get_mesh ran before), with the
dense extraction alone given beside it.  Median, minimum and maximum over REPS repeats, in
milliseconds; the old path's range is its run-to-run spread.  If the old path fails on b (it needs
30 bytes per voxel of the extent) that is recorded and not retried.  Prints one JSON object.
    PYTHONPATH=union-thesis-slam_amd python tools/gpu/hash_mesh_time.py
--new-only times the new path alone on workload a (for a run under rocprofv3 --kernel-trace --stats,
whose per-kernel split then holds nothing of the dense path)."""
import argparse
import contextlib
import ctypes
import io
import json
import sys
import time

import numpy as np
import torch

from tsdf_amd import _ffi, hash_fusion, scene

FRAMES, HW, REPS, WARM = 160, (480, 640), 12, 3
ROOM = 10.24


def summary(v):
    return {"median": round(1e3 * float(np.median(v)), 3), "min": round(1e3 * min(v), 3), "max": round(1e3 * max(v), 3),
            "n": len(v)}


def new_path(ht):
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    t0 = time.perf_counter()
    _ffi.call("tsdf_hash_extract_mesh", ht._h, ctypes.byref(nv), ctypes.byref(nt))
    return time.perf_counter() - t0, nv.value, nt.value


def old_path(ht):
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    t0 = time.perf_counter()
    grid = ht._as_grid()
    t1 = time.perf_counter()
    _ffi.call("tsdf_dense_extract_mesh", grid._h, ctypes.byref(nv), ctypes.byref(nt))
    t2 = time.perf_counter()
    grid.close()
    return t2 - t0, t2 - t1, nv.value, nt.value


def time_table(ht, old=True, old_reps=REPS):
    res = {}
    for _ in range(WARM):
        new_path(ht)
    new, whole, dense = [], [], []
    counts = None
    failed = None
    for i in range(REPS):
        dt, nv, nt = new_path(ht)
        new.append(dt)
        counts = (nv, nt)
        if old and failed is None and i < old_reps:
            try:
                a, b, ov, ot = old_path(ht)
            except _ffi.TSDFError as e:  # (recorded, not retried)
                failed = str(e)
                continue
            if i == 0:
                continue  # the old path's first run is its warm-up
            whole.append(a)
            dense.append(b)
            assert (ov, ot) == counts, ((ov, ot), counts)
    info = ht.mesh_info()
    res.update(vertices=counts[0], triangles=counts[1], live_blocks=info["live_blocks"], mesh_blocks=info["mesh_blocks"],
               scratch_bytes=info["scratch_bytes"], new_ms=summary(new))
    if whole:
        res["old_ms"] = summary(whole)
        res["old_dense_extract_alone_ms"] = summary(dense)
    if failed:
        res["old_failed"] = failed
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--new-only", action="store_true")
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
    torch.cuda.synchronize()
    res = {"build_id": _ffi.build_id(), "frames_fused": FRAMES, "reps": REPS, "warmup": WARM,
           "units": "milliseconds, host clock around the synchronising calls"}
    with contextlib.redirect_stdout(io.StringIO()):
        a = hash_fusion.HashTable(np.array([[0.0, ROOM]] * 3), 0.02, 1 << 22, max_blocks=1 << 15)
    a.integrate_batch(depth.data_ptr(), rgb.data_ptr(), K, Tinv, hw=HW, device_ptrs=True)
    del depth, rgb
    torch.cuda.empty_cache()
    res["a_512_2cm"] = time_table(a, old=not args.new_only)
    res["a_512_2cm"]["table_load"] = round(a.get_load_factor(), 4)
    print("a", json.dumps(res["a_512_2cm"]), file=sys.stderr, flush=True)
    if not args.new_only:
        blocks = a.export_blocks()
        with contextlib.redirect_stdout(io.StringIO()):
            b = hash_fusion.HashTable(np.array([[0.0, ROOM]] * 3), 0.01, 1 << 22, max_blocks=len(blocks[0]) + 64)
        assert tuple(int(x) for x in b._vol_dim) == (1024,) * 3
        b.import_blocks(*blocks)
        del blocks
        res["b_1024_1cm"] = time_table(b, old_reps=4)
        print("b", json.dumps(res["b_1024_1cm"]), file=sys.stderr, flush=True)
        b.close()
    a.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
