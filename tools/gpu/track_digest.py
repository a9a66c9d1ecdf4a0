#!/usr/bin/env python3
"""Byte A/B of the tracker between two builds: sha256 of everything the
linearise and track entry points return, on the corner scene (tests/icp_ref.py), the plane scene
(tests/icp_color_ref.py) and one 640x480 frame of tools/gpu/track_time.py's workload.  Run once per
library (TSDF_HIP_LIB selects one built by tools/build_variant.sh), each in a fresh process; the two
outputs must be equal line for line, the build id line aside.
    PYTHONPATH=union-thesis-slam_amd:tests python tools/gpu/track_digest.py"""
import contextlib
import hashlib
import io

import numpy as np
import torch

import icp_color_ref as C
import icp_ref as I
from tsdf_amd import _ffi, grid_fusion, hash_fusion, scene, tracking


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        if p is None:
            h.update(b"<none>")
        elif isinstance(p, np.ndarray):
            h.update(str((p.dtype, p.shape)).encode() + np.ascontiguousarray(p).tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()[:32]


def lin_digest(r):
    keys = sorted(r)
    return sha(*[x for k in keys for x in (k, r[k])])


def track_digest(res):
    pose, info = res
    keys = sorted(info)
    return sha(pose, *[x for k in keys for x in (k, np.asarray(info[k]) if k == "trajectory" else info[k])])


def frames(frame):
    return (("u16", frame), ("f64", frame.astype(np.float64) / 1000.0))


def main():
    print("build_id", _ffi.build_id())
    K2 = I.FRAME_K.copy()
    K2[:2] *= 2
    M = I.offset_2cm_1deg()
    grey = np.full((106, 142, 3), 128, np.uint8)

    # ---- corner scene, geometric ----
    corner = grid_fusion.TSDFVolume(I.BOUNDS.copy(), I.VS)
    corner.set_state(*I.corner_state())
    d, n, _ = corner.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    print("corner maps", sha(d, n))
    hcorner = hash_fusion.HashTable(I.BOUNDS.copy(), I.VS, 1 << 14)
    rng = np.random.default_rng(9)
    for i in range(4):
        P = np.eye(4) if i == 0 else I.perturbation(rng, 0.03, 2.0)
        hcorner.integrate(grey, I.render(P, K2, (106, 142)).astype(np.float64) / 1000.0, K2, P)
    lin_frame = I.render(np.eye(4), I.FRAME_K, I.FRAME_HW)
    seen = I.render(I.TRUE_POSE, I.FRAME_K, I.FRAME_HW)
    g = I.TRUE_POSE @ I.perturbation(np.random.default_rng(11), 0.04, 2.0)
    for kind, f in frames(lin_frame):
        for s in (1, 3):
            r = tracking.icp_linearize(f, I.FRAME_K, M, d, n, I.MODEL_K, np.eye(4), stride=s, **{
                "dist_max": I.CORNER_GATES["dist_max"], "cos_min": I.CORNER_GATES["cos_min"]})
            print(f"corner linearize {kind} stride{s} inliers {r['inliers']}", lin_digest(r))
    for kind, f in frames(seen):
        for s in (1, 3):
            for name, obj in (("dense", corner), ("hash", hcorner)):
                res = obj.track(f, I.FRAME_K, g, z_far=I.Z_FAR, return_info=True, stride=s)
                print(f"corner track {name} {kind} stride{s} {res[1]['status']} it {res[1]['iterations']}", track_digest(res))

    # ---- plane scene, RGB-D ----
    plane = grid_fusion.TSDFVolume(I.BOUNDS.copy(), I.VS)
    plane.set_state(*C.plane_state())
    pd, pn, pc = plane.raycast(I.MODEL_K, np.eye(4), I.MODEL_HW, z_far=I.Z_FAR)
    print("plane maps", sha(pd, pn, pc))
    hplane = hash_fusion.HashTable(I.BOUNDS.copy(), I.VS, 1 << 14)
    rng = np.random.default_rng(9)
    for i in range(4):
        P = np.eye(4) if i == 0 else I.perturbation(rng, 0.03, 2.0)
        mm, rgb = C.plane_render(P, K2, (106, 142))
        hplane.integrate(rgb, mm.astype(np.float64) / 1000.0, K2, P)
    lframe, lrgb = C.plane_render(extras=True)
    pframe, prgb = C.plane_render()
    start = C.plane_starts()[0]
    for kind, f in frames(lframe):
        for s in (1, 3):
            r = tracking.icp_linearize_rgbd(f, lrgb, I.FRAME_K, M, pd, pn, pc, I.MODEL_K, np.eye(4), stride=s)
            print(f"plane linearize_rgbd {kind} stride{s} inliers {r['inliers']} / {r['color_inliers']}", lin_digest(r))
            r = tracking.icp_linearize(f, I.FRAME_K, M, pd, pn, I.MODEL_K, np.eye(4), stride=s)
            print(f"plane linearize {kind} stride{s} inliers {r['inliers']}", lin_digest(r))
    for kind, f in frames(pframe):
        for s in (1, 3):
            for name, obj in (("dense", plane), ("hash", hplane)):
                for lam in (None, 0.0):
                    kw = {} if lam is None else {"color_weight": lam}
                    res = obj.track(f, I.FRAME_K, start, z_far=I.Z_FAR, return_info=True, color_im=prgb, stride=s, **kw)
                    print(f"plane track_rgbd {name} {kind} stride{s} lambda {lam} {res[1]['status']} it {res[1]['iterations']}",
                          track_digest(res))
    for o in (corner, hcorner, plane, hplane):
        o.close()

    # ---- one 640x480 frame of track_time.py's workload, dense: the grid is capped at 4 CUs ----
    dev = torch.device("cuda", 0)
    FRAMES, F, HW = 160, 120, (480, 640)
    poses = scene.trajectory(FRAMES, seed=0, radius_frac=scene.BENCH_RING)
    sph = scene.make_spheres(0, ring_frac=scene.BENCH_RING)
    depth = torch.empty((FRAMES,) + HW, dtype=torch.int16, device=dev)
    rgb = torch.empty((FRAMES,) + HW + (3,), dtype=torch.uint8, device=dev)
    for s in range(0, FRAMES, 40):
        dd, cc = scene.render(poses[s:s + 40], sph, seed=0, start=s, device=dev, depth_dtype=torch.int16)
        depth[s:s + len(dd)] = dd
        rgb[s:s + len(cc)] = cc
    K = scene.intrinsics()
    Tinv = np.ascontiguousarray(np.linalg.inv(poses))
    torch.cuda.synchronize()
    with contextlib.redirect_stdout(io.StringIO()):
        vol = grid_fusion.TSDFVolume(np.array([[0.0, 10.24]] * 3), 0.02)
    vol.integrate_batch(depth.data_ptr(), rgb.data_ptr(), K, Tinv, hw=HW, device_ptrs=True)
    z_far = 10.24 * 3 ** 0.5
    res = vol.track(depth[F], K, poses[F - 1], z_far=z_far, return_info=True)
    print(f"640x480 track dense {res[1]['status']} it {res[1]['iterations']} inliers {res[1]['inliers']}", track_digest(res))
    res = vol.track(depth[F], K, poses[F - 1], z_far=z_far, return_info=True, color_im=rgb[F])
    print(f"640x480 track_rgbd dense {res[1]['status']} it {res[1]['iterations']} colour inliers {res[1]['color_inliers']}",
          track_digest(res))
    vol.close()


if __name__ == "__main__":
    main()
