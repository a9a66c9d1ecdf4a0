#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the build container, where /root/reference (DiWu9/Union-Thesis-SLAM, read-only)
is mounted; it is a no-op elsewhere.  The reference is imported in a child process with
  PYTHONPATH = tools/refstubs : /root/reference     (numba/skimage are absent here)
  PYTHONDONTWRITEBYTECODE = 1                        (the reference tree is read-only)
and the numba-compiled helpers are replaced by NumPy versions with numba's typing
(`faithful_patch`), because an identity-`njit` stub would run vox2world in float32 under NumPy 2
weak-scalar rules and flip pixels.  rigid_transform (np.dot -> OpenBLAS dgemm)
and every other line of integrate() run as the reference wrote them.

Fixtures written (data only -- inputs and expected outputs, no reference source):
  golden/hash_kat.npz          hash_function KATs, int64 and int32-wrapping modes (G1)
  golden/lounge/               lounge frames 0-9 depth PNG, 0-2 colour JPG, poses, intrinsics
  golden/dense_c1.npz          lounge f0-f2 -> 128^3 @ 4 cm, reference grid CPU path, per frame (G2)
  golden/dense_c1_ow.npz       same with obs_weight = 1.0, 0.7, 2.5 (mixed f32/f64 colour path)
  golden/hash_c1.npz           lounge f0-f2 -> 128^3 @ 4 cm, reference HashTable.integrate (G2h)
  golden/hash_c1_remove.npz    lounge f0, remove_hash_entry over a rule's set, lounge f1: the returns,
                               entry counts, the removed voxels that are back, a state digest (G2r)
  golden/synth_c1.npz          two synthetic frames (tsdf_amd.scene) -> 128^3 @ 8 cm room (G2s)
  golden/hostile_depth.npz     tests/hostile_depth.py's NaN / infinite / negative / tiny / far / huge f64
                               depth frames -> 48x40x24 @ 2 cm, grid CPU path and HashTable.integrate,
                               at 128x96 and 126x95 (G2x)
  golden/hostile_pose.npz      tests/hostile_pose.py's NaN / infinite / huge / singular / non-rigid poses and
                               negative / zero / non-finite intrinsics -> 40x24x20 @ 4 cm and 0.0625 m, grid CPU
                               path on a preloaded volume and HashTable.integrate on a fresh table; their
                               view frusta and the demo's running bounds (G2p)
  golden/lounge2cm_kat.json    lounge 2 cm, frames 0-9: per-frame counts + final-state digest (G3)
  golden/lounge512_kat.json    lounge f0 -> 512^3 @ 2 cm: count + digest (G5)
  golden/frustum_bounds.npz    lounge frames 0-999: per-frame max depth (mm, after the demo's
                               65535 -> 0 masking), poses, and the reference get_view_frustum
                               points + the demo's running min/max bounds (G6)
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLD = os.path.join(REPO, "tests", "golden")

LOUNGE_BNDS = [[-4.22106438, 3.86798203], [-2.6663104, 2.60146141], [0., 5.76272371]]
C1_BNDS = [[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]]
C5_BNDS = [[-5.12, 5.12], [-5.12, 5.12], [-2.0, 8.24]]


def faithful_patch(grid_fusion, hash_fusion):
    """Numba-typing-faithful replacements for the @njit helpers (grid_fusion.py:170-212,
    hash_fusion.py:71-101)."""

    def vox2world(vol_origin, vox_coords, vox_size):
        o = vol_origin.astype(np.float32).astype(np.float64)
        c = vox_coords.astype(np.float32).astype(np.float64)
        return (o[None, :] + float(vox_size) * c).astype(np.float32)

    def cam2pix(cam_pts, intr):
        intr = intr.astype(np.float32).astype(np.float64)
        fx, fy, cx, cy = intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]
        pix = np.empty((cam_pts.shape[0], 2), dtype=np.int64)
        with np.errstate(all="ignore"):
            pix[:, 0] = np.rint((cam_pts[:, 0] * fx) / cam_pts[:, 2] + cx).astype(np.int64)
            pix[:, 1] = np.rint((cam_pts[:, 1] * fy) / cam_pts[:, 2] + cy).astype(np.int64)
        return pix

    def integrate_tsdf(tsdf_vol, dist, w_old, obs_weight):
        w_new = (w_old.astype(np.float64) + float(obs_weight)).astype(np.float32)
        prod = (w_old.astype(np.float32) * tsdf_vol.astype(np.float32)).astype(np.float64)
        t = ((prod + float(obs_weight) * dist) / w_new.astype(np.float64)).astype(np.float32)
        return t, w_new

    grid_fusion.TSDFVolume.vox2world = staticmethod(vox2world)
    grid_fusion.TSDFVolume.cam2pix = staticmethod(cam2pix)
    grid_fusion.TSDFVolume.integrate_tsdf = staticmethod(integrate_tsdf)
    hash_fusion.HashTable.vox2world = staticmethod(vox2world)
    hash_fusion.HashTable.cam2pix = staticmethod(cam2pix)


def load_lounge(i, color=True):
    from PIL import Image
    d = np.array(Image.open(os.path.join(REF, "data", "frame-%06d.depth.png" % i)))
    depth = d.astype(float) / 1000.0
    depth[depth == 65.535] = 0
    pose = np.loadtxt(os.path.join(REF, "data", "frame-%06d.pose.txt" % i))
    rgb = None
    if color:
        rgb = np.array(Image.open(os.path.join(REF, "data", "frame-%06d.color.jpg" % i)).convert("RGB"))
    return d, depth, rgb, pose


def sparse_state(tsdf_obj):
    w = tsdf_obj._weight_vol_cpu.reshape(-1)
    idx = np.flatnonzero(w > 0).astype(np.int64)
    return (idx, tsdf_obj._tsdf_vol_cpu.reshape(-1)[idx].copy(), w[idx].copy(),
            tsdf_obj._color_vol_cpu.reshape(-1)[idx].copy())


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def inner():
    os.makedirs(GOLD, exist_ok=True)
    import grid_fusion  # noqa: E402  (the reference, via PYTHONPATH)
    import hash_fusion  # noqa: E402
    faithful_patch(grid_fusion, hash_fusion)
    cam_intr = np.loadtxt(os.path.join(REF, "data", "camera-intrinsics.txt"), delimiter=" ")
    only = set(sys.argv[sys.argv.index("--inner") + 1:])

    def want(name):
        return not only or name in only

    # ---- lounge inputs (data files copied as-is) --------------------------------------
    if want("lounge"):
        ld = os.path.join(GOLD, "lounge")
        os.makedirs(ld, exist_ok=True)
        shutil.copy(os.path.join(REF, "data", "camera-intrinsics.txt"), ld)
        shas = {}
        for i in range(10):
            for ext in ["depth.png", "pose.txt"] + (["color.jpg"] if i < 3 else []):
                shutil.copy(os.path.join(REF, "data", "frame-%06d.%s" % (i, ext)), ld)
            d, _, rgb, _ = load_lounge(i, color=i < 3)
            shas["frame-%06d.depth" % i] = digest(d)
            if rgb is not None:
                shas["frame-%06d.color" % i] = digest(rgb)
        with open(os.path.join(ld, "decoded_sha256.json"), "w") as f:
            json.dump(shas, f, indent=1, sort_keys=True)
        print("lounge inputs copied")

    # ---- G1 hash KATs ------------------------------------------------------------------
    if want("hash"):
        ht = hash_fusion.HashTable([[0, 0.04], [0, 0.04], [0, 0.04]], 0.02, 10, False)
        rng = np.random.default_rng(1234)
        coords = rng.integers(-1024, 1025, size=(256, 3)).astype(np.int64)
        coords = np.concatenate([coords, np.array([[80, 56, 0], [333, 234, 241], [342, 234, 241],
                                                   [332, 234, 242], [0, 0, 0], [-1, -1, -1]])])
        sizes = np.array([10, 1000, 100000, 1000000, 1 << 22], np.int64)
        out64 = np.empty((len(sizes), len(coords)), np.int64)
        out32 = np.empty_like(out64)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for si, n in enumerate(sizes):
                ht._table_size = int(n)
                for ci, c in enumerate(coords):
                    out64[si, ci] = int(ht.hash_function([np.int64(v) for v in c]))
                    out32[si, ci] = int(ht.hash_function([np.int32(v) for v in c]))
        np.savez_compressed(os.path.join(GOLD, "hash_kat.npz"), coords=coords, sizes=sizes,
                            h64=out64, h32=out32)
        print("hash KAT:", out64[2, -6:-2], out32[2, -6:-2])

    # ---- G2 dense config 1 -------------------------------------------------------------
    for name, ows in (("dense_c1", (1.0, 1.0, 1.0)), ("dense_c1_ow", (1.0, 0.7, 2.5))):
        if not want(name):
            continue
        vol = grid_fusion.TSDFVolume(np.array(C1_BNDS), 0.04, use_gpu=False)
        res = {"dims": np.asarray(vol._vol_dim), "origin": vol._vol_origin,
               "bounds_after": vol._vol_bnds, "obs_weight": np.array(ows)}
        prev = np.zeros(vol._weight_vol_cpu.shape, np.float32)
        for f in range(3):
            _, depth, rgb, pose = load_lounge(f)
            vol.integrate(rgb, depth, cam_intr, pose, obs_weight=ows[f])
            idx, t, w, c = sparse_state(vol)
            res["f%d_idx" % f], res["f%d_tsdf" % f], res["f%d_weight" % f], res["f%d_color" % f] = idx, t, w, c
            res["f%d_nupd" % f] = np.int64((vol._weight_vol_cpu != prev).sum())
            prev = vol._weight_vol_cpu.copy()
            print(name, "frame", f, "updated", int(res["f%d_nupd" % f]), "entries", len(idx),
                  "tsdf<1", int((t < 1).sum()))
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **res)

    # ---- G2h hash config 1 (reference per-voxel loop, ~2 s/frame) ------------------------
    if want("hash_c1"):
        ht = hash_fusion.HashTable(np.array(C1_BNDS), 0.04, 1000000, 0.75, False)
        res = {}
        for f in range(3):
            _, depth, rgb, pose = load_lounge(f)
            ht.integrate(rgb, depth, cam_intr, pose, obs_weight=1.0)
            pos, sdf, w, col = [], [], [], []
            for b in ht._hash_table:
                if b is None:
                    continue
                for j in range(5):
                    e = b.get_ith_entry(j)
                    if e is not None and e.get_voxel() is not None:
                        v = e.get_voxel()
                        pos.append([int(p) for p in e.get_position()])
                        sdf.append(float(v.get_sdf()))
                        w.append(float(v._weight))
                        col.append(float(v.get_color()))
            pos = np.array(pos, np.int64)
            order = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))
            res["f%d_pos" % f] = pos[order]
            res["f%d_sdf" % f] = np.array(sdf)[order]
            res["f%d_weight" % f] = np.array(w)[order]
            res["f%d_color" % f] = np.array(col)[order]
            res["f%d_entries" % f] = np.int64(ht.count_num_hash_entries())
            res["f%d_nonempty" % f] = np.int64(ht.get_num_non_empty_buckets())
            res["f%d_collisions" % f] = np.int64(ht.get_num_collisions())
            print("hash_c1 frame", f, "entries", len(pos), "buckets", ht.get_num_non_empty_buckets())
        np.savez_compressed(os.path.join(GOLD, "hash_c1.npz"), **res)

    # ---- G2r hash config 1 with a removal between two frames ---------------------------------
    # lounge f0, remove_hash_entry over a set taken from hash_c1.npz's f0_pos (tests/hash_model.py
    # removal_rule: every third entry, plus every entry of every fifth block), lounge f1
    if want("hash_c1_remove"):
        sys.path.insert(0, os.path.join(REPO, "tests"))
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        from hash_model import removal_rule
        from data_structures import hash_entry as he
        f0_pos = np.load(os.path.join(GOLD, "hash_c1.npz"))["f0_pos"]
        idx = removal_rule(f0_pos)
        ht = hash_fusion.HashTable(np.array(C1_BNDS), 0.04, 1000000, 0.75, False)
        _, depth, rgb, pose = load_lounge(0)
        ht.integrate(rgb, depth, cam_intr, pose, obs_weight=1.0)
        ret = np.array([ht.remove_hash_entry(he.HashEntry([int(v) for v in p], None, None)) for p in f0_pos[idx]],
                       np.uint8)
        res = {"remove_idx": idx.astype(np.int32), "remove_ret": ret,
               "entries_after_remove": np.int64(ht.count_num_hash_entries()),
               "nonempty_after_remove": np.int64(ht.get_num_non_empty_buckets())}
        _, depth, rgb, pose = load_lounge(1)
        ht.integrate(rgb, depth, cam_intr, pose, obs_weight=1.0)
        pos, sdf, w, col = [], [], [], []
        for b in ht._hash_table:
            if b is None:
                continue
            for j in range(5):
                e = b.get_ith_entry(j)
                if e is not None and e.get_voxel() is not None:
                    pos.append([int(p) for p in e.get_position()])
                    sdf.append(float(e.get_voxel().get_sdf()))
                    w.append(float(e.get_voxel()._weight))
                    col.append(float(e.get_voxel().get_color()))
        pos = np.array(pos, np.int64)
        order = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))
        pos, sdf, w, col = pos[order], np.array(sdf)[order], np.array(w)[order], np.array(col)[order]
        lin = np.ravel_multi_index(tuple(pos.T), (128, 128, 128))
        back = np.isin(lin, np.ravel_multi_index(tuple(f0_pos[idx].T), (128, 128, 128)))
        res.update(entries_f1=np.int64(ht.count_num_hash_entries()), back_pos=pos[back].astype(np.int16),
                   back_sdf=sdf[back], back_weight=w[back].astype(np.float32), back_color=col[back].astype(np.float32),
                   state_sha256=np.array(digest(pos, sdf, w, col)))
        assert np.array_equal(res["back_weight"].astype(np.float64), w[back])
        assert np.array_equal(res["back_color"].astype(np.float64), col[back])
        print("hash_c1_remove removed", int(ret.sum()), "of", len(ret), "entries", int(res["entries_after_remove"]),
              "->", int(res["entries_f1"]), "back", int(back.sum()), "weights", np.unique(w[back]))
        np.savez_compressed(os.path.join(GOLD, "hash_c1_remove.npz"), **res)

    # ---- G2s synthetic frames into 128^3 @ 8 cm of the room ----------------------------
    if want("synth"):
        sys.path.insert(0, os.path.join(REPO, "union-thesis-slam_amd"))
        from tsdf_amd import scene
        sp = scene.make_spheres(0)
        poses = scene.trajectory(1000, seed=0)[[0, 137]]
        depth_u16, rgb = scene.render(poses, sp, seed=0, start=0)
        depth_u16, rgb = depth_u16.numpy(), rgb.numpy()
        vol = grid_fusion.TSDFVolume(np.array([[0.0, 10.24]] * 3), 0.08, use_gpu=False)
        res = {"depth_u16": depth_u16, "rgb": rgb, "poses": poses, "K": scene.intrinsics()}
        prev = np.zeros(vol._weight_vol_cpu.shape, np.float32)
        for f in range(2):
            vol.integrate(rgb[f], scene.depth_metres(depth_u16[f]), scene.intrinsics(), poses[f])
            idx, t, w, c = sparse_state(vol)
            res["f%d_idx" % f], res["f%d_tsdf" % f], res["f%d_weight" % f], res["f%d_color" % f] = idx, t, w, c
            res["f%d_nupd" % f] = np.int64((vol._weight_vol_cpu != prev).sum())
            prev = vol._weight_vol_cpu.copy()
            print("synth frame", f, "updated", int(res["f%d_nupd" % f]))
        np.savez_compressed(os.path.join(GOLD, "synth_c1.npz"), **res)

    # ---- G2x hostile f64 depth (tests/hostile_depth.py) -------------------------------------
    if want("hostile"):
        gen_hostile(grid_fusion, hash_fusion)

    # ---- G2p hostile poses and intrinsics (tests/hostile_pose.py) -----------------------------
    if want("hostile_pose"):
        gen_hostile_pose(grid_fusion, hash_fusion)

    # ---- G3 lounge 2 cm, 10 frames -----------------------------------------------------
    if want("lounge2cm"):
        vol = grid_fusion.TSDFVolume(np.array(LOUNGE_BNDS), 0.02, use_gpu=False)
        kat = {"bounds": LOUNGE_BNDS, "voxel_size": 0.02, "dims": [int(d) for d in vol._vol_dim],
               "frames": []}
        prev = np.zeros(vol._weight_vol_cpu.shape, np.float32)
        for f in range(10):
            _, depth, rgb, pose = load_lounge(f, color=False)
            rgb = np.zeros(depth.shape + (3,), np.uint8)  # colour does not affect the voxel set
            vol.integrate(rgb, depth, cam_intr, pose)
            w = vol._weight_vol_cpu
            nupd = int((w != prev).sum())
            newk = int(((w > 0) & (prev == 0)).sum())
            prev = w.copy()
            kat["frames"].append({"updated": nupd, "new_keys": newk,
                                  "sum_weight": float(w.sum(dtype=np.float64))})
            print("lounge2cm frame", f, nupd, newk)
        idx, t, w, _ = sparse_state(vol)
        kat["unique"] = int(len(idx))
        kat["digest_idx_tsdf_weight"] = digest(idx, t, w)
        with open(os.path.join(GOLD, "lounge2cm_kat.json"), "w") as fh:
            json.dump(kat, fh, indent=1)

    # ---- G6 frustum bounds over the 1000 lounge frames -----------------------------------
    if want("frustum"):
        gen_frustum(grid_fusion, cam_intr)

    # ---- G5 lounge f0 -> 512^3 @ 2 cm --------------------------------------------------
    if want("lounge512"):
        vol = grid_fusion.TSDFVolume(np.array(C5_BNDS), 0.02, use_gpu=False)
        _, depth, rgb, pose = load_lounge(0)
        vol.integrate(rgb, depth, cam_intr, pose)
        idx, t, w, c = sparse_state(vol)
        kat = {"bounds": C5_BNDS, "voxel_size": 0.02, "dims": [int(d) for d in vol._vol_dim],
               "updated": int(len(idx)), "digest_idx_tsdf_weight_color": digest(idx, t, w, c)}
        print("lounge512", kat)
        with open(os.path.join(GOLD, "lounge512_kat.json"), "w") as fh:
            json.dump(kat, fh, indent=1)


def gen_hostile(grid_fusion, hash_fusion):
    """G2x: the frames of tests/hostile_depth.py (NaN, infinities, negatives, tiny, far and huge f64
    depths) through the reference's CPU TSDFVolume.integrate and its HashTable.integrate, once per
    image size.  Stored per size s: the inputs (depth, the three colour images and which frame uses
    which, poses, weights, K, bounds), per frame the voxels whose weight the frame changed with
    their new tsdf / weight / colour (a packed mask over the C-order voxels, then the values of its set
    bits in order; applied frame after frame they give the sparse state after every
    frame) and the update count, and the hash path's final entries (mask and values alike) with its per-frame entry counts."""
    import time
    import warnings
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import hostile_depth as H
    res = {"K": H.K, "bounds": np.array(H.BOUNDS), "voxel_size": np.float64(H.VS), "class_names": np.array(list(H.CLASSES)),
           "class_values": H.VALUES}
    for s in H.SIZES:
        names, depth, rgb, poses, ow = H.sequence(s)
        uniq = np.stack([H.rgb(s, k) for k in range(3)])
        index = np.arange(len(names)) % 3
        assert np.array_equal(uniq[index], rgb)
        res.update({s + "_names": np.array(names), s + "_depth": depth, s + "_rgb": uniq, s + "_rgb_index": index.astype(np.uint8),
                    s + "_poses": poses, s + "_obs_weight": ow})
        vol = grid_fusion.TSDFVolume(np.array(H.BOUNDS), H.VS, use_gpu=False)
        assert tuple(int(d) for d in vol._vol_dim) == H.DIMS and vol._tsdf_vol_cpu.size < 65536
        ht = hash_fusion.HashTable(np.array(H.BOUNDS), H.VS, 100000, 0.75, False)
        prev = np.zeros(vol._weight_vol_cpu.shape, np.float32)
        t_hash, entries = 0.0, []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (overflow in 1.7e308 / trunc; invalid in inf - inf never occurs)
            for f in range(len(names)):
                vol.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f]))
                w = vol._weight_vol_cpu
                prev_flat = prev.reshape(-1)
                idx = np.flatnonzero(w.reshape(-1) != prev_flat)
                p = "%s_f%d_" % (s, f)
                res[p + "mask"] = np.packbits(w.reshape(-1) != prev_flat)
                res[p + "tsdf"] = vol._tsdf_vol_cpu.reshape(-1)[idx].copy()
                res[p + "weight"] = w.reshape(-1)[idx].copy()
                res[p + "color"] = vol._color_vol_cpu.reshape(-1)[idx].copy()
                res[p + "nupd"] = np.int64(len(idx))
                prev = w.copy()
                t0 = time.time()
                ht.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f]))
                t_hash += time.time() - t0
                entries.append(ht.count_num_hash_entries())
        assert not np.isnan(vol._tsdf_vol_cpu).any()
        pos, sdf, w, col = [], [], [], []
        for b in ht._hash_table:
            if b is None:
                continue
            for j in range(5):
                e = b.get_ith_entry(j)
                if e is not None and e.get_voxel() is not None:
                    pos.append([int(q) for q in e.get_position()])
                    sdf.append(float(e.get_voxel().get_sdf()))
                    w.append(float(e.get_voxel()._weight))
                    col.append(float(e.get_voxel().get_color()))
        pos = np.array(pos, np.int64)
        order = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))
        has = np.zeros(H.DIMS, bool)
        has[tuple(pos.T)] = True  # (C-order of the set bits == the lexsort order)
        res.update({s + "_hash_mask": np.packbits(has.reshape(-1)), s + "_hash_sdf": np.array(sdf)[order],
                    s + "_hash_weight": np.array(w)[order].astype(np.float32), s + "_hash_color": np.array(col)[order].astype(np.float32),
                    s + "_hash_entries": np.array(entries, np.int64)})
        assert np.array_equal(res[s + "_hash_weight"].astype(np.float64), np.array(w)[order])
        assert np.array_equal(res[s + "_hash_color"].astype(np.float64), np.array(col)[order])
        print("hostile", s, "updates", [int(res["%s_f%d_nupd" % (s, f)]) for f in range(len(names))], "entries", entries[-1],
              "hash path %.1f s" % t_hash)
    np.savez_compressed(os.path.join(GOLD, "hostile_depth.npz"), **res)
    print("hostile_depth.npz", os.path.getsize(os.path.join(GOLD, "hostile_depth.npz")), "bytes")


def gen_hostile_pose(grid_fusion, hash_fusion):
    """G2p: every case of tests/hostile_pose.py through the reference's CPU TSDFVolume.integrate, on a
    volume preloaded with the good frames, and through HashTable.integrate on a fresh table; in the
    "pose" form as the reference takes it, in the "rows" form with np.linalg.inv answering the case's
    rows for the duration of the call (inv(cam_pose) is the only use integrate makes of the pose).
    Stored per case and form p = "<name>/<form>/": p + "raised" (the exception's type name, "" if none),
    p + "nupd", p + "mask" (packed, C order: voxels whose weight the frame changed), p + "sha" (sha256 of
    the whole tsdf, weight and colour volumes after the frame), p + "hash_mask" (the table's keys) and
    p + "hash_sha" (sdf, weight, colour of the entries in C order, f64).  Per "pose" form also
    p + "frustum" (get_view_frustum for a frame whose max depth is the good frame's; NaN where it
    gives NaN) and p + "frustum_bounds" (the demo's np.minimum / np.amin bounds of that frame alone,
    from zeros); "frustum_running": the same bounds folded over the cases in "frustum_order" (those
    whose own bounds hold no NaN first).  The inputs are stored beside them."""
    import warnings
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import hostile_pose as P
    real_inv = np.linalg.inv
    cases = P.frame_cases()
    res = {"names": np.array(list(cases)), "K_good": P.K, "hw": np.array(P.HW)}
    pre = {}
    for vol, (b, vs) in P.VOLUMES.items():
        v = grid_fusion.TSDFVolume(np.array(b), vs, use_gpu=False)
        assert tuple(int(d) for d in v._vol_dim) == P.DIMS
        for f in range(P.PRELOAD):
            v.integrate(P.rgb(f), P.depth_m(vol, f), P.K, P.good_pose(vol, f))
        pre[vol] = v
        res["preload_sha_" + vol] = np.array(digest(v._tsdf_vol_cpu, v._weight_vol_cpu, v._color_vol_cpu))
        res["preload_n_" + vol] = np.int64((v._weight_vol_cpu > 0).sum())
    run_b = np.zeros((3, 2))
    running, frusta = [], {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, c in cases.items():
            vol = c["vol"]
            b, vs = P.VOLUMES[vol]
            res[name + "/rows"], res[name + "/K"] = c["rows"], c["K"]
            if c["pose"] is not None:
                res[name + "/pose"] = c["pose"]
            for form in P.forms(c):
                p = "%s/%s/" % (name, form)
                v = grid_fusion.TSDFVolume(np.array(b), vs, use_gpu=False)
                for a in ("_tsdf_vol_cpu", "_weight_vol_cpu", "_color_vol_cpu"):
                    setattr(v, a, getattr(pre[vol], a).copy())
                ht = hash_fusion.HashTable(np.array(b), vs, 100000, 0.75, False)
                pose = c["pose"] if form == "pose" else np.eye(4)
                if form == "rows":
                    np.linalg.inv = lambda m, rows=c["rows"]: rows.copy()
                raised = ""
                try:
                    v.integrate(P.rgb(P.PRELOAD), P.depth_m(vol, P.PRELOAD), c["K"], pose)
                    ht.integrate(P.rgb(P.PRELOAD), P.depth_m(vol, P.PRELOAD), c["K"], pose)
                except Exception as e:  # (recorded: the drop-in class must raise the same type)
                    raised = type(e).__name__
                finally:
                    np.linalg.inv = real_inv
                changed = v._weight_vol_cpu.reshape(-1) != pre[vol]._weight_vol_cpu.reshape(-1)
                res[p + "raised"] = np.array(raised)
                res[p + "nupd"] = np.int64(changed.sum())
                res[p + "mask"] = np.packbits(changed)
                res[p + "sha"] = np.array(digest(v._tsdf_vol_cpu, v._weight_vol_cpu, v._color_vol_cpu))
                has = np.zeros(P.DIMS, bool)
                sdf, w, col = np.ones(P.DIMS), np.zeros(P.DIMS), np.zeros(P.DIMS)
                for bk in ht._hash_table:
                    if bk is None:
                        continue
                    for j in range(5):
                        e = bk.get_ith_entry(j)
                        if e is not None and e.get_voxel() is not None:
                            q = tuple(int(x) for x in e.get_position())
                            has[q] = True
                            sdf[q], w[q], col[q] = float(e.get_voxel().get_sdf()), float(e.get_voxel()._weight), float(e.get_voxel().get_color())
                assert int(has.sum()) == ht.count_num_hash_entries()
                res[p + "hash_mask"] = np.packbits(has.reshape(-1))
                res[p + "hash_sha"] = np.array(digest(sdf[has], w[has], col[has]))
                if form == "pose":
                    proxy = np.zeros(P.HW)
                    proxy[0, 0] = float(P.depth_m(vol, P.PRELOAD).max())
                    vfp = grid_fusion.get_view_frustum(proxy, c["K"], c["pose"])
                    res[p + "frustum"] = vfp
                    frusta[name] = vfp
                print("hostile_pose", p, raised or int(res[p + "nupd"]), "entries", int(has.sum()))
    # the demo's loop (grid_demo1.py:50-64) from zeros: over each case alone, and over all of them with
    # the cases whose own bounds hold no NaN first (np.minimum keeps a NaN for good)
    def fold(b, vfp):
        b = b.copy()
        b[:, 0] = np.minimum(b[:, 0], np.amin(vfp, axis=1))
        b[:, 1] = np.maximum(b[:, 1], np.amax(vfp, axis=1))
        return b

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, vfp in frusta.items():
            res[name + "/pose/frustum_bounds"] = fold(np.zeros((3, 2)), vfp)
        order = sorted(frusta, key=lambda n: bool(np.isnan(res[n + "/pose/frustum_bounds"]).any()))
        for name in order:
            run_b = fold(run_b, frusta[name])
            running.append(run_b)
    res["frustum_order"] = np.array(order)
    res["frustum_running"] = np.stack(running)
    np.savez_compressed(os.path.join(GOLD, "hostile_pose.npz"), **res)
    print("hostile_pose.npz", os.path.getsize(os.path.join(GOLD, "hostile_pose.npz")), "bytes")


def gen_frustum(grid_fusion, cam_intr):
    """G6: grid_demo1.py:50-64 over the 1000 lounge frames.  get_view_frustum only reads the
    image shape and np.max(depth), so it is called on a zero image of the frame's shape holding
    the frame's max depth at one pixel -- exactly the reference computation, without shipping
    1000 depth images."""
    from PIL import Image
    n = 1000
    max_mm = np.zeros(n, np.uint16)
    poses = np.zeros((n, 4, 4))
    pts = np.zeros((n, 3, 5))
    bnds_run = np.zeros((n, 3, 2))
    vol_bnds = np.zeros((3, 2))
    for i in range(n):
        d = np.array(Image.open(os.path.join(REF, "data", "frame-%06d.depth.png" % i)))
        depth_im = d.astype(float) / 1000.0
        depth_im[depth_im == 65.535] = 0
        m = int(np.max(np.where(d == 65535, 0, d)))
        assert np.max(depth_im) == m / 1000.0
        max_mm[i] = m
        poses[i] = np.loadtxt(os.path.join(REF, "data", "frame-%06d.pose.txt" % i))
        proxy = np.zeros(d.shape)
        proxy[0, 0] = m / 1000.0
        vfp = grid_fusion.get_view_frustum(proxy, cam_intr, poses[i])
        pts[i] = vfp
        vol_bnds[:, 0] = np.minimum(vol_bnds[:, 0], np.amin(vfp, axis=1))
        vol_bnds[:, 1] = np.maximum(vol_bnds[:, 1], np.amax(vfp, axis=1))
        bnds_run[i] = vol_bnds
    np.savez_compressed(os.path.join(GOLD, "frustum_bounds.npz"), max_depth_mm=max_mm, poses=poses,
                        intr=cam_intr, shape=np.array(d.shape), frustum_pts=pts, bounds_running=bnds_run,
                        bounds=vol_bnds)
    print("frustum bounds", vol_bnds.tolist())


def main():
    if not os.path.isdir(REF):
        print("gen_golden: /root/reference absent; nothing to do")
        return
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tools", "refstubs"), REF])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    env.setdefault("OPENBLAS_NUM_THREADS", "8")
    cmd = [sys.executable, os.path.abspath(__file__), "--inner"] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, env=env, cwd="/tmp").returncode)


if __name__ == "__main__":
    if "--inner" in sys.argv:
        inner()
    else:
        main()
