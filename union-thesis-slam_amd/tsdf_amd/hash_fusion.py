"""Voxel-hash map on MI355X -- drop-in for `hash_fusion.HashTable` (hash_fusion.py:29-507).

The reference hashes single voxels into 5-slot chained buckets and integrates with a Python
loop (hash_fusion.py:134-145, ~45 us per voxel).  Here the map stores 8^3 voxel BLOCKS in an
open-addressed table in HBM: the home slot of a block is the reference's hash_function of the
block coordinates, a wave probes 64 slots per step and inserts with one CAS, and each block's
512 voxels are integrated by one wave (csrc/tsdf_device.h).  What stays the same:

  * hash_function(xyz) returns the reference's value for the same coordinates and table size
    (int64 NumPy arithmetic, or int_bits=32 for the wrapping int32 of the author's run);
  * integrate() updates exactly the voxels the reference updates (the same projection of every
    voxel of the bounded volume), with obs_weight ignored as in hash_fusion.py:141,145, and the
    same weight and colour; tsdf is stored as float32 (the reference keeps a float64 per voxel,
    so tsdf agrees to ~1e-7, inside the 1e-4 parity bound);
  * an "entry" is a voxel that was integrated or added; count_num_hash_entries, get_hash_entry,
    add_hash_entry, remove and double_table_size keep their meaning.

Known, documented differences: add_hash_entry of an existing position finds it
instead of storing a duplicate (hash_map_test.py:68-75 stores 4000 copies of one key); load
factor and collisions are counted over block slots, not 5-voxel buckets.
"""
from __future__ import annotations

import contextlib
import ctypes
import io

import numpy as np

from . import _ffi, grid_fusion
from .data_structures import HashEntry, Voxel
from .grid_fusion import encode_color, encode_depth, volume_geometry

P1 = 73856093
P2 = 19349669
P3 = 83492791


class HashTable:
    """The data structure for voxel storage and retrieval: a GPU hash table of voxel blocks.

    Args as hash_fusion.py:34: vol_bounds (3,2) metres (column 1 rewritten in place),
    voxel_size, map_size (table slots), load_factor / use_gpu (accepted, ignored like the
    reference).  Keyword-only: int_bits (64|32), max_blocks (initial pool size; grows),
    device, shard / n_shards (bucket-range ownership for multi-GPU), defer
    (integrate() collects frames into batches of 8, as TSDFVolume).
    """

    def __init__(self, vol_bounds, voxel_size, map_size=1000000, load_factor=0.75, use_gpu=False,
                 *, int_bits=64, max_blocks=None, device=0, shard=0, n_shards=1, defer=True):
        self._load_factor = 0.75
        self.defer = bool(defer)
        self._vol_bounds, self._vol_dim, self._vol_origin, self._voxel_size = volume_geometry(
            vol_bounds, voxel_size)
        self._trunc_margin = 5 * self._voxel_size
        self._color_const = 256 * 256
        print("Voxel volume size: {} x {} x {} - # points: {:,}".format(
            self._vol_dim[0], self._vol_dim[1], self._vol_dim[2],
            self._vol_dim[0] * self._vol_dim[1] * self._vol_dim[2]))
        self.int_bits = int(int_bits)
        self.device = int(device)
        nb = int(np.prod((np.asarray(self._vol_dim) + 7) // 8))
        if max_blocks is None:
            max_blocks = min(nb, 1 << 16)
        h = ctypes.c_void_p()
        _ffi.call("tsdf_hash_create", _ffi.ptr(np.ascontiguousarray(self._vol_dim, dtype=np.int64)),
                  _ffi.ptr(np.ascontiguousarray(self._vol_origin, dtype=np.float32)),
                  float(self._voxel_size), float(self._trunc_margin), int(map_size),
                  int(max_blocks), self.int_bits, int(shard), int(n_shards), self.device,
                  ctypes.byref(h))
        self._h = h

    # ------------------------------------------------------------------ table geometry
    @property
    def _table_size(self) -> int:
        return self.info()["capacity"]

    def frames_per_launch(self):
        """Frames one launch integrates (the temporal batch, tsdf_hash_frames_per_launch)."""
        if not hasattr(_ffi.load(), "tsdf_hash_frames_per_launch"):  # (an older build under A/B)
            return 8
        n = ctypes.c_int(0)
        _ffi.call("tsdf_hash_frames_per_launch", self._h, ctypes.byref(n))
        return n.value

    def info(self) -> dict:
        s = _ffi.HashInfo()
        _ffi.call("tsdf_hash_info", self._h, ctypes.byref(s))
        return s.as_dict()

    # ------------------------------------------------------------------ integrate
    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1.):
        """hash_fusion.py:103-145 -- obs_weight is ignored exactly like the reference."""
        im_h, im_w = np.shape(depth_im)[:2]
        dk, d = encode_depth(depth_im)
        ck, c = encode_color(color_im)
        K = _ffi.f64(cam_intr, 9)
        Tinv = _ffi.f64(np.linalg.inv(np.asarray(cam_pose, dtype=np.float64)), 16)
        _ffi.call("tsdf_hash_integrate", self._h, _ffi.ptr(d), dk, _ffi.ptr(c), ck, im_h, im_w,
                  _ffi.ptr(K), _ffi.ptr(Tinv), _ffi.DEFER if self.defer else 0)

    def integrate_batch(self, depth, color, cam_intr, world_to_cam, *, depth_kind=None,
                        color_kind=None, hw=None, device_ptrs=False, sync=True, invalid_65535=False):
        """As TSDFVolume.integrate_batch (obs_weight is never forwarded on the hash path)."""
        depth, depth_kind, color, color_kind = grid_fusion.frame_stack(depth, depth_kind, color, color_kind,
                                                                      device_ptrs)
        T = np.ascontiguousarray(np.asarray(world_to_cam, dtype=np.float64).reshape(-1, 16))
        H, W = hw if (device_ptrs or isinstance(depth, int)) else np.shape(depth)[1:3]
        flags = ((_ffi.DEVICE_PTRS if device_ptrs else 0) | (0 if sync else _ffi.ASYNC) |
                 (_ffi.DEPTH_INVALID_65535 if invalid_65535 else 0))
        _ffi.call("tsdf_hash_integrate_batch", self._h, T.shape[0], _ffi.ptr(depth), depth_kind,
                  _ffi.ptr(color), color_kind, int(H), int(W), _ffi.ptr(_ffi.f64(cam_intr, 9)),
                  _ffi.ptr(T), flags)

    # ------------------------------------------------------------------ statistics
    def count_num_hash_entries(self) -> int:
        return int(self.info()["entries"])

    def get_num_non_empty_bucket(self) -> int:
        return int(self.info()["used"])

    get_num_non_empty_buckets = get_num_non_empty_bucket

    def needs_resize(self) -> bool:
        i = self.info()
        return i["used"] / i["capacity"] >= self._load_factor

    def get_load_factor(self) -> float:
        i = self.info()
        return i["used"] / i["capacity"]

    def get_num_collisions(self) -> int:
        """Block keys displaced from their home slot (the open-addressing analogue of the
        reference's 'buckets holding more than one entry', hash_fusion.py:169-180)."""
        return int(self.info()["displaced"])

    # ------------------------------------------------------------------ keys
    def hash_function(self, world_coord):
        """hash_fusion.py:182-190 for one coordinate triple (computed on the device)."""
        return int(self.hash_keys(np.asarray(world_coord, dtype=np.int64).reshape(1, 3))[0])

    def hash_keys(self, coords, table_size=None):
        xyz = np.ascontiguousarray(np.asarray(coords, dtype=np.int64).reshape(-1, 3))
        out = np.empty(xyz.shape[0], np.int64)
        n = self._table_size if table_size is None else int(table_size)
        _ffi.call("tsdf_hash_keys", _ffi.ptr(xyz), xyz.shape[0], n, self.int_bits, _ffi.ptr(out),
                  self.device)
        return out

    # ------------------------------------------------------------------ entries
    @staticmethod
    def _ijk(positions):
        return np.ascontiguousarray(np.asarray(positions, dtype=np.int64).reshape(-1, 3))

    def add_voxel(self, voxel, world_coord):
        self.add_hash_entry(HashEntry(world_coord, None, voxel))

    def add_hash_entry(self, hash_entry):
        """Insert the entry's voxel; returns (table slot, voxel-in-block) -- the reference's
        (bucket, slot) -- or (-1, -1) for None."""
        if hash_entry is None:
            return -1, -1
        ijk = self._ijk(hash_entry.get_position())
        v = hash_entry.get_voxel()
        vals = [None, None, None]
        if v is not None and v.get_sdf() is not None:
            vals = [np.array([float(v.get_sdf())], np.float32), np.array([float(v.get_weight())], np.float32),
                    np.array([float(v.get_color())], np.float32)]
        slot = np.empty(1, np.int64)
        local = np.empty(1, np.int32)
        _ffi.call("tsdf_hash_insert", self._h, _ffi.ptr(ijk), 1, *[_ffi.ptr(a) for a in vals],
                  _ffi.ptr(slot), _ffi.ptr(local))
        hash_entry.set_offset((int(slot[0]), int(local[0])))
        return int(slot[0]), int(local[0])

    def add_entries(self, positions, tsdf=None, weight=None, color=None):
        """Batched add_hash_entry: (n,3) voxel indices, optional per-voxel values."""
        ijk = self._ijk(positions)
        n = ijk.shape[0]
        arr = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(n))
               for a in (tsdf, weight, color)]
        slot = np.empty(n, np.int64)
        local = np.empty(n, np.int32)
        _ffi.call("tsdf_hash_insert", self._h, _ffi.ptr(ijk), n, *[_ffi.ptr(a) for a in arr],
                  _ffi.ptr(slot), _ffi.ptr(local))
        return slot, local

    def lookup(self, positions):
        """Batched get_hash_entry: (found bool, tsdf, weight, colour) arrays."""
        ijk = self._ijk(positions)
        n = ijk.shape[0]
        t, w, c = (np.empty(n, np.float32) for _ in range(3))
        f = np.empty(n, np.uint8)
        _ffi.call("tsdf_hash_lookup", self._h, _ffi.ptr(ijk), n, _ffi.ptr(t), _ffi.ptr(w),
                  _ffi.ptr(c), _ffi.ptr(f))
        return f.astype(bool), t, w, c

    def get_hash_entry(self, world_coord):
        found, t, w, c = self.lookup(world_coord)
        if not found[0]:
            return None
        return HashEntry(list(np.asarray(world_coord).reshape(3)), None,
                         Voxel(float(t[0]), float(c[0]), float(w[0])))

    def get_voxel(self, world_coord):
        e = self.get_hash_entry(world_coord)
        return None if e is None else e.get_voxel()

    def remove_entries(self, positions):
        ijk = self._ijk(positions)
        r = np.empty(ijk.shape[0], np.uint8)
        _ffi.call("tsdf_hash_remove", self._h, _ffi.ptr(ijk), ijk.shape[0], _ffi.ptr(r))
        return r.astype(bool)

    def remove(self, world_coord):
        self.remove_hash_entry(HashEntry(world_coord, None, None))

    def remove_hash_entry(self, hash_entry):
        """1 if removed, 0 if absent (hash_fusion.py:330-385)."""
        return int(self.remove_entries(hash_entry.get_position())[0])

    def double_table_size(self):
        n = self._table_size
        print("Resizing hash table from {} to {}".format(n, n * 2))
        _ffi.call("tsdf_hash_resize", self._h, 2 * n)
        print("Resize finished.")

    # ------------------------------------------------------------------ sparse block transfer
    def export_blocks(self, device=None):
        """Live blocks: (bxyz (n,3) int32, tsdf, weight, colour (n,512) float32 in brick-local order,
        occ (n,8) uint64 entry words) as numpy arrays, or as CUDA tensors on `device`."""
        n = ctypes.c_int64(0)
        _ffi.call("tsdf_hash_export_blocks", self._h, None, None, None, None, None, ctypes.byref(n), 0)
        nb = n.value
        if device is not None:
            import torch
            out = (torch.empty((nb, 3), dtype=torch.int32, device=device),
                   *(torch.empty((nb, 512), dtype=torch.float32, device=device) for _ in range(3)),
                   torch.empty((nb, 8), dtype=torch.int64, device=device))
            if nb:
                _ffi.call("tsdf_hash_export_blocks", self._h, *[o.data_ptr() for o in out], ctypes.byref(n),
                          _ffi.DEVICE_PTRS)
            return out
        out = (np.empty((nb, 3), np.int32), *(np.empty((nb, 512), np.float32) for _ in range(3)),
               np.empty((nb, 8), np.uint64))
        if nb:
            _ffi.call("tsdf_hash_export_blocks", self._h, *[_ffi.ptr(o) for o in out], ctypes.byref(n), 0)
        return out

    def import_blocks(self, bxyz, tsdf, weight, color, occ=None):
        """Insert / overwrite whole blocks (numpy arrays or CUDA tensors, as export_blocks)."""
        dev = not isinstance(bxyz, np.ndarray)
        n = int(bxyz.shape[0])
        if n == 0:
            return
        if dev:
            # the contiguous copies must outlive the call (a temporary's memory could be reused
            # before the library reads it)
            keep = [None if a is None else a.contiguous() for a in (bxyz, tsdf, weight, color, occ)]
            ptrs = [None if a is None else a.data_ptr() for a in keep]
        else:
            arrs = [np.ascontiguousarray(bxyz, np.int32)] + [
                None if a is None else np.ascontiguousarray(a, np.float32) for a in (tsdf, weight, color)] + [
                None if occ is None else np.ascontiguousarray(occ, np.uint64)]
            ptrs = [_ffi.ptr(a) for a in arrs]
        _ffi.call("tsdf_hash_import_blocks", self._h, ptrs[0], n, ptrs[1], ptrs[2], ptrs[3], ptrs[4],
                  _ffi.DEVICE_PTRS if dev else 0)
        if dev:
            del keep

    # ------------------------------------------------------------------ export
    def get_volume(self):
        """hash_fusion.py:442-463: dense (tsdf, colour) float32 arrays of vol_dim."""
        t, _, c = self.get_state(weight=False)
        return t, c

    def get_state(self, weight=True):
        shape = tuple(int(x) for x in self._vol_dim)
        t = np.empty(shape, np.float32)
        w = np.empty(shape, np.float32) if weight else None
        c = np.empty(shape, np.float32)
        _ffi.call("tsdf_hash_get_dense", self._h, _ffi.ptr(t), _ffi.ptr(w), _ffi.ptr(c))
        return t, w, c

    def _as_grid(self):
        """The densified volume (get_volume, hash_fusion.py:442-463) in a dense device handle,
        filled on the device from the live blocks (tsdf_hash_to_dense: no host round trip).  Costs
        the whole extent; get_mesh / get_point_cloud do not use it (extract_mesh)."""
        lo = np.asarray(self._vol_bounds, dtype=np.float64)[:, 0]
        bnds = np.stack([lo, lo + (np.asarray(self._vol_dim) - 0.5) * self._voxel_size], axis=1)  # same dims
        with contextlib.redirect_stdout(io.StringIO()):
            vol = grid_fusion.TSDFVolume(bnds, self._voxel_size, device=self.device)
        _ffi.call("tsdf_hash_to_dense", self._h, vol._h)
        return vol

    def raycast(self, cam_intr, cam_pose, hw, *, z_near=0.0, z_far=None, z_step=None, normals=True,
                colors=True, out=None):
        """As TSDFVolume.raycast, on the table (tsdf_hash_raycast): the raycast of get_volume()'s
        densified volume, without densifying."""
        return grid_fusion.raycast_call("tsdf_hash_raycast", self._h, self.device, self._vol_bounds, self._voxel_size,
                                        cam_intr, cam_pose, hw, z_near, z_far, z_step, normals, colors, out)

    def track(self, depth_im, cam_intr, pose_guess, *, dist_max=0.1, angle_max_deg=30.0, stride=1, max_iter=10,
              min_inliers=100, eps_rot=1e-5, eps_trans=1e-5, z_near=0.0, z_far=None, z_step=None,
              return_info=False, invalid_65535=False, color_im=None, color_weight=0.001, color_max_diff=40.0,
              method="icp"):
        """As TSDFVolume.track, against the table's raycast (tsdf_hash_track), or with method="sdf"
        against the table's blocks themselves (tsdf_hash_track_sdf)."""
        from . import tracking
        return tracking.track_call("tsdf_hash_track", self._h, self._vol_bounds, self._voxel_size, depth_im, cam_intr,
                                   pose_guess, dist_max, angle_max_deg, stride, max_iter, min_inliers, eps_rot,
                                   eps_trans, z_near, z_far, z_step, return_info, invalid_65535, color_im,
                                   color_weight, color_max_diff, method)

    def sample(self, points):
        """The fused signed distance at world points (N,3) (tsdf_hash_sample): (sdf (N,) f32
        metres, grad (N,3) f32 -- the gradient of the trilinear interpolant, metres per metre, not
        normalised, towards positive tsdf --, code (N,) u8: 2 the 8 voxels around the point are not
        all inside the volume, 3 one of them was never observed, 4 one lies on the truncated
        plateau (the value is then no distance), 6 a distance).  Value and gradient are 0 for codes
        2 and 3.  Arrays for an array, CUDA tensors for a contiguous float64 CUDA tensor."""
        from . import tracking
        return tracking.sample_call("tsdf_hash_sample", self._h, self.device, points)

    def merge(self, other, src_to_dst=np.eye(4), return_info=False):
        """TSDFVolume.merge into this table (tsdf_hash_merge): every sampled voxel receives
        an entry, and exactly the blocks with a sample are allocated (the table and the pool grow as
        needed)."""
        return grid_fusion.merge_call("tsdf_hash_merge", self._h, other, src_to_dst, return_info)

    def extract_mesh(self, normals=True, colors=True, faces=True, keys=False):
        """Marching cubes at level 0 over the table's live blocks (tsdf_hash_extract_mesh): the
        mesh of get_state()'s volume, byte for byte what _as_grid().extract_mesh() gives, without
        a dense volume.  Returns as TSDFVolume.extract_mesh: (verts (N,3) f32 world, normals (N,3)
        f32, colors (N,3) u8, faces (M,3) i32[, keys (N,) int64]); a field not asked for is None,
        and normals and faces not asked for are not computed either."""
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        fields = (_ffi.MESH_NORMALS if normals else 0) | (_ffi.MESH_FACES if faces else 0)
        _ffi.call("tsdf_hash_extract_mesh_fields", self._h, fields, ctypes.byref(nv), ctypes.byref(nt))
        v = np.empty((nv.value, 3), np.float32)
        n = np.empty((nv.value, 3), np.float32) if normals else None
        c = np.empty((nv.value, 3), np.uint8) if colors else None
        f = np.empty((nt.value, 3), np.int32) if faces else None
        _ffi.call("tsdf_hash_get_mesh", self._h, _ffi.ptr(v), _ffi.ptr(n), _ffi.ptr(c), _ffi.ptr(f))
        if not keys:
            return v, n, c, f
        k = np.empty(nv.value, np.int64)
        _ffi.call("tsdf_hash_get_mesh_keys", self._h, _ffi.ptr(k))
        return v, n, c, f, k

    def mesh_info(self) -> dict:
        """The last extract_mesh: live_blocks, mesh_blocks (block coordinates meshed), scratch_bytes
        (every device allocation it made, the mesh included), n_verts, n_tris."""
        s = _ffi.HashMeshInfo()
        _ffi.call("tsdf_hash_mesh_info", self._h, ctypes.byref(s))
        return s.as_dict()

    def get_mesh(self):
        """hash_fusion.py:465-484: (verts, faces, norms, colors), marching cubes of the table's
        blocks on the device (the mesh of the densified volume, without densifying)."""
        v, n, c, f = self.extract_mesh()
        return v, f, n, c

    def get_point_cloud(self):
        """hash_fusion.py:486-507: (N, 6) float32 rows x, y, z, r, g, b of the mesh vertices."""
        v, _, c, _ = self.extract_mesh(normals=False, faces=False)
        return np.hstack([v, c])

    # ------------------------------------------------------------------ misc
    def sync(self):
        _ffi.call("tsdf_hash_sync", self._h)

    def trim(self):
        """Hand the block pool's memory above the live blocks back (tsdf_hash_trim: a compaction
        into fresh mapped ranges, one device copy of the live state).  Explicit only -- exports
        (get_volume / get_state / get_mesh) do not trim, so periodic extraction during a run does
        not shrink a pool the next integrate must grow again."""
        _ffi.call("tsdf_hash_trim", self._h)

    def stats(self, reset=False):
        s = _ffi.Stats()
        _ffi.call("tsdf_hash_stats", self._h, ctypes.byref(s), int(bool(reset)))
        return s.as_dict()

    def set_profiling(self, on=True):
        _ffi.call("tsdf_hash_set_profiling", self._h, int(bool(on)))

    def reset(self):
        _ffi.call("tsdf_hash_reset", self._h)

    def close(self):
        if getattr(self, "_h", None):
            _ffi.call("tsdf_hash_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
