/*
 * tsdf_hip.h -- C-ABI of the MI355X (gfx950) TSDF fusion hot path.
 *
 * The drop-in boundary for DiWu9/Union-Thesis-SLAM's integrate path: the reference binds its
 * device code from Python (PyCUDA SourceModule, grid_fusion.py:69-144, launched at :234-259);
 * this library is bound the same way, from Python, through ctypes
 * (union-thesis-slam_amd/tsdf_amd/_ffi.py).  Plain C types only: pointers, sizes, doubles.
 *
 * Conventions
 *   - Every function returns int: 0 = ok, negative = TSDF_E_* code; tsdf_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - A handle owns all of its device memory and one HIP stream on its device.  Host pointers
 *     are borrowed for the duration of the call only and must be C-contiguous.
 *   - Calls are synchronous (stream-synchronised before return) unless TSDF_ASYNC is passed;
 *     then the caller synchronises with tsdf_*_sync().  One handle per host thread.
 *   - Pointer residence is given per call by TSDF_DEVICE_PTRS: without it depth/colour are host
 *     pointers (copied H2D by the call); with it they are device pointers already in HBM.
 *   - Volumes are indexed like the reference: voxel (x, y, z), C-order (X, Y, Z), z fastest
 *     (grid_fusion.py:52-55,158-168).  The state lives in HBM as 8x8x8 bricks;
 *     the get/extract calls return C-order arrays.
 */
#ifndef TSDF_HIP_H
#define TSDF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------------------------ */
#define TSDF_OK 0
#define TSDF_E_ARG -1       /* invalid argument (shape, kind, null pointer) */
#define TSDF_E_HIP -2       /* a HIP runtime call failed (message has the HIP error string) */
#define TSDF_E_NODEV -3     /* no usable gfx950 device */
#define TSDF_E_CAPACITY -4  /* hash table / block pool full and could not grow */
#define TSDF_E_OOM -5       /* device allocation failed */

/* ---- input kinds and flags ---------------------------------------------------------------- */
#define TSDF_DEPTH_U16_MM 0 /* uint16 millimetres: metres = (double)mm / 1000.0 (grid_demo1.py:81-82) */
#define TSDF_DEPTH_F64_M 1  /* float64 metres, as handed to integrate() (grid_fusion.py:214) */
#define TSDF_COLOR_RGB8 0   /* uint8 (H,W,3) RGB; folded B*65536+G*256+R (grid_fusion.py:228-232) */
#define TSDF_COLOR_F32 1    /* float32 (H,W) already folded by the caller */

#define TSDF_DEVICE_PTRS 1  /* depth/colour pointers are device pointers */
#define TSDF_ASYNC 2        /* do not synchronise the handle's stream before returning */
#define TSDF_DEPTH_INVALID_65535 4 /* u16 depth: 65535 mm is invalid (0), the 7-Scenes convention
                                      of the demos (grid_demo1.py:82: depth_im[depth_im == 65.535] = 0) */
#define TSDF_DEFER 8        /* tsdf_*_integrate (host frames only): copy the frame into a pinned
                               staging batch and return; the batch runs (asynchronously, as one
                               temporally batched launch) once it holds 8 frames
                               (TSDF_DEFER_FRAMES overrides; a quarter of a 32-frame
                               launch, the host's copy grain) or at the next other call
                               on the handle -- the reference's one-integrate()-per-
                               frame loop (grid_demo1.py:76-87) at batched speed, same results.
                               f64-metre depth whose every value is exactly RN(k / 1000),
                               k < 65536 integer (png / 1000.), is staged as u16 millimetres.
                               Hash: a full table / pool found after a deferred batch is grown
                               and its skipped bricks re-run at the next call, before anything
                               else runs (exact, as for synchronous calls) */

#define TSDF_RAY_REFLAG 16  /* tsdf_*_raycast: recompute the live-brick bits even though the handle's
                               state has not changed since they were computed (timing tools) */

typedef struct tsdf_dense tsdf_dense_t;
typedef struct tsdf_hash tsdf_hash_t;

/* ---- tracking ------------------------------------------------------------- */
#define TSDF_ICP_MAX_ITER 64    /* the cap on tsdf_icp_params_t.max_iter */
#define TSDF_TRACK_CONVERGED 1  /* an update had |w| <= eps_rot and |t| <= eps_trans */
#define TSDF_TRACK_MAX_ITER 2   /* max_iter updates were applied and none was that small */
#define TSDF_TRACK_LOST 3       /* an iteration found fewer than min_inliers inliers, or a system that
                                   is not positive definite; the pose is that of the iteration before */

/* Parameters of the point-to-plane ICP.  The defaults of the Python wrappers: 0.1 m, cos 30 deg,
 * stride 1, 10 iterations, 100 inliers, 1e-5 rad, 1e-5 m. */
typedef struct {
    double dist_max;      /* m: a pair further apart is no inlier (> 0) */
    double cos_min;       /* the least cosine between the frame's and the model's normal ([-1, 1]) */
    int32_t stride;       /* only pixels with u % stride == 0 and v % stride == 0 are sampled (>= 1) */
    int32_t max_iter;     /* 1 .. TSDF_ICP_MAX_ITER */
    int64_t min_inliers;  /* fewer inliers: lost */
    double eps_rot;       /* rad */
    double eps_trans;     /* m */
} tsdf_icp_params_t;

typedef struct {
    int32_t status;      /* TSDF_TRACK_* */
    int32_t iterations;  /* linearisations run (a lost one included) */
    int64_t inliers;     /* of the last linearisation */
    int64_t candidates;  /* of the last linearisation: pixels with a vertex and a normal (codes 2..6) */
    double rms;          /* sqrt(sum r^2 / inliers) of the last linearisation, metres */
    double w_norm;       /* |w| and |t| of the last update (0 after a lost iteration) */
    double t_norm;
} tsdf_track_info_t;

/* The photometric term of the RGB-D entry points.  The defaults of the Python
 * wrappers: 0.001 m per level, 40 levels. */
typedef struct {
    double color_weight;   /* lambda, metres per intensity level: A = A_g + lambda^2 A_c (finite, >= 0;
                              0: the colour sums are formed and contribute exactly nothing) */
    float color_max_diff;  /* intensity levels: a pixel whose residual is larger is no colour inlier (> 0) */
} tsdf_icp_color_params_t;

/* What an RGB-D track reports besides tsdf_track_info_t, of the last linearisation. */
typedef struct {
    int64_t color_inliers;     /* colour code 5 */
    int64_t color_candidates;  /* colour codes 2..5: pixels whose footprint lies inside the model image */
    double color_rms;          /* sqrt(sum r^2 / color_inliers), intensity levels */
} tsdf_track_color_info_t;

/* Cumulative counters since create/reset (or the last tsdf_*_stats call with reset != 0). */
typedef struct {
    int64_t frames;           /* frames integrated */
    int64_t voxel_updates;    /* sum over frames of V_f (voxels whose tsdf/weight/colour changed) */
    int64_t bricks_visited;   /* bricks that passed the conservative frustum/depth cull */
    int64_t bricks_touched;   /* bricks with >= 1 updated voxel, summed over launches; the fused
                                 launches count each z-half wave that updated a voxel (up to two
                                 per brick) -- per-block counts: lookups */
    int64_t blocks_allocated; /* hash: blocks newly allocated */
    int64_t probe_steps;      /* hash: total linear-probe distance of block lookups */
    int64_t probe_max;        /* hash: longest probe distance seen */
    int64_t lookups;          /* hash: block lookups performed (fused launches: one per kept
                                 block per launch, by the cull's find-or-insert) */
    double kernel_ms;         /* integrate-kernel time from HIP events (profiling on only) */
    int64_t kernel_launches;  /* integrate-kernel launches timed */
    int64_t bricks_skipped;   /* hash: bricks a launch skipped for lack of table/pool space --
                                 re-run exactly after growing by a synchronous call (and counted
                                 here), reported as TSDF_E_CAPACITY by an asynchronous one; see
                                 tsdf_hash_integrate_batch */
    int64_t list_errors;      /* brick-list entries out of range, dropped by the integrate kernel
                                 (always 0 unless device memory was corrupted) */
    int64_t batch_voxels;     /* sum over launches of U_batch: the voxels updated at least once by
                                 the launch's temporal batch (<= voxel_updates; each such voxel's
                                 state is read and written once per launch -- the roofline's bytes) */
} tsdf_stats_t;

typedef struct {
    int64_t capacity;         /* the table size of the API (map_size: hash_function's modulus, doubled
                                 by double_table_size and the 0.75 load-factor policy) */
    int64_t used;             /* live block keys */
    int64_t tombstones;       /* removed keys not yet reclaimed by a rehash */
    int64_t displaced;        /* live keys not in their home slot ("collisions") */
    int64_t max_probe;        /* longest home-to-slot distance of a live key */
    int64_t blocks_in_pool;   /* blocks handed out by the pool (live + free list) */
    int64_t pool_capacity;    /* blocks the pool can hold before it must grow */
    int64_t entries;          /* voxel entries (occupancy bits set), = count_num_hash_entries */
    int64_t slots;            /* slots of the open-addressed device table: the power of two >= capacity */
    int64_t pool_mapped;      /* 1: the pool lives on reserved address ranges grown by mapping (VMM);
                                 0: plain allocations grown by copy */
} tsdf_hash_info_t;

/* The last tsdf_hash_extract_mesh of a table (tsdf_hash_mesh_info). */
typedef struct {
    int64_t live_blocks;      /* live blocks inside the volume that the extraction read */
    int64_t mesh_blocks;      /* block coordinates it meshed: those with a live block among b + {0,1}^3
                                 (live_blocks <= mesh_blocks <= 8 * live_blocks) */
    int64_t scratch_bytes;    /* sum of every device allocation it made, the mesh itself included */
    int64_t n_verts, n_tris;
} tsdf_hash_mesh_info_t;

/* What tsdf_hash_extract_mesh_fields extracts beside vertices, colours and keys. */
#define TSDF_MESH_NORMALS 1
#define TSDF_MESH_FACES 2

const char* tsdf_last_error(void);
/* Build id of the loaded library: the first 16 hex digits of the sha256 of the sources it was
 * compiled from (csrc/, this header, the Makefile).  Profiles under profiles/ record the id of
 * the library they measured; bench.py quotes a profile's counters only for the same id. */
const char* tsdf_build_id(void);
int tsdf_device_count(int* n);

/* ---- dense grid: replaces TSDFVolume (grid_fusion.py:19-320) ------------------------------
 * dims: voxels of THIS shard; index_offset: global voxel index of its (0,0,0) (slab sharding:
 * world coordinates are always computed from the global index, so a slab is bit-identical to
 * the same voxels of an unsharded volume).  origin = f32(vol_bnds[:,0]) (grid_fusion.py:44),
 * trunc = 5 * voxel_size (grid_fusion.py:37). */
int tsdf_dense_create(const int64_t dims[3], const int64_t index_offset[3], const float origin[3],
                      double voxel_size, double trunc, int device, tsdf_dense_t** out);
/* Cyclic brick-column shard of a volume of global_dims voxels: shard s of n owns
 * the 8-voxel x-columns c with c % 2n in {s, 2n-1-s} (mirrored pairs), stored contiguously in
 * local x order, so every rank sees a similar share of each frame's frustum.  The shard's local dims are
 * (sum of its column widths, Y, Z); tsdf_dense_get/set use that local C-order.  n_shards = 1
 * is tsdf_dense_create with a zero offset.  Replaces the same constructor as above. */
int tsdf_dense_create_shard(const int64_t global_dims[3], int shard, int n_shards,
                            const float origin[3], double voxel_size, double trunc, int device,
                            tsdf_dense_t** out);
int tsdf_dense_destroy(tsdf_dense_t* h);
int tsdf_dense_reset(tsdf_dense_t* h); /* tsdf = 1, weight = 0, colour = 0 (grid_fusion.py:52-55) */

/* One frame: TSDFVolume.integrate(color_im, depth_im, cam_intr, cam_pose, obs_weight)
 * (grid_fusion.py:214-314).  K: the 3x3 intrinsics as given (row-major float64); the kernel uses
 * f64(f32(K)) like cam2pix (:190).  world_to_cam: np.linalg.inv(cam_pose) computed by the
 * caller (:265), row-major 4x4 float64.  Images: height, width < 2^24 and height*width < 2^28
 * (the gathers use 32-bit byte offsets), else TSDF_E_ARG. */
int tsdf_dense_integrate(tsdf_dense_t* h, const void* depth, int depth_kind, const void* color,
                         int color_kind, int height, int width, const double K[9],
                         const double world_to_cam[16], double obs_weight, int flags);

/* F frames back to back on the handle's stream (the bench's step).  depth/color point at F
 * consecutive frames (frame stride = H*W elements); world_to_cam: F*16 doubles (host);
 * obs_weight: F doubles (host) or NULL for all 1.0. */
int tsdf_dense_integrate_batch(tsdf_dense_t* h, int n_frames, const void* depth, int depth_kind,
                               const void* color, int color_kind, int height, int width,
                               const double K[9], const double* world_to_cam,
                               const double* obs_weight, int flags);

/* get_volume (grid_fusion.py:316-320) plus weight: C-order (X,Y,Z) float32 host arrays of
 * this shard; any pointer may be NULL to skip that field. */
int tsdf_dense_get(tsdf_dense_t* h, float* tsdf, float* weight, float* color);
int tsdf_dense_set(tsdf_dense_t* h, const float* tsdf, const float* weight, const float* color);
int tsdf_dense_sync(tsdf_dense_t* h);
/* Frames one launch integrates (the temporal batch: 32 in this build, 16 or 8 with -DTSDF_MAX_BATCH;
 * TSDF_BATCH overrides per process); calls of n frames run ceil(n / batch) + 2 pipelined launches. */
int tsdf_dense_frames_per_launch(tsdf_dense_t* h, int* n);
/* Mesh of the shard's tsdf at level 0 (get_mesh / get_point_cloud, grid_fusion.py:322-360; the
 * reference runs skimage's marching_cubes_lewiner on the host).  extract runs marching cubes on
 * the device and keeps the result in the handle; get_mesh copies it out: verts n_verts x 3 f32
 * world coordinates (index-space vertex * voxel_size + origin, in f32 like NumPy), normals
 * n_verts x 3 f32 unit (towards positive tsdf), colors n_verts x 3 uint8 r, g, b of the voxel at
 * round(vertex) (grid_fusion.py:336-346), faces n_tris x 3 int32 vertex ids.  One vertex per
 * grid edge whose end values straddle 0 (one below 0, one not), at the linear interpolation;
 * vertices ordered by (voxel, axis) in C-order and shared by the cells around the edge.  Any
 * output pointer may be NULL.  Vertex world x comes from the GLOBAL voxel index, so a slab
 * shard meshed alone gives the mesh of its own sub-volume in world coordinates; a cyclic column
 * shard needs its neighbours' border rows (tsdf_dense_extract_mesh_halo), else TSDF_E_ARG. */
int tsdf_dense_extract_mesh(tsdf_dense_t* h, int64_t* n_verts, int64_t* n_tris);
int tsdf_dense_get_mesh(tsdf_dense_t* h, float* verts, float* normals, uint8_t* colors, int32_t* faces);
/* Sharded marching cubes.  mesh_halo_rows: the global x rows (sorted) of the
 * unsharded volume (x extent global_x) that this shard's cells and gradients read but do not
 * own; with rows == NULL only *n_rows is set, else rows must hold *n_rows >= that many.
 * extract_mesh_halo: marching cubes over the cells anchored at the shard's own rows, given those
 * rows (halo_gx[n_halo] global x, halo_tsdf / halo_color n_halo x Y x Z C-order float32; host, or
 * device with TSDF_DEVICE_PTRS).  The shard's mesh holds its own cells' triangles and every
 * vertex they use, including copies of the next shard's border vertices; get_mesh_keys gives
 * each vertex's global identity ((x*Y + y)*Z + z)*3 + axis, the order of the unsharded mesh,
 * so the union of the shards' meshes, vertices merged by key, is the unsharded mesh. */
int tsdf_dense_mesh_halo_rows(tsdf_dense_t* h, int64_t global_x, int64_t* rows, int64_t* n_rows);
int tsdf_dense_extract_mesh_halo(tsdf_dense_t* h, int64_t global_x, const int64_t* halo_gx, int64_t n_halo,
                                 const float* halo_tsdf, const float* halo_color, int flags, int64_t* n_verts,
                                 int64_t* n_tris);
int tsdf_dense_get_mesh_keys(tsdf_dense_t* h, int64_t* keys);
/* Local x rows (rows[n_rows], local indices) of the shard in C-order (n_rows, Y, Z) float32 -- the
 * halo rows another shard needs and the rows of a device-side gather (get_volume of a sharded
 * volume).  Host pointers, or device pointers with TSDF_DEVICE_PTRS; NULL skips a field. */
int tsdf_dense_get_rows(tsdf_dense_t* h, const int64_t* rows, int64_t n_rows, float* tsdf, float* weight,
                        float* color, int flags);
/* The marching-cubes case table in use: tri[256][16] cube-edge ids (-1 padded; edge e joins the
 * corners differing in bit e / 4 of the corner index, its lower corner's other two bits being
 * e % 4 in increasing bit order), ntri[256] triangles per case.  Host-only; no device needed. */
int tsdf_mc_table(int8_t* tri, uint8_t* ntri);
/* Raycast of the fused model (not in the reference): what the volume looks like from
 * cam_pose (camera-to-world, row-major 4x4 f64, as integrate() takes it) through K, for an image of
 * height x width pixels (the image limits of tsdf_dense_integrate).  Along the ray of pixel (u, v)
 * the samples k = 0, 1, ... lie at camera depth z_k = z_near + k * z_step <= z_far, at the world
 * point cam_pose * ((u - cx) / fx * z_k, (v - cy) / fy * z_k, z_k).  A sample is valid when the 8
 * voxels around it (voxel centres at integer indices of the GLOBAL lattice) are inside this handle's
 * volume and all have weight > 0; its value f is their trilinear tsdf.  The first k >= 1 that is
 * valid with f_k < 0 decides the ray: a hit when sample k - 1 is valid with f_{k-1} > 0, else a miss
 * (surface met from behind or from unseen space); no such k is a miss.  For a hit
 *   depth   H x W f32: z_{k-1} + z_step * f_{k-1} / (f_{k-1} - f_k), metres along the camera z axis
 *           (a depth image, as integrate() reads it);
 *   normals H x W x 3 f32: unit gradient of the trilinear interpolant in the cell of the hit point,
 *           world axes, towards positive tsdf; 0 if that cell is not valid;
 *   colors  H x W x 3 u8: r, g, b of the voxel nearest the hit point (the rule of the mesh vertices);
 * a miss writes 0 everywhere.  Any output pointer may be NULL.  Host pointers, or device pointers
 * with TSDF_DEVICE_PTRS (then TSDF_ASYNC leaves the result to the handle's stream).  Deferred frames
 * run first; the call follows the launches in flight on the handle's stream.  Space is skipped by
 * one live bit per brick, recomputed only after a call that changed the state; the result is that
 * of evaluating every sample (TSDF_RAY_SKIP=0 in the environment at create does exactly that).
 * The arithmetic is fixed (per-ray setup in f64 rounded once to f32, the march in f32) and restated
 * by tests/raycast_ref.py.  TSDF_E_ARG: z_step <= 0, z_far < z_near, z_near < 0, more than 2^22
 * samples per ray, a bad image size, a cyclic column shard.  Slab shards (index_offset) raycast
 * their own voxels. */
int tsdf_dense_raycast(tsdf_dense_t* h, int height, int width, const double K[9],
                       const double cam_pose[16], double z_near, double z_far, double z_step,
                       float* depth, float* normals, uint8_t* colors, int flags);
/* Track a depth frame against the fused model (not in the reference): frame-to-model
 * point-to-plane ICP, single resolution, geometry only (tsdf_dense_track_rgbd adds colour;
 * tsdf_dense_track_sdf aligns to the volume without a raycast).  The model maps are this handle's own
 * raycast (depth and normals, height x width through K, with z_near / z_far / z_step as there) at
 * pose_guess (camera-to-world); the frame (depth of depth_kind, height x width through the same K;
 * TSDF_DEPTH_INVALID_65535 is honoured; a host pointer, or a device pointer with TSDF_DEVICE_PTRS)
 * is aligned to them starting from the relative pose M_0 = I, for at most params->max_iter
 * iterations of linearise (tsdf_icp_linearize's arithmetic), solve and M <- E(xi) M, all queued on
 * the handle's stream and run without a host synchronisation in between; the call then synchronises
 * once and copies the iterations' records back once (TSDF_ASYNC is accepted and changes nothing:
 * the result is a host value).  out_pose = pose_guess * M in f64.  info (may be NULL) describes the
 * end; trajectory (may be NULL) receives (max_iter + 1) x 16 doubles: M_0 = I, then M after each
 * iteration run (a lost iteration repeats its predecessor), zeros beyond.  Deferred frames run
 * first.  A lost track is no error: the call returns 0, info->status is TSDF_TRACK_LOST and
 * out_pose is the last good pose (pose_guess when the first iteration was lost).  Two calls on the
 * same state and inputs give byte-identical results (no floating-point atomics).  TSDF_E_ARG:
 * stride < 1, max_iter outside [1, TSDF_ICP_MAX_ITER], dist_max <= 0, cos_min outside [-1, 1],
 * a negative min_inliers / eps, a bad image size or depth_kind, a NULL depth / K / pose_guess /
 * params / out_pose, a pose_guess whose rotation block is not orthonormal with determinant +1
 * within 1e-3 (a scaled, sheared, mirrored, zero or NaN rotation: such a guess makes systems of
 * condition 1e15 and steps of kilometres; a pose read from text with eight digits passes; the
 * translation is not looked at, a NaN or infinite one ends lost), and whatever the raycast refuses
 * (its z arguments, a cyclic column shard).  A refused call writes to none of its outputs.  The
 * _rgbd, _sdf and hash entry points refuse the same. */
int tsdf_dense_track(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width,
                     const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                     double z_near, double z_far, double z_step, double out_pose[16],
                     tsdf_track_info_t* info, double* trajectory, int flags);
/* Track a depth frame against the volume itself (Bylow et al., RSS 2013): point-to-SDF
 * alignment.  The stored tsdf is a signed distance field, so the frame's points are aligned to it
 * directly: minimise the sum of sdf(pose_guess * M * p)^2 with the trilinear interpolant of the
 * stored tsdf and its gradient.  No raycast is queued, no live bits are computed and no model maps
 * are allocated; no frame normal is needed, so the last row and column take part.  Arguments, the
 * iteration (linearise, solve, M <- E(xi) M from M_0 = I, one synchronisation), out_pose, info,
 * trajectory, lost, flags and determinism are tsdf_dense_track's, without the z range; one
 * linearisation is tsdf_dense_sdf_linearize's.  params->cos_min is validated and otherwise unused.
 * With profiling on, tsdf_track_last_ms reports 0 for the raycast.  TSDF_E_ARG: what
 * tsdf_dense_track refuses, but for the z arguments. */
int tsdf_dense_track_sdf(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width,
                         const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                         double out_pose[16], tsdf_track_info_t* info, double* trajectory, int flags);
/* One linearisation of the point-to-SDF alignment on this handle's volume, at
 * pose_guess G (camera-to-world) and rel_pose M (frame camera to the guess camera's frame), rounded
 * to f32 by the kernel.  Host side, in f64, each value rounded to f32 once: Qr = R_G / vs, Qo =
 * (t_G - f64(origin)) / vs, Rg = R_G, s = trunc / vs, trunc, dist_max and the pixel tables.  Per
 * sampled pixel (params->stride), every operation a separately rounded f32 operation, three-term
 * sums as (a + b) + c: the depth d as in tsdf_icp_linearize (code 0 without one); p = M (x_u d, y_v d,
 * d); the index-space point q = Qr p + Qo, i0 = floor(q), t = q - i0; the cell i0 + {0,1}^3 is not
 * inside this handle's volume (the raycast's rule): code 2; a corner has weight <= 0 (a hash voxel
 * without an entry has weight 0): 3; a corner has |tsdf| >= 1, the truncated plateau: 4; f the
 * trilinear value and g the gradient of the interpolant as the raycast forms them; r = -(trunc f);
 * |r| > dist_max or g exactly zero: 5; else the inlier, 6, with n_i = s ((Rg_0i g_x + Rg_1i g_y) +
 * Rg_2i g_z), the metric gradient in the guess camera's frame (towards positive tsdf, not
 * normalised), and the row J = (p x n, n).  sums, counts (inliers; candidates = codes 2..6), code
 * and residual, the pointers (host, or all device with TSDF_DEVICE_PTRS) and the determinism are
 * tsdf_icp_linearize's; the call runs on the handle's stream after its deferred frames, and
 * synchronises.  Restated by tests/sdf_ref.py.  TSDF_E_ARG: a NULL depth / K / rel_pose /
 * pose_guess / params / sums / counts, a bad image size, depth_kind or parameter, a cyclic column
 * shard. */
int tsdf_dense_sdf_linearize(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width,
                             const double K[9], const double rel_pose[16], const double pose_guess[16],
                             const tsdf_icp_params_t* params, double sums[28], int64_t counts[2],
                             uint8_t* code, float* residual, int flags);
/* The signed distance and its gradient at n world points (points: n x 3 f64), by the same cell:
 * q_a = f32((P_a - f64(origin_a)) / vs), then the cell tests above.  code (n u8): 2, 3, 4 or 6;
 * sdf (n f32): trunc f, metres; grad (n x 3 f32): s g in world axes, metres per metre, not
 * normalised.  Value and gradient are written for codes 4 and 6, zeros otherwise.  Any output
 * pointer may be NULL.  Host pointers, or all device pointers with TSDF_DEVICE_PTRS.  Deferred
 * frames run first; synchronous.  TSDF_E_ARG: n < 0 or >= 2^31, NULL points with n > 0, a cyclic
 * column shard. */
int tsdf_dense_sample(tsdf_dense_t* h, const double* points, int64_t n, float* sdf, float* grad,
                      uint8_t* code, int flags);
/* tsdf_dense_track with a photometric term: where the view holds one plane, the
 * geometry cannot see the two in-plane translations and the rotation about the normal; the colour
 * can.  color: the frame's RGB8 image, height x width x 3 (a host pointer, or a device pointer with
 * TSDF_DEVICE_PTRS, like depth).  The raycast at pose_guess also writes the model's colour map; one
 * prep launch turns both images into intensities I = (77 R + 150 G + 29 B) >> 8 and the model's into
 * photo texels (I, dI/du, dI/dv, depth); every iteration then adds to the point-to-plane system
 * color_weight^2 times the system of the residuals I_frame(u, v) - I_model(projection of p), bilinear
 * in the model image (tsdf_icp_linearize_rgbd's arithmetic).  Lost looks at the geometric inliers and
 * at the pivots of the combined system.  color_weight = 0 gives tsdf_dense_track's result to the
 * byte.  info as there; color_info (may be NULL) the colour counts.  TSDF_E_ARG: what
 * tsdf_dense_track refuses, a NULL color / color_params, color_weight < 0 or not finite,
 * color_max_diff <= 0 (or NaN), an image smaller than 4 x 4. */
int tsdf_dense_track_rgbd(tsdf_dense_t* h, const void* depth, int depth_kind, const uint8_t* color,
                          int height, int width, const double K[9], const double pose_guess[16],
                          const tsdf_icp_params_t* params, const tsdf_icp_color_params_t* color_params,
                          double z_near, double z_far, double z_step, double out_pose[16],
                          tsdf_track_info_t* info, tsdf_track_color_info_t* color_info,
                          double* trajectory, int flags);
int tsdf_dense_stats(tsdf_dense_t* h, tsdf_stats_t* out, int reset);
int tsdf_dense_set_profiling(tsdf_dense_t* h, int on);

/* ---- voxel hash: replaces HashTable (hash_fusion.py:29-507) --------------------------------
 * Keys are 8x8x8 voxel blocks.  `capacity` is the reference's map_size (hash_fusion.py:34): the
 * modulus of hash_function (hash_fusion.py:182-190, tsdf_hash_keys) and the size the 0.75
 * load-factor policy is kept against.  The device table has S = the power of two >= capacity
 * slots; the home slot of block (bx,by,bz) is the reference's hash of the block coordinates in
 * int64 (int_bits = 64, NumPy 2 / Linux) or wrapping int32 (int_bits = 32, the author's Windows
 * run), floor-mod S.  Open addressing, linear probe, lock-free CAS insert.  Shard s of n_shards
 * owns the blocks whose home slot (in the S of create) falls in [s*S/n, (s+1)*S/n). */
int tsdf_hash_create(const int64_t dims[3], const float origin[3], double voxel_size,
                     double trunc, int64_t capacity, int64_t max_blocks, int int_bits,
                     int shard, int n_shards, int device, tsdf_hash_t** out);
int tsdf_hash_destroy(tsdf_hash_t* h);
int tsdf_hash_reset(tsdf_hash_t* h);

/* HashTable.integrate (hash_fusion.py:103-145): same voxel set as the grid; obs_weight is
 * ignored (always 1) exactly like the reference (hash_fusion.py:141,145). */
int tsdf_hash_integrate(tsdf_hash_t* h, const void* depth, int depth_kind, const void* color,
                        int color_kind, int height, int width, const double K[9],
                        const double world_to_cam[16], int flags);
int tsdf_hash_integrate_batch(tsdf_hash_t* h, int n_frames, const void* depth, int depth_kind,
                              const void* color, int color_kind, int height, int width,
                              const double K[9], const double* world_to_cam, int flags);

/* Per-voxel entry API (get_hash_entry / add_hash_entry / remove, hash_fusion.py:199-393),
 * batched: ijk is n x 3 int64 voxel indices (host).
 *   lookup: found[i] = 1 and the voxel's (tsdf, weight, colour) if voxel i has an entry.
 *   insert: creates the entry (block allocated if needed); if tsdf/weight/color are non-NULL
 *           they set the voxel's values, else the voxel keeps (1, 0, 0).  slot[i] = table slot
 *           of the block, local[i] = voxel index inside the block (the reference returns
 *           (bucket, slot)).  Inserting an existing entry finds it (no duplicates) and leaves the
 *           fields that are not given as they are.
 *   remove: removed[i] = 1 if the entry existed (of a voxel listed twice in one call, one of the
 *           two); a block whose last entry goes is freed.
 * A voxel without an entry holds (1, 0, 0): a removed voxel keeps no state, so an insert without
 * values, or an integrate, after a remove starts from a fresh voxel like the reference's Voxel()
 * (hash_fusion.py:138-143). */
int tsdf_hash_lookup(tsdf_hash_t* h, const int64_t* ijk, int64_t n, float* tsdf, float* weight,
                     float* color, uint8_t* found);
int tsdf_hash_insert(tsdf_hash_t* h, const int64_t* ijk, int64_t n, const float* tsdf,
                     const float* weight, const float* color, int64_t* slot, int32_t* local);
int tsdf_hash_remove(tsdf_hash_t* h, const int64_t* ijk, int64_t n, uint8_t* removed);
/* double_table_size (hash_fusion.py:414-437): the table size becomes new_capacity (the device
 * table rehashes into the power of two >= it when that changes). */
int tsdf_hash_resize(tsdf_hash_t* h, int64_t new_capacity);
int tsdf_hash_info(tsdf_hash_t* h, tsdf_hash_info_t* out);
/* Sparse block transfer for merging bucket-range shards: only live blocks move.
 * export: with bxyz == NULL, *n_blocks = live blocks; else fills up to *n_blocks (must be >= the
 *   live count) blocks: bxyz n x 3 int32 block coordinates, tsdf/weight/color n x 512 float32 in
 *   brick-local order (x*8 + y)*8 + z, occ n x 8 uint64 voxel-entry words (word z, bit x*8+y);
 *   any field pointer may be NULL.  Host pointers, or device pointers with TSDF_DEVICE_PTRS.
 * import: find-or-insert each block (distinct, inside the volume) and overwrite its contents and
 *   entry words (NULL occ: every voxel has an entry).  A field that is NULL stays as it is in a
 *   block the table already holds and is the default in a new one.  A voxel whose bit in occ is
 *   clear has no entry and holds (1, 0, 0) afterwards, whatever the arrays say for it and also in
 *   a NULL field.  The table / pool grow as needed. */
int tsdf_hash_export_blocks(tsdf_hash_t* h, int32_t* bxyz, float* tsdf, float* weight, float* color,
                            uint64_t* occ, int64_t* n_blocks, int flags);
int tsdf_hash_import_blocks(tsdf_hash_t* h, const int32_t* bxyz, int64_t n_blocks, const float* tsdf,
                            const float* weight, const float* color, const uint64_t* occ, int flags);
/* get_volume (hash_fusion.py:442-463): densify into C-order (X,Y,Z) host arrays; voxels
 * without an entry get tsdf 1, weight 0, colour 0.  Any pointer may be NULL. */
int tsdf_hash_get_dense(tsdf_hash_t* h, float* tsdf, float* weight, float* color);
/* The same densify on the device, into a dense handle of the hash's dims (unsharded; it is reset
 * first).  The hash's own mesh does not need it (tsdf_hash_extract_mesh); a densified handle's
 * tsdf_dense_extract_mesh gives the same mesh, at the cost of the whole extent. */
int tsdf_hash_to_dense(tsdf_hash_t* h, tsdf_dense_t* d);
/* get_mesh / get_point_cloud of the hash (hash_fusion.py:465-507): marching cubes at level 0 over
 * the table's live blocks.  The mesh is that of the volume tsdf_hash_get_dense gives
 * (a voxel without an entry: tsdf 1, colour 0; a slot whose pool block is out of range: absent;
 * no voxel at or beyond dims) under the rules of tsdf_dense_extract_mesh, and equals the mesh of
 * the densified handle byte for byte: vertices in increasing key ((x*Y + y)*Z + z)*3 + axis,
 * triangles in C-order of their anchor cell, then in the case table's order.  Deferred frames run
 * first.  Memory and work follow the live blocks, the blocks that can hold a vertex or a triangle
 * (tsdf_hash_mesh_info_t.mesh_blocks) and the mesh -- never dims.  A shard handle (n_shards > 1)
 * gives the mesh of its own blocks' state.  TSDF_E_ARG for 2^31 or more vertices or triangles
 * (faces are int32).  The result stays in the handle until the next extract, reset or destroy.
 * extract_mesh_fields: `fields` (TSDF_MESH_NORMALS | TSDF_MESH_FACES) names what to compute beside
 * vertices, colours and keys; *n_tris is counted either way.  extract_mesh asks for both.
 * get_mesh / get_mesh_keys copy it out as tsdf_dense_get_mesh does (any pointer may be NULL);
 * TSDF_E_ARG for a field that was not extracted. */
int tsdf_hash_extract_mesh(tsdf_hash_t* h, int64_t* n_verts, int64_t* n_tris);
int tsdf_hash_extract_mesh_fields(tsdf_hash_t* h, int fields, int64_t* n_verts, int64_t* n_tris);
int tsdf_hash_get_mesh(tsdf_hash_t* h, float* verts, float* normals, uint8_t* colors, int32_t* faces);
int tsdf_hash_get_mesh_keys(tsdf_hash_t* h, int64_t* keys);
int tsdf_hash_mesh_info(tsdf_hash_t* h, tsdf_hash_mesh_info_t* out);
/* tsdf_dense_raycast on the table: a voxel without an entry has weight 0, as in get_volume.  Absent
 * blocks are skipped by the table alone; each ray keeps the pool blocks of its current 2x2x2 block
 * neighbourhood, so the corner fetches probe only when it leaves that neighbourhood.  The same
 * results as the raycast of the densified volume.  TSDF_E_ARG also for a shard (n_shards > 1). */
int tsdf_hash_raycast(tsdf_hash_t* h, int height, int width, const double K[9],
                      const double cam_pose[16], double z_near, double z_far, double z_step,
                      float* depth, float* normals, uint8_t* colors, int flags);
/* HIP-event times, in milliseconds, of the calling thread's last raycast that synchronised before
 * returning on a handle with profiling on (tsdf_*_set_profiling): the live-bit pass (about 0 when
 * the bits were current) and the march.  -1 before any such call. */
int tsdf_raycast_last_ms(double* live_ms, double* march_ms);
/* tsdf_dense_track on the table (the model maps are tsdf_hash_raycast's).  TSDF_E_ARG also for a
 * shard (n_shards > 1). */
int tsdf_hash_track(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width,
                    const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                    double z_near, double z_far, double z_step, double out_pose[16],
                    tsdf_track_info_t* info, double* trajectory, int flags);
/* tsdf_dense_track_sdf, tsdf_dense_sdf_linearize and tsdf_dense_sample on the table: a cell touches
 * 1, 2, 4 or 8 blocks, each probed once; a voxel without an entry has weight 0.  The same results
 * as on the densified volume.  TSDF_E_ARG also for a shard (n_shards > 1). */
int tsdf_hash_track_sdf(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width,
                        const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                        double out_pose[16], tsdf_track_info_t* info, double* trajectory, int flags);
int tsdf_hash_sdf_linearize(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width,
                            const double K[9], const double rel_pose[16], const double pose_guess[16],
                            const tsdf_icp_params_t* params, double sums[28], int64_t counts[2],
                            uint8_t* code, float* residual, int flags);
int tsdf_hash_sample(tsdf_hash_t* h, const double* points, int64_t n, float* sdf, float* grad,
                     uint8_t* code, int flags);
/* HIP-event times, in milliseconds, of the calling thread's last track on a handle with profiling
 * on: ms[0] the raycast (0 for tsdf_*_track_sdf, which queues none), ms[1] the setup (frame copy, state, pixel tables), ms[2] and ms[3] the
 * linearise and the finish launches summed over the iterations run, ms[4] the launches that
 * fell through after a status was set.  -1 before any such call. */
int tsdf_track_last_ms(double ms[5], int* iterations);
/* tsdf_dense_track_rgbd on the table. */
int tsdf_hash_track_rgbd(tsdf_hash_t* h, const void* depth, int depth_kind, const uint8_t* color,
                         int height, int width, const double K[9], const double pose_guess[16],
                         const tsdf_icp_params_t* params, const tsdf_icp_color_params_t* color_params,
                         double z_near, double z_far, double z_step, double out_pose[16],
                         tsdf_track_info_t* info, tsdf_track_color_info_t* color_info,
                         double* trajectory, int flags);
/* After an RGB-D track with profiling on, tsdf_track_last_ms describes it as it does a geometric
 * one (ms[2] / ms[3]: the RGB-D linearise and finish), and this gives the prep launch (intensity
 * image and photo texels), which is in none of those five.  -1 before any such call. */
int tsdf_track_last_prep_ms(double* ms);
int tsdf_hash_sync(tsdf_hash_t* h);
/* sync, then a pool on mapped memory hands the memory above its live blocks back (pool_capacity
 * = live blocks + ~3 %, in whole 8 MB pieces; the live blocks move into fresh mapped ranges by one
 * device copy): the end of an asynchronous run, whose growth had to stay ahead of the launches in
 * flight.  get_volume / get_mesh call it.  Not in the reference (its pool is a Python dict). */
int tsdf_hash_trim(tsdf_hash_t* h);
int tsdf_hash_stats(tsdf_hash_t* h, tsdf_stats_t* out, int reset);
int tsdf_hash_set_profiling(tsdf_hash_t* h, int on);
/* Frames one launch of this table integrates (as tsdf_dense_frames_per_launch: 32 in this build;
 * shards of n_shards > 1 always kMaxBatch). */
int tsdf_hash_frames_per_launch(tsdf_hash_t* h, int* n);

/* ---- frame utilities ---------------------------------------------------------------------
 * Volume bounds from view frustums: the demo loop grid_demo1.py:50-64 (hash_demo1.py:93-107)
 * over get_view_frustum (grid_fusion.py:371-383).  For each of
 * n_frames depth images (H*W each, kind U16_MM or F64_M; host, or device with TSDF_DEVICE_PTRS;
 * TSDF_DEPTH_INVALID_65535 masks 65535 mm; on HIP device `device`): the image's max depth, the 5 frustum points
 * transformed by cam_pose (n_frames*16 doubles, camera-to-world, host), then
 * bounds[2r] = min(bounds[2r], min over points), bounds[2r+1] = max(...) for r = x, y, z
 * (bounds is in/out: the demo starts from zeros).  Optional outputs: max_depth (n_frames
 * doubles, metres) and frustum_pts (n_frames x 3 x 5 doubles, get_view_frustum's array).
 * Where a frame's max depth is finite and every coordinate it gives is, all values equal the
 * reference's f64 results bit for bit.  F64_M frames from float-depth sources hold more than that,
 * and for them the contract is this (it departs from np.max in the first point only):
 *   - a NaN pixel is ignored: the max depth is the maximum over the other pixels (np.max would
 *     return the NaN); negative and infinite pixels take part like any value;
 *   - a frame without a single non-NaN pixel has max depth 0.0, like a u16 frame whose pixels are
 *     all invalid: its five points are the camera centre;
 *   - a max depth of +inf, or one whose product with a pixel offset overflows, gives infinite
 *     coordinates, and NaN ones where the infinity meets a zero or its opposite (0 * inf, inf - inf).
 *     frustum_pts reports both as computed; bounds folds the infinite ones and passes over the NaN
 *     ones (fmin / fmax), so a depth image never makes it come back holding a NaN;
 *   - a NaN coordinate that the pose or K made -- one that a max depth of 1 m gives as well: a NaN
 *     in cam_pose, fx == 0, an infinite principal point -- is the caller's lost tracking and stays
 *     visible as in the reference, whose np.minimum / np.amin keep it: both bounds of that axis come
 *     back NaN, and NaN bounds passed in stay NaN.  The 1 m probe is the whole rule: a finite pose
 *     whose products overflow to inf - inf only at the frame's real max depth counts as depth-made
 *     and is passed over, where the reference would keep that NaN too;
 *   - frames that are -inf throughout are not specified.
 * tests/test_hostile_depth_gpu.py, tests/test_hostile_pose_gpu.py; oracle.frame_max_depth / frustum_bounds
 * state the same rule. */
int tsdf_frustum_bounds(const void* depth, int depth_kind, int n_frames, int height, int width,
                        const double K[9], const double* cam_poses, int flags, int device,
                        double* max_depth, double* frustum_pts, double bounds[6]);

/* One linearisation of the point-to-plane ICP, without a handle, on HIP device
 * `device`.  depth: the frame, Hf x Wf of depth_kind through Kf (TSDF_DEPTH_INVALID_65535 honoured);
 * model_depth Hm x Wm f32 and model_normals Hm x Wm x 3 f32 (world axes): the maps of a raycast at
 * model_pose through Km; rel_pose: M, frame camera to model camera.  Per sampled pixel (params->
 * stride) a code -- 0 not sampled, last row / column or no depth; 1 no neighbour depth or no
 * normal; 2 behind the model camera or outside its image; 3 no model surface there; 4 further than
 * dist_max; 5 normals' cosine below cos_min; 6 inlier -- and for an inlier the residual r and the row
 * J = (p x n, n), every operation a separately rounded f32 operation in the fixed order of §7e
 * (restated by tests/icp_ref.py).  sums: the 21 upper-triangle entries of sum J_i J_j (row-major),
 * the 6 of sum J_i r, and sum r r, over the inliers, in f64 (every term an exact product; the
 * order of addition is fixed by the image size, the stride and the device: repeatable to the
 * byte, no floating-point atomics).  counts: inliers, candidates (codes 2..6).  code (Hf x Wf u8)
 * and residual (Hf x Wf f32, 0 where code != 6) may be NULL.  The image pointers (depth, the model
 * maps, code, residual) are host pointers, or all device pointers with TSDF_DEVICE_PTRS; host
 * images go through device buffers kept per device (grown on demand).  Synchronous.  Only
 * dist_max, cos_min and stride of params matter (all of it is validated). */
int tsdf_icp_linearize(int device, const void* depth, int depth_kind, int Hf, int Wf, const double Kf[9],
                       const double rel_pose[16], const float* model_depth, const float* model_normals,
                       int Hm, int Wm, const double Km[9], const double model_pose[16],
                       const tsdf_icp_params_t* params, double sums[28], int64_t counts[2],
                       uint8_t* code, float* residual, int flags);

/* One RGB-D linearisation: tsdf_icp_linearize's geometric half -- the same bytes --
 * and, in the same pass over the frame, the photometric half.  color: the frame's RGB8 image
 * (Hf x Wf x 3); model_colors: the raycast's colour map (Hm x Wm x 3 u8, at least 4 x 4).
 * Intensity I = (77 R + 150 G + 29 B) >> 8.  The model's photo texel (I, Gx, Gy, D) at (v, u) has
 * Gx = (I(v,u+1) - I(v,u-1)) / 2, Gy = (I(v+1,u) - I(v-1,u)) / 2 and D = model_depth(v,u) when the
 * pixel and its four 4-neighbours lie inside the image and all have depth > 0; otherwise it is
 * invalid (all zeros).  Per sampled pixel with a depth, p = M V as in the geometric half (no normal
 * is needed; the last row and column take part) and a colour code -- 0 not sampled or no depth;
 * 1 p_z <= 0, or with x = fxm (p_x / p_z) + cxm, y alike, x0 = floor(x), y0 = floor(y), not
 * 1 <= x0 <= Wm - 3 and 1 <= y0 <= Hm - 3; 2 one of the texels (y0 + {0,1}, x0 + {0,1}) invalid;
 * 3 occluded: |D_b - p_z| > dist_max, every bilinear value being lerp_y(lerp_x(t00, t01),
 * lerp_x(t10, t11)) with lerp(a, b, t) = a + t (b - a) at tx = x - x0, ty = y - y0; 4 the residual
 * r = I_frame(u, v) - I_b has |r| > color_max_diff; 5 inlier, with the row J = (p x g, g),
 * g = (Gx_b fxm / p_z, Gy_b fym / p_z, -(g_x p_x + g_y p_y) / p_z) in the fixed f32 order of §7f
 * (restated by tests/icp_color_ref.py).  sums[0..27] and counts[0..1] as tsdf_icp_linearize's;
 * sums[28..55] the same 21 + 6 + 1 sums of the colour rows (not scaled by color_weight), counts[2]
 * the colour inliers, counts[3] the colour candidates (codes 2..5).  code / residual and
 * color_code / color_residual (Hf x Wf; the residual in intensity levels, 0 where the code is not
 * 5) may each be NULL.  Pointers, flags and determinism as tsdf_icp_linearize.  TSDF_E_ARG: what
 * that call refuses, a NULL color / model_colors / color_params, color_weight < 0 or not finite,
 * color_max_diff <= 0 (or NaN), a model map smaller than 4 x 4. */
int tsdf_icp_linearize_rgbd(int device, const void* depth, int depth_kind, const uint8_t* color, int Hf,
                            int Wf, const double Kf[9], const double rel_pose[16],
                            const float* model_depth, const float* model_normals,
                            const uint8_t* model_colors, int Hm, int Wm, const double Km[9],
                            const double model_pose[16], const tsdf_icp_params_t* params,
                            const tsdf_icp_color_params_t* color_params, double sums[56],
                            int64_t counts[4], uint8_t* code, float* residual, uint8_t* color_code,
                            float* color_residual, int flags);

/* ---- merge ------------------------------------------------------------------
 * What a merge did to the destination. */
typedef struct {
    int64_t samples;          /* destination voxels that received a sample */
    int64_t bricks_updated;   /* destination bricks / blocks with >= 1 sample */
    int64_t blocks_allocated; /* hash destination: blocks newly allocated (0 for dense) */
} tsdf_merge_info_t;

/* Merge a fused volume (the source: src_dense or src_hash, exactly one non-NULL) into dst under
 * src_to_dst, a rigid 4x4 row-major matrix taking source world coordinates to destination world
 * coordinates.  Every destination voxel is taken to the source's index space, q = A (x, y, z) + b
 * with A = R^T vs_D / vs_S and b = (R^T (o_D - t) - o_S) / vs_S rounded to f32 once; the source is
 * sampled trilinearly in its cell floor(q) -- an axis with an exactly zero fraction neither fetches
 * nor requires its upper neighbour -- and no sample is taken where the cell leaves the source or a
 * corner that counts has weight <= 0 (a hash voxel without an entry: weight 0).  A sample blends
 * u = clamp(trunc_S / trunc_D * v, -1, 1) with the weight w_S = the least corner weight, and the
 * colour of the nearest corner, into the voxel by the integrate's exact update: w_N = w_D + w_S,
 * t_N = f32((f64(w_D t_D) + f64(w_S u)) / f64(w_N)), colour channels min(255, rint((w_D old +
 * w_S new) / w_N)).  A voxel without a sample keeps its bytes.  Every operation is a separately
 * rounded f32 operation in the fixed order of §7h (restated by tests/merge_ref.py); the same inputs
 * give the same bytes (no floating-point atomics).  Integer weights and canonical colours stay so;
 * a translation by whole voxels between equal lattices copies every observed voxel bit for bit.
 * A hash destination receives an entry for every sampled voxel and blocks for exactly the bricks
 * with a sample; table and pool grow as tsdf_hash_import_blocks grows them.  Deferred frames of both
 * handles run first, the source's stream is complete before the destination reads it, and the call
 * is synchronous.  Frame statistics do not change.  info may be NULL; flags must be 0.
 * TSDF_E_ARG: a NULL handle or matrix, both or neither source, the same handle on both sides,
 * handles on different devices, a cyclic column shard or a hash shard (n_shards > 1) on either side
 * (slab shards -- index_offset -- are accepted and use global indices), a matrix with an entry that
 * is not finite, a last row other than 0 0 0 1 or a rotation not orthonormal with determinant +1 to
 * 1e-6, and a source truncation below the destination's (no downsampling).  The destination is
 * unchanged after a refusal.  TSDF_E_CAPACITY / TSDF_E_OOM (a hash destination whose table or pool
 * could not grow): no voxel has changed, but blocks inserted before the failure stay in the table
 * without entries, as after a failed tsdf_hash_import_blocks. */
int tsdf_dense_merge(tsdf_dense_t* dst, tsdf_dense_t* src_dense, tsdf_hash_t* src_hash,
                     const double src_to_dst[16], tsdf_merge_info_t* info, int flags);
int tsdf_hash_merge(tsdf_hash_t* dst, tsdf_dense_t* src_dense, tsdf_hash_t* src_hash,
                    const double src_to_dst[16], tsdf_merge_info_t* info, int flags);
/* (As tsdf_raycast_last_ms and tsdf_track_last_ms: what a timing record of this path needs and a
 * caller cannot get from outside -- the launches' device time apart from the host work between
 * them, and what the cull skipped.)  The calling thread's last merge: the HIP-event time, in milliseconds, of its launches when the
 * destination had profiling on (tsdf_*_set_profiling; a hash destination: the marking pass and the
 * pass over the marked blocks, not the block insertion between them; -1 before any such call), and
 * the destination bricks the cull let through -- those whose box, taken to the source's index space,
 * can hold a cell inside the source that starts in a source brick with an observed voxel -- against
 * info's bricks_updated (-1 before any merge). */
int tsdf_merge_last_profile(double* ms, int64_t* candidate_bricks);

/* hash_function over n coordinate triples (host in, host out), computed on the device.  The
 * same arithmetic as the kernels' home-slot computation. */
int tsdf_hash_keys(const int64_t* xyz, int64_t n, int64_t table_size, int int_bits,
                   int64_t* out, int device);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_H */
