// tsdf_raycast.hip -- depth, normal and colour maps of the fused model from a pose:
// what a tracker aligns the next frame against, KinectFusion style, and a preview of the map,
// without moving the volume to the host.  Not in the reference (it only exports the volume and
// its mesh).  Dense grids and the voxel hash are served by one marcher.
//
// The contract (restated in NumPy by tests/raycast_ref.py, matched bit for bit):
//   per ray (pixel u, v), in f64, each rounded to f32 once:
//     dc = ((u - cx) / fx, (v - cy) / fy, 1)                      camera ray per unit depth
//     qd = (R dc) / vs,  qo = (t - f64(origin)) / vs              index space, voxel centres at integers
//   per sample k = 0, 1, ..., in f32, every operation rounded (no fma):
//     z_k = zn + f32(k) * zs   while z_k <= zf;   q = qo + qd * z_k;   i0 = floor(q), t = q - i0
//     valid: the 8 corners i0 + {0,1}^3 are inside the volume and all have weight > 0
//     f = lerp_x(lerp_y(lerp_z)), lerp(a, b, t) = a + t * (b - a)
//   outcome: the first k >= 1 valid with f_k < 0 decides; a hit when sample k-1 is valid with
//   f_{k-1} > 0:  z* = z_{k-1} + zs * (f_{k-1} / (f_{k-1} - f_k)), colour of the voxel at
//   rint(q(z*)), unit gradient of the interpolant in the cell of q(z*) (0 if that cell is invalid).
//
// Skipping never changes that: a cell whose 8 corners hold no voxel with weight > 0 and tsdf < 0
// interpolates to f >= 0 (each lerp of non-negative values with t in [0, 1) is non-negative under
// round-to-nearest), so it cannot decide.  One bit per brick (dense) or per pool block (hash) says
// whether such a voxel exists within the cells anchored there; the marcher jumps k over boxes of
// index space it knows to be dead, re-entering two samples early and keeping a margin to the far
// faces that covers the f32 rounding of q (the near faces are safe by monotonicity of q in k).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "tsdf_cell.h"
#include "tsdf_host.h"

using namespace tsdf;

namespace {

constexpr int kRayWG = 256;          // 4 waves, one 8x8 pixel tile each
constexpr int kRayMaxK = 1 << 22;    // samples per ray: f32(k) and the jump arithmetic stay exact enough

struct RayArgs {
    Vol v;
    Pool pool;
    Table t;                  // hash only
    const unsigned* live;     // one bit per brick (dense) / per pool block (hash); unused when !skip
    long long n_live;         // bits in live
    double fx, fy, cx, cy;
    double R[9], tr[3];       // cam_pose rows 0..2: rotation and translation
    float zn, zf, zs;
    int H, W;
    int tiles_x, n_tiles;
    int skip;
    float* depth;
    float* normals;
    unsigned char* colors;
};

// (lerp, floor_i, dense_index, trilinear and the gradient: tsdf_cell.h, shared with the tracker)

// ---- hash: the pool blocks of a 2x2x2 block neighbourhood, per ray, in LDS --------------------
// nb[slot * kRayWG] (slot = ox*4 + oy*2 + oz) is the pool block of block A + (ox, oy, oz), or -1.
struct Hood {
    int* nb;       // this lane's column of the workgroup's LDS array
    int A[3];      // anchor block
    bool have;     // the column is filled for A
    bool live;     // some block of the neighbourhood holds a voxel with weight > 0 and tsdf < 0
};

// Make the neighbourhood cover the cell at i0 (corners i0 and i0 + 1): kept while
// 8A <= i0 <= 8A + 14 on every axis, else re-anchored with its room on the side the ray moves to.
__device__ inline void hood_cover(const RayArgs& a, Hood& h, const int i0[3], const float qd[3]) {
    bool ok = h.have;
    for (int d = 0; d < 3; ++d) ok = ok && i0[d] >= 8 * h.A[d] && i0[d] <= 8 * h.A[d] + 14;
    if (ok) return;
    for (int d = 0; d < 3; ++d) h.A[d] = qd[d] < 0.0f ? ((i0[d] + 1) >> 3) - 1 : (i0[d] >> 3);
    h.have = true;
    h.live = false;
    for (int s = 0; s < 8; ++s) {
        const int bx = h.A[0] + (s >> 2), by = h.A[1] + ((s >> 1) & 1), bz = h.A[2] + (s & 1);
        int blk = -1;
        if (bx >= 0 && by >= 0 && bz >= 0 && bx < a.v.nb[0] && by < a.v.nb[1] && bz < a.v.nb[2])
            blk = hash_find(a.t, bx, by, bz, a.t.max_blocks);
        h.nb[s * kRayWG] = blk;
        if (blk >= 0 && (!a.skip || ((long long)blk < a.n_live && ((a.live[blk >> 5] >> (blk & 31)) & 1u)))) h.live = true;
    }
}

// One voxel (inside the volume) through the neighbourhood; without an entry: (1, 0, 0).
template <bool COLOR>
__device__ inline void hash_voxel(const RayArgs& a, const Hood& h, int x, int y, int z, float* t, float* w) {
    const int s = (((x >> 3) - h.A[0]) << 2) | (((y >> 3) - h.A[1]) << 1) | ((z >> 3) - h.A[2]);
    *t = COLOR ? 0.0f : 1.0f;
    *w = 0.0f;
    if ((unsigned)s > 7u) return;  // (never: hood_cover ran for this cell)
    hash_block_voxel<COLOR>(a.t, a.pool, h.nb[s * kRayWG], x, y, z, t, w);
}

// The 8 corner values of the cell at local index l (c[dx*4 + dy*2 + dz]); false: not valid.
template <bool HASH>
__device__ inline bool load_cell(const RayArgs& a, Hood& h, const int l[3], const float qd[3], float c[8]) {
    for (int d = 0; d < 3; ++d)
        if (l[d] < 0 || l[d] > a.v.dims[d] - 2) return false;
    if (HASH) hood_cover(a, h, l, qd);
    bool valid = true;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int x = l[0] + (s >> 2), y = l[1] + ((s >> 1) & 1), z = l[2] + (s & 1);
        float w;
        if (HASH) {
            hash_voxel<false>(a, h, x, y, z, &c[s], &w);
        } else {
            const size_t j = dense_index(a.v, x, y, z);
            c[s] = a.pool.tsdf[j];
            w = a.pool.weight[j];
        }
        valid = valid && w > 0.0f;
    }
    return valid;
}

struct Ray {
    float qo[3], qd[3];
    float m[3];  // margin kept to a box's far face (the rounding of q, with room to spare)
};

// q, its cell (global index i0, local l) and fractions at depth z
__device__ inline void sample_at(const RayArgs& a, const Ray& r, float z, int l[3], float t[3], float q[3]) {
    for (int d = 0; d < 3; ++d) {
        q[d] = r.qo[d] + r.qd[d] * z;
        const int i0 = floor_i(q[d]);
        t[d] = q[d] - (float)i0;
        l[d] = i0 - a.v.off[d];
    }
}

// The first sample after k that may leave the box [lo, hi) of index space, less two samples.
__device__ inline int jump(const RayArgs& a, const Ray& r, const float lo[3], const float hi[3], int k) {
    float ze = INFINITY;
    for (int d = 0; d < 3; ++d) {  // (a direction component of exactly 0 never leaves: no division)
        if (r.qd[d] > 0.0f) ze = fminf(ze, (hi[d] - r.m[d] - r.qo[d]) / r.qd[d]);
        else if (r.qd[d] < 0.0f) ze = fminf(ze, (lo[d] + r.m[d] - r.qo[d]) / r.qd[d]);
    }
    const float kf = (ze - a.zn) / a.zs;
    const int kn = kf < (float)kRayMaxK ? (int)floorf(fmaxf(kf, 0.0f)) - 2 : kRayMaxK + 1;
    return max(k + 1, kn);
}

template <bool HASH>
__global__ __launch_bounds__(kRayWG) void k_raycast(RayArgs a) {
    __shared__ int s_nb[HASH ? 8 * kRayWG : 1];
    const int tile = blockIdx.x * (kRayWG / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (tile >= a.n_tiles) return;
    const int u = (tile % a.tiles_x) * 8 + (lane & 7), v = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (u >= a.W || v >= a.H) return;

    // ---- per-ray setup: f64, rounded to f32 once
    Ray r;
    {
        const double dx = ((double)u - a.cx) / a.fx, dy = ((double)v - a.cy) / a.fy;
        for (int d = 0; d < 3; ++d) {
            const double D = (a.R[3 * d] * dx + a.R[3 * d + 1] * dy) + a.R[3 * d + 2];
            r.qd[d] = (float)(D / a.v.vs);
            r.qo[d] = (float)((a.tr[d] - (double)a.v.origin[d]) / a.v.vs);
            r.m[d] = 1.9073486328125e-6f * (fabsf(r.qo[d]) + fabsf(r.qd[d]) * a.zf + 16.0f);  // 2^-19 x
        }
    }
    Hood h;
    h.nb = &s_nb[HASH ? threadIdx.x : 0];
    h.A[0] = h.A[1] = h.A[2] = 0;
    h.have = false;
    h.live = false;

    // ---- march: the first k >= 1 whose sample is valid with f < 0
    float c1[8], t1[3], q[3], f1 = 0.0f;
    int l[3];
    int k = 1;
    bool found = false;
    while (k <= kRayMaxK) {
        const float zk = a.zn + (float)k * a.zs;
        if (!(zk <= a.zf)) break;
        sample_at(a, r, zk, l, t1, q);
        bool inside = true, gone = false;
        for (int d = 0; d < 3; ++d) {
            inside = inside && l[d] >= 0 && l[d] <= a.v.dims[d] - 2;
            // past the volume and moving away (or not at all) on this axis: no later sample is valid
            gone = gone || (l[d] < -1 && r.qd[d] <= 0.0f) || (l[d] > a.v.dims[d] && r.qd[d] >= 0.0f);
        }
        if (gone) break;
        float lo[3], hi[3];
        bool dead;
        if (!inside) {
            // Beyond the volume on some axis: every sample is invalid while the ray stays in that
            // axis' outer half-space, q < off (cells < 0) or q >= off + dims - 1 (cells > dims - 2).
            // The brick of the cell will not do as the box here: on the high side it also holds
            // cells that are inside.  The longest stay over the axes that are out.
            int kn = k + 1;
            if (a.skip) {
                for (int d = 0; d < 3; ++d) {
                    if (l[d] >= 0 && l[d] <= a.v.dims[d] - 2) continue;
                    for (int e = 0; e < 3; ++e) {
                        lo[e] = -INFINITY;
                        hi[e] = INFINITY;
                    }
                    if (l[d] < 0) hi[d] = (float)a.v.off[d];
                    else lo[d] = (float)(a.v.off[d] + a.v.dims[d] - 1);
                    kn = max(kn, jump(a, r, lo, hi, k));
                }
            }
            k = kn;
            continue;
        }
        if (!HASH) {  // the 8^3 brick of the cell (its cells beyond the volume are dead anyway)
            const int bx = l[0] >> 3, by = l[1] >> 3, bz = l[2] >> 3;
            const int B[3] = {bx, by, bz};
            for (int d = 0; d < 3; ++d) {
                lo[d] = (float)(a.v.off[d] + 8 * B[d]);
                hi[d] = lo[d] + 8.0f;
            }
            dead = false;
            if (a.skip) {
                const long long b = ((long long)bx * a.v.nb[1] + by) * a.v.nb[2] + bz;
                dead = !(b < a.n_live && ((a.live[b >> 5] >> (b & 31)) & 1u));
            }
        } else {  // the neighbourhood's reach: cells 8A .. 8A + 14
            hood_cover(a, h, l, r.qd);
            for (int d = 0; d < 3; ++d) {
                lo[d] = (float)(8 * h.A[d]);
                hi[d] = lo[d] + 15.0f;
            }
            dead = !h.live;
        }
        if (dead) {
            k = a.skip ? jump(a, r, lo, hi, k) : k + 1;
            continue;
        }
        if (load_cell<HASH>(a, h, l, r.qd, c1)) {
            f1 = trilinear(c1, t1);
            if (f1 < 0.0f) {
                found = true;
                break;
            }
        }
        ++k;
    }

    // ---- the deciding sample finishes the ray
    float depth = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f};
    unsigned char rgb[3] = {0, 0, 0};
    if (found) {
        const float z0 = a.zn + (float)(k - 1) * a.zs;
        float c0[8], t0[3];
        sample_at(a, r, z0, l, t0, q);
        if (load_cell<HASH>(a, h, l, r.qd, c0)) {
            const float f0 = trilinear(c0, t0);
            if (f0 > 0.0f) {
                const float zs = z0 + a.zs * (f0 / (f0 - f1));
                depth = zs;
                float ts[3], cs[8];
                sample_at(a, r, zs, l, ts, q);
                // colour: the voxel at rint(q(z*)) (clamped into the volume; it is inside whenever
                // z* lies between the two samples)
                int rv[3];
                for (int d = 0; d < 3; ++d) {
                    const int g = (int)rintf(fminf(fmaxf(q[d], -1.0e9f), 1.0e9f)) - a.v.off[d];
                    rv[d] = min(max(g, 0), a.v.dims[d] - 1);
                }
                float cv, unused;
                if (HASH) {
                    hood_cover(a, h, rv, r.qd);
                    hash_voxel<true>(a, h, rv[0], rv[1], rv[2], &cv, &unused);
                } else {
                    cv = a.pool.color[dense_index(a.v, rv[0], rv[1], rv[2])];
                }
                const float cb = floorf(cv / 65536.0f);
                const float cg = floorf((cv - cb * 65536.0f) / 256.0f);
                const float cr = cv - cb * 65536.0f - cg * 256.0f;
                rgb[0] = (unsigned char)(int)floorf(cr);
                rgb[1] = (unsigned char)(int)floorf(cg);
                rgb[2] = (unsigned char)(int)floorf(cb);
                if (a.normals && load_cell<HASH>(a, h, l, r.qd, cs)) {
                    float g[3];
                    cell_gradient(cs, ts, g);
                    const float gx = g[0], gy = g[1], gz = g[2];
                    const float len = __fsqrt_rn((gx * gx + gy * gy) + gz * gz);
                    if (len > 0.0f) {
                        nrm[0] = gx / len;
                        nrm[1] = gy / len;
                        nrm[2] = gz / len;
                    }
                }
            }
        }
    }
    const size_t p = (size_t)v * a.W + u;
    if (a.depth) a.depth[p] = depth;
    if (a.normals)
        for (int d = 0; d < 3; ++d) a.normals[3 * p + d] = nrm[d];
    if (a.colors)
        for (int d = 0; d < 3; ++d) a.colors[3 * p + d] = rgb[d];
}

// ---- live bits --------------------------------------------------------------------------------
// Dense: brick b is live when a voxel of its 9^3 reach (its own voxels and the +1 layer the corners
// of its cells touch) inside the volume has weight > 0 and tsdf < 0.  One wave per brick.
__global__ __launch_bounds__(256) void k_ray_live_dense(Vol v, Pool pool, unsigned* live, long long n_bricks) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long b = wave; b < n_bricks; b += nw) {
        const int bz = (int)(b % v.nb[2]), by = (int)((b / v.nb[2]) % v.nb[1]), bx = (int)(b / ((long long)v.nb[1] * v.nb[2]));
        bool neg = false;
        for (int i = lane; i < 729; i += 64) {
            const int x = bx * 8 + i / 81, y = by * 8 + (i / 9) % 9, z = bz * 8 + i % 9;
            if (x < v.dims[0] && y < v.dims[1] && z < v.dims[2]) {
                const size_t j = dense_index(v, x, y, z);
                neg = neg || (pool.weight[j] > 0.0f && pool.tsdf[j] < 0.0f);
            }
        }
        if (__ballot(neg) && lane == 0) atomicOr(&live[b >> 5], 1u << (b & 31));
    }
}

// Hash: the bit of a pool block is set when one of its own voxels with an entry has weight > 0 and
// tsdf < 0; the marcher ORs the bits of a ray's 2x2x2 neighbourhood, which holds every corner of
// the cells it serves.  64 table slots per wave and step; the wave then takes the blocks in turn.
__global__ __launch_bounds__(256) void k_ray_live_hash(Table t, Pool pool, unsigned* live, long long n_live) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long base = wave * 64; base < t.capacity; base += nw * 64) {
        const long long s = base + lane;
        int blk = -1;
        if (s < t.capacity) {
            const unsigned long long key = coh_load(&t.keys[s]);
            if (key != kEmpty && key != kTomb) blk = coh_load(&t.vals[s]);
        }
        unsigned long long m = __ballot(blk >= 0 && blk < t.max_blocks && blk < n_live);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int b = __shfl(blk, src);
            bool neg = false;
            for (int j = 0; j < kBrickVox / 64; ++j) {
                const int local = j * 64 + lane;  // (x*8 + y)*8 + z; entry bit: word z, bit x*8 + y
                const unsigned long long word = coh_load(&t.occ[(size_t)b * 8 + (local & 7)]);
                if ((word >> (local >> 3)) & 1ull) {
                    const size_t i = (size_t)b * kBrickVox + local;
                    neg = neg || (pool.weight[i] > 0.0f && pool.tsdf[i] < 0.0f);
                }
            }
            if (__ballot(neg) && lane == 0) atomicOr(&live[b >> 5], 1u << (b & 31));
        }
    }
}

// The live bits for the handle's current state generation (recomputed only when it changed, or
// when the caller asks: TSDF_RAY_REFLAG).
int ensure_live(const RaySource& S, bool force) {
    Base& B = *S.b;
    const long long bits = S.table ? S.table->max_blocks : B.n_bricks;
    const size_t words = (size_t)((bits + 31) / 32);
    if (words > B.ray_live_words) {
        if (B.ray_live) {
            TSDF_HIP(hipStreamSynchronize(B.stream));
            TSDF_HIP(hipFree(B.ray_live));
            B.ray_live = nullptr;
            B.ray_live_words = 0;
        }
        TSDF_HIP(hipMalloc(&B.ray_live, sizeof(unsigned) * std::max<size_t>(words, 1)));
        B.ray_live_words = words;
        B.ray_live_gen = 0;
    }
    if (!force && B.ray_live_gen == B.state_gen) return TSDF_OK;
    TSDF_HIP(hipMemsetAsync(B.ray_live, 0, sizeof(unsigned) * B.ray_live_words, B.stream));
    const unsigned grid = (unsigned)B.n_cu * 8;
    if (S.table) {
        hipLaunchKernelGGL(k_ray_live_hash, dim3(grid), dim3(256), 0, B.stream, *S.table, B.pool, B.ray_live,
                           (long long)B.ray_live_words * 32);
    } else {
        hipLaunchKernelGGL(k_ray_live_dense, dim3(grid), dim3(256), 0, B.stream, B.vol, B.pool, B.ray_live,
                           B.n_bricks);
    }
    TSDF_HIP(hipGetLastError());
    B.ray_live_gen = B.state_gen;
    return TSDF_OK;
}

// HIP-event times of the calling thread's last synchronous raycast on a handle with profiling on
// (tsdf_*_set_profiling): the live-bit pass (0 when the bits were current) and the march.
thread_local double g_last_ms[2] = {-1.0, -1.0};

int raycast(const RaySource& S, int H, int W, const double* K, const double* pose, double zn, double zf, double zs,
            float* depth, float* normals, uint8_t* colors, int flags) {
    Base& B = *S.b;
    if (!K || !pose) return set_error(TSDF_E_ARG, "null camera pointer");
    if (H <= 0 || W <= 0 || H >= (1 << 24) || W >= (1 << 24) || (long long)H * W >= (1ll << 28))
        return set_error(TSDF_E_ARG, "bad image size %dx%d", H, W);
    if (!(zs > 0.0)) return set_error(TSDF_E_ARG, "z_step must be > 0 (got %g)", zs);
    if (!(zn >= 0.0)) return set_error(TSDF_E_ARG, "z_near must be >= 0 (got %g)", zn);
    if (!(zf >= zn)) return set_error(TSDF_E_ARG, "z_far (%g) must be >= z_near (%g)", zf, zn);
    RayArgs a{};
    a.zn = (float)zn;
    a.zf = (float)zf;
    a.zs = (float)zs;
    if (!(a.zs > 0.0f) || !std::isfinite(a.zf)) return set_error(TSDF_E_ARG, "z_step / z_far out of the f32 range");
    if (!((zf - zn) / zs < (double)(kRayMaxK - 2)))
        return set_error(TSDF_E_ARG, "more than 2^22 samples per ray ((z_far - z_near) / z_step = %g)", (zf - zn) / zs);
    a.v = B.vol;
    a.pool = B.pool;
    if (S.table) a.t = *S.table;
    a.fx = K[0];
    a.fy = K[4];
    a.cx = K[2];
    a.cy = K[5];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a.R[3 * r + c] = pose[4 * r + c];
        a.tr[r] = pose[4 * r + 3];
    }
    a.H = H;
    a.W = W;
    a.tiles_x = (W + 7) / 8;
    a.n_tiles = a.tiles_x * ((H + 7) / 8);
    a.skip = B.ray_skip ? 1 : 0;
    const bool timed = B.prof.on && !((flags & TSDF_DEVICE_PTRS) && (flags & TSDF_ASYNC));
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 3; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};
    if (timed) {
        for (auto& e : ev) TSDF_HIP(hipEventCreate(&e));
        TSDF_HIP(hipEventRecord(ev[0], B.stream));
    }
    if (a.skip) {
        TSDF_TRY(ensure_live(S, (flags & TSDF_RAY_REFLAG) != 0));
        a.live = B.ray_live;
        a.n_live = (long long)B.ray_live_words * 32;
    }
    if (timed) TSDF_HIP(hipEventRecord(ev[1], B.stream));
    const size_t px = (size_t)H * W;
    const bool dev = (flags & TSDF_DEVICE_PTRS) != 0;
    float *dd = depth, *dn = normals;
    unsigned char* dc = colors;
    int r = TSDF_OK;
    if (!dev) {
        // host outputs: through device buffers kept on the handle (a host-pointer call synchronises
        // before it returns, so nothing in flight reads them when the next call grows them)
        const size_t need[3] = {depth ? px * sizeof(float) : 0, normals ? px * 3 * sizeof(float) : 0, colors ? px * 3 : 0};
        for (int i = 0; i < 3; ++i) {
            if (need[i] <= B.ray_out_bytes[i]) continue;
            if (B.ray_out[i]) TSDF_HIP(hipFree(B.ray_out[i]));
            B.ray_out[i] = nullptr;
            B.ray_out_bytes[i] = 0;
            TSDF_HIP(hipMalloc(&B.ray_out[i], need[i]));
            B.ray_out_bytes[i] = need[i];
        }
        dd = depth ? (float*)B.ray_out[0] : nullptr;
        dn = normals ? (float*)B.ray_out[1] : nullptr;
        dc = colors ? (unsigned char*)B.ray_out[2] : nullptr;
    }
    a.depth = dd;
    a.normals = dn;
    a.colors = dc;
    const unsigned grid = (unsigned)((a.n_tiles + kRayWG / 64 - 1) / (kRayWG / 64));
    if (S.table) hipLaunchKernelGGL(k_raycast<true>, dim3(grid), dim3(kRayWG), 0, B.stream, a);
    else hipLaunchKernelGGL(k_raycast<false>, dim3(grid), dim3(kRayWG), 0, B.stream, a);
    hipError_t e = hipGetLastError();
    if (timed && e == hipSuccess) e = hipEventRecord(ev[2], B.stream);
    if (!dev) {
        if (depth && e == hipSuccess) e = hipMemcpyAsync(depth, dd, px * sizeof(float), hipMemcpyDeviceToHost, B.stream);
        if (normals && e == hipSuccess) e = hipMemcpyAsync(normals, dn, px * 3 * sizeof(float), hipMemcpyDeviceToHost, B.stream);
        if (colors && e == hipSuccess) e = hipMemcpyAsync(colors, dc, px * 3, hipMemcpyDeviceToHost, B.stream);
    }
    if (e == hipSuccess && (!dev || !(flags & TSDF_ASYNC))) e = hipStreamSynchronize(B.stream);
    if (timed && e == hipSuccess) {
        float live_ms = 0.0f, march_ms = 0.0f;
        e = hipEventElapsedTime(&live_ms, ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&march_ms, ev[1], ev[2]);
        g_last_ms[0] = live_ms;
        g_last_ms[1] = march_ms;
    }
    if (e != hipSuccess) r = set_error(TSDF_E_HIP, "raycast: %s", hipGetErrorString(e));
    return r;
}

}  // namespace

extern "C" {

int tsdf_dense_raycast(tsdf_dense_t* h, int height, int width, const double K[9], const double cam_pose[16],
                       double z_near, double z_far, double z_step, float* depth, float* normals, uint8_t* colors,
                       int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return raycast(S, height, width, K, cam_pose, z_near, z_far, z_step, depth, normals, colors, flags);
}

int tsdf_hash_raycast(tsdf_hash_t* h, int height, int width, const double K[9], const double cam_pose[16],
                      double z_near, double z_far, double z_step, float* depth, float* normals, uint8_t* colors,
                      int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return raycast(S, height, width, K, cam_pose, z_near, z_far, z_step, depth, normals, colors, flags);
}

int tsdf_raycast_last_ms(double* live_ms, double* march_ms) {
    if (!live_ms || !march_ms) return set_error(TSDF_E_ARG, "null pointer");
    *live_ms = g_last_ms[0];
    *march_ms = g_last_ms[1];
    return TSDF_OK;
}

}  // extern "C"
