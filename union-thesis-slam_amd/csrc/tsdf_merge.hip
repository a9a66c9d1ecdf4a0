// tsdf_merge.hip -- merge one fused volume into another under a rigid transform:
// every destination voxel is taken to the source's index space, the source's stored tsdf is sampled
// trilinearly there (tsdf_cell.h, the raycast's and the tracker's cell) and blended into the voxel by
// the integrate's exact update.  Restated by tests/merge_ref.py and matched byte for byte: every
// operation below is a separately rounded f32 operation in that file's order.
//
// One wave per destination brick, a lane per (x, y), the 8 z voxels in registers, 16-byte loads and
// stores per field; a brick without a sample is not written.  The source is read by gathers.  No
// floating-point atomics: a voxel is written by its own lane, the counters are integers.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "tsdf_cell.h"
#include "tsdf_host.h"

using namespace tsdf;

namespace {

constexpr int kMergeWG = 256;
// what a launch does: the dense destination's one pass; the hash destination's marking pass (which
// bricks receive a sample: they get blocks) and its pass over those bricks
enum MergeMode { kMergeDense = 0, kMergeMark = 1, kMergeBlocks = 2 };

struct MergeArgs {
    Vol dv;
    Pool dpool;
    Table dt;  // hash destination only
    SdfArgs s;  // the source, as the tracker's cell reads it: v, pool and (hash) t
    float A[9], b[3], rho;
    long long n;                // bricks to visit: all of them, or (kMergeBlocks) the list's
    const int* bricks;          // kMergeBlocks: destination bricks with a sample, increasing
    const int* blk;             // ... and the pool block of each
    int* mark;                  // kMergeMark: per brick 0 no sample, 1 a sample and a block, 2 a sample and no block
    const unsigned* seen;       // the source's observed bits: one per brick (dense) or pool block (hash)
    long long n_seen;
    unsigned long long* count;  // samples, bricks updated, bricks the cull let through (candidates)
};

// q_k of rule 1 from pxy = A_k0 x + A_k1 y
__device__ inline float merge_q(const MergeArgs& a, int k, float pxy, float z) { return (pxy + a.A[3 * k + 2] * z) + a.b[k]; }

// Can a voxel of the brick's box [lo, hi] (global indices) have its cell inside the source?  Every
// operation of q_k is monotonic in x, y and z, and so are its roundings and the floor: over the box
// floor(q_k) lies between its values at the 8 corners.  Exact: a skipped brick has no sample.  mn, mx:
// the source voxels (local indices, inside the source) the box's cells can start at.
__device__ inline bool merge_box_may(const MergeArgs& a, const int lo[3], const int hi[3], int mn[3], int mx[3]) {
    bool may = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mn[k] = INT_MAX, mx[k] = INT_MIN;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float x = (float)((s & 4) ? hi[0] : lo[0]), y = (float)((s & 2) ? hi[1] : lo[1]), z = (float)((s & 1) ? hi[2] : lo[2]);
            const int i0 = floor_i(merge_q(a, k, a.A[3 * k] * x + a.A[3 * k + 1] * y, z)) - a.s.v.off[k];
            mn[k] = min(mn[k], i0);
            mx[k] = max(mx[k], i0);
        }
        may = may && mx[k] >= 0 && mn[k] <= a.s.v.dims[k] - 1;
        mn[k] = max(mn[k], 0);
        mx[k] = min(mx[k], a.s.v.dims[k] - 1);
    }
    return may;
}

// Does a source brick that holds one of the voxels [mn, mx] have an observed voxel?  A sample needs
// weight > 0 at every corner it fetches, its first corner -- the voxel its cell starts at -- among
// them: without an observed voxel in those bricks the destination brick has no sample.  Exact, as the
// box test.  The wave's lanes take the source bricks in turn (a hash source: one probe each).
constexpr int kMergeSeenMax = 4096;  // source bricks looked at per destination brick; beyond: no cull
template <bool SHASH>
__device__ inline bool merge_seen_may(const MergeArgs& a, const int mn[3], const int mx[3]) {
    const int b0[3] = {mn[0] >> 3, mn[1] >> 3, mn[2] >> 3};
    const int n[3] = {(mx[0] >> 3) - b0[0] + 1, (mx[1] >> 3) - b0[1] + 1, (mx[2] >> 3) - b0[2] + 1};
    const long long total = (long long)n[0] * n[1] * n[2];
    if (total > kMergeSeenMax) return true;
    bool hit = false;
    for (int j = lane_id(); j < (int)total; j += 64) {
        const int bz = b0[2] + j % n[2], by = b0[1] + (j / n[2]) % n[1], bx = b0[0] + j / (n[2] * n[1]);
        const long long bit = SHASH ? (long long)hash_find(a.s.t, bx, by, bz, a.s.t.max_blocks)
                                    : ((long long)bx * a.s.v.nb[1] + by) * a.s.v.nb[2] + bz;
        hit = hit || (bit >= 0 && bit < a.n_seen && ((a.seen[bit >> 5] >> (bit & 31)) & 1u));
    }
    return __ballot(hit) != 0ull;
}

// Rules 1-4 for one destination voxel: true for a sample (u, its weight and its folded colour).
template <bool SHASH, bool VALUES>
__device__ inline bool merge_sample(const MergeArgs& a, const float pxy[3], float z, float* u, float* ws, float* cs) {
    float f[3], c[8], w[8];
    int l[3], n[3], blk[8];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float q = merge_q(a, k, pxy[k], z);
        const int i0 = floor_i(q);
        f[k] = q - (float)i0;
        n[k] = f[k] > 0.0f ? 1 : 0;
        l[k] = i0 - a.s.v.off[k];
    }
    if (sdf_cell<SHASH, true>(a.s, l, c, n, w, blk) < 4) return false;  // outside (2), or a corner's weight <= 0 (3)
    float wm = w[0];
#pragma unroll
    for (int s = 1; s < 8; ++s) wm = fminf(wm, w[s]);
    if (VALUES) {
        *u = fminf(1.0f, fmaxf(-1.0f, a.rho * trilinear(c, f)));
        *ws = wm;
        const int h[3] = {f[0] >= 0.5f ? 1 : 0, f[1] >= 0.5f ? 1 : 0, f[2] >= 0.5f ? 1 : 0};  // (then n = 1)
        const int x = l[0] + h[0], y = l[1] + h[1], zz = l[2] + h[2];
        if (SHASH) {
            const int sc = h[0] * 4 + h[1] * 2 + h[2];
            int b = blk[0];
#pragma unroll
            for (int s = 1; s < 8; ++s) b = s == sc ? blk[s] : b;
            float unused;
            hash_block_voxel<true>(a.s.t, a.s.pool, b, x, y, zz, cs, &unused);
        } else {
            *cs = a.s.pool.color[dense_index(a.s.v, x, y, zz)];
        }
    }
    return true;
}

// b, g, r of a folded colour: the floor formulas of the integrate's exact update path (tsdf_device.h)
__device__ inline void merge_decode(float c, float* b, float* g, float* r) {
    *b = floorf(c / 65536.0f);
    *g = floorf((c - *b * 65536.0f) / 256.0f);
    *r = c - *b * 65536.0f - *g * 256.0f;
}

// The source's observed bits.  Dense: the bit of brick b is set when one of its voxels has weight > 0;
// one wave per brick, 16-byte loads.  Hash: the bit of a pool block is set when one of its voxels with
// an entry has weight > 0; 64 table slots per wave and step, the wave then takes the blocks in turn
// (the raycast's live-bit passes, with the merge's predicate).
__global__ __launch_bounds__(256) void k_merge_seen_dense(Pool pool, unsigned* seen, long long n_bricks) {
    const int lane = lane_id();
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long b = wave; b < n_bricks; b += nw) {
        const float4* pw = (const float4*)(pool.weight + (size_t)b * kBrickVox + (size_t)lane * 8);
        const float4 w0 = pw[0], w1 = pw[1];
        const bool any = w0.x > 0.0f || w0.y > 0.0f || w0.z > 0.0f || w0.w > 0.0f || w1.x > 0.0f || w1.y > 0.0f || w1.z > 0.0f || w1.w > 0.0f;
        if (__ballot(any) && lane == 0) atomicOr(&seen[b >> 5], 1u << (b & 31));
    }
}

__global__ __launch_bounds__(256) void k_merge_seen_hash(Table t, Pool pool, unsigned* seen, long long n_seen) {
    const int lane = lane_id();
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long base = wave * 64; base < t.capacity; base += nw * 64) {
        const long long s = base + lane;
        int blk = -1;
        if (s < t.capacity) {
            const unsigned long long key = coh_load(&t.keys[s]);
            if (key != kEmpty && key != kTomb) blk = coh_load(&t.vals[s]);
        }
        unsigned long long m = __ballot(blk >= 0 && blk < t.max_blocks && blk < n_seen);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int b = __shfl(blk, src);
            bool any = false;
            for (int j = 0; j < kBrickVox / 64; ++j) {
                const int local = j * 64 + lane;  // (x*8 + y)*8 + z; entry bit: word z, bit x*8 + y
                const unsigned long long word = coh_load(&t.occ[(size_t)b * 8 + (local & 7)]);
                if ((word >> (local >> 3)) & 1ull) any = any || pool.weight[(size_t)b * kBrickVox + local] > 0.0f;
            }
            if (__ballot(any) && lane == 0) atomicOr(&seen[b >> 5], 1u << (b & 31));
        }
    }
}

template <bool SHASH, int MODE>
__global__ __launch_bounds__(kMergeWG) void k_merge(MergeArgs a) {
    const int lane = lane_id();
    const int lx = lane >> 3, ly = lane & 7;
    const long long wave = ((long long)blockIdx.x * kMergeWG + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * kMergeWG) >> 6;
    const Vol& dv = a.dv;
    unsigned long long n_samples = 0, n_bricks = 0, n_cand = 0;
    for (long long i = wave; i < a.n; i += nw) {
        const int brick = MODE == kMergeBlocks ? a.bricks[i] : (int)i;
        const int bz = brick % dv.nb[2], by = (brick / dv.nb[2]) % dv.nb[1], bx = brick / (dv.nb[1] * dv.nb[2]);
        const int b0[3] = {bx * 8, by * 8, bz * 8};
        int lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = dv.off[k] + b0[k];
            hi[k] = dv.off[k] + min(b0[k] + 7, dv.dims[k] - 1);
        }
        // (the list of kMergeBlocks holds the bricks the marking pass found a sample in)
        int mn[3], mx[3];
        if (MODE != kMergeBlocks && (!merge_box_may(a, lo, hi, mn, mx) || !merge_seen_may<SHASH>(a, mn, mx))) {
            if (MODE == kMergeMark && lane == 0) a.mark[brick] = 0;
            continue;
        }
        ++n_cand;
        const bool in_xy = b0[0] + lx < dv.dims[0] && b0[1] + ly < dv.dims[1];
        const float x = (float)(lo[0] + lx), y = (float)(lo[1] + ly);
        float pxy[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) pxy[k] = a.A[3 * k] * x + a.A[3 * k + 1] * y;

        if (MODE == kMergeMark) {
            bool any = false;
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                float u, ws, cs;
                any = any || (in_xy && b0[2] + k < dv.dims[2] && merge_sample<SHASH, false>(a, pxy, (float)(lo[2] + k), &u, &ws, &cs));
            }
            const bool hit = __ballot(any) != 0ull;
            if (lane == 0) a.mark[brick] = !hit ? 0 : hash_find(a.dt, bx, by, bz, a.dt.max_blocks) >= 0 ? 1 : 2;
            continue;
        }

        const size_t base = (size_t)(MODE == kMergeBlocks ? a.blk[i] : brick) * kBrickVox + (size_t)lane * 8;
        float ts[8], ws[8], cs[8];
        {
            const float4 *pt = (const float4*)(a.dpool.tsdf + base), *pw = (const float4*)(a.dpool.weight + base),
                         *pc = (const float4*)(a.dpool.color + base);
            const float4 t0 = pt[0], t1 = pt[1], w0 = pw[0], w1 = pw[1], c0 = pc[0], c1 = pc[1];
            ts[0] = t0.x, ts[1] = t0.y, ts[2] = t0.z, ts[3] = t0.w, ts[4] = t1.x, ts[5] = t1.y, ts[6] = t1.z, ts[7] = t1.w;
            ws[0] = w0.x, ws[1] = w0.y, ws[2] = w0.z, ws[3] = w0.w, ws[4] = w1.x, ws[5] = w1.y, ws[6] = w1.z, ws[7] = w1.w;
            cs[0] = c0.x, cs[1] = c0.y, cs[2] = c0.z, cs[3] = c0.w, cs[4] = c1.x, cs[5] = c1.y, cs[6] = c1.z, cs[7] = c1.w;
        }
        unsigned long long got[8];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float u = 0.0f, w_s = 0.0f, c_s = 0.0f;
            const bool ok = in_xy && b0[2] + k < dv.dims[2] && merge_sample<SHASH, true>(a, pxy, (float)(lo[2] + k), &u, &w_s, &c_s);
            got[k] = __ballot(ok);
            any = any || ok;
            if (ok) {
                const float w_d = ws[k], w_n = w_d + w_s;
                const float t_n = (float)(((double)(w_d * ts[k]) + (double)(w_s * u)) / (double)w_n);
                float ob, og, orr, nb, ng, nr;
                merge_decode(cs[k], &ob, &og, &orr);
                merge_decode(c_s, &nb, &ng, &nr);
                const float cb = fminf(255.0f, rintf((w_d * ob + w_s * nb) / w_n));
                const float cg = fminf(255.0f, rintf((w_d * og + w_s * ng) / w_n));
                const float cr = fminf(255.0f, rintf((w_d * orr + w_s * nr) / w_n));
                ts[k] = t_n;
                ws[k] = w_n;
                cs[k] = cb * 65536.0f + cg * 256.0f + cr;
            }
        }
        if (__ballot(any) == 0ull) continue;  // (kMergeBlocks: the marking pass found a sample, so not taken)
        {
            float4 *pt = (float4*)(a.dpool.tsdf + base), *pw = (float4*)(a.dpool.weight + base), *pc = (float4*)(a.dpool.color + base);
            pt[0] = make_float4(ts[0], ts[1], ts[2], ts[3]);
            pt[1] = make_float4(ts[4], ts[5], ts[6], ts[7]);
            pw[0] = make_float4(ws[0], ws[1], ws[2], ws[3]);
            pw[1] = make_float4(ws[4], ws[5], ws[6], ws[7]);
            pc[0] = make_float4(cs[0], cs[1], cs[2], cs[3]);
            pc[1] = make_float4(cs[4], cs[5], cs[6], cs[7]);
        }
        ++n_bricks;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            n_samples += (unsigned long long)__popcll(got[k]);
            // the sampled voxels' entries: word z, bit x*8 + y = the lane (this wave owns the block)
            if (MODE == kMergeBlocks && lane == 0 && got[k]) atomicOr(&a.dt.occ[(size_t)a.blk[i] * 8 + k], got[k]);
        }
    }
    if (MODE != kMergeBlocks && lane == 0 && n_cand) atomicAdd(&a.count[2], n_cand);
    if (MODE != kMergeMark && lane == 0 && n_bricks) {
        atomicAdd(&a.count[0], n_samples);
        atomicAdd(&a.count[1], n_bricks);
    }
}

template <int MODE>
int launch_merge(const MergeArgs& a, bool shash, const Base& B) {
    if (a.n <= 0) return TSDF_OK;
    // 8 workgroups per CU stride through the bricks.  A workgroup per 4 bricks (65,536 of them at 512^3)
    // was measured on the same workload: as fast or slower with a dense source or a hash destination,
    // by up to 1.9x, and faster only from a hash into a dense volume, by up to 1.26x (profiles/r17_merge/).
    const unsigned grid = (unsigned)std::min<long long>((a.n + kMergeWG / 64 - 1) / (kMergeWG / 64), (long long)B.n_cu * 8);
    if (shash) hipLaunchKernelGGL((k_merge<true, MODE>), dim3(grid), dim3(kMergeWG), 0, B.stream, a);
    else hipLaunchKernelGGL((k_merge<false, MODE>), dim3(grid), dim3(kMergeWG), 0, B.stream, a);
    TSDF_HIP(hipGetLastError());
    return TSDF_OK;
}

// HIP-event time of the calling thread's last merge on a destination with profiling on, and the
// destination bricks its cull (box test and observed bits) let through: tsdf_merge_last_profile, the
// merge's counterpart of tsdf_raycast_last_ms and tsdf_track_last_ms
thread_local double g_merge_ms = -1.0;
thread_local long long g_merge_candidates = -1;

int check_transform(const double* T) {
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return set_error(TSDF_E_ARG, "src_to_dst[%d] is not finite", i);
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0)
        return set_error(TSDF_E_ARG, "the last row of src_to_dst must be 0 0 0 1");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
            if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-6))
                return set_error(TSDF_E_ARG, "the rotation of src_to_dst is not orthonormal ((R^T R)[%d][%d] = %.9g)", i, j, d);
        }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) +
                       T[2] * (T[4] * T[9] - T[5] * T[8]);
    if (!(std::fabs(det - 1.0) <= 1e-6)) return set_error(TSDF_E_ARG, "the rotation of src_to_dst has determinant %.9g, not +1", det);
    return TSDF_OK;
}

// a handle a merge serves: a whole volume or a slab shard
int check_side(const Base& B, bool hash, const char* side) {
    if (!hash && (B.vol.xstride != kBrickEdge || B.vol.xodd != kBrickEdge))
        return set_error(TSDF_E_ARG, "the %s is a cyclic column shard: a merge takes whole volumes and slab shards", side);
    if (hash && B.vol.n_shards > 1)
        return set_error(TSDF_E_ARG, "the %s is a hash shard (%d of %d): a merge takes whole tables", side, B.vol.shard, B.vol.n_shards);
    return TSDF_OK;
}

// D, S: the handles' state after their deferred frames ran (the *_ray_source calls); dh: the hash
// destination's handle.
int merge(const RaySource& D, tsdf_hash_t* dh, const RaySource& S, const double* T, tsdf_merge_info_t* info) {
    Base& DB = *D.b;
    const Base& SB = *S.b;
    const Vol &dv = DB.vol, &sv = SB.vol;
    MergeArgs a{};
    // the host side of §7h, in f64, each value rounded to f32 once; three-term sums are (a + b) + c
    const double s = dv.vs / sv.vs;
    const double d[3] = {(double)dv.origin[0] - T[3], (double)dv.origin[1] - T[7], (double)dv.origin[2] - T[11]};
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) a.A[3 * k + j] = (float)(T[4 * j + k] * s);
        a.b[k] = (float)((((T[k] * d[0] + T[4 + k] * d[1]) + T[8 + k] * d[2]) - (double)sv.origin[k]) / sv.vs);
    }
    a.rho = (float)(sv.trunc / dv.trunc);
    a.s.v = sv;
    a.s.pool = SB.pool;
    if (S.table) a.s.t = *S.table;

    TSDF_HIP(hipStreamSynchronize(SB.stream));  // the source is complete before the destination's stream reads it
    DB.touch_state();
    unsigned long long count[3] = {0, 0, 0};  // (read back: declared before the owner of what it is read from)
    std::vector<int> mark, blocks;
    DevBufs bufs;
    TSDF_TRY(bufs.alloc(&a.count, 3));
    TSDF_HIP(hipMemsetAsync(a.count, 0, sizeof(count), DB.stream));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 2; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};
    const bool timed = DB.prof.on;
    float ms = 0.0f;
    if (timed)
        for (auto& e : ev) TSDF_HIP(hipEventCreate(&e));
    long long allocated = 0;
    // the source's observed bits, for the cull (merge_seen_may)
    a.n_seen = S.table ? S.table->max_blocks : SB.n_bricks;
    unsigned* seen = nullptr;
    const size_t seen_words = (size_t)((a.n_seen + 31) / 32);
    TSDF_TRY(bufs.alloc(&seen, seen_words));
    a.seen = seen;
    auto launch_seen = [&]() -> int {
        TSDF_HIP(hipMemsetAsync(seen, 0, sizeof(unsigned) * seen_words, DB.stream));
        const unsigned grid = (unsigned)DB.n_cu * 8;
        if (S.table) hipLaunchKernelGGL(k_merge_seen_hash, dim3(grid), dim3(256), 0, DB.stream, *S.table, SB.pool, seen, a.n_seen);
        else hipLaunchKernelGGL(k_merge_seen_dense, dim3(grid), dim3(256), 0, DB.stream, SB.pool, seen, SB.n_bricks);
        TSDF_HIP(hipGetLastError());
        return TSDF_OK;
    };
    if (!dh) {
        a.dv = dv;
        a.dpool = DB.pool;
        a.n = DB.n_bricks;
        if (timed) TSDF_HIP(hipEventRecord(ev[0], DB.stream));
        TSDF_TRY(launch_seen());
        TSDF_TRY(launch_merge<kMergeDense>(a, S.table != nullptr, DB));
        if (timed) TSDF_HIP(hipEventRecord(ev[1], DB.stream));
    } else {
        // which bricks receive a sample: exactly those get blocks, so none is left without an entry
        a.dv = dv;
        a.dt = *D.table;
        a.n = DB.n_bricks;
        mark.resize((size_t)DB.n_bricks);
        TSDF_TRY(bufs.alloc(&a.mark, (size_t)DB.n_bricks));
        if (timed) TSDF_HIP(hipEventRecord(ev[0], DB.stream));
        TSDF_TRY(launch_seen());
        TSDF_TRY(launch_merge<kMergeMark>(a, S.table != nullptr, DB));
        if (timed) TSDF_HIP(hipEventRecord(ev[1], DB.stream));
        TSDF_HIP(hipMemcpyAsync(mark.data(), a.mark, sizeof(int) * mark.size(), hipMemcpyDeviceToHost, DB.stream));
        TSDF_HIP(hipStreamSynchronize(DB.stream));
        if (timed) TSDF_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        std::vector<int> bricks;
        std::vector<unsigned long long> keys;
        for (long long b = 0; b < DB.n_bricks; ++b) {
            if (!mark[(size_t)b]) continue;
            allocated += mark[(size_t)b] == 2;
            bricks.push_back((int)b);
            keys.push_back(pack_key((int)(b / ((long long)dv.nb[1] * dv.nb[2])), (int)((b / dv.nb[2]) % dv.nb[1]), (int)(b % dv.nb[2])));
        }
        if (!bricks.empty()) {
            int* dblk = nullptr;
            TSDF_TRY(hash_find_or_insert_blocks(dh, keys, bufs, &dblk));  // (the table and the pool may have moved)
            blocks.resize(bricks.size());
            TSDF_HIP(hipMemcpyAsync(blocks.data(), dblk, sizeof(int) * blocks.size(), hipMemcpyDeviceToHost, DB.stream));
            TSDF_HIP(hipStreamSynchronize(DB.stream));
            // (insert_block_keys made room for every key first, so this does not happen short of a refused
            // growth; then, as after a failed tsdf_hash_import_blocks, the blocks inserted so far stay in
            // the table without entries and no voxel has changed -- tsdf_hash_reset or a later merge or
            // import of those blocks puts the table right)
            for (int b : blocks)
                if (b < 0 || b >= D.table->max_blocks) return set_error(TSDF_E_CAPACITY, "hash merge failed (table or pool full)");
            int* dbricks = nullptr;
            TSDF_TRY(bufs.alloc(&dbricks, bricks.size()));
            TSDF_HIP(hipMemcpyAsync(dbricks, bricks.data(), sizeof(int) * bricks.size(), hipMemcpyHostToDevice, DB.stream));
            a.dt = *D.table;
            a.dpool = DB.pool;
            a.bricks = dbricks;
            a.blk = dblk;
            a.n = (long long)bricks.size();
            a.mark = nullptr;
            if (timed) TSDF_HIP(hipEventRecord(ev[0], DB.stream));
            TSDF_TRY(launch_merge<kMergeBlocks>(a, S.table != nullptr, DB));
            if (timed) TSDF_HIP(hipEventRecord(ev[1], DB.stream));
        }
    }
    TSDF_HIP(hipMemcpyAsync(count, a.count, sizeof(count), hipMemcpyDeviceToHost, DB.stream));
    TSDF_HIP(hipStreamSynchronize(DB.stream));
    if (timed) {
        float last = 0.0f;
        if (!dh || a.bricks) TSDF_HIP(hipEventElapsedTime(&last, ev[0], ev[1]));
        g_merge_ms = (double)ms + (double)last;
    }
    g_merge_candidates = (long long)count[2];
    // canonical state in, canonical state out (integer weights, the least of them; colours blended by
    // the exact path's rint); otherwise the destination is looked at
    if (!(dv.canon && sv.canon)) {
        if (dh) TSDF_TRY(hash_recheck_canon(dh));
        else TSDF_TRY(DB.check_canon(DB.n_bricks * kBrickVox));
    }
    if (info) {
        info->samples = (int64_t)count[0];
        info->bricks_updated = (int64_t)count[1];
        info->blocks_allocated = (int64_t)allocated;
    }
    return TSDF_OK;
}

int merge_call(tsdf_dense_t* dd, tsdf_hash_t* dh, tsdf_dense_t* sd, tsdf_hash_t* sh, const double* T, tsdf_merge_info_t* info,
               int flags) {
    if (!dd && !dh) return set_error(TSDF_E_ARG, "null destination handle");
    if (!T) return set_error(TSDF_E_ARG, "null src_to_dst");
    if ((sd != nullptr) == (sh != nullptr)) return set_error(TSDF_E_ARG, "give exactly one of src_dense and src_hash");
    if (flags != 0) return set_error(TSDF_E_ARG, "merge flags must be 0 (got %d)", flags);
    if ((dd && dd == sd) || (dh && dh == sh)) return set_error(TSDF_E_ARG, "the source and the destination are the same handle");
    TSDF_TRY(check_transform(T));
    const Base& DB = dd ? *dense_base(dd) : *hash_base(dh);
    const Base& SB = sd ? *dense_base(sd) : *hash_base(sh);
    if (DB.device != SB.device)
        return set_error(TSDF_E_ARG, "the handles live on different devices (%d and %d)", SB.device, DB.device);
    TSDF_TRY(check_side(DB, dh != nullptr, "destination"));
    TSDF_TRY(check_side(SB, sh != nullptr, "source"));
    if (SB.vol.trunc < DB.vol.trunc)
        return set_error(TSDF_E_ARG, "the source's truncation (%g) is below the destination's (%g): its band cannot say what "
                                     "the destination's needs (no downsampling)", SB.vol.trunc, DB.vol.trunc);
    RaySource D, S;  // (these run the handles' deferred frames)
    TSDF_TRY(sd ? dense_ray_source(sd, &S) : hash_ray_source(sh, &S));
    TSDF_TRY(dd ? dense_ray_source(dd, &D) : hash_ray_source(dh, &D));
    return merge(D, dh, S, T, info);
}

}  // namespace

extern "C" {

int tsdf_dense_merge(tsdf_dense_t* dst, tsdf_dense_t* src_dense, tsdf_hash_t* src_hash, const double src_to_dst[16],
                     tsdf_merge_info_t* info, int flags) {
    return merge_call(dst, nullptr, src_dense, src_hash, src_to_dst, info, flags);
}

int tsdf_hash_merge(tsdf_hash_t* dst, tsdf_dense_t* src_dense, tsdf_hash_t* src_hash, const double src_to_dst[16],
                    tsdf_merge_info_t* info, int flags) {
    return merge_call(nullptr, dst, src_dense, src_hash, src_to_dst, info, flags);
}

int tsdf_merge_last_profile(double* ms, int64_t* candidate_bricks) {
    if (!ms || !candidate_bricks) return set_error(TSDF_E_ARG, "null pointer");
    *ms = g_merge_ms;
    *candidate_bricks = g_merge_candidates;
    return TSDF_OK;
}

}  // extern "C"
