// tsdf_cell.h -- the trilinear cell of the stored tsdf: the
// arithmetic the raycast (tsdf_raycast.hip) and the point-to-SDF tracker (tsdf_track.hip, §7g)
// share, operation by operation -- both are restated in NumPy and matched bit for bit, so there is
// one copy.  A cell is the 8 voxels i0 + {0,1}^3 around a point q of index space (voxel centres at
// integer indices), c[dx*4 + dy*2 + dz] their tsdf and t = q - i0 the fractions.
#pragma once
#include "tsdf_device.h"

namespace tsdf {

__device__ inline float lerp(float a, float b, float t) { return a + t * (b - a); }

// floor(q) as an int, safe for any q (NaN and huge values land far outside every volume)
__device__ inline int floor_i(float q) { return (int)floorf(fminf(fmaxf(q, -1.0e9f), 1.0e9f)); }

// ---- dense: brick b = (bx*nb1 + by)*nb2 + bz, local voxel (x*8 + y)*8 + z ---------------------
__device__ inline size_t dense_index(const Vol& v, int x, int y, int z) {
    const size_t b = ((size_t)(x >> 3) * v.nb[1] + (y >> 3)) * v.nb[2] + (z >> 3);
    return b * kBrickVox + (size_t)(((x & 7) * 8 + (y & 7)) * 8 + (z & 7));
}

// ---- hash: voxel (x, y, z) of pool block blk (-1: no block); without an entry: (1, 0), colour 0.
// The entry words and the table are read with coherent loads (tsdf_device.h, coh_load).
template <bool COLOR>
__device__ inline void hash_block_voxel(const Table& tb, const Pool& pool, int blk, int x, int y, int z, float* t, float* w) {
    *t = COLOR ? 0.0f : 1.0f;
    *w = 0.0f;
    if (blk < 0) return;
    const unsigned long long word = coh_load(&tb.occ[(size_t)blk * 8 + (z & 7)]);
    if (!((word >> ((x & 7) * 8 + (y & 7))) & 1ull)) return;
    const size_t j = (size_t)blk * kBrickVox + (size_t)(((x & 7) * 8 + (y & 7)) * 8 + (z & 7));
    if (COLOR) {
        *t = pool.color[j];
    } else {
        *t = pool.tsdf[j];
        *w = pool.weight[j];
    }
}

// ---- the cell of a handle's volume: what the tracker (tsdf_track.hip), the sampler and the merge
// (tsdf_merge.hip) read it through ------------------------------------------------------------------
struct SdfArgs {
    Vol v;
    Pool pool;
    Table t;             // hash only
    int hash;
    float Qr[9], Qo[3];  // the guess camera's frame to index space: R_G / vs, (t_G - origin) / vs
    float sc, trunc;     // trunc / vs (tsdf per voxel to metres per metre), trunc
};

// The cell at local index l (corners l + {0,1}^3, c[dx*4 + dy*2 + dz]) and its code: 2, 3, 4 or 6; c
// is filled for 4 and 6.  Dense: the 16 gathers are issued together.  Hash: a cell touches 1, 2, 4
// or 8 blocks ((l & 7) == 7 on an axis crosses to the next); each distinct block is probed once.
// NK (the merge): n[k] = 0 marks a degenerate axis -- its upper neighbour has trilinear
// weight zero and is neither fetched nor required, both corners are the voxel l[k]; w_out / blk_out:
// the corners' weights and (hash) pool blocks.  Without NK none of the three is read or written.
template <bool HASH, bool NK = false>
__device__ inline int sdf_cell(const SdfArgs& x, const int l[3], float c[8], const int* n = nullptr, float* w_out = nullptr,
                            int* blk_out = nullptr) {
    for (int d = 0; d < 3; ++d)
        if (l[d] < 0 || l[d] > x.v.dims[d] - (NK ? 1 + n[d] : 2)) return 2;
    float w[8];
    if (HASH) {
        const bool cr[3] = {(!NK || n[0]) && (l[0] & 7) == 7, (!NK || n[1]) && (l[1] & 7) == 7, (!NK || n[2]) && (l[2] & 7) == 7};
        int blk[8];  // the pool block of corner s
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int ox = s >> 2, oy = (s >> 1) & 1, oz = s & 1;
            if (ox && !cr[0]) blk[s] = blk[s & 3];
            else if (oy && !cr[1]) blk[s] = blk[s & 5];
            else if (oz && !cr[2]) blk[s] = blk[s & 6];
            else {
                const int bx = (l[0] >> 3) + ox, by = (l[1] >> 3) + oy, bz = (l[2] >> 3) + oz;
                blk[s] = bx < x.v.nb[0] && by < x.v.nb[1] && bz < x.v.nb[2] ? hash_find(x.t, bx, by, bz, x.t.max_blocks) : -1;
            }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s)
            hash_block_voxel<false>(x.t, x.pool, blk[s], l[0] + (NK ? (s >> 2) * n[0] : (s >> 2)), l[1] + (NK ? ((s >> 1) & 1) * n[1] : ((s >> 1) & 1)),
                                    l[2] + (NK ? (s & 1) * n[2] : (s & 1)), &c[s], &w[s]);
        if (NK) {
#pragma unroll
            for (int s = 0; s < 8; ++s) blk_out[s] = blk[s];
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const size_t j = dense_index(x.v, l[0] + (NK ? (s >> 2) * n[0] : (s >> 2)), l[1] + (NK ? ((s >> 1) & 1) * n[1] : ((s >> 1) & 1)),
                                          l[2] + (NK ? (s & 1) * n[2] : (s & 1)));
            c[s] = x.pool.tsdf[j];
            w[s] = x.pool.weight[j];
        }
    }
    bool seen = true, flat = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        seen = seen && w[s] > 0.0f;
        flat = flat || fabsf(c[s]) >= 1.0f;
        if (NK) w_out[s] = w[s];
    }
    return !seen ? 3 : flat ? 4 : 6;
}

// lerp_z, then lerp_y, then lerp_x
__device__ inline float trilinear(const float c[8], const float t[3]) {
    const float c00 = lerp(c[0], c[1], t[2]), c01 = lerp(c[2], c[3], t[2]);
    const float c10 = lerp(c[4], c[5], t[2]), c11 = lerp(c[6], c[7], t[2]);
    return lerp(lerp(c00, c01, t[1]), lerp(c10, c11, t[1]), t[0]);
}

// the gradient of the interpolant in index axes (per voxel), not normalised
__device__ inline void cell_gradient(const float c[8], const float t[3], float g[3]) {
    g[0] = lerp(lerp(c[4] - c[0], c[5] - c[1], t[2]), lerp(c[6] - c[2], c[7] - c[3], t[2]), t[1]);
    g[1] = lerp(lerp(c[2] - c[0], c[3] - c[1], t[2]), lerp(c[6] - c[4], c[7] - c[5], t[2]), t[0]);
    g[2] = lerp(lerp(c[1] - c[0], c[3] - c[2], t[1]), lerp(c[5] - c[4], c[7] - c[6], t[1]), t[0]);
}

}  // namespace tsdf
