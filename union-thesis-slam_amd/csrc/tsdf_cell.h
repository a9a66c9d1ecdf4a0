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
