// tsdf_mesh.hip -- mesh / point-cloud extraction from a dense volume: the
// MI355X replacement of get_mesh / get_point_cloud (grid_fusion.py:322-360), which run
// skimage.measure.marching_cubes_lewiner on the host.
//
// Marching cubes at level 0 over the handle's brick layout, in three passes:
//   k_mc_classify  one thread per voxel (C-order): the voxel's three +axis grid edges that cross
//                  0 (a vertex each) and, for voxels that anchor a cell, the cell's case and
//                  triangle count;
//   (exclusive scans of both counts: vertex and triangle offsets, in C-order, entry n the total)
//   k_mc_vertices  one thread per voxel with crossings: vertex position (linear interpolation,
//                  index space, then world = p * voxel_size + origin in f32 as NumPy does),
//                  normal (interpolated central-difference gradient, pointing to positive tsdf)
//                  and colour (grid_fusion.py:336-346: the voxel at round(p), decoded);
//   k_mc_triangles one thread per cell: the case's triangles, each cube edge mapped to the
//                  global vertex id of its grid edge.
// Vertices are ordered by (voxel, axis) in C-order and shared between cells (an indexed mesh
// like skimage's); the case table comes from one rule (tsdf_mc_table, oracle/mc_table.py).
// The voxel hash has its own mesher over the table's live blocks (hash_extract_mesh, further
// down): the same mesh as the dense passes give on the densified table, from the same device
// functions (mc_edges, mc_case, mc_grad, mc_vertex), without a pass over the extent.
// Host side, both meshers alike: a call's scratch is owned by one DevBufs (tsdf_host.h) and laid
// out by a Layout (tsdf_scratch.h), one allocation per stage -- the dense mesher has one stage,
// the hash's four -- freed together at the end of the call; the outputs are Mesh::alloc's, kept
// only if the extraction reaches its end (MeshGuard); every HIP call returns through TSDF_HIP.
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

#include "tsdf_host.h"

using namespace tsdf;

namespace {

// ---- case table (the rule of oracle/mc_table.py) ------------------------------------------------
struct McTable {
    signed char tri[256][16];  // edge ids, -1 padded
    unsigned char ntri[256];
};

McTable build_table() {
    McTable t;
    std::memset(t.tri, -1, sizeof(t.tri));
    int edge_of[8][8];
    int corner_pair[12][2];
    int ne = 0;
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) edge_of[a][b] = -1;
    for (int axis = 0; axis < 3; ++axis)
        for (int c = 0; c < 8; ++c)
            if (!((c >> axis) & 1)) {
                corner_pair[ne][0] = c;
                corner_pair[ne][1] = c | (1 << axis);
                edge_of[c][c | (1 << axis)] = edge_of[c | (1 << axis)][c] = ne;
                ++ne;
            }
    int faces[6][4];
    int nf = 0;
    for (int axis = 0; axis < 3; ++axis) {
        const int u = (axis + 1) % 3, v = (axis + 2) % 3;
        for (int side = 0; side < 2; ++side) {
            const int base = side << axis;
            int cyc[4] = {base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)};
            if (side == 0) std::swap(cyc[0], cyc[3]), std::swap(cyc[1], cyc[2]);  // reverse: CCW from outside
            for (int i = 0; i < 4; ++i) faces[nf][i] = cyc[i];
            ++nf;
        }
    }
    unsigned face_mask[12];  // bit 2 * axis + side: the two cube faces that hold the edge
    for (int e = 0; e < 12; ++e) {
        face_mask[e] = 0;
        for (int axis = 0; axis < 3; ++axis) {
            const int sa = (corner_pair[e][0] >> axis) & 1, sb = (corner_pair[e][1] >> axis) & 1;
            if (sa == sb) face_mask[e] |= 1u << (2 * axis + sa);
        }
    }
    for (int cfg = 0; cfg < 256; ++cfg) {
        int seg[12];
        for (int i = 0; i < 12; ++i) seg[i] = -1;
        auto in = [&](int c) { return (cfg >> c) & 1; };
        for (int f = 0; f < 6; ++f) {
            const int* cyc = faces[f];
            int n_in = 0;
            for (int i = 0; i < 4; ++i) n_in += in(cyc[i]);
            if (n_in == 0 || n_in == 4) continue;
            for (int i = 0; i < 4; ++i) {
                const int a = cyc[i], b = cyc[(i + 1) % 4];
                if (in(a) && !in(b)) {  // the walk leaves a run of inside corners at edge (a, b)
                    int j = i;
                    while (in(cyc[(j + 3) % 4])) j = (j + 3) % 4;
                    const int p = cyc[(j + 3) % 4], q = cyc[j];  // where the run was entered
                    seg[edge_of[a][b]] = edge_of[p][q];
                }
            }
        }
        int k = 0;
        bool left[12];
        for (int i = 0; i < 12; ++i) left[i] = seg[i] >= 0;
        for (int start = 0; start < 12; ++start) {
            if (!left[start]) continue;
            int loop[12], n = 0;
            int e = start;
            do {
                loop[n++] = e;
                left[e] = false;
                e = seg[e];
            } while (e != start);
            // fan from the first position whose diagonals all leave the cube's faces: a diagonal
            // between two crossings of one face lies in that face's plane, where the neighbouring
            // cell may emit the same edge (a non-manifold edge); such a position always exists
            int s = 0;
            for (; s < n; ++s) {
                bool ok = true;
                for (int i = 2; i + 1 < n; ++i) ok = ok && !(face_mask[loop[s]] & face_mask[loop[(s + i) % n]]);
                if (ok) break;
            }
            if (s == n) s = 0;  // (never: tests/test_mesh_cpu.py checks every case)
            for (int i = 1; i + 1 < n; ++i) {
                t.tri[cfg][k++] = (signed char)loop[s];
                t.tri[cfg][k++] = (signed char)loop[(s + i) % n];
                t.tri[cfg][k++] = (signed char)loop[(s + i + 1) % n];
            }
        }
        t.ntri[cfg] = (unsigned char)(k / 3);
    }
    return t;
}

const McTable& table() {
    static const McTable t = build_table();
    return t;
}

// cube edge e -> (corner offset bits of its lower corner, axis); edges are sorted by axis
__device__ inline void edge_anchor(int e, int& off, int& axis) {
    axis = e >> 2;
    const int r = e & 3;  // the two other coordinate bits, in increasing bit order
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    off = ((r & 1) << u) | (((r >> 1) & 1) << v);
}

// The table's loops wind around the inside corners; a triangle is emitted as (0, 2, 1), so the
// face normal points to positive tsdf like the vertex normals: corner j of a table triangle goes
// to slot tri_slot(j) of the face.
__device__ constexpr int tri_slot(int j) { return j == 0 ? 0 : 3 - j; }

// The volume as marching cubes sees it: rows of constant global x.  Local rows live in the
// handle's brick pool; rows owned by other shards (halo rows, exchanged by the caller) arrive as
// C-order (Y, Z) slices.  row_map[gx - xlo] says where global row gx is: >= 0 local row,
// <= -2 halo row -2-r, -1 absent.  Marching cubes runs over the global x range [xlo, xhi):
// gradients clamp there, x-edges and cells need gx + 1 < xhi.  A shard's "vertex rows" are its
// local rows plus each cap row (a halo row gx whose gx - 1 is local): the cells a shard owns are
// those anchored at its local rows, and a cap row carries the y/z-edge vertices of their +x faces
// (duplicates of the next shard's own vertices, identified by the same global key).
struct Grid {
    int Y, Z;
    int xlo, xhi;
    int nby, nbz;              // brick geometry of the local rows
    const int* row_map;        // [xhi - xlo]
    const int* vrow_gx;        // [nrows] global x of the vertex rows, increasing
    const unsigned char* vrow_cap;  // [nrows] 1: cap row (y/z-edge vertices only, no cells)
    const float* t;            // brick-layout state (local rows)
    const float* c;
    const float* ht;           // halo rows, C-order [n_halo][Y][Z]
    const float* hc;
};

__device__ inline float gval(const Grid& g, const float* brick, const float* halo, int gx, int y, int z) {
    const int r = g.row_map[gx - g.xlo];
    if (r >= 0) {
        const size_t b = ((size_t)(r >> 3) * g.nby + (y >> 3)) * g.nbz + (z >> 3);
        return brick[b * kBrickVox + (size_t)(((r & 7) * 8 + (y & 7)) * 8 + (z & 7))];
    }
    return halo[((size_t)(-2 - r) * g.Y + y) * g.Z + z];
}
__device__ inline float tval(const Grid& g, int gx, int y, int z) { return gval(g, g.t, g.ht, gx, y, z); }
__device__ inline float cval(const Grid& g, int gx, int y, int z) { return gval(g, g.c, g.hc, gx, y, z); }

// ---- the arithmetic of marching cubes, compiled into both meshers (dense bricks and halo rows
// below, the voxel hash's LDS tile further down) --------------------------------------------------
// V is the volume as a mesher sees it: t(x, y, z) / c(x, y, z) the tsdf / colour of a voxel of the
// meshed range, xlo / xhi / Y / Z the range the gradients clamp to.

// the voxel's +axis grid edges that cross 0 (bit a: axis a); xn: the voxel has a +x neighbour
template <class V>
__device__ inline unsigned mc_edges(const V& f, int x, int y, int z, bool xn) {
    const bool in0 = f.t(x, y, z) < 0.0f;
    unsigned bits = 0;
    if (xn && (f.t(x + 1, y, z) < 0.0f) != in0) bits |= 1u;
    if (y + 1 < f.Y && (f.t(x, y + 1, z) < 0.0f) != in0) bits |= 2u;
    if (z + 1 < f.Z && (f.t(x, y, z + 1) < 0.0f) != in0) bits |= 4u;
    return bits;
}

// case of the cell anchored at the voxel (all eight corners exist)
template <class V>
__device__ inline unsigned mc_case(const V& f, int x, int y, int z) {
    unsigned cube = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        cube |= (unsigned)(f.t(x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1)) < 0.0f) << c;
    return cube;
}

// central-difference gradient of the tsdf at a voxel (indices clamped at the faces of the
// meshed range)
template <class V>
__device__ inline void mc_grad(const V& f, int x, int y, int z, float out[3]) {
    out[0] = f.t(min(x + 1, f.xhi - 1), y, z) - f.t(max(x - 1, f.xlo), y, z);
    out[1] = f.t(x, min(y + 1, f.Y - 1), z) - f.t(x, max(y - 1, 0), z);
    out[2] = f.t(x, y, min(z + 1, f.Z - 1)) - f.t(x, y, max(z - 1, 0));
}

// vertex `id` of the grid edge from voxel (x, y, z) along axis a: v1 the voxel's tsdf, g1 its
// gradient (read with NRM only), o / vs the volume's origin and voxel size
template <bool NRM, class V>
__device__ inline void mc_vertex(const V& f, int x, int y, int z, int a, float v1, const float g1[3], const float o[3],
                                 float vs, size_t id, float* __restrict__ verts, float* __restrict__ normals,
                                 unsigned char* __restrict__ colors, long long* __restrict__ keys) {
    const int x2 = x + (a == 0), y2 = y + (a == 1), z2 = z + (a == 2);
    const float v2 = f.t(x2, y2, z2);
    const float t = (0.0f - v1) / (v2 - v1);
    float p[3] = {(float)x, (float)y, (float)z};
    p[a] = p[a] + t;
    for (int k = 0; k < 3; ++k) verts[3 * id + k] = p[k] * vs + o[k];  // verts * voxel_size + origin (f32)
    if (NRM) {
        float g2[3];
        mc_grad(f, x2, y2, z2, g2);
        float nrm[3];
        for (int k = 0; k < 3; ++k) nrm[k] = g1[k] + t * (g2[k] - g1[k]);
        const float len = __fsqrt_rn(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        for (int k = 0; k < 3; ++k) normals[3 * id + k] = len > 0.0f ? nrm[k] / len : 0.0f;
    }
    // grid_fusion.py:336-346: colour of the voxel at round(verts), decoded to uint8
    const int rx = (int)rintf(p[0]), ry = (int)rintf(p[1]), rz = (int)rintf(p[2]);
    const float cv = f.c(rx, ry, rz);
    const float cb = floorf(cv / 65536.0f);
    const float cg = floorf((cv - cb * 65536.0f) / 256.0f);
    const float cr = cv - cb * 65536.0f - cg * 256.0f;
    colors[3 * id + 0] = (unsigned char)(int)floorf(cr);
    colors[3 * id + 1] = (unsigned char)(int)floorf(cg);
    colors[3 * id + 2] = (unsigned char)(int)floorf(cb);
    // global identity of the vertex: (voxel, axis) in the unsharded volume's C-order
    keys[id] = ((((long long)x * f.Y) + y) * f.Z + z) * 3 + a;
}

// global key of the vertex on cube edge e of the cell anchored at (x, y, z)
__device__ inline long long mc_edge_key(int e, int x, int y, int z, int Y, int Z) {
    int off, axis;
    edge_anchor(e, off, axis);
    return ((((long long)(x + (off & 1)) * Y) + (y + ((off >> 1) & 1))) * Z + (z + ((off >> 2) & 1))) * 3 + axis;
}

// the dense mesher's volume
struct GridVol {
    const Grid& g;
    int xlo, xhi, Y, Z;
    __device__ explicit GridVol(const Grid& g_) : g(g_), xlo(g_.xlo), xhi(g_.xhi), Y(g_.Y), Z(g_.Z) {}
    __device__ float t(int x, int y, int z) const { return tval(g, x, y, z); }
    __device__ float c(int x, int y, int z) const { return cval(g, x, y, z); }
};

__global__ void k_mc_classify(Grid g, int nrows, const unsigned char* __restrict__ ntri,
                              unsigned char* __restrict__ ebits, unsigned char* __restrict__ cubes,
                              unsigned* __restrict__ vcnt, unsigned* __restrict__ tcnt) {
    const GridVol f(g);
    const size_t n = (size_t)nrows * g.Y * g.Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % g.Z);
        const size_t xy = i / g.Z;
        const int y = (int)(xy % g.Y), row = (int)(xy / g.Y);
        const int x = g.vrow_gx[row];
        const bool cap = g.vrow_cap[row] != 0;
        const bool xn = !cap && x + 1 < g.xhi;  // x-edge and cells only from local rows
        const unsigned bits = mc_edges(f, x, y, z, xn);
        unsigned cube = 0, nt = 0;
        if (xn && y + 1 < g.Y && z + 1 < g.Z) {
            cube = mc_case(f, x, y, z);
            nt = ntri[cube];
        }
        ebits[i] = (unsigned char)bits;
        cubes[i] = (unsigned char)cube;
        vcnt[i] = (unsigned)__popc(bits);
        tcnt[i] = nt;
    }
}

__global__ void k_mc_vertices(Grid g, int nrows, const unsigned char* __restrict__ ebits,
                              const unsigned* __restrict__ vbase, float ox, float oy, float oz, float vs,
                              float* __restrict__ verts, float* __restrict__ normals,
                              unsigned char* __restrict__ colors, long long* __restrict__ keys) {
    const GridVol f(g);
    const size_t n = (size_t)nrows * g.Y * g.Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned bits = ebits[i];
        if (!bits) continue;
        const int z = (int)(i % g.Z);
        const size_t xy = i / g.Z;
        const int y = (int)(xy % g.Y), x = g.vrow_gx[xy / g.Y];
        const float v1 = f.t(x, y, z);
        float g1[3];
        mc_grad(f, x, y, z, g1);
        const float o[3] = {ox, oy, oz};
        unsigned id = vbase[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((bits >> a) & 1u)) continue;
            mc_vertex<true>(f, x, y, z, a, v1, g1, o, vs, (size_t)id, verts, normals, colors, keys);
            ++id;
        }
    }
}

__global__ void k_mc_triangles(Grid g, int nrows, const signed char* __restrict__ tri,
                               const unsigned char* __restrict__ cubes, const unsigned char* __restrict__ ebits,
                               const unsigned* __restrict__ vbase, const unsigned* __restrict__ tbase,
                               int* __restrict__ faces) {
    const size_t n = (size_t)nrows * g.Y * g.Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned cube = cubes[i];
        if (cube == 0 || cube == 255) continue;
        const int z = (int)(i % g.Z);
        const size_t xy = i / g.Z;
        const int y = (int)(xy % g.Y), row = (int)(xy / g.Y);
        size_t f = tbase[i];
        const signed char* rowt = tri + 16 * cube;
        for (int k = 0; rowt[k] >= 0; k += 3) {
            int vid[3];
            for (int j = 0; j < 3; ++j) {
                int off, axis;
                edge_anchor(rowt[k + j], off, axis);
                // the vertex row after a local row is global x + 1 (local or cap)
                const size_t e = (((size_t)(row + (off & 1)) * g.Y + (y + ((off >> 1) & 1))) * g.Z) +
                                 (z + ((off >> 2) & 1));
                const unsigned bits = ebits[e];
                vid[j] = (int)(vbase[e] + (unsigned)__popc(bits & ((1u << axis) - 1u)));
            }
            for (int j = 0; j < 3; ++j) faces[3 * f + tri_slot(j)] = vid[j];
            ++f;
        }
    }
}

// ---- the voxel hash's mesher: marching cubes over the table's live blocks --------
// A "mesh block" is a block coordinate b inside the volume with a live block among b + {0,1}^3: a
// vertex or a triangle needs a corner below 0, hence an entry, and the voxel that anchors it then
// lies in that entry's block or in one of its seven -neighbours.  One workgroup of 256 meshes one
// mesh block (2 anchor voxels per lane) from an LDS tile of the tsdf of the block's reach, 11^3
// voxels (-1 .. +9 per axis: the cells' and +axis edges' far corners and both ends' gradients).
constexpr int kTile = 11;                       // (odd row pitch: no LDS bank conflicts along y / x)
constexpr int kTileVox = kTile * kTile * kTile;  // 1331 floats, 5.3 KB
constexpr int kHoodBlocks = 27;

struct HashGeo {
    int X, Y, Z;        // dims
    int nbx, nby, nbz;  // blocks per axis
};

__device__ inline unsigned long long block_lin(const HashGeo& g, int bx, int by, int bz) {
    return ((unsigned long long)bx * g.nby + by) * g.nbz + bz;
}

// A slot's live block inside the volume (k_to_dense's reading of the table; a slot value outside
// the pool counts as absent, as in the raycast's find).
__device__ inline bool slot_block(const HashGeo& g, const Table& t, long long s, int* bx, int* by, int* bz, int* blk) {
    const unsigned long long key = coh_load(&t.keys[s]);
    if (key == kEmpty || key == kTomb) return false;
    *blk = coh_load(&t.vals[s]);
    if (*blk < 0 || *blk >= t.max_blocks) return false;
    *bx = (int)(key & 0x1FFFFF), *by = (int)((key >> 21) & 0x1FFFFF), *bz = (int)(key >> 42);
    return *bx < g.nbx && *by < g.nby && *bz < g.nbz;
}

// Exclusive scan of one value per lane over the workgroup of 256 (wsum: 4 words of LDS); *total:
// the workgroup's sum.  (The mesh kernels scan pairs of counts packed in the halves of a word.)
__device__ inline unsigned wg_scan(unsigned v, unsigned* wsum, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + inc - v;
}

// The live blocks' coordinates (block_lin, in no order; at most cap), counted in *counter; with
// keys == nullptr only counted.  A workgroup takes 4096 consecutive slots at a time, 16 per lane,
// and claims its blocks' places with one atomic (one per live slot, 89 k on one word, took 590 us
// at the bench table's 2^22 slots).
constexpr int kSlotsPerLane = 16;
__global__ __launch_bounds__(256) void k_hm_live(HashGeo g, Table t, unsigned long long* __restrict__ counter,
                                                 long long cap, unsigned long long* __restrict__ keys) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned long long first;
    constexpr long long kChunk = 256 * kSlotsPerLane;
    int bx, by, bz, blk;
    for (long long c0 = (long long)blockIdx.x * kChunk; c0 < t.capacity; c0 += (long long)gridDim.x * kChunk) {
        unsigned mask = 0;
#pragma unroll
        for (int j = 0; j < kSlotsPerLane; ++j) {
            const long long s = c0 + j * 256 + threadIdx.x;
            if (s < t.capacity && slot_block(g, t, s, &bx, &by, &bz, &blk)) mask |= 1u << j;
        }
        unsigned total;
        const unsigned before = wg_scan((unsigned)__popc(mask), wsum, &total);
        if (threadIdx.x == 0 && total) first = atomicAdd(counter, (unsigned long long)total);
        __syncthreads();
        if (keys && mask) {
            long long i = (long long)first + before;
            for (int j = 0; j < kSlotsPerLane; ++j) {
                if (!((mask >> j) & 1u)) continue;
                (void)slot_block(g, t, c0 + j * 256 + threadIdx.x, &bx, &by, &bz, &blk);
                if (i < cap) keys[i] = block_lin(g, bx, by, bz);
                ++i;
            }
        }
        __syncthreads();
    }
}

// eight candidates per live block: b - {0,1}^3 inside the volume, else `none` (sorts last)
__global__ void k_hm_candidates(HashGeo g, const unsigned long long* __restrict__ live, long long n_live,
                                unsigned long long none, unsigned long long* __restrict__ cand) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 8 * n_live;
         i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long k = live[i >> 3];
        const int bz = (int)(k % g.nbz), by = (int)((k / g.nbz) % g.nby), bx = (int)(k / g.nbz / g.nby);
        const int cx = bx - (int)(i & 1), cy = by - (int)((i >> 1) & 1), cz = bz - (int)((i >> 2) & 1);
        cand[i] = cx >= 0 && cy >= 0 && cz >= 0 ? block_lin(g, cx, cy, cz) : none;
    }
}

// the unique candidates without the `none` at their end
__global__ void k_hm_drop_none(const unsigned long long* __restrict__ uniq, unsigned long long none,
                               long long* __restrict__ n) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *n > 0 && uniq[*n - 1] == none) --*n;
}

// The hash mesher's volume: the tsdf from the workgroup's tile, the colour from the pool blocks of
// the mesh block's 3^3 neighbourhood.
struct TileVol {
    const float* tile;  // [kTile]^3, tile voxel (0,0,0) = global (x0, y0, z0)
    const int* hood;    // [27] pool block of b + {-1,0,1}^3, -1: absent
    int x0, y0, z0, bx, by, bz;
    int xlo, xhi, Y, Z;
    Table tab;
    unsigned long long* occ;
    float* color;
    __device__ float t(int x, int y, int z) const { return tile[((x - x0) * kTile + (y - y0)) * kTile + (z - z0)]; }
    // (a vertex's colour voxel is one of its edge's ends, inside the neighbourhood; the general
    // find serves positions that are not numbers -- tsdf values that are not finite)
    __device__ float c(int x, int y, int z) const {
        if ((unsigned)x >= (unsigned)xhi || (unsigned)y >= (unsigned)Y || (unsigned)z >= (unsigned)Z) return 0.0f;
        const int dx = (x >> 3) - bx + 1, dy = (y >> 3) - by + 1, dz = (z >> 3) - bz + 1;
        const int blk = (unsigned)dx < 3u && (unsigned)dy < 3u && (unsigned)dz < 3u
                            ? hood[(dx * 3 + dy) * 3 + dz]
                            : hash_find(tab, x >> 3, y >> 3, z >> 3, tab.max_blocks);
        if (blk < 0) return 0.0f;
        const unsigned long long word = coh_load(&occ[(size_t)blk * 8 + (z & 7)]);
        if (!((word >> (((x & 7) << 3) | (y & 7))) & 1ull)) return 0.0f;
        return coh_load(&color[(size_t)blk * kBrickVox + (size_t)((((x & 7) << 3) | (y & 7)) << 3 | (z & 7))]);
    }
};

struct HashMeshArgs {
    HashGeo g;
    Table t;
    Pool pool;
    const unsigned long long* mesh_blocks;  // sorted block_lin of the mesh blocks
};

// Resolve the neighbourhood and stage the tile (all 256 lanes; ends with a barrier).  Voxels without
// an entry are 1; tile voxels outside the volume are never read (the gradients clamp first).
__device__ inline TileVol hm_stage(const HashMeshArgs& a, float* tile, int* hood) {
    const unsigned long long k = a.mesh_blocks[blockIdx.x];
    TileVol v;
    v.bz = (int)(k % a.g.nbz), v.by = (int)((k / a.g.nbz) % a.g.nby), v.bx = (int)(k / a.g.nbz / a.g.nby);
    v.x0 = v.bx * 8 - 1, v.y0 = v.by * 8 - 1, v.z0 = v.bz * 8 - 1;
    v.xlo = 0, v.xhi = a.g.X, v.Y = a.g.Y, v.Z = a.g.Z;
    v.tile = tile, v.hood = hood;
    v.tab = a.t;
    v.occ = a.t.occ, v.color = a.pool.color;
    if (threadIdx.x < kHoodBlocks) {
        const int i = threadIdx.x;
        const int cx = v.bx + i / 9 - 1, cy = v.by + (i / 3) % 3 - 1, cz = v.bz + i % 3 - 1;
        const bool in = cx >= 0 && cy >= 0 && cz >= 0 && cx < a.g.nbx && cy < a.g.nby && cz < a.g.nbz;
        hood[i] = in ? hash_find(a.t, cx, cy, cz, a.t.max_blocks) : -1;
    }
    __syncthreads();
    // six tile voxels per lane, in two rounds of independent loads: the entry words, then the
    // values (voxel by voxel, each value's load waited for its word's: twelve round trips)
    constexpr int kPerLane = (kTileVox + 255) / 256;
    long long at[kPerLane];  // the voxel's index in the pool, -1: no entry
    unsigned long long word[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int i = threadIdx.x + k * 256;
        const int tz = i % kTile, ty = (i / kTile) % kTile, tx = i / (kTile * kTile);
        const int x = v.x0 + tx, y = v.y0 + ty, z = v.z0 + tz;
        at[k] = -1;
        word[k] = 0;
        if (i < kTileVox && (unsigned)x < (unsigned)a.g.X && (unsigned)y < (unsigned)a.g.Y && (unsigned)z < (unsigned)a.g.Z) {
            const int blk = hood[(((x >> 3) - v.bx + 1) * 3 + ((y >> 3) - v.by + 1)) * 3 + ((z >> 3) - v.bz + 1)];
            if (blk >= 0) {
                word[k] = coh_load(&a.t.occ[(size_t)blk * 8 + (z & 7)]) >> (((x & 7) << 3) | (y & 7));
                at[k] = (long long)blk * kBrickVox + ((((x & 7) << 3) | (y & 7)) << 3 | (z & 7));
            }
        }
    }
    float val[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) val[k] = (word[k] & 1ull) ? coh_load(&a.pool.tsdf[at[k]]) : 1.0f;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
        if (threadIdx.x + k * 256 < kTileVox) tile[threadIdx.x + k * 256] = val[k];
    __syncthreads();
    return v;
}

// anchor voxel l (0..511, brick-local order) of the workgroup's mesh block; false: beyond dims
__device__ inline bool hm_anchor(const TileVol& v, int l, int* x, int* y, int* z) {
    *x = v.bx * 8 + (l >> 6), *y = v.by * 8 + ((l >> 3) & 7), *z = v.bz * 8 + (l & 7);
    return *x < v.xhi && *y < v.Y && *z < v.Z;
}

// Per anchor: crossing bits and cell case (what k_mc_classify writes per voxel); per mesh block:
// the vertex and triangle counts.
__global__ __launch_bounds__(256) void k_hm_classify(HashMeshArgs a, const unsigned char* __restrict__ ntri,
                                                     unsigned char* __restrict__ ebits,
                                                     unsigned char* __restrict__ cubes,
                                                     unsigned long long* __restrict__ vcnt,
                                                     unsigned long long* __restrict__ tcnt) {
    __shared__ float tile[kTileVox];
    __shared__ int hood[kHoodBlocks];
    __shared__ unsigned wsum[4];
    const TileVol f = hm_stage(a, tile, hood);
    unsigned packed = 0;  // vertices | triangles << 16 (at most 1536 and 2560 per block)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int l = threadIdx.x * 2 + h;
        int x, y, z;
        unsigned bits = 0, cube = 0;
        if (hm_anchor(f, l, &x, &y, &z)) {
            const bool xn = x + 1 < f.xhi;
            bits = mc_edges(f, x, y, z, xn);
            if (xn && y + 1 < f.Y && z + 1 < f.Z) {
                cube = mc_case(f, x, y, z);
                packed += (unsigned)ntri[cube] << 16;
            }
        }
        ebits[(size_t)blockIdx.x * kBrickVox + l] = (unsigned char)bits;
        cubes[(size_t)blockIdx.x * kBrickVox + l] = (unsigned char)cube;
        packed += (unsigned)__popc(bits);
    }
    unsigned total;
    (void)wg_scan(packed, wsum, &total);
    if (threadIdx.x == 0) {
        vcnt[blockIdx.x] = total & 0xFFFFu;
        tcnt[blockIdx.x] = total >> 16;
    }
}

// Vertices (with their keys, and their own index for the sort) and triangles (a sort key: anchor
// cell in C-order, then the table's order; the three vertex keys in face order), block by block.
template <bool NRM, bool TRI>
__global__ __launch_bounds__(256) void k_hm_emit(HashMeshArgs a, const signed char* __restrict__ tri,
                                                 const unsigned char* __restrict__ ebits,
                                                 const unsigned char* __restrict__ cubes,
                                                 const unsigned long long* __restrict__ vbase,
                                                 const unsigned long long* __restrict__ tbase, float ox, float oy,
                                                 float oz, float vs, float* __restrict__ verts,
                                                 float* __restrict__ normals, unsigned char* __restrict__ colors,
                                                 long long* __restrict__ keys, unsigned* __restrict__ vidx,
                                                 unsigned long long* __restrict__ tkey, unsigned* __restrict__ tidx,
                                                 long long* __restrict__ fkeys) {
    __shared__ float tile[kTileVox];
    __shared__ int hood[kHoodBlocks];
    __shared__ unsigned wsum[4];
    if (vbase[blockIdx.x + 1] == vbase[blockIdx.x] && (!TRI || tbase[blockIdx.x + 1] == tbase[blockIdx.x])) return;
    const TileVol f = hm_stage(a, tile, hood);
    unsigned bits[2], cube[2], packed = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        bits[h] = ebits[(size_t)blockIdx.x * kBrickVox + threadIdx.x * 2 + h];
        cube[h] = cubes[(size_t)blockIdx.x * kBrickVox + threadIdx.x * 2 + h];
        packed += (unsigned)__popc(bits[h]);
        if (TRI) {
            int n = 0;
            for (const signed char* r = tri + 16 * cube[h]; r[n] >= 0; n += 3) {}
            packed += (unsigned)(n / 3) << 16;
        }
    }
    unsigned total;
    const unsigned before = wg_scan(packed, wsum, &total);
    size_t id = (size_t)vbase[blockIdx.x] + (before & 0xFFFFu);
    size_t ft = TRI ? (size_t)tbase[blockIdx.x] + (before >> 16) : 0;
    const float o[3] = {ox, oy, oz};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!bits[h] && (!TRI || cube[h] == 0 || cube[h] == 255)) continue;
        int x, y, z;
        (void)hm_anchor(f, threadIdx.x * 2 + h, &x, &y, &z);
        if (bits[h]) {
            const float v1 = f.t(x, y, z);
            float g1[3] = {0.0f, 0.0f, 0.0f};
            if (NRM) mc_grad(f, x, y, z, g1);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!((bits[h] >> ax) & 1u)) continue;
                mc_vertex<NRM>(f, x, y, z, ax, v1, g1, o, vs, id, verts, normals, colors, keys);
                vidx[id] = (unsigned)id;
                ++id;
            }
        }
        if (TRI && cube[h] != 0 && cube[h] != 255) {
            const signed char* rowt = tri + 16 * cube[h];
            const unsigned long long cell = (((unsigned long long)x * f.Y) + y) * f.Z + z;
            for (int k = 0; rowt[k] >= 0; k += 3) {
                for (int j = 0; j < 3; ++j) fkeys[3 * ft + tri_slot(j)] = mc_edge_key(rowt[k + j], x, y, z, f.Y, f.Z);
                tkey[ft] = cell * 8 + (unsigned)(k / 3);
                tidx[ft] = (unsigned)ft;
                ++ft;
            }
        }
    }
}

// vertex attributes into key order
__global__ void k_hm_permute(const unsigned* __restrict__ perm, long long n, const float* __restrict__ vin,
                             const float* __restrict__ nin, const unsigned char* __restrict__ cin,
                             float* __restrict__ verts, float* __restrict__ normals,
                             unsigned char* __restrict__ colors) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const size_t s = perm[i];
        for (int k = 0; k < 3; ++k) {
            verts[3 * i + k] = vin[3 * s + k];
            if (nin) normals[3 * i + k] = nin[3 * s + k];
            colors[3 * i + k] = cin[3 * s + k];
        }
    }
}

// faces in cell order: each vertex key's rank among the sorted keys
__global__ void k_hm_faces(const unsigned* __restrict__ perm, long long n_tris, const long long* __restrict__ fkeys,
                           const long long* __restrict__ keys, long long n_verts, int* __restrict__ faces) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n_tris;
         i += (long long)gridDim.x * blockDim.x) {
        const long long key = fkeys[3 * (size_t)perm[i / 3] + i % 3];
        long long lo = 0, hi = n_verts;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        faces[i] = (int)lo;
    }
}

int bits_for(unsigned long long n) {  // radix-sort bits that hold every value < n
    int b = 1;
    while (b < 64 && (n - 1) >> b) ++b;
    return b;
}

// the case table's triangle counts (256 bytes) and edge lists (4 KB) into the call's scratch
int upload_table(unsigned char* ntri, signed char* tri, hipStream_t s) {
    const McTable& tab = table();
    TSDF_HIP(hipMemcpyAsync(ntri, tab.ntri, sizeof(tab.ntri), hipMemcpyHostToDevice, s));
    TSDF_HIP(hipMemcpyAsync(tri, tab.tri, sizeof(tab.tri), hipMemcpyHostToDevice, s));
    return TSDF_OK;
}

}  // namespace

namespace tsdf {

int Mesh::alloc(long long nv, long long nt, int fields) {
    release();
    DevBufs fresh;  // freed again if an allocation fails
    Mesh f;
    const size_t v = (size_t)nv, t = (size_t)nt;
    TSDF_TRY(fresh.alloc(&f.verts, 3 * v));
    TSDF_TRY(fresh.alloc(&f.colors, 3 * v));
    TSDF_TRY(fresh.alloc(&f.keys, v));
    if (fields & TSDF_MESH_NORMALS) TSDF_TRY(fresh.alloc(&f.normals, 3 * v));
    if (fields & TSDF_MESH_FACES) TSDF_TRY(fresh.alloc(&f.faces, 3 * t));
    fresh.keep();
    f.n_verts = nv;
    f.n_tris = nt;
    *this = f;
    return TSDF_OK;
}

void Mesh::release() {
    for (void* p : {(void*)verts, (void*)normals, (void*)colors, (void*)faces, (void*)keys})
        if (p) (void)hipFree(p);
    verts = normals = nullptr;
    colors = nullptr;
    faces = nullptr;
    keys = nullptr;
    n_verts = n_tris = 0;
}

int mesh_domain(const Vol& v, long long global_x, const int64_t* halo_gx, long long n_halo, MeshDomain* d) {
    const int nl = v.dims[0];
    auto gx_of = [&](int lr) { return v.off[0] + col_gx(v, lr >> 3) + (lr & 7); };
    if (global_x > 0) {
        d->xlo = 0;
        d->xhi = (int)global_x;
    } else {  // the shard alone: its own rows must be contiguous
        if (v.xstride != kBrickEdge && v.nb[0] > 1)
            return set_error(TSDF_E_ARG, "a cyclic column shard is meshed with its neighbours' border rows "
                                         "(tsdf_dense_extract_mesh_halo)");
        d->xlo = gx_of(0);
        d->xhi = gx_of(nl - 1) + 1;
    }
    const int span = d->xhi - d->xlo;
    if (span <= 0 || global_x > (1 << 24)) return set_error(TSDF_E_ARG, "bad global x extent %lld", global_x);
    d->row_map.assign(span, -1);
    for (int lr = 0; lr < nl; ++lr) {
        const int gx = gx_of(lr);
        if (gx < d->xlo || gx >= d->xhi) return set_error(TSDF_E_ARG, "local row %d (x %d) outside [%d, %d)", lr, gx, d->xlo, d->xhi);
        d->row_map[gx - d->xlo] = lr;
    }
    for (long long h = 0; h < n_halo; ++h) {
        const long long gx = halo_gx[h];
        if (gx < d->xlo || gx >= d->xhi) return set_error(TSDF_E_ARG, "halo row %lld outside [%d, %d)", gx, d->xlo, d->xhi);
        if (d->row_map[gx - d->xlo] >= 0) return set_error(TSDF_E_ARG, "halo row %lld is a local row", gx);
        if (d->row_map[gx - d->xlo] <= -2) return set_error(TSDF_E_ARG, "halo row %lld given twice", gx);
        d->row_map[gx - d->xlo] = (int)(-2 - h);
    }
    auto present = [&](long long gx) { return gx < d->xlo || gx >= d->xhi || d->row_map[gx - d->xlo] != -1; };
    d->vrow_gx.clear();
    d->vrow_cap.clear();
    for (int gx = d->xlo; gx < d->xhi; ++gx) {
        const int r = d->row_map[gx - d->xlo];
        const bool local = r >= 0, prev_local = gx > d->xlo && d->row_map[gx - 1 - d->xlo] >= 0;
        if (!local && !prev_local) continue;
        // every row the cells and gradients read: x - 1, x + 1 (and x + 1 of a cap row)
        if (!present(gx) || !present(gx - 1) || !present(gx + 1))
            return set_error(TSDF_E_ARG, "mesh of x row %d needs rows %d..%d: pass the missing border rows "
                                         "(tsdf_dense_mesh_halo_rows)", gx, gx - 1, gx + 1);
        d->vrow_gx.push_back(gx);
        d->vrow_cap.push_back(local ? 0 : 1);
    }
    return TSDF_OK;
}

int mesh_halo_rows(const Vol& v, long long global_x, std::vector<long long>* out) {
    out->clear();
    if (global_x <= 0 || global_x > (1 << 24)) return set_error(TSDF_E_ARG, "bad global x extent %lld", global_x);
    std::vector<char> local((size_t)global_x, 0);
    for (int lr = 0; lr < v.dims[0]; ++lr) {
        const long long gx = v.off[0] + (long long)col_gx(v, lr >> 3) + (lr & 7);
        if (gx >= global_x) return set_error(TSDF_E_ARG, "local row at x %lld beyond the global extent", gx);
        local[gx] = 1;
    }
    std::vector<char> need((size_t)global_x, 0);
    for (long long gx = 0; gx < global_x; ++gx) {
        if (!local[gx]) continue;
        if (gx - 1 >= 0) need[gx - 1] = 1;
        if (gx + 1 < global_x) need[gx + 1] = 1;
        if (gx + 2 < global_x && !local[gx + 1]) need[gx + 2] = 1;  // gradient of the cap row
    }
    for (long long gx = 0; gx < global_x; ++gx)
        if (need[gx] && !local[gx]) out->push_back(gx);
    return TSDF_OK;
}

// Extract into m (device buffers): the cells anchored at the shard's local rows over the range
// and halo rows of `d` (halo rows: device C-order slices, nullptr when there are none).
int extract_mesh(Base& B, const Pool& pool, Mesh& m, const MeshDomain& d, const float* ht, const float* hc) {
    m.release();
    const int nrows = (int)d.vrow_gx.size();
    Grid g;
    g.Y = B.vol.dims[1];
    g.Z = B.vol.dims[2];
    g.xlo = d.xlo;
    g.xhi = d.xhi;
    g.nby = B.vol.nb[1];
    g.nbz = B.vol.nb[2];
    g.t = pool.tsdf;
    g.c = pool.color;
    g.ht = ht;
    g.hc = hc;
    const size_t n = (size_t)nrows * g.Y * g.Z;
    if (n >= (1ull << 31)) return set_error(TSDF_E_ARG, "volume too large for one mesh extraction (>= 2^31 voxels)");
    if (n == 0) return TSDF_OK;  // (no vertex rows: the empty mesh)
    hipStream_t s = B.stream;
    MeshGuard guard(m);
    unsigned totals[2] = {0, 0};  // (read back: declared before the owner of what it is read from)
    DevBufs sc;
    // One allocation: per voxel the crossing bits, the case and both counts with their offsets
    // (entry n of each scan is the total: n + 1 counts, the last one 0), then the tables, the
    // domain's rows and the scan's temporary storage.  (n + 1 < 2^31: every dimension is at most
    // 2^24, and 2^31 - 1 is prime.)
    unsigned char *ebits = nullptr, *cubes = nullptr, *ntri = nullptr, *vcap = nullptr;
    signed char* dtri = nullptr;
    unsigned *vcnt = nullptr, *tcnt = nullptr, *vbase = nullptr, *tbase = nullptr;
    int *rmap = nullptr, *vgx = nullptr;
    char* tmp = nullptr;
    size_t need = 0;
    TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, vcnt, vbase, (int)(n + 1), s));
    Layout l;
    l.add(&ebits, n);
    l.add(&cubes, n);
    l.add(&vcnt, n + 1);
    l.add(&tcnt, n + 1);
    l.add(&vbase, n + 1);
    l.add(&tbase, n + 1);
    l.add(&ntri, 256);
    l.add(&dtri, 256 * 16);
    l.add(&rmap, d.row_map.size());
    l.add(&vgx, (size_t)nrows);
    l.add(&vcap, (size_t)nrows);
    l.add(&tmp, need);
    TSDF_TRY(sc.alloc(l));
    TSDF_TRY(upload_table(ntri, dtri, s));
    TSDF_HIP(hipMemcpyAsync(rmap, d.row_map.data(), sizeof(int) * d.row_map.size(), hipMemcpyHostToDevice, s));
    TSDF_HIP(hipMemcpyAsync(vgx, d.vrow_gx.data(), sizeof(int) * nrows, hipMemcpyHostToDevice, s));
    TSDF_HIP(hipMemcpyAsync(vcap, d.vrow_cap.data(), nrows, hipMemcpyHostToDevice, s));
    TSDF_HIP(hipMemsetAsync(vcnt + n, 0, sizeof(unsigned), s));
    TSDF_HIP(hipMemsetAsync(tcnt + n, 0, sizeof(unsigned), s));
    g.row_map = rmap;
    g.vrow_gx = vgx;
    g.vrow_cap = vcap;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)B.n_cu * 32);
    hipLaunchKernelGGL(k_mc_classify, dim3(grid), dim3(256), 0, s, g, nrows, (const unsigned char*)ntri, ebits, cubes,
                       vcnt, tcnt);
    TSDF_HIP(hipGetLastError());
    TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, need, vcnt, vbase, (int)(n + 1), s));
    TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, need, tcnt, tbase, (int)(n + 1), s));
    TSDF_HIP(hipMemcpyAsync(&totals[0], vbase + n, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    TSDF_HIP(hipMemcpyAsync(&totals[1], tbase + n, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    TSDF_HIP(hipStreamSynchronize(s));
    TSDF_TRY(m.alloc(totals[0], totals[1], TSDF_MESH_NORMALS | TSDF_MESH_FACES));
    hipLaunchKernelGGL(k_mc_vertices, dim3(grid), dim3(256), 0, s, g, nrows, (const unsigned char*)ebits,
                       (const unsigned*)vbase, B.vol.origin[0], B.vol.origin[1], B.vol.origin[2], (float)B.vol.vs,
                       m.verts, m.normals, m.colors, m.keys);
    hipLaunchKernelGGL(k_mc_triangles, dim3(grid), dim3(256), 0, s, g, nrows, (const signed char*)dtri,
                       (const unsigned char*)cubes, (const unsigned char*)ebits, (const unsigned*)vbase,
                       (const unsigned*)tbase, m.faces);
    TSDF_HIP(hipGetLastError());
    TSDF_HIP(hipStreamSynchronize(s));
    guard.done = true;
    return TSDF_OK;
}

namespace {

unsigned flat_grid(const Base& B, long long n) {
    return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)B.n_cu * 32));
}

}  // namespace

// Marching cubes of the table's state (the volume tsdf_hash_get_dense gives) over its live blocks:
// the dense mesher's mesh of that volume, byte for byte and in its order.  Nothing here is sized
// by the volume's extent: the passes walk the table's slots, the live blocks, the mesh blocks and
// the mesh.  fields: TSDF_MESH_NORMALS | TSDF_MESH_FACES, what to extract beside vertices, colours
// and keys (the triangle count is given either way).
// One allocation per stage (an allocation costs the host more than any of the stages' kernels): a
// stage records its arrays in a Layout and the call's DevBufs allocates them together; all of
// them are freed at the end of the call.  scratch_bytes of tsdf_hash_mesh_info: everything
// allocated, the mesh included.
int hash_extract_mesh(Base& B, const Table& t, Mesh& m, int fields, tsdf_hash_mesh_info_t* info) {
    m.release();
    *info = tsdf_hash_mesh_info_t{};
    const bool want_n = (fields & TSDF_MESH_NORMALS) != 0, want_f = (fields & TSDF_MESH_FACES) != 0;
    hipStream_t s = B.stream;
    HashMeshArgs a;
    a.g.X = B.vol.dims[0], a.g.Y = B.vol.dims[1], a.g.Z = B.vol.dims[2];
    a.g.nbx = B.vol.nb[0], a.g.nby = B.vol.nb[1], a.g.nbz = B.vol.nb[2];
    a.t = t;
    a.pool = B.pool;
    const unsigned long long n_blocks = (unsigned long long)a.g.nbx * a.g.nby * a.g.nbz;  // also the `none` candidate
    const unsigned long long n_vox = (unsigned long long)a.g.X * a.g.Y * a.g.Z;
    MeshGuard guard(m);
    // (read back: declared before the owner of what they are read from)
    unsigned long long n_live_u = 0, totals[2] = {0, 0};
    long long n_mesh = 0;
    DevBufs sc;
    // 1. the live blocks' coordinates
    unsigned long long* counters = nullptr;  // [0] live blocks, [1] the list's cursor, [2] mesh blocks
    unsigned char* ntri = nullptr;
    signed char* dtri = nullptr;
    Layout l1;
    l1.add(&counters, 4);
    l1.add(&ntri, 256);
    l1.add(&dtri, 256 * 16);
    TSDF_TRY(sc.alloc(l1));
    TSDF_HIP(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 4, s));
    TSDF_TRY(upload_table(ntri, dtri, s));
    const unsigned slot_grid =
        (unsigned)std::max<long long>(1, std::min<long long>((t.capacity + 256 * kSlotsPerLane - 1) / (256 * kSlotsPerLane), 1024));
    hipLaunchKernelGGL(k_hm_live, dim3(slot_grid), dim3(256), 0, s, a.g, t, counters, 0ll, (unsigned long long*)nullptr);
    TSDF_HIP(hipGetLastError());
    TSDF_HIP(hipMemcpyAsync(&n_live_u, counters, sizeof(n_live_u), hipMemcpyDeviceToHost, s));
    TSDF_HIP(hipStreamSynchronize(s));
    const long long n_live = (long long)n_live_u;
    info->live_blocks = n_live;
    if (n_live >= (1ll << 28)) return set_error(TSDF_E_ARG, "too many live blocks for one mesh extraction (%lld)", n_live);
    // 2. the mesh blocks: the live blocks' -neighbourhoods, sorted, each once
    unsigned long long* mesh_blocks = nullptr;
    if (n_live > 0) {
        const int nc = (int)(8 * n_live), bb = bits_for(n_blocks + 1);
        unsigned long long *live = nullptr, *cand = nullptr, *cand_s = nullptr;
        long long* d_n_mesh = (long long*)(counters + 2);
        size_t need_sort = 0, need_uniq = 0;
        TSDF_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need_sort, cand, cand_s, nc, 0, bb, s));
        TSDF_HIP(hipcub::DeviceSelect::Unique(nullptr, need_uniq, cand_s, mesh_blocks, d_n_mesh, nc, s));
        char* tmp = nullptr;
        Layout l;
        l.add(&live, (size_t)n_live);
        l.add(&cand, (size_t)nc);
        l.add(&cand_s, (size_t)nc);
        l.add(&mesh_blocks, (size_t)nc);
        l.add(&tmp, std::max(need_sort, need_uniq));
        TSDF_TRY(sc.alloc(l));
        hipLaunchKernelGGL(k_hm_live, dim3(slot_grid), dim3(256), 0, s, a.g, t, counters + 1, n_live, live);
        TSDF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_hm_candidates, dim3(flat_grid(B, nc)), dim3(256), 0, s, a.g,
                           (const unsigned long long*)live, n_live, n_blocks, cand);
        TSDF_HIP(hipGetLastError());
        TSDF_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, need_sort, cand, cand_s, nc, 0, bb, s));
        TSDF_HIP(hipcub::DeviceSelect::Unique(tmp, need_uniq, cand_s, mesh_blocks, d_n_mesh, nc, s));
        hipLaunchKernelGGL(k_hm_drop_none, dim3(1), dim3(64), 0, s, (const unsigned long long*)mesh_blocks, n_blocks,
                           d_n_mesh);
        TSDF_HIP(hipGetLastError());
        TSDF_HIP(hipMemcpyAsync(&n_mesh, d_n_mesh, sizeof(n_mesh), hipMemcpyDeviceToHost, s));
        TSDF_HIP(hipStreamSynchronize(s));
    }
    info->mesh_blocks = n_mesh;
    a.mesh_blocks = mesh_blocks;
    // 3. classify, and the blocks' offsets (entry n_mesh of each scan: the total)
    unsigned char *ebits = nullptr, *cubes = nullptr;
    unsigned long long *vcnt = nullptr, *tcnt = nullptr, *vbase = nullptr, *tbase = nullptr;
    if (n_mesh > 0) {
        size_t need = 0;
        TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, vcnt, vbase, (int)(n_mesh + 1), s));
        char* tmp = nullptr;
        Layout l;
        l.add(&ebits, (size_t)n_mesh * kBrickVox);
        l.add(&cubes, (size_t)n_mesh * kBrickVox);
        l.add(&vcnt, (size_t)n_mesh + 1);
        l.add(&tcnt, (size_t)n_mesh + 1);
        l.add(&vbase, (size_t)n_mesh + 1);
        l.add(&tbase, (size_t)n_mesh + 1);
        l.add(&tmp, need);
        TSDF_TRY(sc.alloc(l));
        TSDF_HIP(hipMemsetAsync(vcnt + n_mesh, 0, sizeof(unsigned long long), s));
        TSDF_HIP(hipMemsetAsync(tcnt + n_mesh, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_hm_classify, dim3((unsigned)n_mesh), dim3(256), 0, s, a, (const unsigned char*)ntri, ebits,
                           cubes, vcnt, tcnt);
        TSDF_HIP(hipGetLastError());
        TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, need, vcnt, vbase, (int)(n_mesh + 1), s));
        TSDF_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, need, tcnt, tbase, (int)(n_mesh + 1), s));
        TSDF_HIP(hipMemcpyAsync(&totals[0], vbase + n_mesh, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        TSDF_HIP(hipMemcpyAsync(&totals[1], tbase + n_mesh, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        TSDF_HIP(hipStreamSynchronize(s));
    }
    if (totals[0] >= (1ull << 31) || totals[1] >= (1ull << 31))
        return set_error(TSDF_E_ARG, "mesh too large for int32 faces (%llu vertices, %llu triangles)", totals[0], totals[1]);
    const long long nv = (long long)totals[0], nt = (long long)totals[1];
    // 4. emit block by block, 5. into the global order.  The outputs belong to the mesh.
    TSDF_TRY(m.alloc(nv, nt, fields));
    const size_t out_bytes = (size_t)nv * (12 + 3 + 8 + (want_n ? 12 : 0)) + (want_f ? (size_t)nt * 12 : 0);
    if (nv > 0) {
        const bool tris = want_f && nt > 0;
        const int kb = bits_for(n_vox * 3), cb = bits_for(n_vox * 8);
        float *vu = nullptr, *nu = nullptr;
        unsigned char* cu = nullptr;
        long long *ku = nullptr, *fkeys = nullptr;
        unsigned *vi = nullptr, *vperm = nullptr, *ti = nullptr, *tperm = nullptr;
        unsigned long long *tk = nullptr, *tk_s = nullptr;
        size_t need_v = 0, need_t = 0;
        TSDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need_v, ku, m.keys, vi, vperm, (int)nv, 0, kb, s));
        if (tris) TSDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need_t, tk, tk_s, ti, tperm, (int)nt, 0, cb, s));
        char* tmp = nullptr;
        Layout l;
        l.add(&vu, 3 * (size_t)nv);
        l.add(&cu, 3 * (size_t)nv);
        l.add(&ku, (size_t)nv);
        l.add(&vi, (size_t)nv);
        l.add(&vperm, (size_t)nv);
        if (want_n) l.add(&nu, 3 * (size_t)nv);
        if (tris) {
            l.add(&fkeys, 3 * (size_t)nt);
            l.add(&tk, (size_t)nt);
            l.add(&tk_s, (size_t)nt);
            l.add(&ti, (size_t)nt);
            l.add(&tperm, (size_t)nt);
        }
        l.add(&tmp, std::max(need_v, need_t));
        TSDF_TRY(sc.alloc(l));
        auto emit = want_n ? (tris ? k_hm_emit<true, true> : k_hm_emit<true, false>)
                           : (tris ? k_hm_emit<false, true> : k_hm_emit<false, false>);
        hipLaunchKernelGGL(emit, dim3((unsigned)n_mesh), dim3(256), 0, s, a, (const signed char*)dtri,
                           (const unsigned char*)ebits, (const unsigned char*)cubes, (const unsigned long long*)vbase,
                           (const unsigned long long*)tbase, B.vol.origin[0], B.vol.origin[1], B.vol.origin[2],
                           (float)B.vol.vs, vu, nu, cu, ku, vi, tk, ti, fkeys);
        TSDF_HIP(hipGetLastError());
        TSDF_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, need_v, ku, m.keys, vi, vperm, (int)nv, 0, kb, s));
        hipLaunchKernelGGL(k_hm_permute, dim3(flat_grid(B, nv)), dim3(256), 0, s, (const unsigned*)vperm, nv,
                           (const float*)vu, (const float*)nu, (const unsigned char*)cu, m.verts, m.normals, m.colors);
        TSDF_HIP(hipGetLastError());
        if (tris) {
            TSDF_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, need_t, tk, tk_s, ti, tperm, (int)nt, 0, cb, s));
            hipLaunchKernelGGL(k_hm_faces, dim3(flat_grid(B, 3 * nt)), dim3(256), 0, s, (const unsigned*)tperm, nt,
                               (const long long*)fkeys, (const long long*)m.keys, nv, m.faces);
            TSDF_HIP(hipGetLastError());
        }
        TSDF_HIP(hipStreamSynchronize(s));
    }
    guard.done = true;
    info->scratch_bytes = (int64_t)(sc.bytes + out_bytes);
    info->n_verts = nv;
    info->n_tris = nt;
    return TSDF_OK;
}

int copy_mesh(Base& B, const Mesh& m, float* verts, float* normals, uint8_t* colors, int32_t* faces,
              int64_t* keys) {
    hipStream_t s = B.stream;
    if (keys) TSDF_HIP(hipMemcpyAsync(keys, m.keys, sizeof(long long) * m.n_verts, hipMemcpyDeviceToHost, s));
    if (verts) TSDF_HIP(hipMemcpyAsync(verts, m.verts, sizeof(float) * 3 * m.n_verts, hipMemcpyDeviceToHost, s));
    if (normals) TSDF_HIP(hipMemcpyAsync(normals, m.normals, sizeof(float) * 3 * m.n_verts, hipMemcpyDeviceToHost, s));
    if (colors) TSDF_HIP(hipMemcpyAsync(colors, m.colors, 3 * m.n_verts, hipMemcpyDeviceToHost, s));
    if (faces) TSDF_HIP(hipMemcpyAsync(faces, m.faces, sizeof(int) * 3 * m.n_tris, hipMemcpyDeviceToHost, s));
    TSDF_HIP(hipStreamSynchronize(s));
    return TSDF_OK;
}

}  // namespace tsdf

extern "C" int tsdf_mc_table(int8_t* out, uint8_t* ntri) {
    if (!out) return set_error(TSDF_E_ARG, "null pointer");
    const McTable& t = table();
    std::memcpy(out, t.tri, sizeof(t.tri));
    if (ntri) std::memcpy(ntri, t.ntri, sizeof(t.ntri));
    return TSDF_OK;
}
