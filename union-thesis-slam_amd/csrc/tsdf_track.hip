// tsdf_track.hip -- camera tracking against the fused model: frame-to-model
// point-to-plane ICP, single resolution, with an optional photometric term.  Not in the reference
// (its poses come from files).  A depth frame is aligned against the depth and normal maps of a
// raycast (§7d): per sampled pixel a projective association and one row of the linearised
// point-to-plane system, a deterministic reduction to the 6x6 normal equations, and the Cholesky
// solve and pose update on the device, so that an N-iteration alignment costs one host
// synchronisation.
//
// The contract (restated in NumPy by tests/icp_ref.py; codes and residuals matched bit for bit):
// everything per pixel is a separately rounded f32 operation in the model camera's frame, the sums
// are f64 sums of exact products of two f32 values.  See §7e for the steps; the codes are
//   0 not sampled / last row or column / no depth     1 no neighbour depth or degenerate normal
//   2 behind the model camera or outside its image     3 no model surface there
//   4 too far (dist_max)    5 normals disagree (cos_min)    6 inlier
//
// Two kernels per iteration, each a template over COLOR: false is the geometric track, true adds
// the photometric term of §7f (see the banner above k_icp_linearize).  k_icp_linearize: one lane per
// sampled pixel over a grid-stride loop, 28 f64 sums and 2 counts per lane and term, a butterfly
// over the wave, the waves of a workgroup through LDS in wave order, one partial record per
// workgroup.  k_icp_finish (one workgroup of 1024): the partial records in a fixed order, then one
// lane solves and updates.  No floating-point atomics anywhere: the order of every addition is fixed
// by the launch shape, which depends on the image size, the stride and the device only.  The finish
// is a kernel of its own, not the last workgroup of the linearise: a kernel boundary makes the
// partial records visible across the XCDs' L2s by itself, where a last-arriver protocol needs an
// agent-scope release per workgroup, a ticket atomic and an acquire, for the price of one more
// launch of a few microseconds (§7e).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "tsdf_cell.h"
#include "tsdf_host.h"

using namespace tsdf;

namespace tsdf {

constexpr int kIcpWG = 256;
constexpr int kIcpRec = 32;       // doubles per term of a partial record: 28 sums, inliers, candidates, 2 unused
constexpr int kIcpMaxIter = TSDF_ICP_MAX_ITER;
constexpr int kIcpRunning = 0;    // internal status while iterating (the public ones: TSDF_TRACK_*)

// The iteration state, in device memory.
struct IcpState {
    double M[16];  // frame camera -> model camera
    int status;
    int iters;     // linearisations run
};

// One iteration's record (device array indexed by iteration; copied back once).
struct IcpRecord {
    double M[16];        // after the iteration (unchanged by a lost one)
    double sums[28];     // 21 upper-triangle entries of sum J_i J_j (row-major), 6 of sum J_i r, sum r r
    long long inliers, candidates;
    double w_norm, t_norm;
    int status;          // after the iteration
    int pad;
    // the colour term's (§7f): written by the RGB-D finish and read after an RGB-D call only
    double csums[28];    // the same layout (not scaled by lambda^2)
    long long c_inliers, c_candidates;
};

// Device buffers of a handle's tracks, or of a device's handle-less linearisations: grown on
// demand, never allocated per call once they fit.
struct IcpCtx {
    int device = 0;
    hipStream_t stream = nullptr;  // the handle's, or the context's own
    bool own_stream = false;
    void* buf[14] = {};            // see the enum
    size_t bytes[14] = {};
    std::mutex mu;
    void release();
};
enum { kBufDepth, kBufModelD, kBufModelN, kBufCode, kBufResid, kBufTables, kBufPartial, kBufState,
       // the photometric term (§7f): frame RGB8, model colour map, frame intensity, photo texels, colour code / residual
       kBufRgb, kBufModelC, kBufFrameI, kBufTexel, kBufCodeC, kBufResidC, kNumBuf };
static_assert(kNumBuf == 14, "IcpCtx::buf holds one pointer per enumerator");

void IcpCtx::release() {
    for (int i = 0; i < kNumBuf; ++i) {
        if (buf[i]) (void)hipFree(buf[i]);
        buf[i] = nullptr;
        bytes[i] = 0;
    }
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

void icp_ctx_free(IcpCtx* c) {
    if (!c) return;
    c->release();
    delete c;
}

}  // namespace tsdf

namespace {

struct IcpArgs {
    const void* depth;  // Hf x Wf, u16 mm or f64 m
    int dk, inval;
    int Hf, Wf, Hm, Wm;
    int stride, su, sv;  // sampled pixels per row / rows
    const float* dm;     // Hm x Wm
    const float* nm;     // Hm x Wm x 3, world axes
    const float *xf, *yf, *xm, *ym;  // pixel direction tables of the two cameras
    float Rm[9];         // rotation of model_pose (row-major)
    float fxm, fym, cxm, cym;
    float dist_max, cos_min;
    const IcpState* st;
    double* partial;     // gridDim.x records of kIcpRec doubles (twice that with the colour term)
    unsigned char* code;
    float* resid;
    // the colour term (§7f); null / 0 for the geometric instance, which fi == nullptr selects
    const unsigned char* fi;  // Hf x Wf: the frame's intensity
    const float4* tex;        // Hm x Wm: (I, Gx, Gy, D) of the model, all 0 where invalid
    float color_max;
    unsigned char* ccode;
    float* cresid;
};

// x_u = f32((u - cx) / fx), y_v = f32((v - cy) / fy): f64, one rounding (§7d step 1)
__global__ void k_icp_tables(int Wf, int Hf, int Wm, int Hm, double fxf, double fyf, double cxf, double cyf, double fxm,
                             double fym, double cxm, double cym, float* t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Wf) t[i] = (float)(((double)i - cxf) / fxf);
    else if (i < Wf + Hf) t[i] = (float)(((double)(i - Wf) - cyf) / fyf);
    else if (i < Wf + Hf + Wm) t[i] = (float)(((double)(i - Wf - Hf) - cxm) / fxm);
    else if (i < Wf + Hf + Wm + Hm) t[i] = (float)(((double)(i - Wf - Hf - Wm) - cym) / fym);
}

__global__ void k_icp_init(IcpState* st, const double* M) {
    if (threadIdx.x < 16) st->M[threadIdx.x] = M ? M[threadIdx.x] : (threadIdx.x % 5 == 0 ? 1.0 : 0.0);
    if (threadIdx.x == 0) {
        st->status = kIcpRunning;
        st->iters = 0;
    }
}

template <int DK>
__device__ inline float depth_at(const IcpArgs& a, int u, int v) {
    const size_t p = (size_t)v * a.Wf + u;
    if (DK == TSDF_DEPTH_U16_MM) {
        const unsigned mm = ((const unsigned short*)a.depth)[p];
        if (a.inval && mm == 65535u) return 0.0f;
        return (float)((double)mm / 1000.0);
    }
    return (float)((const double*)a.depth)[p];
}

__device__ inline bool good_depth(float d) { return d > 0.0f && d < INFINITY; }

__device__ inline float intensity_u8(const unsigned char* c) {
    return (float)((77u * c[0] + 150u * c[1] + 29u * c[2]) >> 8);
}

// Once per RGB-D call: the frame's intensity image and the model's photo texels.
__global__ void k_icp_photo_prep(const unsigned char* rgb, int n_frame, unsigned char* fi, const unsigned char* mc,
                                 const float* dm, int Hm, int Wm, float4* tex) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_frame) fi[i] = (unsigned char)((77u * rgb[3 * (size_t)i] + 150u * rgb[3 * (size_t)i + 1] + 29u * rgb[3 * (size_t)i + 2]) >> 8);
    if (i >= Hm * Wm) return;
    const int u = i % Wm, v = i / Wm;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (u >= 1 && u <= Wm - 2 && v >= 1 && v <= Hm - 2) {
        const float d = dm[i];
        if (d > 0.0f && dm[i - 1] > 0.0f && dm[i + 1] > 0.0f && dm[i - Wm] > 0.0f && dm[i + Wm] > 0.0f) {
            const unsigned char* c = mc + 3 * (size_t)i;
            t.x = intensity_u8(c);
            t.y = (intensity_u8(c + 3) - intensity_u8(c - 3)) * 0.5f;
            t.z = (intensity_u8(c + 3 * (size_t)Wm) - intensity_u8(c - 3 * (size_t)Wm)) * 0.5f;
            t.w = d;
        }
    }
    tex[i] = t;
}

__device__ inline float lerpf(float a, float b, float t) { return a + t * (b - a); }
__device__ inline float bilerp(float t00, float t01, float t10, float t11, float tx, float ty) {
    return lerpf(lerpf(t00, t01, tx), lerpf(t10, t11, tx), ty);
}

// ---- what the linearise kernels share (k_icp_linearize, k_sdf_linearize) ---------------------------
// One inlier row into a lane's sums s[BASE .. BASE + 27]: the 21 upper-triangle products of J, the 6
// of J r, and r r, each an exact f64 product of two f32 values.
template <int BASE, int N>
__device__ inline void icp_add_row(double (&s)[N], const float (&J)[6], float r) {
    int k = BASE;
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = x; y < 6; ++y) s[k++] += (double)J[x] * (double)J[y];
#pragma unroll
    for (int x = 0; x < 6; ++x) s[BASE + 21 + x] += (double)J[x] * (double)r;
    s[BASE + 27] += (double)r * (double)r;
}

// The lanes' sums and counts to one partial record per workgroup (kIcpRec doubles per term; COLOR:
// two terms), in an order the launch shape alone fixes.
template <bool COLOR>
__device__ inline void icp_reduce(double (&s)[COLOR ? 56 : 28], unsigned n_in, unsigned n_cand, [[maybe_unused]] unsigned c_in,
                                  [[maybe_unused]] unsigned c_cand, double* partial) {
    constexpr int kSums = COLOR ? 56 : 28;
    constexpr int kRec = COLOR ? 2 * kIcpRec : kIcpRec;
    // the wave: a butterfly (every lane ends with the same sum, formed in the same order)
#pragma unroll
    for (int i = 0; i < kSums; ++i)
        for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
    for (int o = 32; o > 0; o >>= 1) {
        n_in += __shfl_xor(n_in, o);
        n_cand += __shfl_xor(n_cand, o);
        if constexpr (COLOR) {
            c_in += __shfl_xor(c_in, o);
            c_cand += __shfl_xor(c_cand, o);
        }
    }
    // the workgroup: through LDS, waves added in wave order
    __shared__ double sh[kIcpWG / 64][kRec];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 28; ++i) sh[wave][i] = s[i];
        sh[wave][28] = (double)n_in;  // (counts < 2^28: exact)
        sh[wave][29] = (double)n_cand;
        sh[wave][30] = sh[wave][31] = 0.0;
        if constexpr (COLOR) {
#pragma unroll
            for (int i = 0; i < 28; ++i) sh[wave][kIcpRec + i] = s[28 + i];
            sh[wave][kIcpRec + 28] = (double)c_in;
            sh[wave][kIcpRec + 29] = (double)c_cand;
            sh[wave][kIcpRec + 30] = sh[wave][kIcpRec + 31] = 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x < kRec) {
        double t = sh[0][threadIdx.x];
        for (int w = 1; w < kIcpWG / 64; ++w) t += sh[w][threadIdx.x];
        partial[(size_t)blockIdx.x * kRec + threadIdx.x] = t;
    }
}

// ---- the iteration's two kernels ----------------------------------------------
// COLOR = false is the geometric track.  COLOR = true adds, in the same pass over the frame, the
// photometric term: the frame's depth is read once, p and the projection are shared, and the
// geometric half is the same operations in the same order (the same bytes).  What COLOR switches, at
// compile time: the colour half of the pixel loop, its 28 sums and 2 counts, the second half of the
// partial record (columns 32..59 the colour sums, 60 / 61 the colour inliers / candidates), and in
// the finish the second column per lane, the lambda^2 combination and the record's tail.  Colour
// codes:
//   0 not sampled / no depth     1 behind the model camera or footprint outside its image
//   2 an invalid texel under the footprint     3 occluded (dist_max)     4 too different (color_max_diff)
//   5 inlier
template <int DK, bool COLOR>
__global__ __launch_bounds__(kIcpWG) void k_icp_linearize(IcpArgs a) {
    constexpr int kSums = COLOR ? 56 : 28;  // per lane: 0..27 geometric, 28..55 colour
    if (a.st->status != kIcpRunning) return;  // a status is set: the queued launches fall through
    float M[12];
    for (int i = 0; i < 12; ++i) M[i] = (float)a.st->M[i];
    const float dist2 = a.dist_max * a.dist_max;

    double s[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) s[i] = 0.0;
    unsigned n_in = 0, n_cand = 0;
    [[maybe_unused]] unsigned c_in = 0, c_cand = 0;

    const long long n = (long long)a.su * a.sv;
    for (long long i = (long long)blockIdx.x * kIcpWG + threadIdx.x; i < n; i += (long long)gridDim.x * kIcpWG) {
        const int u = (int)(i % a.su) * a.stride, v = (int)(i / a.su) * a.stride;
        const size_t pf = (size_t)v * a.Wf + u;
        int code = 0;
        float r = 0.0f, J[6];
        [[maybe_unused]] int cc = 0;
        [[maybe_unused]] float rc = 0.0f, Jc[6];
        const float d = depth_at<DK>(a, u, v);
        if (good_depth(d)) {
            const float xu = a.xf[u], yv = a.yf[v];
            const float V[3] = {xu * d, yv * d, d};
            float p[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = ((M[4 * k] * V[0] + M[4 * k + 1] * V[1]) + M[4 * k + 2] * V[2]) + M[4 * k + 3];
            // the projection both halves start from (the geometric half rounds it, the colour half floors it)
            const float x = a.fxm * (p[0] / p[2]) + a.cxm, y = a.fym * (p[1] / p[2]) + a.cym;
            // the geometric half
            do {
                if (u >= a.Wf - 1 || v >= a.Hf - 1) break;
                code = 1;
                const float dr = depth_at<DK>(a, u + 1, v), dd = depth_at<DK>(a, u, v + 1);
                if (!good_depth(dr) || !good_depth(dd)) break;
                const float xr = a.xf[u + 1], yd = a.yf[v + 1];
                const float Ar[3] = {xr * dr - V[0], yv * dr - V[1], dr - V[2]};
                const float Bd[3] = {xu * dd - V[0], yd * dd - V[1], dd - V[2]};
                const float c[3] = {Bd[1] * Ar[2] - Bd[2] * Ar[1], Bd[2] * Ar[0] - Bd[0] * Ar[2], Bd[0] * Ar[1] - Bd[1] * Ar[0]};
                const float l = __fsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
                if (l == 0.0f) break;
                const float nf[3] = {c[0] / l, c[1] / l, c[2] / l};
                float m[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = (M[4 * k] * nf[0] + M[4 * k + 1] * nf[1]) + M[4 * k + 2] * nf[2];
                code = 2;
                if (p[2] <= 0.0f) break;
                const float uf = rintf(x), vf = rintf(y);
                if (!(uf >= 0.0f && uf <= (float)(a.Wm - 1) && vf >= 0.0f && vf <= (float)(a.Hm - 1))) break;
                const int um = (int)uf, vm = (int)vf;
                const size_t pm = (size_t)vm * a.Wm + um;
                const float dm = a.dm[pm];
                const float nw[3] = {a.nm[3 * pm], a.nm[3 * pm + 1], a.nm[3 * pm + 2]};
                code = 3;
                if (!(dm > 0.0f) || (nw[0] == 0.0f && nw[1] == 0.0f && nw[2] == 0.0f)) break;
                const float q[3] = {a.xm[um] * dm, a.ym[vm] * dm, dm};
                float nn[3], e[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    nn[k] = (a.Rm[k] * nw[0] + a.Rm[3 + k] * nw[1]) + a.Rm[6 + k] * nw[2];
                    e[k] = q[k] - p[k];
                }
                code = 4;
                if ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > dist2) break;
                code = 5;
                if ((nn[0] * m[0] + nn[1] * m[1]) + nn[2] * m[2] < a.cos_min) break;
                code = 6;
                r = (nn[0] * e[0] + nn[1] * e[1]) + nn[2] * e[2];
                J[0] = p[1] * nn[2] - p[2] * nn[1];
                J[1] = p[2] * nn[0] - p[0] * nn[2];
                J[2] = p[0] * nn[1] - p[1] * nn[0];
                J[3] = nn[0];
                J[4] = nn[1];
                J[5] = nn[2];
            } while (false);
            // the colour half
            if constexpr (COLOR) do {
                cc = 1;
                if (p[2] <= 0.0f) break;
                const float x0 = floorf(x), y0 = floorf(y);
                if (!(x0 >= 1.0f && x0 <= (float)(a.Wm - 3) && y0 >= 1.0f && y0 <= (float)(a.Hm - 3))) break;
                const size_t pm = (size_t)(int)y0 * a.Wm + (int)x0;  // rows y0, y0 + 1 <= Hm - 2; columns x0, x0 + 1 <= Wm - 2
                const float4 t00 = a.tex[pm], t01 = a.tex[pm + 1], t10 = a.tex[pm + a.Wm], t11 = a.tex[pm + a.Wm + 1];
                cc = 2;
                if (!(t00.w > 0.0f && t01.w > 0.0f && t10.w > 0.0f && t11.w > 0.0f)) break;
                const float tx = x - x0, ty = y - y0;
                const float Db = bilerp(t00.w, t01.w, t10.w, t11.w, tx, ty);
                cc = 3;
                if (fabsf(Db - p[2]) > a.dist_max) break;
                const float Ib = bilerp(t00.x, t01.x, t10.x, t11.x, tx, ty);
                const float res = (float)a.fi[pf] - Ib;
                cc = 4;
                if (fabsf(res) > a.color_max) break;
                cc = 5;
                rc = res;
                const float ga = bilerp(t00.y, t01.y, t10.y, t11.y, tx, ty) * a.fxm;
                const float gb = bilerp(t00.z, t01.z, t10.z, t11.z, tx, ty) * a.fym;
                const float iz = 1.0f / p[2];
                const float gx = ga * iz, gy = gb * iz;
                const float g[3] = {gx, gy, -((gx * p[0] + gy * p[1]) * iz)};
                Jc[0] = p[1] * g[2] - p[2] * g[1];
                Jc[1] = p[2] * g[0] - p[0] * g[2];
                Jc[2] = p[0] * g[1] - p[1] * g[0];
                Jc[3] = g[0];
                Jc[4] = g[1];
                Jc[5] = g[2];
            } while (false);
        }
        if (code >= 2) ++n_cand;
        if (code == 6) {
            ++n_in;
            icp_add_row<0>(s, J, r);
        }
        if (a.code) a.code[pf] = (unsigned char)code;
        if (a.resid) a.resid[pf] = r;
        if constexpr (COLOR) {
            if (cc >= 2) ++c_cand;
            if (cc == 5) {
                ++c_in;
                icp_add_row<28>(s, Jc, rc);
            }
            if (a.ccode) a.ccode[pf] = (unsigned char)cc;
            if (a.cresid) a.cresid[pf] = rc;
        }
    }

    icp_reduce<COLOR>(s, n_in, n_cand, c_in, c_cand, a.partial);
}

// ---- point-to-SDF alignment -------------------------------------------------------
// The volume is a signed distance field, so a frame can be aligned to it directly: minimise the sum
// of sdf(G M p)^2 over the frame's points, with the trilinear interpolant of the stored tsdf and its
// gradient (tsdf_cell.h, the raycast's own arithmetic).  No raycast, no model maps, no frame normals.
// The row has the ICP's form (n the metric gradient in the guess camera's frame, r = -sdf), so the
// sums, the finish, the records and the host path are the ICP's.  Restated by tests/sdf_ref.py.  Codes:
//   0 not sampled / no depth     2 the cell is not inside the volume     3 a corner has weight <= 0
//   4 a corner lies on the truncated plateau (|tsdf| >= 1)     5 |r| > dist_max or a zero gradient
//   6 inlier
// One lane per sampled pixel over k_icp_linearize's launch shape, feeding k_icp_finish<false>.
template <int DK, bool HASH>
__global__ __launch_bounds__(kIcpWG) void k_sdf_linearize(IcpArgs a, SdfArgs x) {
    if (a.st->status != kIcpRunning) return;  // a status is set: the queued launches fall through
    float M[12];
    for (int i = 0; i < 12; ++i) M[i] = (float)a.st->M[i];

    double s[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) s[i] = 0.0;
    unsigned n_in = 0, n_cand = 0;

    const long long n = (long long)a.su * a.sv;
    for (long long i = (long long)blockIdx.x * kIcpWG + threadIdx.x; i < n; i += (long long)gridDim.x * kIcpWG) {
        const int u = (int)(i % a.su) * a.stride, v = (int)(i / a.su) * a.stride;
        const size_t pf = (size_t)v * a.Wf + u;
        int code = 0;
        float r = 0.0f, J[6];
        const float d = depth_at<DK>(a, u, v);
        if (good_depth(d)) {
            const float V[3] = {a.xf[u] * d, a.yf[v] * d, d};
            float p[3], t[3], c[8];
            int l[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = ((M[4 * k] * V[0] + M[4 * k + 1] * V[1]) + M[4 * k + 2] * V[2]) + M[4 * k + 3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float q = ((x.Qr[3 * k] * p[0] + x.Qr[3 * k + 1] * p[1]) + x.Qr[3 * k + 2] * p[2]) + x.Qo[k];
                const int i0 = floor_i(q);
                t[k] = q - (float)i0;
                l[k] = i0 - x.v.off[k];
            }
            code = sdf_cell<HASH>(x, l, c);
            if (code == 6) {
                float g[3];
                const float f = trilinear(c, t);
                cell_gradient(c, t, g);
                const float res = -(x.trunc * f);
                if (fabsf(res) > a.dist_max || (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f)) {
                    code = 5;
                } else {
                    float nn[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) nn[k] = x.sc * ((a.Rm[k] * g[0] + a.Rm[3 + k] * g[1]) + a.Rm[6 + k] * g[2]);
                    r = res;
                    J[0] = p[1] * nn[2] - p[2] * nn[1];
                    J[1] = p[2] * nn[0] - p[0] * nn[2];
                    J[2] = p[0] * nn[1] - p[1] * nn[0];
                    J[3] = nn[0];
                    J[4] = nn[1];
                    J[5] = nn[2];
                }
            }
        }
        if (code >= 2) ++n_cand;
        if (code == 6) {
            ++n_in;
            icp_add_row<0>(s, J, r);
        }
        if (a.code) a.code[pf] = (unsigned char)code;
        if (a.resid) a.resid[pf] = r;
    }
    icp_reduce<false>(s, n_in, n_cand, 0u, 0u, a.partial);
}

// tsdf_*_sample: the same cell at n world points.
template <bool HASH>
__global__ __launch_bounds__(256) void k_sdf_sample(SdfArgs x, const double* P, long long n, float* sdf, float* grad,
                                                    unsigned char* code) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float t[3], c[8];
    int l[3];
    for (int k = 0; k < 3; ++k) {
        const float q = (float)((P[3 * i + k] - (double)x.v.origin[k]) / x.v.vs);
        const int i0 = floor_i(q);
        t[k] = q - (float)i0;
        l[k] = i0 - x.v.off[k];
    }
    const int cd = sdf_cell<HASH>(x, l, c);
    float f = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    if (cd >= 4) {
        f = x.trunc * trilinear(c, t);
        cell_gradient(c, t, g);
        for (int k = 0; k < 3; ++k) g[k] = x.sc * g[k];
    }
    if (sdf) sdf[i] = f;
    if (grad)
        for (int k = 0; k < 3; ++k) grad[3 * i + k] = g[k];
    if (code) code[i] = (unsigned char)cd;
}

struct FinishArgs {
    const double* partial;  // n_partial records, as wide as the linearise instance wrote them
    int n_partial;
    IcpState* st;
    IcpRecord* rec;   // this iteration's
    int solve;        // 0: sums only (the handle-less linearisations)
    int last;         // the last iteration of the call: still running afterwards means max_iter
    long long min_inliers;
    double eps_rot, eps_trans;
    double l2;        // color_weight^2 (the RGB-D instance)
};

constexpr int kFinSlices = 32;
constexpr int kFinWG = kFinSlices * kIcpRec;  // 1024: the loads of the partial records spread over many lanes

// A xi = b by Cholesky (A = L L^T, lower triangle, then the two triangular solves), E = Rodrigues(w)
// with translation t, M <- E M, on the 27 sums in t.  Returns the status; M, w_norm and t_norm change
// only when the step is taken.  Every loop is unrolled so that L, y and xi are never indexed by a
// variable: they stay in registers (no private segment).
__device__ int icp_solve_update(const double* t, bool enough, int last, double eps_rot, double eps_trans, double* M,
                                double* w_norm, double* t_norm) {
    double L[6][6], b[6];
    int k = 0;
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = x; y < 6; ++y) L[y][x] = t[k++];
#pragma unroll
    for (int x = 0; x < 6; ++x) b[x] = t[21 + x];
    bool ok = enough;
#pragma unroll
    for (int c = 0; c < 6 && ok; ++c) {
        double d = L[c][c];
#pragma unroll
        for (int e = 0; e < c; ++e) d -= L[c][e] * L[c][e];
        if (!(d > 0.0) || !(d < INFINITY)) {
            ok = false;
            break;
        }
        d = sqrt(d);
        L[c][c] = d;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            double x = L[r][c];
#pragma unroll
            for (int e = 0; e < c; ++e) x -= L[r][e] * L[c][e];
            L[r][c] = x / d;
        }
    }
    if (!ok) return TSDF_TRACK_LOST;
    double y[6], xi[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double x = b[r];
#pragma unroll
        for (int e = 0; e < r; ++e) x -= L[r][e] * y[e];
        y[r] = x / L[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double x = y[r];
#pragma unroll
        for (int e = r + 1; e < 6; ++e) x -= L[e][r] * xi[e];
        xi[r] = x / L[r][r];
    }
    const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2, th = sqrt(th2);
    double A = 1.0, Bc = 0.5;
    if (th > 1e-8) {
        A = sin(th) / th;
        Bc = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double E[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double k2 = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
            E[3 * r + c] = ((r == c ? 1.0 : 0.0) + A * K[3 * r + c]) + Bc * k2;
        }
    double N[16];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double x = (E[3 * r] * M[c] + E[3 * r + 1] * M[4 + c]) + E[3 * r + 2] * M[8 + c];
            if (c == 3) x += xi[3 + r];
            N[4 * r + c] = x;
        }
    N[12] = N[13] = N[14] = 0.0;
    N[15] = 1.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && N[i] - N[i] == 0.0;
    if (!finite) return TSDF_TRACK_LOST;
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = N[i];
    *w_norm = th;
    *t_norm = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
    if (*w_norm <= eps_rot && *t_norm <= eps_trans) return TSDF_TRACK_CONVERGED;
    return last ? TSDF_TRACK_MAX_ITER : kIcpRunning;
}

template <bool COLOR>
__global__ __launch_bounds__(kFinWG) void k_icp_finish(FinishArgs a) {
    constexpr int kHalves = COLOR ? 2 : 1, kRec = kHalves * kIcpRec;
    if (a.st->status != kIcpRunning) return;
    // the partial records: lane (slice, j) adds column j of each half over the records slice,
    // slice + 32, ...; then the slices in order.  A half is added in the same order in both instances
    // (which is what makes lambda = 0 byte-identical to the geometric track)
    __shared__ double sh[kFinSlices][kRec];
    __shared__ double tot[kRec];
    const int j = threadIdx.x & 31, slice = threadIdx.x >> 5;
    double t[kHalves];
#pragma unroll
    for (int h = 0; h < kHalves; ++h) t[h] = 0.0;
    if (j < 30) {
#pragma unroll 4
        for (int g = slice; g < a.n_partial; g += kFinSlices)
#pragma unroll
            for (int h = 0; h < kHalves; ++h) t[h] += a.partial[(size_t)g * kRec + h * kIcpRec + j];
    }
#pragma unroll
    for (int h = 0; h < kHalves; ++h) sh[slice][h * kIcpRec + j] = t[h];
    __syncthreads();
    if (threadIdx.x < kRec) {
        double x = sh[0][threadIdx.x];
        for (int k = 1; k < kFinSlices; ++k) x += sh[k][threadIdx.x];
        tot[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    IcpRecord& R = *a.rec;
    for (int i = 0; i < 28; ++i) R.sums[i] = tot[i];
    R.inliers = (long long)tot[28];
    R.candidates = (long long)tot[29];
    if constexpr (COLOR) {
        for (int i = 0; i < 28; ++i) R.csums[i] = tot[kIcpRec + i];
        R.c_inliers = (long long)tot[kIcpRec + 28];
        R.c_candidates = (long long)tot[kIcpRec + 29];
    }
    R.w_norm = R.t_norm = 0.0;
    double M[16];
    for (int i = 0; i < 16; ++i) M[i] = a.st->M[i];
    int status = kIcpRunning;
    if (a.solve) {
        double comb[27];  // A = A_g + lambda^2 A_c, b = b_g + lambda^2 b_c; the geometric totals go in as they are
        if constexpr (COLOR)
            for (int i = 0; i < 27; ++i) comb[i] = tot[i] + a.l2 * tot[kIcpRec + i];
        status = icp_solve_update(COLOR ? comb : tot, R.inliers >= a.min_inliers, a.last, a.eps_rot, a.eps_trans, M, &R.w_norm,
                                  &R.t_norm);
    }
    for (int i = 0; i < 16; ++i) {
        R.M[i] = M[i];
        a.st->M[i] = M[i];
    }
    R.status = status;
    a.st->iters += 1;
    a.st->status = status;
}

// ---- host side ---------------------------------------------------------------------------------
int ensure(IcpCtx& c, int which, size_t need) {
    if (need <= c.bytes[which]) return TSDF_OK;
    if (c.buf[which]) {
        TSDF_HIP(hipStreamSynchronize(c.stream));
        TSDF_HIP(hipFree(c.buf[which]));
        c.buf[which] = nullptr;
        c.bytes[which] = 0;
    }
    TSDF_HIP(hipMalloc(&c.buf[which], need));
    c.bytes[which] = need;
    return TSDF_OK;
}

bool bad_size(int H, int W) {
    return H <= 0 || W <= 0 || H >= (1 << 24) || W >= (1 << 24) || (long long)H * W >= (1ll << 28);
}

int check_params(const tsdf_icp_params_t* p) {
    if (!p) return set_error(TSDF_E_ARG, "null params pointer");
    if (p->stride < 1) return set_error(TSDF_E_ARG, "stride must be >= 1 (got %d)", p->stride);
    if (p->max_iter < 1 || p->max_iter > kIcpMaxIter)
        return set_error(TSDF_E_ARG, "max_iter must be in [1, %d] (got %d)", kIcpMaxIter, p->max_iter);
    if (!(p->dist_max > 0.0) || !((float)p->dist_max > 0.0f) || !std::isfinite((float)p->dist_max))
        return set_error(TSDF_E_ARG, "dist_max must be > 0 (got %g)", p->dist_max);
    if (!(p->cos_min >= -1.0 && p->cos_min <= 1.0))
        return set_error(TSDF_E_ARG, "cos_min must be in [-1, 1] (got %g)", p->cos_min);
    if (p->min_inliers < 0) return set_error(TSDF_E_ARG, "min_inliers must be >= 0 (got %lld)", (long long)p->min_inliers);
    if (!(p->eps_rot >= 0.0) || !(p->eps_trans >= 0.0))
        return set_error(TSDF_E_ARG, "eps_rot / eps_trans must be >= 0 (got %g, %g)", p->eps_rot, p->eps_trans);
    return TSDF_OK;
}

// The guess of a track is a camera pose: its rotation must be one.  A scaled, sheared, mirrored, zero
// or NaN rotation block makes systems the solver steps to nowhere from (a guess scaled by (1, 2, 0.5)
// gave cond(A) = 6e15 and a step of 37 km), so it is refused like the merge's transform.  The tolerance
// admits poses read from text with about eight digits ((R^T R - I) up to 1.5e-4 in the lounge
// sequence); the translation is not looked at: a NaN or infinite one finds no inlier and ends lost.
int check_guess(const double* T) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
            if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-3))
                return set_error(TSDF_E_ARG, "the rotation of pose_guess is not orthonormal ((R^T R)[%d][%d] = %.9g)", i, j, d);
        }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) +
                       T[2] * (T[4] * T[9] - T[5] * T[8]);
    if (!(std::fabs(det - 1.0) <= 1e-3)) return set_error(TSDF_E_ARG, "the rotation of pose_guess has determinant %.9g, not +1", det);
    return TSDF_OK;
}

int check_color_params(const tsdf_icp_color_params_t* q) {
    if (!q) return set_error(TSDF_E_ARG, "null color params pointer");
    if (!(q->color_weight >= 0.0) || !std::isfinite(q->color_weight))
        return set_error(TSDF_E_ARG, "color_weight must be finite and >= 0 (got %g)", q->color_weight);
    if (!(q->color_max_diff > 0.0f)) return set_error(TSDF_E_ARG, "color_max_diff must be > 0 (got %g)", (double)q->color_max_diff);
    return TSDF_OK;
}

struct Cameras {
    int Hf, Wf, Hm, Wm;
    const double *Kf, *Km, *model_pose;
};

// The device images of one call.  rgb and mc (the frame's RGB8 image and the model's colour map) are
// null for a geometric call; the four maps are optional outputs.
struct Images {
    const void* depth;
    const float *dm, *nm;
    const unsigned char *rgb, *mc;
    unsigned char* code;
    float* resid;
    unsigned char* ccode;
    float* cresid;
};

// The volume's side of an SDF linearisation at pose_guess (null: tsdf_*_sample, which needs none):
// f64, each value rounded to f32 once.
void sdf_volume(const RaySource& S, const double* pose_guess, SdfArgs* x) {
    const Base& B = *S.b;
    *x = SdfArgs{};
    x->v = B.vol;
    x->pool = B.pool;
    if (S.table) x->t = *S.table;
    x->hash = S.table ? 1 : 0;
    for (int r = 0; r < 3 && pose_guess; ++r) {
        for (int k = 0; k < 3; ++k) x->Qr[3 * r + k] = (float)(pose_guess[4 * r + k] / B.vol.vs);
        x->Qo[r] = (float)((pose_guess[4 * r + 3] - (double)B.vol.origin[r]) / B.vol.vs);
    }
    x->sc = (float)(B.vol.trunc / B.vol.vs);
    x->trunc = (float)B.vol.trunc;
}

// The tracking buffers of a handle (created by its first track), on the handle's stream.
IcpCtx& handle_ctx(Base& B) {
    if (!B.icp) {
        B.icp = new IcpCtx();
        B.icp->device = B.device;
        B.icp->stream = B.stream;
    }
    return *B.icp;
}

unsigned linearize_grid(const IcpArgs& a, int n_cu) {
    const long long n = (long long)a.su * a.sv;
    return (unsigned)std::max(1ll, std::min<long long>((n + kIcpWG - 1) / kIcpWG, (long long)std::max(n_cu, 1) * 4));
}

// The arguments of the linearise launches of one call, with the tables queued on the stream; with a
// colour image (q is then its parameters) also the intensity image and the photo texels, by one prep
// launch queued after ev_prep.
int prepare(IcpCtx& c, const Cameras& cam, const tsdf_icp_params_t& p, int dk, int flags, const Images& im,
            const tsdf_icp_color_params_t* q, int n_cu, IcpArgs* out, unsigned* grid, hipEvent_t ev_prep = nullptr) {
    IcpArgs a{};
    a.depth = im.depth;
    a.dk = dk;
    a.inval = (flags & TSDF_DEPTH_INVALID_65535) ? 1 : 0;
    a.Hf = cam.Hf;
    a.Wf = cam.Wf;
    a.Hm = cam.Hm;
    a.Wm = cam.Wm;
    a.stride = p.stride;
    a.su = (cam.Wf + p.stride - 1) / p.stride;
    a.sv = (cam.Hf + p.stride - 1) / p.stride;
    a.dm = im.dm;
    a.nm = im.nm;
    const size_t nt = (size_t)cam.Wf + cam.Hf + cam.Wm + cam.Hm;
    TSDF_TRY(ensure(c, kBufTables, nt * sizeof(float)));
    float* t = (float*)c.buf[kBufTables];
    a.xf = t;
    a.yf = t + cam.Wf;
    a.xm = a.yf + cam.Hf;
    a.ym = a.xm + cam.Wm;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) a.Rm[3 * r + k] = (float)cam.model_pose[4 * r + k];
    a.fxm = (float)cam.Km[0];
    a.fym = (float)cam.Km[4];
    a.cxm = (float)cam.Km[2];
    a.cym = (float)cam.Km[5];
    a.dist_max = (float)p.dist_max;
    a.cos_min = (float)p.cos_min;
    a.st = (const IcpState*)c.buf[kBufState];
    *grid = linearize_grid(a, n_cu);
    TSDF_TRY(ensure(c, kBufPartial, (size_t)*grid * (im.rgb ? 2 : 1) * kIcpRec * sizeof(double)));
    a.partial = (double*)c.buf[kBufPartial];
    a.code = im.code;
    a.resid = im.resid;
    hipLaunchKernelGGL(k_icp_tables, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c.stream, cam.Wf, cam.Hf, cam.Wm,
                       cam.Hm, cam.Kf[0], cam.Kf[4], cam.Kf[2], cam.Kf[5], cam.Km[0], cam.Km[4], cam.Km[2], cam.Km[5], t);
    TSDF_HIP(hipGetLastError());
    // pixels no lane visits (stride > 1) read code 0, residual 0
    const size_t pf = (size_t)cam.Hf * cam.Wf, pm = (size_t)cam.Hm * cam.Wm;
    if (p.stride > 1) {
        if (im.code) TSDF_HIP(hipMemsetAsync(im.code, 0, pf, c.stream));
        if (im.resid) TSDF_HIP(hipMemsetAsync(im.resid, 0, pf * sizeof(float), c.stream));
    }
    if (im.rgb) {
        if (ev_prep) TSDF_HIP(hipEventRecord(ev_prep, c.stream));
        TSDF_TRY(ensure(c, kBufFrameI, pf));
        TSDF_TRY(ensure(c, kBufTexel, pm * sizeof(float4)));
        a.fi = (const unsigned char*)c.buf[kBufFrameI];
        a.tex = (const float4*)c.buf[kBufTexel];
        a.color_max = q->color_max_diff;
        a.ccode = im.ccode;
        a.cresid = im.cresid;
        hipLaunchKernelGGL(k_icp_photo_prep, dim3((unsigned)((std::max(pf, pm) + 255) / 256)), dim3(256), 0, c.stream, im.rgb,
                           (int)pf, (unsigned char*)c.buf[kBufFrameI], im.mc, a.dm, a.Hm, a.Wm, (float4*)c.buf[kBufTexel]);
        TSDF_HIP(hipGetLastError());
        if (p.stride > 1) {
            if (im.ccode) TSDF_HIP(hipMemsetAsync(im.ccode, 0, pf, c.stream));
            if (im.cresid) TSDF_HIP(hipMemsetAsync(im.cresid, 0, pf * sizeof(float), c.stream));
        }
    }
    *out = a;
    return TSDF_OK;
}

// One iteration: the linearise instance of the depth kind and of whether prepare() saw a colour
// image -- or, with x, the SDF linearise of the depth kind and of the handle's kind --, then the
// finish of the same kind.
int launch_iteration(IcpCtx& c, const IcpArgs& a, const SdfArgs* x, unsigned grid, IcpRecord* rec, int solve, int last,
                     const tsdf_icp_params_t& p, const tsdf_icp_color_params_t* q, hipEvent_t ev_mid = nullptr,
                     hipEvent_t ev_end = nullptr) {
    const bool u16 = a.dk == TSDF_DEPTH_U16_MM, rgbd = a.fi != nullptr;
    if (x) {
        auto lin = x->hash ? (u16 ? k_sdf_linearize<TSDF_DEPTH_U16_MM, true> : k_sdf_linearize<TSDF_DEPTH_F64_M, true>)
                           : (u16 ? k_sdf_linearize<TSDF_DEPTH_U16_MM, false> : k_sdf_linearize<TSDF_DEPTH_F64_M, false>);
        hipLaunchKernelGGL(lin, dim3(grid), dim3(kIcpWG), 0, c.stream, a, *x);
    } else {
        auto lin = rgbd ? (u16 ? k_icp_linearize<TSDF_DEPTH_U16_MM, true> : k_icp_linearize<TSDF_DEPTH_F64_M, true>)
                        : (u16 ? k_icp_linearize<TSDF_DEPTH_U16_MM, false> : k_icp_linearize<TSDF_DEPTH_F64_M, false>);
        hipLaunchKernelGGL(lin, dim3(grid), dim3(kIcpWG), 0, c.stream, a);
    }
    TSDF_HIP(hipGetLastError());
    if (ev_mid) TSDF_HIP(hipEventRecord(ev_mid, c.stream));
    FinishArgs f{};
    f.partial = a.partial;
    f.n_partial = (int)grid;
    f.st = (IcpState*)c.buf[kBufState];
    f.rec = rec;
    f.solve = solve;
    f.last = last;
    f.min_inliers = p.min_inliers;
    f.eps_rot = p.eps_rot;
    f.eps_trans = p.eps_trans;
    f.l2 = rgbd ? q->color_weight * q->color_weight : 0.0;
    hipLaunchKernelGGL(rgbd ? k_icp_finish<true> : k_icp_finish<false>, dim3(1), dim3(kFinWG), 0, c.stream, f);
    TSDF_HIP(hipGetLastError());
    if (ev_end) TSDF_HIP(hipEventRecord(ev_end, c.stream));
    return TSDF_OK;
}

// state block: IcpState, 16 doubles of an uploaded pose, then the records
constexpr size_t kStateOff = 0, kPoseOff = 256, kRecOff = 512;
size_t state_bytes(int n_rec) { return kRecOff + sizeof(IcpRecord) * (size_t)n_rec; }

// per-device contexts of the handle-less call
constexpr int kMaxDev = 64;
IcpCtx* g_dev_ctx[kMaxDev] = {};
std::mutex g_dev_mu;

// HIP-event times of the calling thread's last track on a handle with profiling on
thread_local double g_track_ms[6] = {-1.0, -1.0, -1.0, -1.0, -1.0, 0.0};
thread_local double g_track_prep_ms = -1.0;  // the prep launch of its last RGB-D track

// The six handle entry points.  rgbd: the raycast also writes the model's colour map, one prep
// launch, and the colour instances of the two kernels; else color, q and cinfo are null.  sdf (never
// with rgbd): point-to-SDF alignment on the volume itself (§7g) -- no raycast (cast is null and the
// z range unused), no model maps; everything else is the same path.
int track(const RaySource& S, int (*cast)(void*, int, int, const double*, const double*, double, double, double, float*,
                                          float*, uint8_t*, int),
          void* handle, bool rgbd, bool sdf, const void* depth, int dk, const uint8_t* color, int H, int W, const double* K,
          const double* pose_guess, const tsdf_icp_params_t* p, const tsdf_icp_color_params_t* q, double zn, double zf,
          double zs, double* out_pose, tsdf_track_info_t* info, tsdf_track_color_info_t* cinfo, double* trajectory,
          int flags) {
    Base& B = *S.b;
    if (!depth) return set_error(TSDF_E_ARG, "null depth pointer");
    if (rgbd && !color) return set_error(TSDF_E_ARG, "null color image pointer");
    if (!K || !pose_guess) return set_error(TSDF_E_ARG, "null camera pointer");
    if (!out_pose) return set_error(TSDF_E_ARG, "null out_pose pointer");
    if (dk != TSDF_DEPTH_U16_MM && dk != TSDF_DEPTH_F64_M) return set_error(TSDF_E_ARG, "bad depth_kind %d", dk);
    if (bad_size(H, W)) return set_error(TSDF_E_ARG, "bad image size %dx%d", H, W);
    if (rgbd && (H < 4 || W < 4))
        return set_error(TSDF_E_ARG, "the colour term needs a model map of at least 4x4 (got %dx%d)", H, W);
    TSDF_TRY(check_params(p));
    if (rgbd) TSDF_TRY(check_color_params(q));
    TSDF_TRY(check_guess(pose_guess));
    IcpCtx& c = handle_ctx(B);
    const size_t px = (size_t)H * W;
    const bool dev = (flags & TSDF_DEVICE_PTRS) != 0;
    if (!sdf) {
        TSDF_TRY(ensure(c, kBufModelD, px * sizeof(float)));
        TSDF_TRY(ensure(c, kBufModelN, px * 3 * sizeof(float)));
    }
    if (rgbd) TSDF_TRY(ensure(c, kBufModelC, px * 3));
    TSDF_TRY(ensure(c, kBufState, state_bytes(p->max_iter)));
    Images im{};
    im.depth = depth;
    im.rgb = rgbd ? color : nullptr;
    if (!dev) {
        TSDF_TRY(ensure(c, kBufDepth, frame_bytes_depth(dk, H, W)));
        im.depth = c.buf[kBufDepth];
        if (rgbd) {
            TSDF_TRY(ensure(c, kBufRgb, px * 3));
            im.rgb = (const unsigned char*)c.buf[kBufRgb];
        }
    }
    im.dm = sdf ? nullptr : (const float*)c.buf[kBufModelD];
    im.nm = sdf ? nullptr : (const float*)c.buf[kBufModelN];
    im.mc = rgbd ? (const unsigned char*)c.buf[kBufModelC] : nullptr;
    // profiling on: events around the raycast, the setup, the prep of an RGB-D track and every launch
    // of the iterations
    const bool timed = B.prof.on;
    const size_t off = rgbd ? 1 : 0;  // the prep's event
    std::vector<hipEvent_t> ev(timed ? 3 + off + 2 * (size_t)p->max_iter : 0, nullptr);
    struct EvGuard {
        std::vector<hipEvent_t>& e;
        ~EvGuard() {
            for (auto x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev_guard{ev};
    for (auto& e : ev) TSDF_HIP(hipEventCreate(&e));
    if (timed) TSDF_HIP(hipEventRecord(ev[0], c.stream));
    // the model maps: the handle's own raycast at pose_guess (it runs the deferred frames first and
    // refuses what a raycast refuses)
    if (!sdf)
        TSDF_TRY(cast(handle, H, W, K, pose_guess, zn, zf, zs, (float*)c.buf[kBufModelD], (float*)c.buf[kBufModelN],
                      rgbd ? (uint8_t*)c.buf[kBufModelC] : nullptr, TSDF_DEVICE_PTRS | TSDF_ASYNC));
    if (timed) TSDF_HIP(hipEventRecord(ev[1], c.stream));
    if (!dev) {
        TSDF_HIP(hipMemcpyAsync(c.buf[kBufDepth], depth, frame_bytes_depth(dk, H, W), hipMemcpyHostToDevice, c.stream));
        if (rgbd) TSDF_HIP(hipMemcpyAsync(c.buf[kBufRgb], color, px * 3, hipMemcpyHostToDevice, c.stream));
    }
    char* sb = (char*)c.buf[kBufState];
    IcpRecord* rec = (IcpRecord*)(sb + kRecOff);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, c.stream, (IcpState*)(sb + kStateOff), (const double*)nullptr);
    TSDF_HIP(hipGetLastError());
    Cameras cam{H, W, sdf ? 0 : H, sdf ? 0 : W, K, K, pose_guess};  // (SDF: no model camera; Rm is R_G either way)
    IcpArgs a;
    SdfArgs sx;
    if (sdf) sdf_volume(S, pose_guess, &sx);
    unsigned grid;
    TSDF_TRY(prepare(c, cam, *p, dk, flags, im, q, B.n_cu, &a, &grid, timed && rgbd ? ev[2] : nullptr));
    if (timed) TSDF_HIP(hipEventRecord(ev[2 + off], c.stream));
    for (int it = 0; it < p->max_iter; ++it)
        TSDF_TRY(launch_iteration(c, a, sdf ? &sx : nullptr, grid, rec + it, 1, it == p->max_iter - 1, *p, q,
                                  timed ? ev[3 + off + 2 * it] : nullptr, timed ? ev[4 + off + 2 * it] : nullptr));
    // one synchronisation, one copy back
    std::vector<char> host(state_bytes(p->max_iter));
    TSDF_HIP(hipMemcpyAsync(host.data(), sb, host.size(), hipMemcpyDeviceToHost, c.stream));
    TSDF_HIP(hipStreamSynchronize(c.stream));
    const IcpState* st = (const IcpState*)(host.data() + kStateOff);
    const IcpRecord* hr = (const IcpRecord*)(host.data() + kRecOff);
    const int iters = std::min(std::max(st->iters, 0), p->max_iter);
    if (timed) {
        // raycast, setup, linearise, finish (iterations run), fall-through launches; and the prep launch
        double ms[5] = {0, 0, 0, 0, 0}, prep = 0.0;
        for (size_t i = 0; i + 1 < ev.size(); ++i) {
            float x = 0.0f;
            TSDF_HIP(hipEventElapsedTime(&x, ev[i], ev[i + 1]));
            if (i < 2) ms[i] += sdf && i == 0 ? 0.0f : x;  // (no raycast was queued between ev[0] and ev[1])
            else if (i < 2 + off) prep += x;
            else ms[(int)(i - 2 - off) / 2 >= iters ? 4 : 2 + (int)(i - 2 - off) % 2] += x;
        }
        for (int i = 0; i < 5; ++i) g_track_ms[i] = ms[i];
        g_track_ms[5] = (double)iters;
        if (rgbd) g_track_prep_ms = prep;
    }
    // out_pose = pose_guess * M, f64, three-term sums left to right
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            double x = 0.0;
            for (int e = 0; e < 4; ++e) x += pose_guess[4 * r + e] * st->M[4 * e + k];
            out_pose[4 * r + k] = x;
        }
    if (info) memset(info, 0, sizeof(*info));
    if (cinfo) memset(cinfo, 0, sizeof(*cinfo));
    if (info) {
        info->status = st->status;
        info->iterations = iters;
    }
    if (iters > 0) {
        const IcpRecord& L = hr[iters - 1];
        if (info) {
            info->inliers = L.inliers;
            info->candidates = L.candidates;
            info->rms = L.inliers > 0 ? std::sqrt(L.sums[27] / (double)L.inliers) : 0.0;
            info->w_norm = L.w_norm;
            info->t_norm = L.t_norm;
        }
        if (cinfo) {
            cinfo->color_inliers = L.c_inliers;
            cinfo->color_candidates = L.c_candidates;
            cinfo->color_rms = L.c_inliers > 0 ? std::sqrt(L.csums[27] / (double)L.c_inliers) : 0.0;
        }
    }
    if (trajectory) {
        memset(trajectory, 0, sizeof(double) * 16 * ((size_t)p->max_iter + 1));
        for (int i = 0; i < 4; ++i) trajectory[5 * i] = 1.0;
        for (int i = 0; i < iters; ++i) memcpy(trajectory + 16 * (i + 1), hr[i].M, sizeof(double) * 16);
    }
    return TSDF_OK;
}

int cast_dense(void* h, int H, int W, const double* K, const double* pose, double zn, double zf, double zs, float* d,
               float* n, uint8_t* c, int flags) {
    return tsdf_dense_raycast((tsdf_dense_t*)h, H, W, K, pose, zn, zf, zs, d, n, c, flags);
}
int cast_hash(void* h, int H, int W, const double* K, const double* pose, double zn, double zf, double zs, float* d,
              float* n, uint8_t* c, int flags) {
    return tsdf_hash_raycast((tsdf_hash_t*)h, H, W, K, pose, zn, zf, zs, d, n, c, flags);
}

// The per-device context of the handle-less calls (created on first use), with the device made current.
int device_context(int device, IcpCtx** out, int* n_cu) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error(TSDF_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= ndev || device >= kMaxDev)
        return set_error(TSDF_E_ARG, "device %d out of range [0,%d)", device, std::min(ndev, kMaxDev));
    TSDF_HIP(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!g_dev_ctx[device]) {
        IcpCtx* n = new IcpCtx();
        n->device = device;
        n->own_stream = true;
        const hipError_t e = hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete n;
            TSDF_HIP(e);
        }
        g_dev_ctx[device] = n;
    }
    *out = g_dev_ctx[device];
    *n_cu = 256;
    (void)hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, device);
    return TSDF_OK;
}

// The two handle-less entry points and the two SDF ones: one linearisation at rel_pose, no solve.
// rgbd: sums[56] and counts[4], else sums[28] and counts[2], and color, model_colors, q and the colour
// maps are null.  S (never with rgbd): the SDF linearisation on that handle, with its buffers and on
// its stream; the model maps and the model camera are null / 0 and model_pose is the guess.
int linearize_once(const RaySource* S, bool rgbd, int device, const void* depth, int dk, const uint8_t* color, int Hf, int Wf, const double* Kf,
                   const double* rel_pose, const float* model_depth, const float* model_normals, const uint8_t* model_colors,
                   int Hm, int Wm, const double* Km, const double* model_pose, const tsdf_icp_params_t* params,
                   const tsdf_icp_color_params_t* q, double* sums, int64_t* counts, uint8_t* code, float* residual,
                   uint8_t* color_code, float* color_residual, int flags) {
    if (!depth) return set_error(TSDF_E_ARG, "null depth pointer");
    if (rgbd && !color) return set_error(TSDF_E_ARG, "null color image pointer");
    if (!S && (!model_depth || !model_normals || (rgbd && !model_colors))) return set_error(TSDF_E_ARG, "null model map pointer");
    if (!Kf || !Km || !rel_pose || !model_pose) return set_error(TSDF_E_ARG, "null camera pointer");
    if (!sums || !counts) return set_error(TSDF_E_ARG, "null sums / counts pointer");
    if (dk != TSDF_DEPTH_U16_MM && dk != TSDF_DEPTH_F64_M) return set_error(TSDF_E_ARG, "bad depth_kind %d", dk);
    if (bad_size(Hf, Wf)) return set_error(TSDF_E_ARG, "bad frame image size %dx%d", Hf, Wf);
    if (!S && bad_size(Hm, Wm)) return set_error(TSDF_E_ARG, "bad model image size %dx%d", Hm, Wm);
    if (rgbd && (Hm < 4 || Wm < 4))
        return set_error(TSDF_E_ARG, "the colour term needs a model map of at least 4x4 (got %dx%d)", Hm, Wm);
    TSDF_TRY(check_params(params));
    if (rgbd) TSDF_TRY(check_color_params(q));
    IcpCtx* cp;
    int n_cu;
    if (S) {
        cp = &handle_ctx(*S->b);
        n_cu = S->b->n_cu;
    } else {
        TSDF_TRY(device_context(device, &cp, &n_cu));
    }
    IcpCtx& c = *cp;
    std::lock_guard<std::mutex> lk(c.mu);  // one call at a time per device context
    const bool dev = (flags & TSDF_DEVICE_PTRS) != 0;
    const size_t pf = (size_t)Hf * Wf, pm = (size_t)Hm * Wm;
    TSDF_TRY(ensure(c, kBufState, state_bytes(1)));
    // host images go through the context's buffers: {caller's pointer, buffer, bytes}; a null row
    // (the colour rows of the geometric call, an output not asked for) is skipped
    struct Img {
        const void* host;
        int buf;
        size_t bytes;
    };
    const Img in[5] = {{depth, kBufDepth, frame_bytes_depth(dk, Hf, Wf)}, {color, kBufRgb, pf * 3},
                       {model_depth, kBufModelD, pm * sizeof(float)}, {model_normals, kBufModelN, pm * 3 * sizeof(float)},
                       {model_colors, kBufModelC, pm * 3}};
    const Img outs[4] = {{code, kBufCode, pf}, {residual, kBufResid, pf * sizeof(float)}, {color_code, kBufCodeC, pf},
                         {color_residual, kBufResidC, pf * sizeof(float)}};
    const void* din[5];
    void* dout[4];
    for (int i = 0; i < 5; ++i) {
        din[i] = in[i].host;
        if (dev || !in[i].host) continue;
        TSDF_TRY(ensure(c, in[i].buf, in[i].bytes));
        TSDF_HIP(hipMemcpyAsync(c.buf[in[i].buf], in[i].host, in[i].bytes, hipMemcpyHostToDevice, c.stream));
        din[i] = c.buf[in[i].buf];
    }
    for (int i = 0; i < 4; ++i) {
        dout[i] = const_cast<void*>(outs[i].host);
        if (dev || !outs[i].host) continue;
        TSDF_TRY(ensure(c, outs[i].buf, outs[i].bytes));
        dout[i] = c.buf[outs[i].buf];
    }
    char* sb = (char*)c.buf[kBufState];
    TSDF_HIP(hipMemcpyAsync(sb + kPoseOff, rel_pose, sizeof(double) * 16, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, c.stream, (IcpState*)(sb + kStateOff), (const double*)(sb + kPoseOff));
    TSDF_HIP(hipGetLastError());
    Cameras cam{Hf, Wf, Hm, Wm, Kf, Km, model_pose};
    const Images im{din[0], (const float*)din[2], (const float*)din[3], (const unsigned char*)din[1],
                    (const unsigned char*)din[4], (unsigned char*)dout[0], (float*)dout[1], (unsigned char*)dout[2],
                    (float*)dout[3]};
    IcpArgs a;
    SdfArgs sx;
    if (S) sdf_volume(*S, model_pose, &sx);
    unsigned grid;
    TSDF_TRY(prepare(c, cam, *params, dk, flags, im, q, n_cu, &a, &grid));
    TSDF_TRY(launch_iteration(c, a, S ? &sx : nullptr, grid, (IcpRecord*)(sb + kRecOff), 0, 1, *params, q));
    IcpRecord rec;
    TSDF_HIP(hipMemcpyAsync(&rec, sb + kRecOff, sizeof(rec), hipMemcpyDeviceToHost, c.stream));
    if (!dev)
        for (int i = 0; i < 4; ++i)
            if (outs[i].host) TSDF_HIP(hipMemcpyAsync(const_cast<void*>(outs[i].host), dout[i], outs[i].bytes, hipMemcpyDeviceToHost, c.stream));
    TSDF_HIP(hipStreamSynchronize(c.stream));
    memcpy(sums, rec.sums, sizeof(double) * 28);
    counts[0] = rec.inliers;
    counts[1] = rec.candidates;
    if (rgbd) {
        memcpy(sums + 28, rec.csums, sizeof(double) * 28);
        counts[2] = rec.c_inliers;
        counts[3] = rec.c_candidates;
    }
    return TSDF_OK;
}

// tsdf_*_sample: the cell of k_sdf_linearize at n world points, through the handle's tracking buffers.
int sample(const RaySource& S, const double* points, int64_t n, float* sdf, float* grad, uint8_t* code, int flags) {
    Base& B = *S.b;
    if (n < 0 || n >= (1ll << 31)) return set_error(TSDF_E_ARG, "bad point count %lld", (long long)n);
    if (n == 0) return TSDF_OK;
    if (!points) return set_error(TSDF_E_ARG, "null points pointer");
    IcpCtx& c = handle_ctx(B);
    const bool dev = (flags & TSDF_DEVICE_PTRS) != 0;
    const double* dp = points;
    void* out[3] = {sdf, grad, code};
    const int buf[3] = {kBufResid, kBufModelN, kBufCode};
    const size_t bytes[3] = {(size_t)n * sizeof(float), (size_t)n * 3 * sizeof(float), (size_t)n};
    void* dout[3] = {sdf, grad, code};
    if (!dev) {
        TSDF_TRY(ensure(c, kBufDepth, (size_t)n * 3 * sizeof(double)));
        TSDF_HIP(hipMemcpyAsync(c.buf[kBufDepth], points, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c.stream));
        dp = (const double*)c.buf[kBufDepth];
        for (int i = 0; i < 3; ++i) {
            if (!out[i]) continue;
            TSDF_TRY(ensure(c, buf[i], bytes[i]));
            dout[i] = c.buf[buf[i]];
        }
    }
    SdfArgs sx;
    sdf_volume(S, nullptr, &sx);
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(sx.hash ? k_sdf_sample<true> : k_sdf_sample<false>, dim3(grid), dim3(256), 0, c.stream, sx, dp,
                       (long long)n, (float*)dout[0], (float*)dout[1], (unsigned char*)dout[2]);
    TSDF_HIP(hipGetLastError());
    if (!dev)
        for (int i = 0; i < 3; ++i)
            if (out[i]) TSDF_HIP(hipMemcpyAsync(out[i], dout[i], bytes[i], hipMemcpyDeviceToHost, c.stream));
    TSDF_HIP(hipStreamSynchronize(c.stream));
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_icp_linearize(int device, const void* depth, int depth_kind, int Hf, int Wf, const double Kf[9],
                       const double rel_pose[16], const float* model_depth, const float* model_normals, int Hm, int Wm,
                       const double Km[9], const double model_pose[16], const tsdf_icp_params_t* params, double sums[28],
                       int64_t counts[2], uint8_t* code, float* residual, int flags) {
    return linearize_once(nullptr, false, device, depth, depth_kind, nullptr, Hf, Wf, Kf, rel_pose, model_depth, model_normals, nullptr,
                          Hm, Wm, Km, model_pose, params, nullptr, sums, counts, code, residual, nullptr, nullptr, flags);
}

int tsdf_icp_linearize_rgbd(int device, const void* depth, int depth_kind, const uint8_t* color, int Hf, int Wf,
                            const double Kf[9], const double rel_pose[16], const float* model_depth,
                            const float* model_normals, const uint8_t* model_colors, int Hm, int Wm, const double Km[9],
                            const double model_pose[16], const tsdf_icp_params_t* params,
                            const tsdf_icp_color_params_t* color_params, double sums[56], int64_t counts[4], uint8_t* code,
                            float* residual, uint8_t* color_code, float* color_residual, int flags) {
    return linearize_once(nullptr, true, device, depth, depth_kind, color, Hf, Wf, Kf, rel_pose, model_depth, model_normals,
                          model_colors, Hm, Wm, Km, model_pose, params, color_params, sums, counts, code, residual, color_code,
                          color_residual, flags);
}

int tsdf_dense_track(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                     const double pose_guess[16], const tsdf_icp_params_t* params, double z_near, double z_far,
                     double z_step, double out_pose[16], tsdf_track_info_t* info, double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return track(S, cast_dense, h, false, false, depth, depth_kind, nullptr, height, width, K, pose_guess, params, nullptr, z_near,
                 z_far, z_step, out_pose, info, nullptr, trajectory, flags);
}

int tsdf_hash_track(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                    const double pose_guess[16], const tsdf_icp_params_t* params, double z_near, double z_far,
                    double z_step, double out_pose[16], tsdf_track_info_t* info, double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return track(S, cast_hash, h, false, false, depth, depth_kind, nullptr, height, width, K, pose_guess, params, nullptr, z_near,
                 z_far, z_step, out_pose, info, nullptr, trajectory, flags);
}

int tsdf_dense_track_rgbd(tsdf_dense_t* h, const void* depth, int depth_kind, const uint8_t* color, int height, int width,
                          const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                          const tsdf_icp_color_params_t* color_params, double z_near, double z_far, double z_step,
                          double out_pose[16], tsdf_track_info_t* info, tsdf_track_color_info_t* color_info,
                          double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return track(S, cast_dense, h, true, false, depth, depth_kind, color, height, width, K, pose_guess, params, color_params, z_near,
                 z_far, z_step, out_pose, info, color_info, trajectory, flags);
}

int tsdf_hash_track_rgbd(tsdf_hash_t* h, const void* depth, int depth_kind, const uint8_t* color, int height, int width,
                         const double K[9], const double pose_guess[16], const tsdf_icp_params_t* params,
                         const tsdf_icp_color_params_t* color_params, double z_near, double z_far, double z_step,
                         double out_pose[16], tsdf_track_info_t* info, tsdf_track_color_info_t* color_info,
                         double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return track(S, cast_hash, h, true, false, depth, depth_kind, color, height, width, K, pose_guess, params, color_params, z_near,
                 z_far, z_step, out_pose, info, color_info, trajectory, flags);
}

int tsdf_dense_track_sdf(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                         const double pose_guess[16], const tsdf_icp_params_t* params, double out_pose[16],
                         tsdf_track_info_t* info, double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return track(S, nullptr, h, false, true, depth, depth_kind, nullptr, height, width, K, pose_guess, params, nullptr, 0.0, 0.0,
                 0.0, out_pose, info, nullptr, trajectory, flags);
}

int tsdf_hash_track_sdf(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                        const double pose_guess[16], const tsdf_icp_params_t* params, double out_pose[16],
                        tsdf_track_info_t* info, double* trajectory, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return track(S, nullptr, h, false, true, depth, depth_kind, nullptr, height, width, K, pose_guess, params, nullptr, 0.0, 0.0,
                 0.0, out_pose, info, nullptr, trajectory, flags);
}

int tsdf_dense_sdf_linearize(tsdf_dense_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                             const double rel_pose[16], const double pose_guess[16], const tsdf_icp_params_t* params,
                             double sums[28], int64_t counts[2], uint8_t* code, float* residual, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return linearize_once(&S, false, 0, depth, depth_kind, nullptr, height, width, K, rel_pose, nullptr, nullptr, nullptr, 0, 0,
                          K, pose_guess, params, nullptr, sums, counts, code, residual, nullptr, nullptr, flags);
}

int tsdf_hash_sdf_linearize(tsdf_hash_t* h, const void* depth, int depth_kind, int height, int width, const double K[9],
                            const double rel_pose[16], const double pose_guess[16], const tsdf_icp_params_t* params,
                            double sums[28], int64_t counts[2], uint8_t* code, float* residual, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return linearize_once(&S, false, 0, depth, depth_kind, nullptr, height, width, K, rel_pose, nullptr, nullptr, nullptr, 0, 0,
                          K, pose_guess, params, nullptr, sums, counts, code, residual, nullptr, nullptr, flags);
}

int tsdf_dense_sample(tsdf_dense_t* h, const double* points, int64_t n, float* sdf, float* grad, uint8_t* code, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(dense_ray_source(h, &S));
    return sample(S, points, n, sdf, grad, code, flags);
}

int tsdf_hash_sample(tsdf_hash_t* h, const double* points, int64_t n, float* sdf, float* grad, uint8_t* code, int flags) {
    if (!h) return set_error(TSDF_E_ARG, "null handle");
    RaySource S;
    TSDF_TRY(hash_ray_source(h, &S));
    return sample(S, points, n, sdf, grad, code, flags);
}

int tsdf_track_last_prep_ms(double* ms) {
    if (!ms) return set_error(TSDF_E_ARG, "null pointer");
    *ms = g_track_prep_ms;
    return TSDF_OK;
}

int tsdf_track_last_ms(double ms[5], int* iterations) {
    if (!ms || !iterations) return set_error(TSDF_E_ARG, "null pointer");
    for (int i = 0; i < 5; ++i) ms[i] = g_track_ms[i];
    *iterations = (int)g_track_ms[5];
    return TSDF_OK;
}

}  // extern "C"
