/* tsdf_pixel.h -- host side of the integrate's fast pixel path: the per-frame constants that
 * prepare_batch (tsdf_common.hip) puts into Frame, in plain C so that tools/check_pixel_fixed.c
 * checks the very functions the library runs.  The device side is project_part (tsdf_device.h).
 *
 * The fast path computes a pixel coordinate as u = X*rz + c with X = x*f up to the folding error
 * (fold_bound) and rz the bare v_rcp_f64 (2^-24.4 relative, tools/gpu/rcp_probe.hip), and delivers
 * it in 16.16 fixed point: the FMA's addend is not c but
 *     C = c + 0.5 + m*2^-16 + 1.5*2^36,
 * so t = fma(X, rz, C) lies in [2^36, 2^37), where an f64's ulp is 2^-16: the FMA's one rounding
 * lands on that grid, and the low dword of t is n mod 2^32 with n = round((u + 0.5)*2^16) + m.
 * Its upper half is floor(u + 0.5) mod 65536 and its lower half the distance past the rounding
 * boundary below, plus m, in units of 2^-16.  A coordinate is "fine" iff that lower half is >= 2m:
 * then u lies at least m*2^-16 - 2^-17 - |C's own rounding error| from both boundaries, and the
 * upper half is rint(u) (an exact tie is inside the margin, so half-to-even against
 * floor(u + 0.5) never matters).  Every other step is redone with the reference's division. */
#ifndef TSDF_PIXEL_H
#define TSDF_PIXEL_H
#include <limits.h>
#include <math.h>
#include <string.h>

/* The fast path's pixel error is < |u - c| * 2^-24.3 (the bare reciprocal), and wherever the
 * boundary test matters |u - c| <= max(W, H) + max(|cx|, |cy|) -- a step closer than this margin to
 * a rounding boundary takes the exact path.  1e-4 px covers images up to ~1000 px; larger ones
 * scale it. */
static inline double frame_margin(int W, int H, double cx, double cy) {
    const double span = (double)(W > H ? W : H) + fmax(fabs(cx), fabs(cy));
    return fmax(1e-4, 1e-7 * span);
}

/* |X| <= f * (|T0| X + |T1| Y + |T2| Z + |T3|) for world coordinates bounded by (X, Y, Z): the
 * bound of the x (out[0]) and y (out[1]) numerators (|f|: a negative focal length mirrors the image). */
static inline void fold_rows(const double* T, double fx, double fy, const double wmax[3], double out[2]) {
    for (int r = 0; r < 2; ++r) {
        const double* t = T + 4 * r;
        out[r] = fabs(r == 0 ? fx : fy) *
                 (fabs(t[0]) * wmax[0] + fabs(t[1]) * wmax[1] + fabs(t[2]) * wmax[2] + fabs(t[3]));
    }
}

/* The fast path folds fx, fy and the translation into its rows: X = fma(Tf2, pz, fma(Tf1, py,
 * fma(Tf0, px, Tf3))) with Tf = RN(T * f) -- four roundings, each within 2^-53 of its operands'
 * magnitudes, so |X - f * x| <= E = 8 * 2^-53 * (the bound of fold_rows) (a factor 2 of slack).
 * Its pixel error E / z stays below a quarter of the margin where z > zmin = 4 E / margin.
 * Returns zmin. */
static inline double fold_bound(const double* T, double fx, double fy, const double wmax[3], double margin) {
    double b[2];
    fold_rows(T, fx, fy, wmax, b);
    return 4.0 * (8.0 * 0x1p-53 * fmax(b[0], b[1])) / margin;
}

/* A frame from which the reference updates no voxel whatever the depth image holds:
 *  - a non-finite entry in rows 0..2 of inv(cam_pose) or in fx, fy, cx, cy: the entry reaches every
 *    voxel's x, y or z (0 * inf and inf - inf are NaN), a non-finite x or y gives a non-finite u or v,
 *    whose np.rint(.).astype(int) is the most negative integer and fails 0 <= u; z = NaN or -inf fails
 *    z > 0, and z = +inf fails depth - z >= -trunc for every depth (inf - inf is NaN);
 *  - a zero third row with T[11] <= 0: z is that number for every voxel and fails z > 0.
 * prepare_batch integrates such a frame as the zero matrix and culls it outright. */
static inline int frame_is_dead(const double* T, double fx, double fy, double cx, double cy) {
    int finite = isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy);
    for (int r = 0; r < 12; ++r) finite = finite && isfinite(T[r]);
    if (!finite) return 1;
    return T[8] == 0.0 && T[9] == 0.0 && T[10] == 0.0 && !(T[11] > 0.0);
}

#define TSDF_PIXEL_BIAS 0x1.8p36 /* 1.5 * 2^36 */

typedef struct {
    double Cx, Cy;    /* the pixel FMAs' addends */
    unsigned mm;      /* (2*my) << 16 | 2*mx: a coordinate is fine iff its low half is >= 2m */
    unsigned whm1;    /* (H - 1) << 16 | (W - 1) */
    unsigned wmul;    /* W << 16 | 1: pixel = dot2((iv, iu), (W, 1)) */
    int zmin_hi;      /* fast path iff hi dword of z > zmin_hi (signed); INT_MAX: never */
    int mx, my;       /* (for the checker) */
    double zmin;      /* (for the checker) the depth limit behind zmin_hi; +inf: never */
} PixelFixed;

/* One axis: the addend C and the margin count m, the smallest integer with
 * m*2^-16 - 2^-17 - |C's error| >= margin.  c is an f32 value and need not lie on the 2^-16 grid:
 * C is rounded onto it, and that error -- taken exactly -- is added to the margin. */
static inline int pixel_axis(double c, double margin, double* C) {
    const double C0 = (c + 0.5) + TSDF_PIXEL_BIAS;
    /* C0 - bias is exact (a multiple of 2^-16 below 2^35), and so are the next two steps up to a
     * relative 2^-53 of a difference below 2^-16 */
    const double err = fabs(((C0 - TSDF_PIXEL_BIAS) - 0.5) - c);
    double m = ceil((margin + 0x1p-17 + err) * 65536.0);
    while (m * 0x1p-16 - 0x1p-17 - err < margin) m += 1.0;
    *C = C0 + m * 0x1p-16; /* exact: both on the grid */
    return m < 32768.0 ? (int)m : -1;
}

/* The frame's constants.  T: rows 0..2 of inv(cam_pose); wmax: bounds of the volume's world
 * coordinates.  The 16-bit pixel field must not alias -- a voxel far outside the image must not
 * wrap into it -- so the fast path needs |u| + 1 < 65536 - W (and the y analogue): zmin is raised
 * to numerator bound / (65536 - W - |c| - 2).  Where that cannot hold (an image side above 16384,
 * a huge principal point), or where anything is not finite, no step takes the fast path. */
static inline PixelFixed pixel_fixed(const double* T, double fx, double fy, double cx, double cy, int W,
                                     int H, const double wmax[3]) {
    PixelFixed p;
    memset(&p, 0, sizeof p);
    p.zmin_hi = INT_MAX;
    p.zmin = INFINITY;
    int finite = isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy);
    for (int r = 0; r < 12; ++r) finite = finite && isfinite(T[r]);
    for (int j = 0; j < 4; ++j) finite = finite && isfinite(T[j] * fx) && isfinite(T[4 + j] * fy);
    if (!finite || W < 1 || H < 1 || W > 16384 || H > 16384) return p;
    const double margin = frame_margin(W, H, cx, cy);
    double b[2];
    fold_rows(T, fx, fy, wmax, b);
    const double denx = 65536.0 - (double)W - fabs(cx) - 2.0, deny = 65536.0 - (double)H - fabs(cy) - 2.0;
    if (!(denx >= 1.0) || !(deny >= 1.0)) return p;
    /* (at least 2^-1000: rows 0 and 1 may be zero -- fx == 0, the zero matrix -- and the bounds with
     * them; 1 / z must stay finite, or the numerator's exact 0 times an infinite reciprocal is NaN) */
    const double zmin = fmax(fmax(fold_bound(T, fx, fy, wmax, margin), fmax(b[0] / denx, b[1] / deny)), 0x1p-1000);
    double Cx, Cy;
    const int mx = pixel_axis(cx, margin, &Cx), my = pixel_axis(cy, margin, &Cy);
    if (mx < 0 || my < 0 || !isfinite(zmin) || !(zmin < 1e300)) return p;
    long long bits;
    memcpy(&bits, &zmin, sizeof bits);
    p.zmin_hi = (int)(bits >> 32) + 1; /* rounded up: hi(z) > zmin_hi implies z > zmin */
    p.zmin = zmin;
    p.Cx = Cx;
    p.Cy = Cy;
    p.mx = mx;
    p.my = my;
    p.mm = ((unsigned)(2 * my) << 16) | (unsigned)(2 * mx);
    p.whm1 = ((unsigned)(H - 1) << 16) | (unsigned)(W - 1);
    p.wmul = ((unsigned)W << 16) | 1u;
    return p;
}

/* Texels (DK == 2): the prep writes an invalid depth (0 after the optional 65535 masking) as
 * this dword, and the integrate converts the texel's depth as a signed integer: about -2.1e6 m,
 * which fails depth - z >= -trunc for every z > 0 while trunc is below kTexelMaxTrunc -- so the
 * texel route needs no depth > 0 test.  Handles with a larger trunc do not take the route. */
#define TSDF_TEXEL_INVALID 0x80000000u
#define TSDF_TEXEL_MAX_TRUNC 1.0e6
/* the kernels' u16 millimetres -> metres (depth_m), here on the texel's signed dword */
static inline double texel_depth_m(int raw) {
    const double m = (double)raw;
    return fma(m, 0.001, m * -2.0858186326137145e-20);
}

#endif
