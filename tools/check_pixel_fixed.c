/* Checks the integrate's 16.16 fixed-point pixel path (project_part, tsdf_device.h) against the
 * reference's rint((x*fx)/z + cx), with the host functions the library itself runs (pixel_fixed,
 * tsdf_pixel.h).  The fast path is emulated as the kernel computes it: t = fma(X, rz, C) with
 * X = x*fx off by up to the folding error E (fold_bound) and rz = (1/z)(1 + e), |e| <= 2^-24.4 (the
 * bound of v_rcp_f64, tools/gpu/rcp_probe.hip); a step is fine iff z > zmin (by the high dword)
 * and the low half of t's low dword is >= 2m; its pixel is the high half.
 *   (a) 1e7 random (X, z, c) from the kernels' ranges, over image sides up to 16384 and principal
 *       points on and off the 2^-16 grid, negative and large: every fine step's pixel is inside the
 *       image iff the reference's is, and equals it there and wherever |u - c| is within the
 *       span frame_margin is made for (farther out both are outside, which is all the kernel asks);
 *   (b) the same on values within +-3e-4 px of every half-integer of the image and its surround;
 *   (c) no step with z > zmin aliases: t stays in [2^36, 2^37) and |u| + 1 < 65536 - side at the
 *       extreme numerators and the smallest z the high-dword test passes;
 *   (d) a non-finite row, intrinsic or an oversized image gives zmin_hi = INT_MAX;
 *   (e) the texel's invalid-depth sentinel fails the truncation test for the smallest positive z
 *       and the largest trunc of the texel route, and valid u16 depths convert as before.
 *   (hostile) hostile rows and intrinsics (tests/hostile_pose.py): NaN, infinities and a translation whose
 *       T * f overflows give zmin_hi = INT_MAX and, where an entry is non-finite, frame_is_dead; the
 *       finite ones -- negative, zero, tiny and huge focal lengths, scaled, sheared and mirrored rows,
 *       translations of 1e30, 1e39 and 1e300, a zero third row, the zero matrix -- either take no fast
 *       path or return a zmin above which, with the numerator bound taken here from |f| and |T|, no
 *       pixel aliases and every fine step's pixel is the reference's;
 * Prints "pixel_fixed <case> checked N fine F bad B" per case (expected B = 0); the last case is
 * named "hostile".
 * Build: gcc -O2 -ffp-contract=off -I union-thesis-slam_amd/csrc tools/check_pixel_fixed.c -lm. */
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include "tsdf_pixel.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return s;
}
static double urand(void) { return (double)(next() >> 11) * 0x1.0p-53; } /* [0,1) */
static double srand1(void) { return 2.0 * urand() - 1.0; }               /* [-1,1) */

typedef struct {
    PixelFixed p;
    double c, C, f, bound, E, span;
    int side, m;
} Axis;

static int hi_dword(double z) {
    long long b;
    memcpy(&b, &z, sizeof b);
    return (int)(b >> 32);
}

/* one step: 1 if the fixed-point path calls it fine; *bad set on a contradiction */
static int step(const Axis* a, double xf, double z, double rcp_err, long* bad) {
    if (!(hi_dword(z) > a->p.zmin_hi)) return 0;
    volatile double q = xf / z; /* the reference: (x*fx)/z + c, rounded */
    volatile double u = q + a->c;
    const double ref = rint(u);
    const double X = xf + a->E * srand1();
    const double rz = (1.0 / z) * (1.0 + rcp_err);
    const double t = fma(X, rz, a->C);
    if (!(t >= 0x1p36 && t < 0x1p37)) { ++*bad; return 0; } /* (c): the 2^-16 grid */
    unsigned long long b;
    memcpy(&b, &t, sizeof b);
    const unsigned lo = (unsigned)b & 0xFFFFu, hi = ((unsigned)b >> 16) & 0xFFFFu;
    if (lo < 2u * (unsigned)a->m) return 0;
    const int in_fast = hi < (unsigned)a->side, in_ref = ref >= 0.0 && ref < (double)a->side;
    if (in_fast != in_ref) ++*bad;
    else if ((in_ref || fabs(u - a->c) <= a->span + 2.0) && (double)hi != (ref < 0.0 ? ref + 65536.0 : ref)) ++*bad;
    return 1;
}

static int setup(Axis* a, int axis, int W, int H, double fx, double fy, double cx, double cy, double t3, double wm) {
    /* a camera looking along +z from inside the volume, rotated a little so every row is full */
    const double T[12] = {0.96, -0.2, 0.196, axis == 0 ? t3 : -1.0, 0.2, 0.9798, 0.02, axis == 1 ? t3 : 0.5, -0.196, 0.02, 0.98, -0.3};
    const double wmax[3] = {wm, wm, wm};
    a->p = pixel_fixed(T, fx, fy, cx, cy, W, H, wmax);
    if (a->p.zmin_hi == INT_MAX) return 0;
    double b[2];
    fold_rows(T, fx, fy, wmax, b);
    a->c = axis ? cy : cx;
    a->C = axis ? a->p.Cy : a->p.Cx;
    a->f = axis ? fy : fx;
    a->side = axis ? H : W;
    a->m = axis ? a->p.my : a->p.mx;
    a->bound = b[axis];
    a->E = 8.0 * 0x1p-53 * b[axis];
    a->span = (double)(W > H ? W : H) + fmax(fabs(cx), fabs(cy));
    return 1;
}

/* (hostile): one frame.  expect_off: 1 the fast path must be off, 0 either; dead: frame_is_dead's answer. */
static void hostile(const double* T, double fx, double fy, double cx, double cy, int expect_off, int dead, long* n,
                    long* fine, long* bad) {
    const int W = 80, H = 60;
    const double wmax[3] = {2.25, 1.75, 2.25};
    const double rcp_max = exp2(-24.4);
    const long bad0 = *bad;
    ++*n;
    if (frame_is_dead(T, fx, fy, cx, cy) != dead) ++*bad;
    const PixelFixed p = pixel_fixed(T, fx, fy, cx, cy, W, H, wmax);
    if (p.zmin_hi != INT_MAX && expect_off) ++*bad;
    if (p.zmin_hi != INT_MAX && (!(p.zmin >= 0.0) || !isfinite(p.zmin))) ++*bad;
    if (p.zmin_hi == INT_MAX || *bad != bad0) {
        if (*bad != bad0) fprintf(stderr, "hostile: f %g %g c %g %g T3 %g T11 %g: zmin %g\n", fx, fy, cx, cy, T[3], T[11], p.zmin);
        return;
    }
    long long zb = ((long long)p.zmin_hi + 1) << 32;
    double zmin_q;
    memcpy(&zmin_q, &zb, sizeof zmin_q);
    if (!(zmin_q > p.zmin)) ++*bad;
    for (int axis = 0; axis < 2; ++axis) {
        const double* t = T + 4 * axis;
        Axis a;
        a.p = p;
        a.c = axis ? cy : cx;
        a.C = axis ? p.Cy : p.Cx;
        a.f = axis ? fy : fx;
        a.side = axis ? H : W;
        a.m = axis ? p.my : p.mx;
        /* the numerator's bound, from |f| and |T| (not through fold_rows) */
        a.bound = fabs(a.f) * (fabs(t[0]) * wmax[0] + fabs(t[1]) * wmax[1] + fabs(t[2]) * wmax[2] + fabs(t[3]));
        a.E = 8.0 * 0x1p-53 * a.bound;
        a.span = (double)(W > H ? W : H) + fmax(fabs(cx), fabs(cy));
        for (int j = 0; j < 4000; ++j, ++*n) {
            const double z = zmin_q * (1.0 + (j & 3 ? 0.0 : 0.5 * urand()));
            const double xf = (j & 1 ? 1.0 : -1.0) * a.bound * (j & 2 ? 1.0 : 1.0 - 0.01 * urand());
            if (!(fabs(xf / z * (1.0 + rcp_max)) + fabs(a.c) + 1.0 < 65536.0 - a.side)) ++*bad;
            *fine += step(&a, xf, z, j & 4 ? rcp_max : -rcp_max, bad);
        }
        const double zhi = fmax(64.0, 1e6 * zmin_q), lz = log(zhi / zmin_q);
        for (int j = 0; j < 20000; ++j, ++*n) {
            const double z = zmin_q * exp(lz * urand());
            double xf = (j & 1) ? ((3.0 * urand() - 1.0) * a.side - a.c) * z : a.bound * srand1();
            if (fabs(xf) > a.bound) xf = a.bound * srand1();
            *fine += step(&a, xf, z, rcp_max * srand1(), bad);
        }
    }
    if (*bad != bad0) fprintf(stderr, "hostile: f %g %g c %g %g T3 %g T11 %g: zmin %g, %ld bad\n", fx, fy, cx, cy, T[3], T[11], p.zmin, *bad - bad0);
}

int main(void) {
    const double rcp_max = exp2(-24.4); /* the probe's bound on v_rcp_f64 */
    const int sides[][2] = {{640, 480}, {97, 61}, {1280, 1024}, {16384, 16384}, {4000, 3}, {61, 97}, {1, 1}};
    const float cs[][2] = {{319.5f, 239.5f}, {-40.3f, 200.7f}, {30000.123f, -20000.77f}, {0.1f, 1e-9f},
                           {8191.51f, 8000.0f}, {-3.0e4f, 100.49999f}, {48.000004f, 30.3333f}};
    const int ns = sizeof(sides) / sizeof(sides[0]), nc = sizeof(cs) / sizeof(cs[0]);
    long bad_a = 0, n_a = 0, fine_a = 0, bad_b = 0, n_b = 0, fine_b = 0, bad_c = 0, n_c = 0, fine_c = 0;
    int setups = 0, m8 = 0;
    for (int si = 0; si < ns; ++si)
        for (int ci = 0; ci < nc; ++ci)
            for (int axis = 0; axis < 2; ++axis) {
                Axis a;
                const double fx = (double)525.0f, fy = (double)(si & 1 ? 1050.25f : 525.0f);
                const double t3 = ci & 1 ? -7.5 : 3.25, wm = si & 1 ? 41.0 : 11.24;
                if (!setup(&a, axis, sides[si][0], sides[si][1], fx, fy, (double)cs[ci][0], (double)cs[ci][1], t3, wm)) {
                    ++bad_a; /* every one of these frames has a fast path */
                    continue;
                }
                ++setups;
                if (si == 0 && ci == 0 && a.m == 8) ++m8;
                /* the margin the fine test grants: m*2^-16 - 2^-17 - |C's error| >= frame_margin */
                const double errC = fabs(((a.C - TSDF_PIXEL_BIAS) - 0.5 - a.m * 0x1p-16) - a.c);
                if (a.m * 0x1p-16 - 0x1p-17 - errC < frame_margin(sides[si][0], sides[si][1], (double)cs[ci][0], (double)cs[ci][1])) ++bad_a;
                if (!(a.p.zmin > 0.0)) ++bad_a;
                const double zlo = a.p.zmin, lz = log(64.0 / zlo);
                /* (a) random: half aimed at the image and its surround, half over the whole range */
                const long na = 10000000 / (ns * nc * 2) + 1;
                for (long i = 0; i < na; ++i, ++n_a) {
                    const double z = zlo * exp(lz * urand());
                    double xf;
                    if (i & 1) xf = ((3.0 * urand() - 1.0) * a.side - a.c) * z;
                    else xf = a.bound * srand1();
                    if (fabs(xf) > a.bound) xf = a.bound * srand1();
                    const double e = (i % 7 == 0) ? rcp_max : (i % 7 == 1) ? -rcp_max : rcp_max * srand1();
                    fine_a += step(&a, xf, z, e, &bad_a);
                }
                /* (b) within +-3e-4 px of every half-integer from -2.5 to side + 1.5 */
                const int stride = a.side > 4096 ? 7 : 1;
                for (int b = -3; b <= a.side + 1; b += stride)
                    for (int j = 0; j < (a.side > 1000 ? 6 : 60); ++j, ++n_b) {
                        const double z = zlo * exp(lz * urand());
                        const double d = j == 0 ? 0.0 : 3e-4 * srand1() * (j & 1 ? 1.0 : 0.4);
                        const double xf = (((double)b + 0.5 + d) - a.c) * z;
                        if (fabs(xf) > a.bound) continue;
                        const double e = (j % 5 == 0) ? rcp_max : (j % 5 == 1) ? -rcp_max : rcp_max * srand1();
                        fine_b += step(&a, xf, z, e, &bad_b);
                    }
                /* (c) the extreme numerators at the smallest z the high-dword test passes */
                long long zb = ((long long)a.p.zmin_hi + 1) << 32;
                double zmin_q;
                memcpy(&zmin_q, &zb, sizeof zmin_q);
                if (!(zmin_q > a.p.zmin)) ++bad_c;
                for (int j = 0; j < 20000; ++j, ++n_c) {
                    const double z = zmin_q * (1.0 + (j & 3 ? 0.0 : 0.5 * urand()));
                    const double xf = (j & 1 ? 1.0 : -1.0) * a.bound * (j & 2 ? 1.0 : 1.0 - 0.01 * urand());
                    if (!(fabs(xf / z * (1.0 + rcp_max)) + fabs(a.c) + 1.0 < 65536.0 - a.side)) ++bad_c;
                    fine_c += step(&a, xf, z, j & 4 ? rcp_max : -rcp_max, &bad_c);
                }
            }
    if (!m8) ++bad_a; /* 640x480, cx = 319.5: m = 8 */
    printf("pixel_fixed a checked %ld fine %ld bad %ld (setups %d)\n", n_a, fine_a, bad_a, setups);
    printf("pixel_fixed b checked %ld fine %ld bad %ld\n", n_b, fine_b, bad_b);
    printf("pixel_fixed c checked %ld fine %ld bad %ld\n", n_c, fine_c, bad_c);

    long bad_d = 0, n_d = 0;
    {
        const double wmax[3] = {11.24, 11.24, 11.24};
        const double T0[12] = {1, 0, 0, -5, 0, 1, 0, -5, 0, 0, 1, -5};
        const double nf[3] = {NAN, INFINITY, -INFINITY};
        if (pixel_fixed(T0, 525, 525, 319.5, 239.5, 640, 480, wmax).zmin_hi == INT_MAX) ++bad_d; /* the control */
        for (int r = 0; r < 12; ++r)
            for (int k = 0; k < 3; ++k, ++n_d) {
                double T[12];
                memcpy(T, T0, sizeof T);
                T[r] = nf[k];
                bad_d += pixel_fixed(T, 525, 525, 319.5, 239.5, 640, 480, wmax).zmin_hi != INT_MAX;
            }
        for (int k = 0; k < 3; ++k, n_d += 4) {
            bad_d += pixel_fixed(T0, nf[k], 525, 319.5, 239.5, 640, 480, wmax).zmin_hi != INT_MAX;
            bad_d += pixel_fixed(T0, 525, nf[k], 319.5, 239.5, 640, 480, wmax).zmin_hi != INT_MAX;
            bad_d += pixel_fixed(T0, 525, 525, nf[k], 239.5, 640, 480, wmax).zmin_hi != INT_MAX;
            bad_d += pixel_fixed(T0, 525, 525, 319.5, nf[k], 640, 480, wmax).zmin_hi != INT_MAX;
        }
        /* oversized images and principal points that leave no room in the 16-bit field */
        bad_d += pixel_fixed(T0, 525, 525, 319.5, 239.5, 40000, 2, wmax).zmin_hi != INT_MAX;
        bad_d += pixel_fixed(T0, 525, 525, 319.5, 239.5, 2, 16385, wmax).zmin_hi != INT_MAX;
        bad_d += pixel_fixed(T0, 525, 525, 60000.0, 239.5, 16384, 480, wmax).zmin_hi != INT_MAX;
        bad_d += pixel_fixed(T0, 525, 525, 319.5, -65100.0, 640, 480, wmax).zmin_hi != INT_MAX;
        n_d += 4;
    }
    printf("pixel_fixed d checked %ld bad %ld\n", n_d, bad_d);

    long bad_e = 0, n_e = 0;
    {
        const double trunc = nextafter(TSDF_TEXEL_MAX_TRUNC, 0.0);
        const double zs[] = {0x1p-1074, DBL_MIN, 1e-6, 0.16, 100.0};
        const double dep = texel_depth_m((int)TSDF_TEXEL_INVALID);
        for (unsigned k = 0; k < sizeof(zs) / sizeof(zs[0]); ++k, ++n_e) {
            volatile double diff = dep - zs[k];
            bad_e += diff >= -trunc;
        }
        for (unsigned d = 1; d < 65536; ++d, ++n_e) { /* valid depths: the signed conversion changes nothing */
            const double m = (double)d;
            bad_e += texel_depth_m((int)d) != fma(m, 0.001, m * -2.0858186326137145e-20);
        }
    }
    printf("pixel_fixed e checked %ld bad %ld\n", n_e, bad_e);
    long bad_f = 0, n_f = 0, fine_f = 0;
    {
        /* the good rows of tests/hostile_pose.py, frame 0 (a 6 degree turn about y, 2 degrees about x) */
        const double G[12] = {0.9945218953682733, 0.0, -0.10452846326765347, -0.045,
                              0.0036479567, 0.9993908270190958, 0.0347081937, -0.02,
                              0.1044647897, -0.03489949670250097, 0.9939160672, 0.6};
        const double fx = 60.0, fy = 62.0, cx = 39.5, cy = 29.5;
        const double nf[3] = {NAN, INFINITY, -INFINITY};
        hostile(G, fx, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        if (pixel_fixed(G, fx, fy, cx, cy, 80, 60, (const double[3]){2.25, 1.75, 2.25}).zmin_hi == INT_MAX) ++bad_f; /* the control */
        double T[12];
        for (int k = 0; k < 3; ++k) { /* NaN / +-inf: everywhere, then in each translation entry alone */
            for (int r = 0; r < 12; ++r) T[r] = nf[k];
            hostile(T, fx, fy, cx, cy, 1, 1, &n_f, &fine_f, &bad_f);
            for (int r = 3; r < 12; r += 4) {
                memcpy(T, G, sizeof T);
                T[r] = nf[k];
                hostile(T, fx, fy, cx, cy, 1, 1, &n_f, &fine_f, &bad_f);
            }
            hostile(G, nf[k], fy, cx, cy, 1, 1, &n_f, &fine_f, &bad_f);
            hostile(G, fx, nf[k], cx, cy, 1, 1, &n_f, &fine_f, &bad_f);
            hostile(G, fx, fy, nf[k], cy, 1, 1, &n_f, &fine_f, &bad_f);
            hostile(G, fx, fy, cx, nf[k], 1, 1, &n_f, &fine_f, &bad_f);
        }
        const double huge[4] = {1e30, 1e39, 1e300, 1e307};
        for (int k = 0; k < 4; ++k) { /* finite rows; at 1e307 T * f overflows: no fast path */
            memcpy(T, G, sizeof T);
            T[3] = huge[k]; T[7] = -huge[k]; T[11] = huge[k];
            hostile(T, fx, fy, cx, cy, k == 3, 0, &n_f, &fine_f, &bad_f);
        }
        memcpy(T, G, sizeof T);
        T[8] = T[9] = T[10] = T[11] = 0.0; /* z == 0 everywhere */
        hostile(T, fx, fy, cx, cy, 0, 1, &n_f, &fine_f, &bad_f);
        memset(T, 0, sizeof T);
        hostile(T, fx, fy, cx, cy, 0, 1, &n_f, &fine_f, &bad_f);
        T[11] = 1.0; /* (a zero rotation in front of the camera is a frame like any other) */
        hostile(T, fx, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        /* non-rigid rows A * G about (0, 0, 1): scales, a shear, a mirror */
        const double A[5][9] = {{2, 0, 0, 0, 2, 0, 0, 0, 2}, {0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5}, {1, 0, 0, 0, 2, 0, 0, 0, 0.5},
                                {1, 0.35, 0, 0, 1, 0.25, 0.2, 0, 1}, {-1, 0, 0, 0, 1, 0, 0, 0, 1}};
        for (int k = 0; k < 5; ++k) {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c)
                    T[4 * r + c] = A[k][3 * r] * G[c] + A[k][3 * r + 1] * G[4 + c] + A[k][3 * r + 2] * G[8 + c] +
                                   (c == 3 ? (r == 2 ? 1.0 : 0.0) - A[k][3 * r + 2] : 0.0);
            hostile(T, fx, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        }
        /* intrinsics */
        hostile(G, -fx, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, fx, -fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, -fx, -fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, -6000.0, -6200.0, cx, cy, 0, 0, &n_f, &fine_f, &bad_f); /* (negative and large: the bound matters) */
        hostile(G, 0.0, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, (double)1e-30f, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, (double)1e30f, fy, cx, cy, 0, 0, &n_f, &fine_f, &bad_f);
        hostile(G, fx, fy, 70000.0, cy, 1, 0, &n_f, &fine_f, &bad_f);
        hostile(G, fx, fy, (double)1e30f, cy, 1, 0, &n_f, &fine_f, &bad_f);
    }
    printf("pixel_fixed hostile checked %ld fine %ld bad %ld\n", n_f, fine_f, bad_f);
    return (bad_a | bad_b | bad_c | bad_d | bad_e | bad_f) != 0;
}
