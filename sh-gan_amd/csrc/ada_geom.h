// The coordinate arithmetic of the ADA geometry, shared by every kernel of csrc/ada.hip and -- compiled as plain host C++ -- by the
// brute-force check of the gather window (tests/test_ada_gather_cpu.py): the sym6 taps, the reflect fold, the affine sample coordinate,
// the per-axis resampling weights of the forward, and the candidate window of the gather-form adjoint.  The forward, the scatter adjoint
// and the gather adjoint must take the SAME decision (floor, clamp) on every sample, so all of them call the functions of this file.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define ADA_HD __host__ __device__ __forceinline__
#define ADA_CONST __device__ constexpr
#else
#include <algorithm>
#define ADA_HD inline
#define ADA_CONST constexpr
#endif

namespace {
#if !defined(__HIPCC__)
using std::max;
using std::min;
#endif

// sym6 low-pass (an orthonormal wavelet filter: the taps sum to sqrt 2), normalised to sum 1 as ada.py's Hz_geom
constexpr double ADA_SYM6[12] = {0.015404109327027373,  0.0034907120842174702, -0.11799011114819057,  -0.048311742585633,
                                 0.4910559419267466,    0.787641141030194,     0.3379294217276218,    -0.07263752278646252,
                                 -0.021060292512300564, 0.04472490177066578,   0.0017677118642428036, -0.007800708325034148};
constexpr double ada_sym6_sum() {
    double s = 0.0;
    for (int i = 0; i < 12; ++i) s += ADA_SYM6[i];
    return s;
}
#define ADA_TAP(i) (float)(ADA_SYM6[i] / ada_sym6_sum())
ADA_CONST float ADA_F[12] = {ADA_TAP(0), ADA_TAP(1), ADA_TAP(2), ADA_TAP(3), ADA_TAP(4),  ADA_TAP(5),
                             ADA_TAP(6), ADA_TAP(7), ADA_TAP(8), ADA_TAP(9), ADA_TAP(10), ADA_TAP(11)};

// ------------------------------------------------------------------------------------------------ the resampling weights of one axis
struct AdaAxis {
    int lo;          // first padded index
    int idx[7];      // source index of padded index lo + k (reflected, clamped into the image)
    float w[7];
};

ADA_HD int ada_reflect(int i, int m0, int n) {
    int r = i - m0;
    r = r < 0 ? -r : r;
    r = r > n - 1 ? 2 * (n - 1) - r : r;
    return min(max(r, 0), n - 1);
}

// upsampled-pixel coordinate of sample index j (the other axis' index is jo): a, b = the row of G_inv for this axis (own, other), t its
// translation, n / no the sizes of this and the other axis, m0 / m1 this axis' margins
ADA_HD double ada_coord(int j, int jo, float a, float b, float t, int n, int no, int m0, int m1) {
    const double uo = 0.5 * (double)(j - n - 5), uu = 0.5 * (double)(jo - no - 5);
    const double np = (double)(n + m0 + m1);
    double c = 2.0 * ((double)a * uo + (double)b * uu + (double)t) + (double)(m0 - m1) + np - 1.0;
    return fmin(fmax(c, -4.0), 2.0 * np + 4.0);           // (a NaN ends at -4: every weight zero)
}

ADA_HD void ada_axis(double c, int n, int m0, int m1, AdaAxis& ax) {
    constexpr float A[7] = {ADA_F[11], ADA_F[9], ADA_F[7], ADA_F[5], ADA_F[3], ADA_F[1], 0.f};      // f[11 - 2k]
    constexpr float B[7] = {ADA_F[10], ADA_F[8], ADA_F[6], ADA_F[4], ADA_F[2], ADA_F[0], 0.f};      // f[10 - 2k]
    constexpr float BS[7] = {0.f, ADA_F[10], ADA_F[8], ADA_F[6], ADA_F[4], ADA_F[2], ADA_F[0]};     // f[12 - 2k]
    const int np = n + m0 + m1, nu = 2 * np;
    const double fl = floor(c);
    const float t = (float)(c - fl);
    const int x0 = (int)fl;
    const float b0 = (x0 >= 0 && x0 < nu) ? 2.f * (1.f - t) : 0.f;
    const float b1 = (x0 + 1 >= 0 && x0 + 1 < nu) ? 2.f * t : 0.f;
    const bool odd = (x0 & 1) != 0;
    ax.lo = (x0 - 5) >> 1;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int i = ax.lo + k;
        const float w = b0 * (odd ? B[k] : A[k]) + b1 * (odd ? A[k] : BS[k]);
        ax.w[k] = (i >= 0 && i < np) ? w : 0.f;
        ax.idx[k] = ada_reflect(i, m0, n);
    }
}

struct AdaGeo {
    float g[6];
    int mx0, my0, mx1, my1;
};
ADA_HD AdaGeo ada_geo(const float* __restrict__ G, const int* __restrict__ margins, int n, int H, int W) {
    AdaGeo q;
#pragma unroll
    for (int i = 0; i < 6; ++i) q.g[i] = G[(long)n * 9 + i];
    q.mx0 = min(max(margins[0], 0), W - 1), q.my0 = min(max(margins[1], 0), H - 1);
    q.mx1 = min(max(margins[2], 0), W - 1), q.my1 = min(max(margins[3], 0), H - 1);
    return q;
}

// ------------------------------------------------------------------------------------------------ the window of the gather-form adjoint
// The sample coordinate is affine in the sample index q = (jx, jy): (cx, cy) = L q + k with L = [[g0, g1], [g3, g4]].  An upsampled pixel
// v = (vx, vy) is touched by the samples with cx in [vx - 1, vx + 1) and cy in [vy - 1, vy + 1); their indices lie in the bounding box of
// M (box(v) - k), M = L^-1: centre M (v - k), half extents hx = |M00| + |M01| and hy = |M10| + |M11|.  The gather route takes a sample
// only when hx, hy <= ADA_GATHER_HMAX (24 covers a 16-fold magnification at any rotation; the parameter kernel with |normal draw| <= 6
// gives at most 2^1.2 * 2^1.2 = 5.3 per axis) and when the magnitudes that enter a coordinate, |k| + |L| (2 (W + H) + 20), stay below
// ADA_GATHER_MAG = 2^24 (a NaN or an infinity fails the comparison): the candidate count per pixel is then at most (2 * 24 + 1)^2, and
// the float64 rounding of a coordinate (<= 2^-52 * a few * 2^24 = 1e-8), of M and of the centre (<= 24 * 1e-8) stays far below the
// ADA_GATHER_EPS = 1e-5 of an index by which the box is widened -- which is all the slack it needs: the exact box is closed, so a
// sample exactly on its edge (every sample of a pure blit) is inside.  A singular, strongly magnifying, huge or non-finite matrix
// (window = the whole grid, or coordinates without digits) is left to the scatter kernel.
constexpr double ADA_GATHER_HMAX = 24.0;
constexpr double ADA_GATHER_MAG = 16777216.0;
constexpr double ADA_GATHER_EPS = 1e-5;

struct AdaInv {
    double m00, m01, m10, m11;       // M
    double kx, ky;                   // k
    double hx, hy;
    int ok;                          // the gather route takes this sample
};

ADA_HD AdaInv ada_gather_inverse(const AdaGeo& q, int H, int W) {
    AdaInv m;
    const double a = (double)q.g[0], b = (double)q.g[1], c = (double)q.g[3], d = (double)q.g[4];
    const double det = a * d - b * c;
    m.m00 = d / det, m.m01 = -b / det, m.m10 = -c / det, m.m11 = a / det;
    m.hx = fabs(m.m00) + fabs(m.m01), m.hy = fabs(m.m10) + fabs(m.m11);
    m.kx = -a * (double)(W + 5) - b * (double)(H + 5) + 2.0 * (double)q.g[2] + (double)(q.mx0 - q.mx1) + (double)(W + q.mx0 + q.mx1) - 1.0;
    m.ky = -d * (double)(H + 5) - c * (double)(W + 5) + 2.0 * (double)q.g[5] + (double)(q.my0 - q.my1) + (double)(H + q.my0 + q.my1) - 1.0;
    const double mag = fabs(m.kx) + fabs(m.ky) + (fabs(a) + fabs(b) + fabs(c) + fabs(d)) * (2.0 * (double)(W + H) + 20.0);
    m.ok = (mag <= ADA_GATHER_MAG && m.hx <= ADA_GATHER_HMAX && m.hy <= ADA_GATHER_HMAX) ? 1 : 0;      // (false for NaN)
    return m;
}

// candidate sample indices of upsampled pixel (vx, vy): jx in [jx0, jx1], jy in [jy0, jy1] (empty when lo > hi), the closed box widened
// by ADA_GATHER_EPS, clipped to the sample grid [1, 2W + 10] x [1, 2H + 10].  Only for m.ok.
ADA_HD void ada_gather_window(const AdaInv& m, int vx, int vy, int H, int W, int& jx0, int& jx1, int& jy0, int& jy1) {
    const double dx = (double)vx - m.kx, dy = (double)vy - m.ky;
    const double qx = m.m00 * dx + m.m01 * dy, qy = m.m10 * dx + m.m11 * dy;
    const double xmax = (double)(2 * W + 10), ymax = (double)(2 * H + 10);
    jx0 = (int)fmin(fmax(ceil(qx - m.hx - ADA_GATHER_EPS), 1.0), xmax + 1.0);
    jx1 = (int)fmax(fmin(floor(qx + m.hx + ADA_GATHER_EPS), xmax), 0.0);
    jy0 = (int)fmin(fmax(ceil(qy - m.hy - ADA_GATHER_EPS), 1.0), ymax + 1.0);
    jy1 = (int)fmax(fmin(floor(qy + m.hy + ADA_GATHER_EPS), ymax), 0.0);
}

}  // namespace
