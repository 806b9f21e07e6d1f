// The ADA augmentation pipe (StyleGAN2-ADA's AugmentPipe: blit, geometry and colour categories) for the critic's input, on the device.
//
// ADA's geometric stage is   reflect-pad by (mx0, mx1, my0, my1) -> upsample x2 with the 12-tap sym6 low-pass (zero insertion, padding
// (6, 5), gain 4) -> bilinear grid_sample (zeros outside, align_corners=False) on a [(H+6)*2, (W+6)*2] grid -> downsample x2 with the same
// filter (padding -6, filter not flipped)   followed by a per-sample 3x4 colour matrix.  Here it is
//   * ada_params_kernel: one workgroup turns the draws (u [N,24] uniform, g [N,8] normal; column layout in sh-gan_amd/ada.py) and the
//     probability p (read from device memory) into G_inv [N,3,3], the colour matrix [N,3,4] and the four batch-wide pad margins (int32).
//     The arithmetic is float64 (N threads of a few hundred operations): every integer decision (round of the integer translation, ceil of
//     the margins) is taken on the float64 value and the matrices are rounded to float32 once.
//   * ada_apply_kernel: the whole chain in one launch.  Per axis, a sample of the x2 grid at upsampled-pixel coordinate c reads the
//     upsampled image at x0 = floor(c) and x0 + 1 with weights (1 - t, t); the upsampled image is U[o] = 2 sum_i P[i] f[o - 2 i + 5] of
//     the padded image P, so the sample is sum_i P[i] w[i] over the (at most) 7 padded indices i = floor((x0 - 5) / 2) .. + 6 with
//         w[i] = 2 ((1 - t) [0 <= x0 < 2 Wp] f[x0 - 2 i + 5] + t [0 <= x0 + 1 < 2 Wp] f[x0 - 2 i + 6]) [0 <= i < Wp]
//     (the brackets are where ADA's tensors end: grid_sample's zeros outside the upsampled image, upfirdn2d's zeros outside the padded
//     one) and P[i] = x[reflect(i - mx0)].  Neither the padded nor the upsampled tensor exists.  With q the sample's index in the grid,
//     c = 2 (G_inv ((q - W - 5) / 2, .) + (mx0 - mx1) / 2) + Wp - 1 (ADA's margin translate and x2 conjugation folded; float64).
//     A workgroup owns a 16 x 16 output tile of one image: the source window its samples can read (their bounding box in padded-image
//     indices, reflected while it is loaded) is staged in LDS when it has at most 2304 pixels, its 42 x 42 samples are gathered from
//     there -- from memory where the window does not fit -- into LDS for four channels at a time (the weights are shared by the channels), the 12-tap decimating filter runs from LDS along y, then along x, and every thread applies the
//     colour matrix to its pixel before the one store.  The colour channels are processed first so that they meet in one thread.
//   * ada_adjoint_kernel: the exact transpose, one workgroup per (output tile, image, channel): the colour matrix transposed while the
//     cotangent tile is read, the decimating filter transposed into a 42 x 42 LDS tile of sample cotangents, then every sample scatters
//     its 7 x 7 weights with LDS atomics into a float64 LDS tile that covers the tile's bounding box in padded-image coordinates; the non-zero
//     entries are flushed with one global atomic each at the reflect-folded index.  Taps outside the box (a box that does not fit) go to
//     global memory directly.  gx must be zero on entry.  The order of float atomics is not fixed: the gradient is not bit-reproducible.
// Source indices are clamped into the image and the margins (device data) into [0, size - 1]: no access is out of bounds whatever the
// matrices hold (NaN included).
//   * ada_cot_kernel + ada_gather_kernel (shg_ada_apply_adjoint_gather_f32, ada.py: deterministic=True): the same transpose in gather
//     form, without atomics.  The forward is y = C D S U P x (reflect pad, x2 upsampling, bilinear sampling, x2 decimation, colour);
//     launch 1 stores gs = D^T C^T gy on the sample grid into a workspace, launch 2 gives every 16 x 16 source tile its (at most 3 x 3)
//     reflect images in turn: gather the upsampled cotangents gU = S^T gs on the 42 x 42 pixels the image reads, from the candidate
//     window of ada_geom.h, apply U^T from LDS, fold into registers, store once.  Float64 sums in a fixed order: the same bits on every
//     run, and gx need not be cleared.  A sample whose window is not bounded (ada_gather_inverse: singular, non-finite or magnifying
//     beyond ADA_GATHER_HMAX) gets zeros there and is handled by ada_adjoint_kernel<true> behind it: correct, not bit-reproducible.
// The coordinate arithmetic every kernel shares (ada_coord, ada_axis, ada_reflect, ada_geo, the window) lives in ada_geom.h.
#include "shg_common.h"
#include "../../include/shgan_hip.h"
#include "ada_geom.h"

namespace {

constexpr int ADA_THREADS = 256;
constexpr int ADA_T = 16;                      // output tile side
constexpr int ADA_S = 2 * ADA_T + 10;          // samples of the x2 grid a tile's outputs read, per axis
constexpr int ADA_SP = ADA_S + 1;              // LDS pitch
constexpr int ADA_CH = 4;                      // channels per pass of the forward kernel
constexpr int ADA_FBOX = 2304;                 // entries per channel of the forward's source-window LDS tile
constexpr int ADA_BOX = 4096;                  // entries (doubles) of the adjoint's source-space LDS tile
constexpr int ADA_NU = 24, ADA_NG = 8;         // draw columns

// ------------------------------------------------------------------------------------------------ parameters
struct M3 {
    double a[3][3];
};
__device__ M3 m3_eye() {
    M3 m;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.a[i][j] = i == j ? 1.0 : 0.0;
    return m;
}
__device__ M3 m3_mul(const M3& x, const M3& y) {
    M3 m;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.a[i][j] = x.a[i][0] * y.a[0][j] + x.a[i][1] * y.a[1][j] + x.a[i][2] * y.a[2][j];
    return m;
}
__device__ M3 m3_translate(double tx, double ty) {
    M3 m = m3_eye();
    m.a[0][2] = tx, m.a[1][2] = ty;
    return m;
}
__device__ M3 m3_scale(double sx, double sy) {
    M3 m = m3_eye();
    m.a[0][0] = sx, m.a[1][1] = sy;
    return m;
}
__device__ M3 m3_rotate(double th) {          // ADA's rotate2d: [[cos, sin(-th)], [sin, cos]]
    M3 m = m3_eye();
    m.a[0][0] = cos(th), m.a[0][1] = sin(-th), m.a[1][0] = sin(th), m.a[1][1] = cos(th);
    return m;
}

__global__ __launch_bounds__(ADA_THREADS) void ada_params_kernel(const float* __restrict__ u, const float* __restrict__ g,
                                                                 const float* __restrict__ p, shg_ada_config cf, float* __restrict__ Gout,
                                                                 float* __restrict__ Cout, int* __restrict__ margins, int N, int H, int W) {
    __shared__ double red[4][ADA_THREADS];
    const double PI = 3.14159265358979323846;
    const double P = (double)p[0];
    const double cx = (W - 1) * 0.5, cy = (H - 1) * 0.5;
    double mg[4] = {-1e300, -1e300, -1e300, -1e300};
    for (int n = threadIdx.x; n < N; n += ADA_THREADS) {
        const float* un = u + (long)n * ADA_NU;
        const float* gn = g + (long)n * ADA_NG;
        M3 G = m3_eye();
        {   // xflip
            double i = floor((double)un[0] * 2.0);
            if (!((double)un[1] < (double)cf.xflip * P)) i = 0.0;
            G = m3_mul(G, m3_scale(1.0 / (1.0 - 2.0 * i), 1.0));
        }
        {   // rotate90: rotate2d_inv(-pi/2 i) = rotate2d(pi/2 i)
            double i = floor((double)un[2] * 4.0);
            if (!((double)un[3] < (double)cf.rotate90 * P)) i = 0.0;
            G = m3_mul(G, m3_rotate(PI / 2 * i));
        }
        {   // integer translation
            double tx = ((double)un[4] * 2.0 - 1.0) * (double)cf.xint_max, ty = ((double)un[5] * 2.0 - 1.0) * (double)cf.xint_max;
            if (!((double)un[6] < (double)cf.xint * P)) tx = ty = 0.0;
            G = m3_mul(G, m3_translate(-rint(tx * W), -rint(ty * H)));
        }
        {   // isotropic scale
            double s = exp2((double)gn[0] * (double)cf.scale_std);
            if (!((double)un[7] < (double)cf.scale * P)) s = 1.0;
            G = m3_mul(G, m3_scale(1.0 / s, 1.0 / s));
        }
        const double p_rot = 1.0 - sqrt(fmin(fmax(1.0 - (double)cf.rotate * P, 0.0), 1.0));
        {   // pre-rotation
            double th = ((double)un[8] * 2.0 - 1.0) * PI * (double)cf.rotate_max;
            if (!((double)un[9] < p_rot)) th = 0.0;
            G = m3_mul(G, m3_rotate(th));
        }
        {   // anisotropic scale
            double s = exp2((double)gn[1] * (double)cf.aniso_std);
            if (!((double)un[10] < (double)cf.aniso * P)) s = 1.0;
            G = m3_mul(G, m3_scale(1.0 / s, s));
        }
        {   // post-rotation
            double th = ((double)un[11] * 2.0 - 1.0) * PI * (double)cf.rotate_max;
            if (!((double)un[12] < p_rot)) th = 0.0;
            G = m3_mul(G, m3_rotate(th));
        }
        {   // fractional translation
            double tx = (double)gn[2] * (double)cf.xfrac_std, ty = (double)gn[3] * (double)cf.xfrac_std;
            if (!((double)un[13] < (double)cf.xfrac * P)) tx = ty = 0.0;
            G = m3_mul(G, m3_translate(-tx * W, -ty * H));
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Gout[(long)n * 9 + i * 3 + j] = (float)G.a[i][j];
        const double sx[4] = {-cx, cx, cx, -cx}, sy[4] = {-cy, -cy, cy, cy};
        for (int k = 0; k < 4; ++k) {
            const double x = G.a[0][0] * sx[k] + G.a[0][1] * sy[k] + G.a[0][2], y = G.a[1][0] * sx[k] + G.a[1][1] * sy[k] + G.a[1][2];
            mg[0] = fmax(mg[0], -x), mg[1] = fmax(mg[1], -y), mg[2] = fmax(mg[2], x), mg[3] = fmax(mg[3], y);
        }

        // colour: a 3x4 matrix [M | t], every factor multiplied from the left
        double C[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        auto left = [&](const double (&M)[3][3]) {
            double R[3][4];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) R[i][j] = M[i][0] * C[0][j] + M[i][1] * C[1][j] + M[i][2] * C[2][j];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) C[i][j] = R[i][j];
        };
        {   // brightness
            double b = (double)gn[4] * (double)cf.brightness_std;
            if (!((double)un[14] < (double)cf.brightness * P)) b = 0.0;
            for (int i = 0; i < 3; ++i) C[i][3] += b;
        }
        {   // contrast
            double c = exp2((double)gn[5] * (double)cf.contrast_std);
            if (!((double)un[15] < (double)cf.contrast * P)) c = 1.0;
            const double M[3][3] = {{c, 0, 0}, {0, c, 0}, {0, 0, c}};
            left(M);
        }
        const double v = 1.0 / sqrt(3.0), vv = v * v;
        {   // luma flip: I - 2 v v^T i
            double i = floor((double)un[16] * 2.0);
            if (!((double)un[17] < (double)cf.lumaflip * P)) i = 0.0;
            double M[3][3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) M[a][b] = (a == b ? 1.0 : 0.0) - 2.0 * vv * i;
            left(M);
        }
        if (cf.color_count == 3) {
            {   // hue: rotation about v
                double th = ((double)un[18] * 2.0 - 1.0) * PI * (double)cf.hue_max;
                if (!((double)un[19] < (double)cf.hue * P)) th = 0.0;
                const double s = sin(th), c = cos(th), cc = 1.0 - c;
                const double M[3][3] = {{vv * cc + c, vv * cc - v * s, vv * cc + v * s},
                                        {vv * cc + v * s, vv * cc + c, vv * cc - v * s},
                                        {vv * cc - v * s, vv * cc + v * s, vv * cc + c}};
                left(M);
            }
            {   // saturation: v v^T + (I - v v^T) s
                double s = exp2((double)gn[6] * (double)cf.saturation_std);
                if (!((double)un[20] < (double)cf.saturation * P)) s = 1.0;
                double M[3][3];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) M[a][b] = vv + ((a == b ? 1.0 : 0.0) - vv) * s;
                left(M);
            }
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) Cout[(long)n * 12 + i * 4 + j] = (float)C[i][j];
    }
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = mg[k];
    __syncthreads();
    for (int s = ADA_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = fmax(red[k][threadIdx.x], red[k][threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const double c = (k & 1) ? cy : cx, hi = (k & 1) ? (double)(H - 1) : (double)(W - 1);
        double m = red[k][0] + (6.0 - c);                 // Hz_pad * 2 - c, Hz_pad = 12 / 4
        m = fmin(fmax(m, 0.0), hi);
        margins[k] = (int)ceil(m);                        // mx0, my0, mx1, my1
    }
}

// The bounding box, in padded-image indices, of everything the samples of a tile read: the coordinate is affine in the sample index, so the
// tile's corner samples bound it.  One index of slack on each side, clipped to the padded image (weights are zero outside it); a box of
// more than `cap` entries is returned empty.
__device__ __forceinline__ void ada_box(const AdaGeo& q, int ty0, int tx0, int H, int W, int cap, int& bx0, int& by0, int& bw, int& bh) {
    const int sy_l = min(ADA_S - 1, 2 * H + 10 - (2 * ty0 + 1)), sx_l = min(ADA_S - 1, 2 * W + 10 - (2 * tx0 + 1));
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
    for (int k = 0; k < 4; ++k) {
        const int jy = 2 * ty0 + 1 + ((k & 2) ? sy_l : 0), jx = 2 * tx0 + 1 + ((k & 1) ? sx_l : 0);
        const double cxk = ada_coord(jx, jy, q.g[0], q.g[1], q.g[2], W, H, q.mx0, q.mx1);
        const double cyk = ada_coord(jy, jx, q.g[4], q.g[3], q.g[5], H, W, q.my0, q.my1);
        xmin = fmin(xmin, cxk), xmax = fmax(xmax, cxk), ymin = fmin(ymin, cyk), ymax = fmax(ymax, cyk);
    }
    const int wp = W + q.mx0 + q.mx1, hp = H + q.my0 + q.my1;
    bx0 = max((((int)floor(xmin) - 5) >> 1) - 1, 0);
    by0 = max((((int)floor(ymin) - 5) >> 1) - 1, 0);
    const int bx1 = min((((int)floor(xmax) - 5) >> 1) + 7, wp - 1), by1 = min((((int)floor(ymax) - 5) >> 1) + 7, hp - 1);
    bw = max(bx1 - bx0 + 1, 0), bh = max(by1 - by0 + 1, 0);
    if ((long)bw * bh > cap) bw = bh = 0;
}

// one sample of one channel: sum_r wy[r] sum_c wx[c] base[ro[r] + co[c]]
__device__ __forceinline__ float ada_dot(const float* base, const int (&ro)[7], const int (&co)[7], const float (&wy)[7], const float (&wx)[7]) {
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const float* row = base + ro[r];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 7; ++c) s = __builtin_fmaf(wx[c], row[co[c]], s);
        acc = __builtin_fmaf(wy[r], s, acc);
    }
    return acc;
}

// channel j of the processing order: the colour channels first, the others ascending
__device__ __forceinline__ int ada_perm(int j, int cf, int cc) { return j < cc ? cf + j : (j - cc < cf ? j - cc : j); }

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(ADA_THREADS) void ada_apply_kernel(const float* __restrict__ x, const float* __restrict__ G,
                                                                const float* __restrict__ Cm, const int* __restrict__ margins,
                                                                float* __restrict__ y, int C, int H, int W, int cf, int cc, int bias) {
    __shared__ float smp[ADA_CH][ADA_S][ADA_SP];
    __shared__ float vt[ADA_CH][ADA_T][ADA_SP];
    __shared__ float win[ADA_CH][ADA_FBOX];      // the source window of the tile (reflect-padded indexing), when it fits
    const int n = blockIdx.z, ty0 = (int)blockIdx.y * ADA_T, tx0 = (int)blockIdx.x * ADA_T, tid = threadIdx.x;
    const AdaGeo q = ada_geo(G, margins, n, H, W);
    const long plane = (long)H * W;
    const int jy_max = 2 * H + 10, jx_max = 2 * W + 10;
    const int wp = W + q.mx0 + q.mx1, hp = H + q.my0 + q.my1;
    int bx0, by0, bw, bh;
    ada_box(q, ty0, tx0, H, W, ADA_FBOX, bx0, by0, bw, bh);
    for (int c0 = 0; c0 < C; c0 += ADA_CH) {
        const int nch = min(ADA_CH, C - c0);
        const float* pl[ADA_CH];
#pragma unroll
        for (int k = 0; k < ADA_CH; ++k) pl[k] = x + ((long)n * C + ada_perm(c0 + min(k, nch - 1), cf, cc)) * plane;
        for (int e = tid; e < bw * bh; e += ADA_THREADS) {
            const int bi = e / bw, bj = e - bi * bw;
            const long at = (long)ada_reflect(by0 + bi, q.my0, H) * W + ada_reflect(bx0 + bj, q.mx0, W);
#pragma unroll
            for (int k = 0; k < ADA_CH; ++k)
                if (k < nch) win[k][e] = pl[k][at];
        }
        __syncthreads();
        for (int e = tid; e < ADA_S * ADA_S; e += ADA_THREADS) {
            const int sy = e / ADA_S, sx = e - sy * ADA_S;
            const int jy = 2 * ty0 + 1 + sy, jx = 2 * tx0 + 1 + sx;
            float acc[ADA_CH] = {0.f, 0.f, 0.f, 0.f};
            if (jy <= jy_max && jx <= jx_max) {            // (samples past the grid feed only outputs past the image)
                AdaAxis ax, ay;
                ada_axis(ada_coord(jx, jy, q.g[0], q.g[1], q.g[2], W, H, q.mx0, q.mx1), W, q.mx0, q.mx1, ax);
                ada_axis(ada_coord(jy, jx, q.g[4], q.g[3], q.g[5], H, W, q.my0, q.my1), H, q.my0, q.my1, ay);
                // the taps that can carry weight (inside the padded image) against the window
                const int xl = max(ax.lo, 0), xh = min(ax.lo + 6, wp - 1), yl = max(ay.lo, 0), yh = min(ay.lo + 6, hp - 1);
                int ro[7], co[7];
                if (xl > xh || yl > yh) {
                    // every weight is zero
                } else if (xl >= bx0 && xh < bx0 + bw && yl >= by0 && yh < by0 + bh) {
#pragma unroll
                    for (int r = 0; r < 7; ++r) {
                        ro[r] = min(max(ay.lo + r - by0, 0), bh - 1) * bw;
                        co[r] = min(max(ax.lo + r - bx0, 0), bw - 1);
                    }
#pragma unroll
                    for (int k = 0; k < ADA_CH; ++k)
                        if (k < nch) acc[k] = ada_dot(win[k], ro, co, ay.w, ax.w);
                } else {                                   // (the window did not fit, or this sample leaves it: gather from memory)
#pragma unroll
                    for (int r = 0; r < 7; ++r) ro[r] = ay.idx[r] * W, co[r] = ax.idx[r];
#pragma unroll
                    for (int k = 0; k < ADA_CH; ++k)
                        if (k < nch) acc[k] = ada_dot(pl[k], ro, co, ay.w, ax.w);
                }
            }
#pragma unroll
            for (int k = 0; k < ADA_CH; ++k) smp[k][sy][sx] = acc[k];
        }
        __syncthreads();
        for (int e = tid; e < ADA_T * ADA_S; e += ADA_THREADS) {        // decimating filter along y: y[o] = sum_t S[2 o + t + 1] f[t]
            const int oy = e / ADA_S, sx = e - oy * ADA_S;
#pragma unroll
            for (int k = 0; k < ADA_CH; ++k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < 12; ++t) s = __builtin_fmaf(ADA_F[t], smp[k][2 * oy + t][sx], s);
                vt[k][oy][sx] = s;
            }
        }
        __syncthreads();
        const int oy = tid / ADA_T, ox = tid - oy * ADA_T;
        float o[ADA_CH];
#pragma unroll
        for (int k = 0; k < ADA_CH; ++k) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 12; ++t) s = __builtin_fmaf(ADA_F[t], vt[k][oy][2 * ox + t], s);
            o[k] = s;
        }
        if (c0 == 0 && cc > 0) {
            const float* M = Cm + (long)n * 12;
            if (cc == 3) {
                const float a0 = o[0], a1 = o[1], a2 = o[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) o[r] = M[r * 4] * a0 + M[r * 4 + 1] * a1 + M[r * 4 + 2] * a2 + (bias ? M[r * 4 + 3] : 0.f);
            } else {                                     // one channel: the mean of the rows
                const float sc = (M[0] + M[1] + M[2] + M[4] + M[5] + M[6] + M[8] + M[9] + M[10]) * (1.f / 3.f);
                const float of = (M[3] + M[7] + M[11]) * (1.f / 3.f);
                o[0] = o[0] * sc + (bias ? of : 0.f);
            }
        }
        if (ty0 + oy < H && tx0 + ox < W) {
#pragma unroll
            for (int k = 0; k < ADA_CH; ++k)
                if (k < nch) y[((long)n * C + ada_perm(c0 + k, cf, cc)) * plane + (long)(ty0 + oy) * W + tx0 + ox] = o[k];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ adjoint
// REST: launched behind the gather route, for the samples it left alone (it wrote zeros there); a workgroup of any other sample returns.
template <bool REST>
__global__ __launch_bounds__(ADA_THREADS) void ada_adjoint_kernel(const float* __restrict__ gy, const float* __restrict__ G,
                                                                  const float* __restrict__ Cm, const int* __restrict__ margins,
                                                                  float* __restrict__ gx, int C, int H, int W, int cf, int cc) {
    __shared__ float gt[ADA_T][ADA_T + 1];
    __shared__ float ht[ADA_T][ADA_SP];
    __shared__ float gs[ADA_S][ADA_SP];
    __shared__ double box[ADA_BOX];          // float64: a source pixel collects some hundred signed terms when the image is magnified
    const int n = (int)blockIdx.z / C, ch = (int)blockIdx.z - n * C;
    const int ty0 = (int)blockIdx.y * ADA_T, tx0 = (int)blockIdx.x * ADA_T, tid = threadIdx.x;
    const AdaGeo q = ada_geo(G, margins, n, H, W);
    if (REST && ada_gather_inverse(q, H, W).ok) return;
    const long plane = (long)H * W;
    {   // the cotangent tile of this source channel, colour matrix transposed
        const int oy = tid / ADA_T, ox = tid - oy * ADA_T;
        float v = 0.f;
        if (ty0 + oy < H && tx0 + ox < W) {
            const long at = (long)(ty0 + oy) * W + tx0 + ox;
            const float* M = Cm + (long)n * 12;
            if (cc == 3 && ch >= cf && ch < cf + 3) {
                const float* b = gy + ((long)n * C + cf) * plane + at;
                const int j = ch - cf;
                v = M[j] * b[0] + M[4 + j] * b[plane] + M[8 + j] * b[2 * plane];
            } else if (cc == 1 && ch == cf) {
                const float sc = (M[0] + M[1] + M[2] + M[4] + M[5] + M[6] + M[8] + M[9] + M[10]) * (1.f / 3.f);
                v = sc * gy[((long)n * C + ch) * plane + at];
            } else {
                v = gy[((long)n * C + ch) * plane + at];
            }
        }
        gt[oy][ox] = v;
    }
    __syncthreads();
    for (int e = tid; e < ADA_T * ADA_S; e += ADA_THREADS) {           // along x: sample 2 o + t gets f[t] gy[o]
        const int oy = e / ADA_S, sx = e - oy * ADA_S;
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 6; ++h) {
            const int t = (sx & 1) + 2 * h, o = (sx - t) >> 1;
            if (o >= 0 && o < ADA_T) s = __builtin_fmaf(ADA_F[t], gt[oy][o], s);
        }
        ht[oy][sx] = s;
    }
    __syncthreads();
    for (int e = tid; e < ADA_S * ADA_S; e += ADA_THREADS) {           // along y
        const int sy = e / ADA_S, sx = e - sy * ADA_S;
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 6; ++h) {
            const int t = (sy & 1) + 2 * h, o = (sy - t) >> 1;
            if (o >= 0 && o < ADA_T) s = __builtin_fmaf(ADA_F[t], ht[o][sx], s);
        }
        gs[sy][sx] = s;
    }
    const int sy_l = min(ADA_S - 1, 2 * H + 10 - (2 * ty0 + 1)), sx_l = min(ADA_S - 1, 2 * W + 10 - (2 * tx0 + 1));
    int bx0, by0, bw, bh;                                               // a box that does not fit: every tap goes to global memory
    ada_box(q, ty0, tx0, H, W, ADA_BOX, bx0, by0, bw, bh);
    for (int e = tid; e < bw * bh; e += ADA_THREADS) box[e] = 0.0;
    __syncthreads();
    float* out = gx + ((long)n * C + ch) * plane;
    for (int e = tid; e < ADA_S * ADA_S; e += ADA_THREADS) {
        const int sy = e / ADA_S, sx = e - sy * ADA_S;
        const float gv = gs[sy][sx];
        if (gv == 0.f || sy > sy_l || sx > sx_l) continue;
        const int jy = 2 * ty0 + 1 + sy, jx = 2 * tx0 + 1 + sx;
        AdaAxis ax, ay;
        ada_axis(ada_coord(jx, jy, q.g[0], q.g[1], q.g[2], W, H, q.mx0, q.mx1), W, q.mx0, q.mx1, ax);
        ada_axis(ada_coord(jy, jx, q.g[4], q.g[3], q.g[5], H, W, q.my0, q.my1), H, q.my0, q.my1, ay);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const float wr = ay.w[r] * gv;
            if (wr == 0.f) continue;
            const int bi = ay.lo + r - by0;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const float w = wr * ax.w[c];
                if (w == 0.f) continue;
                const int bj = ax.lo + c - bx0;
                if (bi >= 0 && bi < bh && bj >= 0 && bj < bw)
                    __hip_atomic_fetch_add(&box[bi * bw + bj], (double)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    unsafeAtomicAdd(out + (long)ay.idx[r] * W + ax.idx[c], w);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < bw * bh; e += ADA_THREADS) {
        const float v = (float)box[e];
        if (v != 0.f) {
            const int bi = e / bw, bj = e - bi * bw;
            unsafeAtomicAdd(out + (long)ada_reflect(by0 + bi, q.my0, H) * W + ada_reflect(bx0 + bj, q.mx0, W), v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ adjoint, gather form (no atomics)
constexpr int ADA_GT = 32;                     // samples per axis of one workgroup of the cotangent kernel
constexpr int ADA_GO = ADA_GT / 2 + 5;         // outputs per axis that feed them

// Launch 1: gs = D^T C^T gy on the sample grid, ws [N, C, 2H + 10, 2W + 10] (element [j - 1] is sample index j): the colour matrix
// transposed while the cotangent is read, then gs[j] = sum_t f[t] gy[(j - 1 - t) / 2] over the t of the parity of j - 1, along x, then y.
// A workgroup owns 32 x 32 samples of one (sample, channel) and stores each once.  Samples the gather does not take are skipped.
__global__ __launch_bounds__(ADA_THREADS) void ada_cot_kernel(const float* __restrict__ gy, const float* __restrict__ G,
                                                              const float* __restrict__ Cm, const int* __restrict__ margins,
                                                              float* __restrict__ ws, int C, int H, int W, int cf, int cc) {
    __shared__ float gt[ADA_GO][ADA_GO + 1];
    __shared__ float ht[ADA_GO][ADA_GT + 1];
    const int n = (int)blockIdx.z / C, ch = (int)blockIdx.z - n * C, tid = threadIdx.x;
    if (!ada_gather_inverse(ada_geo(G, margins, n, H, W), H, W).ok) return;
    const int oy0 = (int)blockIdx.y * (ADA_GT / 2) - 5, ox0 = (int)blockIdx.x * (ADA_GT / 2) - 5;
    const long plane = (long)H * W;
    for (int e = tid; e < ADA_GO * ADA_GO; e += ADA_THREADS) {
        const int ly = e / ADA_GO, lx = e - ly * ADA_GO;
        const int oy = oy0 + ly, ox = ox0 + lx;
        float v = 0.f;
        if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
            const long at = (long)oy * W + ox;
            const float* M = Cm + (long)n * 12;
            if (cc == 3 && ch >= cf && ch < cf + 3) {
                const float* b = gy + ((long)n * C + cf) * plane + at;
                const int j = ch - cf;
                v = M[j] * b[0] + M[4 + j] * b[plane] + M[8 + j] * b[2 * plane];
            } else if (cc == 1 && ch == cf) {
                const float sc = (M[0] + M[1] + M[2] + M[4] + M[5] + M[6] + M[8] + M[9] + M[10]) * (1.f / 3.f);
                v = sc * gy[((long)n * C + ch) * plane + at];
            } else {
                v = gy[((long)n * C + ch) * plane + at];
            }
        }
        gt[ly][lx] = v;
    }
    __syncthreads();
    for (int e = tid; e < ADA_GO * ADA_GT; e += ADA_THREADS) {         // along x: output (s - t) / 2 is local (s - t) / 2 + 5
        const int ly = e / ADA_GT, sx = e - ly * ADA_GT;
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 6; ++h) {
            const int t = (sx & 1) + 2 * h;
            s = __builtin_fmaf(ADA_F[t], gt[ly][((sx - t) >> 1) + 5], s);
        }
        ht[ly][sx] = s;
    }
    __syncthreads();
    const int SH = 2 * H + 10, SW = 2 * W + 10;
    float* out = ws + ((long)n * C + ch) * ((long)SH * SW);
    for (int e = tid; e < ADA_GT * ADA_GT; e += ADA_THREADS) {         // along y
        const int sy = e / ADA_GT, sx = e - sy * ADA_GT;
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 6; ++h) {
            const int t = (sy & 1) + 2 * h;
            s = __builtin_fmaf(ADA_F[t], ht[((sy - t) >> 1) + 5][sx], s);
        }
        const int gy_ = (int)blockIdx.y * ADA_GT + sy, gx_ = (int)blockIdx.x * ADA_GT + sx;
        if (gy_ < SH && gx_ < SW) out[(long)gy_ * SW + gx_] = s;
    }
}

// One axis of one reflect image of a 16-wide source tile.  Source index y has the padded preimages m0 + y (img 0), m0 - y for y >= 1
// (img 1) and m0 + 2 (n - 1) - y for y <= n - 2 (img 2), each where it lies inside [0, n + m0 + m1).
struct AdaImage {
    int base, sgn;       // padded index of local l: base + sgn * l
    int imin;            // padded index of row 0 of the LDS tile (the smallest of the 16)
    int p0, p1;          // the padded indices that are preimages, [p0, p1]; p0 > p1: none
};
__device__ __forceinline__ bool ada_image_valid(int img, int y, int pi, int n, int np) {
    return y < n && (img == 0 || (img == 1 && y >= 1 && pi >= 0) || (img == 2 && y <= n - 2 && pi < np));
}
__device__ __forceinline__ AdaImage ada_image(int img, int t0, int m0, int n, int np) {
    AdaImage a;
    a.sgn = img == 0 ? 1 : -1;
    a.base = (img == 2 ? m0 + 2 * (n - 1) : m0) + a.sgn * t0;
    a.imin = a.sgn > 0 ? a.base : a.base - (ADA_T - 1);
    a.p0 = 1 << 30, a.p1 = -(1 << 30);
    for (int l = 0; l < ADA_T; ++l) {
        const int pi = a.base + a.sgn * l;
        if (ada_image_valid(img, t0 + l, pi, n, np)) a.p0 = min(a.p0, pi), a.p1 = max(a.p1, pi);
    }
    return a;
}

// Launch 2: gx = P^T U^T S^T gs.  A workgroup owns a 16 x 16 tile of the source image of one sample and up to ADA_CH channels.  For each
// of the (at most 3 x 3) reflect images of the tile, in a fixed order: gather gU on the 42 x 42 upsampled pixels the image's padded pixels
// read (every candidate sample of the pixel's window, in index order, evaluated with the forward's ada_coord: it contributes 2 (1 - t) or
// 2 t per axis according to floor(c) = v or v - 1), U^T along y, then along x, from LDS, and the fold into per-thread accumulators.  One
// store; every sum is float64 in a fixed order.  A sample the gather does not take (ada_gather_inverse) gets zeros.
__global__ __launch_bounds__(ADA_THREADS) void ada_gather_kernel(const float* __restrict__ ws, const float* __restrict__ G,
                                                                 const int* __restrict__ margins, float* __restrict__ gx, int C, int H,
                                                                 int W) {
    __shared__ double gu[ADA_CH][ADA_S][ADA_SP];
    __shared__ double mid[ADA_CH][ADA_T][ADA_SP];
    const int groups = (C + ADA_CH - 1) / ADA_CH;
    const int n = (int)blockIdx.z / groups, c0 = ((int)blockIdx.z - n * groups) * ADA_CH, nch = min(ADA_CH, C - c0);
    const int ty0 = (int)blockIdx.y * ADA_T, tx0 = (int)blockIdx.x * ADA_T, tid = threadIdx.x;
    const int yl = tid / ADA_T, xl = tid - yl * ADA_T;
    const AdaGeo q = ada_geo(G, margins, n, H, W);
    const AdaInv m = ada_gather_inverse(q, H, W);
    double acc[ADA_CH] = {0.0, 0.0, 0.0, 0.0};
    if (m.ok) {
        const int hp = H + q.my0 + q.my1, wp = W + q.mx0 + q.mx1, SW = 2 * W + 10;
        const long splane = (long)(2 * H + 10) * SW;
        const float* src[ADA_CH];
#pragma unroll
        for (int k = 0; k < ADA_CH; ++k) src[k] = ws + ((long)n * C + c0 + min(k, nch - 1)) * splane;
        for (int iy = 0; iy < 3; ++iy) {
            const AdaImage ay = ada_image(iy, ty0, q.my0, H, hp);
            if (ay.p0 > ay.p1) continue;
            for (int ix = 0; ix < 3; ++ix) {
                const AdaImage ax = ada_image(ix, tx0, q.mx0, W, wp);
                if (ax.p0 > ax.p1) continue;
                for (int e = tid; e < ADA_S * ADA_S; e += ADA_THREADS) {
                    const int uy = e / ADA_S, ux = e - uy * ADA_S;
                    const int vy = 2 * ay.imin - 5 + uy, vx = 2 * ax.imin - 5 + ux;
                    double a[ADA_CH] = {0.0, 0.0, 0.0, 0.0};
                    if (vy >= max(0, 2 * ay.p0 - 5) && vy <= min(2 * hp - 1, 2 * ay.p1 + 6) && vx >= max(0, 2 * ax.p0 - 5) &&
                        vx <= min(2 * wp - 1, 2 * ax.p1 + 6)) {
                        int jx0, jx1, jy0, jy1;
                        ada_gather_window(m, vx, vy, H, W, jx0, jx1, jy0, jy1);
                        for (int jy = jy0; jy <= jy1; ++jy) {
                            for (int jx = jx0; jx <= jx1; ++jx) {
                                const double cx = ada_coord(jx, jy, q.g[0], q.g[1], q.g[2], W, H, q.mx0, q.mx1);
                                const double fx = floor(cx);
                                const int dx = vx - (int)fx;
                                if (dx != 0 && dx != 1) continue;
                                const double cy = ada_coord(jy, jx, q.g[4], q.g[3], q.g[5], H, W, q.my0, q.my1);
                                const double fy = floor(cy);
                                const int dy = vy - (int)fy;
                                if (dy != 0 && dy != 1) continue;
                                const float tx = (float)(cx - fx), ty = (float)(cy - fy);          // the forward's weights
                                const float wx = dx == 0 ? 2.f * (1.f - tx) : 2.f * tx, wy = dy == 0 ? 2.f * (1.f - ty) : 2.f * ty;
                                const double w = (double)wx * (double)wy;
                                const long at = (long)(jy - 1) * SW + (jx - 1);
#pragma unroll
                                for (int k = 0; k < ADA_CH; ++k)
                                    if (k < nch) a[k] += w * (double)src[k][at];
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < ADA_CH; ++k) gu[k][uy][ux] = a[k];
                }
                __syncthreads();
                for (int e = tid; e < ADA_T * ADA_S; e += ADA_THREADS) {       // U^T along y: gP[i] = sum_o gU[o] f[o - 2 i + 5]
                    const int ly = e / ADA_S, ux = e - ly * ADA_S;
#pragma unroll
                    for (int k = 0; k < ADA_CH; ++k) {
                        double s = 0.0;
#pragma unroll
                        for (int t = 0; t < 12; ++t) s += gu[k][2 * ly + t][ux] * (double)ADA_F[t];
                        mid[k][ly][ux] = s;
                    }
                }
                __syncthreads();
                {   // along x, for this thread's source pixel, and the fold
                    const int ly = ay.sgn > 0 ? yl : ADA_T - 1 - yl, lx = ax.sgn > 0 ? xl : ADA_T - 1 - xl;
                    if (ada_image_valid(iy, ty0 + yl, ay.base + ay.sgn * yl, H, hp) && ada_image_valid(ix, tx0 + xl, ax.base + ax.sgn * xl, W, wp)) {
#pragma unroll
                        for (int k = 0; k < ADA_CH; ++k) {
                            double s = 0.0;
#pragma unroll
                            for (int t = 0; t < 12; ++t) s += mid[k][ly][2 * lx + t] * (double)ADA_F[t];
                            acc[k] += s;
                        }
                    }
                }
                // (the next image's gather writes gu, which nobody reads any more; mid is written again only behind that gather's barrier)
            }
        }
    }
    if (ty0 + yl < H && tx0 + xl < W) {
#pragma unroll
        for (int k = 0; k < ADA_CH; ++k)
            if (k < nch) gx[(((long)n * C + c0 + k) * H + ty0 + yl) * W + tx0 + xl] = (float)acc[k];
    }
}

// ------------------------------------------------------------------------------------------------ colour alone (geometry off)
template <bool ADJ>
__global__ __launch_bounds__(ADA_THREADS) void ada_color_kernel(const float* __restrict__ x, const float* __restrict__ Cm,
                                                                float* __restrict__ y, int C, long plane, int cf, int cc, int bias) {
    const long i = (long)blockIdx.x * ADA_THREADS + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= plane) return;
    const float* xi = x + (long)n * C * plane + i;
    float* yi = y + (long)n * C * plane + i;
    const float* M = Cm + (long)n * 12;
    for (int c = 0; c < C; ++c)
        if (c < cf || c >= cf + cc) yi[c * plane] = xi[c * plane];
    if (cc == 3) {
        const float a0 = xi[cf * plane], a1 = xi[(cf + 1) * plane], a2 = xi[(cf + 2) * plane];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            yi[(cf + r) * plane] = ADJ ? M[r] * a0 + M[4 + r] * a1 + M[8 + r] * a2
                                       : M[r * 4] * a0 + M[r * 4 + 1] * a1 + M[r * 4 + 2] * a2 + (bias ? M[r * 4 + 3] : 0.f);
    } else if (cc == 1) {
        const float sc = (M[0] + M[1] + M[2] + M[4] + M[5] + M[6] + M[8] + M[9] + M[10]) * (1.f / 3.f);
        const float of = (M[3] + M[7] + M[11]) * (1.f / 3.f);
        yi[cf * plane] = xi[cf * plane] * sc + ((!ADJ && bias) ? of : 0.f);
    }
}

int ada_check(const char* name, const void* x, const void* G, const void* Cm, const void* margins, const void* y, int N, int C, int H, int W,
              int geom, int cf, int cc) {
    SHG_CHECK_ARG(x && y && x != y, "%s: null or aliased image pointer", name);
    SHG_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: N, C, H, W must be >= 1 (got %d, %d, %d, %d)", name, N, C, H, W);
    SHG_CHECK_ARG(H <= 16384 && W <= 16384 && (long)N * C <= 65535, "%s: H, W <= 16384 and N * C <= 65535 (got %d x %d, %d x %d)", name, H, W,
                  N, C);
    SHG_CHECK_ARG(geom == 0 || geom == 1, "%s: geom must be 0 or 1", name);
    SHG_CHECK_ARG(cc == 0 || cc == 1 || cc == 3, "%s: color_count must be 0, 1 or 3 (got %d)", name, cc);
    SHG_CHECK_ARG(cc == 0 || (cf >= 0 && cf + cc <= C), "%s: colour channels [%d, %d) lie outside the %d channels", name, cf, cf + cc, C);
    SHG_CHECK_ARG(geom || cc, "%s: nothing to do (geometry and colour both off)", name);
    SHG_CHECK_ARG(!geom || (G && margins), "%s: geometry needs G_inv and the margins", name);
    SHG_CHECK_ARG(!cc || Cm, "%s: colour needs the colour matrix", name);
    return SHG_OK;
}

}  // namespace

extern "C" int shg_ada_params_f32(const float* u, const float* g, const float* p, const shg_ada_config* cfg, float* G_inv, float* Cm,
                                  int* margins, int N, int H, int W, void* stream) {
    SHG_CHECK_ARG(u && g && p && cfg && G_inv && Cm && margins, "ada_params_f32: null pointer");
    SHG_CHECK_ARG(N >= 1 && N <= (1 << 20) && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "ada_params_f32: N in [1, 2^20], H, W in [1, 16384]");
    SHG_CHECK_ARG(cfg->color_count == 1 || cfg->color_count == 3, "ada_params_f32: color_count must be 1 or 3 (got %d)", cfg->color_count);
    hipLaunchKernelGGL(ada_params_kernel, dim3(1), dim3(ADA_THREADS), 0, (hipStream_t)stream, u, g, p, *cfg, G_inv, Cm, margins, N, H, W);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_ada_apply_f32(const float* x, const float* G_inv, const float* Cm, const int* margins, float* y, int N, int C, int H, int W,
                                 int geom, int color_first, int color_count, int bias, void* stream) {
    const int rc = ada_check("ada_apply_f32", x, G_inv, Cm, margins, y, N, C, H, W, geom, color_first, color_count);
    if (rc != SHG_OK) return rc;
    const int cf = color_count ? color_first : 0;
    if (geom) {
        const dim3 grid(shg_cdiv(W, ADA_T), shg_cdiv(H, ADA_T), N);
        hipLaunchKernelGGL(ada_apply_kernel, grid, dim3(ADA_THREADS), 0, (hipStream_t)stream, x, G_inv, Cm, margins, y, C, H, W, cf, color_count,
                           bias);
    } else {
        const long plane = (long)H * W;
        hipLaunchKernelGGL(ada_color_kernel<false>, dim3(shg_cdiv(plane, ADA_THREADS), N), dim3(ADA_THREADS), 0, (hipStream_t)stream, x, Cm, y,
                           C, plane, cf, color_count, bias);
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_ada_apply_adjoint_f32(const float* gy, const float* G_inv, const float* Cm, const int* margins, float* gx, int N, int C,
                                         int H, int W, int geom, int color_first, int color_count, void* stream) {
    const int rc = ada_check("ada_apply_adjoint_f32", gy, G_inv, Cm, margins, gx, N, C, H, W, geom, color_first, color_count);
    if (rc != SHG_OK) return rc;
    const int cf = color_count ? color_first : 0;
    if (geom) {
        const dim3 grid(shg_cdiv(W, ADA_T), shg_cdiv(H, ADA_T), N * C);
        hipLaunchKernelGGL(ada_adjoint_kernel<false>, grid, dim3(ADA_THREADS), 0, (hipStream_t)stream, gy, G_inv, Cm, margins, gx, C, H, W, cf,
                           color_count);
    } else {
        const long plane = (long)H * W;
        hipLaunchKernelGGL(ada_color_kernel<true>, dim3(shg_cdiv(plane, ADA_THREADS), N), dim3(ADA_THREADS), 0, (hipStream_t)stream, gy, Cm, gx,
                           C, plane, cf, color_count, 0);
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" long shg_ada_adjoint_gather_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || (long)N * C > 65535) return 0;
    return (long)N * C * (2 * H + 10) * (2 * W + 10) * (long)sizeof(float);
}

extern "C" int shg_ada_apply_adjoint_gather_f32(const float* gy, const float* G_inv, const float* Cm, const int* margins, float* gx,
                                                void* workspace, long workspace_bytes, int N, int C, int H, int W, int geom, int color_first,
                                                int color_count, void* stream) {
    const int rc = ada_check("ada_apply_adjoint_gather_f32", gy, G_inv, Cm, margins, gx, N, C, H, W, geom, color_first, color_count);
    if (rc != SHG_OK) return rc;
    const int cf = color_count ? color_first : 0;
    if (geom) {
        const long need = shg_ada_adjoint_gather_workspace_bytes(N, C, H, W);
        SHG_CHECK_ARG(workspace && workspace_bytes >= need, "ada_apply_adjoint_gather_f32: the workspace must hold %ld bytes (got %s, %ld)", need,
                      workspace ? "a pointer" : "null", workspace_bytes);
        SHG_CHECK_ARG(workspace != (const void*)gy && workspace != (void*)gx, "ada_apply_adjoint_gather_f32: the workspace aliases an image");
        const hipStream_t s = (hipStream_t)stream;
        float* ws = (float*)workspace;
        const dim3 cot(shg_cdiv(2 * W + 10, ADA_GT), shg_cdiv(2 * H + 10, ADA_GT), N * C);
        hipLaunchKernelGGL(ada_cot_kernel, cot, dim3(ADA_THREADS), 0, s, gy, G_inv, Cm, margins, ws, C, H, W, cf, color_count);
        const dim3 tiles(shg_cdiv(W, ADA_T), shg_cdiv(H, ADA_T), N * shg_cdiv(C, ADA_CH));
        hipLaunchKernelGGL(ada_gather_kernel, tiles, dim3(ADA_THREADS), 0, s, (const float*)ws, G_inv, margins, gx, C, H, W);
        // the samples the gather left alone (it wrote zeros): the scatter kernel, whose other workgroups return at once
        const dim3 grid(shg_cdiv(W, ADA_T), shg_cdiv(H, ADA_T), N * C);
        hipLaunchKernelGGL(ada_adjoint_kernel<true>, grid, dim3(ADA_THREADS), 0, s, gy, G_inv, Cm, margins, gx, C, H, W, cf, color_count);
    } else {
        const long plane = (long)H * W;
        hipLaunchKernelGGL(ada_color_kernel<true>, dim3(shg_cdiv(plane, ADA_THREADS), N), dim3(ADA_THREADS), 0, (hipStream_t)stream, gy, Cm, gx,
                           C, plane, cf, color_count, 0);
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
