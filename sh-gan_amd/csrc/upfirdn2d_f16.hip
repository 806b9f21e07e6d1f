// FIR resampling on NHWC halves (reference: upfirdn2d.cu's half instantiation, upfirdn2d.cpp:59; fp32 accumulation as its `scalar_t` ->
// float path).  gfx950 only; 8 channels per lane (data layout: conv_f16.hip).
//
//   upfirdn2d_f16        the generic gather of upfirdn2d.cu:29-92;
//   updn4_f16            the 4x4 filter at up 2 or down 2;
//   fir_same_f16         same-size FIR of any filter size, fir4_march_f16 its marching 4x4 form.
#include <type_traits>
#include "shg_common.h"
#include "conv_f16_p.h"

namespace f16 {

struct UfdH {
    const _Float16* x;
    const float* f;
    _Float16* y;
    int N, C, H, W, OH, OW, fh, fw, upx, upy, dnx, dny, px0, py0, flip;
    float gain;
};

__global__ __launch_bounds__(256) void upfirdn2d_f16_kernel(const UfdH p) {
    __shared__ float sf[64];
    for (int k = threadIdx.x; k < p.fh * p.fw; k += 256) {
        const int ky = k / p.fw, kx = k - ky * p.fw;
        const int sy = p.flip ? ky : p.fh - 1 - ky, sx = p.flip ? kx : p.fw - 1 - kx;
        sf[k] = p.f[sy * p.fw + sx] * p.gain;
    }
    __syncthreads();
    const int c8n = p.C >> 3;
    const long total = (long)p.N * p.OH * p.OW * c8n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c8 = (int)(e % c8n);
        long r = e / c8n;
        const int ox = (int)(r % p.OW);
        r /= p.OW;
        const int oy = (int)(r % p.OH), n = (int)(r / p.OH);
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int ky = 0; ky < p.fh; ++ky) {
            const int uy = oy * p.dny + ky - p.py0;
            if (uy < 0 || (uy % p.upy) != 0) continue;
            const int iy = uy / p.upy;
            if (iy >= p.H) continue;
            for (int kx = 0; kx < p.fw; ++kx) {
                const int ux = ox * p.dnx + kx - p.px0;
                if (ux < 0 || (ux % p.upx) != 0) continue;
                const int ix = ux / p.upx;
                if (ix >= p.W) continue;
                const h8 xv = *(const h8*)(p.x + (((long)n * p.H + iy) * p.W + ix) * p.C + c8 * 8);
                const float fk = sf[ky * p.fw + kx];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] += (float)xv[q] * fk;
            }
        }
        h8 out;
#pragma unroll
        for (int q = 0; q < 8; ++q) out[q] = (_Float16)v[q];
        *(h8*)(p.y + e * 8) = out;
    }
}

// up = down = 1 (the pad-2 pre-filter of the stride-2 layers, the pad-1 post-filter of the transposed convolutions and both their
// gradients -- all but the x2 resampling of the skip paths): a lane produces 2 x 4 adjacent pixels x 8 channels, so that each loaded
// input vector feeds up to 2 x 4 outputs (35 loads per 8 outputs of a 4x4 filter instead of 16 each) and nothing is divided.
// 4x4 filter with up = 2 or down = 2 (the skip branches of the half blocks and their gradients): the factors are compile-time constants (the generic
// kernel above divides by run-time up / down factors per tap and waits for every guarded load), every load is issued unconditionally from a clamped
// address and masked afterwards -- 16 loads per output for down = 2, the 4 taps that hit a real sample for up = 2.
template <int UP, int DN>
__global__ __launch_bounds__(256) void updn4_f16_kernel(const UfdH p) {
    static_assert((UP == 1 && DN == 2) || (UP == 2 && DN == 1), "one factor of two");
    __shared__ float sf[16];
    if (threadIdx.x < 16) {
        const int ky = threadIdx.x >> 2, kx = threadIdx.x & 3;
        sf[threadIdx.x] = p.f[(p.flip ? ky : 3 - ky) * 4 + (p.flip ? kx : 3 - kx)] * p.gain;
    }
    __syncthreads();
    const unsigned c8n = p.C >> 3, total = (unsigned)p.N * p.OH * p.OW * c8n;                  // (host: < 2^31)
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned c8 = e % c8n;
        unsigned r = e / c8n;
        const int ox = r % p.OW;
        r /= p.OW;
        const int oy = r % p.OH, n = r / p.OH;
        const _Float16* xb = p.x + (long)n * p.H * p.W * p.C + c8 * 8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (DN == 2) {
            h8 xin[4][4];
            float m[4][4];
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const int iy = oy * 2 + ky - p.py0, iyc = iy < 0 ? 0 : (iy >= p.H ? p.H - 1 : iy);
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    const int ix = ox * 2 + kx - p.px0, ixc = ix < 0 ? 0 : (ix >= p.W ? p.W - 1 : ix);
                    xin[ky][kx] = *(const h8*)(xb + ((long)iyc * p.W + ixc) * p.C);
                    m[ky][kx] = (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? sf[ky * 4 + kx] : 0.f;
                }
            }
#pragma unroll
            for (int ky = 0; ky < 4; ++ky)
#pragma unroll
                for (int kx = 0; kx < 4; ++kx)
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] += (float)xin[ky][kx][q] * m[ky][kx];
        } else {
            // sample (oy + ky - py0) / 2 exists for the two ky of the right parity
            const int ky0 = (p.py0 - oy) & 1, kx0 = (p.px0 - ox) & 1;
            h8 xin[2][2];
            float m[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int ky = ky0 + 2 * a, uy = oy + ky - p.py0, iy = uy >> 1, iyc = iy < 0 ? 0 : (iy >= p.H ? p.H - 1 : iy);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int kx = kx0 + 2 * b, ux = ox + kx - p.px0, ix = ux >> 1, ixc = ix < 0 ? 0 : (ix >= p.W ? p.W - 1 : ix);
                    xin[a][b] = *(const h8*)(xb + ((long)iyc * p.W + ixc) * p.C);
                    m[a][b] = (uy >= 0 && iy < p.H && ux >= 0 && ix < p.W) ? sf[ky * 4 + kx] : 0.f;
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] += (float)xin[a][b][q] * m[a][b];
        }
        h8 out;
#pragma unroll
        for (int q = 0; q < 8; ++q) out[q] = (_Float16)v[q];
        *(h8*)(p.y + (long)e * 8) = out;
    }
}

// Same-size FIR of any filter size (up to 64 taps), guarded loop; the 4x4 filter of the model takes fir4_march_f16_kernel below.
constexpr int FIR_SAME_RB = 2;                               // output rows per lane
__global__ __launch_bounds__(256) void fir_same_f16_kernel(const UfdH p) {
    constexpr int RB = FIR_SAME_RB;
    __shared__ float sf[64];
    for (int k = threadIdx.x; k < p.fh * p.fw; k += 256) {
        const int ky = k / p.fw, kx = k - ky * p.fw;
        const int sy = p.flip ? ky : p.fh - 1 - ky, sx = p.flip ? kx : p.fw - 1 - kx;
        sf[k] = p.f[sy * p.fw + sx] * p.gain;
    }
    __syncthreads();
    // a lane = 2 rows x 4 columns of outputs x 8 channels: (fh + 1) x (fw + 3) loads feed 8 outputs (4.4 per output for a 4x4 filter)
    const int c8n = p.C >> 3, oxg = (p.OW + 3) >> 2, oyg = (p.OH + RB - 1) / RB;
    const long total = (long)p.N * oyg * oxg * c8n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c8 = (int)(e % c8n);
        long r = e / c8n;
        const int ox0 = (int)(r % oxg) * 4;
        r /= oxg;
        const int oy0 = (int)(r % oyg) * RB, n = (int)(r / oyg);
        float v[RB][4][8];
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 8; ++q) v[b][a][q] = 0.f;
        for (int ry = 0; ry < p.fh + RB - 1; ++ry) {                  // input row oy0 + ry - py0 feeds output row b with tap ky = ry - b
            const int iy = oy0 + ry - p.py0;
            if (iy < 0 || iy >= p.H) continue;
            const _Float16* row = p.x + ((long)n * p.H + iy) * p.W * p.C + c8 * 8;
            for (int cx = 0; cx < p.fw + 3; ++cx) {                   // input column ox0 + cx - px0 feeds output a with tap kx = cx - a
                const int ix = ox0 + cx - p.px0;
                if (ix < 0 || ix >= p.W) continue;
                const h8 xv = *(const h8*)(row + (long)ix * p.C);
                float xf[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) xf[q] = (float)xv[q];
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    const int ky = ry - b;
                    if (ky < 0 || ky >= p.fh) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int kx = cx - a;
                        if (kx < 0 || kx >= p.fw) continue;
                        const float fk = sf[ky * p.fw + kx];
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[b][a][q] += xf[q] * fk;
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            if (oy0 + b >= p.OH) break;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (ox0 + a >= p.OW) break;
                h8 out;
#pragma unroll
                for (int q = 0; q < 8; ++q) out[q] = (_Float16)v[b][a][q];
                *(h8*)(p.y + ((((long)n * p.OH + oy0 + b) * p.OW + ox0 + a) * p.C) + c8 * 8) = out;
            }
        }
    }
}

// Same-size 4x4 FIR, marching: a lane owns TWO adjacent output columns x 8 channels and walks down `rows` output rows.  Per input row it loads
// 5 pixels (2.5 sixteen-byte loads per output piece instead of 4.4), forms the two horizontal 4-tap sums in fp32 and keeps the last four of them in
// registers; an output row is the vertical 4-tap sum of that ring -- 8 multiply-adds per output value instead of 16, written on float2 so that the
// compiler emits packed fp32 math.  The 4x4 filter of the model is an outer product (upfirdn2d.setup_filter of [1,3,3,1]); every thread factors the
// taps itself (pivot row / column) and a filter that is NOT rank one takes the plain 16-tap loop below, same launch.  Column masks are folded into the
// horizontal coefficients once per lane, out-of-range rows are loaded from a clamped address and multiplied by zero.  The 2 x 4-output
// lanes of the unrolled 4x4 form that preceded it spent 206 VALU operations per output piece (105 us of pure issue at 64 ch x 513^2 x 8) and ran
// at 2.3 TB/s.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 hh2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void fir4_march_f16_kernel(const UfdH p, int rows) {
    const int c8n = p.C >> 3, oxg = (p.OW + 1) >> 1, nstrip = (p.OH + rows - 1) / rows;
    const unsigned total = (unsigned)p.N * nstrip * oxg * c8n;
    unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const int c8 = e % c8n;
    e /= c8n;
    const int ox0 = (e % oxg) * 2;
    e /= oxg;
    const int oy0 = (e % nstrip) * rows, n = e / nstrip;
    // taps as the gather form uses them: output (oy, ox) = sum_k t[ky][kx] * x[oy + ky - py0][ox + kx - px0]
    float t[4][4];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) t[ky][kx] = p.f[(p.flip ? ky : 3 - ky) * 4 + (p.flip ? kx : 3 - kx)] * p.gain;
    int pky = 0, pkx = 0;
    float piv = 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx)
            if (fabsf(t[ky][kx]) > fabsf(piv)) { piv = t[ky][kx]; pky = ky; pkx = kx; }
    float fr[4], fc[4];
    bool sep = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) { fr[k] = t[pky][k]; fc[k] = piv != 0.f ? t[k][pkx] / piv : 0.f; }
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) sep = sep && fabsf(t[ky][kx] - fc[ky] * fr[kx]) <= 1e-6f * fabsf(piv);
    const _Float16* xb = p.x + (long)n * p.H * p.W * p.C + c8 * 8;
    _Float16* yb = p.y + (long)n * p.OH * p.OW * p.C + c8 * 8;
    if (!sep) {                                                     // not an outer product: 16 guarded taps per output
        for (int oy = oy0; oy < oy0 + rows && oy < p.OH; ++oy)
            for (int a = 0; a < 2 && ox0 + a < p.OW; ++a) {
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx) {
                        const int iy = oy + ky - p.py0, ix = ox0 + a + kx - p.px0;
                        if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
                        const h8 xv = *(const h8*)(xb + ((long)iy * p.W + ix) * p.C);
#pragma unroll
                        for (int q = 0; q < 8; ++q) acc[q] += (float)xv[q] * t[ky][kx];
                    }
                h8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = (_Float16)acc[q];
                *(h8*)(yb + ((long)oy * p.OW + ox0 + a) * p.C) = o;
            }
        return;
    }
    float cx[2][4];
    int ixc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int ix = ox0 + j - p.px0;
        ixc[j] = (ix < 0 ? 0 : (ix >= p.W ? p.W - 1 : ix)) * p.C;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ix = ox0 + a + k - p.px0;
            cx[a][k] = (ix >= 0 && ix < p.W) ? fr[k] : 0.f;
        }
    f2 h[4][2][4];                                                  // ring of horizontal sums: [input row & 3][column][channel pair]
    auto step = [&](int rr, auto SLOT) __attribute__((always_inline)) {
        constexpr int S = decltype(SLOT)::value;
        const int iy = oy0 + rr - p.py0;
        const float my = (iy >= 0 && iy < p.H) ? 1.f : 0.f;
        const _Float16* row = xb + (long)(iy < 0 ? 0 : (iy >= p.H ? p.H - 1 : iy)) * p.W * p.C;
        h8 xv[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) xv[j] = *(const h8*)(row + ixc[j]);
        f2 xf[5][4];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) { hh2 v = {xv[j][2 * q], xv[j][2 * q + 1]}; xf[j][q] = __builtin_convertvector(v, f2); }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f2 sum = xf[a][q] * cx[a][0];
#pragma unroll
                for (int k = 1; k < 4; ++k) sum += xf[a + k][q] * cx[a][k];
                h[S][a][q] = sum * my;
            }
        const int oy = oy0 + rr - 3;                                // rows oy - py0 + 0..3 = ring slots S+1, S+2, S+3, S
        if (rr >= 3 && oy < p.OH) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                h8 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f2 v = h[(S + 1) & 3][a][q] * fc[0] + h[(S + 2) & 3][a][q] * fc[1] + h[(S + 3) & 3][a][q] * fc[2] + h[S][a][q] * fc[3];
                    const hh2 r = __builtin_convertvector(v, hh2);
                    o[2 * q] = r[0]; o[2 * q + 1] = r[1];
                }
                if (ox0 + a < p.OW) *(h8*)(yb + ((long)oy * p.OW + ox0 + a) * p.C) = o;
            }
        }
    };
    for (int rb = 0; rb < rows + 3; rb += 4) {                      // rows % 4 == 0: the last group has three steps
        step(rb, std::integral_constant<int, 0>{});
        step(rb + 1, std::integral_constant<int, 1>{});
        step(rb + 2, std::integral_constant<int, 2>{});
        if (rb + 3 < rows + 3) step(rb + 3, std::integral_constant<int, 3>{});
    }
}

}  // namespace f16

// upfirdn2d on NHWC halves: the semantics of shg_upfirdn2d_f32 / upfirdn2d.cu:29-92; C % 8 == 0
extern "C" int shg_upfirdn2d_f16(const void* x, const float* f, void* y, int N, int C, int H, int W, int fh, int fw, int upx, int upy, int downx,
                                 int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream) {
    SHG_CHECK_ARG(x && f && y, "upfirdn2d_f16: null pointer");
    SHG_CHECK_ARG(N >= 1 && C >= 8 && (C % 8) == 0 && H >= 1 && W >= 1, "upfirdn2d_f16: bad shape (C must be a multiple of 8)");
    SHG_CHECK_ARG(fh >= 1 && fw >= 1 && fh * fw <= 64 && upx >= 1 && upy >= 1 && downx >= 1 && downy >= 1, "upfirdn2d_f16: bad filter / factors");
    const int OW = (W * upx + padx0 + padx1 - fw + downx) / downx, OH = (H * upy + pady0 + pady1 - fh + downy) / downy;
    SHG_CHECK_ARG(OW >= 1 && OH >= 1, "upfirdn2d_f16: empty output");
    f16::UfdH p{(const _Float16*)x, f, (_Float16*)y, N, C, H, W, OH, OW, fh, fw, upx, upy, downx, downy, padx0, pady0, flip, gain};
    const bool same = upx == 1 && upy == 1 && downx == 1 && downy == 1;
    const int rb = f16::FIR_SAME_RB;                         // (one row per lane was measured too: 287 vs 221 us at 64 ch x 513^2)
    const long total = same ? (long)N * ((OH + rb - 1) / rb) * ((OW + 3) / 4) * (C / 8) : (long)N * OH * OW * (C / 8);
    int grid = shg_cdiv(total, 256);
    if (grid > 256 * 32) grid = 256 * 32;
    if (same && fh == 4 && fw == 4) {
        // marching strips: the longest of 32 / 16 / 8 / 4 rows that still leaves >= 8 workgroups per CU
        int rows = 32;
        auto lanes = [&](int r) { return (long)N * ((OH + r - 1) / r) * ((OW + 1) / 2) * (C / 8); };
        while (rows > 4 && lanes(rows) < 256L * 256 * 8) rows /= 2;
        SHG_CHECK_ARG(lanes(rows) < (1L << 31), "upfirdn2d_f16: tensor too large");
        hipLaunchKernelGGL(f16::fir4_march_f16_kernel, dim3((unsigned)shg_cdiv(lanes(rows), 256)), dim3(256), 0, (hipStream_t)stream, p, rows);
    } else if (same) hipLaunchKernelGGL(f16::fir_same_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (fh == 4 && fw == 4 && upx == 1 && upy == 1 && downx == 2 && downy == 2 && total < (1L << 31))
        hipLaunchKernelGGL((f16::updn4_f16_kernel<1, 2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (fh == 4 && fw == 4 && upx == 2 && upy == 2 && downx == 1 && downy == 1 && total < (1L << 31))
        hipLaunchKernelGGL((f16::updn4_f16_kernel<2, 1>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(f16::upfirdn2d_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
