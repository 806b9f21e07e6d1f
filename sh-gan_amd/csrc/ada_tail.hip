// The tail of the ADA augmentation pipe (StyleGAN2-ADA's AugmentPipe after the colour stage): image-space filter, additive noise, cutout.
//
// ADA's sequence is   gains g [N,4] from four gated log-normal draws -> Hz' = g @ Hz_fbank [N,43] -> reflect-pad by 21 -> conv2d along x
// with Hz' -> conv2d along y with Hz' (both per sample, correlations)   then   x += sigma_n z   then   x *= [outside the cutout box].  Here
//   * ada_tail_params_kernel: one workgroup turns the draws (ut [N,8] uniform, gt [N,5] normal; column layout in sh-gan_amd/ada.py) and the
//     probability p (device memory) into Hz' [N,43], sigma [N] and the box {cx, cy, half_w, half_h} [N,4].  float64 arithmetic, rounded to
//     float32 once.  The 4 x 43 bank (sym2 -> Hz_lo2, Hz_hi2 -> three zero-stuff / convolve / add rounds) is built by the compiler in double
//     (TT_BANK).  A sample none of whose band gates fired gets the exact unit impulse, not ADA's impulse + 1e-12.
//   * ada_tail_kernel<false>: y = mask * (fir(x) + sigma z) on the colour channels, y = mask * x on the others, one launch.  A workgroup owns a
//     64 x 32 output tile of one (sample, channel) plane, so the 43 taps are wave-uniform (scalar registers).  The 106 x 74 source window is
//     staged in LDS with the reflection folded into the load index; the x pass (16 outputs per thread from a sliding window of 58 LDS reads)
//     writes a 106 x 32 LDS intermediate, the y pass (8 outputs per thread, 50 reads) ends in the noise term, the mask and the one store.
//     Neither the padded tensor nor the x-pass result exists in memory.  46 KiB of LDS: three workgroups per CU.  A plane that is not
//     filtered (another channel, a null Hz, a sample whose taps are the exact impulse) is copied through the noise and mask terms.
//   * ada_tail_kernel<true>: gx = A^T gy, A the linear part (mask * fir).  A is not self-adjoint: the reflected pad folds back.  Written as
//     a gather with the same tiling: the window holds the masked, ZERO-extended cotangent, the taps are flipped, and per axis an output j
//     adds to its own correlation c[j] the folded ones c[-j] (1 <= j <= 21) and c[2 (n - 1) - j] (n - 22 <= j <= n - 2), whose operands lie
//     inside the same window (n >= 22: one fold).  No atomics: the same bits on every run.
// Every source index is clamped into the image; outputs past the image are computed and not stored.
#include "shg_common.h"
#include "../../include/shgan_hip.h"

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_K = 43, TT_P = 21;              // taps, pad
constexpr int TT_H = 64, TT_W = 32;              // output tile
constexpr int TT_SH = TT_H + 2 * TT_P;           // 106 window rows
constexpr int TT_SW = TT_W + 2 * TT_P;           // 74 window columns
// LDS pitches.  A ds_read_b32 / ds_write_b32 is served per 32-lane half of the wave over 32 banks (bank = dword address mod 32; lanes l and
// l + 32 never conflict).  x pass: a half holds 16 consecutive rows r x 2 column groups g and reads dword 75 r + 16 g + t: 75 r mod 32 =
// 11 r mod 32 and 16 = 11 * 16 mod 32, so the 32 lanes sit on 11 (r + 16 g) mod 32, 32 distinct banks.  Its writes 33 r + 16 g + j are
// r + 16 g mod 32, distinct as well.  y pass: a half holds ONE group of rows and 32 consecutive columns, i.e. consecutive banks.
constexpr int TT_SPITCH = TT_SW + 1;             // 75
constexpr int TT_MPITCH = TT_W + 1;              // 33
constexpr int TT_RX = 16, TT_RY = 8;             // outputs per thread of the x pass / the y pass
constexpr int TT_NU = 8, TT_NG = 5;              // draw columns

// ------------------------------------------------------------------------------------------------ the filter bank, in double
struct TtBank {
    double v[4][TT_K];
};
constexpr TtBank tt_bank() {
    const double lo[4] = {-0.12940952255092145, 0.22414386804185735, 0.836516303737469, 0.48296291314469025};      // sym2
    double lo2[7] = {}, hi2[7] = {};
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {            // conv(f, reversed f)
            const double ha = (a & 1) ? -lo[a] : lo[a], hc = ((3 - c) & 1) ? -lo[3 - c] : lo[3 - c];
            lo2[a + c] += lo[a] * lo[3 - c];
            hi2[a + c] += ha * hc;
        }
    for (int t = 0; t < 7; ++t) lo2[t] /= 2, hi2[t] /= 2;
    TtBank cur{};
    cur.v[0][0] = 1.0;
    int len = 1;
    for (int i = 1; i < 4; ++i) {
        TtBank nxt{};
        for (int r = 0; r < 4; ++r)              // zero-stuffed (last zero dropped) row, convolved with Hz_lo2
            for (int j = 0; j < len; ++j)
                for (int t = 0; t < 7; ++t) nxt.v[r][2 * j + t] += cur.v[r][j] * lo2[t];
        len = 2 * len - 1 + 6;
        for (int t = 0; t < 7; ++t) nxt.v[i][(len - 7) / 2 + t] += hi2[t];
        cur = nxt;
    }
    return cur;
}
__device__ constexpr TtBank TT_BANK = tt_bank();

// ------------------------------------------------------------------------------------------------ parameters
__global__ __launch_bounds__(TT_THREADS) void ada_tail_params_kernel(const float* __restrict__ ut, const float* __restrict__ gt,
                                                                     const float* __restrict__ p, shg_ada_tail_config cf,
                                                                     float* __restrict__ Hz, float* __restrict__ sigma, float* __restrict__ cut,
                                                                     int N) {
    const double P = (double)p[0];
    const double ep[4] = {10.0 / 13.0, 1.0 / 13.0, 1.0 / 13.0, 1.0 / 13.0};          // ADA's expected power per band
    for (int n = threadIdx.x; n < N; n += TT_THREADS) {
        const float* un = ut + (long)n * TT_NU;
        const float* gn = gt + (long)n * TT_NG;
        double g[4] = {1.0, 1.0, 1.0, 1.0};
        bool any = false;
        for (int i = 0; i < 4; ++i) {
            const bool fired = (double)un[i] < (double)cf.imgfilter * P * (double)cf.bands[i];
            const double ti = fired ? exp2((double)gn[i] * (double)cf.imgfilter_std) : 1.0;
            any = any || fired;
            double t[4] = {1.0, 1.0, 1.0, 1.0};
            t[i] = ti;
            double s = 0.0;
            for (int b = 0; b < 4; ++b) s += ep[b] * t[b] * t[b];
            s = sqrt(s);
            for (int b = 0; b < 4; ++b) g[b] *= t[b] / s;
        }
        for (int k = 0; k < TT_K; ++k) {
            double h = 0.0;
            for (int b = 0; b < 4; ++b) h += g[b] * TT_BANK.v[b][k];
            Hz[(long)n * TT_K + k] = any ? (float)h : (k == TT_P ? 1.f : 0.f);
        }
        {   // noise
            const bool fired = (double)un[4] < (double)cf.noise * P;
            sigma[n] = fired ? (float)(fabs((double)gn[4]) * (double)cf.noise_std) : 0.f;
        }
        {   // cutout: ADA compares in float32 against size / 2
            const bool fired = (double)un[5] < (double)cf.cutout * P;
            const float half = fired ? cf.cutout_size * 0.5f : 0.f;
            cut[(long)n * 4 + 0] = un[6], cut[(long)n * 4 + 1] = un[7], cut[(long)n * 4 + 2] = half, cut[(long)n * 4 + 3] = half;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the image operator and its transpose
__device__ __forceinline__ int tt_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// 1 outside the box, 0 inside: ADA's two float32 compares
__device__ __forceinline__ float tt_mask(const float* __restrict__ cn, int gy, int gx, int H, int W) {
    if (!cn) return 1.f;
    const bool mx = fabsf(__fdiv_rn((float)gx + 0.5f, (float)W) - cn[0]) >= cn[2];
    const bool my = fabsf(__fdiv_rn((float)gy + 0.5f, (float)H) - cn[1]) >= cn[3];
    return (mx || my) ? 1.f : 0.f;
}

// The folded correlations of output i (global index on an axis of n) of the transpose: line[(q - base) * stride] holds the zero-extended
// cotangent at global index q, sk the flipped taps.
__device__ __forceinline__ float tt_fold(const float* line, int stride, int span, int i, int n, int base, const float* sk) {
    float e = 0.f;
    if (i >= 1 && i <= TT_P)                       // c[-i]: operands q = s - 21 - i >= 0
        for (int s = TT_P + i; s < TT_K; ++s) {
            const int at = min(max(s - TT_P - i - base, 0), span - 1);
            e = __builtin_fmaf(sk[s], line[at * stride], e);
        }
    if (i >= n - TT_P - 1 && i <= n - 2)           // c[2 (n - 1) - i]: operands q = 2 (n - 1) - i + s - 21 <= n - 1
        for (int s = 0; s <= i + TT_P + 1 - n; ++s) {
            const int at = min(max(2 * (n - 1) - i + s - TT_P - base, 0), span - 1);
            e = __builtin_fmaf(sk[s], line[at * stride], e);
        }
    return e;
}

template <bool ADJ>
__global__ __launch_bounds__(TT_THREADS) void ada_tail_kernel(const float* __restrict__ x, const float* __restrict__ Hz,
                                                              const float* __restrict__ sigma, const float* __restrict__ z,
                                                              const float* __restrict__ cut, float* __restrict__ y, int C, int H, int W, int cf,
                                                              int cc, int tiles_x, int tiles_y) {
    __shared__ float S[TT_SH * TT_SPITCH];
    __shared__ float M[TT_SH * TT_MPITCH];
    __shared__ float sk[TT_K];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TT_W;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TT_H;
    const int pl = b / tiles_y, n = pl / C, c = pl - n * C;
    const bool colour = c >= cf && c < cf + cc;
    const long plane = (long)H * W;
    const float* xp = x + (long)pl * plane;
    float* yp = y + (long)pl * plane;
    const float* cn = cut ? cut + (long)n * 4 : nullptr;
    const float* zp = (!ADJ && z && colour) ? z + ((long)n * cc + (c - cf)) * plane : nullptr;
    const float sg = zp ? sigma[n] : 0.f;

    float k[TT_K];                                   // wave-uniform: the taps of this sample (flipped for the transpose)
    bool fir = Hz != nullptr && colour;
    if (fir) {
        const float* hn = Hz + (long)n * TT_K;
        bool impulse = true;
#pragma unroll
        for (int t = 0; t < TT_K; ++t) {
            k[t] = hn[ADJ ? TT_K - 1 - t : t];
            impulse = impulse && k[t] == (t == TT_P ? 1.f : 0.f);
        }
        fir = !impulse;
    }
    if (!fir) {                                      // no filter on this plane: its bits pass through the noise and mask terms
        for (int e = tid; e < TT_H * TT_W; e += TT_THREADS) {
            const int gy = ty0 + e / TT_W, gx = tx0 + e % TT_W;
            if (gy < H && gx < W) {
                const long at = (long)gy * W + gx;
                float v = xp[at];
                if (zp) v = __builtin_fmaf(sg, zp[at], v);
                if (cn) v *= tt_mask(cn, gy, gx, H, W);
                yp[at] = v;
            }
        }
        return;
    }

    if (ADJ && tid < TT_K) sk[tid] = Hz[(long)n * TT_K + TT_K - 1 - tid];
    for (int e = tid; e < TT_SH * TT_SW; e += TT_THREADS) {
        const int r = e / TT_SW, q = e - r * TT_SW;
        const int gy = ty0 - TT_P + r, gx = tx0 - TT_P + q;
        float v;
        if (ADJ) {                                   // the masked cotangent, zero outside the image
            v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                v = xp[(long)gy * W + gx];
                if (cn) v *= tt_mask(cn, gy, gx, H, W);
            }
        } else {
            v = xp[(long)tt_reflect(gy, H) * W + tt_reflect(gx, W)];
        }
        S[r * TT_SPITCH + q] = v;
    }
    __syncthreads();

    // along x: M[r][o] = sum_t k[t] S[r][o + t], for the window rows that outputs inside the image read
    // (at most 212 items of 16 outputs for 256 threads: one round with 44 threads idle; 8 outputs per item would take two rounds)
    const int rows = min(TT_SH, H - ty0 + 2 * TT_P);
    for (int e = tid; e < rows * (TT_W / TT_RX); e += TT_THREADS) {
        const int r = e / (TT_W / TT_RX), o0 = (e % (TT_W / TT_RX)) * TT_RX;
        const float* line = S + r * TT_SPITCH;
        float acc[TT_RX];
#pragma unroll
        for (int j = 0; j < TT_RX; ++j) acc[j] = 0.f;
#pragma unroll
        for (int t = 0; t < TT_K + TT_RX - 1; ++t) {
            const float v = line[o0 + t];
#pragma unroll
            for (int j = 0; j < TT_RX; ++j)
                if (t - j >= 0 && t - j < TT_K) acc[j] = __builtin_fmaf(k[t - j], v, acc[j]);
        }
        if (ADJ) {
#pragma unroll
            for (int j = 0; j < TT_RX; ++j) {
                const int i = tx0 + o0 + j;
                if (i < W && (i <= TT_P || i >= W - TT_P - 1)) acc[j] += tt_fold(line, 1, TT_SW, i, W, tx0 - TT_P, sk);
            }
        }
#pragma unroll
        for (int j = 0; j < TT_RX; ++j) M[r * TT_MPITCH + o0 + j] = acc[j];
    }
    __syncthreads();

    // along y: out[o][x] = sum_t k[t] M[o + t][x]
    {
        const int ox = tid % TT_W, o0 = (tid / TT_W) * TT_RY;
        const int gx = tx0 + ox;
        if (gx >= W || ty0 + o0 >= H) return;
        const float* line = M + ox;
        float acc[TT_RY];
#pragma unroll
        for (int j = 0; j < TT_RY; ++j) acc[j] = 0.f;
#pragma unroll
        for (int t = 0; t < TT_K + TT_RY - 1; ++t) {
            const float v = line[(o0 + t) * TT_MPITCH];
#pragma unroll
            for (int j = 0; j < TT_RY; ++j)
                if (t - j >= 0 && t - j < TT_K) acc[j] = __builtin_fmaf(k[t - j], v, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < TT_RY; ++j) {
            const int gy = ty0 + o0 + j;
            if (gy >= H) break;                      // (acc of the rows past the image came from rows of M the x pass skipped: not stored)
            const long at = (long)gy * W + gx;
            float v = acc[j];
            if (ADJ) {
                if (gy <= TT_P || gy >= H - TT_P - 1) v += tt_fold(line, TT_MPITCH, TT_SH, gy, H, ty0 - TT_P, sk);
            } else {
                if (zp) v = __builtin_fmaf(sg, zp[at], v);
                if (cn) v *= tt_mask(cn, gy, gx, H, W);
            }
            yp[at] = v;
        }
    }
}

int tt_check(const char* name, const void* x, const void* Hz, const void* cut, const void* y, int N, int C, int H, int W, int cf, int cc,
             long* blocks, int* tiles_x, int* tiles_y) {
    SHG_CHECK_ARG(x && y && x != y, "%s: null or aliased image pointer", name);
    SHG_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: N, C, H, W must be >= 1 (got %d, %d, %d, %d)", name, N, C, H, W);
    SHG_CHECK_ARG(H <= 16384 && W <= 16384, "%s: H, W <= 16384 (got %d x %d)", name, H, W);
    SHG_CHECK_ARG(cc >= 0 && (cc == 0 || (cf >= 0 && cf + cc <= C)), "%s: colour channels [%d, %d) lie outside the %d channels", name, cf, cf + cc, C);
    SHG_CHECK_ARG(!Hz || cc > 0, "%s: the filter needs colour channels (color_count = 0)", name);
    SHG_CHECK_ARG(!Hz || (H > TT_P && W > TT_P), "%s: the image filter reflect-pads by %d and needs H, W >= %d (got %d x %d)", name, TT_P,
                  TT_P + 1, H, W);
    *tiles_x = shg_cdiv(W, TT_W), *tiles_y = shg_cdiv(H, TT_H);
    *blocks = (long)N * C * *tiles_x * *tiles_y;
    SHG_CHECK_ARG(*blocks <= 2147483647L, "%s: %ld tiles exceed the grid (N * C = %ld planes of %d x %d)", name, *blocks, (long)N * C, H, W);
    return SHG_OK;
}

}  // namespace

extern "C" int shg_ada_tail_params_f32(const float* ut, const float* gt, const float* p, const shg_ada_tail_config* cfg, float* Hz, float* sigma,
                                       float* cut, int N, void* stream) {
    SHG_CHECK_ARG(ut && gt && p && cfg && Hz && sigma && cut, "ada_tail_params_f32: null pointer");
    SHG_CHECK_ARG(N >= 1 && N <= (1 << 20), "ada_tail_params_f32: N in [1, 2^20] (got %d)", N);
    hipLaunchKernelGGL(ada_tail_params_kernel, dim3(1), dim3(TT_THREADS), 0, (hipStream_t)stream, ut, gt, p, *cfg, Hz, sigma, cut, N);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_ada_tail_apply_f32(const float* x, const float* Hz, const float* sigma, const float* z, const float* cut, float* y, int N,
                                      int C, int H, int W, int color_first, int color_count, int bias, void* stream) {
    long blocks;
    int tiles_x, tiles_y;
    const int rc = tt_check("ada_tail_apply_f32", x, Hz, cut, y, N, C, H, W, color_first, color_count, &blocks, &tiles_x, &tiles_y);
    if (rc != SHG_OK) return rc;
    SHG_CHECK_ARG((z != nullptr) == (sigma != nullptr), "ada_tail_apply_f32: the noise needs both sigma and z");
    SHG_CHECK_ARG(!z || color_count > 0, "ada_tail_apply_f32: the noise needs colour channels (color_count = 0)");
    if (!bias) z = nullptr;
    SHG_CHECK_ARG(Hz || z || cut, "ada_tail_apply_f32: nothing to do (no filter, no noise, no cutout)");
    hipLaunchKernelGGL(ada_tail_kernel<false>, dim3((unsigned)blocks), dim3(TT_THREADS), 0, (hipStream_t)stream, x, Hz, sigma, z, cut, y, C, H, W,
                       color_count ? color_first : 0, color_count, tiles_x, tiles_y);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_ada_tail_adjoint_f32(const float* gy, const float* Hz, const float* cut, float* gx, int N, int C, int H, int W,
                                        int color_first, int color_count, void* stream) {
    long blocks;
    int tiles_x, tiles_y;
    const int rc = tt_check("ada_tail_adjoint_f32", gy, Hz, cut, gx, N, C, H, W, color_first, color_count, &blocks, &tiles_x, &tiles_y);
    if (rc != SHG_OK) return rc;
    SHG_CHECK_ARG(Hz || cut, "ada_tail_adjoint_f32: nothing to do (no filter, no cutout)");
    hipLaunchKernelGGL(ada_tail_kernel<true>, dim3((unsigned)blocks), dim3(TT_THREADS), 0, (hipStream_t)stream, gy, Hz, nullptr, nullptr, cut, gx,
                       C, H, W, color_count ? color_first : 0, color_count, tiles_x, tiles_y);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
