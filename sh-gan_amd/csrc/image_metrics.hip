// Per-image PSNR and SSIM of an evaluation batch (reference lib/evaluator/eva_psnr.py with for_dataset=None, rgb_range=1, and
// eva_ssim._ssim with size_average=False).  pred, gt [B,C,H,W] contiguous; each operand is uint8 (value = lut[u8]) or float32, then
// an affine map v*scale + bias (the evaluator's `fake/255` and `(real+1)/2`) -- produced in the load, no separate pass.
// Operand precision follows the reference's evaluator batch: PSNR subtracts pred as float64 (numpy `fake/255`; its table is float64)
// from gt as float32; SSIM sees both as float32 (torch.FloatTensor).  With pred == gt up to float32 rounding the PSNR is therefore
// finite (~155 dB), exactly as the reference reports it.
//
// Launch 1 (image_metrics_tile_kernel): one workgroup = one TW x TH output tile of one image, all C channels.  Per channel:
//   stage x, y of the tile + its R-pixel halo into LDS (zero outside the image: F.conv2d's zero padding), and take the squared
//   error of the tile's own pixels (PSNR) in the same load;
//   horizontal pass: the five products (x, y, x^2, y^2, xy) filtered along the row with the 1-D Gaussian -> LDS;
//   vertical pass: the same taps down the column -> mu1, mu2, E[x^2], E[y^2], E[xy] -> the SSIM map value (fp32, the reference's
//   formula in its order).
//   The 2-D window of create_window is the outer product of the 1-D taps, so the separable form computes the same filter with 2(2R+1)
//   instead of (2R+1)^2 taps.  Per-lane sums in fp32, the workgroup's sum in fp64 through a fixed LDS tree -> scratch[b][tile][2].
// Launch 2 (image_metrics_finish_kernel): one workgroup per image adds its tile partials in a fixed order (fp64) and writes
//   psnr = -10 log10(mse) (+inf when mse == 0, as numpy) and the SSIM mean.  No atomics: an image's result does not depend on the
//   batch it sits in or on the run.
#include "shg_common.h"
#include <math.h>

namespace {

constexpr int IM_THREADS = 256;
constexpr int IM_RMAX = 15;           // window_size <= 31
constexpr int IM_TH = 16;

// compile-time radius RC >= 0: the default window (11 -> R = 5), 64-wide tiles; RC < 0: any radius up to IM_RMAX at run time, 32-wide
// tiles (the LDS of the widest halo stays below 64 KiB)
template <int RC> struct ImGeom {
    static constexpr int TW = RC >= 0 ? 64 : 32;
    static constexpr int RL = RC >= 0 ? RC : IM_RMAX;          // radius the LDS is sized for
    static constexpr int SW = TW + 2 * RL;                     // staged row length (allocation)
    static constexpr int SH = IM_TH + 2 * RL;                  // staged / filtered rows (allocation)
};

struct ImTaps { float w[2 * IM_RMAX + 1]; };

struct ImOperand {
    const void* p;
    const void* lut;       // uint8 operands: value table [256] (pred: double, gt: float); NULL: float32 elements
    float scale, bias;
};

__device__ __forceinline__ float im_load(const ImOperand& o, const float* lut_s, long i) {
    const float v = o.lut ? lut_s[reinterpret_cast<const uint8_t*>(o.p)[i]] : reinterpret_cast<const float*>(o.p)[i];
    return fmaf(v, o.scale, o.bias);
}

// pred: the float64 value (PSNR) and its float32 form (SSIM)
__device__ __forceinline__ float im_load_pred(const ImOperand& o, const double* lut_s, long i, double& v64) {
    const double v = o.lut ? lut_s[reinterpret_cast<const uint8_t*>(o.p)[i]] : (double)reinterpret_cast<const float*>(o.p)[i];
    v64 = fma(v, (double)o.scale, (double)o.bias);
    return fmaf((float)v, o.scale, o.bias);
}

// fixed-order fp64 sum of one value per thread (IM_THREADS threads) -> returned in thread 0
__device__ __forceinline__ double im_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = IM_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <int RC>
__global__ __launch_bounds__(IM_THREADS) void image_metrics_tile_kernel(ImOperand pa, ImOperand pb, ImTaps taps, int rr, int C, int H, int W,
                                                                       int tiles_x, int do_ssim, double* part) {
    using G = ImGeom<RC>;
    constexpr int TW = G::TW, TH = IM_TH;
    const int R = RC >= 0 ? RC : rr;
    const int SW = TW + 2 * R, SH = TH + 2 * R;                // this launch's staged tile
    __shared__ float xs[G::SH * G::SW], ys[G::SH * G::SW];
    __shared__ float hs[5][G::SH * TW];
    __shared__ double lut_pred[256];
    __shared__ float lut_gt[256];
    __shared__ double red[IM_THREADS];

    const int t = threadIdx.x;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int x0 = (tile % tiles_x) * TW, y0 = (tile / tiles_x) * TH;
    if (pa.lut) lut_pred[t] = reinterpret_cast<const double*>(pa.lut)[t];
    if (pb.lut) lut_gt[t] = reinterpret_cast<const float*>(pb.lut)[t];
    __syncthreads();

    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float acc_ssim = 0.f, acc_sq = 0.f;
    for (int c = 0; c < C; ++c) {
        const long plane = ((long)b * C + c) * H * W;
        for (int i = t; i < SH * SW; i += IM_THREADS) {
            const int r = i / SW, q = i - r * SW;
            const int gy = y0 - R + r, gx = x0 - R + q;
            float xv = 0.f, yv = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const long off = plane + (long)gy * W + gx;
                double x64;
                xv = im_load_pred(pa, lut_pred, off, x64);
                yv = im_load(pb, lut_gt, off);
                if (r >= R && r < R + TH && q >= R && q < R + TW) {       // a pixel of this tile: its squared error (PSNR)
                    const double d = x64 - (double)yv;
                    acc_sq += (float)(d * d);
                }
            }
            xs[r * SW + q] = xv;
            ys[r * SW + q] = yv;
        }
        __syncthreads();
        if (do_ssim) {
            for (int i = t; i < SH * TW; i += IM_THREADS) {
                const int r = i / TW, q = i - r * TW;
                const float* xr = xs + r * SW + q;
                const float* yr = ys + r * SW + q;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
                if constexpr (RC >= 0) {
#pragma unroll
                    for (int j = 0; j <= 2 * RC; ++j) {
                        const float w = taps.w[j], xv = xr[j], yv = yr[j];
                        s0 += w * xv; s1 += w * yv; s2 += w * (xv * xv); s3 += w * (yv * yv); s4 += w * (xv * yv);
                    }
                } else {
                    for (int j = 0; j <= 2 * R; ++j) {
                        const float w = taps.w[j], xv = xr[j], yv = yr[j];
                        s0 += w * xv; s1 += w * yv; s2 += w * (xv * xv); s3 += w * (yv * yv); s4 += w * (xv * yv);
                    }
                }
                hs[0][i] = s0; hs[1][i] = s1; hs[2][i] = s2; hs[3][i] = s3; hs[4][i] = s4;
            }
            __syncthreads();
        }
        for (int i = t; i < TH * TW; i += IM_THREADS) {
            const int r = i / TW, q = i - r * TW;
            if (!do_ssim || y0 + r >= H || x0 + q >= W) continue;
            float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
            if constexpr (RC >= 0) {
#pragma unroll
                for (int j = 0; j <= 2 * RC; ++j) {
                    const int k = (r + j) * TW + q;
                    const float w = taps.w[j];
                    m1 += w * hs[0][k]; m2 += w * hs[1][k]; e11 += w * hs[2][k]; e22 += w * hs[3][k]; e12 += w * hs[4][k];
                }
            } else {
                for (int j = 0; j <= 2 * R; ++j) {
                    const int k = (r + j) * TW + q;
                    const float w = taps.w[j];
                    m1 += w * hs[0][k]; m2 += w * hs[1][k]; e11 += w * hs[2][k]; e22 += w * hs[3][k]; e12 += w * hs[4][k];
                }
            }
            const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu1_mu2 = m1 * m2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
            acc_ssim += ((2.f * mu1_mu2 + C1) * (2.f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        }
        __syncthreads();              // xs / ys / hs are restaged by the next channel
    }
    const double sq = im_block_sum((double)acc_sq, red);
    const double ss = im_block_sum((double)acc_ssim, red);
    if (t == 0) {
        double* p = part + ((long)b * gridDim.x + tile) * 2;
        p[0] = sq;
        p[1] = ss;
    }
}

__global__ __launch_bounds__(IM_THREADS) void image_metrics_finish_kernel(const double* part, int tiles, double inv_n, double* psnr, double* ssim) {
    __shared__ double red[IM_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* p = part + (long)b * tiles * 2;
    double sq = 0.0, ss = 0.0;
    for (int i = t; i < tiles; i += IM_THREADS) {
        sq += p[2 * i];
        ss += p[2 * i + 1];
    }
    sq = im_block_sum(sq, red);
    ss = im_block_sum(ss, red);
    if (t == 0) {
        const double mse = sq * inv_n;
        if (psnr) psnr[b] = mse == 0.0 ? __builtin_inf() : -10.0 * log10(mse);
        if (ssim) ssim[b] = ss * inv_n;
    }
}

int im_tile_width(int window_size) { return window_size == 11 ? ImGeom<5>::TW : ImGeom<-1>::TW; }

long im_tiles(int H, int W, int window_size) {
    return (long)shg_cdiv(W, im_tile_width(window_size)) * shg_cdiv(H, IM_TH);
}

}  // namespace

extern "C" size_t shg_image_metrics_scratch_bytes(int B, int H, int W, int window_size) {
    if (B < 1 || H < 1 || W < 1 || window_size < 1 || window_size > 2 * IM_RMAX + 1 || window_size % 2 == 0) return 0;
    return (size_t)B * im_tiles(H, W, window_size) * 2 * sizeof(double);
}

extern "C" int shg_image_metrics(const void* pred, const double* pred_lut, float pred_scale, float pred_bias, const void* gt, const float* gt_lut,
                                 float gt_scale, float gt_bias, int B, int C, int H, int W, int window_size, int psnr_only, void* scratch,
                                 size_t scratch_bytes, double* psnr, double* ssim, void* stream) {
    SHG_CHECK_ARG(pred && gt && scratch && psnr, "image_metrics: null pointer");
    SHG_CHECK_ARG(psnr_only || ssim, "image_metrics: null pointer (ssim output)");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1, "image_metrics: B, C, H, W must be >= 1");
    SHG_CHECK_ARG(window_size >= 1 && window_size <= 2 * IM_RMAX + 1 && window_size % 2 == 1,
                  "image_metrics: window_size must be odd and in [1, %d] (got %d)", 2 * IM_RMAX + 1, window_size);
    const long tiles = im_tiles(H, W, window_size);
    SHG_CHECK_ARG(tiles <= 0x7fffffffL && B <= 65535, "image_metrics: image or batch too large");
    SHG_CHECK_ARG(scratch_bytes >= shg_image_metrics_scratch_bytes(B, H, W, window_size),
                  "image_metrics: scratch of %zu bytes is too small (%zu needed)", scratch_bytes, shg_image_metrics_scratch_bytes(B, H, W, window_size));
    // create_window: the 1-D Gaussian (sigma 1.5) in float64, rounded to float32, normalised in float32
    ImTaps taps = {};
    float sum = 0.f;
    const int R = window_size / 2;
    for (int j = 0; j < window_size; ++j) {
        taps.w[j] = (float)exp(-(double)((j - R) * (j - R)) / (2.0 * 1.5 * 1.5));
        sum += taps.w[j];
    }
    for (int j = 0; j < window_size; ++j) taps.w[j] /= sum;
    const ImOperand a = {pred, pred_lut, pred_scale, pred_bias}, g = {gt, gt_lut, gt_scale, gt_bias};
    double* part = reinterpret_cast<double*>(scratch);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
    if (window_size == 11) {
        hipLaunchKernelGGL((image_metrics_tile_kernel<5>), grid, dim3(IM_THREADS), 0, st, a, g, taps, R, C, H, W, shg_cdiv(W, ImGeom<5>::TW),
                           psnr_only ? 0 : 1, part);
    } else {
        hipLaunchKernelGGL((image_metrics_tile_kernel<-1>), grid, dim3(IM_THREADS), 0, st, a, g, taps, R, C, H, W, shg_cdiv(W, ImGeom<-1>::TW),
                           psnr_only ? 0 : 1, part);
    }
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(B), dim3(IM_THREADS), 0, st, part, (int)tiles, 1.0 / ((double)C * H * W), psnr,
                       psnr_only ? nullptr : ssim);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
