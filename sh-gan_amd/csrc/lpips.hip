// LPIPS with the AlexNet backbone (`lpips.LPIPS(net='alex')`, version 0.1, as the reference's lib/evaluator/eva_lpips.py:39-52 calls it):
// the two pieces the FID detector's kernels (inception.hip) do not cover.  conv2..conv5 and the two max pools of AlexNet run on
// shg_inception_conv_f32 / shg_inception_pool_f32; sh-gan_amd/lpips.py drives the whole network.
//
// shg_lpips_conv1_f32: operand load + eva_lpips.py's `(x - 0.5) * 2` + the scaling layer + conv 3 -> 64, 11 x 11, stride 4, pad 2 + bias +
//   ReLU in one launch.  Implicit GEMM on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32), in the detector's layout: rows = the 64
//   output channels (A = packed weight [368][64], K = 363 in tap-major order k = (ky*11 + kx)*3 + c, zero rows up to 368), columns =
//   output pixels m = (b, oy, ox) gathered on the fly; one workgroup = 64 channels x 64 pixels, four waves of 32 x 32, K in 23 steps of
//   16 through two LDS stages.  The scaling layer `(v - shift_c) / scale_c` is applied to the in-bounds taps only -- the convolution's
//   zero padding is of the SCALED image, so the shift cannot move into the bias.  The division is a multiplication by float32(1 /
//   scale_c): at most one ulp of the operand away from the published float32 division.  uint8 operands take the whole per-channel map
//   from a 3 x 256 table a workgroup builds in LDS.
// shg_lpips_head_f32: for one tap, per pixel f^ = f / (sqrt(sum_c f^2) + 1e-10) of both images and d = sum_c w_c (f^_pred - f^_gt)^2;
//   one lane per pixel, both channel sums float32 FMA chains in channel order (the second loop re-reads the wave's 64-pixel columns from
//   cache: each map comes from memory once); a wave's 64 values are added in float64 by a fixed butterfly -> scratch[b][tile]; a second
//   launch adds an image's tiles in a fixed order (float64) and adds the spatial mean to out[b].  No atomics: the same bits run to run
//   and in any batch.  A pixel whose features are all zero gives 0 / (0 + 1e-10) = 0.
// shg_lpips_head_pairs_f32: the same head for a table of P pairs (ia[p], ib[p]) of rows of ONE feature tensor f [M,C,h,w] -- the same
//   per-tile function, the same butterfly, the same finish: a pair's bits are those of shg_lpips_head_f32 on (f[ia], f[ib]) and depend
//   neither on P nor on the pair's place in the table.
#include "det_conv_tile.h"
#include "../../include/shgan_hip.h"

#define LP_K 363                        // 3 * 11 * 11
#define LP_KT ((LP_K + DET_BK - 1) / DET_BK)
#define LP_HEAD_THREADS 256

namespace {

struct LpScale { float shift[3], inv[3]; };     // scaling layer: (v - shift) * inv

// shift, scaling: HOST arrays of 3 floats -> the kernels' form; a scale of 0 is refused
int lp_scale_make(const float* shift, const float* scaling, const char* who, LpScale* s) {
    SHG_CHECK_ARG(scaling[0] != 0.f && scaling[1] != 0.f && scaling[2] != 0.f, "%s: a scaling-layer scale of 0", who);
    for (int c = 0; c < 3; ++c) {
        s->shift[c] = shift[c];
        s->inv[c] = (float)(1.0 / (double)scaling[c]);
    }
    return SHG_OK;
}

struct LpConv1Args {
    const void* x;
    const float* lut;                   // uint8 operands: value of every code after `(x - 0.5) * 2`; NULL: float32 elements
    float scale, bias;                  // float32 operands: u = x*scale + bias (the evaluator batch's [0, 1] form), v = (u - 0.5) * 2
    LpScale s;
    const float* wp;
    const float* bp;
    float* y;
    int B, H, W, OH, OW;
};

__device__ __forceinline__ float lp_scaled(float v, float shift, float inv) { return __fmul_rn(__fsub_rn(v, shift), inv); }

template <bool U8>
__global__ __launch_bounds__(256) void lp_conv1_kernel(const LpConv1Args a) {
    __shared__ float Ws[2][DET_BK][DET_BM];
    __shared__ float Xs[2][DET_BK][DET_BN];
    __shared__ float lut3[U8 ? 3 * 256 : 1];
    const DetRoles t = det_roles();
    if (U8) {
        const int tid = threadIdx.x;
        const float v = a.lut[tid];
#pragma unroll
        for (int c = 0; c < 3; ++c) lut3[c * 256 + tid] = lp_scaled(v, a.s.shift[c], a.s.inv[c]);
        __syncthreads();
    }
    const int OHW = a.OH * a.OW, M = a.B * OHW;
    const int m = (int)blockIdx.x * DET_BN + t.px;
    const bool mvalid = m < M;
    int b = 0, oy = 0, ox = 0;
    if (mvalid) {
        b = m / OHW;
        const int r = m - b * OHW;
        oy = r / a.OW;
        ox = r - oy * a.OW;
    }
    const int iy0 = oy * 4 - 2, ix0 = ox * 4 - 2;
    const long HW = (long)a.H * a.W;
    const long xb = (long)b * 3 * HW;
    const float* wp = a.wp + t.wc;
    const uint8_t* x8 = reinterpret_cast<const uint8_t*>(a.x);

    const f32x16 acc = det_conv_tile(Ws, Xs, 0, LP_KT, [&](int kt, float (&xr)[4], float4& wreg) {
        wreg = *reinterpret_cast<const float4*>(wp + (long)(kt * DET_BK + t.wr) * DET_BM);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kt * DET_BK + t.kr0 + 4 * i;
            xr[i] = 0.f;
            if (mvalid && k < LP_K) {
                const int tap = k / 3, c = k - tap * 3;
                const int ky = tap / 11, kx = tap - ky * 11;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const long idx = xb + (long)c * HW + (long)iy * a.W + ix;
                    if (U8) {
                        xr[i] = lut3[c * 256 + x8[idx]];
                    } else {
                        const float u = det_value(a.x, nullptr, a.scale, a.bias, idx);
                        const float sh = c == 0 ? a.s.shift[0] : (c == 1 ? a.s.shift[1] : a.s.shift[2]);
                        const float iv = c == 0 ? a.s.inv[0] : (c == 1 ? a.s.inv[1] : a.s.inv[2]);
                        xr[i] = lp_scaled(__fmul_rn(__fsub_rn(u, 0.5f), 2.f), sh, iv);
                    }
                }
            }
        }
    });

    const int mo = (int)blockIdx.x * DET_BN + t.wn + t.lj;
    if (mo >= M) return;
    const int bo = mo / OHW, pix = mo - bo * OHW;
    float* yb = a.y + (long)bo * DET_BM * OHW + pix;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = t.wm + t.row(r);
        yb[(long)o * OHW] = fmaxf(acc[r] + a.bp[o], 0.f);
    }
}

// one 64-pixel tile of one (pred, gt) pair of maps: the wave's float64 sum of d over its pixels (the same value in every lane)
__device__ __forceinline__ double lp_head_tile(const float* p, const float* g, const float* w, int C, int HW, int pix) {
    float d = 0.f;
    if (pix < HW) {
        p += pix;
        g += pix;
        float sp = 0.f, sg = 0.f;
        for (int c = 0; c < C; ++c) {
            const float u = p[(long)c * HW], v = g[(long)c * HW];
            sp = fmaf(u, u, sp);
            sg = fmaf(v, v, sg);
        }
        const float np = sqrtf(sp) + 1e-10f, ng = sqrtf(sg) + 1e-10f;
        for (int c = 0; c < C; ++c) {
            const float diff = __fsub_rn(p[(long)c * HW] / np, g[(long)c * HW] / ng);
            d = fmaf(w[c], __fmul_rn(diff, diff), d);
        }
    }
    double s = (double)d;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__global__ __launch_bounds__(64) void lp_head_tile_kernel(const float* fp, const float* fg, const float* w, int C, int HW, double* part) {
    const int lane = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const double s = lp_head_tile(fp + (long)b * C * HW, fg + (long)b * C * HW, w, C, HW, tile * 64 + lane);
    if (lane == 0) part[(long)b * gridDim.x + tile] = s;
}

// the same tile for pair p of a table: both maps are rows of ONE feature tensor f [M,C,h,w].  An index outside [0, M) is clamped into
// it (no read leaves f) and reported through *err (every reporter stores the same 1).
__global__ __launch_bounds__(64) void lp_head_pairs_tile_kernel(const float* f, const int* ia, const int* ib, const float* w, int M, int C, int HW,
                                                                double* part, int* err) {
    const int lane = threadIdx.x, tile = blockIdx.x, p = blockIdx.y;
    int a = ia[p], b = ib[p];
    if (a < 0 || a >= M || b < 0 || b >= M) {
        a = min(max(a, 0), M - 1);
        b = min(max(b, 0), M - 1);
        if (err && lane == 0 && tile == 0) *err = 1;
    }
    const double s = lp_head_tile(f + (long)a * C * HW, f + (long)b * C * HW, w, C, HW, tile * 64 + lane);
    if (lane == 0) part[(long)p * gridDim.x + tile] = s;
}

__global__ __launch_bounds__(LP_HEAD_THREADS) void lp_head_finish_kernel(const double* part, int tiles, double inv_hw, double* out) {
    __shared__ double red[LP_HEAD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* p = part + (long)b * tiles;
    double s = 0.0;
    for (int i = t; i < tiles; i += LP_HEAD_THREADS) s += p[i];
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int k = LP_HEAD_THREADS / 2; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) out[b] += red[0] * inv_hw;
}

}  // namespace

extern "C" int shg_lpips_conv1_weight_prep_f32(const float* w, const float* bias, float* wp, float* bp, void* stream) {
    SHG_CHECK_ARG(w && bias && wp && bp, "lpips_conv1_weight_prep: null pointer");
    return shg_det_weight_prep(w, bias, wp, bp, DET_BM, 3, 11, 11, (hipStream_t)stream);      // the detector's packing: [368][64], bp [64]
}

extern "C" int shg_lpips_conv1_f32(const void* x, const float* lut, float scale, float bias, const float* shift, const float* scaling,
                                   const float* wp, const float* bp, float* y, int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && shift && scaling && wp && bp && y, "lpips_conv1: null pointer");
    SHG_CHECK_ARG(((uintptr_t)wp & 15) == 0, "lpips_conv1: packed weight not 16-byte aligned");
    SHG_CHECK_ARG(B >= 1 && H >= 7 && W >= 7 && H <= 65536 && W <= 65536, "lpips_conv1: bad geometry B %d %dx%d (B >= 1, H and W >= 7)", B, H, W);
    LpConv1Args a;
    const int rc = lp_scale_make(shift, scaling, "lpips_conv1", &a.s);
    if (rc) return rc;
    a.x = x; a.lut = lut; a.scale = scale; a.bias = bias; a.wp = wp; a.bp = bp; a.y = y;
    a.B = B; a.H = H; a.W = W;
    a.OH = (H + 4 - 11) / 4 + 1;
    a.OW = (W + 4 - 11) / 4 + 1;
    const long M = (long)B * a.OH * a.OW;
    SHG_CHECK_ARG(M * DET_BM < (1L << 31), "lpips_conv1: tensor too large for 32-bit pixel indices");
    const dim3 grid((unsigned)((M + DET_BN - 1) / DET_BN));
    if (lut) hipLaunchKernelGGL((lp_conv1_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lp_conv1_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" size_t shg_lpips_head_scratch_bytes(int B, int h, int w) {
    if (B < 1 || h < 1 || w < 1) return 0;
    return (size_t)B * (size_t)(((long)h * w + 63) / 64) * sizeof(double);
}

extern "C" int shg_lpips_head_f32(const float* fp, const float* fg, const float* w, int B, int C, int h, int wd, void* scratch, size_t scratch_bytes,
                                  double* out, void* stream) {
    SHG_CHECK_ARG(fp && fg && w && scratch && out, "lpips_head: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && h >= 1 && wd >= 1, "lpips_head: B, C, h, w must be >= 1");
    const long HW = (long)h * wd, tiles = (HW + 63) / 64;
    SHG_CHECK_ARG(HW < (1L << 31) && B <= 65535, "lpips_head: feature map or batch too large");
    SHG_CHECK_ARG(scratch_bytes >= shg_lpips_head_scratch_bytes(B, h, wd), "lpips_head: scratch of %zu bytes is too small (%zu needed)", scratch_bytes,
                  shg_lpips_head_scratch_bytes(B, h, wd));
    double* part = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(lp_head_tile_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(64), 0, (hipStream_t)stream, fp, fg, w, C, (int)HW, part);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(lp_head_finish_kernel, dim3(B), dim3(LP_HEAD_THREADS), 0, (hipStream_t)stream, part, (int)tiles, 1.0 / (double)HW, out);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// Pair form of the head (diversity.py: the K(K-1)/2 pairs among the K samples of one input after ONE trunk pass over all of them).
extern "C" size_t shg_lpips_head_pairs_scratch_bytes(int P, int h, int w) { return shg_lpips_head_scratch_bytes(P, h, w); }

extern "C" int shg_lpips_head_pairs_f32(const float* f, const int* ia, const int* ib, const int* ia_host, const int* ib_host, const float* w, int M, int P,
                                        int C, int h, int wd, void* scratch, size_t scratch_bytes, double* out, int* err, void* stream) {
    SHG_CHECK_ARG(f && ia && ib && w && scratch && out, "lpips_head_pairs: null pointer");
    SHG_CHECK_ARG((ia_host == nullptr) == (ib_host == nullptr), "lpips_head_pairs: pass both host tables or neither");
    SHG_CHECK_ARG(M >= 1 && P >= 1 && C >= 1 && h >= 1 && wd >= 1, "lpips_head_pairs: M, P, C, h, w must be >= 1");
    const long HW = (long)h * wd, tiles = (HW + 63) / 64;
    SHG_CHECK_ARG(HW < (1L << 31) && P <= 65535, "lpips_head_pairs: feature map or pair table too large");
    SHG_CHECK_ARG(scratch_bytes >= shg_lpips_head_pairs_scratch_bytes(P, h, wd), "lpips_head_pairs: scratch of %zu bytes is too small (%zu needed)",
                  scratch_bytes, shg_lpips_head_pairs_scratch_bytes(P, h, wd));
    if (ia_host)
        for (int p = 0; p < P; ++p)
            SHG_CHECK_ARG(ia_host[p] >= 0 && ia_host[p] < M && ib_host[p] >= 0 && ib_host[p] < M, "lpips_head_pairs: pair %d = (%d, %d) is outside [0, %d)", p,
                          ia_host[p], ib_host[p], M);
    double* part = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(lp_head_pairs_tile_kernel, dim3((unsigned)tiles, (unsigned)P), dim3(64), 0, (hipStream_t)stream, f, ia, ib, w, M, C, (int)HW, part,
                       err);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(lp_head_finish_kernel, dim3(P), dim3(LP_HEAD_THREADS), 0, (hipStream_t)stream, part, (int)tiles, 1.0 / (double)HW, out);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- the scaling layer as a pass of its own, for a backbone whose first convolution is not conv1 above (net = 'vgg': its 3 x 3
// convolutions run on the detector's kernel, which takes a finished float32 image).  Same operand forms and the same float32 steps as
// conv1's load: v = lut[x] or ((x*scale + bias) - 0.5) * 2, then (v - shift_c) * float32(1 / scaling_c).
namespace {
template <bool U8>
__global__ __launch_bounds__(256) void lp_scaling_kernel(const void* x, const float* lut, float scale, float bias, LpScale k, float* y, long n,
                                                         long HW) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int c = (int)((e / HW) % 3);
    float v = det_value(x, U8 ? lut : nullptr, scale, bias, e);
    if (!U8) v = __fmul_rn(__fsub_rn(v, 0.5f), 2.f);
    y[e] = lp_scaled(v, k.shift[c], k.inv[c]);
}
}  // namespace

extern "C" int shg_lpips_scaling_f32(const void* x, const float* lut, float scale, float bias, const float* shift, const float* scaling, float* y,
                                     int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && shift && scaling && y, "lpips_scaling: null pointer");
    SHG_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && (long)B * 3 * H * W < (1L << 38), "lpips_scaling: bad geometry B %d %dx%d",
                  B, H, W);
    LpScale k;
    const int rc = lp_scale_make(shift, scaling, "lpips_scaling", &k);
    if (rc) return rc;
    const long HW = (long)H * W, n = (long)B * 3 * HW;
    const dim3 grid((unsigned)shg_cdiv(n, 256));
    if (lut) hipLaunchKernelGGL((lp_scaling_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x, lut, scale, bias, k, y, n, HW);
    else hipLaunchKernelGGL((lp_scaling_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x, lut, scale, bias, k, y, n, HW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
