// Front end of the perceptual path length (`ppl2_wend`, the reference's lib/evaluator/stylegan_metrics/perceptual_path_length.py:71-85;
// sh-gan_amd/ppl.py drives this file): centre crop, box downsample to 256, [-1, 1] -> [0, 255], grey -> three channels and the
// detector's normalisation in ONE pass over the synthesis output, where the reference makes four torch passes.  A bandwidth kernel:
// every element of the cropped x is read once, every element of y is written once, no LDS, no atomics.
//
// Arithmetic per output element: m = float32(sum of the f x f box / (f*f)) with the sum held in float64 (the correctly rounded float32
// mean up to a double rounding, whatever order a float32 reduction would have taken; f = 1: m = x), then the reference's float32 steps
// u = (m + 1) * 127.5 and the detector's (u - mean_c) / std_c, each rounded once.
#include "shg_common.h"

namespace {

struct PplArgs {
    const float* x;
    float* y;
    int N, C, R, S, f, y0, x0;          // x [N,C,R,R]; window rows y0.., columns x0.., side S*f; y [N,3,S,S]
    float mean[3], stdv[3];
};

__device__ __forceinline__ float ppl_value(double sum, double cnt, float mean, float stdv) {
    const float m = (float)(sum / cnt);
    const float u = __fmul_rn(__fadd_rn(m, 1.f), 127.5f);
    return __fdiv_rn(__fsub_rn(u, mean), stdv);
}

// One thread per group of GW consecutive output pixels of one row and one INPUT channel (a grey image's thread writes all three output
// channels).  VEC: f = 4 / GW in {1, 2, 4}, every box row of the group is one aligned float4 and the group is one aligned GW-float store.
// Otherwise GW = 1 and the f x f box is read element by element (any factor, any alignment).  Boxes are added row by row, left to right.
template <int GW, bool VEC>
__global__ __launch_bounds__(256) void ppl_frontend_kernel(const PplArgs a) {
    const int G = (a.S + GW - 1) / GW;
    const long total = (long)a.N * a.C * a.S * G;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int gx = (int)(e % G);
    long t = e / G;
    const int oy = (int)(t % a.S);
    t /= a.S;
    const int c = (int)(t % a.C), n = (int)(t / a.C);
    const int f = VEC ? 4 / GW : a.f;
    const float* row = a.x + (((long)n * a.C + c) * a.R + (a.y0 + oy * f)) * (long)a.R + a.x0 + (long)gx * GW * f;
    double s[GW];
#pragma unroll
    for (int j = 0; j < GW; ++j) s[j] = 0.0;
    if (VEC) {
        for (int r = 0; r < f; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(row + (long)r * a.R);
            const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j * GW / 4] += (double)q[j];
        }
    } else {
        for (int r = 0; r < f; ++r)
            for (int i = 0; i < f; ++i) s[0] += (double)row[(long)r * a.R + i];
    }
    const double cnt = (double)(f * f);
    const long plane = (long)a.S * a.S;
    const long o = (long)oy * a.S + (long)gx * GW;
    for (int k = 0; k < (a.C == 1 ? 3 : 1); ++k) {
        const int oc = a.C == 1 ? k : c;
        float* dst = a.y + ((long)n * 3 + oc) * plane + o;
        float out[GW];
#pragma unroll
        for (int j = 0; j < GW; ++j) out[j] = ppl_value(s[j], cnt, a.mean[oc], a.stdv[oc]);
        if (GW == 4) *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[GW > 1 ? 1 : 0], out[GW > 2 ? 2 : 0], out[GW > 3 ? 3 : 0]);
        else if (GW == 2) *reinterpret_cast<float2*>(dst) = make_float2(out[0], out[GW > 1 ? 1 : 0]);
        else dst[0] = out[0];
    }
}

template <int GW, bool VEC>
void ppl_launch(const PplArgs& a, hipStream_t stream) {
    const long total = (long)a.N * a.C * a.S * ((a.S + GW - 1) / GW);
    hipLaunchKernelGGL((ppl_frontend_kernel<GW, VEC>), dim3((unsigned)shg_cdiv(total, 256)), dim3(256), 0, stream, a);
}

}  // namespace

// x [N,C,H,W] float32 in [-1, 1], C in {1, 3}, H == W -> y [N,3,S,S] float32 (see include/shgan_hip.h).
extern "C" int shg_ppl_frontend_f32(const float* x, float* y, int N, int C, int H, int W, int factor, int crop, const float* mean,
                                    const float* stdv, void* stream) {
    SHG_CHECK_ARG(x && y && mean && stdv, "ppl_frontend: null pointer");
    SHG_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && H <= 65536 && W <= 65536, "ppl_frontend: bad geometry N %d %dx%d", N, H, W);
    SHG_CHECK_ARG(C == 1 || C == 3, "ppl_frontend: %d channels (an image has 1 or 3)", C);
    SHG_CHECK_ARG(H == W, "ppl_frontend: a %d x %d image is not square", H, W);
    SHG_CHECK_ARG(factor >= 0 && factor <= 256, "ppl_frontend: downsampling factor %d outside 0..256", factor);
    SHG_CHECK_ARG(crop == 0 || crop == 1, "ppl_frontend: crop must be 0 or 1");
    PplArgs a;
    a.x = x; a.y = y; a.N = N; a.C = C; a.R = H;
    a.f = factor > 1 ? factor : 1;
    const int c8 = H / 8;
    const int side = crop ? 4 * c8 : H;                 // rows [3c, 7c), columns [2c, 6c)
    a.y0 = crop ? 3 * c8 : 0;
    a.x0 = crop ? 2 * c8 : 0;
    SHG_CHECK_ARG(side >= 1, "ppl_frontend: the centre crop of a %d x %d image is empty", H, W);
    SHG_CHECK_ARG(side % a.f == 0, "ppl_frontend: a side of %d is not divisible by the factor %d", side, a.f);
    a.S = side / a.f;
    SHG_CHECK_ARG((long)N * C * H * W < (1L << 40) && (long)N * 3 * a.S * a.S < (1L << 38), "ppl_frontend: tensor too large");
    for (int k = 0; k < 3; ++k) {
        SHG_CHECK_ARG(stdv[k] > 0.f, "ppl_frontend: std[%d] = %g must be positive", k, (double)stdv[k]);
        a.mean[k] = mean[k];
        a.stdv[k] = stdv[k];
    }
    // the window [y0, y0 + S*f) x [x0, x0 + S*f) lies inside the R x R plane by construction (7c <= R, 6c <= R); the float4 form
    // additionally needs 16-byte aligned box rows and whole groups
    const int gw = a.f == 1 ? 4 : (a.f == 2 ? 2 : (a.f == 4 ? 1 : 0));
    const bool vec = gw && a.S % gw == 0 && H % 4 == 0 && a.x0 % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec && gw == 4) ppl_launch<4, true>(a, st);
    else if (vec && gw == 2) ppl_launch<2, true>(a, st);
    else if (vec) ppl_launch<1, true>(a, st);
    else ppl_launch<1, false>(a, st);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
