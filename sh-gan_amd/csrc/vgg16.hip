// VGG16 up to fc2: the detector of the improved precision / recall metric (`pr50k3_full`, the reference's lib/evaluator/
// stylegan_metrics/precision_recall.py:64-76; sh-gan_amd/vgg16.py drives this file).  The 13 convolutions (3 x 3, stride 1, pad 1,
// ReLU) run on the FID detector's convolution (inception.hip), fc1 / fc2 on shg_dense_f32 (dense.hip: a wave per output feature, the
// weight row read once per slab of up to 16 images).  This file adds what neither has: the area-resize front end and the 2 x 2 pool.
#include "det_conv_tile.h"

#define VGG_RES 224      // the network's input side

// ---- front end: value map (det_value, as the FID detector's: lut[u8], or x*scale + bias rounded twice), `F.interpolate(mode='area')` to
// 224 x 224 = adaptive average pooling over the bins [floor(i*H/224), ceil((i+1)*H/224)) (integer arithmetic: exact for any ratio, up-
// or down-scaling; a 1 x 1 bin at 224), then (v - mean_c) / std_c.  A bin is summed row by row, left to right, in fp32 and divided by
// its sample count.
struct VggNorm { float mean[3], stdv[3]; };

__global__ __launch_bounds__(256) void vgg_frontend_kernel(const void* x, const float* lut, float scale, float bias, VggNorm nrm, float* y, int B,
                                                           int H, int W) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long plane = (long)VGG_RES * VGG_RES;
    if (e >= (long)B * 3 * plane) return;
    const long bc = e / plane;
    const int r = (int)(e - bc * plane), oy = r / VGG_RES, ox = r - oy * VGG_RES, c = (int)(bc % 3);
    const long base = bc * (long)H * W;
    const int y0 = (int)((long)oy * H / VGG_RES), y1 = (int)(((long)(oy + 1) * H + VGG_RES - 1) / VGG_RES);
    const int x0 = (int)((long)ox * W / VGG_RES), x1 = (int)(((long)(ox + 1) * W + VGG_RES - 1) / VGG_RES);
    float s = 0.f;
    for (int iy = y0; iy < y1; ++iy)
        for (int ix = x0; ix < x1; ++ix) s = __fadd_rn(s, det_value(x, lut, scale, bias, base + (long)iy * W + ix));
    const float v = __fdiv_rn(s, (float)((y1 - y0) * (x1 - x0)));
    y[e] = __fdiv_rn(__fsub_rn(v, nrm.mean[c]), nrm.stdv[c]);
}

// x [B,3,H,W] uint8 (lut [256] given) or float32 (lut NULL: x*scale + bias) -> y [B,3,224,224] float32; mean / std [3] host floats.
extern "C" int shg_vgg16_frontend_f32(const void* x, const float* lut, float scale, float bias, const float* mean, const float* stdv, float* y,
                                      int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && y && mean && stdv, "vgg16_frontend: null pointer");
    SHG_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (long)B * 3 * H * W < (1L << 40) && H <= 65536 && W <= 65536,
                  "vgg16_frontend: bad geometry B %d %dx%d", B, H, W);
    VggNorm nrm;
    for (int c = 0; c < 3; ++c) {
        SHG_CHECK_ARG(stdv[c] > 0.f, "vgg16_frontend: std[%d] = %g must be positive", c, (double)stdv[c]);
        nrm.mean[c] = mean[c];
        nrm.stdv[c] = stdv[c];
    }
    const long n = (long)B * 3 * VGG_RES * VGG_RES;
    hipLaunchKernelGGL(vgg_frontend_kernel, dim3(shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, lut, scale, bias, nrm, y, B, H, W);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- 2 x 2 max pool, stride 2, floor: y [BC, H/2, W/2] = max over the 2 x 2 window (an odd last row / column is dropped)
__global__ __launch_bounds__(256) void vgg_maxpool2_kernel(const float* x, float* y, long BC, int H, int W, int OH, int OW) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long OHW = (long)OH * OW;
    if (e >= BC * OHW) return;
    const long bc = e / OHW;
    const int r = (int)(e - bc * OHW), oy = r / OW, ox = r - oy * OW;
    const float* p = x + bc * (long)H * W + (long)(2 * oy) * W + 2 * ox;
    y[e] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
}

extern "C" int shg_vgg16_maxpool2_f32(const float* x, float* y, int B, int C, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && y, "vgg16_maxpool2: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && H >= 2 && W >= 2 && (long)B * C * H * W < (1L << 40), "vgg16_maxpool2: bad geometry B %d C %d %dx%d", B, C, H, W);
    const int OH = H / 2, OW = W / 2;
    const long n = (long)B * C * OH * OW;
    hipLaunchKernelGGL(vgg_maxpool2_kernel, dim3(shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)B * C, H, W, OH, OW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
