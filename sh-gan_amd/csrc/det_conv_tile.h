// What the detector family (inception.hip, lpips.hip, vgg16.hip) shares on the device: the value of a source sample, and the implicit-GEMM
// tile of the exact-fp32 convolution -- the one place that knows the operand and accumulator layout of v_mfma_f32_32x32x2_f32.
#pragma once
#include "shg_device.h"

#define DET_BM 64        // output channels per workgroup
#define DET_BN 64        // output pixels per workgroup
#define DET_BK 16        // K per stage

// The value of a source sample: lut[u8] (uint8 input), or x*scale + bias rounded twice (float32 input, lut NULL).
__device__ __forceinline__ float det_value(const void* x, const float* lut, float scale, float bias, long i) {
    if (lut) return lut[reinterpret_cast<const uint8_t*>(x)[i]];
    return __fadd_rn(__fmul_rn(reinterpret_cast<const float*>(x)[i], scale), bias);
}

// Packed weight of a convolution, the A operand of the tile: w [O][I][kh][kw], bias [O] -> wp [Kp][Np] (k = (ky*kw + kx)*I + c, Kp = K
// rounded up to DET_BK, Np = O rounded up to DET_BM, zero outside K x O), bp [Np].  Any kernel size; internal to the library
// (inception.hip; the exported entry points keep their own argument checks).
__attribute__((visibility("hidden"))) int shg_det_weight_prep(const float* w, const float* bias, float* wp, float* bp, int O, int I, int kh, int kw,
                                                              hipStream_t stream);

// One workgroup of 256 threads = 64 channels x 64 pixels, four waves of 32 x 32.  A thread's part, by its index alone:
// staging: X rows kr0 + 4i (i < 4) of pixel px, W row wr, columns wc..wc+3; MFMA: the wave's channel / pixel sub-tile at (wm, wn),
// operand row lk and column lj; accumulator element r is D[wm + row(r)][wn + lj].
struct DetRoles {
    int px, kr0, wr, wc, wm, wn, lk, lj;
    __device__ __forceinline__ int row(int r) const { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
};
__device__ __forceinline__ DetRoles det_roles() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return {tid & 63, tid >> 6, tid >> 4, (tid & 15) * 4, (wave & 1) * 32, (wave >> 1) * 32, lane >> 5, lane & 31};
}

// K steps [kt0, kt1) of 16 through two LDS stages (one barrier per step).  `load(kt, xr, wreg)` fetches what the calling thread stages
// of step kt: xr[i] = X row kr0 + 4i of pixel px, wreg = W row wr, columns wc..wc+3.  Returns the wave's 32 x 32 accumulator.
template <class Load>
__device__ __forceinline__ f32x16 det_conv_tile(float (&Ws)[2][DET_BK][DET_BM], float (&Xs)[2][DET_BK][DET_BN], int kt0, int kt1, Load load) {
    const DetRoles t = det_roles();
    float xr[4];
    float4 wreg;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // xr and wreg reach `load` through a closure, as a kernel's own locals would: handed over as plain arguments, xr is promoted to one
    // register quad and a gather's loads are waited for in front of the MFMAs they are issued to run under
    auto fetch = [&](int kt) { load(kt, xr, wreg); };
    if (kt0 < kt1) {
        fetch(kt0);
        int buf = 0;
        for (int kt = kt0; kt < kt1; ++kt) {
            *reinterpret_cast<float4*>(&Ws[buf][t.wr][t.wc]) = wreg;
#pragma unroll
            for (int i = 0; i < 4; ++i) Xs[buf][t.kr0 + 4 * i][t.px] = xr[i];
            __syncthreads();
            if (kt + 1 < kt1) fetch(kt + 1);                   // next step's loads in flight under this step's MFMAs
#pragma unroll
            for (int kk = 0; kk < DET_BK; kk += 2) {
                const float av = Ws[buf][kk + t.lk][t.wm + t.lj];
                const float bv = Xs[buf][kk + t.lk][t.wn + t.lj];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
            buf ^= 1;
        }
    }
    return acc;
}
