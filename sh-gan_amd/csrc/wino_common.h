// Host-side launch glue shared by the fp32 Winograd family: conv_wino.hip (F(2x2,3x3)), conv_wino4.hip (F(4x4,3x3)) and the
// up launches of conv_wino_poly.hip.  Each entry point keeps its own argument checks, plan function and instantiation switch.
#pragma once
#include "shg_device.h"

// Every file of the family has a 64-float zero source of its own (shg_wino_zeros, shg_wino4_zeros, shg_poly_zeros) for LDS-DMA lanes
// that fall into padding and for absent tail operands: a __device__ variable is a per-translation-unit symbol, and one shared
// definition would need relocatable device code, which the build turns off (-fno-gpu-rdc).

// Launch parameters of conv_wino_kernel and conv_wino4_kernel (only the layout of wu and the tile extent differ between the two).
struct WinoParams {
    const float* x;          // [NB, I, H, W]
    const float* wu;         // transformed weights: [OP/64][nchunk][16][64 lanes][KC] (F(2x2)), [OP/64][nchunk][4 k-steps][72 units][64 lanes] (F(4x4))
    float* y;                // [NB, O, H, W]
    const float* in_scale;   // [NB, I] or null
    const float* out_scale;  // [NB, O] or null
    const float* bias;       // [O] or null
    const float* noise;      // see noise_mode
    const float* residual;   // like y, added after the activation
    int NB, I, O, OP, H, W;
    int tiles_x, tiles_y;    // tiles per image
    int n_ttiles, n_otiles, nchunk;
    int cps;                 // chunks per K slice (= nchunk when the launch is not split); slice = blockIdx.y
    long part_stride;        // floats between the slices' partial outputs (0: y itself)
    int noise_mode;          // 0 none, 1 [H,W], 2 [NB,H,W]
    float noise_strength;
    int act;
    float alpha, gain, clamp;
};

// conv_wino.hip
int shg_wino_ksplit(long tiles, int nchunk);
void shg_launch_wino_split_reduce(const float* part, float* y, int ks, int NB, int O, int H, int W, const float* out_scale, const float* bias,
                                  const float* noise, int noise_mode, float noise_strength, int act, float alpha, float gain, float clamp,
                                  const float* residual, hipStream_t s);

static inline uintptr_t shg_addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the arguments of an entry point as launch parameters (tiling and K split still to be filled in)
static inline WinoParams shg_wino_params(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W, const float* in_scale,
                                         const float* out_scale, const float* bias, const float* noise, int noise_mode, float noise_strength,
                                         int act, float alpha, float gain, float clamp, const float* residual) {
    WinoParams p{};
    p.x = x; p.wu = wu; p.y = y; p.in_scale = in_scale; p.out_scale = out_scale; p.bias = bias;
    p.noise = noise_mode ? noise : nullptr; p.residual = residual;
    p.NB = NB; p.I = I; p.O = O; p.OP = OP; p.H = H; p.W = W;
    p.noise_mode = noise ? noise_mode : 0; p.noise_strength = noise_strength;
    p.act = act; p.alpha = alpha; p.gain = gain; p.clamp = clamp;
    return p;
}

// bytes of scratch with which a launch of `tiles` workgroups over `nchunk` channel chunks is split (0: it is not)
static inline size_t shg_wino_split_bytes(long tiles, int nchunk, size_t out_bytes) {
    const int ks = shg_wino_ksplit(tiles, nchunk);
    return ks > 1 ? (size_t)ks * out_bytes : 0;
}

// The K-split decision of a launch: returns the number of slices ks (gridDim.y) and sets the chunks per slice.  Split only with
// scratch for it and when every address or-ed into `align16` is 16-byte aligned (the reduction's accesses are float4; WHICH operands
// that covers is the entry point's rule and differs between them on purpose); as many slices as the workspace holds.  When split, the
// slices write raw partial outputs `part_stride` floats apart into the workspace instead of y.
static inline int shg_wino_split(long tiles, int nchunk, size_t out_bytes, void* workspace, size_t ws_bytes, uintptr_t align16, float** y, int* cps,
                                 long* part_stride) {
    int ks = (workspace && (align16 & 15) == 0) ? shg_wino_ksplit(tiles, nchunk) : 1;
    while (ks > 1 && (size_t)ks * out_bytes > ws_bytes) ks /= 2;
    *cps = shg_cdiv(nchunk, ks);
    ks = shg_cdiv(nchunk, *cps);
    *part_stride = 0;
    if (ks > 1) { *y = (float*)workspace; *part_stride = (long)(out_bytes / sizeof(float)); }
    return ks;
}

// shg_wino_split for a WinoParams launch: when split, the slices write raw sums and the layer tail moves to the reduction
static inline int shg_wino_split(WinoParams& p, void* workspace, size_t ws_bytes, uintptr_t align16) {
    const int ks = shg_wino_split((long)p.n_ttiles * p.n_otiles, p.nchunk, (size_t)p.NB * p.O * p.H * p.W * sizeof(float), workspace, ws_bytes, align16,
                                  &p.y, &p.cps, &p.part_stride);
    if (ks > 1) { p.out_scale = nullptr; p.bias = nullptr; p.noise = nullptr; p.noise_mode = 0; p.residual = nullptr; p.act = 0; p.gain = 1.f; }
    return ks;
}
