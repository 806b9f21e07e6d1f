// Streaming passes on NHWC halves (data layout: conv_f16.hip).  gfx950 only.
//
//   bias_act_f16 (+bwd)  x + bias[c] -> lrelu_agc, and its gradient from the saved output (common/utils.py:135-143);
//   modtail_f16 (+bwd)   the modulation tail of a half layer in one pass each way;
//   relayout_*           the block-boundary casts float32 NCHW <-> float16 NHWC.
#include "shg_common.h"
#include "conv_f16_p.h"

namespace f16 {

// y = lrelu_agc(x + bias[c]) on NHWC halves (arithmetic in fp32, one rounding), and its gradient from the saved output
// Streaming passes: the per-channel operands are read as two float4 ONCE per thread when 256 % (C/8) == 0 (a thread then keeps its channels for
// the whole grid-stride loop) -- eight scalar operand loads and a 64-bit modulo per 16-byte piece ran at 2.0-3.1 TB/s of read + write traffic, this
// form at 5.4-6.3 (tools/conv_f16_bench.py).  EU > 1 requests several pieces before the first use: no gain (4.8 TB/s at 4), the pass is not
// short of loads in flight.
constexpr int EU = 1;

__device__ __forceinline__ void load8f(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// CONSTC: 256 % (C/8) == 0 -- a thread keeps its 8 channels for the whole grid-stride loop and holds their bias in registers
template <bool CONSTC>
__global__ __launch_bounds__(256) void bias_act_f16_kernel(const _Float16* x, const float* bias, _Float16* y, long total8, int C, int act,
                                                           float alpha, float gain, float clamp) {
    const int c8n = C >> 3;
    const long stride = (long)gridDim.x * 256, e0 = (long)blockIdx.x * 256 + threadIdx.x;
    float bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (CONSTC && bias) load8f(bias + (int)(e0 % c8n) * 8, bb);
    for (long eb = e0; eb < total8; eb += EU * stride) {
        h8 v[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const long e = eb + u * stride;
            v[u] = *(const h8*)(x + (e < total8 ? e : total8 - 1) * 8);
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const long e = eb + u * stride;
            if (!CONSTC && bias) load8f(bias + (int)((e < total8 ? e : total8 - 1) % c8n) * 8, bb);
            h8 out;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float t = (float)v[u][q] + bb[q];
                t = act ? shg_lrelu_agc(t, alpha, gain, clamp) : t * gain;
                out[q] = (_Float16)t;
            }
            if (e < total8) *(h8*)(y + e * 8) = out;
        }
    }
}

// (three streams and no per-channel operand: the plain loop already runs at 5+ TB/s, grouping the loads measured 5 % slower)
__global__ __launch_bounds__(256) void bias_act_backward_f16_kernel(const _Float16* g, const _Float16* y, _Float16* dx, long total8, int act,
                                                                    float alpha, float gain, float clamp) {
    const float gp = gain, gn = act ? alpha * gain : gain;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total8; e += (long)gridDim.x * 256) {
        const h8 gv = *(const h8*)(g + e * 8), yv = *(const h8*)(y + e * 8);
        h8 out;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float v = (float)yv[q];
            const float slope = (act && clamp >= 0.f && fabsf(v) >= clamp) ? 0.f : (v > 0.f ? gp : gn);
            out[q] = (_Float16)((float)gv[q] * slope);
        }
        *(h8*)(dx + e * 8) = out;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Modulation tail of a half layer in ONE pass each way (stylegan.py:176-181 `fma(x, dcoefs, noise)` + :298-304 bias / lrelu_agc, and
// with act = 0 / no noise / no bias the input scaling `x * styles` of :173):
//     y = A(t * d[n,c] + noise[n?,h,w] + bias[c])
// backward (first order): gz = gy * A'(y) read from the saved output, gt = gz * d, and the three reductions of the same pass --
// sum_{hw} gz t (-> d), sum_{hw} gz (-> bias) per (n, c) as per-workgroup partials [n][block][2][C] (summed in a fixed order by the
// caller: deterministic), sum_c gz per pixel (-> noise).  A lane holds 8 channels of one pixel; the C/8 lanes of a pixel are adjacent.
// ---------------------------------------------------------------------------------------------------------------------------
struct TailP {
    const _Float16* t; const _Float16* y_in; const _Float16* gy;
    const float* d; const float* noise; const float* bias;
    const _Float16* u; const float* e;  // backward: optional second product, out = A'(y) (gy d + u e)
    _Float16* out;                    // forward: y; backward: gt
    float* part; float* gnoise;
    int N, HW, C, noise_mode, act, nblk;
    float alpha, gain, clamp;
};

template <bool CONSTC>
__global__ __launch_bounds__(256) void modtail_f16_kernel(const TailP p) {
    const int c8n = p.C >> 3, n = blockIdx.y;
    const long total = (long)p.HW * c8n;
    const _Float16* tp = p.t + (long)n * p.HW * p.C;
    _Float16* yp = p.out + (long)n * p.HW * p.C;
    const float* np_ = p.noise_mode == 0 ? nullptr : p.noise + (p.noise_mode == 2 ? (long)n * p.HW : 0);
    const long stride = (long)gridDim.x * 256, e0 = (long)blockIdx.x * 256 + threadIdx.x;
    float dd[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (CONSTC) {
        const int c = (int)(e0 % c8n) * 8;
        if (p.d) load8f(p.d + (long)n * p.C + c, dd);
        if (p.bias) load8f(p.bias + c, bb);
    }
    for (long eb = e0; eb < total; eb += EU * stride) {
        h8 v[EU];
        float nz[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const long e = eb + u * stride, ec = e < total ? e : total - 1;
            v[u] = *(const h8*)(tp + ec * 8);
            nz[u] = np_ ? np_[ec / c8n] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const long e = eb + u * stride;
            if (!CONSTC) {
                const int c = (int)((e < total ? e : total - 1) % c8n) * 8;
                if (p.d) load8f(p.d + (long)n * p.C + c, dd);
                if (p.bias) load8f(p.bias + c, bb);
            }
            h8 o;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float z = (float)v[u][q] * dd[q] + nz[u] + bb[q];
                z = p.act ? shg_lrelu_agc(z, p.alpha, p.gain, p.clamp) : z * p.gain;
                o[q] = (_Float16)z;
            }
            if (e < total) *(h8*)(yp + e * 8) = o;
        }
    }
}

__global__ __launch_bounds__(256) void modtail_backward_f16_kernel(const TailP p) {
    __shared__ float red[2][256][8];
    const int c8n = p.C >> 3, n = blockIdx.y, tid = threadIdx.x;
    const long total = (long)p.HW * c8n, off = (long)n * p.HW * p.C;
    const float gp = p.gain, gn = p.act ? p.alpha * p.gain : p.gain;
    float s1[8], s0[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s1[q] = s0[q] = 0.f;
    // (256 and the grid stride are multiples of C/8 <= 64: a thread keeps its channel group for the whole loop)
    const int c = (int)(((long)blockIdx.x * 256 + tid) % c8n) * 8;
    float dd[8], ee[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { dd[q] = p.d ? p.d[(long)n * p.C + c + q] : 1.f; ee[q] = (p.u && p.e) ? p.e[(long)n * p.C + c + q] : 1.f; }
    const long stride = (long)gridDim.x * 256;
    const int iters = (int)((total + stride - 1) / stride);                                        // uniform trip count: whole waves stay in the shuffle
    for (int it = 0; it < iters; ++it) {
        const long e = (long)blockIdx.x * 256 + tid + it * stride;
        const bool ok = e < total;
        float pix_sum = 0.f;
        if (ok) {
            const h8 g = *(const h8*)(p.gy + off + e * 8), yv = *(const h8*)(p.y_in + off + e * 8);
            h8 tv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (p.t) tv = *(const h8*)(p.t + off + e * 8);
            h8 uv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (p.u) uv = *(const h8*)(p.u + off + e * 8);
            h8 o;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float yq = (float)yv[q];
                const float slope = (p.act && p.clamp >= 0.f && fabsf(yq) >= p.clamp) ? 0.f : (yq > 0.f || !p.act ? gp : gn);
                const float gz = (float)g[q] * slope;
                o[q] = p.u ? (_Float16)__builtin_fmaf((float)uv[q] * slope, ee[q], gz * dd[q]) : (_Float16)(gz * dd[q]);
                s1[q] += gz * (float)tv[q];
                s0[q] += gz;
                pix_sum += gz;
            }
            *(h8*)(p.out + off + e * 8) = o;
        }
        if (p.gnoise) {                                           // sum over the C/8 adjacent lanes of this pixel
            for (int m = 1; m < c8n; m <<= 1) pix_sum += __shfl_xor(pix_sum, m, 64);
            if (ok && (e % c8n) == 0) p.gnoise[(long)n * p.HW + e / c8n] = pix_sum;
        }
    }
    if (!p.part) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) { red[0][tid][q] = s1[q]; red[1][tid][q] = s0[q]; }
    __syncthreads();
    // threads tid, tid + c8n, tid + 2 c8n, ... share a channel group
    if (tid < c8n) {
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float a = 0.f;
                for (int j = tid; j < 256; j += c8n) a += red[k][j][q];
                p.part[(((long)n * p.nblk + blockIdx.x) * 2 + k) * p.C + tid * 8 + q] = a;
            }
    }
}

// ---- block-boundary casts (stylegan.py:486-495,659-663; comodgan.py:39-43,305-312: `x.to(dtype)`): float32 NCHW <-> float16 NHWC as one
// transposing pass through LDS.  Tile = 64 channels x 64 pixels; global accesses are 256-byte runs along the pixels on the float32 side and
// whole 16-byte pieces of 8 channels (128 bytes per pixel and tile) on the float16 side.  torch's `.to(dtype, memory_format)` reached
// 1.6 TB/s on these tensors (63 us for [8, 512, 64, 64]).
__global__ __launch_bounds__(256) void relayout_to_half_kernel(const float* x, _Float16* y, int C, int HW) {
    __shared__ float t[64][65];
    const int tid = threadIdx.x, n = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const float* xn = x + (long)n * C * HW;
    _Float16* yn = y + (long)n * C * HW;
    const int pl = tid & 63, cw = tid >> 6;
#pragma unroll 4
    for (int c = cw; c < 64; c += 4) t[c][pl] = (c0 + c < C && p0 + pl < HW) ? xn[(long)(c0 + c) * HW + p0 + pl] : 0.f;
    __syncthreads();
    const int cq = (tid & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int pp = (tid >> 3) + 32 * it;
        if (p0 + pp < HW && c0 + cq < C) {                       // C % 8 == 0: a piece is inside or outside as a whole
            h8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (_Float16)t[cq + k][pp];
            *(h8*)(yn + (long)(p0 + pp) * C + c0 + cq) = v;
        }
    }
}

__global__ __launch_bounds__(256) void relayout_to_float_kernel(const _Float16* x, float* y, int C, int HW) {
    __shared__ float t[64][65];
    const int tid = threadIdx.x, n = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const _Float16* xn = x + (long)n * C * HW;
    float* yn = y + (long)n * C * HW;
    const int cq = (tid & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int pp = (tid >> 3) + 32 * it;
        h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p0 + pp < HW && c0 + cq < C) v = *(const h8*)(xn + (long)(p0 + pp) * C + c0 + cq);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[cq + k][pp] = (float)v[k];
    }
    __syncthreads();
    const int pl = tid & 63, cw = tid >> 6;
#pragma unroll 4
    for (int c = cw; c < 64; c += 4)
        if (c0 + c < C && p0 + pl < HW) yn[(long)(c0 + c) * HW + p0 + pl] = t[c][pl];
}

// thin tensors (the 4-channel network inputs, RGB): a lane owns a pixel, C <= 16 planes on the float32 side, 2 C contiguous bytes on the other
template <bool TO_HALF>
__global__ __launch_bounds__(256) void relayout_thin_kernel(const void* src, void* dst, int C, long HW, long total) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long n = p / HW, q = p - n * HW;
        if (TO_HALF) {
            const float* x = (const float*)src + n * C * HW + q;
            _Float16* y = (_Float16*)dst + p * C;
            for (int c = 0; c < C; ++c) y[c] = (_Float16)x[(long)c * HW];
        } else {
            const _Float16* x = (const _Float16*)src + p * C;
            float* y = (float*)dst + n * C * HW + q;
            for (int c = 0; c < C; ++c) y[(long)c * HW] = (float)x[c];
        }
    }
}

}  // namespace f16

// src float32 [N,C,HW] (NCHW) -> dst float16 [N,HW,C] (NHWC) when to_half, the reverse otherwise; C % 8 == 0.
extern "C" int shg_relayout_f32_f16(const void* src, void* dst, int N, int C, long HW, int to_half, void* stream) {
    SHG_CHECK_ARG(src && dst && N >= 1 && C >= 1 && (C % 8 == 0 || C <= 16) && HW >= 1 && HW <= 0x7fffffffL && N <= 65535, "relayout: C % 8 == 0 or C <= 16");
    if (C % 8) {
        const long total = (long)N * HW;
        long grid = (total + 255) / 256;
        if (grid > 65536) grid = 65536;
        if (to_half) hipLaunchKernelGGL(f16::relayout_thin_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, dst, C, HW, total);
        else hipLaunchKernelGGL(f16::relayout_thin_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, dst, C, HW, total);
        SHG_CHECK_LAUNCH();
        return SHG_OK;
    }
    SHG_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "relayout: 16-byte aligned tensors");
    const dim3 grid((unsigned)((HW + 63) / 64), (C + 63) / 64, N);
    if (to_half) hipLaunchKernelGGL(f16::relayout_to_half_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, (_Float16*)dst, C, (int)HW);
    else hipLaunchKernelGGL(f16::relayout_to_float_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)src, (float*)dst, C, (int)HW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_bias_act_f16(const void* x, const float* bias, void* y, long pixels, int C, int act, float alpha, float gain, float clamp,
                                void* stream) {
    SHG_CHECK_ARG(x && y, "bias_act_f16: null pointer");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                  "bias_act_f16: x, y and bias must be 16-byte aligned");
    SHG_CHECK_ARG(pixels >= 0 && C >= 8 && (C % 8) == 0, "bias_act_f16: C must be a multiple of 8");
    const long total8 = pixels * (C / 8);
    if (total8 == 0) return SHG_OK;
    int grid = (int)shg_cdiv(total8, 256L * f16::EU);
    if (grid > 256 * 16) grid = 256 * 16;
    if (256 % (C / 8) == 0)
        hipLaunchKernelGGL(f16::bias_act_f16_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x, bias, (_Float16*)y, total8, C,
                           act, alpha, gain, clamp);
    else
        hipLaunchKernelGGL(f16::bias_act_f16_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x, bias, (_Float16*)y, total8, C,
                           act, alpha, gain, clamp);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_bias_act_backward_f16(const void* g, const void* y, void* dx, long total, int act, float alpha, float gain, float clamp,
                                         void* stream) {
    SHG_CHECK_ARG(g && y && dx, "bias_act_backward_f16: null pointer");
    SHG_CHECK_ARG(total >= 0 && (total % 8) == 0, "bias_act_backward_f16: element count must be a multiple of 8");
    if (total == 0) return SHG_OK;
    int grid = shg_cdiv(total / 8, 256);
    if (grid > 256 * 32) grid = 256 * 32;
    hipLaunchKernelGGL(f16::bias_act_backward_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)g, (const _Float16*)y,
                       (_Float16*)dx, total / 8, act, alpha, gain, clamp);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// y = A(t * d[n,c] + noise + bias[c]) on NHWC halves: d fp32 [N,C] or NULL, noise fp32 [HW] (noise_mode 1) / [N,HW] (2) / none (0), bias fp32
// [C] or NULL; act = 0: (..) * gain.  C a multiple of 8.
extern "C" int shg_modtail_f16(const void* t, const float* d, const float* noise, int noise_mode, const float* bias, void* y, int N, long HW, int C,
                               int act, float alpha, float gain, float clamp, void* stream) {
    SHG_CHECK_ARG(t && y && N >= 1 && HW >= 1 && C >= 8 && (C % 8) == 0, "modtail_f16: bad arguments (C must be a multiple of 8)");
    SHG_CHECK_ARG(HW < 2147483647L, "modtail_f16: H*W must fit 31 bits");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                  "modtail_f16: t, y, d and bias must be 16-byte aligned");
    f16::TailP p{};
    p.t = (const _Float16*)t; p.d = d; p.noise = noise_mode ? noise : nullptr; p.noise_mode = noise ? noise_mode : 0; p.bias = bias;
    p.out = (_Float16*)y; p.N = N; p.HW = (int)HW; p.C = C; p.act = act; p.alpha = alpha; p.gain = gain; p.clamp = clamp;
    long blocks = (HW * (C / 8) + 256 * f16::EU - 1) / (256 * f16::EU);
    if (blocks > 2048) blocks = 2048;
    if (256 % (C / 8) == 0) hipLaunchKernelGGL(f16::modtail_f16_kernel<true>, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(f16::modtail_f16_kernel<false>, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, p);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// workgroups per sample of shg_modtail_backward_f16 (rows of its `part` buffer)
extern "C" int shg_modtail_backward_f16_blocks(long HW, int C) {
    long blocks = (HW * (C / 8) + 255) / 256;
    return (int)(blocks > 256 ? 256 : blocks);
}

// gt = gy * A'(y) * d [+ u * A'(y) * e] (halves); part [N][blocks][2][C] fp32 = per-workgroup sums over pixels of gz*t and gz (NULL: skipped; t may be
// NULL when only sum gz is wanted); gnoise [N,HW] fp32 = sum over channels of gz (NULL: skipped); u (halves like gy) / e [N,C] fp32: the optional second
// product of the tail's double backward.  C in {8,16,...,512} with C/8 a power of two.
extern "C" int shg_modtail_backward_f16(const void* gy, const void* y, const void* t, const float* d, const void* u, const float* e, void* gt, float* part,
                                        float* gnoise, int N, long HW, int C, int act, float alpha, float gain, float clamp, void* stream) {
    SHG_CHECK_ARG(gy && y && gt && N >= 1 && HW >= 1, "modtail_backward_f16: null pointer / empty");
    SHG_CHECK_ARG(HW < 2147483647L, "modtail_backward_f16: H*W must fit 31 bits");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(gt) |
                    reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(u)) & 15) == 0, "modtail_backward_f16: gy, y, t, u, gt and d must be 16-byte aligned (vector accesses)");
    const int c8n = C / 8;
    SHG_CHECK_ARG(C >= 8 && (C % 8) == 0 && c8n <= 64 && (c8n & (c8n - 1)) == 0, "modtail_backward_f16: C/8 must be a power of two <= 64");
    f16::TailP p{};
    p.gy = (const _Float16*)gy; p.y_in = (const _Float16*)y; p.t = (const _Float16*)t; p.d = d; p.out = (_Float16*)gt; p.part = part;
    p.u = (const _Float16*)u; p.e = e;
    p.gnoise = gnoise; p.N = N; p.HW = (int)HW; p.C = C; p.act = act; p.alpha = alpha; p.gain = gain; p.clamp = clamp;
    p.nblk = shg_modtail_backward_f16_blocks(HW, C);
    hipLaunchKernelGGL(f16::modtail_backward_f16_kernel, dim3(p.nblk, N), dim3(256), 0, (hipStream_t)stream, p);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
