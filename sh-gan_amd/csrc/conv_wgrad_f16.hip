// fp16 weight gradient of the 1x1 / 3x3 convolutions (reference: conv2d_gradfix.py:140-149 on the cuDNN half kernels of the `use_fp16`
// blocks).  gfx950 only; NHWC halves in, fp32 out (data layout: conv_f16.hip).
//
//   conv_wgrad_f16       dw[t][o][i] = sum_{n,oy,ox} g[n,oy,ox,o] * x[n, oy*s + dy_t, ox*s + dx_t, i]: K = pixels, so an operand is 8
//                        consecutive pixels of ONE channel -- the NHWC tiles are transposed while they are staged ([channel][pixel]
//                        LDS images) and every operand is an aligned ds_read_b128; the three kx taps of a row share their reads
//                        (shift by one half = v_alignbit, by two = registers; stride 2: even / odd column halves); 64 x 64 (o,i) tile
//                        per workgroup, all taps per wave, split over pixel slices with fp32 partials + a fixed-order reduction
//                        (wgrad_reduce_kernel; deterministic).
#include "shg_common.h"
#include "conv_f16_p.h"

namespace f16 {

constexpr int WR = 4;                // output rows per staged block (the 3x3 stride-1 kernel stages 8: wgrad_rows)
constexpr int wgrad_rows(int k, int s) { return (k == 3 && s == 1) ? 8 : WR; }
constexpr int WC = 16;               // output columns per staged block = one MFMA k-step

struct WgradP {
    const _Float16* x;               // [N,H,W,I]
    const _Float16* g;               // [N,OH,OW,O]
    float* part;                     // [slices][NT][OP][IP] fp32 partial sums (OP, IP = O, I rounded up to 64)
    int N, I, O, H, W, OH, OW;
    int s, pad, k;                   // stride, padding, kernel size (1 or 3)
    int bx, by;                      // blocks per image along x / y
    long nblocks;                    // N * by * bx
    int slices, OP, IP;
    int XR, XC;                      // staged input rows / columns per block
};

// LDS images are TRANSPOSED while staging ([channel][pixel], 2-byte scatter writes of the 16-byte NHWC loads), so that an MFMA operand --
// 8 consecutive pixels of one channel -- is ONE aligned ds_read_b128 instead of eight 2-byte gathers:
//   gT[64 o][4 rows x 16 px (+8)]                       A operand of row r, k-group kg: gT[o][r*16 + kg*8 ..]
//   xT[64 i][XR rows][RP (+8 per channel)]              stride 1: RP = 24, columns as they come (18 used); the three kx taps of a row are
//                                                        the aligned 8 columns, the same shifted by one half (v_alignbit) and by two (registers)
//                                                        from one b128 + one b32 read;  stride 2: RP = 48 = even columns | odd columns,
//                                                        kx = 0 / 2 from the even half (aligned / shifted by one), kx = 1 from the odd half.
// Channel pitches (144 / 304 / 880 / 208 bytes) put the 16 lanes of a b128 group on 16 different 16-byte slots: conflict-free.
template <int K, int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv_wgrad_f16_kernel(const WgradP p) {
    constexpr int NT = K * K, WR = wgrad_rows(K, S);         // (8 rows at 3x3 stride 1: 72 MFMAs per wave between two barriers instead of 36)
    constexpr int XR = (WR - 1) * S + K, XC = (WC - 1) * S + K, RP = S == 1 ? 24 : 48, GP = WR * WC + 8, XP = XR * RP + 8;
    extern __shared__ __attribute__((aligned(16))) _Float16 sm[];
    _Float16* gT = sm;                               // [64][GP]
    _Float16* xT = sm + 64 * GP;                     // [64][XP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kg = lane >> 5;
    const int it = blockIdx.x % (p.IP / 64), ot = blockIdx.x / (p.IP / 64);
    const int wo = (wave >> 1) * 32, wi = (wave & 1) * 32;                 // this wave's 32 x 32 corner of the 64 x 64 tile
    f16x acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // staging is software-pipelined: the NHWC loads of block b+1 are issued before the multiply loop of block b and are written
    // (transposed) into LDS after it.  A thread stages FOUR ADJACENT PIXELS of one 8-channel group: per channel they are 8 contiguous bytes
    // of the [channel][pixel] image -- one ds_write_b64 (stride 2: the even and the odd pair, two ds_write_b32) instead of four 2-byte
    // scatter writes (48 ds_write_b16 per thread and block kept the LDS pipe busier than the matrix pipe: bank-conflict rate 0.54,
    // profiles/r05_f16_pmc_base_summary.txt).  Gradient tile: 16 quads x 8 groups (threads 0-127; K = 1: the input tile has the same shape
    // and takes threads 128-255); input tile: XR rows x QPR quads (the last one partial).
    constexpr int GITEMS = WR * 4 * 8;               // 128 (4 rows) or 256 (8 rows)
    constexpr int QPR = (XC + 3) / 4, XITEMS = XR * QPR * 8, XROUNDS = K == 1 ? 1 : (XITEMS + 255) / 256;
    h8 gv[4], xv[XROUNDS][4];
    const int sq = tid & 7;                          // 8-channel group of this thread's items
    auto fetch = [&](long blk) __attribute__((always_inline)) {
        const int bxi = (int)(blk % p.bx);
        const long rest = blk / p.bx;
        const int byi = (int)(rest % p.by), n = (int)(rest / p.by);
        const int oy0 = byi * WR, ox0 = bxi * WC;
        if (K != 1 || tid < 128) {
            const int quad = (tid >> 3) & (WR * 4 - 1), r = quad >> 2, c = (quad & 3) * 4;
            const int oy = oy0 + r, ch = ot * 64 + sq * 8;
            const _Float16* gp = p.g + (((long)n * p.OH + oy) * p.OW + ox0 + c) * p.O + ch;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (tid < GITEMS && oy < p.OH && ox0 + c + m < p.OW && ch < p.O) v = *(const h8*)(gp + (long)m * p.O);
                gv[m] = v;
            }
        }
        const int iy0 = oy0 * S - p.pad, ix0 = ox0 * S - p.pad;
#pragma unroll
        for (int u = 0; u < XROUNDS; ++u) {
            const int e = K == 1 ? tid - 128 : tid + u * 256, quad = e >> 3, r = quad / QPR, c = (quad - r * QPR) * 4;
            const int iy = iy0 + r, ch = it * 64 + sq * 8;
            const bool rok = e >= 0 && e < XITEMS && iy >= 0 && iy < p.H && ch < p.I;
            const _Float16* xp = p.x + (((long)n * p.H + iy) * p.W + ix0 + c) * p.I + ch;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                const int ix = ix0 + c + m;
                if (rok && c + m < XC && ix >= 0 && ix < p.W) v = *(const h8*)(xp + (long)m * p.I);
                xv[u][m] = v;
            }
        }
    };
    if ((long)blockIdx.y < p.nblocks) fetch(blockIdx.y);
    for (long blk = blockIdx.y; blk < p.nblocks; blk += p.slices) {
        __syncthreads();
        // LDS row = (ch % 8) * 8 + ch / 8: the 8 lanes of a pixel quad hit 8 different 16-byte slots
        if (tid < GITEMS) {
            const int quad = tid >> 3, pp = (quad >> 2) * WC + (quad & 3) * 4;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                h4 w4 = {gv[0][k], gv[1][k], gv[2][k], gv[3][k]};
                *(h4*)(gT + (k * 8 + sq) * GP + pp) = w4;
            }
        }
#pragma unroll
        for (int u = 0; u < XROUNDS; ++u) {
            const int e = K == 1 ? tid - 128 : tid + u * 256, quad = e >> 3, r = quad / QPR, c = (quad - r * QPR) * 4;
            if (e >= 0 && e < XITEMS) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    _Float16* row = xT + (k * 8 + sq) * XP + r * RP;
                    if constexpr (S == 1) {
                        h4 w4 = {xv[u][0][k], xv[u][1][k], xv[u][2][k], xv[u][3][k]};
                        *(h4*)(row + c) = w4;
                    } else {                                         // columns c, c + 2 -> even half, c + 1, c + 3 -> odd half (at + 24)
                        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                        h2 ev = {xv[u][0][k], xv[u][2][k]}, od = {xv[u][1][k], xv[u][3][k]};
                        *(h2*)(row + (c >> 1)) = ev;
                        *(h2*)(row + 24 + (c >> 1)) = od;
                    }
                }
            }
        }
        __syncthreads();
        if (blk + p.slices < p.nblocks) fetch(blk + p.slices);
#pragma unroll 1
        for (int r = 0; r < WR; ++r) {
            const h8 a = *(const h8*)(gT + (wo + j) * GP + r * WC + kg * 8);
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const _Float16* row = xT + (wi + j) * XP + (r * S + ky) * RP + kg * 8;
                const u32x4 e0 = *(const u32x4*)row;
                if constexpr (K == 1) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(h8, e0), acc[0], 0, 0, 0);
                } else {
                    const unsigned e4 = *(const unsigned*)(row + 8);
                    u32x4 sh;                                              // the same 8 pixels shifted by one
                    sh[0] = __builtin_amdgcn_alignbit(e0[1], e0[0], 16); sh[1] = __builtin_amdgcn_alignbit(e0[2], e0[1], 16);
                    sh[2] = __builtin_amdgcn_alignbit(e0[3], e0[2], 16); sh[3] = __builtin_amdgcn_alignbit(e4, e0[3], 16);
                    u32x4 third;
                    if constexpr (S == 1) { third[0] = e0[1]; third[1] = e0[2]; third[2] = e0[3]; third[3] = e4; }       // shifted by two
                    else third = *(const u32x4*)(row + 24);                                                             // the odd columns
                    const h8 b0 = __builtin_bit_cast(h8, e0), b1 = __builtin_bit_cast(h8, S == 1 ? sh : third), b2 = __builtin_bit_cast(h8, S == 1 ? third : sh);
                    acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b0, acc[ky * 3 + 0], 0, 0, 0);
                    acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b1, acc[ky * 3 + 1], 0, 0, 0);
                    acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b2, acc[ky * 3 + 2], 0, 0, 0);
                }
            }
        }
    }
    // partial sums: row (o) = (r & 3) + 8 (r >> 2) + 4 kg, column (i) = j
    float* pp = p.part + (long)blockIdx.y * NT * p.OP * p.IP;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // (LDS row R of a tile holds channel (R % 8) * 8 + R / 8, see the staging)
            const int ro = wo + (r & 3) + 8 * (r >> 2) + 4 * kg, ri = wi + j;
            const int o = ot * 64 + (ro & 7) * 8 + (ro >> 3), i = it * 64 + (ri & 7) * 8 + (ri >> 3);
            pp[((long)t * p.OP + o) * p.IP + i] = acc[t][r];
        }
}

// dw[t][o][i] = sum over slices in a fixed order: G slice groups per workgroup (256 / G elements each), thread (g, el) adds slices g, g + G, ...
// in four interleaved accumulators, the groups are combined in group order through LDS (deterministic for a given shape).  With one thread per
// element over all slices a 64-channel layer (36 864 weights x 512 slices) ran on 144 workgroups of serial strided loads.
template <int G>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* part, float* dw, int slices, int NT, int O, int I, int OP, int IP) {
    __shared__ float red[256];
    constexpr int EL = 256 / G;
    const int el = threadIdx.x % EL, g = threadIdx.x / EL;
    const long total = (long)NT * O * I, e = (long)blockIdx.x * EL + el, sl = (long)NT * OP * IP;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (e < total) {
        const int i = (int)(e % I);
        const long r = e / I;
        const int o = (int)(r % O), t = (int)(r / O);
        const float* pe = part + ((long)t * OP + o) * IP + i;
        int k = g;
        for (; k + 3 * G < slices; k += 4 * G) {
            v0 += pe[k * sl]; v1 += pe[(k + G) * sl]; v2 += pe[(k + 2 * G) * sl]; v3 += pe[(k + 3 * G) * sl];
        }
        for (; k < slices; k += G) v0 += pe[k * sl];
    }
    float v = (v0 + v1) + (v2 + v3);
    if (G > 1) {
        red[threadIdx.x] = v;
        __syncthreads();
        if (g == 0)
            for (int k = 1; k < G; ++k) v += red[k * EL + el];
    }
    if (g == 0 && e < total) dw[e] = v;
}

}  // namespace f16

// pixel slices of the fp16 weight gradient: workgroups in total / (64 x 64 tiles)
// (measured at 256 / 512 / 768 / 1024 workgroups: 3x3 best at 512 = two resident per CU in one round, 467 / 531 / 467 / 478 TFLOP/s at 64 channels
// stride 1, 372 / 449 / 381 at stride 2 -- whose 260-register build held ONE workgroup per CU (346 TFLOP/s) until amdgpu_waves_per_eu(2) brought it to
// 255 without spills; the load-bound 1x1 layers at 1024: 126 / 211 / 237 / 253 at 512 channels)
static long wgrad_f16_slices(long tiles, long nblocks, long wgs) {
    long slices = (wgs + tiles - 1) / tiles;
    if (slices > nblocks) slices = nblocks;
    return slices < 1 ? 1 : slices;
}

extern "C" size_t shg_conv2d_wgrad_f16_workspace_bytes(int N, int I, int O, int OH, int OW, int k) {
    const int OP = (O + 63) / 64 * 64, IP = (I + 63) / 64 * 64;
    const long nblocks = (long)N * shg_cdiv(OH, f16::WR) * shg_cdiv(OW, f16::WC);
    return (size_t)wgrad_f16_slices((long)(OP / 64) * (IP / 64), nblocks, k == 1 ? 1024 : 512) * k * k * OP * IP * sizeof(float);
}

// dw [k*k][O][I] fp32 = sum_{n,oy,ox} g[n,oy,ox,o] x[n, oy*stride - pad + ky, ox*stride - pad + kx, i]; x [N,H,W,I], g [N,OH,OW,O] halves
extern "C" int shg_conv2d_wgrad_f16(const void* x, const void* g, float* dw, int N, int I, int O, int H, int W, int OH, int OW, int k, int stride,
                                    int pad, void* workspace, size_t ws_bytes, void* stream) {
    SHG_CHECK_ARG(x && g && dw && workspace, "conv2d_wgrad_f16: null pointer");
    SHG_CHECK_ARG(N >= 1 && I >= 8 && (I % 8) == 0 && O >= 8 && (O % 8) == 0, "conv2d_wgrad_f16: I and O must be multiples of 8");
    SHG_CHECK_ARG((k == 1 || k == 3) && (stride == 1 || stride == 2) && pad >= 0, "conv2d_wgrad_f16: 1x1 / 3x3 kernels, stride 1 / 2");
    SHG_CHECK_ARG(OH == (H + 2 * pad - k) / stride + 1 && OW == (W + 2 * pad - k) / stride + 1, "conv2d_wgrad_f16: output extent");
    SHG_CHECK_ARG(ws_bytes >= shg_conv2d_wgrad_f16_workspace_bytes(N, I, O, OH, OW, k), "conv2d_wgrad_f16: workspace too small");
    f16::WgradP p{};
    p.x = (const _Float16*)x; p.g = (const _Float16*)g; p.part = (float*)workspace;
    p.N = N; p.I = I; p.O = O; p.H = H; p.W = W; p.OH = OH; p.OW = OW; p.s = stride; p.pad = pad; p.k = k;
    p.OP = (O + 63) / 64 * 64; p.IP = (I + 63) / 64 * 64;
    const int wr = f16::wgrad_rows(k, stride);
    p.by = shg_cdiv(OH, wr); p.bx = shg_cdiv(OW, f16::WC);
    p.nblocks = (long)N * p.by * p.bx;
    const long tiles = (long)(p.OP / 64) * (p.IP / 64);
    const long slices = wgrad_f16_slices(tiles, p.nblocks, k == 1 ? 1024 : 512);
    p.slices = (int)slices;
    SHG_CHECK_ARG(!(k == 1 && stride == 2), "conv2d_wgrad_f16: 1x1 stride-2 (the forward decimates with upfirdn2d first)");
    p.XR = (wr - 1) * stride + k; p.XC = (f16::WC - 1) * stride + k;
    const size_t lds = ((size_t)64 * (wr * f16::WC + 8) + (size_t)64 * (p.XR * (stride == 1 ? 24 : 48) + 8)) * sizeof(_Float16);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)slices);
    if (k == 3 && stride == 1) hipLaunchKernelGGL((f16::conv_wgrad_f16_kernel<3, 1>), grid, dim3(256), lds, st, p);
    else if (k == 3) hipLaunchKernelGGL((f16::conv_wgrad_f16_kernel<3, 2>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((f16::conv_wgrad_f16_kernel<1, 1>), grid, dim3(256), lds, st, p);
    SHG_CHECK_LAUNCH();
    const long total = (long)k * k * O * I;
    int G = 1;
    while (G < 16 && (total + 256 / G - 1) / (256 / G) < 2048 && p.slices >= 8 * G) G *= 2;
    const dim3 rgrid((unsigned)((total + 256 / G - 1) / (256 / G)));
    const float* part = (const float*)workspace;
    switch (G) {
        case 1: hipLaunchKernelGGL(f16::wgrad_reduce_kernel<1>, rgrid, dim3(256), 0, st, part, dw, p.slices, k * k, O, I, p.OP, p.IP); break;
        case 2: hipLaunchKernelGGL(f16::wgrad_reduce_kernel<2>, rgrid, dim3(256), 0, st, part, dw, p.slices, k * k, O, I, p.OP, p.IP); break;
        case 4: hipLaunchKernelGGL(f16::wgrad_reduce_kernel<4>, rgrid, dim3(256), 0, st, part, dw, p.slices, k * k, O, I, p.OP, p.IP); break;
        case 8: hipLaunchKernelGGL(f16::wgrad_reduce_kernel<8>, rgrid, dim3(256), 0, st, part, dw, p.slices, k * k, O, I, p.OP, p.IP); break;
        default: hipLaunchKernelGGL(f16::wgrad_reduce_kernel<16>, rgrid, dim3(256), 0, st, part, dw, p.slices, k * k, O, I, p.OP, p.IP); break;
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
