// fp16 convolutions of the training / config-5 rows (reference: the `use_fp16` branches -- stylegan.py:136-138,486,660-667,
// comodgan.py:40-47,305 -- whose convolutions are cuDNN half kernels with fp32 accumulation): the gather kernel, the routing of a launch to
// it or to one of the persistent kernels (conv_f16_ring.hip, conv_f16_upring.hip, conv_f16_down.hip), and the weight packers.  gfx950 only.
// The other fp16 families live beside it: conv_wgrad_f16.hip (weight gradient), upfirdn2d_f16.hip (FIR resampling), pointwise_f16.hip
// (bias_act, modulation tail, fp32 <-> fp16 relayouts).
//
// Data layout (all fp16 files): fp16 activations live in HBM channels-LAST ([N,H,W,C], torch.channels_last on a [N,C,H,W] tensor): the
// v_mfma_f32_32x32x16_f16 operands are 8 consecutive K values per lane, and with K = input channels that is ONE 16-byte load
// per lane from an NHWC tensor (an NCHW tensor would need a transposing gather for every operand).  Weights are prepared as
// [tap][O][I] (I fastest), accumulation is fp32, results are rounded to fp16 once.
//
//   conv_f16_kernel      y[n,oy,ox,o] = sum_t sum_i w[t][o][i] * x[n, oy'*s_in + dy_t, ox'*s_in + dx_t, i]  with the output pixel
//                        (oy,ox) = (oy'*s_out + oy0, ox'*s_out + ox0): stride-1 / stride-2 convolutions (s_out = 1) and, launched once
//                        per sub-pixel phase, the stride-2 transposed convolution (s_out = 2, each phase has its own 1 / 2 / 4 taps:
//                        no multiplies by inserted zeros).  Implicit GEMM: M = output channels (A = weights, global/L2 -> registers),
//                        N = a tile of 8x16 output pixels (B = the input patch of a 32-channel chunk in LDS, one ds_read_b128 per
//                        operand, pixel stride 80 B = conflict-free), K = taps x channels.
#include "shg_common.h"
#include "conv_f16_p.h"

namespace f16 {

constexpr int TH = 8, TW = 16;       // output-pixel tile of a workgroup (4 waves x 2 rows x 16 columns)
constexpr int KC = 32;               // channels per LDS chunk (two MFMA k-steps)
constexpr int PSTR = 40;             // halves per staged pixel: 32 + 8 padding -> 80-byte stride, conflict-free ds_read_b128


template <int MB, int NT, int NB, bool WLDS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MB == 2 && NB == 2 && !WLDS) ? 3 : 1))) void conv_f16_kernel(const ConvP p) {
    // tile = TH x (16 NB) output pixels: wave w owns rows 2w, 2w+1; with NB = 1 its 32 lanes-of-a-block are 2 rows x 16 columns, with
    // NB = 2 block nb is row 2w + nb and the lanes are its 32 columns -- every weight operand then feeds two MFMAs
    extern __shared__ __attribute__((aligned(16))) _Float16 patch[];
    constexpr int TWK = TW * NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kg = lane >> 5;
    int tile = blockIdx.x;
    const int tx = tile % p.tiles_x;
    tile /= p.tiles_x;
    const int ty = tile % p.tiles_y, n = tile / p.tiles_y;
    const int ob0 = blockIdx.y * MB;                                                   // first 32-channel block of this workgroup
    const int ry = NB == 1 ? wave * 2 + (j >> 4) : wave * 2, rx = NB == 1 ? (j & 15) : j;   // lane's pixel inside the tile (block 0)
    const int iy_base = ty * TH * p.s_in + p.org_y, ix_base = tx * TWK * p.s_in + p.org_x;
    f16x acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][b][r] = 0.f;
    const int npix = p.PH * p.PW;
    const _Float16* xn = p.x + (long)n * p.H * p.W * p.I;
    const int c16n = p.I >> 4;
    // weights in MFMA operand order: [32-channel block][tap slot][16-channel k-step][lane][8] -- one coalesced 1 KiB load per operand
    const _Float16* wl = p.w + (long)lane * 8;
    // Patch staging, software-pipelined: 4 lanes x 16 bytes per pixel; the pixel -> address map does not depend on the channel chunk,
    // so it is computed once; the loads of chunk c+1 are issued BEFORE the multiply loop of chunk c and land in LDS after it.
    constexpr int SIT = NB == 2 ? 6 : 9;                            // ceil(max patch pixels / 64): 10 x 34 (NB = 2), 17 x 33 (stride 2)
    int goff[SIT];
    const int q8 = (tid & 3) * 8;
#pragma unroll
    for (int it = 0; it < SIT; ++it) {
        const int pp = (tid >> 2) + it * 64, py = pp / p.PW, px = pp - py * p.PW;
        const int iy = iy_base + py, ix = ix_base + px;
        goff[it] = (pp < npix && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? iy * p.W + ix : -1;
    }
    h8 stage[SIT];
    auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (goff[it] >= 0) v = *(const h8*)(xn + (long)goff[it] * p.I + c0 + q8);
            stage[it] = v;
        }
        if (p.in_scale) {                                           // `x * styles.to(x.dtype)` (stylegan.py:173): half x half -> half
            const float* sp = p.in_scale + (long)n * p.I + c0 + q8;
            _Float16 sh[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) sh[k] = (_Float16)sp[k];
#pragma unroll
            for (int it = 0; it < SIT; ++it)
#pragma unroll
                for (int k = 0; k < 8; ++k) stage[it][k] = stage[it][k] * sh[k];
        }
    };
    // WLDS: the weight slab of a chunk ([MB blocks][NT taps][2 k-steps] pieces of 1 KiB, already in operand order) is staged ONCE per
    // workgroup through the same register pipeline and read from LDS lane-linearly (conflict-free) -- instead of every wave loading every
    // operand from L2 one tap ahead (half the wave cycles parked on those loads, profiles/r03_f16_pmc_summary.txt)
    constexpr int WPC = MB * NT * 2, WIT = WLDS ? (WPC + 3) / 4 : 1;      // pieces per chunk; a pass of the 256 threads moves 4 pieces
    _Float16* wlds = patch + p.wlds_off;
    h8 wstage[WIT];
    auto fetch_w = [&](int c0) __attribute__((always_inline)) {
        if constexpr (WLDS) {
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pi = it * 4 + wave;                          // piece = (m * NT + t) * 2 + ks
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (pi < WPC) {
                    const int ks = pi & 1, mt = pi >> 1, m = mt / NT, t = mt - m * NT;
                    v = *(const h8*)(wl + ((((long)(ob0 + m) * p.wslots + p.tw[t]) * c16n + (c0 >> 4) + ks) << 9));
                }
                wstage[it] = v;
            }
        }
    };
    fetch(0);
    fetch_w(0);
    for (int c0 = 0; c0 < p.I; c0 += KC) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            const int pp = (tid >> 2) + it * 64;
            if (pp < npix) *(h8*)(patch + pp * PSTR + q8) = stage[it];
        }
        if constexpr (WLDS) {
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pi = it * 4 + wave;
                if (pi < WPC) *(h8*)(wlds + pi * 512 + lane * 8) = wstage[it];
            }
        }
        __syncthreads();
        if (c0 + KC < p.I) { fetch(c0 + KC); fetch_w(c0 + KC); }
        // Weight operands: unconditional loads (the packed tensor is zero-padded to whole MB groups of blocks and I % 32 == 0), those of
        // tap t+1 requested before the MFMAs of tap t -- a conditional load would be waited for on the spot (vmcnt(0) per MFMA pair).
        const _Float16* wc = wl + ((long)ob0 * p.wslots * c16n + (c0 >> 4)) * 512;
        constexpr int AD = 1;                                       // operand prefetch distance in taps (ring of AD + 1 slots)
        h8 a[AD + 1][2][MB];
        if constexpr (!WLDS) {
#pragma unroll
            for (int t = 0; t < AD && t < NT; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < MB; ++m) a[t][ks][m] = *(const h8*)(wc + (((long)m * p.wslots + p.tw[t]) * c16n + ks) * 512);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (WLDS) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < MB; ++m) a[t % (AD + 1)][ks][m] = *(const h8*)(wlds + ((m * NT + t) * 2 + ks) * 512 + lane * 8);
            } else if (t + AD < NT) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < MB; ++m) a[(t + AD) % (AD + 1)][ks][m] = *(const h8*)(wc + (((long)m * p.wslots + p.tw[t + AD]) * c16n + ks) * 512);
            }
            // the compiler otherwise sinks the operand requests to just before their use (measured: 3-8 % on the 128 / 256-channel layers)
            __builtin_amdgcn_sched_barrier(0);
            const _Float16* bp = patch + ((ry * p.s_in + p.tdy[t]) * p.PW + rx * p.s_in + p.tdx[t]) * PSTR + kg * 8;
            h8 b[2][NB];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int q = 0; q < NB; ++q) b[ks][q] = *(const h8*)(bp + q * p.s_in * p.PW * PSTR + ks * 16);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int q = 0; q < NB; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t % (AD + 1)][ks][m], b[ks][q], acc[m][q], 0, 0, 0);
        }
    }
    // C/D layout: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  A lane holds 4-channel runs of ONE
    // pixel: stored directly, every store instruction would touch 64 different 128-byte lines with 8 bytes each.  The tile is therefore
    // transposed through LDS (pixel-major, 16 bytes of padding per pixel) and leaves as whole 16-byte pieces of contiguous channel runs.
    constexpr int OPS = MB * 32 + 8;
    float bv[MB][4][4];                                             // bias of a lane's channels (no-tail launches), requested before the barrier
    const bool pre_bias = p.bias && !p.tail;
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = ob0 * 32 + m * 32 + qq * 8 + kg * 4 + e;
                bv[m][qq][e] = pre_bias ? p.bias[o < p.O ? o : p.O - 1] : 0.f;
            }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int pl = NB == 1 ? ry * TW + rx : (ry + q) * TWK + rx;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int ol = m * 32 + qq * 8 + kg * 4;
                h4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (_Float16)(acc[m][q][qq * 4 + e] + bv[m][qq][e]);
                *(h4*)(patch + pl * OPS + ol) = v;
            }
    }
    __syncthreads();
    constexpr int PCS = MB * 4;                                   // 16-byte pieces per pixel
    if ((p.O & 7) == 0) {
        // whole 8-channel pieces: all LDS reads first, every operand load unconditional (clamped address), only the store predicated -- a
        // rolled loop with early exits spent 550 cycles per piece (clock trace: LDS latency + address arithmetic in series)
        constexpr int EIT = TH * TWK * PCS / 256, EG = EIT < 4 ? EIT : 4;    // pieces per thread, in groups of EG (registers)
        for (int i0 = 0; i0 < EIT; i0 += EG) {
        h8 vv[EG];
#pragma unroll
        for (int it = 0; it < EG; ++it) {
            const int e = tid + (i0 + it) * 256, pl = e / PCS, pc = e - pl * PCS;
            vv[it] = *(const h8*)(patch + pl * OPS + pc * 8);
        }
#pragma unroll
        for (int it = 0; it < EG; ++it) {
            const int e = tid + (i0 + it) * 256, pl = e / PCS, pc = e - pl * PCS, row = pl / TWK, col = pl - row * TWK;
            const int gy = ty * TH + row, gx = tx * TWK + col;
            const int oy = gy * p.s_out + p.oy0, ox = gx * p.s_out + p.ox0, o = ob0 * 32 + pc * 8;
            const bool ok = gy < p.GH && gx < p.GW && oy >= 0 && oy < p.OHt && ox >= 0 && ox < p.OWt && o < p.O;
            const int oyc = oy < 0 ? 0 : (oy < p.OHt ? oy : p.OHt - 1), oxc = ox < 0 ? 0 : (ox < p.OWt ? ox : p.OWt - 1), oc = o < p.O ? o : p.O - 8;
            const long pix = (long)oyc * p.OWt + oxc, off = ((long)n * p.OHt * p.OWt + pix) * p.O + oc;
            h8 v = vv[it];
            if (p.tail) {
                const float nz = p.noise_mode == 0 ? 0.f : p.noise[(p.noise_mode == 2 ? (long)n * p.OHt * p.OWt : 0) + pix] * p.noise_strength;
                const float4 d0 = p.out_scale ? *(const float4*)(p.out_scale + (long)n * p.O + oc) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float4 d1 = p.out_scale ? *(const float4*)(p.out_scale + (long)n * p.O + oc + 4) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float4 b0 = p.bias ? *(const float4*)(p.bias + oc) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 b1 = p.bias ? *(const float4*)(p.bias + oc + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                h8 rs = {0, 0, 0, 0, 0, 0, 0, 0};
                if (p.residual) rs = *(const h8*)(p.residual + off);
                const float dd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float z = __builtin_fmaf((float)v[k], dd[k], nz) + bb[k];     // (spelled out: conv_f16_ring.hip's tail is the same expression)
                    z = p.act ? shg_lrelu_agc(z, p.alpha, p.gain, p.clamp) : z * p.gain;
                    v[k] = (_Float16)((float)(_Float16)z + (float)rs[k]);
                }
            }
            if (ok) *(h8*)(p.y + off) = v;
        }
        }
    } else
    for (int e = tid; e < TH * TWK * PCS; e += 256) {
        const int pl = e / PCS, pc = e - pl * PCS, row = pl / TWK, col = pl - row * TWK;
        const int gy = ty * TH + row, gx = tx * TWK + col;
        if (gy >= p.GH || gx >= p.GW) continue;
        const int oy = gy * p.s_out + p.oy0, ox = gx * p.s_out + p.ox0;
        if (oy < 0 || oy >= p.OHt || ox < 0 || ox >= p.OWt) continue;
        const int o = ob0 * 32 + pc * 8;
        _Float16* yp = p.y + (((long)n * p.OHt + oy) * p.OWt + ox) * p.O + o;
        h8 v = *(const h8*)(patch + pl * OPS + pc * 8);
        if (p.tail) {                                               // the layer tail on the half-rounded convolution result, as the reference applies it
            const long pix = (long)oy * p.OWt + ox;
            const float nz = p.noise_mode == 0 ? 0.f : p.noise[(p.noise_mode == 2 ? (long)n * p.OHt * p.OWt : 0) + pix] * p.noise_strength;
            const bool full = (p.O & 7) == 0 && o + 7 < p.O;
            float dd[8], bb[8];
            h8 rs = {0, 0, 0, 0, 0, 0, 0, 0};
            if (full) {                                             // 8 consecutive channels: vector loads of the per-channel operands
                const float4 d0 = p.out_scale ? *(const float4*)(p.out_scale + (long)n * p.O + o) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float4 d1 = p.out_scale ? *(const float4*)(p.out_scale + (long)n * p.O + o + 4) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float4 b0 = p.bias ? *(const float4*)(p.bias + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 b1 = p.bias ? *(const float4*)(p.bias + o + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                dd[0] = d0.x; dd[1] = d0.y; dd[2] = d0.z; dd[3] = d0.w; dd[4] = d1.x; dd[5] = d1.y; dd[6] = d1.z; dd[7] = d1.w;
                bb[0] = b0.x; bb[1] = b0.y; bb[2] = b0.z; bb[3] = b0.w; bb[4] = b1.x; bb[5] = b1.y; bb[6] = b1.z; bb[7] = b1.w;
                if (p.residual) rs = *(const h8*)(p.residual + (yp - p.y));
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int oc = o + k < p.O ? o + k : p.O - 1;
                    dd[k] = p.out_scale ? p.out_scale[(long)n * p.O + oc] : 1.f;
                    bb[k] = p.bias ? p.bias[oc] : 0.f;
                    if (p.residual && o + k < p.O) rs[k] = p.residual[(yp - p.y) + k];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float z = __builtin_fmaf((float)v[k], dd[k], nz) + bb[k];     // (spelled out: conv_f16_ring.hip's tail is the same expression)
                z = p.act ? shg_lrelu_agc(z, p.alpha, p.gain, p.clamp) : z * p.gain;
                v[k] = (_Float16)((float)(_Float16)z + (float)rs[k]);
            }
        }
        if ((p.O & 7) == 0 && o + 7 < p.O) *(h8*)yp = v;
        else
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (o + k < p.O) yp[k] = v[k];
    }
}

template <int MB, int NB>
static int launch_conv(ConvP p, hipStream_t st) {
    const dim3 grid((unsigned)((long)p.N * p.tiles_x * p.tiles_y), (unsigned)shg_cdiv(p.OB, MB));
    size_t lds = (size_t)p.PH * p.PW * PSTR * sizeof(_Float16);
    const size_t out_tile = (size_t)TH * TW * NB * (MB * 32 + 8) * sizeof(_Float16);       // the epilogue's transposed output tile reuses the patch
    if (out_tile > lds) lds = out_tile;
    // Thick 3x3 layers (I >= 384: >= 12 chunks per tile) stage their weight slab in LDS (MB * 9 * 2 KiB behind the patch): 206 -> 181 us at
    // 512 channels.  Thin layers lose (64 ch: 256 -> 312 us, 128 ch: 196 -> 214: two chunks cannot amortise the second staging stream and the
    // 232-register kernel), MB = 4 would need 72 KB + the patch: both keep the L2 route with one-tap-ahead operand prefetch.
    const bool wl = p.ntaps == 9 && MB <= 2 && p.I >= 384;
    p.wlds_off = (int)(lds / sizeof(_Float16));
    if (wl) lds += (size_t)MB * 9 * 2 * 1024;
    switch (p.ntaps) {
        case 1: hipLaunchKernelGGL((conv_f16_kernel<MB, 1, NB, false>), grid, dim3(256), lds, st, p); break;
        case 2: hipLaunchKernelGGL((conv_f16_kernel<MB, 2, NB, false>), grid, dim3(256), lds, st, p); break;
        case 4: hipLaunchKernelGGL((conv_f16_kernel<MB, 4, NB, false>), grid, dim3(256), lds, st, p); break;
        case 9:
            if (wl) hipLaunchKernelGGL((conv_f16_kernel<MB, 9, NB, (MB <= 2)>), grid, dim3(256), lds, st, p);
            else hipLaunchKernelGGL((conv_f16_kernel<MB, 9, NB, false>), grid, dim3(256), lds, st, p);
            break;
        default: shg_set_error("conv2d_f16: %d taps", p.ntaps); return SHG_ERR_UNSUPPORTED;
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// one launch of the gather convolution for a tap list; dy/dx are INPUT offsets relative to (oy'*s_in, ox'*s_in)
static int conv_taps(ConvP p, int ntaps, const int* dy, const int* dx, const int* slot, int GH, int GW, hipStream_t st) {
    if (GH <= 0 || GW <= 0) return SHG_OK;
    int mny = dy[0], mxy = dy[0], mnx = dx[0], mxx = dx[0];
    for (int t = 1; t < ntaps; ++t) {
        mny = dy[t] < mny ? dy[t] : mny; mxy = dy[t] > mxy ? dy[t] : mxy;
        mnx = dx[t] < mnx ? dx[t] : mnx; mxx = dx[t] > mxx ? dx[t] : mxx;
    }
    p.ntaps = ntaps;
    for (int t = 0; t < ntaps; ++t) { p.tdy[t] = dy[t] - mny; p.tdx[t] = dx[t] - mnx; p.tw[t] = slot[t]; }
    p.org_y = mny; p.org_x = mnx;
    p.GH = GH; p.GW = GW;
    if (conv_ring_eligible(p, mxy - mny + 1, mxx - mnx + 1)) return conv_ring_launch(p, st);
    if (mny == mnx && mxy - mny == 2 && mxx - mnx == 2 && conv_down_eligible(p)) return conv_down_launch(p, -mny, st);
    // wide grids of stride-1 reads: 8 x 32 pixel tiles, two pixel blocks per wave (each weight operand feeds two MFMAs); stride-2 reads
    // (a 4x larger patch) and narrow grids keep 8 x 16
    const int nb = (p.s_in == 1 && GW > TW) ? 2 : 1;
    p.PH = (TH - 1) * p.s_in + (mxy - mny) + 1;
    p.PW = (TW * nb - 1) * p.s_in + (mxx - mnx) + 1;
    p.GH = GH; p.GW = GW;
    p.tiles_y = shg_cdiv(GH, TH); p.tiles_x = shg_cdiv(GW, TW * nb);
    if (nb == 2) {                   // (4 channel blocks x 2 pixel blocks need 290 VGPRs = one wave per SIMD: 2 x 2 keeps three)
        if (p.OB > 1) return launch_conv<2, 2>(p, st);
        return launch_conv<1, 2>(p, st);
    }
    if (p.OB > 2) return launch_conv<4, 1>(p, st);
    if (p.OB > 1) return launch_conv<2, 1>(p, st);
    return launch_conv<1, 1>(p, st);
}

}  // namespace f16

// x [N,H,W,I] halves, bias fp32 [O] or null, y halves.  w: k*k tap slots (cross-correlation taps in row-major (ky,kx) order) packed in MFMA operand
// order by shg_conv2d_f16_pack_weight: [ceil(O/32)][k*k][I/16][64][8] halves.
//   mode 0: y[N,OH,OW,O] = conv2d(x, w, stride, pad)                      OH = (H + 2 pad - k) / stride + 1
//   mode 1: y[N,OH,OW,O] = rows / columns [crop, crop + OH) of conv_transpose2d(x, w, stride 2) (3x3; w[t][o][i] = torch weight[i][o][ky][kx]),
//           zero where the (2H+1) x (2W+1) result ends earlier.  I % 32 == 0.
struct shg_f16_tail_ { const float* in_scale; const float* out_scale; const float* noise; int noise_mode; float noise_strength; int act; float alpha, gain, clamp; const void* residual; };

static int conv2d_f16_impl(const void* x, const void* w, const float* bias, void* y, int N, int I, int O, int H, int W, int k, int stride,
                           int pad, int mode, int crop, int OH, int OW, const shg_f16_tail_* tl, void* stream) {
    SHG_CHECK_ARG(x && w && y, "conv2d_f16: null pointer");
    SHG_CHECK_ARG(N >= 1 && I >= 32 && (I % 32) == 0 && O >= 1 && H >= 1 && W >= 1, "conv2d_f16: bad shape (I must be a multiple of 32)");
    SHG_CHECK_ARG((k == 1 || k == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad <= k, "conv2d_f16: 1x1 / 3x3 kernels, stride 1 / 2");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w)) & 15) == 0,
                  "conv2d_f16: x, w and y must be 16-byte aligned (vector loads / stores)");
    f16::ConvP p{};
    p.x = (const _Float16*)x; p.w = (const _Float16*)w; p.bias = bias; p.y = (_Float16*)y;
    p.N = N; p.I = I; p.O = O; p.H = H; p.W = W; p.OHt = OH; p.OWt = OW;
    p.OB = (O + 31) / 32; p.wslots = k * k;
    if (tl) {
        p.in_scale = tl->in_scale; p.out_scale = tl->out_scale; p.noise = tl->noise_mode ? tl->noise : nullptr; p.noise_mode = tl->noise ? tl->noise_mode : 0;
        p.noise_strength = tl->noise_strength; p.act = tl->act; p.alpha = tl->alpha; p.gain = tl->gain; p.clamp = tl->clamp;
        p.residual = (const _Float16*)tl->residual;
        p.tail = (tl->out_scale || p.noise_mode || tl->act || tl->gain != 1.f || tl->residual) ? 1 : 0;
    }
    p.gain = p.tail ? p.gain : 1.f;
    hipStream_t st = (hipStream_t)stream;
    int dy[9], dx[9], slot[9];
    if (mode == 0) {
        SHG_CHECK_ARG(OH == (H + 2 * pad - k) / stride + 1 && OW == (W + 2 * pad - k) / stride + 1 && OH >= 1 && OW >= 1, "conv2d_f16: output extent");
        p.s_in = stride; p.s_out = 1; p.oy0 = 0; p.ox0 = 0;
        for (int t = 0; t < k * k; ++t) { dy[t] = t / k - pad; dx[t] = t % k - pad; slot[t] = t; }
        return f16::conv_taps(p, k * k, dy, dx, slot, OH, OW, st);
    }
    SHG_CHECK_ARG(mode == 1 && k == 3 && stride == 2 && crop >= 0 && OH >= 1 && OW >= 1, "conv2d_f16: the transposed form is 3x3 stride 2");
    // full[oy][ox] = sum_{ky,kx} x[(oy-ky)/2][(ox-kx)/2] w[ky][kx] over even (oy-ky), (ox-kx); phase (py,px) = parity of (oy,ox)
    if (f16::convt_upring_eligible(p)) return f16::convt_upring_launch(p, crop, st);      // all four phases from one pass over the input
    p.s_in = 1; p.s_out = 2;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            int nt = 0;
            for (int ky = py; ky < 3; ky += 2)
                for (int kx = px; kx < 3; kx += 2) { dy[nt] = -(ky / 2); dx[nt] = -(kx / 2); slot[nt] = ky * 3 + kx; ++nt; }
            p.oy0 = py - crop; p.ox0 = px - crop;
            // grid rows oy' with 0 <= 2 oy' + py < 2H+1 intersected with the crop window [crop, crop + OH)
            const int GH = py ? H : H + 1, GW = px ? W : W + 1;
            const int rc = f16::conv_taps(p, nt, dy, dx, slot, GH, GW, st);
            if (rc != SHG_OK) return rc;
        }
    return SHG_OK;
}


extern "C" int shg_conv2d_f16(const void* x, const void* w, const float* bias, void* y, int N, int I, int O, int H, int W, int k, int stride,
                              int pad, int mode, int crop, int OH, int OW, void* stream) {
    return conv2d_f16_impl(x, w, bias, y, N, I, O, H, W, k, stride, pad, mode, crop, OH, OW, nullptr, stream);
}

// The same convolution with the layer tail of the INFERENCE route fused (half layers under no_grad): x * in_scale[n,i] (half x half) while the
// patch is staged -- both modes --, and for mode 0: y = A(conv * out_scale[n,o] + noise * noise_strength + bias[o]) + residual applied to the
// half-rounded convolution result in the store pass (stylegan.py:173-181,298-304; comodgan.py:320-327).  in_scale [N,I], out_scale [N,O], noise
// [OH,OW] (noise_mode 1) / [N,OH,OW] (2), bias [O]: fp32, each optional; residual: halves like y; act = 0: (..) * gain.
extern "C" int shg_conv2d_f16_fused(const void* x, const void* w, void* y, int N, int I, int O, int H, int W, int k, int stride, int pad, int mode,
                                    int crop, int OH, int OW, const float* in_scale, const float* out_scale, const float* noise, int noise_mode,
                                    float noise_strength, const float* bias, int act, float alpha, float gain, float clamp, const void* residual,
                                    void* stream) {
    SHG_CHECK_ARG(mode == 0 || !(out_scale || noise || act || residual || gain != 1.f), "conv2d_f16_fused: the transposed form takes in_scale only (its tail follows the FIR)");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(residual) |
                    reinterpret_cast<uintptr_t>(out_scale) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                  "conv2d_f16: x, w, y, residual, out_scale and bias must be 16-byte aligned (vector loads)");
    const shg_f16_tail_ tl{in_scale, out_scale, noise, noise_mode, noise_strength, act, alpha, gain, clamp, residual};
    return conv2d_f16_impl(x, w, bias, y, N, I, O, H, W, k, stride, pad, mode, crop, OH, OW, &tl, stream);
}

// w [T][O][I] halves (T tap slots) -> MFMA operand order [ceil(O/32)][T][I/16][64][8], rows beyond O zero
__global__ __launch_bounds__(256) void pack_weight_f16_kernel(const _Float16* w, _Float16* wp, int T, int O, int I, long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int el = (int)(e & 7), lane = (int)((e >> 3) & 63);
        long r = e >> 9;
        const int c16n = I >> 4, c16 = (int)(r % c16n);
        r /= c16n;
        const int t = (int)(r % T), ob = (int)(r / T);
        const int o = ob * 32 + (lane & 31), i = c16 * 16 + (lane >> 5) * 8 + el;
        wp[e] = o < O ? w[((long)t * O + o) * I + i] : (_Float16)0.f;
    }
}

// (32-channel blocks rounded up to a multiple of 4: the kernel loads the operands of whole groups of MB <= 4 blocks unconditionally)
extern "C" long shg_conv2d_f16_packed_weight_elems(int T, int O, int I) { return (long)(((O + 31) / 32 + 3) / 4 * 4) * T * (I / 16) * 512; }

extern "C" int shg_conv2d_f16_pack_weight(const void* w, void* wp, int T, int O, int I, void* stream) {
    SHG_CHECK_ARG(w && wp && T >= 1 && O >= 1 && I >= 32 && (I % 32) == 0, "conv2d_f16_pack_weight: bad arguments (I must be a multiple of 32)");
    const long total = shg_conv2d_f16_packed_weight_elems(T, O, I);
    int grid = shg_cdiv(total, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(pack_weight_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)w, (_Float16*)wp, T, O, I, total);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// The same operand order straight from a torch-layout weight: src [A][B][T] halves (T = k*k), logical W[o][i][t] = src[o][i][t] (A = O, B = I)
// or, `transposed`, src[i][o][t] (A = I, B = O: the conv_transpose2d layout / the channel-transposed weight of an input gradient); `flip`
// reverses the taps (t -> T-1-t: the 180-degree rotation of an input gradient).  Input channels beyond I read zero (Ip = I rounded up to 32).
// One gather pass instead of flip + permute-copy + pack (three launches per fp16 data-gradient convolution).
__global__ __launch_bounds__(256) void pack_weight_oihw_f16_kernel(const _Float16* src, _Float16* wp, int T, int O, int I, int Ip, int transposed, int flip,
                                                                   long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int el = (int)(e & 7), lane = (int)((e >> 3) & 63);
        long r = e >> 9;
        const int c16n = Ip >> 4, c16 = (int)(r % c16n);
        r /= c16n;
        const int t = (int)(r % T), ob = (int)(r / T);
        const int o = ob * 32 + (lane & 31), i = c16 * 16 + (lane >> 5) * 8 + el;
        const int ts = flip ? T - 1 - t : t;
        _Float16 v = (_Float16)0.f;
        if (o < O && i < I) v = transposed ? src[((long)i * O + o) * T + ts] : src[((long)o * I + i) * T + ts];
        wp[e] = v;
    }
}

extern "C" int shg_conv2d_f16_pack_weight_oihw(const void* src, void* wp, int T, int O, int I, int transposed, int flip, void* stream) {
    SHG_CHECK_ARG(src && wp && (T == 1 || T == 9) && O >= 1 && I >= 1, "conv2d_f16_pack_weight_oihw: bad arguments");
    const int Ip = (I + 31) / 32 * 32;
    const long total = shg_conv2d_f16_packed_weight_elems(T, O, Ip);
    int grid = shg_cdiv(total, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(pack_weight_oihw_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)src, (_Float16*)wp, T, O, I, Ip,
                       transposed, flip, total);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// the transposed form writes every pixel of its crop window only where the (2H+1) x (2W+1) result exists: callers zero y first when
// crop + OH > 2H + 1 (shg_conv2d_f16_needs_clear says so)
extern "C" int shg_conv2d_f16_needs_clear(int H, int W, int crop, int OH, int OW) {
    return (crop + OH > 2 * H + 1 || crop + OW > 2 * W + 1) ? 1 : 0;
}
