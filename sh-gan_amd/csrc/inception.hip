// Inception-v3 FID detector (the feature extractor of the TF graph `inception-2015-12-05`, as the reference's eva_fid.py loads it):
// front end, convolution + folded BatchNorm + ReLU, pools and the final global mean.  Float32 NCHW throughout; the convolutions are
// an implicit GEMM on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain per output, no reduced precision).
//
// Convolution GEMM: rows = output channels (A = packed weight [Kp][Np], K in tap-major order k = (ky*kw + kx)*I + c), columns =
// output pixels m = (b, oy, ox) (B = the input window gathered on the fly), so that the accumulator's lane index runs over pixels and
// the epilogue's stores are 128-byte row segments of one output channel plane.  One workgroup = 64 channels x 64 pixels, four waves
// of 32 x 32, K in steps of 16 through two LDS stages (one barrier per step).  When I % 16 == 0 a K-step lies inside one tap: the
// window offset and the border test are computed once per step, and the four values a thread stages are one channel apart.
// The epilogue writes at a channel offset of the Mixed block's concat buffer (no concat pass).  Several independent convolutions
// (the branches of a Mixed block at one depth) are one grouped launch; a group may split K over `splitk` workgroups, whose fp32
// partial sums go to the workspace and are added in a fixed order (split index ascending) by a second, grouped launch.
#include "det_conv_tile.h"
#include "../../include/shgan_hip.h"

#define INC_OUT 299      // the detector's input resolution

struct IncConvArgs {
    shg_inc_conv_desc g[SHG_INC_MAX_GROUPS];
    int first_block[SHG_INC_MAX_GROUPS + 1];   // prefix sum of mt * nt * splitk
    long ws_off[SHG_INC_MAX_GROUPS];           // float offset of the group's partial sums in the workspace (split groups only)
    float* ws;
    int G, B;
};

__global__ __launch_bounds__(256) void inc_conv_kernel(const IncConvArgs a) {
    __shared__ float Ws[2][DET_BK][DET_BM];
    __shared__ float Xs[2][DET_BK][DET_BN];
    int gi = 0;
    while (gi + 1 < a.G && (int)blockIdx.x >= a.first_block[gi + 1]) ++gi;
    const shg_inc_conv_desc& g = a.g[gi];
    int local = (int)blockIdx.x - a.first_block[gi];
    const int S = g.splitk;
    const int s = local % S;
    local /= S;
    const int NT = (g.O + DET_BM - 1) / DET_BM, Np = NT * DET_BM;
    const int nt = local % NT, mt = local / NT;
    const int OHW = g.OH * g.OW, M = a.B * OHW;
    const int K = g.I * g.kh * g.kw, KT = (K + DET_BK - 1) / DET_BK;
    const int chunk = (KT + S - 1) / S, kt0 = s * chunk, kt1 = min(KT, kt0 + chunk);
    const DetRoles t = det_roles();
    const bool fast = (g.I % DET_BK) == 0;

    const int m = mt * DET_BN + t.px;
    const bool mvalid = m < M;
    int b = 0, oy = 0, ox = 0;
    if (mvalid) {
        b = m / OHW;
        const int r = m - b * OHW;
        oy = r / g.OW;
        ox = r - oy * g.OW;
    }
    const int iy0 = oy * g.sh - g.ph, ix0 = ox * g.sw - g.pw;
    const long HW = (long)g.H * g.W;
    const float* xb = g.x + ((long)b * g.x_ctot + g.x_coff) * HW;
    const float* wp = g.w + (long)nt * DET_BM + t.wc;

    const f32x16 acc = det_conv_tile(Ws, Xs, kt0, kt1, [&](int kt, float (&xr)[4], float4& wreg) {
        wreg = *reinterpret_cast<const float4*>(wp + (long)(kt * DET_BK + t.wr) * Np);
        const int kb = kt * DET_BK;
        if (fast) {
            const int tap = kb / g.I, c0 = kb - tap * g.I;
            const int ky = tap / g.kw, kx = tap - ky * g.kw;
            const int iy = iy0 + ky, ix = ix0 + kx;
            const bool ok = mvalid && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            const float* p = xb + (long)(c0 + t.kr0) * HW + (long)iy * g.W + ix;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xr[i] = 0.f;
                if (ok) xr[i] = p[(long)i * 4 * HW];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kb + t.kr0 + 4 * i;
                xr[i] = 0.f;
                if (mvalid && k < K) {
                    const int tap = k / g.I, c = k - tap * g.I;
                    const int ky = tap / g.kw, kx = tap - ky * g.kw;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) xr[i] = xb[(long)c * HW + (long)iy * g.W + ix];
                }
            }
        }
    });

    const int mo = mt * DET_BN + t.wn + t.lj;
    if (mo >= M) return;
    const int ob = nt * DET_BM + t.wm;
    if (S == 1) {
        const int bo = mo / OHW, pix = mo - bo * OHW;
        float* yb = g.y + ((long)bo * g.y_ctot + g.y_coff) * OHW + pix;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = ob + t.row(r);
            if (o < g.O) yb[(long)o * OHW] = fmaxf(acc[r] + g.bias[o], 0.f);
        }
    } else {
        float* wsb = a.ws + a.ws_off[gi] + (long)s * g.O * M + mo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = ob + t.row(r);
            if (o < g.O) wsb[(long)o * M] = acc[r];
        }
    }
}

// the split groups' partial sums, added in split order, + bias, ReLU, at the channel offset; blockIdx.y = group
__global__ __launch_bounds__(256) void inc_splitk_reduce_kernel(const IncConvArgs a) {
    const shg_inc_conv_desc& g = a.g[blockIdx.y];
    if (g.splitk <= 1) return;
    const int OHW = g.OH * g.OW, M = a.B * OHW;
    const long n = (long)g.O * M;
    const float* ws = a.ws + a.ws_off[blockIdx.y];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const int o = (int)(e / M), m = (int)(e - (long)o * M);
        float v = 0.f;
        for (int s = 0; s < g.splitk; ++s) v += ws[(long)s * n + e];
        const int bo = m / OHW, pix = m - bo * OHW;
        g.y[((long)bo * g.y_ctot + g.y_coff + o) * OHW + pix] = fmaxf(v + g.bias[o], 0.f);
    }
}

static int inc_check_group(const shg_inc_conv_desc& d, int i) {
    SHG_CHECK_ARG(d.x && d.w && d.bias && d.y, "inception_conv: group %d: null pointer", i);
    SHG_CHECK_ARG(((uintptr_t)d.w & 15) == 0, "inception_conv: group %d: packed weight not 16-byte aligned", i);
    SHG_CHECK_ARG(d.kh >= 1 && d.kh <= 7 && d.kw >= 1 && d.kw <= 7 && d.sh >= 1 && d.sh <= 2 && d.sw >= 1 && d.sw <= 2 && d.ph >= 0 &&
                      d.ph < d.kh && d.pw >= 0 && d.pw < d.kw,
                  "inception_conv: group %d: kernel %dx%d stride %dx%d pad %dx%d not supported (kernel <= 7, stride 1 or 2, pad < kernel)", i,
                  d.kh, d.kw, d.sh, d.sw, d.ph, d.pw);
    SHG_CHECK_ARG(d.I >= 1 && d.O >= 1 && d.H >= 1 && d.W >= 1 && d.OH >= 1 && d.OW >= 1 && d.OH == (d.H + 2 * d.ph - d.kh) / d.sh + 1 &&
                      d.OW == (d.W + 2 * d.pw - d.kw) / d.sw + 1 && d.H + 2 * d.ph >= d.kh && d.W + 2 * d.pw >= d.kw,
                  "inception_conv: group %d: bad geometry (I %d O %d, %dx%d -> %dx%d)", i, d.I, d.O, d.H, d.W, d.OH, d.OW);
    SHG_CHECK_ARG(d.x_coff >= 0 && d.x_coff + d.I <= d.x_ctot, "inception_conv: group %d: input channels [%d, %d) exceed the input's %d", i,
                  d.x_coff, d.x_coff + d.I, d.x_ctot);
    SHG_CHECK_ARG(d.y_coff >= 0 && d.y_coff + d.O <= d.y_ctot, "inception_conv: group %d: channel offset %d + O %d exceeds the output's %d channels",
                  i, d.y_coff, d.O, d.y_ctot);
    const int KT = (d.I * d.kh * d.kw + DET_BK - 1) / DET_BK;
    SHG_CHECK_ARG(d.splitk >= 1 && d.splitk <= 16 && (d.splitk - 1) * ((KT + d.splitk - 1) / d.splitk) < KT,
                  "inception_conv: group %d: splitk %d leaves a split without K steps (%d steps)", i, d.splitk, KT);
    return SHG_OK;
}

static long inc_ws_floats(const shg_inc_conv_desc& d, int B) {
    return d.splitk > 1 ? (long)d.splitk * d.O * B * d.OH * d.OW : 0;
}

extern "C" size_t shg_inception_conv_workspace_bytes(const shg_inc_conv_desc* groups, int G, int B) {
    if (!groups || G < 1 || G > SHG_INC_MAX_GROUPS || B < 1) return 0;
    size_t n = 0;
    for (int i = 0; i < G; ++i) n += (size_t)inc_ws_floats(groups[i], B) * sizeof(float);
    return n;
}

extern "C" long shg_inception_packed_weight_elems(int O, int I, int kh, int kw) {
    if (O < 1 || I < 1 || kh < 1 || kw < 1) return -1;
    const long Kp = ((long)I * kh * kw + DET_BK - 1) / DET_BK * DET_BK, Np = ((long)O + DET_BM - 1) / DET_BM * DET_BM;
    return Kp * Np;
}

extern "C" int shg_inception_conv_f32(const shg_inc_conv_desc* groups, int G, int B, void* workspace, size_t ws_bytes, void* stream) {
    SHG_CHECK_ARG(groups && G >= 1 && G <= SHG_INC_MAX_GROUPS && B >= 1, "inception_conv: null descriptors, B < 1 or G outside [1, %d]",
                  SHG_INC_MAX_GROUPS);
    IncConvArgs a;
    a.G = G;
    a.B = B;
    a.first_block[0] = 0;
    long off = 0, blocks = 0;
    bool split = false;
    for (int i = 0; i < G; ++i) {
        const shg_inc_conv_desc& d = groups[i];
        const int rc = inc_check_group(d, i);
        if (rc) return rc;
        SHG_CHECK_ARG((long)B * d.H * d.W * d.x_ctot < (1L << 31) && (long)B * d.OH * d.OW * d.y_ctot < (1L << 31) &&
                          (long)B * d.OH * d.OW * d.O * d.splitk < (1L << 31),
                      "inception_conv: group %d: tensor too large for 32-bit pixel indices", i);
        a.g[i] = d;
        a.ws_off[i] = off;
        off += inc_ws_floats(d, B);
        split |= d.splitk > 1;
        const long mt = ((long)B * d.OH * d.OW + DET_BN - 1) / DET_BN, nt = (d.O + DET_BM - 1) / DET_BM;
        blocks += mt * nt * d.splitk;
        SHG_CHECK_ARG(blocks < (1L << 31), "inception_conv: too many workgroups");
        a.first_block[i + 1] = (int)blocks;
    }
    SHG_CHECK_ARG(!split || workspace, "inception_conv: split-K groups need a workspace");
    SHG_CHECK_ARG((size_t)off * sizeof(float) <= ws_bytes, "inception_conv: workspace of %zu bytes is too small (%zu needed)", ws_bytes,
                  (size_t)off * sizeof(float));
    a.ws = (float*)workspace;
    hipLaunchKernelGGL(inc_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SHG_CHECK_LAUNCH();
    if (split) {
        hipLaunchKernelGGL(inc_splitk_reduce_kernel, dim3(64, G), dim3(256), 0, (hipStream_t)stream, a);
        SHG_CHECK_LAUNCH();
    }
    return SHG_OK;
}

// ---- weight prep: folded w [O][I][kh][kw], b [O] -> wp [Kp][Np] (k = (ky*kw + kx)*I + c; zero outside K x O), bp [Np]
__global__ __launch_bounds__(256) void inc_weight_prep_kernel(const float* w, const float* bias, float* wp, float* bp, int O, int I, int kh, int kw,
                                                              int Kp, int Np) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < Np && bp) bp[e] = e < O ? bias[e] : 0.f;
    if (e >= (long)Kp * Np) return;
    const int k = (int)(e / Np), o = (int)(e - (long)k * Np);
    float v = 0.f;
    if (k < I * kh * kw && o < O) {
        const int tap = k / I, c = k - tap * I;
        const int ky = tap / kw, kx = tap - ky * kw;
        v = w[(((long)o * I + c) * kh + ky) * kw + kx];
    }
    wp[e] = v;
}

int shg_det_weight_prep(const float* w, const float* bias, float* wp, float* bp, int O, int I, int kh, int kw, hipStream_t stream) {
    const long n = shg_inception_packed_weight_elems(O, I, kh, kw);
    const int Kp = (I * kh * kw + DET_BK - 1) / DET_BK * DET_BK, Np = (O + DET_BM - 1) / DET_BM * DET_BM;
    hipLaunchKernelGGL(inc_weight_prep_kernel, dim3(shg_cdiv(n, 256)), dim3(256), 0, stream, w, bias, wp, bp, O, I, kh, kw, Kp, Np);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_inception_weight_prep_f32(const float* w, const float* bias, float* wp, float* bp, int O, int I, int kh, int kw, void* stream) {
    SHG_CHECK_ARG(w && bias && wp && bp, "inception_weight_prep: null pointer");
    SHG_CHECK_ARG(shg_inception_packed_weight_elems(O, I, kh, kw) > 0 && kh <= 7 && kw <= 7, "inception_weight_prep: bad shape O %d I %d %dx%d", O, I,
                  kh, kw);
    return shg_det_weight_prep(w, bias, wp, bp, O, I, kh, kw, (hipStream_t)stream);
}

// ---- front end: value map, TF1 legacy bilinear resize to 299 x 299 (source = i * size / 299, no half-pixel offset, border clamp),
// (v - 128) / 128.  The value of a source sample is lut[u8] (uint8 input) or v*scale + bias rounded twice (float input: the reference's
// `real.float()*127.5 + 127.5`).  Skipped resize when the input is 299 x 299.
__global__ __launch_bounds__(256) void inc_frontend_kernel(const void* x, const float* lut, float scale, float bias, float* y, int B, int H, int W) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long plane = (long)INC_OUT * INC_OUT;
    if (e >= (long)B * 3 * plane) return;
    const long bc = e / plane;
    const int r = (int)(e - bc * plane), oy = r / INC_OUT, ox = r - oy * INC_OUT;
    const long base = bc * (long)H * W;
    float v;
    if (H == INC_OUT && W == INC_OUT) {
        v = det_value(x, lut, scale, bias, base + r);
    } else {
        // source = i * size / 299 as an integer part and a fraction (num % 299) / 299: exact to one rounding of the fraction (a float32
        // coordinate would carry an error of ~1e-4 pixel at 1024); at and beyond the last sample the border clamp leaves fraction 0
        int y0 = oy * H / INC_OUT, x0 = ox * W / INC_OUT;
        float fy = __fdiv_rn((float)(oy * H - y0 * INC_OUT), (float)INC_OUT), fx = __fdiv_rn((float)(ox * W - x0 * INC_OUT), (float)INC_OUT);
        if (y0 >= H - 1) { y0 = H - 1; fy = 0.f; }
        if (x0 >= W - 1) { x0 = W - 1; fx = 0.f; }
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float v00 = det_value(x, lut, scale, bias, base + (long)y0 * W + x0), v01 = det_value(x, lut, scale, bias, base + (long)y0 * W + x1);
        const float v10 = det_value(x, lut, scale, bias, base + (long)y1 * W + x0), v11 = det_value(x, lut, scale, bias, base + (long)y1 * W + x1);
        v = v00 * ((1.f - fx) * (1.f - fy)) + v01 * (fx * (1.f - fy)) + v10 * ((1.f - fx) * fy) + v11 * (fx * fy);
    }
    y[e] = __fmul_rn(__fsub_rn(v, 128.f), 0.0078125f);
}

extern "C" int shg_inception_frontend_f32(const void* x, const float* lut, float scale, float bias, float* y, int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && y, "inception_frontend: null pointer");
    SHG_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (long)B * 3 * H * W < (1L << 40) && H <= 65536 && W <= 65536,
                  "inception_frontend: bad geometry B %d %dx%d", B, H, W);
    const long n = (long)B * 3 * INC_OUT * INC_OUT;
    hipLaunchKernelGGL(inc_frontend_kernel, dim3(shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, lut, scale, bias, y, B, H, W);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- 3 x 3 pools: mode 0 max, 1 average over the in-bounds taps (count_include_pad=False); output at a channel offset
__global__ __launch_bounds__(256) void inc_pool_kernel(const float* x, float* y, int B, int C, int H, int W, int mode, int stride, int pad, int OH,
                                                       int OW, int y_ctot, int y_coff) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long OHW = (long)OH * OW;
    if (e >= (long)B * C * OHW) return;
    const long bc = e / OHW;
    const int r = (int)(e - bc * OHW), oy = r / OW, ox = r - oy * OW;
    const int b = (int)(bc / C), c = (int)(bc - (long)b * C);
    const float* p = x + bc * (long)H * W;
    float acc = mode == 0 ? -__builtin_inff() : 0.f;
    int cnt = 0;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * stride - pad + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * stride - pad + dx;
            if (ix < 0 || ix >= W) continue;
            const float v = p[(long)iy * W + ix];
            acc = mode == 0 ? fmaxf(acc, v) : acc + v;
            ++cnt;
        }
    }
    if (mode == 1) acc = acc / (float)cnt;
    y[((long)b * y_ctot + y_coff + c) * OHW + r] = acc;
}

extern "C" int shg_inception_pool_f32(const float* x, float* y, int B, int C, int H, int W, int mode, int stride, int pad, int y_ctot, int y_coff,
                                      void* stream) {
    SHG_CHECK_ARG(x && y, "inception_pool: null pointer");
    SHG_CHECK_ARG((mode == 0 || mode == 1) && (stride == 1 || stride == 2) && (pad == 0 || pad == 1), "inception_pool: mode %d stride %d pad %d not supported",
                  mode, stride, pad);
    SHG_CHECK_ARG(B >= 1 && C >= 1 && H + 2 * pad >= 3 && W + 2 * pad >= 3, "inception_pool: bad geometry");
    SHG_CHECK_ARG(y_coff >= 0 && y_coff + C <= y_ctot, "inception_pool: channel offset %d + C %d exceeds the output's %d channels", y_coff, C, y_ctot);
    const int OH = (H + 2 * pad - 3) / stride + 1, OW = (W + 2 * pad - 3) / stride + 1;
    const long n = (long)B * C * OH * OW;
    SHG_CHECK_ARG((long)B * y_ctot * OH * OW < (1L << 40), "inception_pool: too large");
    hipLaunchKernelGGL(inc_pool_kernel, dim3(shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, B, C, H, W, mode, stride, pad, OH, OW, y_ctot,
                       y_coff);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- global mean over H*W: one wave per (b, c), lane-strided sums then a fixed butterfly (same bits whatever the batch)
__global__ __launch_bounds__(256) void inc_mean_kernel(const float* x, float* y, long BC, int HW) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= BC) return;
    const float* p = x + row * HW;
    float s = 0.f;
    for (int i = lane; i < HW; i += 64) s += p[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) y[row] = s / (float)HW;
}

extern "C" int shg_inception_mean_f32(const float* x, float* y, int B, int C, int HW, void* stream) {
    SHG_CHECK_ARG(x && y, "inception_mean: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && HW >= 1, "inception_mean: bad geometry");
    const long BC = (long)B * C;
    hipLaunchKernelGGL(inc_mean_kernel, dim3(shg_cdiv(BC, 4)), dim3(256), 0, (hipStream_t)stream, x, y, BC, HW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- classifier head (the detector's softmax output, return_features=False): probs [B, C] = softmax(feats [B, D] . w [C, D]^T (+ bias)).
// One workgroup per image and one launch: the feature row sits in LDS, the waves stride over the classes (lane-strided float4
// products in four fp32 FMA chains, then a fixed butterfly), the logits stay in LDS, max and sum go through LDS, and the row is
// normalised on the way out.  B * C * D is far too small for matrix cores to matter; an image's row is the same bits in any batch.
#define INC_HEAD_THREADS 512
__device__ __forceinline__ float inc_head_block_reduce(float v, float* red, bool is_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    __syncthreads();                                   // red may still be read from the previous reduction
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < INC_HEAD_THREADS / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

__global__ __launch_bounds__(INC_HEAD_THREADS) void inc_head_kernel(const float* feats, const float* w, const float* bias, float* probs, int C, int D) {
    extern __shared__ float inc_head_lds[];
    float* sf = inc_head_lds;                          // [D] the image's pooled features
    float* sl = inc_head_lds + D;                      // [C] logits, then exp(logit - max)
    __shared__ float red[INC_HEAD_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    for (int k = tid * 4; k < D; k += INC_HEAD_THREADS * 4)
        *reinterpret_cast<float4*>(sf + k) = *reinterpret_cast<const float4*>(feats + (long)b * D + k);
    __syncthreads();
    for (int c = wave; c < C; c += INC_HEAD_THREADS / 64) {
        const float* wr = w + (long)c * D;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int k = lane * 4; k < D; k += 256) {
            const float4 x = *reinterpret_cast<const float4*>(sf + k), y = *reinterpret_cast<const float4*>(wr + k);
            a0 = fmaf(x.x, y.x, a0);
            a1 = fmaf(x.y, y.y, a1);
            a2 = fmaf(x.z, y.z, a2);
            a3 = fmaf(x.w, y.w, a3);
        }
        float a = (a0 + a1) + (a2 + a3);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) sl[c] = bias ? a + bias[c] : a;
    }
    __syncthreads();
    float mx = -__builtin_inff();
    for (int c = tid; c < C; c += INC_HEAD_THREADS) mx = fmaxf(mx, sl[c]);
    mx = inc_head_block_reduce(mx, red, true);
    float sum = 0.f;
    for (int c = tid; c < C; c += INC_HEAD_THREADS) {
        const float e = expf(sl[c] - mx);
        sl[c] = e;                                     // (each thread rereads only what it wrote)
        sum += e;
    }
    sum = inc_head_block_reduce(sum, red, false);
    for (int c = tid; c < C; c += INC_HEAD_THREADS) probs[(long)b * C + c] = sl[c] / sum;
}

// feats [B, D] float32 (D a multiple of 4), w [C, D], bias [C] or NULL (no_output_bias), probs [B, C]; 4 (C + D) + 32 bytes of LDS (the
// two arrays and the reduction scratch) <= 64 KiB.
extern "C" int shg_inception_head_f32(const float* feats, const float* w, const float* bias, float* probs, int B, int C, int D, void* stream) {
    SHG_CHECK_ARG(feats && w && probs, "inception_head: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && D >= 4 && D % 4 == 0, "inception_head: need B, C >= 1 and D a positive multiple of 4");
    SHG_CHECK_ARG(4L * ((long)C + D) + 32 <= 65536, "inception_head: 4 (C + D) + 32 = %ld bytes do not fit 64 KiB of LDS", 4L * ((long)C + D) + 32);
    SHG_CHECK_ARG(((uintptr_t)feats | (uintptr_t)w) % 16 == 0, "inception_head: feats and w must be 16-byte aligned");
    hipLaunchKernelGGL(inc_head_kernel, dim3(B), dim3(INC_HEAD_THREADS), (size_t)(C + D) * 4, (hipStream_t)stream, feats, w, bias, probs, C, D);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
