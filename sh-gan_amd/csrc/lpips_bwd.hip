// LPIPS as a training loss: the backward pass of the frozen network with respect to the pred image (sh-gan_amd/lpips.py: Lpips.loss drives
// this file), the two forward pieces whose operand is a [-1, 1] float image, and the per-image L1 mean with its gradient.
//
// ONE masking rule: whoever writes a gradient into the buffer of a post-ReLU activation y masks it by y > 0 itself, with a select (never a
// multiply: a NaN or inf formed at a dead position must not reach memory).  Masking distributes over the sum, so a tap's buffer is written
// by its downstream consumer (dgrad or pool backward) and then accumulated into by the head: no join pass, every activation gradient is
// written once (or written and accumulated once at a tap) and read once.  No atomics, no host synchronisation, every sum in a fixed order:
// the same inputs give the same bits on every run.
//
// shg_lpips_dgrad_f32: input gradient of a stride-1 convolution = the forward convolution of g with w.transpose(0,1).flip(2,3) at the same
//   padding, on the detector's implicit-GEMM tile (det_conv_tile.h, exact-fp32 MFMA, K never split) with its own epilogue: no bias, no
//   ReLU, the output selected by ymask > 0 read at the output position (ymask NULL: stored as it is -- the gradient of a pooled tensor or
//   of the image).
// shg_lpips_maxpool_bwd_f32: gather form of the k x k / stride 2 / floor max pool (k = 2: VGG16, k = 3: AlexNet, overlapping).  Each input
//   element sums (windows in row-major order) the gradients of the windows whose FIRST maximum in row-major order it is (torch's CPU
//   rule); rows / columns outside every window get 0; the y > 0 select is fused (the pool's input is a post-ReLU activation).
// shg_lpips_head_bwd_f32: the distance head of one tap.  Per position s = sqrt(sum f^2), a = 1 / (s + 1e-10), n = a f,
//   q_c = 2 w_c (n_c - n^real_c) g_b / (h w), df_c = a q_c - f_c a^2 (sum_j q_j f_j) / s, selected by f_c > 0, stored or accumulated.
//   A position whose tap vector is all zero has every channel masked: exactly 0.
// shg_lpips_conv1_pm1_f32 / shg_lpips_scale_pm1_f32: conv1 of AlexNet (lpips.hip's kernel) / the scaling layer as a pass of its own for a
//   float32 image v in [-1, 1] that enters the scaling layer as it is: (v - shift_c) * float32(1 / scale_c).
// shg_lpips_conv1_dgrad_f32: the transposed 11 x 11 / stride 4 / pad 2 convolution, 64 -> 3 channels (plain VALU: three outputs per
//   pixel); the caller folds 1 / scale_c into the weights.  Pixels no window reaches get 0.
// shg_l1_mean_f32 / shg_l1_mean_bwd_f32: out[b] = mean |a - b| of image b (float64, fixed order, rounded once); dx = sign(a - b) g_b / n.
#include "det_conv_tile.h"
#include "../../include/shgan_hip.h"

#define LPB_K1 363                      // 3 * 11 * 11
#define LPB_KT1 ((LPB_K1 + DET_BK - 1) / DET_BK)
#define LPB_L1_THREADS 1024

namespace {

struct LpbScale { float shift[3], inv[3]; };     // scaling layer: (v - shift) * inv

int lpb_scale_make(const float* shift, const float* scaling, const char* who, LpbScale* s) {
    SHG_CHECK_ARG(scaling[0] != 0.f && scaling[1] != 0.f && scaling[2] != 0.f, "%s: a scaling-layer scale of 0", who);
    for (int c = 0; c < 3; ++c) {
        s->shift[c] = shift[c];
        s->inv[c] = (float)(1.0 / (double)scaling[c]);
    }
    return SHG_OK;
}

__device__ __forceinline__ float lpb_scaled(float v, const LpbScale& s, int c) {
    const float sh = c == 0 ? s.shift[0] : (c == 1 ? s.shift[1] : s.shift[2]);
    const float iv = c == 0 ? s.inv[0] : (c == 1 ? s.inv[1] : s.inv[2]);
    return __fmul_rn(__fsub_rn(v, sh), iv);
}

// ---- masked dgrad on the detector's tile: rows = the O output channels (the forward convolution's inputs), columns = pixels, K = I k k
// (I = the forward convolution's outputs) in tap-major order, the geometry walk of inception.hip's kernel at stride 1.
struct LpbDgradArgs {
    const float* g;          // [B][I][H][W]
    const float* w;          // packed [Kp][Np]
    const float* ymask;      // [B][O][H][W] or NULL
    float* dx;               // [B][O][H][W]
    int B, I, O, H, W, k, p;
};

template <bool MASK>
__global__ __launch_bounds__(256) void lpb_dgrad_kernel(const LpbDgradArgs a) {
    __shared__ float Ws[2][DET_BK][DET_BM];
    __shared__ float Xs[2][DET_BK][DET_BN];
    const int NT = (a.O + DET_BM - 1) / DET_BM, Np = NT * DET_BM;
    const int nt = (int)blockIdx.x % NT, mt = (int)blockIdx.x / NT;
    const int HW = a.H * a.W, M = a.B * HW;
    const int K = a.I * a.k * a.k, KT = (K + DET_BK - 1) / DET_BK;
    const DetRoles t = det_roles();
    const bool fast = (a.I % DET_BK) == 0;

    const int m = mt * DET_BN + t.px;
    const bool mvalid = m < M;
    int b = 0, oy = 0, ox = 0;
    if (mvalid) {
        b = m / HW;
        const int r = m - b * HW;
        oy = r / a.W;
        ox = r - oy * a.W;
    }
    const int iy0 = oy - a.p, ix0 = ox - a.p;
    const float* gb = a.g + (long)b * a.I * HW;
    const float* wp = a.w + (long)nt * DET_BM + t.wc;

    const f32x16 acc = det_conv_tile(Ws, Xs, 0, KT, [&](int kt, float (&xr)[4], float4& wreg) {
        wreg = *reinterpret_cast<const float4*>(wp + (long)(kt * DET_BK + t.wr) * Np);
        const int kb = kt * DET_BK;
        if (fast) {
            const int tap = kb / a.I, c0 = kb - tap * a.I;
            const int ky = tap / a.k, kx = tap - ky * a.k;
            const int iy = iy0 + ky, ix = ix0 + kx;
            const bool ok = mvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const float* p = gb + (long)(c0 + t.kr0) * HW + (long)iy * a.W + ix;
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
                    const int tap = k / a.I, c = k - tap * a.I;
                    const int ky = tap / a.k, kx = tap - ky * a.k;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) xr[i] = gb[(long)c * HW + (long)iy * a.W + ix];
                }
            }
        }
    });

    const int mo = mt * DET_BN + t.wn + t.lj;
    if (mo >= M) return;
    const int ob = nt * DET_BM + t.wm;
    const int bo = mo / HW, pix = mo - bo * HW;
    const long base = (long)bo * a.O * HW + pix;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = ob + t.row(r);
        if (o < a.O) {
            const long e = base + (long)o * HW;
            float v = acc[r];
            if (MASK) v = a.ymask[e] > 0.f ? v : 0.f;
            a.dx[e] = v;
        }
    }
}

// ---- max-pool backward, gather form: one thread per INPUT element
template <int KS>
__global__ __launch_bounds__(256) void lpb_maxpool_bwd_kernel(const float* x, const float* gy, float* dx, long BC, int H, int W, int OH, int OW) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW = (long)H * W;
    if (e >= BC * HW) return;
    const float v = x[e];
    float sum = 0.f;
    if (v > 0.f) {                                               // a masked element needs no window
        const long bc = e / HW;
        const int r = (int)(e - bc * HW), iy = r / W, ix = r - iy * W;
        const float* xp = x + bc * HW;
        const float* gp = gy + bc * (long)OH * OW;
        // windows (oy, ox) with 2 oy <= iy <= 2 oy + KS - 1
        const int oy0 = max(0, (iy - KS + 2) >> 1), oy1 = min(OH - 1, iy >> 1);
        const int ox0 = max(0, (ix - KS + 2) >> 1), ox1 = min(OW - 1, ix >> 1);
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                // the window's first maximum in row-major order: an earlier element beats this one with >=, a later one with >
                bool mine = true;
#pragma unroll
                for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                    for (int dxx = 0; dxx < KS; ++dxx) {
                        const int yy = 2 * oy + dy, xx = 2 * ox + dxx;
                        const float u = xp[(long)yy * W + xx];
                        const bool before = yy < iy || (yy == iy && xx < ix);
                        if (yy != iy || xx != ix) mine = mine && (before ? u < v : u <= v);
                    }
                if (mine) sum += gp[(long)oy * OW + ox];
            }
    }
    dx[e] = sum;
}

// ---- distance-head backward: one lane per position, the channel sums float32 FMA chains in channel order (as the forward head's)
__global__ __launch_bounds__(64) void lpb_head_bwd_kernel(const float* f, const float* fr, const float* w, const float* g, float* df, int C, int HW,
                                                          float inv_hw, int accumulate) {
    const int pix = (int)blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (pix >= HW) return;
    const float* p = f + (long)b * C * HW + pix;
    const float* q = fr + (long)b * C * HW + pix;
    float* d = df + (long)b * C * HW + pix;
    float sp = 0.f, sr = 0.f;
    for (int c = 0; c < C; ++c) {
        const float u = p[(long)c * HW], v = q[(long)c * HW];
        sp = fmaf(u, u, sp);
        sr = fmaf(v, v, sr);
    }
    const float s = sqrtf(sp);
    const float a = 1.f / (s + 1e-10f), ar = 1.f / (sqrtf(sr) + 1e-10f);
    const float coef = 2.f * g[b] * inv_hw;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
        const float u = p[(long)c * HW];
        const float qc = coef * w[c] * (a * u - ar * q[(long)c * HW]);
        dot = fmaf(qc, u, dot);
    }
    const float t = s > 0.f ? a * a * dot / s : 0.f;              // s = 0: every channel is masked below
    for (int c = 0; c < C; ++c) {
        const float u = p[(long)c * HW];
        const float qc = coef * w[c] * (a * u - ar * q[(long)c * HW]);
        const float v = u > 0.f ? a * qc - u * t : 0.f;
        d[(long)c * HW] = accumulate ? d[(long)c * HW] + v : v;
    }
}

// ---- conv1 of AlexNet for a [-1, 1] float image (lpips.hip's lp_conv1_kernel with the plain operand)
struct LpbConv1Args {
    const float* x;
    LpbScale s;
    const float* wp;
    const float* bp;
    float* y;
    int B, H, W, OH, OW;
};

__global__ __launch_bounds__(256) void lpb_conv1_pm1_kernel(const LpbConv1Args a) {
    __shared__ float Ws[2][DET_BK][DET_BM];
    __shared__ float Xs[2][DET_BK][DET_BN];
    const DetRoles t = det_roles();
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
    const float* xb = a.x + (long)b * 3 * HW;
    const float* wp = a.wp + t.wc;

    const f32x16 acc = det_conv_tile(Ws, Xs, 0, LPB_KT1, [&](int kt, float (&xr)[4], float4& wreg) {
        wreg = *reinterpret_cast<const float4*>(wp + (long)(kt * DET_BK + t.wr) * DET_BM);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kt * DET_BK + t.kr0 + 4 * i;
            xr[i] = 0.f;
            if (mvalid && k < LPB_K1) {
                const int tap = k / 3, c = k - tap * 3;
                const int ky = tap / 11, kx = tap - ky * 11;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) xr[i] = lpb_scaled(xb[(long)c * HW + (long)iy * a.W + ix], a.s, c);
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

__global__ __launch_bounds__(256) void lpb_scale_pm1_kernel(const float* x, LpbScale k, float* y, long n, long HW) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    y[e] = lpb_scaled(x[e], k, (int)((e / HW) % 3));
}

// ---- conv1 dgrad: g [B][64][OH][OW], w [64][3][11][11] (1 / scale_c folded in) -> dx [B][3][H][W]; one thread per pixel, taps (ky, kx)
// ascending, channels ascending inside a tap
__global__ __launch_bounds__(256) void lpb_conv1_dgrad_kernel(const float* g, const float* w, float* dx, int B, int H, int W, int OH, int OW) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW = (long)H * W;
    if (e >= (long)B * HW) return;
    const int b = (int)(e / HW), r = (int)(e - (long)b * HW), iy = r / W, ix = r - iy * W;
    const long OHW = (long)OH * OW;
    const float* gb = g + (long)b * DET_BM * OHW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    // oy * 4 - 2 + ky = iy: ky = iy + 2 - 4 oy in [0, 10]
    for (int ky = (iy + 2) & 3; ky < 11; ky += 4) {
        const int oy = (iy + 2 - ky) >> 2;
        if (oy < 0 || oy >= OH) continue;
        for (int kx = (ix + 2) & 3; kx < 11; kx += 4) {
            const int ox = (ix + 2 - kx) >> 2;
            if (ox < 0 || ox >= OW) continue;
            const float* gp = gb + (long)oy * OW + ox;
            const float* wq = w + ky * 11 + kx;
            for (int o = 0; o < DET_BM; ++o) {
                const float gv = gp[(long)o * OHW];
                a0 = fmaf(gv, wq[(o * 3 + 0) * 121], a0);
                a1 = fmaf(gv, wq[(o * 3 + 1) * 121], a1);
                a2 = fmaf(gv, wq[(o * 3 + 2) * 121], a2);
            }
        }
    }
    float* d = dx + (long)b * 3 * HW + r;
    d[0] = a0;
    d[HW] = a1;
    d[2 * HW] = a2;
}

// ---- L1: one workgroup per image, thread-strided float64 sums, then a fixed tree
__global__ __launch_bounds__(LPB_L1_THREADS) void lpb_l1_mean_kernel(const float* a, const float* b, float* out, long n) {
    __shared__ double red[LPB_L1_THREADS];
    const int t = threadIdx.x;
    const float* pa = a + (long)blockIdx.x * n;
    const float* pb = b + (long)blockIdx.x * n;
    double s = 0.0;
    for (long i = t; i < n; i += LPB_L1_THREADS) s += (double)fabsf(__fsub_rn(pa[i], pb[i]));
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int k = LPB_L1_THREADS / 2; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = (float)(red[0] / (double)n);
}

__global__ __launch_bounds__(256) void lpb_l1_mean_bwd_kernel(const float* a, const float* b, const float* g, float* dx, long n, long total, float inv_n) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float d = __fsub_rn(a[e], b[e]);
    const float gv = g[e / n] * inv_n;
    dx[e] = d > 0.f ? gv : (d < 0.f ? -gv : 0.f);
}

}  // namespace

extern "C" int shg_lpips_dgrad_f32(const float* g, const float* wp, const float* ymask, float* dx, int B, int I, int O, int H, int W, int k, int pad,
                                   void* stream) {
    SHG_CHECK_ARG(g && wp && dx, "lpips_dgrad: null pointer");
    SHG_CHECK_ARG(((uintptr_t)wp & 15) == 0, "lpips_dgrad: packed weight not 16-byte aligned");
    SHG_CHECK_ARG(k >= 1 && k <= 7 && (k & 1) == 1 && pad == k / 2, "lpips_dgrad: kernel %d pad %d not supported (odd kernel <= 7 at 'same' padding)", k,
                  pad);
    SHG_CHECK_ARG(B >= 1 && I >= 1 && O >= 1 && H >= 1 && W >= 1, "lpips_dgrad: bad geometry (B %d I %d O %d, %dx%d)", B, I, O, H, W);
    SHG_CHECK_ARG((long)B * H * W * I < (1L << 31) && (long)B * H * W * O < (1L << 31), "lpips_dgrad: tensor too large for 32-bit pixel indices");
    const long mt = ((long)B * H * W + DET_BN - 1) / DET_BN, nt = (O + DET_BM - 1) / DET_BM;
    SHG_CHECK_ARG(mt * nt < (1L << 31), "lpips_dgrad: too many workgroups");
    LpbDgradArgs a;
    a.g = g; a.w = wp; a.ymask = ymask; a.dx = dx;
    a.B = B; a.I = I; a.O = O; a.H = H; a.W = W; a.k = k; a.p = pad;
    const dim3 grid((unsigned)(mt * nt));
    if (ymask) hipLaunchKernelGGL((lpb_dgrad_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lpb_dgrad_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_lpips_maxpool_bwd_f32(const float* x, const float* gy, float* dx, int B, int C, int H, int W, int k, void* stream) {
    SHG_CHECK_ARG(x && gy && dx, "lpips_maxpool_bwd: null pointer");
    SHG_CHECK_ARG(k == 2 || k == 3, "lpips_maxpool_bwd: window %d not supported (2 or 3, stride 2)", k);
    SHG_CHECK_ARG(B >= 1 && C >= 1 && H >= k && W >= k && (long)B * C * H * W < (1L << 38), "lpips_maxpool_bwd: bad geometry B %d C %d %dx%d", B, C, H,
                  W);
    const int OH = (H - k) / 2 + 1, OW = (W - k) / 2 + 1;
    const long BC = (long)B * C, n = BC * H * W;
    const dim3 grid((unsigned)shg_cdiv(n, 256));
    if (k == 2) hipLaunchKernelGGL((lpb_maxpool_bwd_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, x, gy, dx, BC, H, W, OH, OW);
    else hipLaunchKernelGGL((lpb_maxpool_bwd_kernel<3>), grid, dim3(256), 0, (hipStream_t)stream, x, gy, dx, BC, H, W, OH, OW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_lpips_head_bwd_f32(const float* f, const float* fr, const float* w, const float* g, float* df, int B, int C, int h, int wd,
                                      int accumulate, void* stream) {
    SHG_CHECK_ARG(f && fr && w && g && df, "lpips_head_bwd: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && h >= 1 && wd >= 1, "lpips_head_bwd: B, C, h, w must be >= 1");
    const long HW = (long)h * wd, tiles = (HW + 63) / 64;
    SHG_CHECK_ARG(HW < (1L << 31) && B <= 65535, "lpips_head_bwd: feature map or batch too large");
    hipLaunchKernelGGL(lpb_head_bwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(64), 0, (hipStream_t)stream, f, fr, w, g, df, C, (int)HW,
                       (float)(1.0 / (double)HW), accumulate ? 1 : 0);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_lpips_conv1_pm1_f32(const float* x, const float* shift, const float* scaling, const float* wp, const float* bp, float* y, int B, int H,
                                       int W, void* stream) {
    SHG_CHECK_ARG(x && shift && scaling && wp && bp && y, "lpips_conv1_pm1: null pointer");
    SHG_CHECK_ARG(((uintptr_t)wp & 15) == 0, "lpips_conv1_pm1: packed weight not 16-byte aligned");
    SHG_CHECK_ARG(B >= 1 && H >= 7 && W >= 7 && H <= 65536 && W <= 65536, "lpips_conv1_pm1: bad geometry B %d %dx%d (B >= 1, H and W >= 7)", B, H, W);
    LpbConv1Args a;
    const int rc = lpb_scale_make(shift, scaling, "lpips_conv1_pm1", &a.s);
    if (rc) return rc;
    a.x = x; a.wp = wp; a.bp = bp; a.y = y;
    a.B = B; a.H = H; a.W = W;
    a.OH = (H + 4 - 11) / 4 + 1;
    a.OW = (W + 4 - 11) / 4 + 1;
    const long M = (long)B * a.OH * a.OW;
    SHG_CHECK_ARG(M * DET_BM < (1L << 31), "lpips_conv1_pm1: tensor too large for 32-bit pixel indices");
    hipLaunchKernelGGL(lpb_conv1_pm1_kernel, dim3((unsigned)((M + DET_BN - 1) / DET_BN)), dim3(256), 0, (hipStream_t)stream, a);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_lpips_scale_pm1_f32(const float* x, const float* shift, const float* scaling, float* y, int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(x && shift && scaling && y, "lpips_scale_pm1: null pointer");
    SHG_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && (long)B * 3 * H * W < (1L << 38), "lpips_scale_pm1: bad geometry B %d %dx%d", B,
                  H, W);
    LpbScale k;
    const int rc = lpb_scale_make(shift, scaling, "lpips_scale_pm1", &k);
    if (rc) return rc;
    const long HW = (long)H * W, n = (long)B * 3 * HW;
    hipLaunchKernelGGL(lpb_scale_pm1_kernel, dim3((unsigned)shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, k, y, n, HW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_lpips_conv1_dgrad_f32(const float* g, const float* w, float* dx, int B, int H, int W, void* stream) {
    SHG_CHECK_ARG(g && w && dx, "lpips_conv1_dgrad: null pointer");
    SHG_CHECK_ARG(B >= 1 && H >= 7 && W >= 7 && H <= 65536 && W <= 65536 && (long)B * H * W < (1L << 36),
                  "lpips_conv1_dgrad: bad geometry B %d %dx%d (B >= 1, H and W >= 7)", B, H, W);
    const int OH = (H + 4 - 11) / 4 + 1, OW = (W + 4 - 11) / 4 + 1;
    const long n = (long)B * H * W;
    hipLaunchKernelGGL(lpb_conv1_dgrad_kernel, dim3((unsigned)shg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g, w, dx, B, H, W, OH, OW);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_l1_mean_f32(const float* a, const float* b, float* out, int B, long n, void* stream) {
    SHG_CHECK_ARG(a && b && out, "l1_mean: null pointer");
    SHG_CHECK_ARG(B >= 1 && n >= 1 && (long)B * n < (1L << 40), "l1_mean: need B >= 1 images of n >= 1 elements (got %d x %ld)", B, n);
    hipLaunchKernelGGL(lpb_l1_mean_kernel, dim3((unsigned)B), dim3(LPB_L1_THREADS), 0, (hipStream_t)stream, a, b, out, n);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_l1_mean_bwd_f32(const float* a, const float* b, const float* g, float* dx, int B, long n, void* stream) {
    SHG_CHECK_ARG(a && b && g && dx, "l1_mean_bwd: null pointer");
    SHG_CHECK_ARG(B >= 1 && n >= 1 && (long)B * n < (1L << 38), "l1_mean_bwd: need B >= 1 images of n >= 1 elements (got %d x %ld)", B, n);
    const long total = (long)B * n;
    hipLaunchKernelGGL(lpb_l1_mean_bwd_kernel, dim3((unsigned)shg_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, b, g, dx, n, total,
                       (float)(1.0 / (double)n));
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
