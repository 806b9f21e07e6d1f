// What a training run keeps beside the G / D step (sh-gan_amd/training_stats.py, optim.py, train_stage.py drive it):
//   shg_stats_moments_f64   count / sum / sum of squares / non-finite count of many small float32 tensors, one launch, float64
//   shg_health_reduce_f64   the per-chunk rows of shg_adam_buckets_health_f32 (csrc/optim.hip) folded per segment and over the optimiser
//   shg_image_grid_u8       the sample grid of draw_functor.output (lib/experiments/stylegan_default.py:74-84), optionally of the
//                           composite real * mask + x * (1 - mask) (shgan_default.py:107)
// What they replace: `training_stats.report` (a host-side list of moments per name and a torch reduction per report), nothing (the reference
// keeps no gradient health), and numpy on a host copy of every sample.
//
// Reduction shapes are fixed by the data alone: within a row / a segment lane-strided partial sums in index order, a xor tree over the 64
// lanes of a wave, then ((w0 + w1) + (w2 + w3)) over the four waves in LDS.  Nothing depends on the grid, nothing is an atomic: the same
// inputs give the same bits on every run.  Every loop is bounded by a launch argument or a table entry; the tables hold raw addresses, are
// built and range-checked on the host (training_stats.validate_stats_table, optim.validate_adam_table) and trusted here.
#include "shg_common.h"
#include <math.h>

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int STATS_ROW = 4;                                 // training_stats.py STATS_ROW: {address, numel, slot, 0}
constexpr int STATS_COLS = 4;                                // {count, sum, sum of squares, non-finite count}
constexpr int ADAM_ROW = 10;                                 // csrc/optim.hip
constexpr int HEALTH_COLS = 5;                               // {sum g^2, replaced, max |g|, sum p^2, sum dp^2}

#define TS_GLOBAL __attribute__((address_space(1)))
typedef TS_GLOBAL const float gcfloat;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// One workgroup per slot; the rows of the slot in table order.
__global__ __launch_bounds__(TS_THREADS) void stats_moments_kernel(const long* __restrict__ tab, int rows, double* __restrict__ acc) {
    __shared__ double part[TS_WAVES][STATS_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = blockIdx.x;
    double tot[STATS_COLS] = {0.0, 0.0, 0.0, 0.0};
    bool any = false;
    for (int r = 0; r < rows; ++r) {
        const long* row = tab + (long)r * STATS_ROW;
        if (row[2] != slot) continue;                    // (uniform over the workgroup)
        any = true;
        gcfloat* x = (gcfloat*)row[0];
        const long n = row[1];
        double cnt = 0.0, s = 0.0, ss = 0.0, bad = 0.0;
        for (long i = tid; i < n; i += TS_THREADS) {
            const float f = x[i];
            if (fabsf(f) <= 3.402823466e38f) {           // finite (false for NaN)
                const double d = (double)f;
                cnt += 1.0, s += d, ss += d * d;
            } else {
                bad += 1.0;
            }
        }
        cnt = wave_sum(cnt), s = wave_sum(s), ss = wave_sum(ss), bad = wave_sum(bad);
        __syncthreads();                                 // the previous row's partials have been read
        if (lane == 0) part[wave][0] = cnt, part[wave][1] = s, part[wave][2] = ss, part[wave][3] = bad;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < STATS_COLS; ++k) tot[k] += (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
        }
    }
    if (tid == 0 && any) {
#pragma unroll
        for (int k = 0; k < STATS_COLS; ++k) acc[slot * STATS_COLS + k] += tot[k];
    }
}

// largest segment whose first chunk is <= c (csrc/optim.hip opt_find)
__device__ __forceinline__ int seg_find(const long* __restrict__ tab, int nseg, long c) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(long)mid * ADAM_ROW + ADAM_ROW - 1] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Workgroup s < nseg: the chunk rows of segment s.  Workgroup nseg: the chunk rows of every touched segment, the optimiser's total; it
// also counts the step.  Untouched segments are left alone.
__global__ __launch_bounds__(TS_THREADS) void health_reduce_kernel(const long* __restrict__ tab, int nseg, const double* __restrict__ ws,
                                                                   double* __restrict__ health, double* __restrict__ steps) {
    __shared__ double part[TS_WAVES][HEALTH_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const bool total = s == nseg;
    long c0, c1;
    if (total) {
        c0 = 0, c1 = tab[(long)nseg * ADAM_ROW + ADAM_ROW - 1];
    } else {
        if (!tab[(long)s * ADAM_ROW + 5]) return;
        c0 = tab[(long)s * ADAM_ROW + ADAM_ROW - 1], c1 = tab[(long)(s + 1) * ADAM_ROW + ADAM_ROW - 1];
    }
    double a[HEALTH_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool any = !total;
    for (long c = c0 + tid; c < c1; c += TS_THREADS) {
        if (total && !tab[(long)seg_find(tab, nseg, c) * ADAM_ROW + 5]) continue;
        const double* w = ws + c * HEALTH_COLS;
        a[0] += w[0], a[1] += w[1], a[2] = fmax(a[2], w[2]), a[3] += w[3], a[4] += w[4];
    }
    if (total) {                                         // a step without any touched segment is no step
        for (int i = 0; i < nseg; ++i) any = any || tab[(long)i * ADAM_ROW + 5] != 0;
    }
#pragma unroll
    for (int k = 0; k < HEALTH_COLS; ++k) a[k] = k == 2 ? wave_max(a[k]) : wave_sum(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < HEALTH_COLS; ++k) part[wave][k] = a[k];
    }
    __syncthreads();
    if (tid == 0 && any) {
        double* h = health + (long)s * HEALTH_COLS;
#pragma unroll
        for (int k = 0; k < HEALTH_COLS; ++k) {
            if (k == 2) h[k] = fmax(h[k], fmax(fmax(part[0][k], part[1][k]), fmax(part[2][k], part[3][k])));
            else h[k] += (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
        }
        if (total) steps[0] += 1.0;
    }
}

// One thread per output pixel.  Every float32 operation is rounded on its own: contraction is off in this kernel.
__global__ __launch_bounds__(256) void image_grid_u8_kernel(const float* __restrict__ x, const float* __restrict__ real,
                                                            const float* __restrict__ mask, uint8_t* __restrict__ out, int C, int H, int W,
                                                            int gw, int gh, float lo, float scale) {
#pragma clang fp contract(off)
    const long OW = (long)gw * W, total = (long)gh * H * OW;
    const long plane = (long)H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long oy = i / OW, ox = i - oy * OW;
        const int gy = (int)(oy / H), y = (int)(oy - (long)gy * H), gx = (int)(ox / W), xx = (int)(ox - (long)gx * W);
        const long n = (long)gy * gw + gx, pix = (long)y * W + xx;
        const float m = mask ? mask[n * plane + pix] : 0.f;
        for (int c = 0; c < C; ++c) {
            float v = x[(n * C + c) * plane + pix];
            if (mask) v = __fadd_rn(__fmul_rn(real[(n * C + c) * plane + pix], m), __fmul_rn(v, __fsub_rn(1.f, m)));
            v = rintf(__fmul_rn(__fsub_rn(v, lo), scale));               // ties to even
            v = fminf(fmaxf(v, 0.f), 255.f);                             // NaN -> 0
            out[i * C + c] = (uint8_t)v;
        }
    }
}

}  // namespace

extern "C" int shg_stats_moments_f64(const long* table, int rows, double* acc, int slots, void* stream) {
    SHG_CHECK_ARG(rows >= 0 && rows <= (1 << 16), "stats_moments_f64: rows must lie in [0, 65536] (got %d)", rows);
    SHG_CHECK_ARG(slots >= 1 && slots <= (1 << 16), "stats_moments_f64: slots must lie in [1, 65536] (got %d)", slots);
    if (rows == 0) return SHG_OK;
    SHG_CHECK_ARG(table && acc, "stats_moments_f64: null pointer");
    hipLaunchKernelGGL(stats_moments_kernel, dim3(slots), dim3(TS_THREADS), 0, (hipStream_t)stream, table, rows, acc);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_health_reduce_f64(const long* table, int nseg, long chunks, const double* workspace, double* health, double* steps,
                                     void* stream) {
    SHG_CHECK_ARG(table && workspace && health && steps, "health_reduce_f64: null pointer");
    SHG_CHECK_ARG(nseg >= 1 && nseg <= (1 << 20), "health_reduce_f64: nseg must lie in [1, 2^20] (got %d)", nseg);
    SHG_CHECK_ARG(chunks >= nseg && chunks <= (1L << 40), "health_reduce_f64: chunks must lie in [nseg, 2^40] (every segment has one)");
    hipLaunchKernelGGL(health_reduce_kernel, dim3(nseg + 1), dim3(TS_THREADS), 0, (hipStream_t)stream, table, nseg, workspace, health, steps);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_image_grid_u8(const float* x, const float* real, const float* mask, uint8_t* out, int C, int H, int W, int gw, int gh,
                                 float lo, float scale, void* stream) {
    SHG_CHECK_ARG(x && out, "image_grid_u8: null pointer");
    SHG_CHECK_ARG((real == nullptr) == (mask == nullptr), "image_grid_u8: real and mask go together");
    SHG_CHECK_ARG(C == 1 || C == 3, "image_grid_u8: C is 1 or 3 (got %d)", C);
    SHG_CHECK_ARG(H >= 1 && W >= 1 && gw >= 1 && gh >= 1 && H <= 65536 && W <= 65536 && gw <= 4096 && gh <= 4096,
                  "image_grid_u8: H, W in [1, 65536], gw, gh in [1, 4096]");
    SHG_CHECK_ARG((long)gw * gh * C * H * W < (1L << 40), "image_grid_u8: the grid is too large");
    SHG_CHECK_ARG(scale == scale && lo == lo && fabsf(scale) <= 3.402823466e38f && fabsf(lo) <= 3.402823466e38f,
                  "image_grid_u8: lo and scale must be finite");
    const long total = (long)gh * H * gw * W;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(image_grid_u8_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, x, real,
                       mask, out, C, H, W, gw, gh, lo, scale);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
