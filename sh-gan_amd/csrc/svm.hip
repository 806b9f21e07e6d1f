// The streaming pass of the linear SVM behind U-IDS / P-IDS (CoModGAN's inception discriminative scores; sh-gan_amd/ids_score.py
// drives this file).  The fit minimises f(w, b) = (|w|^2 + b^2) / 2 + C sum_i max(0, 1 - y_i (w.x_i + b))^2 over 2 x 50 000 rows of 2048
// float32 detector features by a truncated Newton method; the gradient and every Hessian-vector product are ONE pass of the form
//
//     q = X~^T phi(X~ v),   X~ = [X, 1] (the intercept is a feature of value 1),  v, q in R^(D+1), float64
//
// over the rows of up to two row sets (reals and fakes stay two tensors).  A row is read once, converted to float64 in registers,
// dotted with v (t_i), turned into the per-row scalar s_i = phi(t_i), and added as s_i x~_i into a float64 partial of q that lives in
// the registers of the wave for the whole launch:
//
//     grad  (mode 0)  z_i = t_i and a_i = [1 - y_i t_i > 0] are written, loss += a_i (1 - y_i t_i)^2,  s_i = -2 C y_i a_i (1 - y_i t_i)
//     hv    (mode 1)  a_i is read,  s_i = 2 C a_i t_i,  z_i = t_i is written when z is given (the line search wants X~ s)
//
// The caller adds the regulariser's v.  Geometry: one wave per row, lane l owns the columns (64 c + l) 4 .. + 3 of every 256-column
// chunk c (a wave's load instruction covers 1 KB of the row: 16-byte loads when D, the row pitch and the base allow, else dword
// loads), so q costs 8 ceil(D / 256) VGPRs per lane and v sits in LDS in the lanes' order (ds_read_b128 at consecutive lanes).  The
// row after the current one is in flight while the current one is reduced.  Wave g of the grid walks the rows g, g + G, g + 2G, ...
// of the concatenated sets: at any time the grid streams one contiguous window of X.  The grid is a function of (n, D) alone, every
// workgroup adds its four waves' partials in wave order and writes D + 2 doubles (q, the intercept's entry, the loss) to the
// workspace, and a second launch adds the workgroups' partials in a fixed order: no atomics, the same bits on every run.  The
// arithmetic (two float64 FMAs and a conversion per element, half rate) is about a sixth of the time the HBM read of the row takes.
#include "shg_common.h"

#define SVM_MAX_D 4096
#define SVM_WG 256

static inline int svm_chunks(int D) {                 // 256-column chunks per row, rounded up to the instantiated tiers
    const int k = (D + 255) / 256;
    return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)));
}

// workgroups of a pass: persistent, at most two per CU of a 256-CU device while q fits beside the rows in 256 VGPRs (D <= 2048), one
// above; never more than one row per wave is left without work
static inline int svm_grid(long n, int D) {
    const long cap = svm_chunks(D) <= 8 ? 512 : 256;
    const long want = (n + 3) / 4;
    return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}

template <int KCH, bool VEC>
__device__ __forceinline__ void svm_load_row(const float* row, int D, int lane, float4 x[KCH]) {
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
        const int col = (c * 64 + lane) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (VEC) {
            if (col < D) v = *reinterpret_cast<const float4*>(row + col);        // D % 4 == 0: the load ends inside the row
        } else {
            if (col < D) v.x = row[col];
            if (col + 1 < D) v.y = row[col + 1];
            if (col + 2 < D) v.z = row[col + 2];
            if (col + 3 < D) v.w = row[col + 3];
        }
        x[c] = v;
    }
}

template <int KCH, bool VEC>
__global__ __launch_bounds__(SVM_WG) void svm_pass_kernel(const float* __restrict__ x0, const float* __restrict__ x1, long n0, long n1, long ld0,
                                                          long ld1, double y0, double y1, int D, int mode, double C,
                                                          const double* __restrict__ v, double* __restrict__ z, unsigned char* __restrict__ a,
                                                          double* __restrict__ ws) {
    // v in the lanes' order: sv[(2 c + h) * 64 + lane] = v[(64 c + lane) 4 + 2 h .. + 1]; afterwards the staging area of the partials
    __shared__ double2 sv[KCH * 2 * 64];
    __shared__ double stail[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < KCH * 256; i += SVM_WG) {
        const int c = i >> 8, l = (i & 255) >> 2, j = i & 3;
        reinterpret_cast<double*>(sv)[((c * 2 + (j >> 1)) * 64 + l) * 2 + (j & 1)] = i < D ? v[i] : 0.0;
    }
    const double vb = v[D];
    __syncthreads();

    const long n = n0 + n1, G = (long)gridDim.x * 4;
    double q[KCH * 4];
#pragma unroll
    for (int i = 0; i < KCH * 4; ++i) q[i] = 0.0;
    double qb = 0.0, loss = 0.0;
    float4 xc[KCH], xn[KCH];
    long r = (long)blockIdx.x * 4 + wave;
    int act_c = 0, act_n = 0;
    if (r < n) {
        svm_load_row<KCH, VEC>(r < n0 ? x0 + r * ld0 : x1 + (r - n0) * ld1, D, lane, xc);
        if (mode) act_c = a[r];
    }
    for (; r < n; r += G) {
        const long rn = r + G;
        if (rn < n) {                                       // the next row flies under this row's arithmetic
            svm_load_row<KCH, VEC>(rn < n0 ? x0 + rn * ld0 : x1 + (rn - n0) * ld1, D, lane, xn);
            if (mode) act_n = a[rn];
        }
        // v is re-read from LDS for every row: hoisted out of the loop it would cost as many registers as q and halve the waves per SIMD
        asm volatile("" ::: "memory");
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const double2 va = sv[(c * 2) * 64 + lane], vc = sv[(c * 2 + 1) * 64 + lane];
            t0 = fma((double)xc[c].x, va.x, t0);
            t1 = fma((double)xc[c].y, va.y, t1);
            t2 = fma((double)xc[c].z, vc.x, t2);
            t3 = fma((double)xc[c].w, vc.y, t3);
        }
        double t = (t0 + t1) + (t2 + t3);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);      // (a + b == b + a: every lane ends with the same bits)
        t += vb;
        const double y = r < n0 ? y0 : y1;
        double s;
        if (mode == 0) {
            const double m = 1.0 - y * t;
            const bool on = m > 0.0;
            s = on ? -2.0 * C * y * m : 0.0;
            loss += on ? m * m : 0.0;
            if (lane == 0) {
                z[r] = t;
                a[r] = on ? 1 : 0;
            }
        } else {
            s = act_c ? 2.0 * C * t : 0.0;
            if (z != nullptr && lane == 0) z[r] = t;
        }
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            q[c * 4 + 0] = fma(s, (double)xc[c].x, q[c * 4 + 0]);
            q[c * 4 + 1] = fma(s, (double)xc[c].y, q[c * 4 + 1]);
            q[c * 4 + 2] = fma(s, (double)xc[c].z, q[c * 4 + 2]);
            q[c * 4 + 3] = fma(s, (double)xc[c].w, q[c * 4 + 3]);
        }
        qb += s;
#pragma unroll
        for (int c = 0; c < KCH; ++c) xc[c] = xn[c];
        act_c = act_n;
    }

    // waves 1, 2, 3 hand their partials to wave 0 one after the other: ((q0 + q1) + q2) + q3
    double* stage = reinterpret_cast<double*>(sv);
    for (int w = 1; w < 4; ++w) {
        __syncthreads();                                    // v (first round) / the previous round's partial has been read
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < KCH * 4; ++i) stage[i * 64 + lane] = q[i];
            if (lane == 0) {
                stail[0] = qb;
                stail[1] = loss;
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < KCH * 4; ++i) q[i] += stage[i * 64 + lane];
            qb += stail[0];
            loss += stail[1];
        }
    }
    if (wave == 0) {
        double* out = ws + (long)blockIdx.x * (D + 2);
#pragma unroll
        for (int c = 0; c < KCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = (c * 64 + lane) * 4 + j;
                if (col < D) out[col] = q[c * 4 + j];
            }
        if (lane == 0) {
            out[D] = qb;
            out[D + 1] = loss;
        }
    }
}

// q[col] = sum over the W workgroups' partials, col < P = D + 2: 16 columns x 16 slices of the workgroups per block; a slice adds its
// partials in workgroup order, thread 0..15 then adds the 16 slices in slice order
__global__ __launch_bounds__(256) void svm_reduce_kernel(const double* __restrict__ ws, double* __restrict__ q, int W, int P) {
    __shared__ double sh[16][17];
    const int tid = threadIdx.x, cx = tid & 15, slice = tid >> 4;
    const int col = blockIdx.x * 16 + cx;
    const int per = (W + 15) / 16, lo = slice * per, hi = min(W, lo + per);
    double sum = 0.0;
    if (col < P)
        for (int w = lo; w < hi; ++w) sum += ws[(long)w * P + col];
    sh[slice][cx] = sum;
    __syncthreads();
    if (slice == 0 && col < P) {
        double tot = sh[0][cx];
#pragma unroll
        for (int k = 1; k < 16; ++k) tot += sh[k][cx];
        q[col] = tot;
    }
}

extern "C" size_t shg_svm_pass_workspace_bytes(long n0, long n1, int D) {
    if (D < 1 || D > SVM_MAX_D || n0 < 1 || n1 < 0 || n0 + n1 >= (1L << 31)) return 0;
    return (size_t)svm_grid(n0 + n1, D) * (size_t)(D + 2) * sizeof(double);
}

template <int KCH>
static void svm_launch(bool vec, int W, hipStream_t st, const float* x0, const float* x1, long n0, long n1, long ld0, long ld1, double y0, double y1,
                       int D, int mode, double C, const double* v, double* z, unsigned char* a, double* ws) {
    if (vec) hipLaunchKernelGGL((svm_pass_kernel<KCH, true>), dim3(W), dim3(SVM_WG), 0, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws);
    else hipLaunchKernelGGL((svm_pass_kernel<KCH, false>), dim3(W), dim3(SVM_WG), 0, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws);
}

// x0 [n0, D] with the label y0 and (optional: null with n1 = 0) x1 [n1, D] with y1: float32 rows at a pitch of ld0 / ld1 >= D floats.
// v [D + 1] float64 (the intercept's entry last).  mode 0 (grad): z [n0 + n1] float64 and a [n0 + n1] bytes are written; mode 1 (hv):
// a is read, z is written unless null.  q [D + 2] float64: X~^T s, then (mode 0) the loss sum_i a_i (1 - y_i t_i)^2, (mode 1) 0.
extern "C" int shg_svm_pass_f64(const float* x0, long n0, long ld0, double y0, const float* x1, long n1, long ld1, double y1, int D, int mode, double C,
                                const double* v, double* z, unsigned char* a, double* q, void* workspace, size_t ws_bytes, void* stream) {
    SHG_CHECK_ARG(mode == 0 || mode == 1, "svm_pass: mode must be 0 (grad) or 1 (hv), got %d", mode);
    SHG_CHECK_ARG(x0 && v && a && q, "svm_pass: null pointer (x0, v, a and q are required)");
    SHG_CHECK_ARG(C > 0.0 && __builtin_isfinite(C), "svm_pass: C must be positive and finite, got %g", C);
    SHG_CHECK_ARG(__builtin_isfinite(y0) && __builtin_isfinite(y1), "svm_pass: the labels y0, y1 must be finite, got %g and %g", y0, y1);
    SHG_CHECK_ARG(mode == 1 || z, "svm_pass: null pointer (the grad mode writes z)");
    SHG_CHECK_ARG(D >= 1 && D <= SVM_MAX_D, "svm_pass: D must be 1..%d, got %d", SVM_MAX_D, D);
    SHG_CHECK_ARG(n0 >= 1 && n1 >= 0 && n0 + n1 < (1L << 31), "svm_pass: need n0 >= 1, n1 >= 0 and fewer than 2^31 rows (got %ld and %ld)", n0, n1);
    SHG_CHECK_ARG((n1 == 0) == (x1 == nullptr), "svm_pass: the second row set is a pointer with n1 >= 1 rows, or null with n1 = 0");
    SHG_CHECK_ARG(ld0 >= D && (n1 == 0 || ld1 >= D), "svm_pass: a row pitch is smaller than D = %d (got %ld and %ld)", D, ld0, ld1);
    SHG_CHECK_ARG(((uintptr_t)x0 | (uintptr_t)x1) % 4 == 0, "svm_pass: the rows must be 4-byte aligned");
    SHG_CHECK_ARG(((uintptr_t)v | (uintptr_t)z | (uintptr_t)q | (uintptr_t)workspace) % 8 == 0,
                  "svm_pass: v, z, q and the workspace must be 8-byte aligned");
    SHG_CHECK_ARG(workspace, "svm_pass: null workspace");
    const size_t need = shg_svm_pass_workspace_bytes(n0, n1, D);
    SHG_CHECK_ARG(ws_bytes >= need, "svm_pass: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    // 16-byte loads: every row of both sets must start on a 16-byte boundary and hold whole float4s
    const bool vec = D % 4 == 0 && (uintptr_t)x0 % 16 == 0 && ld0 % 4 == 0 && (n1 == 0 || ((uintptr_t)x1 % 16 == 0 && ld1 % 4 == 0));
    const int W = svm_grid(n0 + n1, D);
    double* ws = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    switch (svm_chunks(D)) {
    case 1: svm_launch<1>(vec, W, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws); break;
    case 2: svm_launch<2>(vec, W, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws); break;
    case 4: svm_launch<4>(vec, W, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws); break;
    case 8: svm_launch<8>(vec, W, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws); break;
    default: svm_launch<16>(vec, W, st, x0, x1, n0, n1, ld0, ld1, y0, y1, D, mode, C, v, z, a, ws); break;
    }
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(svm_reduce_kernel, dim3(shg_cdiv(D + 2, 16)), dim3(256), 0, st, ws, q, W, D + 2);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
