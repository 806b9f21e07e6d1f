// Kernel Inception Distance and Inception Score on the device (reference lib/evaluator/stylegan_metrics/
// kernel_inception_distance.py:34-44 and inception_score.py:30-36; sh-gan_amd/kid.py and inception_score.py drive this file).
//
// KID: per subset s the reference gathers m fake rows x and m real rows y and sums the cubic polynomial kernel
// (u.v / D + 1)^3 over the off-diagonal of x x^T and y y^T and over all of x y^T -- three m x m float matrices per subset on the
// host.  Here one workgroup owns a 64 x 64 tile of one of the three products: it gathers its 64 + 64 rows THROUGH the index
// table while it stages the operand chunks in LDS (no gathered copy of a subset exists in memory), runs the dot products on
// v_mfma_f64_16x16x4_f64 (layout: fid_stats.hip), and applies /D + 1, the cube and the tile's sum to the accumulator registers:
// the m x m kernel matrix never exists either.  The symmetric products walk the tiles on / above the diagonal only
// (off-diagonal tiles count twice, diagonal tiles drop i == j).  Every tile writes ONE partial sum to the caller's workspace
// and a second launch adds a subset's partials in a fixed order: no atomics, the same bits run to run, and a subset's sums do
// not depend on which other subsets share the launch.
//
// LDS operand image: [64 rows][KID_KC doubles] with a row pitch of KID_KP = 18 doubles.  An MFMA operand read is one
// ds_read_b64 per lane at row (lane & 15), k (lane >> 4); the instruction serves lanes 0-31 and 32-63 in one LDS cycle each, and
// within such a half the 16 rows x 2 k's land on dword banks (36 * row + 2 * k) mod 64 = every even bank once: conflict-free.
#include "shg_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define KID_TILE 64
#define KID_KC 16
#define KID_KP 18

static inline long kid_tiles_per_subset(int m) {
    const long T = (m + KID_TILE - 1) / KID_TILE;
    return T * (T + 1) + T * T;          // xx and yy: T (T + 1) / 2 each; xy: T^2
}

template <bool F64IN>
__device__ __forceinline__ void kid_load_row4(const void* base, int row, int D, int k, double v[4]) {
    // row >= 0: a feature row; -1: padding of a ragged tile (zeros, masked in the epilogue); -2: an index outside the feature
    // matrix (NaN: the subset's sums come out NaN instead of the kernel reading out of bounds)
    if (row < 0 || k >= D) {
        const double f = (row == -2 && k < D) ? __builtin_nan("") : 0.0;
        v[0] = v[1] = v[2] = v[3] = f;
        return;
    }
    if (F64IN) {
        const double2* p = reinterpret_cast<const double2*>(reinterpret_cast<const double*>(base) + (long)row * D + k);
        const double2 a = p[0], b = p[1];
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
        const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + (long)row * D + k);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
}

template <bool F64IN>
__global__ __launch_bounds__(256) void kid_tile_kernel(const void* fake, const void* real, const int* idx_f, const int* idx_r, double* ws,
                                                       int n_f, int n_r, int D, int m, int T) {
    __shared__ double sA[KID_TILE * KID_KP], sB[KID_TILE * KID_KP];
    __shared__ int rows[2 * KID_TILE];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y, nsym = T * (T + 1) / 2;
    int tile = blockIdx.x, term = 0, ti, tj;
    if (tile >= 2 * nsym) { term = 2; tile -= 2 * nsym; }
    else if (tile >= nsym) { term = 1; tile -= nsym; }
    if (term == 2) { ti = tile / T; tj = tile - ti * T; }
    else {
        ti = 0;
        while (tile >= T - ti) { tile -= T - ti; ++ti; }      // row ti of the upper triangle holds T - ti tiles
        tj = ti + tile;
    }
    const void* pa = term == 1 ? real : fake;
    const void* pb = term == 0 ? fake : real;
    if (tid < 2 * KID_TILE) {
        const bool isb = tid >= KID_TILE;
        const int r = (isb ? tj : ti) * KID_TILE + (tid & (KID_TILE - 1));
        const int* tab = (isb ? term == 0 : term != 1) ? idx_f : idx_r;
        const int n = (isb ? term == 0 : term != 1) ? n_f : n_r;
        int v = -1;
        if (r < m) {
            v = tab[(long)s * m + r];
            if (v < 0 || v >= n) v = -2;
        }
        rows[tid] = v;
    }
    __syncthreads();
    const int sr = tid >> 2, sk = (tid & 3) * 4;               // staging: 4 threads per row, 4 consecutive k each
    const int ra = rows[sr], rb = rows[KID_TILE + sr];
    const int li = lane & 15, lk = lane >> 4, wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double va[4], vb[4];
    kid_load_row4<F64IN>(pa, ra, D, sk, va);
    kid_load_row4<F64IN>(pb, rb, D, sk, vb);
    for (int k0 = 0; k0 < D; k0 += KID_KC) {
        __syncthreads();                                       // the previous chunk's reads are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sA[sr * KID_KP + sk + q] = va[q];
            sB[sr * KID_KP + sk + q] = vb[q];
        }
        __syncthreads();
        if (k0 + KID_KC < D) {                                 // the next chunk's global loads fly under this chunk's MFMAs
            kid_load_row4<F64IN>(pa, ra, D, k0 + KID_KC + sk, va);
            kid_load_row4<F64IN>(pb, rb, D, k0 + KID_KC + sk, vb);
        }
#pragma unroll
        for (int kk = 0; kk < KID_KC; kk += 4) {
            const double a0 = sA[(wi + li) * KID_KP + kk + lk], a1 = sA[(wi + 16 + li) * KID_KP + kk + lk];
            const double b0 = sB[(wj + li) * KID_KP + kk + lk], b1 = sB[(wj + 16 + li) * KID_KP + kk + lk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // epilogue on the accumulator registers: (dot / D + 1)^3 of the in-range entries (i != j in the symmetric products), summed
    const double dD = (double)D;
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ti * KID_TILE + wi + a * 16 + lk + 4 * r, col = tj * KID_TILE + wj + b * 16 + li;
                const double v = acc[a][b][r] / dD + 1.0;
                if (row < m && col < m && !(term != 2 && row == col)) sum += v * v * v;
            }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const double t = (red[0] + red[1]) + (red[2] + red[3]);
        ws[(long)s * gridDim.x + blockIdx.x] = (term != 2 && tj != ti) ? 2.0 * t : t;
    }
}

// one wave per (term, subset): lane-strided sums of the term's tile partials in tile order, then a fixed butterfly
__global__ __launch_bounds__(64) void kid_reduce_kernel(const double* ws, double* out, int T) {
    const int term = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const int nsym = T * (T + 1) / 2, per = 2 * nsym + T * T;
    const int lo = term == 0 ? 0 : (term == 1 ? nsym : 2 * nsym), hi = term == 0 ? nsym : (term == 1 ? 2 * nsym : per);
    const double* p = ws + (long)s * per;
    double sum = 0.0;
    for (int i = lo + lane; i < hi; i += 64) sum += p[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) out[(long)s * 3 + term] = sum;
}

extern "C" size_t shg_kid_workspace_bytes(int S, int m) {
    if (S < 1 || m < 2) return 0;
    return (size_t)S * (size_t)kid_tiles_per_subset(m) * sizeof(double);
}

// fake [n_f, D], real [n_r, D] (float32, or float64 when is_f64), idx_f / idx_r [S, m] int32 (row numbers of subset s on each
// side), out [S, 3] float64 = { sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j) } with
// k(u, v) = (u.v / D + 1)^3; workspace of shg_kid_workspace_bytes(S, m) bytes.  An index outside [0, n) turns its subset's
// sums into NaN.
extern "C" int shg_kid_sums_f64(const void* fake, const void* real, int is_f64, int n_f, int n_r, int D, const int* idx_f, const int* idx_r,
                                int S, int m, void* workspace, size_t ws_bytes, double* out, void* stream) {
    SHG_CHECK_ARG(fake && real && idx_f && idx_r && out, "kid_sums: null pointer");
    SHG_CHECK_ARG(m >= 2, "kid_sums: a subset needs m >= 2 rows (the estimator divides by m - 1), got %d", m);
    SHG_CHECK_ARG(n_f >= 1 && n_r >= 1 && S >= 1 && S <= 65535, "kid_sums: need n_f, n_r >= 1 and 1 <= S <= 65535");
    SHG_CHECK_ARG(D >= 64 && D % 4 == 0, "kid_sums: D must be at least 64 and a multiple of 4, got %d", D);
    SHG_CHECK_ARG(((uintptr_t)fake | (uintptr_t)real) % 16 == 0, "kid_sums: the feature matrices must be 16-byte aligned");
    const long per = kid_tiles_per_subset(m);
    SHG_CHECK_ARG(per < (1L << 31), "kid_sums: m too large");
    SHG_CHECK_ARG(workspace, "kid_sums: null workspace");
    SHG_CHECK_ARG(ws_bytes >= shg_kid_workspace_bytes(S, m), "kid_sums: workspace too small (%zu bytes, need %zu)", ws_bytes,
                  shg_kid_workspace_bytes(S, m));
    const int T = (m + KID_TILE - 1) / KID_TILE;
    dim3 grid((unsigned)per, S);
    double* ws = reinterpret_cast<double*>(workspace);
    if (is_f64) hipLaunchKernelGGL((kid_tile_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, fake, real, idx_f, idx_r, ws, n_f, n_r, D, m, T);
    else hipLaunchKernelGGL((kid_tile_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, fake, real, idx_f, idx_r, ws, n_f, n_r, D, m, T);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(kid_reduce_kernel, dim3(3, S), dim3(64), 0, (hipStream_t)stream, ws, out, T);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// ---- Inception Score without storing probabilities: exp(mean_i sum_c p_ic (log p_ic - log pbar_c)) over a split equals
// exp(A / n - sum_c pbar_c log pbar_c) with A = sum_i sum_c p_ic log p_ic, P_c = sum_i p_ic, pbar = P / n: a split needs n, A and
// P[C].  acc [num_splits][C + 2] float64 += this batch: columns 0..C-1 = P, column C = A, column C + 1 = n.  Thread c walks the
// batch's images in order (fixed order, no float atomics); the last workgroup forms each image's sum_c p log p by a fixed tree.
// p == 0 contributes 0 to A (the limit of p log p; the reference's numpy gives 0 * -inf = NaN there).
__global__ __launch_bounds__(256) void is_accumulate_kernel(const float* probs, const int* split, double* acc, int B, int C, int num_splits) {
    const int tid = threadIdx.x, W = C + 2;
    if (blockIdx.x + 1 < gridDim.x) {
        const int c = blockIdx.x * 256 + tid;
        if (c >= C) return;
        int cur = -1;
        double run = 0.0;
        for (int i = 0; i < B; ++i) {
            const int s = split[i];
            if (s < 0 || s >= num_splits) continue;
            if (s != cur) {
                if (cur >= 0) acc[(long)cur * W + c] += run;
                cur = s;
                run = 0.0;
            }
            run += (double)probs[(long)i * C + c];
        }
        if (cur >= 0) acc[(long)cur * W + c] += run;
        return;
    }
    __shared__ double red[4];
    for (int i = 0; i < B; ++i) {
        const int s = split[i];
        if (s < 0 || s >= num_splits) continue;             // (uniform over the workgroup)
        double a = 0.0;
        for (int c = tid; c < C; c += 256) {
            const double p = (double)probs[(long)i * C + c];
            if (p > 0.0) a += p * log(p);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) {
            acc[(long)s * W + C] += (red[0] + red[1]) + (red[2] + red[3]);
            acc[(long)s * W + C + 1] += 1.0;
        }
        __syncthreads();
    }
}

// probs [B, C] float32, split [B] int32 (the image's split; negative = skip, a padded duplicate), acc [num_splits, C + 2] float64
// accumulated in place.
extern "C" int shg_is_accumulate_f64(const float* probs, const int* split, double* acc, int B, int C, int num_splits, void* stream) {
    SHG_CHECK_ARG(probs && split && acc, "is_accumulate: null pointer");
    SHG_CHECK_ARG(B >= 1 && C >= 1 && num_splits >= 1, "is_accumulate: need B, C, num_splits >= 1");
    hipLaunchKernelGGL(is_accumulate_kernel, dim3(shg_cdiv(C, 256) + 1), dim3(256), 0, (hipStream_t)stream, probs, split, acc, B, C, num_splits);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
