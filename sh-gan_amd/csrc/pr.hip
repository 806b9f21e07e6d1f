// Improved precision and recall (Kynkaanniemi et al.; the `pr50k3_full` metric of the reference's lib/evaluator/stylegan_metrics/
// precision_recall.py:19-60 and metric_main.py; sh-gan_amd/precision_recall.py drives this file).
//
// Semantics.  Features are IEEE fp16 rows [n, D].  d(i, j) = sqrt(max(0, |a|^2 + |b|^2 - 2 a.b)) with the dot product on the fp16 MFMA
// (products of two halves are exact there, the sums are fp32), the squared row norms summed in fp32, one fp32 square root, then ONE
// rounding to fp16: d16.  radius_j = the (k + 1)-th smallest d16(j, .) over the whole set, j itself included (line 53, `kthvalue(k + 1)`
// of a row of cdist(manifold, manifold)).  inside_p = some j has d16(p, j) <= radius_j, a comparison of two fp16 values (line 58).
//
// One sweep kernel serves both.  A workgroup OWNS 128 points (radii: the rows whose k-th neighbour is sought; inside: the probes) and
// SWEEPS a slice of the other side in tiles of 128 rows.  The owners are the MFMA's B operand and the swept rows its A operand, so that
// in the 32 x 32 accumulator block a lane holds ONE owner (column lane & 31) against 16 swept rows (the registers): what a point keeps
// -- its KMAX smallest distances so far, or one flag -- lives in its lane's registers and is updated from the accumulators with no
// lane movement.  No distance is ever written to memory.  The four lists (flags) an owner has at the end of the sweep -- two halves
// of the wave (rows 4 * (lane >> 5) of each 8) times two waves over the swept rows -- are merged through LDS and the slice's result
// goes to the caller's workspace; a second launch merges the slices in slice order.  The slice count depends on the swept side's row
// count alone.  No atomics: the same inputs give the same bits.  Padding rows of a ragged tile are loaded as zeros and masked in the
// epilogue: a padded swept row enters no list and carries radius -1, a padded owner is not written.
//
// LDS operand image: [128 rows][64 halves] per side with a row pitch of 72 halves = 144 bytes.  An operand read is one ds_read_b128
// per lane at row (lane & 31), k = 8 * (lane >> 5); sixteen consecutive rows start at dword banks 36 r mod 64 = the sixteen multiples
// of 4, four banks each: conflict-free.  The next chunk's global loads fly under the current chunk's MFMAs (registers, as kid.hip).
#include "shg_common.h"

typedef _Float16 pr_h8 __attribute__((ext_vector_type(8)));
typedef float pr_f16v __attribute__((ext_vector_type(16)));

#define PR_TILE 128
#define PR_KC 64
#define PR_KP 72
#define PR_MAX_SLICES 16
#define PR_MAX_K 15

static inline int pr_slices(int n_swept, int* tiles_per_slice) {
    const int T = (n_swept + PR_TILE - 1) / PR_TILE;
    const int S0 = T < PR_MAX_SLICES ? T : PR_MAX_SLICES;
    const int tps = (T + S0 - 1) / S0;
    *tiles_per_slice = tps;
    return (T + tps - 1) / tps;
}
static inline int pr_kmax(int k) { return k + 1 <= 4 ? 4 : (k + 1 <= 8 ? 8 : 16); }
static inline size_t pr_round(size_t v) { return (v + 255) / 256 * 256; }

// squared norm of every fp16 row in fp32: one wave per row, lane-strided 16-byte loads, a fixed butterfly
__global__ __launch_bounds__(256) void pr_norm_kernel(const _Float16* x, float* norms, int n, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const pr_h8* p = reinterpret_cast<const pr_h8*>(x + (long)row * D);
    float s = 0.f;
    for (int c = lane; c < D / 8; c += 64) {
        const pr_h8 v = p[c];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += (float)v[q] * (float)v[q];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) norms[row] = s;
}

// keep the K smallest: l ascending, +inf = empty
template <int K>
__device__ __forceinline__ void pr_insert(float (&l)[K], float v) {
    if (v < l[K - 1]) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const float lo = fminf(l[q], v);
            v = fmaxf(l[q], v);
            l[q] = lo;
        }
    }
}

__device__ __forceinline__ uint4 pr_load8(const _Float16* base, int row, int n, int D, int k) {
    if (row >= n || k >= D) return make_uint4(0u, 0u, 0u, 0u);
    return *reinterpret_cast<const uint4*>(base + (long)row * D + k);
}

// KMAX > 0: radii (lists of the KMAX smallest d16 per owner -> ws_lists [slice][n_own][KMAX]); KMAX == 0: the inside test
// (ws_flags [slice][n_own]).  grid (owner tiles, slices), 256 threads = 2 x 2 waves of 64 swept rows x 64 owners.
template <int KMAX>
__global__ __launch_bounds__(256) void pr_sweep_kernel(const _Float16* own, const float* own_norm, int n_own, const _Float16* swp,
                                                       const float* swp_norm, const _Float16* swp_radii, int n_swp, int D,
                                                       int tiles_per_slice, float* ws_lists, unsigned char* ws_flags) {
    constexpr int KL = KMAX > 0 ? KMAX : 1;
    __shared__ __attribute__((aligned(16))) _Float16 sAB[2 * PR_TILE * PR_KP];
    __shared__ float sN[PR_TILE], sR[PR_TILE];
    _Float16* sA = sAB;                          // swept rows
    _Float16* sB = sAB + PR_TILE * PR_KP;        // owners
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, half = lane >> 5, lc = lane & 31;
    const int own_base = blockIdx.x * PR_TILE;
    const int T = (n_swp + PR_TILE - 1) / PR_TILE;
    const int t0 = blockIdx.y * tiles_per_slice, t1 = min(T, t0 + tiles_per_slice);
    const int sr = tid >> 3, sk = (tid & 7) * 8;                 // staging: 8 threads per row, 8 halves each, rows sr + 32 q

    float nb[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int o = own_base + wj * 64 + b * 32 + lc;
        nb[b] = o < n_own ? own_norm[o] : 0.f;
    }
    float list[2][KL];
    int flag[2] = {0, 0};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < KL; ++q) list[b][q] = __builtin_inff();

    for (int t = t0; t < t1; ++t) {
        const int swp_base = t * PR_TILE;
        __syncthreads();                                         // the previous tile's epilogue has read sN / sR
        if (tid < PR_TILE) {
            const int r = swp_base + tid;
            sN[tid] = r < n_swp ? swp_norm[r] : 0.f;
            if (KMAX == 0) sR[tid] = r < n_swp ? (float)swp_radii[r] : -1.f;
        }
        pr_f16v acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
        uint4 va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            va[q] = pr_load8(swp, swp_base + sr + 32 * q, n_swp, D, sk);
            vb[q] = pr_load8(own, own_base + sr + 32 * q, n_own, D, sk);
        }
        for (int k0 = 0; k0 < D; k0 += PR_KC) {
            __syncthreads();                                     // the previous chunk's operand reads are done
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                *reinterpret_cast<uint4*>(sA + (sr + 32 * q) * PR_KP + sk) = va[q];
                *reinterpret_cast<uint4*>(sB + (sr + 32 * q) * PR_KP + sk) = vb[q];
            }
            __syncthreads();
            if (k0 + PR_KC < D) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    va[q] = pr_load8(swp, swp_base + sr + 32 * q, n_swp, D, k0 + PR_KC + sk);
                    vb[q] = pr_load8(own, own_base + sr + 32 * q, n_own, D, k0 + PR_KC + sk);
                }
            }
#pragma unroll
            for (int ks = 0; ks < PR_KC; ks += 16) {
                const int ko = ks + 8 * half;
                const pr_h8 a0 = *reinterpret_cast<const pr_h8*>(sA + (wi * 64 + lc) * PR_KP + ko);
                const pr_h8 a1 = *reinterpret_cast<const pr_h8*>(sA + (wi * 64 + 32 + lc) * PR_KP + ko);
                const pr_h8 b0 = *reinterpret_cast<const pr_h8*>(sB + (wj * 64 + lc) * PR_KP + ko);
                const pr_h8 b1 = *reinterpret_cast<const pr_h8*>(sB + (wj * 64 + 32 + lc) * PR_KP + ko);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        // epilogue on the accumulators: register i of block a is swept row 32 a + (i & 3) + 8 (i >> 2) + 4 half, the lane's column is
        // its owner.  d16 = fp16(sqrt(max(0, |a|^2 + |b|^2 - 2 a.b))), held as the float of that half.
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rl = wi * 64 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
                const float na = sN[rl];
                const bool live = swp_base + rl < n_swp;
                const float rad = KMAX == 0 ? sR[rl] : 0.f;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float d2 = fmaxf((na + nb[b]) - 2.f * acc[a][b][i], 0.f);
                    const float d = (float)(_Float16)__builtin_sqrtf(d2);
                    if (KMAX > 0) {
                        if (live) pr_insert<KL>(list[b], d);
                    } else {
                        flag[b] |= (int)(d <= rad);              // a padded row carries radius -1
                    }
                }
            }
    }
    // merge the owner's four sources (wi, half) through LDS (the operand image is free now), in source order
    __syncthreads();
    const int src = wi * 2 + half;
    if (KMAX > 0) {
        float* buf = reinterpret_cast<float*>(sAB);              // [4 sources][KMAX][128 owners]: 32 KiB at KMAX = 16
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < KL; ++q) buf[(src * KL + q) * PR_TILE + wj * 64 + b * 32 + lc] = list[b][q];
        __syncthreads();
        if (tid < PR_TILE && own_base + tid < n_own) {
            float m[KL];
#pragma unroll
            for (int q = 0; q < KL; ++q) m[q] = buf[q * PR_TILE + tid];
            for (int s = 1; s < 4; ++s)
#pragma unroll
                for (int q = 0; q < KL; ++q) pr_insert<KL>(m, buf[(s * KL + q) * PR_TILE + tid]);
            float* dst = ws_lists + ((long)blockIdx.y * n_own + own_base + tid) * KL;
#pragma unroll
            for (int q = 0; q < KL; ++q) dst[q] = m[q];
        }
    } else {
        int* buf = reinterpret_cast<int*>(sAB);                  // [4 sources][128 owners]
#pragma unroll
        for (int b = 0; b < 2; ++b) buf[src * PR_TILE + wj * 64 + b * 32 + lc] = flag[b];
        __syncthreads();
        if (tid < PR_TILE && own_base + tid < n_own)
            ws_flags[(long)blockIdx.y * n_own + own_base + tid] =
                (unsigned char)((buf[tid] | buf[PR_TILE + tid] | buf[2 * PR_TILE + tid] | buf[3 * PR_TILE + tid]) != 0);
    }
}

// one thread per point: the slices' lists in slice order -> the (k + 1)-th smallest
template <int KMAX>
__global__ __launch_bounds__(256) void pr_radii_merge_kernel(const float* ws_lists, int S, int n, int k, _Float16* radii) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float m[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) m[q] = __builtin_inff();
    for (int s = 0; s < S; ++s) {
        const float* p = ws_lists + ((long)s * n + j) * KMAX;
#pragma unroll
        for (int q = 0; q < KMAX; ++q) pr_insert<KMAX>(m, p[q]);
    }
    float r = m[0];
#pragma unroll
    for (int q = 1; q < KMAX; ++q) r = q == k ? m[q] : r;
    radii[j] = (_Float16)r;                                      // exact: r is the float of a half
}

__global__ __launch_bounds__(256) void pr_inside_merge_kernel(const unsigned char* ws_flags, int S, int m, unsigned char* inside) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    int f = 0;
    for (int s = 0; s < S; ++s) f |= ws_flags[(long)s * m + p];
    inside[p] = (unsigned char)(f != 0);
}

// k >= 1: the workspace of shg_pr_radii_f16 on n rows with neighbourhood k (m is not read); k == 0: the workspace of
// shg_pr_inside_f16 of m probes against n manifold rows.  0 for arguments those calls reject.
extern "C" size_t shg_pr_workspace_bytes(int m, int n, int k) {
    if (n < 2 || k < 0 || k > PR_MAX_K) return 0;
    int tps;
    const size_t S = (size_t)pr_slices(n, &tps);
    if (k >= 1) return pr_round((size_t)n * sizeof(float)) + S * (size_t)n * pr_kmax(k) * sizeof(float);
    if (m < 1) return 0;
    return pr_round((size_t)m * sizeof(float)) + pr_round((size_t)n * sizeof(float)) + S * (size_t)m;
}

static int pr_check_common(const void* p, int rows, int D, const char* what) {
    SHG_CHECK_ARG(D >= 64 && D % 8 == 0, "%s: D must be at least 64 and a multiple of 8, got %d", what, D);
    SHG_CHECK_ARG((uintptr_t)p % 16 == 0, "%s: the feature matrices must be 16-byte aligned", what);
    SHG_CHECK_ARG(rows <= (1 << 30), "%s: too many rows (%d)", what, rows);
    return SHG_OK;
}

// feats [n, D] fp16 -> radii [n] fp16: the (k + 1)-th smallest d16(j, .) over all n rows, j included.  1 <= k <= 15, n >= k + 1,
// D >= 64 a multiple of 8, feats 16-byte aligned; workspace of shg_pr_workspace_bytes(n, n, k) bytes.  Three launches.
extern "C" int shg_pr_radii_f16(const void* feats, int n, int D, int k, void* workspace, size_t ws_bytes, void* radii_out, void* stream) {
    SHG_CHECK_ARG(feats && radii_out, "pr_radii: null pointer");
    SHG_CHECK_ARG(k >= 1 && k <= PR_MAX_K, "pr_radii: nhood_size must be 1..%d, got %d", PR_MAX_K, k);
    SHG_CHECK_ARG(n >= k + 1, "pr_radii: need at least nhood_size + 1 = %d rows, got %d", k + 1, n);
    if (int rc = pr_check_common(feats, n, D, "pr_radii")) return rc;
    SHG_CHECK_ARG(workspace, "pr_radii: null workspace");
    const size_t need = shg_pr_workspace_bytes(n, n, k);
    SHG_CHECK_ARG(ws_bytes >= need, "pr_radii: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    int tps;
    const int S = pr_slices(n, &tps), KM = pr_kmax(k);
    const _Float16* x = reinterpret_cast<const _Float16*>(feats);
    float* norms = reinterpret_cast<float*>(workspace);
    float* lists = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pr_round((size_t)n * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pr_norm_kernel, dim3(shg_cdiv(n, 4)), dim3(256), 0, st, x, norms, n, D);
    SHG_CHECK_LAUNCH();
    const dim3 grid(shg_cdiv(n, PR_TILE), S);
    _Float16* out = reinterpret_cast<_Float16*>(radii_out);
    if (KM == 4) {
        hipLaunchKernelGGL((pr_sweep_kernel<4>), grid, dim3(256), 0, st, x, norms, n, x, norms, nullptr, n, D, tps, lists, nullptr);
        SHG_CHECK_LAUNCH();
        hipLaunchKernelGGL((pr_radii_merge_kernel<4>), dim3(shg_cdiv(n, 256)), dim3(256), 0, st, lists, S, n, k, out);
    } else if (KM == 8) {
        hipLaunchKernelGGL((pr_sweep_kernel<8>), grid, dim3(256), 0, st, x, norms, n, x, norms, nullptr, n, D, tps, lists, nullptr);
        SHG_CHECK_LAUNCH();
        hipLaunchKernelGGL((pr_radii_merge_kernel<8>), dim3(shg_cdiv(n, 256)), dim3(256), 0, st, lists, S, n, k, out);
    } else {
        hipLaunchKernelGGL((pr_sweep_kernel<16>), grid, dim3(256), 0, st, x, norms, n, x, norms, nullptr, n, D, tps, lists, nullptr);
        SHG_CHECK_LAUNCH();
        hipLaunchKernelGGL((pr_radii_merge_kernel<16>), dim3(shg_cdiv(n, 256)), dim3(256), 0, st, lists, S, n, k, out);
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// probes [m, D], manifold [n, D], radii [n] (shg_pr_radii_f16 of the manifold), all fp16 -> inside [m] uint8: 1 when some j has
// d16(p, j) <= radii[j].  m >= 1, n >= 2, D as above; workspace of shg_pr_workspace_bytes(m, n, 0) bytes.  Four launches.
extern "C" int shg_pr_inside_f16(const void* probes, int m, const void* manifold, int n, int D, const void* radii, void* workspace,
                                 size_t ws_bytes, unsigned char* inside_out, void* stream) {
    SHG_CHECK_ARG(probes && manifold && radii && inside_out, "pr_inside: null pointer");
    SHG_CHECK_ARG(m >= 1 && n >= 2, "pr_inside: need m >= 1 probes and n >= 2 manifold rows, got %d and %d", m, n);
    if (int rc = pr_check_common(probes, m, D, "pr_inside")) return rc;
    if (int rc = pr_check_common(manifold, n, D, "pr_inside")) return rc;
    SHG_CHECK_ARG(workspace, "pr_inside: null workspace");
    const size_t need = shg_pr_workspace_bytes(m, n, 0);
    SHG_CHECK_ARG(ws_bytes >= need, "pr_inside: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    int tps;
    const int S = pr_slices(n, &tps);
    const _Float16* xp = reinterpret_cast<const _Float16*>(probes);
    const _Float16* xm = reinterpret_cast<const _Float16*>(manifold);
    char* w = reinterpret_cast<char*>(workspace);
    float* norm_p = reinterpret_cast<float*>(w);
    float* norm_m = reinterpret_cast<float*>(w + pr_round((size_t)m * sizeof(float)));
    unsigned char* flags = reinterpret_cast<unsigned char*>(w + pr_round((size_t)m * sizeof(float)) + pr_round((size_t)n * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pr_norm_kernel, dim3(shg_cdiv(m, 4)), dim3(256), 0, st, xp, norm_p, m, D);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pr_norm_kernel, dim3(shg_cdiv(n, 4)), dim3(256), 0, st, xm, norm_m, n, D);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL((pr_sweep_kernel<0>), dim3(shg_cdiv(m, PR_TILE), S), dim3(256), 0, st, xp, norm_p, m, xm, norm_m,
                       reinterpret_cast<const _Float16*>(radii), n, D, tps, nullptr, flags);
    SHG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pr_inside_merge_kernel, dim3(shg_cdiv(m, 256)), dim3(256), 0, st, flags, S, m, inside_out);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
