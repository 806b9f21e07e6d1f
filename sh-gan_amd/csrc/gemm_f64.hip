// Square float64 GEMM on v_mfma_f64_16x16x4_f64 for the device tail of FID (sh-gan_amd/fid_stats.py drives this file): the trace of
// sqrt(Sigma_f Sigma_r) comes from a coupled Newton-Schulz iteration whose every step is three n x n products, n = 2048,
//
//     C[b] = alpha * A[b] . B[b] + beta_diag * I        row-major, leading dimensions lda / ldb / ldc >= n, b < batch (grid.z)
//
// so that T = 1.5 I - 0.5 Z Y is one launch and the two independent products Y T and T Z the next (batch 2: 512 workgroups at n = 2048,
// two per CU).  Not a BLAS: square, float64, row-major, no transposes.
//
// Tile: a workgroup of 4 waves owns 128 x 128 of C, wave w the 64 x 64 quadrant (w >> 1, w & 1) = 4 x 4 MFMA tiles, 128 accumulator
// registers.  The MFMA's lane layout (top of csrc/fid_stats.hip): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], one f64 per
// lane; D: column l & 15, row (l >> 4) + 4 reg.  Per k-step of 4 a wave reads 4 + 4 operand values per lane (ds_read_b64) for 16 MFMAs.
//
// Staging: K in chunks of 16, both operands through LDS, double-buffered: the next chunk's global loads are issued before the current
// chunk's MFMAs and stored to the other buffer after them, one barrier per chunk.  Both images are [k][128 + 16] doubles:
//   B as it lies in memory (k rows, j contiguous);
//   A TRANSPOSED on the way in (its rows are k-contiguous in memory, the fragment wants i fastest across 16 lanes): thread t loads
//     A[i = t & 127][8 (t >> 7) .. + 7] (64 contiguous bytes) and stores 8 doubles down a column of the image, consecutive lanes at
//     consecutive i (ds_write_b64, 128 contiguous bytes per 16 lanes).
//   A ds_read_b64 is served in two groups of 32 lanes, bank = (byte / 4) mod 64: lanes 0-15 read 16 consecutive doubles of row k (32
//   banks), lanes 16-31 those of row k + 1.  The row pitch of 144 doubles = 288 banks = 32 mod 64 puts them on the other 32 banks: no
//   conflict for either operand.  2 operands x 2 buffers x 16 x 144 x 8 B = 72 KiB per workgroup, two workgroups in the CU's 160 KiB.
//
// Edges: any n >= 1.  Loads outside [0, n) are replaced by zeros, stores outside are skipped; nothing beside C[:n, :n] is written.
// 16-byte global loads when every base, pitch and batch stride keeps pairs aligned, 8-byte loads otherwise: the same values reach the
// same lanes, so both forms give the same bits.
//
// Epilogue: every workgroup also writes, when `partials` is given, the sum of the diagonal entries and the sum of the squares of the
// entries of C it has stored, to partials[b][0][tile] and partials[b][1][tile] (tile = blockIdx.y * tiles_x + blockIdx.x): lanes add
// their values in register order, the wave by an xor butterfly (a + b == b + a: the same bits in every lane), the four waves in wave
// order.  The caller adds the tiles in a fixed order (torch.sum over the last axis): tr C and |C|_F^2 without another pass over C.
// No atomics anywhere: the same inputs give the same bits on every run.
#include "shg_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define GEMM64_TILE 128
#define GEMM64_KC 16
#define GEMM64_PITCH 144                                            // doubles per image row: 128 + 16 (32 banks mod 64)
#define GEMM64_IMAGE (GEMM64_KC * GEMM64_PITCH)                     // doubles per operand image
#define GEMM64_LDS (4 * GEMM64_IMAGE * (int)sizeof(double))         // A, B x 2 buffers = 73 728 bytes
#define GEMM64_MAX_N 46336                                          // tiles^2 and n * n stay below 2^31

struct Gemm64Args {
    const double* A;
    const double* B;
    double* C;
    double* partials;
    long lda, ldb, ldc, sa, sb, sc;
    double alpha, beta;
    int n;
};

template <bool VEC>
__device__ __forceinline__ double2 gemm64_load2(const double* p, int col, int n, bool row_ok) {
    double2 v = make_double2(0.0, 0.0);
    if (!row_ok) return v;
    if (VEC) {
        if (col + 1 < n) v = *reinterpret_cast<const double2*>(p);
        else if (col < n) v.x = p[0];
    } else {
        if (col < n) v.x = p[0];
        if (col + 1 < n) v.y = p[1];
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void gemm_f64_kernel(Gemm64Args g) {
    extern __shared__ __align__(16) double lds[];
    __shared__ double wsum[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = g.n, b = blockIdx.z;
    const int i0 = blockIdx.y * GEMM64_TILE, j0 = blockIdx.x * GEMM64_TILE;
    const double* __restrict__ A = g.A + (long)b * g.sa;
    const double* __restrict__ B = g.B + (long)b * g.sb;
    double* __restrict__ C = g.C + (long)b * g.sc;

    // this thread's share of a chunk: A row ai, k = ak .. ak + 7;  B rows bk + 4 p (p < 4), columns bj, bj + 1
    const int ai = tid & 127, ak = (tid >> 7) * 8;
    const int bk = tid >> 6, bj = (tid & 63) * 2;
    const bool a_row_ok = i0 + ai < n;
    const double* a_src = A + (long)(i0 + ai) * g.lda + ak;
    const double* b_src = B + (long)bk * g.ldb + j0 + bj;
    double2 ra[4], rb[4];

    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ra[q] = gemm64_load2<VEC>(a_src + k0 + 2 * q, k0 + ak + 2 * q, n, a_row_ok);
#pragma unroll
        for (int p = 0; p < 4; ++p) rb[p] = gemm64_load2<VEC>(b_src + (long)(k0 + 4 * p) * g.ldb, j0 + bj, n, k0 + bk + 4 * p < n);
    };
    auto stage = [&](int buf) {
        double* as = lds + buf * 2 * GEMM64_IMAGE;
        double* bs = as + GEMM64_IMAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            as[(ak + 2 * q) * GEMM64_PITCH + ai] = ra[q].x;
            as[(ak + 2 * q + 1) * GEMM64_PITCH + ai] = ra[q].y;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<double2*>(bs + (bk + 4 * p) * GEMM64_PITCH + bj) = rb[p];
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int li = lane & 15, lk = lane >> 4;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const int chunks = (n + GEMM64_KC - 1) / GEMM64_KC;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < chunks) fetch((c + 1) * GEMM64_KC);                 // in flight under this chunk's MFMAs
        const double* as = lds + buf * 2 * GEMM64_IMAGE + lk * GEMM64_PITCH + wr + li;
        const double* bs = lds + buf * 2 * GEMM64_IMAGE + GEMM64_IMAGE + lk * GEMM64_PITCH + wc + li;
#pragma unroll
        for (int kk = 0; kk < GEMM64_KC / 4; ++kk) {
            double fa[4], fb[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) fa[m] = as[kk * 4 * GEMM64_PITCH + m * 16];
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = bs[kk * 4 * GEMM64_PITCH + j * 16];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[m], fb[j], acc[m][j], 0, 0, 0);
        }
        if (c + 1 < chunks) stage(buf ^ 1);                             // (the buffer the previous iteration read: every wave is past the barrier below)
        __syncthreads();
    }

    double diag = 0.0, sq = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + wr + m * 16 + lk + 4 * r, col = j0 + wc + j * 16 + li;
                if (row < n && col < n) {
                    const double v = g.alpha * acc[m][j][r] + (row == col ? g.beta : 0.0);
                    C[(long)row * g.ldc + col] = v;
                    sq = fma(v, v, sq);
                    if (row == col) diag += v;
                }
            }
    if (g.partials == nullptr) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        diag += __shfl_xor(diag, o, 64);
        sq += __shfl_xor(sq, o, 64);
    }
    if (lane == 0) {
        wsum[0][wave] = diag;
        wsum[1][wave] = sq;
    }
    __syncthreads();
    if (tid < 2) {
        const long tiles = (long)gridDim.x * gridDim.y;
        g.partials[((long)b * 2 + tid) * tiles + (long)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
    }
}

// the number of C tiles (= partial sums per batch entry and kind) of an n x n product; 0 for an n that is not served
extern "C" int shg_gemm_f64_tiles(int n) {
    if (n < 1 || n > GEMM64_MAX_N) return 0;
    const int t = (n + GEMM64_TILE - 1) / GEMM64_TILE;
    return t * t;
}

// C[b] = alpha A[b] B[b] + beta_diag I for b < batch: n x n float64, row-major at pitches lda, ldb, ldc >= n (doubles); entry b of an
// operand starts stride_x * b doubles after entry 0 (any sign; 0 shares the operand).  C must not overlap A or B.  partials: null, or
// [batch][2][shg_gemm_f64_tiles(n)] doubles = per tile the sum of the diagonal entries and of the squared entries of C.
extern "C" int shg_gemm_f64(const double* A, const double* B, double* C, int n, long lda, long ldb, long ldc, double alpha, double beta_diag,
                            int batch, long stride_a, long stride_b, long stride_c, double* partials, void* stream) {
    SHG_CHECK_ARG(A && B && C, "gemm_f64: null pointer");
    SHG_CHECK_ARG(n >= 1 && n <= GEMM64_MAX_N, "gemm_f64: n must be 1..%d, got %d", GEMM64_MAX_N, n);
    SHG_CHECK_ARG(lda >= n && ldb >= n && ldc >= n, "gemm_f64: a leading dimension is smaller than n = %d (got %ld, %ld, %ld)", n, lda, ldb, ldc);
    SHG_CHECK_ARG(batch >= 1 && batch <= 65535, "gemm_f64: batch must be 1..65535, got %d", batch);
    SHG_CHECK_ARG(batch == 1 || stride_c != 0, "gemm_f64: the batch entries of C must not share their memory (stride_c = 0)");
    SHG_CHECK_ARG(((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)partials) % 8 == 0, "gemm_f64: the operands must be 8-byte aligned");
    const bool vec = (((uintptr_t)A | (uintptr_t)B) % 16 == 0) && lda % 2 == 0 && ldb % 2 == 0 && (batch == 1 || (stride_a % 2 == 0 && stride_b % 2 == 0));
    static ShgDeviceOnce attr_once;
    const int dev_now = shg_current_device();
    if (attr_once.pending(dev_now)) {
        if (hipFuncSetAttribute((const void*)gemm_f64_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM64_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)gemm_f64_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM64_LDS) != hipSuccess) {
            shg_set_error("gemm_f64: cannot reserve %d bytes of LDS", GEMM64_LDS);
            return SHG_ERR_LAUNCH;
        }
        attr_once.mark(dev_now);
    }
    const int t = (n + GEMM64_TILE - 1) / GEMM64_TILE;
    Gemm64Args g{A, B, C, partials, lda, ldb, ldc, stride_a, stride_b, stride_c, alpha, beta_diag, n};
    const dim3 grid(t, t, batch);
    if (vec) hipLaunchKernelGGL(gemm_f64_kernel<true>, grid, dim3(256), GEMM64_LDS, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(gemm_f64_kernel<false>, grid, dim3(256), GEMM64_LDS, (hipStream_t)stream, g);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
