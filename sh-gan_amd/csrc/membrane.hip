// Gradient-domain (Poisson) paste-back for sh-gan_amd/inpaint.py: the generated window keeps its gradients and takes its absolute level from
// the photograph at the rim of the blended region.  Three entry points:
//
//   shg_inpaint_membrane_setup_f32   per (image, sample): g (the resampled, scaled generator output -- the bits paste_back computes, through
//                                    the device functions of inpaint_common.h), the field (d = orig - g where A = 0, 0 in Omega = {A > 0})
//                                    and the uint8 Omega mask, over the solve grid (a box of the window named by the host);
//   shg_membrane_solve_f32           a masked Laplace solver that knows nothing about images (below);
//   shg_inpaint_membrane_paste_u8    paste_back's last step with clamp(g + c, 0, 255) in place of g.
//
// THE SOLVER.  P ragged problems {h, w, field offset, omega offset}: field float32 [h][w][3], omega uint8 [h][w].  On return the field holds
// c in Omega, 4 c(p) - sum_{q in N4(p)} c(q) = 0, with the values outside Omega as Dirichlet data (outside the h x w grid: 0); it is
// untouched outside Omega.  Geometric multigrid V(2,2)-cycles:
//   * levels: cell-centred 2x coarsening, (h, w) -> (ceil(h / 2), ceil(w / 2)), until both sides are <= MB_COARSEST;
//   * a coarse cell is in Omega when ALL four children are (in the grid and in Omega): the coarse domain lies inside the fine one, so the
//     coarse correction is never larger than the fine error near the rim.  (With "any child" the coarse domain overhangs the Dirichlet
//     rim, the correction overshoots there, and the cycle diverges on every irregular domain that was tried.)  Thin parts of Omega vanish
//     from the coarse levels; the smoother alone serves them, which it does well: a thin part is strongly diagonally dominant;
//   * the unscaled (4, -1) stencil on every level, the residual restricted by summing the four children, bilinear prolongation;
//   * smoother: red-black Gauss-Seidel, two sweeps (four half-sweeps) per launch on an LDS tile of MB_TILE x MB_TILE cells with a halo
//     of four cells.  Half-sweep s updates the tile grown by 4 - s cells, so the interior comes out exactly as four global half-sweeps
//     would leave it: no iterate depends on the tiling.  A launch reads one buffer and writes the other (field <-> a shadow in the
//     workspace), so no workgroup reads what another writes.  A tile without a cell of Omega returns on a workgroup-uniform test before
//     it reads a value; the two buffers agree there because nothing outside Omega is ever written;
//   * coarsest level: one workgroup, the level in LDS, 60 red-black SOR sweeps (omega = 1.7) and 4 plain ones.
// Stop rule, on the device: before every cycle (and after the last) the residual's max norm over Omega and the three channels is reduced
// through per-tile partial maxima (plain stores, one reducing workgroup per problem, no atomics) and compared: <= res_tol -> state 1;
// not lower than before the previous cycle -> state 2 (the float32 floor); a problem whose state is set makes every later launch return
// at once.  The launch sequence of max_cycles cycles is fixed and enqueued without a host round trip.  A problem's arithmetic touches
// its own slices only: its bits do not depend on the batch or on the run.
//
// Workspace of the solver, per problem a slice of mb_ws_floats(max_h, max_w) floats: the level-0 shadow [h][w][3], the partial maxima of
// the level-0 tiles, and per coarse level u, its shadow, the right-hand side (each [h_l][w_l][3]) and the level's Omega bytes.
#include "inpaint_common.h"

namespace {

constexpr int MB_TILE = 32;              // inpaint.py MEMBRANE_TILE
constexpr int MB_HALO = 4;               // two red-black sweeps
constexpr int MB_REG = MB_TILE + 2 * MB_HALO;
constexpr int MB_COARSEST = 16;          // inpaint.py MEMBRANE_COARSEST
constexpr int MB_THREADS = 256;
constexpr int MB_MAX_SIDE = 16384;
constexpr int MB_SOR_SWEEPS = 60, MB_GS_SWEEPS = 4;
constexpr float MB_SOR = 1.7f;

__host__ __device__ inline long mb_r4(long n) { return (n + 3) & ~3L; }

__host__ __device__ inline int mb_levels(int h, int w) {
    int L = 1;
    while ((h > w ? h : w) > MB_COARSEST) h = (h + 1) >> 1, w = (w + 1) >> 1, ++L;
    return L;
}

__host__ __device__ inline long mb_tiles(int h, int w) { return (long)((h + MB_TILE - 1) / MB_TILE) * ((w + MB_TILE - 1) / MB_TILE); }

// floats of one problem's workspace slice (monotone in h and in w)
__host__ __device__ inline long mb_ws_floats(int h, int w) {
    long n = mb_r4(3L * h * w) + mb_r4(mb_tiles(h, w));
    while ((h > w ? h : w) > MB_COARSEST) {
        h = (h + 1) >> 1, w = (w + 1) >> 1;
        n += 3 * mb_r4(3L * h * w) + mb_r4(((long)h * w + 3) >> 2);
    }
    return n;
}

struct MbArgs {
    float* field;
    long field_elems;
    const uint8_t* omega;
    long omega_bytes;
    const int* table;
    float* ws;
    long ws_stride;
    int* info;
    const float* res_tol;
    int max_h, max_w;
};

struct MbLevel {
    int h, w;
    float *A, *B;          // the level's unknowns and their shadow (level 0: the field and the workspace's copy)
    const float* f;        // right-hand side (level 0: none, it is 0)
    float* fw;
    uint8_t* om;
    float* partial;        // level 0 only
};

struct MbProb {
    int h, w, L;
    long foff, ooff;
};

// Problem p, or false when its descriptor points outside the buffers or (check_state) its state is set.
__device__ __forceinline__ bool mb_enter(const MbArgs& a, int p, bool check_state, MbProb& pr) {
    const int* t = a.table + 4L * p;
    pr.h = t[0], pr.w = t[1], pr.foff = t[2], pr.ooff = t[3];
    if (pr.h < 1 || pr.w < 1 || pr.h > a.max_h || pr.w > a.max_w || pr.foff < 0 || pr.ooff < 0) return false;
    if (pr.foff + 3L * pr.h * pr.w > a.field_elems || pr.ooff + (long)pr.h * pr.w > a.omega_bytes) return false;
    if (check_state && a.info[3L * p + 2] != 0) return false;
    pr.L = mb_levels(pr.h, pr.w);
    return true;
}

// Level l (< pr.L) of problem p.  Level 0's Omega is the caller's (read only; `om` is written on coarse levels alone).
__device__ __forceinline__ void mb_level(const MbArgs& a, int p, const MbProb& pr, int l, MbLevel& lv) {
    float* s = a.ws + (long)p * a.ws_stride;
    int h = pr.h, w = pr.w;
    lv.partial = s + mb_r4(3L * h * w);
    if (l == 0) {
        lv.h = h, lv.w = w, lv.A = a.field + pr.foff, lv.B = s, lv.f = nullptr, lv.fw = nullptr;
        lv.om = const_cast<uint8_t*>(a.omega) + pr.ooff;
        return;
    }
    s = lv.partial + mb_r4(mb_tiles(h, w));
    for (int i = 1;; ++i) {
        h = (h + 1) >> 1, w = (w + 1) >> 1;
        const long n = mb_r4(3L * h * w);
        if (i == l) {
            lv.h = h, lv.w = w, lv.A = s, lv.B = s + n, lv.fw = s + 2 * n, lv.f = lv.fw, lv.om = reinterpret_cast<uint8_t*>(s + 3 * n);
            return;
        }
        s += 3 * n + mb_r4(((long)h * w + 3) >> 2);
    }
}

// The workgroup's tile of a level: false when the level has fewer tiles.
__device__ __forceinline__ bool mb_tile(int h, int w, int& ty0, int& tx0) {
    const int nx = (w + MB_TILE - 1) / MB_TILE, ny = (h + MB_TILE - 1) / MB_TILE;
    const int t = blockIdx.x, ty = t / nx;
    if (ty >= ny) return false;
    ty0 = ty * MB_TILE, tx0 = (t - ty * nx) * MB_TILE;
    return true;
}

__device__ __forceinline__ float mb_at(const float* u, int h, int w, int y, int x, int c) {
    return (y >= 0 && y < h && x >= 0 && x < w) ? u[((long)y * w + x) * 3 + c] : 0.f;
}

// 4 u - (sum of the four neighbours), neighbours outside the grid 0
__device__ __forceinline__ float mb_stencil(const float* u, int h, int w, int y, int x, int c) {
    const float nb = (mb_at(u, h, w, y - 1, x, c) + mb_at(u, h, w, y + 1, x, c)) + (mb_at(u, h, w, y, x - 1, c) + mb_at(u, h, w, y, x + 1, c));
    return 4.f * u[((long)y * w + x) * 3 + c] - nb;
}

// info[p] = (0, +inf, 0); the shadow of the field
__global__ __launch_bounds__(MB_THREADS) void mb_init_kernel(MbArgs a) {
    const int p = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.info[3L * p] = 0, a.info[3L * p + 1] = 0x7f800000, a.info[3L * p + 2] = 0;
    MbProb pr;
    if (!mb_enter(a, p, false, pr)) return;
    MbLevel lv;
    mb_level(a, p, pr, 0, lv);
    int ty0, tx0;
    if (!mb_tile(lv.h, lv.w, ty0, tx0)) return;
    const int rows = min(MB_TILE, lv.h - ty0), nf = 3 * min(MB_TILE, lv.w - tx0);
    for (int e = threadIdx.x; e < rows * nf; e += MB_THREADS) {
        const int r = e / nf, j = e - r * nf;
        const long i = ((long)(ty0 + r) * lv.w + tx0) * 3 + j;
        lv.B[i] = lv.A[i];
    }
}

// Omega of level l + 1 from level l; the level's unknowns and their shadow start as 0 (outside Omega they stay 0)
__global__ __launch_bounds__(MB_THREADS) void mb_coarsen_kernel(MbArgs a, int l) {
    const int p = blockIdx.y;
    MbProb pr;
    if (!mb_enter(a, p, false, pr) || l + 1 >= pr.L) return;
    MbLevel fi, co;
    mb_level(a, p, pr, l, fi);
    mb_level(a, p, pr, l + 1, co);
    int ty0, tx0;
    if (!mb_tile(co.h, co.w, ty0, tx0)) return;
    for (int e = threadIdx.x; e < MB_TILE * MB_TILE; e += MB_THREADS) {
        const int y = ty0 + e / MB_TILE, x = tx0 + e % MB_TILE;
        if (y >= co.h || x >= co.w) continue;
        int in = 2 * y + 1 < fi.h && 2 * x + 1 < fi.w;
        if (in) {
            const uint8_t* o = fi.om + (long)(2 * y) * fi.w + 2 * x;
            in = o[0] != 0 && o[1] != 0 && o[fi.w] != 0 && o[fi.w + 1] != 0;
        }
        const long i = (long)y * co.w + x;
        co.om[i] = (uint8_t)in;
        for (int c = 0; c < 3; ++c) co.A[3 * i + c] = 0.f, co.B[3 * i + c] = 0.f;
    }
}

// per-tile maxima of |residual| of the field (level 0, right-hand side 0)
__global__ __launch_bounds__(MB_THREADS) void mb_norm_kernel(MbArgs a) {
    __shared__ float red[MB_THREADS];
    const int p = blockIdx.y;
    MbProb pr;
    if (!mb_enter(a, p, true, pr)) return;
    MbLevel lv;
    mb_level(a, p, pr, 0, lv);
    int ty0, tx0;
    if (!mb_tile(lv.h, lv.w, ty0, tx0)) return;
    float m = 0.f;
    for (int e = threadIdx.x; e < MB_TILE * MB_TILE; e += MB_THREADS) {
        const int y = ty0 + e / MB_TILE, x = tx0 + e % MB_TILE;
        if (y >= lv.h || x >= lv.w || lv.om[(long)y * lv.w + x] == 0) continue;
        for (int c = 0; c < 3; ++c) {
            const float r = fabsf(mb_stencil(lv.A, lv.h, lv.w, y, x, c));
            m = r > m || r != r ? r : m;                            // (a NaN sticks: such a problem is never certified)
        }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = MB_THREADS >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float o = red[threadIdx.x + s], v = red[threadIdx.x];
            red[threadIdx.x] = (o > v || o != o) ? o : v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) lv.partial[blockIdx.x] = red[0];
}

// the problem's norm from its partials, and the stop rule: `cyc` cycles have run
__global__ __launch_bounds__(MB_THREADS) void mb_state_kernel(MbArgs a, int cyc) {
    __shared__ float red[MB_THREADS];
    const int p = blockIdx.x;
    MbProb pr;
    if (!mb_enter(a, p, true, pr)) return;
    MbLevel lv;
    mb_level(a, p, pr, 0, lv);
    const int nt = (int)mb_tiles(lv.h, lv.w);
    float m = 0.f;
    for (int e = threadIdx.x; e < nt; e += MB_THREADS) {
        const float o = lv.partial[e];
        m = (o > m || o != o) ? o : m;
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = MB_THREADS >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float o = red[threadIdx.x + s], v = red[threadIdx.x];
            red[threadIdx.x] = (o > v || o != o) ? o : v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float n = red[0], prev = __int_as_float(a.info[3L * p + 1]);
        int state = 0;
        if (n <= a.res_tol[p]) state = 1;
        else if (!(n < prev)) state = 2;
        a.info[3L * p] = cyc, a.info[3L * p + 1] = __float_as_int(n), a.info[3L * p + 2] = state;
    }
}

// two red-black Gauss-Seidel sweeps of level l on the tile's LDS copy; dir 0: A -> B, dir 1: B -> A
__global__ __launch_bounds__(MB_THREADS) void mb_smooth_kernel(MbArgs a, int l, int dir) {
    __shared__ __attribute__((aligned(16))) float u[MB_REG * MB_REG * 3];
    __shared__ __attribute__((aligned(16))) float f[MB_REG * MB_REG * 3];
    __shared__ uint8_t om[MB_REG * MB_REG];
    const int p = blockIdx.y;
    MbProb pr;
    if (!mb_enter(a, p, true, pr) || l + 1 >= pr.L) return;
    MbLevel lv;
    mb_level(a, p, pr, l, lv);
    int ty0, tx0;
    if (!mb_tile(lv.h, lv.w, ty0, tx0)) return;
    const float* src = dir ? lv.B : lv.A;
    float* dst = dir ? lv.A : lv.B;
    const int h = lv.h, w = lv.w;
    int found = 0;
    for (int e = threadIdx.x; e < MB_REG * MB_REG; e += MB_THREADS) {
        const int ry = e / MB_REG, rx = e - ry * MB_REG, y = ty0 - MB_HALO + ry, x = tx0 - MB_HALO + rx;
        const int o = (y >= 0 && y < h && x >= 0 && x < w) ? lv.om[(long)y * w + x] != 0 : 0;
        om[e] = (uint8_t)o;
        found |= o && ry >= MB_HALO && ry < MB_HALO + MB_TILE && rx >= MB_HALO && rx < MB_HALO + MB_TILE;
    }
    if (!__syncthreads_or(found)) return;                           // no cell of Omega in the tile: nothing to update
    for (int e = threadIdx.x; e < MB_REG * MB_REG * 3; e += MB_THREADS) {
        const int ry = e / (3 * MB_REG), j = e - ry * (3 * MB_REG), y = ty0 - MB_HALO + ry, x = tx0 - MB_HALO + j / 3;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        const long i = ((long)y * w + tx0 - MB_HALO) * 3 + j;
        u[e] = in ? src[i] : 0.f;
        f[e] = (in && lv.f) ? lv.f[i] : 0.f;
    }
    __syncthreads();
    for (int s = 1; s <= MB_HALO; ++s) {
        const int par = (s - 1) & 1, n = MB_REG - 2 * s;            // the region of this half-sweep: [s, s + n) both ways
        for (int e = threadIdx.x; e < n * (MB_REG / 2); e += MB_THREADS) {
            const int ry = s + e / (MB_REG / 2), rx = 2 * (e % (MB_REG / 2)) + ((ry + par) & 1);     // (ty0 + tx0 - 2 MB_HALO is even)
            if (rx < s || rx >= s + n || !om[ry * MB_REG + rx]) continue;
            float* q = u + (ry * MB_REG + rx) * 3;
            const float* fq = f + (ry * MB_REG + rx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = 0.25f * (fq[c] + ((q[c - 3 * MB_REG] + q[c + 3 * MB_REG]) + (q[c - 3] + q[c + 3])));
        }
        __syncthreads();
    }
    const int rows = min(MB_TILE, h - ty0), nf = 3 * min(MB_TILE, w - tx0);
    for (int e = threadIdx.x; e < rows * nf; e += MB_THREADS) {
        const int r = e / nf, j = e - r * nf, cell = (r + MB_HALO) * MB_REG + MB_HALO + j / 3;
        if (om[cell]) dst[((long)(ty0 + r) * w + tx0) * 3 + j] = u[(r + MB_HALO) * MB_REG * 3 + MB_HALO * 3 + j];
    }
}

// right-hand side of level l + 1: the residual of level l's shadow, summed over the four children; level l + 1 starts from 0
__global__ __launch_bounds__(MB_THREADS) void mb_restrict_kernel(MbArgs a, int l) {
    const int p = blockIdx.y;
    MbProb pr;
    if (!mb_enter(a, p, true, pr) || l + 1 >= pr.L) return;
    MbLevel fi, co;
    mb_level(a, p, pr, l, fi);
    mb_level(a, p, pr, l + 1, co);
    int ty0, tx0;
    if (!mb_tile(co.h, co.w, ty0, tx0)) return;
    for (int e = threadIdx.x; e < MB_TILE * MB_TILE; e += MB_THREADS) {
        const int y = ty0 + e / MB_TILE, x = tx0 + e % MB_TILE;
        if (y >= co.h || x >= co.w) continue;
        const long i = (long)y * co.w + x;
        float r[3] = {0.f, 0.f, 0.f};
        if (co.om[i]) {                                             // all four children lie in the grid and in Omega
            for (int c = 0; c < 3; ++c) {
                float s4[4];
                for (int k = 0; k < 4; ++k) {
                    const int cy = 2 * y + (k >> 1), cx = 2 * x + (k & 1);
                    const float fv = fi.f ? fi.f[((long)cy * fi.w + cx) * 3 + c] : 0.f;
                    s4[k] = fv - mb_stencil(fi.B, fi.h, fi.w, cy, cx, c);
                }
                r[c] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            }
        }
        for (int c = 0; c < 3; ++c) co.fw[3 * i + c] = r[c], co.A[3 * i + c] = 0.f;
    }
}

// the coarsest level of every problem, in one workgroup: red-black SOR, then plain sweeps
__global__ __launch_bounds__(MB_THREADS) void mb_coarsest_kernel(MbArgs a) {
    constexpr int S = MB_COARSEST + 2;
    __shared__ float u[S * S * 3];
    const int p = blockIdx.x;
    MbProb pr;
    if (!mb_enter(a, p, true, pr)) return;
    MbLevel lv;
    mb_level(a, p, pr, pr.L - 1, lv);
    const int h = lv.h, w = lv.w;                                   // both <= MB_COARSEST
    for (int e = threadIdx.x; e < S * S * 3; e += MB_THREADS) u[e] = 0.f;
    __syncthreads();
    const int y = threadIdx.x / MB_COARSEST, x = threadIdx.x % MB_COARSEST;
    const bool in = y < h && x < w;
    const long i = (long)y * w + x;
    const bool act = in && lv.om[i] != 0;
    float fv[3] = {0.f, 0.f, 0.f};
    float* q = u + ((y + 1) * S + x + 1) * 3;
    if (in)
        for (int c = 0; c < 3; ++c) {
            q[c] = lv.A[3 * i + c];
            if (act && lv.f) fv[c] = lv.f[3 * i + c];
        }
    __syncthreads();
    for (int it = 0; it < 2 * (MB_SOR_SWEEPS + MB_GS_SWEEPS); ++it) {
        const float om = it < 2 * MB_SOR_SWEEPS ? MB_SOR : 1.f;
        if (act && ((y + x + it) & 1) == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = 0.25f * (fv[c] + ((q[c - 3 * S] + q[c + 3 * S]) + (q[c - 3] + q[c + 3])));
                q[c] = om == 1.f ? t : q[c] + om * (t - q[c]);
            }
        }
        __syncthreads();
    }
    if (act)
        for (int c = 0; c < 3; ++c) lv.A[3 * i + c] = q[c];
}

// level l's shadow += the bilinear interpolation of level l + 1's unknowns (0 outside its Omega and outside its grid), in Omega
__global__ __launch_bounds__(MB_THREADS) void mb_prolong_kernel(MbArgs a, int l) {
    const int p = blockIdx.y;
    MbProb pr;
    if (!mb_enter(a, p, true, pr) || l + 1 >= pr.L) return;
    MbLevel fi, co;
    mb_level(a, p, pr, l, fi);
    mb_level(a, p, pr, l + 1, co);
    int ty0, tx0;
    if (!mb_tile(fi.h, fi.w, ty0, tx0)) return;
    for (int e = threadIdx.x; e < MB_TILE * MB_TILE; e += MB_THREADS) {
        const int y = ty0 + e / MB_TILE, x = tx0 + e % MB_TILE;
        if (y >= fi.h || x >= fi.w || fi.om[(long)y * fi.w + x] == 0) continue;
        const int Y = y >> 1, X = x >> 1, Y2 = Y + ((y & 1) ? 1 : -1), X2 = X + ((x & 1) ? 1 : -1);
        float* q = fi.B + ((long)y * fi.w + x) * 3;
        for (int c = 0; c < 3; ++c) {
            const float e4 = (9.f * mb_at(co.A, co.h, co.w, Y, X, c) + 3.f * mb_at(co.A, co.h, co.w, Y2, X, c)) +
                             (3.f * mb_at(co.A, co.h, co.w, Y, X2, c) + mb_at(co.A, co.h, co.w, Y2, X2, c));
            q[c] = q[c] + 0.0625f * e4;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the two image-side kernels.  grids: int32 [B][6] = {gy0, gx0, gh, gw (the solve grid, in window coordinates), float offset of the
// image's K planes [K][gh][gw][3] in g / field, byte offset of its Omega [gh][gw]}.
// ---------------------------------------------------------------------------------------------------------------------------------------

struct MbGrid {
    int gy0, gx0, gh, gw;
    long foff, ooff;
};

__device__ __forceinline__ bool mb_load_grid(const int* grids, int b, const IpDesc& d, int K, long g_elems, long om_bytes, MbGrid& g) {
    const int* t = grids + 6L * b;
    g.gy0 = t[0], g.gx0 = t[1], g.gh = t[2], g.gw = t[3], g.foff = t[4], g.ooff = t[5];
    if (g.gy0 < 0 || g.gx0 < 0 || g.gh < 1 || g.gw < 1 || (long)g.gy0 + g.gh > d.ch || (long)g.gx0 + g.gw > d.cw) return false;
    if (g.foff < 0 || g.ooff < 0 || g.foff + 3L * K * g.gh * g.gw > g_elems || g.ooff + (long)g.gh * g.gw > om_bytes) return false;
    return true;
}

__global__ __launch_bounds__(IP_THREADS) void membrane_setup_kernel(const uint8_t* __restrict__ src, long img_bytes, const uint8_t* __restrict__ msk,
                                                                    long msk_bytes, const int* __restrict__ tab, long tab_elems,
                                                                    const int* __restrict__ grids, const float* __restrict__ fake,
                                                                    float* __restrict__ gws, float* __restrict__ field, long g_elems,
                                                                    uint8_t* __restrict__ omega, long om_bytes, int R, int K, int feather,
                                                                    int lds_bytes, const int* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ip_lds[];
    const int b = blockIdx.z;
    IpDesc d;
    if (!ip_load_desc(tab, tab_elems, b, img_bytes, msk_bytes, false, R, d)) return;
    const int key = ip_load_key(keys, b);
    if (key < 0) return;
    MbGrid g;
    if (!mb_load_grid(grids, b, d, K, g_elems, om_bytes, g)) return;
    const int y0 = (int)blockIdx.y * d.TB, c0 = (int)blockIdx.x * d.CW;
    if (y0 >= d.ch || c0 >= d.cw) return;
    const int y1 = min(y0 + d.TB, d.ch), rows = y1 - y0, cn = min(d.CW, d.cw - c0);
    // the part of the tile inside the solve grid (workgroup-uniform)
    const int ry0 = max(y0, g.gy0), ry1 = min(y1, g.gy0 + g.gh), rx0 = max(c0, g.gx0), rx1 = min(c0 + cn, g.gx0 + g.gw);
    if (ry0 >= ry1 || rx0 >= rx1) return;
    const int sy0 = max(tab[d.vb + 2 * y0], 0);
    const int sy1 = (int)min((long)tab[d.vb + 2 * (y1 - 1)] + tab[d.vb + 2 * (y1 - 1) + 1], (long)R);
    const int span = sy1 - sy0;
    IpTile t;
    ip_tile_make(t, ip_lds, y0, c0, rows, cn, feather);
    if (span < 1 || (long)t.a_bytes + max((long)t.t_bytes + t.r_bytes, 12L * span * cn) > lds_bytes) return;
    const bool holes = ip_feather_tile(t, msk, d, feather, (uint32_t)key);   // false: A = 0 in the tile (t.A is not written)
    const long RR = (long)R * R, plane = 3L * g.gh * g.gw;
    const int nr = ry1 - ry0, nq = 3 * (rx1 - rx0), nb = 3 * cn;
    const uint8_t* img = src + d.off;
    for (int k = 0; k < K; ++k) {
        ip_resample_rows(t, tab, d, fake + ((long)b * K + k) * 3 * RR, R, sy0, span);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * nq; e += IP_THREADS) {
            const int rr = e / nq, j = e - rr * nq, oy = ry0 + rr, r = oy - y0, q = 3 * (rx0 - c0) + j;
            const int rel = tab[d.vb + 2 * oy] - sy0, n = tab[d.vb + 2 * oy + 1];
            if (rel < 0 || n < 0 || n > d.KV || (long)rel + n > span) continue;
            const float gv = ip_scale(ip_resample_col(tab + d.vk + (long)oy * d.KV, t.mid + (long)rel * nb, n, nb, q));
            const int a = holes ? t.A[r * cn + q / 3] : 0;
            const float orig = (float)img[((long)(d.wy0 + oy) * d.w + d.wx0 + c0) * 3 + q];
            const long cell = (long)(oy - g.gy0) * g.gw + (c0 - g.gx0) + q / 3;
            const long i = g.foff + k * plane + 3 * cell + q % 3;
            gws[i] = gv;
            field[i] = a ? 0.f : orig - gv;
            if (k == 0 && q % 3 == 0) omega[g.ooff + cell] = (uint8_t)(a != 0);
        }
        __syncthreads();                                            // the next sample overwrites mid
    }
}

__global__ __launch_bounds__(IP_THREADS) void membrane_paste_kernel(uint8_t* __restrict__ out, long img_bytes, const uint8_t* __restrict__ msk,
                                                                    long msk_bytes, const int* __restrict__ tab, long tab_elems,
                                                                    const int* __restrict__ grids, const float* __restrict__ gws,
                                                                    const float* __restrict__ field, long g_elems, uint8_t* __restrict__ alpha,
                                                                    int R, int K, int feather, int lds_bytes, const int* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ip_lds[];
    const int b = blockIdx.z;
    IpDesc d;
    if (!ip_load_desc(tab, tab_elems, b, img_bytes, msk_bytes, false, R, d)) return;
    const int key = ip_load_key(keys, b);
    if (key < 0) return;
    MbGrid g;
    if (!mb_load_grid(grids, b, d, K, g_elems, 0x7fffffffL, g)) return;
    const int y0 = (int)blockIdx.y * d.TB, c0 = (int)blockIdx.x * d.CW;
    if (y0 >= d.ch || c0 >= d.cw) return;
    const int y1 = min(y0 + d.TB, d.ch), rows = y1 - y0, cn = min(d.CW, d.cw - c0);
    const int F = feather + 1;
    IpTile t;
    ip_tile_make(t, ip_lds, y0, c0, rows, cn, feather);
    if ((long)t.a_bytes + t.t_bytes + t.r_bytes > lds_bytes) return;
    if (!ip_feather_tile(t, msk, d, feather, (uint32_t)key)) return;
    const uint8_t* A = t.A;
    if (alpha) ip_store_alpha(t, alpha, d, keys != nullptr);
    const int uo = (3 * cn + 6) >> 2;
    const float ff = (float)F;
    const long plane = 3L * g.gh * g.gw;
    for (int k = 0; k < K; ++k) {
        uint8_t* outk = out + (long)k * img_bytes + d.off;
        for (int e = threadIdx.x; e < rows * uo; e += IP_THREADS) {
            const int r = e / uo, u = e - r * uo, oy = y0 + r, nb = 3 * cn;
            const int gy = oy - g.gy0;
            if (gy < 0 || gy >= g.gh) continue;                     // (Omega lies inside the solve grid: nothing to blend outside it)
            uint8_t* p = outk + ((long)(d.wy0 + oy) * d.w + d.wx0 + c0) * 3;
            const int lo = 4 * u - (int)(reinterpret_cast<uintptr_t>(p) & 3);
            if (lo >= nb || lo + 4 <= 0) continue;
            const int q0 = max(lo, 0), q1 = min(lo + 4, nb);
            const uint8_t* ar = A + r * cn;
            int any = 0;
            for (int q = q0; q < q1; ++q) any |= ar[q / 3];
            if (!any) continue;
            const bool whole = q1 - q0 == 4;
            uint32_t word = 0u;
            if (whole) word = *reinterpret_cast<const uint32_t*>(p + lo);
            for (int q = q0; q < q1; ++q) {
                const int av = ar[q / 3], gx = c0 + q / 3 - g.gx0;
                if (!av || gx < 0 || gx >= g.gw) continue;
                const long i = g.foff + k * plane + 3 * ((long)gy * g.gw + gx) + q % 3;
                const float uv = fminf(fmaxf(gws[i] + field[i], 0.f), 255.f);
                const int sh = 8 * (q - lo);
                const float orig = whole ? (float)((word >> sh) & 255u) : (float)p[q];
                const uint32_t o = ip_mix(uv, (float)av, (float)(F - av), orig, ff);
                if (whole) word = (word & ~(255u << sh)) | o << sh;
                else p[q] = (uint8_t)o;
            }
            if (whole) *reinterpret_cast<uint32_t*>(p + lo) = word;
        }
    }
}

int mb_check_paste_args(const char* who, long img_bytes, long mask_bytes, long table_elems, int B, int K, int R, int feather, int chunks, int bands,
                        int lds_bytes) {
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must lie in [1, 65535] (got %d)", who, B);
    SHG_CHECK_ARG(K >= 1 && K <= 65535, "%s: K must lie in [1, 65535] (got %d)", who, K);
    SHG_CHECK_ARG(R >= 1 && R <= 16384, "%s: R must lie in [1, 16384] (got %d)", who, R);
    SHG_CHECK_ARG(feather >= 0 && feather <= IP_MAX_FEATHER, "%s: feather must lie in [0, %d] (got %d)", who, IP_MAX_FEATHER, feather);
    SHG_CHECK_ARG(img_bytes >= 3 && img_bytes <= 0x7fffffffL, "%s: img_bytes must lie in [3, 2^31) (int32 offsets)", who);
    SHG_CHECK_ARG(mask_bytes >= 1 && mask_bytes <= 0x7fffffffL, "%s: mask_bytes must lie in [1, 2^31) (int32 offsets)", who);
    SHG_CHECK_ARG(table_elems >= (long)B * IP_DESC, "%s: the table holds fewer than B descriptors of %d ints", who, IP_DESC);
    SHG_CHECK_ARG(chunks >= 1 && chunks <= 65535 && bands >= 1 && bands <= 65535, "%s: chunks and bands must lie in [1, 65535] (got %d, %d)", who,
                  chunks, bands);
    SHG_CHECK_ARG(lds_bytes >= 32 && lds_bytes <= IP_LDS_BYTES, "%s: lds_bytes must lie in [32, %d] (got %d)", who, IP_LDS_BYTES, lds_bytes);
    return SHG_OK;
}

int mb_launch_setup(const void* src, long img_bytes, const void* mask, long mask_bytes, const int* keys, const int* table, long table_elems,
                    const int* grids, const float* fake, float* g, float* field, long g_elems, void* omega, long omega_bytes, int B, int K, int R,
                    int feather, int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(src && mask && table && grids && fake && g && field && omega, "membrane_setup: null pointer");
    if (int rc = mb_check_paste_args("membrane_setup", img_bytes, mask_bytes, table_elems, B, K, R, feather, chunks, bands, lds_bytes)) return rc;
    SHG_CHECK_ARG(g_elems >= 3 && g_elems <= 0x7fffffffL && omega_bytes >= 1 && omega_bytes <= 0x7fffffffL,
                  "membrane_setup: g_elems must lie in [3, 2^31) and omega_bytes in [1, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(fake) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(field)) & 3) == 0,
                  "membrane_setup: fake, g and field must be 4-byte aligned");
    hipLaunchKernelGGL(membrane_setup_kernel, dim3(chunks, bands, B), dim3(IP_THREADS), (size_t)lds_bytes, (hipStream_t)stream, (const uint8_t*)src,
                       img_bytes, (const uint8_t*)mask, mask_bytes, table, table_elems, grids, fake, g, field, g_elems, (uint8_t*)omega, omega_bytes,
                       R, K, feather, lds_bytes, keys);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

int mb_launch_paste(void* out, long img_bytes, const void* mask, long mask_bytes, const int* keys, const int* table, long table_elems, const int* grids,
                    const float* g, const float* field, long g_elems, void* alpha, int B, int K, int R, int feather, int chunks, int bands,
                    int lds_bytes, void* stream) {
    SHG_CHECK_ARG(out && mask && table && grids && g && field, "membrane_paste: null pointer");
    if (int rc = mb_check_paste_args("membrane_paste", img_bytes, mask_bytes, table_elems, B, K, R, feather, chunks, bands, lds_bytes)) return rc;
    SHG_CHECK_ARG(g_elems >= 3 && g_elems <= 0x7fffffffL, "membrane_paste: g_elems must lie in [3, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(field)) & 3) == 0, "membrane_paste: g and field must be 4-byte aligned");
    hipLaunchKernelGGL(membrane_paste_kernel, dim3(chunks, bands, B), dim3(IP_THREADS), (size_t)lds_bytes, (hipStream_t)stream, (uint8_t*)out, img_bytes,
                       (const uint8_t*)mask, mask_bytes, table, table_elems, grids, g, field, g_elems, (uint8_t*)alpha, R, K, feather, lds_bytes, keys);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

}  // namespace

extern "C" int shg_membrane_tile(void) { return MB_TILE; }
extern "C" int shg_membrane_coarsest(void) { return MB_COARSEST; }

// bytes of the solver's workspace for P problems of at most max_h x max_w (0 when an argument is out of range)
extern "C" size_t shg_membrane_workspace_bytes(int P, int max_h, int max_w) {
    if (P < 1 || max_h < 1 || max_w < 1 || max_h > MB_MAX_SIDE || max_w > MB_MAX_SIDE) return 0;
    return (size_t)P * (size_t)mb_ws_floats(max_h, max_w) * sizeof(float);
}

// src: the packed originals; g / field: float32 [g_elems], omega: uint8 [omega_bytes], written inside the solve grids `grids` names
// (device int32 [B][6]); table, fake, chunks, bands, lds_bytes as shg_inpaint_paste_u8.
extern "C" int shg_inpaint_membrane_setup_f32(const void* src, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                              const int* grids, const float* fake, float* g, float* field, long g_elems, void* omega,
                                              long omega_bytes, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream) {
    return mb_launch_setup(src, img_bytes, mask, mask_bytes, nullptr, table, table_elems, grids, fake, g, field, g_elems, omega, omega_bytes, B, K, R,
                           feather, chunks, bands, lds_bytes, stream);
}

// out as shg_inpaint_paste_u8; g / field: what setup wrote and the solver turned into c.
extern "C" int shg_inpaint_membrane_paste_u8(void* out, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                             const int* grids, const float* g, const float* field, long g_elems, void* alpha, int B, int K, int R,
                                             int feather, int chunks, int bands, int lds_bytes, void* stream) {
    return mb_launch_paste(out, img_bytes, mask, mask_bytes, nullptr, table, table_elems, grids, g, field, g_elems, alpha, B, K, R, feather, chunks, bands,
                           lds_bytes, stream);
}

// The keyed forms (csrc/hole_label.hip; shg_inpaint_paste_keyed_u8 states the rule): `owner` stands where the mask went, window b takes
// the holes whose byte equals keys[b] (device int [B], 1..255).  Descriptors, grids and LDS budget are those of the forms above.
extern "C" int shg_inpaint_membrane_setup_keyed_f32(const void* src, long img_bytes, const void* owner, long mask_bytes, const int* keys,
                                                    const int* table, long table_elems, const int* grids, const float* fake, float* g, float* field,
                                                    long g_elems, void* omega, long omega_bytes, int B, int K, int R, int feather, int chunks,
                                                    int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(keys, "membrane_setup_keyed: null pointer");
    return mb_launch_setup(src, img_bytes, owner, mask_bytes, keys, table, table_elems, grids, fake, g, field, g_elems, omega, omega_bytes, B, K, R,
                           feather, chunks, bands, lds_bytes, stream);
}

extern "C" int shg_inpaint_membrane_paste_keyed_u8(void* out, long img_bytes, const void* owner, long mask_bytes, const int* keys, const int* table,
                                                   long table_elems, const int* grids, const float* g, const float* field, long g_elems, void* alpha,
                                                   int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(keys, "membrane_paste_keyed: null pointer");
    return mb_launch_paste(out, img_bytes, owner, mask_bytes, keys, table, table_elems, grids, g, field, g_elems, alpha, B, K, R, feather, chunks, bands,
                           lds_bytes, stream);
}

// table: device int32 [P][4] = {h, w, float offset into field, byte offset into omega}, every h <= max_h and w <= max_w (a problem that
// breaks this, or points outside field / omega, is left alone with info = (0, +inf, 0)); the problems' slices of `field` must not
// overlap.  res_tol: device float32 [P].  ws: ws_bytes >= shg_membrane_workspace_bytes(P, max_h, max_w), old contents irrelevant.
// info: device int32 [P][3] = (cycles run, bits of the last residual max norm, state 1 certified / 2 stalled / 0 out of cycles).
extern "C" int shg_membrane_solve_f32(float* field, long field_elems, const void* omega, long omega_bytes, const int* table, int P,
                                      const float* res_tol, int max_cycles, int max_h, int max_w, void* ws, size_t ws_bytes, int* info, void* stream) {
    SHG_CHECK_ARG(field && omega && table && res_tol && ws && info, "membrane_solve: null pointer");
    SHG_CHECK_ARG(P >= 1 && P <= 65535, "membrane_solve: P must lie in [1, 65535] (got %d)", P);
    SHG_CHECK_ARG(max_cycles >= 0 && max_cycles <= 1024, "membrane_solve: max_cycles must lie in [0, 1024] (got %d)", max_cycles);
    SHG_CHECK_ARG(max_h >= 1 && max_h <= MB_MAX_SIDE && max_w >= 1 && max_w <= MB_MAX_SIDE, "membrane_solve: max_h and max_w must lie in [1, %d] (got %d, %d)",
                  MB_MAX_SIDE, max_h, max_w);
    SHG_CHECK_ARG(field_elems >= 3 && field_elems <= 0x7fffffffL && omega_bytes >= 1 && omega_bytes <= 0x7fffffffL,
                  "membrane_solve: field_elems must lie in [3, 2^31) and omega_bytes in [1, 2^31) (int32 offsets)");
    const long stride = mb_ws_floats(max_h, max_w);
    SHG_CHECK_ARG(ws_bytes >= (size_t)P * (size_t)stride * sizeof(float), "membrane_solve: the workspace holds %zu bytes, %zu are needed", ws_bytes,
                  (size_t)P * (size_t)stride * sizeof(float));
    SHG_CHECK_ARG(((reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0, "membrane_solve: field and the workspace must be 16-byte aligned");
    MbArgs a{field, field_elems, (const uint8_t*)omega, omega_bytes, table, (float*)ws, stride, info, res_tol, max_h, max_w};
    hipStream_t st = (hipStream_t)stream;
    const int L = mb_levels(max_h, max_w);
    int lh[32], lw[32];
    lh[0] = max_h, lw[0] = max_w;
    for (int l = 1; l < L; ++l) lh[l] = (lh[l - 1] + 1) >> 1, lw[l] = (lw[l - 1] + 1) >> 1;
    auto grid = [&](int l) { return dim3((unsigned)mb_tiles(lh[l], lw[l]), (unsigned)P); };
    hipLaunchKernelGGL(mb_init_kernel, grid(0), dim3(MB_THREADS), 0, st, a);
    for (int l = 0; l + 1 < L; ++l) hipLaunchKernelGGL(mb_coarsen_kernel, grid(l + 1), dim3(MB_THREADS), 0, st, a, l);
    for (int cyc = 0;; ++cyc) {
        hipLaunchKernelGGL(mb_norm_kernel, grid(0), dim3(MB_THREADS), 0, st, a);
        hipLaunchKernelGGL(mb_state_kernel, dim3(P), dim3(MB_THREADS), 0, st, a, cyc);
        if (cyc == max_cycles) break;
        for (int l = 0; l + 1 < L; ++l) {
            hipLaunchKernelGGL(mb_smooth_kernel, grid(l), dim3(MB_THREADS), 0, st, a, l, 0);
            hipLaunchKernelGGL(mb_restrict_kernel, grid(l + 1), dim3(MB_THREADS), 0, st, a, l);
        }
        hipLaunchKernelGGL(mb_coarsest_kernel, dim3(P), dim3(MB_THREADS), 0, st, a);
        for (int l = L - 2; l >= 0; --l) {
            hipLaunchKernelGGL(mb_prolong_kernel, grid(l), dim3(MB_THREADS), 0, st, a, l);
            hipLaunchKernelGGL(mb_smooth_kernel, grid(l), dim3(MB_THREADS), 0, st, a, l, 1);
        }
    }
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
