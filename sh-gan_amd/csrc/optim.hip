// The tail of a training iteration on the gradient buckets (sh-gan_amd/optim.py drives it):
//   shg_adam_tick         step counters and bias corrections of the touched segments, on the device (float64 arithmetic)
//   shg_adam_buckets_f32  gradient average + sanitisation + Adam over every segment of an optimiser, one launch
//   shg_adam_buckets_health_f32  the same pass (one kernel template, the same bits), which also leaves five float64 figures per chunk of
//                         what it read anyway: sum g^2, elements the sanitisation replaced, max |g|, sum p_old^2, sum (p_old - p_new)^2
//   shg_ema_lerp_f32      G_ema <- lerp(G, G_ema, beta) over the parameters and a bitwise copy of the buffers, one launch
// What they replace (lib/experiments/stylegan_default.py:159-166, :383-390): `div_` + `nan_to_num` per bucket, torch.optim.Adam, and the
// per-parameter `p_ema.copy_(p.lerp(p_ema, beta))` loop.
//
// All three are driven by a small int64 table on the device: one row per segment (= one parameter), the last column of a row being the
// first CHUNK of the segment; row `nseg` is a sentinel that holds the total number of chunks.  A chunk is OPT_CHUNK consecutive
// elements of one segment; workgroups grid-stride over the chunks and find a chunk's segment by bisection of that column (wave-uniform).
// The two stream kernels are pure HBM streams: 16-byte loads and stores, no LDS, no atomics.  The gradient, exp_avg and exp_avg_sq of a
// segment sit at the same offset of buffers laid out alike, so they share one alignment: the first (up to 3) elements up to their
// 16-byte boundary and the last (up to 3) are handled one by one by chunk 0 of the segment, the rest as float4.  The parameter is an
// allocation of its own and only 4-byte aligned RELATIVE to them: it is accessed 16 bytes at a time with 4-byte alignment, which global
// memory instructions allow (the two address LSBs are all a dwordx4 access ignores).  The EMA's source is treated the same way.
//
// The tables hold raw addresses.  They are built and range-checked on the host (optim.validate_adam_table / validate_ema_table raise
// before a launch); the kernels trust them.
#include "shg_common.h"
#include <math.h>

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_VPT = 4;                                   // float4 per lane and chunk
constexpr int OPT_CHUNK_VEC = OPT_THREADS * OPT_VPT;         // 1024 float4
static_assert(OPT_CHUNK_VEC * 4 == 4096, "optim.py CHUNK, SHG_OPT_CHUNK");
constexpr int OPT_MAX_BLOCKS = 2048;                         // 256 CUs x 8 workgroups; the rest is grid-strided
constexpr int ADAM_ROW = 10;                                 // optim.py ADAM_ROW: {p, g, m, v, numel, touched, scalar slot, group, 0, first chunk}
constexpr int EMA_ROW = 6;                                   // optim.py EMA_ROW:  {dst, src, words, kind, 0, first chunk}
constexpr int ADAM_SCALARS = 8;                              // optim.py ADAM_SCALARS: float32 per segment written by the tick
constexpr int EMA_COPY = 1;                                  // optim.py EMA_COPY (0: lerp)
constexpr int HEALTH_COLS = 5;                               // optim.py HEALTH_COLS: {sum g^2, replaced, max |g|, sum p_old^2, sum dp^2}

// The tables carry addresses as integers: the pointers made from them are given the global address space by hand (a pointer of unknown
// origin would compile to flat_* instructions).
#define OPT_GLOBAL __attribute__((address_space(1)))
typedef float fv4 __attribute__((ext_vector_type(4)));
typedef fv4 fv4u __attribute__((aligned(4)));                // 16 bytes at 4-byte alignment
typedef OPT_GLOBAL float gfloat;
typedef OPT_GLOBAL fv4 gfv4;
typedef OPT_GLOBAL fv4u gfv4u;

__device__ __forceinline__ fv4 ld4u(const gfloat* p) { return *(const gfv4u*)p; }
__device__ __forceinline__ void st4u(gfloat* p, fv4 v) { *(gfv4u*)p = v; }

// largest row whose first chunk is <= c
__device__ __forceinline__ int opt_find(const long* __restrict__ tab, int row, int nseg, long c) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(long)mid * row + row - 1] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct AdamK { float step_size, bc2, w1, b2, w2, eps; };

// bucket value -> gradient: the average over the ranks as torch's `div_` by a host scalar computes it on the device (div_mode 1: times
// the float32 reciprocal) or as a true division (div_mode 2), then nan_to_num(nan=0, posinf=1e5, neginf=-1e5)
__device__ __forceinline__ float adam_avg(float g, float world, float inv_world, int div_mode) {
    if (div_mode == 1) g = g * inv_world;
    else if (div_mode == 2) g = g / world;
    return g;
}
__device__ __forceinline__ float adam_grad(float g, float world, float inv_world, int div_mode, int sanitize) {
    g = adam_avg(g, world, inv_world, div_mode);
    if (sanitize) {
        if (g != g) g = 0.f;
        else if (g == __builtin_inff()) g = 1e5f;
        else if (g == -__builtin_inff()) g = -1e5f;
    }
    return g;
}

// The health figures of one lane over one chunk.  `raw` is the bucket value, `g` what adam_grad made of it.
struct AdamHealth {
    double g2 = 0.0, p2 = 0.0, d2 = 0.0;
    float gmax = 0.f;
    int replaced = 0;
    __device__ __forceinline__ void grad(float raw, float g, float world, float inv_world, int div_mode, int sanitize) {
        const float a = adam_avg(raw, world, inv_world, div_mode);
        replaced += (sanitize && !(fabsf(a) <= 3.402823466e38f)) ? 1 : 0;      // NaN, +-Inf, tested after the average
        g2 += (double)g * (double)g;
        gmax = fmaxf(gmax, fabsf(g));
    }
    __device__ __forceinline__ void param(float p_old, float p_new) {
        const float d = p_old - p_new;                   // in float32, as the two stored values give it
        p2 += (double)p_old * (double)p_old;
        d2 += (double)d * (double)d;
    }
};

__device__ __forceinline__ double opt_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch.optim.Adam, weight_decay = 0, amsgrad off: exp_avg.lerp_(grad, 1 - beta1) (torch's lerp: two forms around weight 0.5, so beta1 = 0
// gives exp_avg == grad exactly), exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad^2, p -= step_size * exp_avg / (sqrt(exp_avg_sq) * bc2 + eps)
//
// Every rounding is written out and contraction is off inside: which products fuse into an fma must not depend on what else the compiler
// sees around the call (the two instantiations of the stream kernel would otherwise differ in a last bit now and then).  The forms are the
// ones this kernel has always computed: everything fused except exp_avg_sq of the one-by-one elements at a segment's ends (VEC false),
// where beta2 * v is rounded before the sum.
template <bool VEC>
__device__ __forceinline__ void adam_elem(float g, float& p, float& m, float& v, const AdamK& k) {
#pragma clang fp contract(off)
    const float d = g - m;
    m = k.w1 < 0.5f ? __builtin_fmaf(k.w1, d, m) : __builtin_fmaf(-d, 1.f - k.w1, g);
    const float g2 = k.w2 * (g * g);
    v = VEC ? __builtin_fmaf(k.b2, v, g2) : k.b2 * v + g2;
    const float denom = __builtin_fmaf(sqrtf(v), k.bc2, k.eps);
    p = __builtin_fmaf(-k.step_size, m / denom, p);
}

__global__ __launch_bounds__(64) void adam_tick_kernel(const long* __restrict__ tab, int nseg, const double* __restrict__ hyper, int ngroups,
                                                       float* __restrict__ steps, float* __restrict__ scalars) {
    for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
        const long* r = tab + (long)s * ADAM_ROW;
        const long slot = r[6], grp = r[7];
        if (!r[5] || grp < 0 || grp >= ngroups) continue;
        const float t = steps[slot] + 1.f;
        steps[slot] = t;
        const double lr = hyper[4 * grp], b1 = hyper[4 * grp + 1], b2 = hyper[4 * grp + 2], eps = hyper[4 * grp + 3];
        const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
        float* o = scalars + slot * ADAM_SCALARS;
        o[0] = (float)(lr / bc1);
        o[1] = (float)(1.0 / sqrt(bc2));
        o[2] = (float)(1.0 - b1);
        o[3] = (float)b2;
        o[4] = (float)(1.0 - b2);
        o[5] = (float)eps;
    }
}

// HEALTH: the same walk and the same arithmetic on p, exp_avg and exp_avg_sq; each chunk of a touched segment also writes its row of `ws`
// [chunks][5] (float64): lane partials, a xor tree over the wave, ((w0 + w1) + (w2 + w3)) in LDS -- a shape fixed by the chunk alone.
template <bool HEALTH>
__global__ __launch_bounds__(OPT_THREADS) void adam_buckets_f32_kernel(const long* __restrict__ tab, int nseg, const float* __restrict__ scalars,
                                                                       float world, float inv_world, int div_mode, int sanitize,
                                                                       double* __restrict__ ws) {
    __shared__ double hpart[HEALTH ? 2 : 1][OPT_THREADS / 64][HEALTH_COLS];
    const long total = tab[(long)nseg * ADAM_ROW + ADAM_ROW - 1];
    const int tid = threadIdx.x;
    int trip = 0;
    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        AdamHealth hl;
        const long* r = tab + (long)opt_find(tab, ADAM_ROW, nseg, c) * ADAM_ROW;
        gfloat* p = (gfloat*)r[0];
        gfloat* g = (gfloat*)r[1];
        gfloat* m = (gfloat*)r[2];
        gfloat* v = (gfloat*)r[3];
        const long n = r[4], ci = c - r[ADAM_ROW - 1];
        const bool touched = r[5] != 0;
        const long head = min((long)(((16 - (r[1] & 15)) & 15) >> 2), n);
        const long nvec = (n - head) >> 2;
        AdamK k = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (touched) {
            const float* sc = scalars + r[6] * ADAM_SCALARS;
            k.step_size = sc[0], k.bc2 = sc[1], k.w1 = sc[2], k.b2 = sc[3], k.w2 = sc[4], k.eps = sc[5];
        }
        if (ci == 0) {                                   // the unaligned ends, one element per lane
            const long ntail = n - head - 4 * nvec;
            long e = -1;
            if (tid < head) e = tid;
            else if (tid >= 64 && tid - 64 < ntail) e = head + 4 * nvec + (tid - 64);
            if (e >= 0) {
                const float raw = g[e];
                const float ge = adam_grad(raw, world, inv_world, div_mode, sanitize);
                g[e] = ge;
                if (touched) {
                    float pe = p[e], me = m[e], ve = v[e];
                    const float p_old = pe;
                    adam_elem<false>(ge, pe, me, ve, k);
                    p[e] = pe, m[e] = me, v[e] = ve;
                    if (HEALTH) hl.grad(raw, ge, world, inv_world, div_mode, sanitize), hl.param(p_old, pe);
                }
            }
        }
        const long v0 = ci * OPT_CHUNK_VEC + tid;
        gfv4* g4 = (gfv4*)(g + head);
        gfv4* m4 = (gfv4*)(m + head);
        gfv4* v4 = (gfv4*)(v + head);
        gfloat* pb = p + head;
        // one float4 of each stream per lane and trip: the loads of a trip are independent, the occupancy (not a deep software pipeline)
        // hides HBM latency
#pragma unroll 2
        for (int j = 0; j < OPT_VPT; ++j) {
            const long vi = v0 + j * OPT_THREADS;
            if (vi >= nvec) break;
            const fv4 raw = g4[vi];
            fv4 a;
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = adam_grad(raw[q], world, inv_world, div_mode, sanitize);
            g4[vi] = a;
            if (touched) {                               // else: no gradient this step, parameter, moments and step stay as they are
                fv4 M = m4[vi], V = v4[vi], P = ld4u(pb + 4 * vi);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float pe = P[q], me = M[q], ve = V[q];
                    adam_elem<true>(a[q], pe, me, ve, k);
                    if (HEALTH) hl.grad(raw[q], a[q], world, inv_world, div_mode, sanitize), hl.param(P[q], pe);
                    P[q] = pe, M[q] = me, V[q] = ve;
                }
                m4[vi] = M, v4[vi] = V;
                st4u(pb + 4 * vi, P);
            }
        }
        if (HEALTH && touched) {                         // (uniform over the workgroup: one segment per chunk)
            double r[HEALTH_COLS] = {hl.g2, (double)hl.replaced, (double)hl.gmax, hl.p2, hl.d2};
#pragma unroll
            for (int q = 0; q < HEALTH_COLS; ++q) {
                if (q == 2) {
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) r[q] = fmax(r[q], __shfl_xor(r[q], o, 64));
                } else {
                    r[q] = opt_wave_sum(r[q]);
                }
            }
            // two LDS blocks in turn: a wave that runs ahead writes the other one, and cannot pass the next barrier before this one is read
            if ((tid & 63) == 0) {
#pragma unroll
                for (int q = 0; q < HEALTH_COLS; ++q) hpart[trip][tid >> 6][q] = r[q];
            }
            __syncthreads();
            if (tid == 0) {
                double* o = ws + c * HEALTH_COLS;
#pragma unroll
                for (int q = 0; q < HEALTH_COLS; ++q) {
                    const double w0 = hpart[trip][0][q], w1 = hpart[trip][1][q], w2 = hpart[trip][2][q], w3 = hpart[trip][3][q];
                    o[q] = q == 2 ? fmax(fmax(w0, w1), fmax(w2, w3)) : (w0 + w1) + (w2 + w3);
                }
            }
            trip ^= 1;                                   // (only where a barrier was passed)
        }
    }
}

// torch's lerp(start, end, weight) with start = the live parameter, end = the average, weight = beta
__device__ __forceinline__ float ema_elem(float avg, float live, float w) {
    const float d = avg - live;
    return w < 0.5f ? live + w * d : avg - d * (1.f - w);
}

__global__ __launch_bounds__(OPT_THREADS) void ema_lerp_f32_kernel(const long* __restrict__ tab, int nseg, const float* __restrict__ beta) {
    const long total = tab[(long)nseg * EMA_ROW + EMA_ROW - 1];
    const int tid = threadIdx.x;
    const float w = beta[0];
    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const long* r = tab + (long)opt_find(tab, EMA_ROW, nseg, c) * EMA_ROW;
        gfloat* dst = (gfloat*)r[0];
        const gfloat* src = (const gfloat*)r[1];
        const long n = r[2], ci = c - r[EMA_ROW - 1];
        const bool copy = r[3] == EMA_COPY;
        const long head = min((long)(((16 - (r[0] & 15)) & 15) >> 2), n);
        const long nvec = (n - head) >> 2;
        if (ci == 0) {
            const long ntail = n - head - 4 * nvec;
            long e = -1;
            if (tid < head) e = tid;
            else if (tid >= 64 && tid - 64 < ntail) e = head + 4 * nvec + (tid - 64);
            if (e >= 0) dst[e] = copy ? src[e] : ema_elem(dst[e], src[e], w);
        }
        const long v0 = ci * OPT_CHUNK_VEC + tid;
        gfv4* d4 = (gfv4*)(dst + head);
        const gfloat* sb = src + head;
#pragma unroll 2
        for (int j = 0; j < OPT_VPT; ++j) {
            const long vi = v0 + j * OPT_THREADS;
            if (vi >= nvec) break;
            const fv4 S = ld4u(sb + 4 * vi);
            if (copy) {                                  // words move as they are: no arithmetic touches them
                d4[vi] = S;
            } else {
                const fv4 D = d4[vi];
                fv4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = ema_elem(D[q], S[q], w);
                d4[vi] = o;
            }
        }
    }
}

}  // namespace

extern "C" int shg_adam_tick(const long* table, int nseg, const double* hyper, int ngroups, float* steps, float* scalars, void* stream) {
    SHG_CHECK_ARG(table && hyper && steps && scalars, "adam_tick: null pointer");
    SHG_CHECK_ARG(nseg >= 1 && nseg <= (1 << 20), "adam_tick: nseg must lie in [1, 2^20] (got %d)", nseg);
    SHG_CHECK_ARG(ngroups >= 1 && ngroups <= 65536, "adam_tick: ngroups must lie in [1, 65536] (got %d)", ngroups);
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, table, nseg, hyper, ngroups, steps, scalars);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// both forms of the Adam pass: one set of argument checks, one grid
template <bool HEALTH>
static int adam_buckets_launch(const char* name, const long* table, int nseg, long chunks, const float* scalars, float world, int div_mode,
                               int sanitize, double* workspace, void* stream) {
    SHG_CHECK_ARG(table && scalars && (workspace || !HEALTH), "%s: null pointer", name);
    SHG_CHECK_ARG(nseg >= 1 && nseg <= (1 << 20), "%s: nseg must lie in [1, 2^20] (got %d)", name, nseg);
    SHG_CHECK_ARG(chunks >= nseg && chunks <= (1L << 40), "%s: chunks must lie in [nseg, 2^40] (every segment has one)", name);
    SHG_CHECK_ARG(world >= 1.f && world == floorf(world) && world <= 65536.f, "%s: world must be a whole number in [1, 65536]", name);
    SHG_CHECK_ARG(div_mode >= 0 && div_mode <= 2, "%s: div_mode is 0 (none), 1 (reciprocal) or 2 (division), got %d", name, div_mode);
    const int grid = (int)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    hipLaunchKernelGGL(adam_buckets_f32_kernel<HEALTH>, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, nseg, scalars, world,
                       1.f / world, div_mode, sanitize != 0, workspace);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_adam_buckets_f32(const long* table, int nseg, long chunks, const float* scalars, float world, int div_mode, int sanitize,
                                    void* stream) {
    return adam_buckets_launch<false>("adam_buckets_f32", table, nseg, chunks, scalars, world, div_mode, sanitize, nullptr, stream);
}

extern "C" int shg_adam_buckets_health_f32(const long* table, int nseg, long chunks, const float* scalars, float world, int div_mode,
                                           int sanitize, double* workspace, void* stream) {
    return adam_buckets_launch<true>("adam_buckets_health_f32", table, nseg, chunks, scalars, world, div_mode, sanitize, workspace, stream);
}

extern "C" int shg_ema_lerp_f32(const long* table, int nseg, long chunks, const float* beta, void* stream) {
    SHG_CHECK_ARG(table && beta, "ema_lerp_f32: null pointer");
    SHG_CHECK_ARG(nseg >= 1 && nseg <= (1 << 20), "ema_lerp_f32: nseg must lie in [1, 2^20] (got %d)", nseg);
    SHG_CHECK_ARG(chunks >= nseg && chunks <= (1L << 40), "ema_lerp_f32: chunks must lie in [nseg, 2^40] (every segment has one)");
    const int grid = (int)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    hipLaunchKernelGGL(ema_lerp_f32_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, nseg, beta);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
