// Micro-benchmark: what does a global load cost inside a stream of fp32 MFMAs on gfx950?  512 threads (2 waves / SIMD), 256 blocks.
//  mode 0: 8 MFMAs per iteration, nothing else                  mode 1: + 8 global_load_dword (64-bit VGPR address), one behind each MFMA
//  mode 2: + 8 loads with SGPR base + 32-bit VGPR offset         mode 3: + 2 global_load_dwordx4 (same bytes)
//  mode 4: + 8 ds_read_b32                                       mode 5: loads refill the A operand of the MFMA issued 2 earlier (ring)
//  mode 6: like 5, refill right behind the reader               mode 7: mode 1 with ONE wave per SIMD (256 threads)
//  mode 8: mode 1 with the accumulators in AGPRs (inline asm)   mode 9: mode 0 with the accumulators in AGPRs   mode 10: mode 4 + AGPR
//  mode 11: the 8 loads of an iteration in one burst ahead of its 8 MFMAs   mode 12: 8 MFMAs + 8 loads whose results are never used as
//  MFMA operands but land in registers (mode 1) vs. loads into ONE register (same destination, write-after-write)
//  Wave-private LDS ring for the A operands (the weight route conv_wino4 could take): a ring of two k-steps x 8 units x 256 B per wave;
//  k-step t multiplies out of registers, reads k-step t+1 from slot (t+1)&1 and copies k-step t+2 into slot t&1 by LDS-DMA.
//  mode 13: + 2 global_load_lds_dwordx4 (inline assembly, as conv_wino4's dma_piece) + 8 ds_read_b32 that refill the A operand of the MFMA
//           issued 2 earlier, behind a counted vmcnt(1): three pieces are never in flight, and the older of two is the one about to be read
//  mode 14: mode 13 with the reads paired (ds_read2st64_b32: two units of one lane lie 256 B apart; the [unit][lane] layout that a verbatim
//           16-byte copy produces gives a lane no 16 contiguous bytes, so there is no b128 form)
//  mode 15: mode 13 + the 4 B-operand ds_read_b32 of the real loop
//  `mfma_vmem ring` prints modes 0, 1, 4, 13, 14, 15 three times over.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
__global__ __launch_bounds__(512, 2) void k(const float* __restrict__ src, float* out, int iters) {
    __shared__ float lds[4096];
    __shared__ __attribute__((aligned(16))) float ring[MODE >= 13 ? 8 * 1024 : 4];       // [wave][slot][unit][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x16 acc[8];
    for (int j = 0; j < 8; ++j) for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float a[8], b = 1.0001f;
    for (int j = 0; j < 8; ++j) a[j] = lane * 0.001f + j;
    lds[threadIdx.x] = lane; lds[threadIdx.x + 512] = lane;
    __syncthreads();
    const float* pl = src + (blockIdx.x * 8 + wave) * 4096 + lane;     // per-lane 64-bit pointer
    const float* pu = src + (blockIdx.x * 8 + wave) * 4096;            // uniform base
    float sink = 0.f;
    float* rw = ring + (MODE >= 13 ? wave * 1024 : 0);
    if (MODE >= 13) {
        for (int j = 0; j < 16; ++j) rw[j * 64 + lane] = 0.f;
        __syncthreads();
    }
    auto dma = [&](const float* g, float* dst) __attribute__((always_inline)) {
        const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)dst);
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(l), "v"(g) : "m0", "memory");
    };
    for (int it = 0; it < iters; ++it) {
        const int o = (it & 7) * 512;
        float ld[8];
        f32x4 l4[2];
        if (MODE == 11) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ld[j] = pl[o + j * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (MODE >= 8 && MODE <= 10) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[j]) : "v"(a[j]), "v"(b));
            else acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b, acc[j], 0, 0, 0);
            if (MODE == 1 || MODE == 7 || MODE == 8) ld[j] = pl[o + j * 64];
            if (MODE == 2) ld[j] = pu[o + j * 64 + lane];
            if (MODE == 3 && (j & 3) == 0) l4[j >> 2] = *reinterpret_cast<const f32x4*>(pu + o + (j >> 2) * 256 + lane * 4);
            if (MODE == 4 || MODE == 10) ld[j] = lds[(lane + j * 64 + o) & 4095];
            if (MODE == 5 && j >= 2) a[j - 2] = pl[o + j * 64];
            if (MODE == 6) a[j] = pl[o + j * 64];
            if (MODE >= 13) {
                // slot it&1 was read during iteration it-1; its units 0..3 have arrived once MFMA 3 has issued, all of them once MFMA 7 has
                const float* rd = rw + ((it + 1) & 1) * 512 + lane;
                float* wr = rw + (it & 1) * 512;
                if (j == 2 || j == 6) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
                if (MODE == 14) {
                    if (j >= 2 && (j & 1) == 0) { a[j - 2] = rd[(j - 2) * 64]; a[j - 1] = rd[(j - 1) * 64]; }
                } else if (j >= 2) a[j - 2] = rd[(j - 2) * 64];
                if (MODE == 15 && (j & 1)) ld[j >> 1] = lds[(lane + j * 64 + o) & 4095];
                if (j == 3) dma(pu + o + lane * 4, wr);
                if (j == 7) dma(pu + o + 256 + lane * 4, wr + 256);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (MODE == 5) { a[6] = pl[o + 6 * 64 + 1]; a[7] = pl[o + 7 * 64 + 1]; }
        if (MODE == 1 || MODE == 2 || MODE == 4 || MODE == 7 || MODE == 8 || MODE == 10 || MODE == 11) for (int j = 0; j < 8; ++j) sink += ld[j];
        if (MODE == 3) sink += l4[0][0] + l4[1][3];
        if (MODE >= 13) { const float* rd = rw + ((it + 1) & 1) * 512 + lane; a[6] = rd[6 * 64]; a[7] = rd[7 * 64]; }
        if (MODE == 15) sink += ld[0] + ld[1] + ld[2] + ld[3];
    }
    float s = sink;
    for (int j = 0; j < 8; ++j) { s += a[j]; for (int r = 0; r < 16; ++r) s += acc[j][r]; }
    out[blockIdx.x * 512 + threadIdx.x] = s;
}

template <int MODE>
void run(const float* src, float* out, int iters) {
    const int threads = MODE == 7 ? 256 : 512;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int w = 0; w < 2; ++w) hipLaunchKernelGGL(k<MODE>, dim3(256), dim3(threads), 0, 0, src, out, iters);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(256), dim3(threads), 0, 0, src, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double mf = (double)iters * 8 * (threads / 64) / 4;     // MFMAs per SIMD
    printf("mode %d: %.3f ms  %.1f ns per MFMA per SIMD (64 cycles = %.1f ns at 2.4 GHz)\n", MODE, ms, ms * 1e6 / mf, 64 / 2.4);
}
int main(int argc, char** argv) {
    float *src, *out;
    hipMalloc(&src, (size_t)256 * 8 * 4096 * 4 + 65536); hipMemset(src, 0, (size_t)256 * 8 * 4096 * 4 + 65536);
    hipMalloc(&out, 256 * 512 * 4);
    const int iters = 50000;
    if (argc > 1 && argv[1][0] == 'r') {
        for (int rep = 0; rep < 3; ++rep) {
            run<0>(src, out, iters); run<1>(src, out, iters); run<4>(src, out, iters);
            run<13>(src, out, iters); run<14>(src, out, iters); run<15>(src, out, iters);
        }
        return 0;
    }
    run<0>(src, out, iters); run<1>(src, out, iters); run<2>(src, out, iters); run<3>(src, out, iters);
    run<4>(src, out, iters); run<5>(src, out, iters); run<6>(src, out, iters); run<7>(src, out, iters);
    run<8>(src, out, iters); run<9>(src, out, iters); run<10>(src, out, iters); run<11>(src, out, iters);
    run<13>(src, out, iters); run<14>(src, out, iters); run<15>(src, out, iters);
    return 0;
}
