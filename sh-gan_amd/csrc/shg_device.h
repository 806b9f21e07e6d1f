// Device helpers shared by the hand-scheduled kernels of libshgan_hip.so (gfx950 / CDNA4 only).  Everything here is
// __forceinline__ and takes its operands by value: these kernels are scheduled around inline assembly and sched_barriers, and a
// helper that becomes a call or gains an indirection shows up in their instruction streams.
#pragma once
#include "shg_common.h"

// Identity on a value in a VGPR that the optimiser cannot see through; it emits no instruction.  Placed on the scalars of a straight-line
// fp32 chain (an inverse Winograd transform, a layer tail) it keeps the SLP vectoriser from pairing them into v_pk_* operations: a pair
// wants its halves in adjacent registers, and in conv_wino4's epilogue the moves that arrange that outnumbered the instructions saved
// and pushed the kernel from 243 registers into scratch.
__device__ __forceinline__ void shg_opaque(float& v) { asm("" : "+v"(v)); }

// native vectors: they stay in registers (HIP's float4 struct copies may not)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Bijective XCD-aware remap (blocks b, b+8, ... share an XCD and its L2): every XCD walks a
// contiguous range of the o-tile-major work list, so its L2 holds one weight slice at a time.
__device__ __forceinline__ int shg_xcd_remap(int bid, int total) {
    const int q = total >> 3, r = total & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// buffer resource descriptor over [base, base + bytes): a byte offset outside that range makes an LDS-DMA lane deliver zeros
__device__ __forceinline__ i32x4 shg_make_srd(const void* base, unsigned bytes) {
    const unsigned long long b = (unsigned long long)base;
    i32x4 s;
    s[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    s[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    s[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    s[3] = 0x00020000;                          // raw buffer, dword data format (tools/micro/lds_dma_probe.hip pins the semantics used here)
    return s;
}

// 64 lanes x 16 bytes global -> LDS [lds_addr + 16 lane]; lanes whose voff + soff fails the range check deliver zeros.
// Deliberately WITHOUT a "memory" clobber: the callers order these loads by hand (counted vmcnt), and a clobber would make the
// compiler place its own waits around every request.  conv_wgrad_wino.hip keeps a variant of its own that has one.
__device__ __forceinline__ void shg_dma16(unsigned lds_addr, unsigned voff, i32x4 srd, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(srd), "s"(soff));
}

// n / d for wave-uniform values with a precomputed m = floor((2^32 - 1) / d): the estimate is at most one short (scalar unit: ~8 instructions
// instead of the ~40 of a runtime division -- the decode of the next tile stood between two steps' multiplies in a clock trace)
__device__ __forceinline__ unsigned shg_fastdiv(unsigned n, unsigned d, unsigned m, unsigned& rem) {
    unsigned q = __umulhi(n, m), r = n - q * d;
    if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

// The fused layer tail in its "defaults" form (absent operands passed as osc = 1, nzterm = 0, bs = 0), before the caller adds the
// residual.  Sites that go through this function compute identical bits for identical operands; conv_mfma.hip's conv_epilogue
// (conditional multiply / adds) and the polyphase kernels' tails (a different sum) are other expressions.
// The activation arrives as a ShgAct that the kernel builds ONCE from its launch parameters, outside every loop: the per-launch
// decisions (activation on / off, clamp on / off) are then constants of the tail and not branches or compares per value.
__device__ __forceinline__ float shg_conv_tail(float v, float osc, float nzterm, float bs, const ShgAct& a) {
    v = __builtin_fmaf(v, osc, nzterm) + bs;         // the fused form the contraction of `v * osc + nzterm` always took, now independent of what the vectoriser pairs up
    return shg_act_apply(v, a);
}
