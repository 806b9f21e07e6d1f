// Shared by the fp16 sources: the vector types, the launch parameters of the fp16 convolutions (conv_f16.hip: conv_f16_kernel and the
// routing) and the tile walk, epilogue exchange and launcher of the three persistent LDS-DMA kernels (conv_f16_ring.hip,
// conv_f16_upring.hip, conv_f16_down.hip).  gfx950 only.
#pragma once
#include <tuple>
#include "shg_device.h"

namespace f16 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f16x __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct ConvP {
    const _Float16* x;
    const _Float16* w;               // MFMA operand order [OB][wslots][I/16][64 lanes][8]: element = W[slot][ob*32 + (lane & 31)][c16*16 + (lane >> 5)*8 + e]
    int OB, wslots;                  // 32-channel output blocks (O rounded up), tap slots of the weight tensor
    const float* bias;               // optional [O]
    _Float16* y;
    int N, I, O, H, W;               // input tensor
    int OHt, OWt;                    // output tensor extent
    int GH, GW;                      // extent of the computed pixel grid (oy', ox')
    int tiles_x, tiles_y;
    int s_in, s_out, oy0, ox0;
    int ntaps;
    int tdy[9], tdx[9], tw[9];       // input offset of tap t (already minus the patch origin) and its weight slot
    int org_y, org_x;                // patch origin: input row of patch row 0 for grid row 0 = org_y
    int PH, PW;                      // patch extent
    int wlds_off;                    // halves: start of the staged weight slab behind the patch / output tile (WLDS kernels)
    // fused layer tail of the inference route (all optional): x * in_scale[n,i] while the patch is staged; then
    // y = A(conv * out_scale[n,o] + noise * noise_strength + bias[o]) + residual in the store pass
    const float* in_scale; const float* out_scale; const float* noise; const _Float16* residual;
    int noise_mode, act, tail;       // noise: 0 none, 1 [OH,OW], 2 [N,OH,OW]; tail: any of the epilogue operands present
    float noise_strength, alpha, gain, clamp;
};

// ---- the tile walk of the three persistent kernels (conv_f16_ring.hip, conv_f16_upring.hip, conv_f16_down.hip): one 512-thread workgroup
// per CU takes tiles blockIdx.x, blockIdx.x + gridDim.x, ... of a list ordered [sample][tile row][tile column][output-channel tile]
constexpr unsigned OOB = 0x80000000u;           // a byte offset no descriptor range admits: the DMA writes zeros for that lane, a buffer store is dropped

struct Coord { int n, ty, tx, ot; };

struct TileWalk {
    int tiles_x, tiles_y, n_ot, ntiles;
    unsigned m_ot, m_tx, m_ty;       // floor((2^32 - 1) / divisor) of the tile decode (shg_fastdiv)
};

__device__ __forceinline__ Coord tile_decode(int tile, const TileWalk w) {
    Coord c;
    unsigned r, t = shg_fastdiv((unsigned)tile, (unsigned)w.n_ot, w.m_ot, r);
    c.ot = (int)r;
    t = shg_fastdiv(t, (unsigned)w.tiles_x, w.m_tx, r);
    c.tx = (int)r;
    c.n = (int)shg_fastdiv(t, (unsigned)w.tiles_y, w.m_ty, r);
    c.ty = (int)r;
    return c;
}

// Epilogue of the persistent kernels.  C/D layout of v_mfma_f32_32x32x16: lanes 0-31 hold channels 8g .. 8g+3 of group g, lanes 32-63
// channels 8g+4 .. 8g+7.  a / b = a lane's four halves of groups 2 gp / 2 gp + 1: after the half exchange the lower lanes own the 16 bytes
// (8 channels) of group 2 gp, the upper lanes those of group 2 gp + 1 -- one 16-byte store per lane.
__device__ __forceinline__ u32x4 lane_exchange(u32x2 a, u32x2 b) {
    auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
    auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
    u32x4 v;
    v[0] = r0[0]; v[1] = r1[0]; v[2] = r0[1]; v[3] = r1[1];
    return v;
}

// the kernels form byte offsets inside one sample's input / output tensor in 32 bits (launches beyond that stay on the gather kernel)
inline bool offsets_fit_32bit(const ConvP& p) {
    return (long)p.H * p.W * p.I * 2 < (1L << 31) && (long)p.OHt * p.OWt * p.O * 2 < (1L << 31);
}

// Launch of a persistent kernel: min(tiles, CUs) workgroups of 512 threads with lds_bytes of dynamic LDS (the attribute that allows more than
// 64 KiB is set once per device).  fill(walk) returns the kernel's arguments as a tuple.
template <auto Kernel, class Fill>
int persistent_launch(int N, int tiles_y, int tiles_x, int n_ot, int lds_bytes, const char* what, Fill fill, hipStream_t st) {
    const long ntiles = (long)N * tiles_y * tiles_x * n_ot;
    if (ntiles > 0x7fffffffL) { shg_set_error("conv2d_f16 (%s): too many tiles", what); return SHG_ERR_ARG; }
    const TileWalk w{tiles_x, tiles_y, n_ot, (int)ntiles, 0xFFFFFFFFu / (unsigned)n_ot, 0xFFFFFFFFu / (unsigned)tiles_x, 0xFFFFFFFFu / (unsigned)tiles_y};
    const int cus = shg_cu_count();
    static ShgDeviceOnce attr_once;
    const int dev_now = shg_current_device();
    if (attr_once.pending(dev_now)) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) {
            shg_set_error("conv2d_f16 (%s): cannot reserve %d bytes of LDS", what, lds_bytes);
            return SHG_ERR_LAUNCH;
        }
        attr_once.mark(dev_now);
    }
    const unsigned grid = (unsigned)(ntiles < cus ? ntiles : cus);
    std::apply([&](const auto&... args) { hipLaunchKernelGGL(Kernel, dim3(grid), dim3(512), lds_bytes, st, args...); }, fill(w));
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// conv_f16_ring.hip: true when the persistent ring kernel serves this launch
// (span = extent of the tap offsets: 3 for a 3x3 kernel; p carries the tap table, the patch origin and the pixel grid, not yet a tiling)
bool conv_ring_eligible(const ConvP& p, int span_y, int span_x);
int conv_ring_launch(const ConvP& p, hipStream_t st);

// conv_f16_upring.hip: the stride-2 transposed 3x3 form (mode 1 of conv2d_f16_impl) with all four phases in one persistent launch
int conv_f16_routes();          // conv_f16_ring.hip: the mask of shg_conv2d_f16_set_routes
bool convt_upring_eligible(const ConvP& p);
int convt_upring_launch(const ConvP& p, int crop, hipStream_t st);

// conv_f16_down.hip: the stride-2 3x3 launches (p.s_in == 2, nine taps) on a persistent kernel; pad = the convolution's padding
bool conv_down_eligible(const ConvP& p);
int conv_down_launch(const ConvP& p, int pad, hipStream_t st);

}  // namespace f16
