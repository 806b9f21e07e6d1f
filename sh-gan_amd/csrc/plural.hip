// Pluralistic sampling (K completions of one masked input; model_zoo/comodgan.py Generator.sample_many): the two passes that turn a batch
// of N inputs into N*K synthesis rows and back into images.
//
// shg_plural_expand: the encoder ran once on N inputs; the synthesis network runs on N*K rows and reads its skip features and x_global per
//   row.  One launch writes dst[n*K + k] = src[n] for every level of the pyramid: a table in DEVICE memory holds (src, dst,
//   bytes_per_image) per level, blockIdx.y is the level, blockIdx.x walks the level's N images in a grid-stride loop.  A value is read
//   once and stored K times.  The copy knows nothing about the element type: a level moves in units of the widest of 16 / 8 / 4 / 2 / 1
//   bytes that divides its size and both of its addresses (every feature map of the network is a multiple of 16 bytes from a 16-byte
//   aligned allocation; the narrow forms are for the odd operand).  K = 1 is a plain copy.  A level with a null pointer or bytes <= 0
//   is skipped.
// shg_plural_composite_u8: shg_composite_u8 (pointwise.hip) for img [N*K,3,H,W] -- the same separately rounded float32 steps and the same
//   truncation; the mask and the known pixels of row r come from x4[r / K].
#include "shg_device.h"
#include "../../include/shgan_hip.h"

namespace {

template <typename T>
__device__ __forceinline__ void expand_units(const T* src, T* dst, long units, int N, int K, long start, long stride) {
    const long total = (long)N * units;                       // src is [N][units]: element e of it is unit e % units of image e / units
    for (long e = start; e < total; e += stride) {
        const long n = e / units, q = e - n * units;
        const T v = src[e];
        T* d = dst + n * K * units + q;
        for (int k = 0; k < K; ++k) d[(long)k * units] = v;
    }
}

__global__ __launch_bounds__(256) void plural_expand_kernel(const shg_expand_level* table, int N, int K) {
    const shg_expand_level lv = table[blockIdx.y];
    if (!lv.src || !lv.dst || lv.bytes <= 0) return;
    const long start = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const unsigned long a = (unsigned long)lv.src | (unsigned long)lv.dst | (unsigned long)lv.bytes;
    if ((a & 15) == 0) expand_units(reinterpret_cast<const uint4*>(lv.src), reinterpret_cast<uint4*>(lv.dst), lv.bytes >> 4, N, K, start, stride);
    else if ((a & 7) == 0) expand_units(reinterpret_cast<const uint2*>(lv.src), reinterpret_cast<uint2*>(lv.dst), lv.bytes >> 3, N, K, start, stride);
    else if ((a & 3) == 0) expand_units(reinterpret_cast<const uint32_t*>(lv.src), reinterpret_cast<uint32_t*>(lv.dst), lv.bytes >> 2, N, K, start, stride);
    else if ((a & 1) == 0) expand_units(reinterpret_cast<const uint16_t*>(lv.src), reinterpret_cast<uint16_t*>(lv.dst), lv.bytes >> 1, N, K, start, stride);
    else expand_units(reinterpret_cast<const uint8_t*>(lv.src), reinterpret_cast<uint8_t*>(lv.dst), lv.bytes, N, K, start, stride);
}

__global__ __launch_bounds__(256) void plural_composite_u8_kernel(const float* x4, const float* img, uint8_t* out, int HW, int K, long total4) {
    // one thread = 4 consecutive pixels of one (row, c) plane; row = n*K + k reads the mask and the known pixels of input n
    const long stride = (long)gridDim.x * 256;
    const int HW4 = HW >> 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += stride) {
        const long rc = e / HW4;
        const int p4 = (int)(e - rc * HW4) * 4;
        const long row = rc / 3;
        const int c = (int)(rc - row * 3);
        const long n = row / K;
        const float4 mk = *reinterpret_cast<const float4*>(x4 + (n * 4) * HW + p4);
        const float4 kn = *reinterpret_cast<const float4*>(x4 + (n * 4 + 1 + c) * HW + p4);
        const float4 gi = *reinterpret_cast<const float4*>(img + rc * HW + p4);
        const float m[4] = {mk.x + 0.5f, mk.y + 0.5f, mk.z + 0.5f, mk.w + 0.5f};
        const float k[4] = {kn.x, kn.y, kn.z, kn.w};
        const float g[4] = {gi.x, gi.y, gi.z, gi.w};
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // composite_u8_kernel's expression: every product and sum rounded separately (no contraction), then the truncation
#pragma clang fp contract(off)
            const float a = k[j] * m[j];
            const float b = g[j] * (1.0f - m[j]);
            float v = a + b;
            v = v * 127.5f;
            v = v + 127.5f;
            v = fminf(fmaxf(v, 0.f), 255.f);
            packed |= ((uint32_t)(uint8_t)(int)v) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(out + rc * HW + p4) = packed;
    }
}

}  // namespace

extern "C" int shg_plural_expand(const shg_expand_level* levels, int n_levels, int N, int K, long max_bytes_per_image, void* stream) {
    SHG_CHECK_ARG(levels, "plural_expand: null level table");
    SHG_CHECK_ARG(n_levels >= 1 && n_levels <= 65535 && N >= 0 && K >= 1, "plural_expand: levels %d (1..65535), N %d (>= 0), K %d (>= 1)", n_levels, N, K);
    SHG_CHECK_ARG(max_bytes_per_image >= 1, "plural_expand: max_bytes_per_image must be >= 1");
    if (N == 0) return SHG_OK;
    // the grid is sized for the largest level in 16-byte units; every level walks its images in a grid-stride loop, whatever its width
    long blocks = ((long)N * ((max_bytes_per_image + 15) / 16) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(plural_expand_kernel, dim3((unsigned)blocks, (unsigned)n_levels), dim3(256), 0, (hipStream_t)stream, levels, N, K);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

extern "C" int shg_plural_composite_u8(const float* x4, const float* img, uint8_t* out, int N, int K, int H, int W, void* stream) {
    SHG_CHECK_ARG(x4 && img && out, "plural_composite_u8: null pointer");
    SHG_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && (H * W) % 4 == 0, "plural_composite_u8: H*W must be a positive multiple of 4");
    SHG_CHECK_ARG(K >= 1, "plural_composite_u8: K must be >= 1");
    const long total4 = (long)N * K * 3 * (H * W / 4);
    if (total4 == 0) return SHG_OK;
    int grid = shg_cdiv(total4, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(plural_composite_u8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x4, img, out, H * W, K, total4);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
