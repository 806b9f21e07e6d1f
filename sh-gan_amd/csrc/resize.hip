// Ragged-batch bicubic resize of decoded uint8 RGB images to R x R (Places2's FixResolutionLoader, lib/data_factory/ds_places2.py:90-103:
// PIL Image.resize([R, R], BICUBIC)), with the formatter's horizontal flip of the resized image (FreeFormMaskFormatter, :214-229).
// src: B packed HWC images of their own sizes; dst: uint8 [B,3,R,R] (NCHW, the evaluation loop's input).
//
// The arithmetic (Pillow's 8-bit fixed-point passes), the tiling of a launch into workgroups and its LDS use are stated in
// csrc/pillow_resample.h, which holds both passes; the kernels here read their descriptors and call it.
//
// table (int32): B descriptors of RS_DESC ints {h, w, byte offset, flip, h-bounds, h-coefs, KH, v-bounds, v-coefs, KV, TB, CW}, then
// bounds [R][2] = (first tap, taps) and coefficients [R][K] per axis at the offsets the descriptors name.  The kernel checks every
// descriptor and tap range against src_bytes / table_elems: a malformed table leaves output bytes unwritten, it never reads or writes
// out of bounds.
//
// shg_resize_fit_pad_u8 is the OpenImages variant (FixResolutionLoader, lib/data_factory/ds_openimages.py:63-81): every image is resized
// to its own box (h', w') <= R (aspect preserved; the box is the image's own size when it fits) and pasted at the top-left of a zero
// R x R canvas; the formatter's flip mirrors the whole canvas (FreeFormMaskFormatter, :148-166).  The same passes, with descriptors of
// RS_FIT_DESC ints {the 12 above, h', w'} and per-axis tables [w'][..] / [h'][..]; the grid covers the R x R canvas and the workgroups
// write the padding zeros themselves, so every byte of dst comes out of the one launch.
#include "pillow_resample.h"

namespace {

constexpr int RS_LDS_BYTES = 49152;      // resize.py LDS_BYTES: the largest band a launch may ask for
constexpr int RS_DESC = 12;              // resize.py DESC_INTS
constexpr int RS_FIT_DESC = 14;          // resize.py FIT_DESC_INTS

// One workgroup = one (image, band of TB canvas rows, chunk of CW canvas columns).  FIT: the descriptor carries the box (h', w') and the
// tables describe the box; otherwise the box is the canvas.
template <bool FIT>
__device__ __forceinline__ void rs_resize_tile(uint8_t* mid, const uint8_t* __restrict__ src, long src_bytes, const int* __restrict__ tab,
                                               long tab_elems, uint8_t* __restrict__ dst, int R, int lds_bytes) {
    const int b = blockIdx.z;
    const int* d = tab + (long)b * (FIT ? RS_FIT_DESC : RS_DESC);
    const int h = d[0], w = d[1], off = d[2], flip = d[3], TB = d[10], CW = d[11];
    const PilAxis H = {d[4], d[5], d[6]}, V = {d[7], d[8], d[9]};
    const int oh = FIT ? d[12] : R, ow = FIT ? d[13] : R;
    if (h < 1 || w < 1 || off < 0 || (long)off + (long)h * w * 3 > src_bytes || TB < 1 || CW < 1) return;
    if (oh < 1 || oh > R || ow < 1 || ow > R) return;
    if (!pil_axis_ok(H.bounds, H.coefs, H.K, ow, tab_elems) || !pil_axis_ok(V.bounds, V.coefs, V.K, oh, tab_elems)) return;
    const int y0 = (int)blockIdx.y * TB, c0 = (int)blockIdx.x * CW;
    if (y0 >= R || c0 >= R) return;
    pil_resample_tile<FIT>(mid, lds_bytes, tab, H, V, src + off, (long)w * 3, h, w, y0, min(y0 + TB, R), c0, min(CW, R - c0),
                           dst + (long)b * 3 * R * R, R, flip, oh, ow);
}

__global__ __launch_bounds__(PIL_THREADS) void resize_bicubic_u8_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                        const int* __restrict__ tab, long tab_elems,
                                                                        uint8_t* __restrict__ dst, int R, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mid[];
    rs_resize_tile<false>(mid, src, src_bytes, tab, tab_elems, dst, R, lds_bytes);
}

__global__ __launch_bounds__(PIL_THREADS) void resize_fit_pad_u8_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                        const int* __restrict__ tab, long tab_elems,
                                                                        uint8_t* __restrict__ dst, int R, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mid[];
    rs_resize_tile<true>(mid, src, src_bytes, tab, tab_elems, dst, R, lds_bytes);
}

}  // namespace

extern "C" int shg_resize_bicubic_u8(const void* src, long src_bytes, const int* table, long table_elems, void* dst, int B, int R,
                                     int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(src && table && dst, "resize_bicubic_u8: null pointer");
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "resize_bicubic_u8: B must lie in [1, 65535] (got %d)", B);
    SHG_CHECK_ARG(R >= 1 && R <= 16384, "resize_bicubic_u8: R must lie in [1, 16384] (got %d)", R);
    SHG_CHECK_ARG(src_bytes >= 3 && src_bytes <= 0x7fffffffL, "resize_bicubic_u8: src_bytes must lie in [3, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(table_elems >= (long)B * RS_DESC, "resize_bicubic_u8: the table holds fewer than B descriptors of %d ints", RS_DESC);
    SHG_CHECK_ARG(chunks >= 1 && chunks <= R && bands >= 1 && bands <= R && bands <= 65535,
                  "resize_bicubic_u8: chunks and bands must lie in [1, R] (got %d, %d)", chunks, bands);
    SHG_CHECK_ARG(lds_bytes >= 12 && lds_bytes <= RS_LDS_BYTES, "resize_bicubic_u8: lds_bytes must lie in [12, %d] (got %d)", RS_LDS_BYTES,
                  lds_bytes);
    hipLaunchKernelGGL(resize_bicubic_u8_kernel, dim3(chunks, bands, B), dim3(PIL_THREADS), (size_t)lds_bytes, (hipStream_t)stream,
                       (const uint8_t*)src, src_bytes, table, table_elems, (uint8_t*)dst, R, lds_bytes);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// The OpenImages variant: src / dst as above; table = B descriptors of 14 ints {h, w, byte offset, flip, h-bounds, h-coefs, KH, v-bounds,
// v-coefs, KV, band rows, column chunk, h', w'} and the (in, out) tables they point at (bounds [w'][2] / [h'][2], coefficients
// [w'][KH] / [h'][KV]).  dst uint8 [B,3,R,R]: the resized image at the top-left of the canvas, zeros elsewhere, the whole canvas
// mirrored when flip is set.
extern "C" int shg_resize_fit_pad_u8(const void* src, long src_bytes, const int* table, long table_elems, void* dst, int B, int R,
                                     int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(src && table && dst, "resize_fit_pad_u8: null pointer");
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "resize_fit_pad_u8: B must lie in [1, 65535] (got %d)", B);
    SHG_CHECK_ARG(R >= 1 && R <= 16384, "resize_fit_pad_u8: R must lie in [1, 16384] (got %d)", R);
    SHG_CHECK_ARG(src_bytes >= 3 && src_bytes <= 0x7fffffffL, "resize_fit_pad_u8: src_bytes must lie in [3, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(table_elems >= (long)B * RS_FIT_DESC, "resize_fit_pad_u8: the table holds fewer than B descriptors of %d ints",
                  RS_FIT_DESC);
    SHG_CHECK_ARG(chunks >= 1 && chunks <= R && bands >= 1 && bands <= R && bands <= 65535,
                  "resize_fit_pad_u8: chunks and bands must lie in [1, R] (got %d, %d)", chunks, bands);
    SHG_CHECK_ARG(lds_bytes >= 12 && lds_bytes <= RS_LDS_BYTES, "resize_fit_pad_u8: lds_bytes must lie in [12, %d] (got %d)", RS_LDS_BYTES,
                  lds_bytes);
    hipLaunchKernelGGL(resize_fit_pad_u8_kernel, dim3(chunks, bands, B), dim3(PIL_THREADS), (size_t)lds_bytes, (hipStream_t)stream,
                       (const uint8_t*)src, src_bytes, table, table_elems, (uint8_t*)dst, R, lds_bytes);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
