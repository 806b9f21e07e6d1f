// Ragged-batch bicubic resize of decoded uint8 RGB images to R x R (Places2's FixResolutionLoader, lib/data_factory/ds_places2.py:90-103:
// PIL Image.resize([R, R], BICUBIC)), with the formatter's horizontal flip of the resized image (FreeFormMaskFormatter, :214-229).
// src: B packed HWC images of their own sizes; dst: uint8 [B,3,R,R] (NCHW, the evaluation loop's input).
//
// Pillow's 8-bit resample is integer arithmetic on fixed-point tables (22 fractional bits) built in double precision on the host
// (resize.py) and passed in `table`; here only integers are added, so the result is Pillow's byte for byte:
//   horizontal pass  mid = clip8((1 << 21 + sum_j src[y][xmin+j] * kh[x][j]) >> 22)    (uint8, as Pillow's intermediate image)
//   vertical pass    out = clip8((1 << 21 + sum_j mid[ymin+j][x] * kv[y][j]) >> 22)
// An axis that keeps its size carries the one-tap identity table (Pillow skips that pass: the same bytes).
//
// One launch.  One workgroup = one (image, band of TB output rows, chunk of CW output columns): the band's source rows are resampled
// horizontally into LDS as three uint8 planes [rows][CW], then the vertical pass reads 4 columns per lane from LDS and writes them with
// one 4-byte store per plane row (byte stores when R % 4 != 0 or at a chunk's ragged end).  The host picks TB and CW per image so that
// the band fits lds_bytes (dynamic LDS, the batch's largest band, <= RS_LDS_BYTES).  No atomics, no inter-workgroup communication:
// deterministic, and an image's bytes do not depend on its neighbours in the batch.
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
#include "shg_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_BYTES = 49152;      // resize.py LDS_BYTES: the largest band a launch may ask for
constexpr int RS_DESC = 12;              // resize.py DESC_INTS
constexpr int RS_FIT_DESC = 14;          // resize.py FIT_DESC_INTS
constexpr int RS_BITS = 22;

__device__ __forceinline__ uint32_t rs_clip8(int s) {
    s >>= RS_BITS;
    return (uint32_t)min(max(s, 0), 255);
}

__global__ __launch_bounds__(RS_THREADS) void resize_bicubic_u8_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                       const int* __restrict__ tab, long tab_elems,
                                                                       uint8_t* __restrict__ dst, int R, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mid[];
    const int b = blockIdx.z;
    const int* d = tab + (long)b * RS_DESC;
    const int h = d[0], w = d[1], off = d[2], flip = d[3];
    const int hb = d[4], hk = d[5], KH = d[6], vb = d[7], vk = d[8], KV = d[9], TB = d[10], CW = d[11];
    if (h < 1 || w < 1 || off < 0 || (long)off + (long)h * w * 3 > src_bytes || TB < 1 || CW < 1 || KH < 1 || KV < 1) return;
    if (hb < 0 || hk < 0 || vb < 0 || vk < 0 || (long)hb + 2L * R > tab_elems || (long)hk + (long)R * KH > tab_elems ||
        (long)vb + 2L * R > tab_elems || (long)vk + (long)R * KV > tab_elems)
        return;
    const int y0 = (int)blockIdx.y * TB, c0 = (int)blockIdx.x * CW;
    if (y0 >= R || c0 >= R) return;
    const int y1 = min(y0 + TB, R), cn = min(CW, R - c0);
    const int cwp = (cn + 3) & ~3;                                  // LDS row pitch: 4-byte reads in the vertical pass
    const int sy0 = max(tab[vb + 2 * y0], 0);
    const int sy1 = (int)min((long)tab[vb + 2 * (y1 - 1)] + tab[vb + 2 * (y1 - 1) + 1], (long)h);
    const int span = sy1 - sy0;                                     // source rows of the band
    if (span < 1 || 3L * span * cwp > lds_bytes) return;

    // horizontal pass: one lane = one (source row, output column), three channels
    const uint8_t* img = src + off;
    const long pitch = (long)w * 3;
    for (int e = threadIdx.x; e < span * cn; e += RS_THREADS) {
        const int r = e / cn, c = e - r * cn, x = c0 + c;
        int xmin = tab[hb + 2 * x], n = tab[hb + 2 * x + 1];
        if (xmin < 0 || n < 0 || n > KH || (long)xmin + n > w) xmin = 0, n = 0;
        const uint8_t* p = img + (long)(sy0 + r) * pitch + xmin * 3;
        const int* k = tab + hk + (long)x * KH;
        int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
        for (int j = 0; j < n; ++j) {
            const int kj = k[j];
            s0 += (int)p[3 * j] * kj;
            s1 += (int)p[3 * j + 1] * kj;
            s2 += (int)p[3 * j + 2] * kj;
        }
        mid[(0 * span + r) * cwp + c] = (uint8_t)rs_clip8(s0);
        mid[(1 * span + r) * cwp + c] = (uint8_t)rs_clip8(s1);
        mid[(2 * span + r) * cwp + c] = (uint8_t)rs_clip8(s2);
    }
    __syncthreads();

    // vertical pass: one lane = 4 consecutive output columns of one (channel, output row)
    const int groups = cwp >> 2, rows = y1 - y0;
    for (int e = threadIdx.x; e < 3 * rows * groups; e += RS_THREADS) {
        const int g = e % groups, t = e / groups;
        const int oy = y0 + t % rows, ch = t / rows;
        int rel = tab[vb + 2 * oy] - sy0, n = tab[vb + 2 * oy + 1];
        if (rel < 0 || n < 0 || n > KV || (long)rel + n > span) rel = 0, n = 0;
        const uint8_t* m = mid + (ch * span + rel) * cwp + 4 * g;
        const int* k = tab + vk + (long)oy * KV;
        int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < n; ++j) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(m + j * cwp);
            const int kj = k[j];
            a0 += (int)(v & 255u) * kj;
            a1 += (int)((v >> 8) & 255u) * kj;
            a2 += (int)((v >> 16) & 255u) * kj;
            a3 += (int)(v >> 24) * kj;
        }
        const uint32_t o0 = rs_clip8(a0), o1 = rs_clip8(a1), o2 = rs_clip8(a2), o3 = rs_clip8(a3);
        const int c = c0 + 4 * g;                                   // first output column of the group (c0 % 4 == 0 on the host's tiling)
        uint8_t* orow = dst + (((long)b * 3 + ch) * R + oy) * R;
        const int nv = min(4, c0 + cn - c);
        if (nv == 4 && (R & 3) == 0 && (c & 3) == 0) {
            const uint32_t word = flip ? (o3 | o2 << 8 | o1 << 16 | o0 << 24) : (o0 | o1 << 8 | o2 << 16 | o3 << 24);
            *reinterpret_cast<uint32_t*>(orow + (flip ? R - 4 - c : c)) = word;
        } else {
            const uint32_t o[4] = {o0, o1, o2, o3};
            for (int q = 0; q < nv; ++q) orow[flip ? R - 1 - c - q : c + q] = (uint8_t)o[q];
        }
    }
}

// One workgroup = one (image, band of TB canvas rows, chunk of CW canvas columns).  The part of the tile inside the image's box is
// resampled as above; rows at or below h' take no taps (sum 1 << 21 -> 0), columns at or right of w' are stored as 0.
__global__ __launch_bounds__(RS_THREADS) void resize_fit_pad_u8_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                       const int* __restrict__ tab, long tab_elems,
                                                                       uint8_t* __restrict__ dst, int R, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mid[];
    const int b = blockIdx.z;
    const int* d = tab + (long)b * RS_FIT_DESC;
    const int h = d[0], w = d[1], off = d[2], flip = d[3];
    const int hb = d[4], hk = d[5], KH = d[6], vb = d[7], vk = d[8], KV = d[9], TB = d[10], CW = d[11], oh = d[12], ow = d[13];
    if (h < 1 || w < 1 || off < 0 || (long)off + (long)h * w * 3 > src_bytes || TB < 1 || CW < 1 || KH < 1 || KV < 1) return;
    if (oh < 1 || oh > R || ow < 1 || ow > R) return;
    if (hb < 0 || hk < 0 || vb < 0 || vk < 0 || (long)hb + 2L * ow > tab_elems || (long)hk + (long)ow * KH > tab_elems ||
        (long)vb + 2L * oh > tab_elems || (long)vk + (long)oh * KV > tab_elems)
        return;
    const int y0 = (int)blockIdx.y * TB, c0 = (int)blockIdx.x * CW;
    if (y0 >= R || c0 >= R) return;
    const int y1 = min(y0 + TB, R), cn = min(CW, R - c0);
    const int cwp = (cn + 3) & ~3;                                  // LDS row pitch: 4-byte reads in the vertical pass
    const int cc = min(c0 + cn, ow) - c0;                           // columns of the tile inside the box (<= 0: none)
    const bool inside = y0 < oh && cc > 0;                          // workgroup-uniform
    int sy0 = 0, span = 0;
    if (inside) {
        const int yl = min(y1, oh) - 1;                             // last box row of the band
        sy0 = max(tab[vb + 2 * y0], 0);
        const int sy1 = (int)min((long)tab[vb + 2 * yl] + tab[vb + 2 * yl + 1], (long)h);
        span = sy1 - sy0;
        if (span < 1 || 3L * span * cwp > lds_bytes) return;

        const uint8_t* img = src + off;
        const long pitch = (long)w * 3;
        for (int e = threadIdx.x; e < span * cc; e += RS_THREADS) {
            const int r = e / cc, c = e - r * cc, x = c0 + c;
            int xmin = tab[hb + 2 * x], n = tab[hb + 2 * x + 1];
            if (xmin < 0 || n < 0 || n > KH || (long)xmin + n > w) xmin = 0, n = 0;
            const uint8_t* p = img + (long)(sy0 + r) * pitch + xmin * 3;
            const int* k = tab + hk + (long)x * KH;
            int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                s0 += (int)p[3 * j] * kj;
                s1 += (int)p[3 * j + 1] * kj;
                s2 += (int)p[3 * j + 2] * kj;
            }
            mid[(0 * span + r) * cwp + c] = (uint8_t)rs_clip8(s0);
            mid[(1 * span + r) * cwp + c] = (uint8_t)rs_clip8(s1);
            mid[(2 * span + r) * cwp + c] = (uint8_t)rs_clip8(s2);
        }
        __syncthreads();
    }

    const int groups = cwp >> 2, rows = y1 - y0;
    for (int e = threadIdx.x; e < 3 * rows * groups; e += RS_THREADS) {
        const int g = e % groups, t = e / groups;
        const int oy = y0 + t % rows, ch = t / rows;
        int rel = 0, n = 0;
        const int* k = tab;
        if (inside && oy < oh) {
            rel = tab[vb + 2 * oy] - sy0, n = tab[vb + 2 * oy + 1];
            if (rel < 0 || n < 0 || n > KV || (long)rel + n > span) rel = 0, n = 0;
            k = tab + vk + (long)oy * KV;
        }
        const uint8_t* m = mid + (ch * span + rel) * cwp + 4 * g;
        int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < n; ++j) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(m + j * cwp);
            const int kj = k[j];
            a0 += (int)(v & 255u) * kj;
            a1 += (int)((v >> 8) & 255u) * kj;
            a2 += (int)((v >> 16) & 255u) * kj;
            a3 += (int)(v >> 24) * kj;
        }
        const int c = c0 + 4 * g;                                   // first canvas column of the group
        const uint32_t o0 = c < ow ? rs_clip8(a0) : 0u, o1 = c + 1 < ow ? rs_clip8(a1) : 0u;
        const uint32_t o2 = c + 2 < ow ? rs_clip8(a2) : 0u, o3 = c + 3 < ow ? rs_clip8(a3) : 0u;
        uint8_t* orow = dst + (((long)b * 3 + ch) * R + oy) * R;
        const int nv = min(4, c0 + cn - c);
        if (nv == 4 && (R & 3) == 0 && (c & 3) == 0) {
            const uint32_t word = flip ? (o3 | o2 << 8 | o1 << 16 | o0 << 24) : (o0 | o1 << 8 | o2 << 16 | o3 << 24);
            *reinterpret_cast<uint32_t*>(orow + (flip ? R - 4 - c : c)) = word;
        } else {
            const uint32_t o[4] = {o0, o1, o2, o3};
            for (int q = 0; q < nv; ++q) orow[flip ? R - 1 - c - q : c + q] = (uint8_t)o[q];
        }
    }
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
    hipLaunchKernelGGL(resize_bicubic_u8_kernel, dim3(chunks, bands, B), dim3(RS_THREADS), (size_t)lds_bytes, (hipStream_t)stream,
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
    hipLaunchKernelGGL(resize_fit_pad_u8_kernel, dim3(chunks, bands, B), dim3(RS_THREADS), (size_t)lds_bytes, (hipStream_t)stream,
                       (const uint8_t*)src, src_bytes, table, table_elems, (uint8_t*)dst, R, lds_bytes);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
