// Inpainting photographs of any size (sh-gan_amd/inpaint.py drives both kernels): a window of each image around its hole is resized to the
// generator's R x R input (gather_windows), and the generator's output is resampled back to the window and blended into the original bytes
// with a feathered weight (paste_back).  Images are decoded uint8 HWC RGB packed back to back (resize.pack_images), masks uint8 HW packed
// the same way (1 / non-zero = known, 0 = hole), each image with a window {y0, x0, ch, cw} that lies inside it.
//
// gather_windows.  Image: the bytes of Pillow's Image.crop(box).resize((R, R), BICUBIC) -- the integer passes of pillow_resample.h on the
// fixed-point tables of (cw -> R) and (ch -> R), the source read at the image's own row pitch from the window origin (nothing is copied
// first).  Mask: output pixel (i, j) is known iff every native pixel of rows [i ch / R, max(ceil((i + 1) ch / R), lo + 1)) x the same
// columns is known (integers; conservative: no hole pixel lies outside the low-resolution hole).  One workgroup = (image, band of TB
// output rows, chunk of CW output columns), as pillow_resample.h tiles a launch.
//
// paste_back, for a pixel p of the window, F = feather + 1:
//   d(p) = Chebyshev distance to the nearest hole pixel inside the window,  A(p) = max(0, F - d(p))              (an integer 0..F)
//   v    = separable resample of fake (R x R -> ch x cw) at p: float32 tap tables from the host (Pillow's bicubic, a = -0.5, normalised),
//          horizontal pass first (into LDS), then vertical, each a chain of fused multiply-adds in tap order starting from 0
//   g    = clamp(v * 127.5 + 127.5, 0, 255)                     (each operation rounded on its own, as composite_u8_kernel writes it)
//   out  = (uint8)(int)((A g + (F - A) orig) / F)               (truncation; A = 0 stores nothing, A = F gives (uint8)(int)g)
// `out` holds K copies of the packed originals (row k = sample k) when the launch starts; the launch covers the windows only.
// One workgroup = (image, band of TB window rows, chunk of CW window columns):
//   1. the mask tile with a halo of `feather` pixels is staged in LDS as hole flags (outside the window: not a hole).  A(p) > 0 iff a
//      hole lies within `feather` of p, so a staged tile without a hole has A = 0 everywhere: the workgroup returns on that
//      workgroup-uniform test, before anything else is read.  Most of a window is such tiles.
//   2. row pass (distance to the nearest hole in the row, capped at F), column pass (min over dy of max(|dy|, rowdist)) -> A, bytes in LDS;
//   3. per sample k: the band's rows of fake are resampled horizontally into float LDS (pixel-interleaved, [row][3 col + channel], which
//      is the byte order of the HWC destination), then one lane = one aligned 4-byte word of a destination row: the vertical pass of its
//      four bytes, the blend with the word read from `out`, one 4-byte store (bytes at the ragged ends of the chunk's row and where the
//      word would cross them).  A word belongs to one lane of one workgroup, and a word whose four A are 0 is not stored.
// Dynamic LDS only, every carve 16-byte aligned; the staging of step 3 reuses the bytes of steps 1-2.  No atomics, no inter-workgroup
// communication: an image's bytes do not depend on its neighbours in the batch or on the run.
//
// table (int32; the float32 weights of paste_back travel as their bit patterns): B descriptors of IP_DESC ints {h, w, image byte offset,
// mask byte offset, y0, x0, ch, cw, h-bounds, h-coefs, KH, v-bounds, v-coefs, KV, TB, CW}, then per axis bounds [n][2] = (first tap, taps)
// and coefficients [n][K] at the offsets the descriptors name (n = R for gather_windows, cw / ch for paste_back).  The kernels check every
// descriptor and tap range against the buffer sizes they are given: a malformed table leaves bytes unwritten, it never reads or writes
// out of bounds.
#include "inpaint_common.h"

namespace {

static_assert(IP_THREADS == PIL_THREADS, "gather_windows runs pil_resample_tile on its own block size");

__global__ __launch_bounds__(IP_THREADS) void gather_windows_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                    const uint8_t* __restrict__ msk, long msk_bytes,
                                                                    const int* __restrict__ tab, long tab_elems, uint8_t* __restrict__ dst,
                                                                    float* __restrict__ mdst, int R, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ip_lds[];
    const int b = blockIdx.z;
    IpDesc d;
    if (!ip_load_desc(tab, tab_elems, b, src_bytes, msk_bytes, true, R, d)) return;
    const int y0 = (int)blockIdx.y * d.TB, c0 = (int)blockIdx.x * d.CW;
    if (y0 >= R || c0 >= R) return;
    const int y1 = min(y0 + d.TB, R), rows = y1 - y0, cn = min(d.CW, R - c0);

    // image: the window, read at the image's row pitch from the window origin
    const long pitch = (long)d.w * 3;
    const uint8_t* win = src + d.off + (long)d.wy0 * pitch + (long)d.wx0 * 3;
    if (!pil_resample_tile<false>(ip_lds, lds_bytes, tab, {d.hb, d.hk, d.KH}, {d.vb, d.vk, d.KV}, win, pitch, d.ch, d.cw, y0, y1, c0, cn,
                                  dst + (long)b * 3 * R * R, R, 0, R, R))
        return;

    // mask: one lane = one output pixel, known iff its whole native footprint is known
    const uint8_t* mwin = msk + d.moff + (long)d.wy0 * d.w + d.wx0;
    for (int e = threadIdx.x; e < rows * cn; e += IP_THREADS) {
        const int t = e / cn, oy = y0 + t, ox = c0 + (e - t * cn);
        const int rlo = (int)((long)oy * d.ch / R), rhi = max((int)(((long)(oy + 1) * d.ch + R - 1) / R), rlo + 1);
        const int clo = (int)((long)ox * d.cw / R), chi = max((int)(((long)(ox + 1) * d.cw + R - 1) / R), clo + 1);
        bool known = true;
        for (int y = rlo; y < rhi; ++y) {
            const uint8_t* mr = mwin + (long)y * d.w;
            for (int x = clo; x < chi; ++x) known = known && mr[x] != 0;
        }
        mdst[((long)b * R + oy) * R + ox] = known ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(IP_THREADS) void paste_back_kernel(uint8_t* __restrict__ out, long img_bytes, const uint8_t* __restrict__ msk,
                                                                long msk_bytes, const int* __restrict__ tab, long tab_elems,
                                                                const float* __restrict__ fake, uint8_t* __restrict__ alpha, int R, int K,
                                                                int feather, int lds_bytes, const int* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ip_lds[];
    const int b = blockIdx.z;
    IpDesc d;
    if (!ip_load_desc(tab, tab_elems, b, img_bytes, msk_bytes, false, R, d)) return;
    const int key = ip_load_key(keys, b);
    if (key < 0) return;
    const int y0 = (int)blockIdx.y * d.TB, c0 = (int)blockIdx.x * d.CW;
    if (y0 >= d.ch || c0 >= d.cw) return;
    const int y1 = min(y0 + d.TB, d.ch), rows = y1 - y0, cn = min(d.CW, d.cw - c0);
    const int F = feather + 1;
    const int sy0 = max(tab[d.vb + 2 * y0], 0);
    const int sy1 = (int)min((long)tab[d.vb + 2 * (y1 - 1)] + tab[d.vb + 2 * (y1 - 1) + 1], (long)R);
    const int span = sy1 - sy0;                                     // rows of fake under the band
    IpTile t;
    ip_tile_make(t, ip_lds, y0, c0, rows, cn, feather);
    if (span < 1 || (long)t.a_bytes + max((long)t.t_bytes + t.r_bytes, 12L * span * cn) > lds_bytes) return;
    // 1.-2. the feather weight; a tile without a hole within `feather` has A = 0 everywhere: nothing to store
    if (!ip_feather_tile(t, msk, d, feather, (uint32_t)key)) return;
    const uint8_t* A = t.A;
    float* mid = t.mid;

    const int uo = (3 * cn + 6) >> 2;                               // aligned words a destination row of the chunk can touch
    if (alpha) ip_store_alpha(t, alpha, d, keys != nullptr);

    // 3. per sample: horizontal pass into LDS, then vertical pass + blend, one lane per destination word
    const long RR = (long)R * R;
    const float ff = (float)F;
    for (int k = 0; k < K; ++k) {
        const float* fk = fake + ((long)b * K + k) * 3 * RR;
        ip_resample_rows(t, tab, d, fk, R, sy0, span);
        __syncthreads();
        uint8_t* outk = out + (long)k * img_bytes + d.off;
        for (int e = threadIdx.x; e < rows * uo; e += IP_THREADS) {
            const int r = e / uo, u = e - r * uo, oy = y0 + r, nb = 3 * cn;
            const int rel = tab[d.vb + 2 * oy] - sy0, n = tab[d.vb + 2 * oy + 1];
            if (rel < 0 || n < 0 || n > d.KV || (long)rel + n > span) continue;
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
            const int* wk = tab + d.vk + (long)oy * d.KV;
            const float* m = mid + (long)rel * nb;
            for (int q = q0; q < q1; ++q) {
                const int a = ar[q / 3];
                if (!a) continue;
                const float v = ip_resample_col(wk, m, n, nb, q);
                const int sh = 8 * (q - lo);
                const float orig = whole ? (float)((word >> sh) & 255u) : (float)p[q];
                const uint32_t o = ip_mix(ip_scale(v), (float)a, (float)(F - a), orig, ff);
                if (whole) word = (word & ~(255u << sh)) | o << sh;
                else p[q] = (uint8_t)o;
            }
            if (whole) *reinterpret_cast<uint32_t*>(p + lo) = word;
        }
        __syncthreads();                                            // the next sample overwrites mid
    }
}

int ip_launch_paste(void* out, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems, const float* fake, void* alpha,
                    const int* keys, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(out && mask && table && fake, "inpaint_paste: null pointer");
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "inpaint_paste: B must lie in [1, 65535] (got %d)", B);
    SHG_CHECK_ARG(K >= 1 && K <= 65535, "inpaint_paste: K must lie in [1, 65535] (got %d)", K);
    SHG_CHECK_ARG(R >= 1 && R <= 16384, "inpaint_paste: R must lie in [1, 16384] (got %d)", R);
    SHG_CHECK_ARG(feather >= 0 && feather <= IP_MAX_FEATHER, "inpaint_paste: feather must lie in [0, %d] (got %d)", IP_MAX_FEATHER, feather);
    SHG_CHECK_ARG(img_bytes >= 3 && img_bytes <= 0x7fffffffL, "inpaint_paste: img_bytes must lie in [3, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(mask_bytes >= 1 && mask_bytes <= 0x7fffffffL, "inpaint_paste: mask_bytes must lie in [1, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(table_elems >= (long)B * IP_DESC, "inpaint_paste: the table holds fewer than B descriptors of %d ints", IP_DESC);
    SHG_CHECK_ARG(chunks >= 1 && chunks <= 65535 && bands >= 1 && bands <= 65535, "inpaint_paste: chunks and bands must lie in [1, 65535] (got %d, %d)",
                  chunks, bands);
    SHG_CHECK_ARG(lds_bytes >= 32 && lds_bytes <= IP_LDS_BYTES, "inpaint_paste: lds_bytes must lie in [32, %d] (got %d)", IP_LDS_BYTES, lds_bytes);
    SHG_CHECK_ARG((reinterpret_cast<uintptr_t>(fake) & 3) == 0, "inpaint_paste: fake must be 4-byte aligned");
    hipLaunchKernelGGL(paste_back_kernel, dim3(chunks, bands, B), dim3(IP_THREADS), (size_t)lds_bytes, (hipStream_t)stream, (uint8_t*)out,
                       img_bytes, (const uint8_t*)mask, mask_bytes, table, table_elems, fake, (uint8_t*)alpha, R, K, feather, lds_bytes, keys);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

}  // namespace

// gather_windows: src / mask as above, dst uint8 [B,3,R,R], mask_dst float32 [B,1,R,R] (1 = known).  table: B descriptors of 16 ints and
// the fixed-point tables of resize.py's bicubic_coeffs(cw, R) / (ch, R).  Grid chunks x bands x B; lds_bytes as shg_resize_bicubic_u8.
extern "C" int shg_inpaint_gather_u8(const void* src, long src_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                     void* dst, float* mask_dst, int B, int R, int chunks, int bands, int lds_bytes, void* stream) {
    SHG_CHECK_ARG(src && mask && table && dst && mask_dst, "inpaint_gather: null pointer");
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "inpaint_gather: B must lie in [1, 65535] (got %d)", B);
    SHG_CHECK_ARG(R >= 1 && R <= 16384, "inpaint_gather: R must lie in [1, 16384] (got %d)", R);
    SHG_CHECK_ARG(src_bytes >= 3 && src_bytes <= 0x7fffffffL, "inpaint_gather: src_bytes must lie in [3, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(mask_bytes >= 1 && mask_bytes <= 0x7fffffffL, "inpaint_gather: mask_bytes must lie in [1, 2^31) (int32 offsets)");
    SHG_CHECK_ARG(table_elems >= (long)B * IP_DESC, "inpaint_gather: the table holds fewer than B descriptors of %d ints", IP_DESC);
    SHG_CHECK_ARG(chunks >= 1 && chunks <= R && bands >= 1 && bands <= R && bands <= 65535,
                  "inpaint_gather: chunks and bands must lie in [1, R] (got %d, %d)", chunks, bands);
    SHG_CHECK_ARG(lds_bytes >= 12 && lds_bytes <= IP_LDS_BYTES, "inpaint_gather: lds_bytes must lie in [12, %d] (got %d)", IP_LDS_BYTES, lds_bytes);
    hipLaunchKernelGGL(gather_windows_kernel, dim3(chunks, bands, B), dim3(IP_THREADS), (size_t)lds_bytes, (hipStream_t)stream,
                       (const uint8_t*)src, src_bytes, (const uint8_t*)mask, mask_bytes, table, table_elems, (uint8_t*)dst, mask_dst, R, lds_bytes);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// paste_back: out uint8 [K][img_bytes], every row a copy of the packed originals on entry; fake float32 [B*K,3,R,R] (row n K + k: sample k
// of image n); alpha: NULL, or uint8 [mask_bytes] that receives A inside the windows' tiles that hold a non-zero A (the caller zeroes it
// first).  table: B descriptors of 16 ints and the float32 tables (bit patterns) of (R -> cw) / (R -> ch).  Grid chunks x bands x B.
extern "C" int shg_inpaint_paste_u8(void* out, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                    const float* fake, void* alpha, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes,
                                    void* stream) {
    return ip_launch_paste(out, img_bytes, mask, mask_bytes, table, table_elems, fake, alpha, nullptr, B, K, R, feather, chunks, bands, lds_bytes, stream);
}

// paste_back over the windows of hole groups (csrc/hole_label.hip): `owner` (uint8 [mask_bytes]: 0 = known, a group's key at its hole
// pixels) stands where the mask went and window b blends the holes whose byte equals keys[b] (device int [B], 1..255; a window with
// another value is left alone).  The rows of `table` are per window; the windows of one image may overlap.  alpha receives A only where
// A > 0, so the windows of an image fill one plane between them.
extern "C" int shg_inpaint_paste_keyed_u8(void* out, long img_bytes, const void* owner, long mask_bytes, const int* keys, const int* table,
                                          long table_elems, const float* fake, void* alpha, int B, int K, int R, int feather, int chunks, int bands,
                                          int lds_bytes, void* stream) {
    SHG_CHECK_ARG(keys, "inpaint_paste_keyed: null pointer");
    return ip_launch_paste(out, img_bytes, owner, mask_bytes, table, table_elems, fake, alpha, keys, B, K, R, feather, chunks, bands, lds_bytes, stream);
}
