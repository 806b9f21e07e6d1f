// The "random scale, random crop" training formatter on the device (AdvInpaintingFormatter, lib/data_factory/ds_places2.py:183-207 and
// ds_openimages.py:117-141; InpaintingFormatter, ds_texture.py:121-149): per image the s x s window [ch:ch+s, cw:cw+s] of
//   F.interpolate((ToTensor(img) - 0.5) * 2, size=[nh, nw], mode='bicubic', align_corners=False)
// with the texture formatter's vertical / horizontal flips of the window, uint8 in, float32 [B,3,s,s] out, one launch for a ragged batch.
// Only window pixels are computed: the nh x nw image never exists.
//
// Arithmetic (torch's upsample_bicubic2d, not antialiased), per axis in float32:
//   scale = float(in) / float(out);  src = scale * (dst + 0.5) - 0.5 (not clamped below zero);  i0 = floor(src), t = src - i0;
//   weights = cubic convolution, A = -0.75, at t+1, t, 1-t, 2-t;  taps i0-1 .. i0+2, each clamped to [0, in-1].
// Always 4 x 4 taps, also when the image shrinks (the reference point-samples there).  A sample's value is lut[byte] (256 floats: the
// reference's float32 byte / 255, then (v - 0.5) * 2).  Each of the four tap rows is summed along x first, then the four row sums along y,
// with explicit multiply / fma steps: the order is the same on both paths below, so they give the same bits, and nh = h, nw = w (t = 0,
// weights 0, 1, 0, 0) returns the table values themselves.
//
// One workgroup = one (image, tile of RC_TH window rows x RC_TW window columns).  The tile's column and row parameters (first tap,
// four weights) are computed once into LDS.  Then
//   * staged path (the tile's source rows number at most RC_ROWS: in/out up to about 2.7): every source row the tile touches is summed
//     along x for the tile's columns into LDS (float [3][rows][RC_TW]), once -- neighbouring window rows share three of their four tap
//     rows when the image grows -- and the vertical pass reads four LDS rows per output, four columns per lane, one 16-byte store;
//   * direct path (stronger shrinking: the tap rows of neighbouring window rows are disjoint, nothing to share): every output gathers its
//     16 taps through the vector cache.
// The choice depends on the image's own descriptor and tile only.  Source bytes are read one at a time (packed HWC images start at any byte
// offset and their rows are 3 w bytes long: nothing is aligned).  No atomics, no communication between workgroups: an image's window has
// the same bits alone and inside any batch.
//
// desc (int32 [B][9]): h, w, byte offset of the image in src, nh, nw, ch, cw, flip_v, flip_h.  Ragged layout: HWC bytes at the offset;
// planar layout: three h x w planes at the offset (a uint8 [B,3,H,W] tensor: offset = b * 3 * H * W).  The host copy is checked by the entry
// points before the launch; the kernel checks the device copy again and leaves an image with a bad descriptor unwritten -- every tap index
// is clamped into the image, so there is no out-of-bounds access either way.
#include "shg_common.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_TH = 16;                // window rows of a tile
constexpr int RC_TW = 64;                // window columns of a tile
constexpr int RC_ROWS = 48;              // source rows the staged path holds: 3 * 48 * 64 floats = 36 KiB
constexpr int RC_DESC = 9;               // resize.py RANDCROP_DESC_INTS
constexpr int RC_MAX_S = 16384;
constexpr int RC_MAX_N = 1 << 20;        // nh, nw: dst + 0.5 stays exact in float32 far beyond

struct RcAxis {                          // one window row or column: first of its four taps (unclamped) and the weights
    int i0;
    float w[4];
};

// torch's area_pixel_compute_source_index (cubic) and get_cubic_upsample_coefficients.  Contraction is off: every step rounds on its own, as
// written, so that the coordinate is the float32 value the reference computes
__device__ __forceinline__ RcAxis rc_axis(int n_in, int n_out, int dst) {
#pragma clang fp contract(off)
    const float scale = (float)n_in / (float)n_out;
    const float src = scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const float t = src - fl;
    const float A = -0.75f;
    RcAxis a;
    a.i0 = (int)fl - 1;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    a.w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    a.w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    a.w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    a.w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
    return a;
}

__device__ __forceinline__ int rc_clamp(int i, int n) { return min(max(i, 0), n - 1); }

// sum along x of one source row's four taps, three channels
template <bool PLANAR>
__device__ __forceinline__ void rc_hsum(const uint8_t* __restrict__ img, const float* __restrict__ lut, int h, int w, int y, const RcAxis& cx,
                                        float& r0, float& r1, float& r2) {
    const long plane = PLANAR ? (long)h * w : 1L, step = PLANAR ? 1L : 3L;
    const uint8_t* row = img + (long)y * w * step;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = row + (long)rc_clamp(cx.i0 + j, w) * step;
        const float v0 = lut[p[0]], v1 = lut[p[plane]], v2 = lut[p[2 * plane]];
        if (j == 0) {
            s0 = cx.w[0] * v0, s1 = cx.w[0] * v1, s2 = cx.w[0] * v2;
        } else {
            s0 = __builtin_fmaf(cx.w[j], v0, s0), s1 = __builtin_fmaf(cx.w[j], v1, s1), s2 = __builtin_fmaf(cx.w[j], v2, s2);
        }
    }
    r0 = s0, r1 = s1, r2 = s2;
}

__device__ __forceinline__ float rc_vsum(const float* w, float a0, float a1, float a2, float a3) {
    return __builtin_fmaf(w[3], a3, __builtin_fmaf(w[2], a2, __builtin_fmaf(w[1], a1, w[0] * a0)));
}

template <bool PLANAR>
__global__ __launch_bounds__(RC_THREADS) void randcrop_bicubic_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                      const int* __restrict__ desc, const float* __restrict__ lut,
                                                                      float* __restrict__ dst, int s) {
    __shared__ __attribute__((aligned(16))) float hs[3][RC_ROWS][RC_TW];
    __shared__ RcAxis colp[RC_TW];
    __shared__ RcAxis rowp[RC_TH];
    const int b = blockIdx.z;
    const int* d = desc + (long)b * RC_DESC;
    const int h = d[0], w = d[1], off = d[2], nh = d[3], nw = d[4], ch = d[5], cw = d[6], fv = d[7], fh = d[8];
    if (h < 1 || w < 1 || off < 0 || (long)off + 3L * h * w > src_bytes) return;
    if (nh < s || nw < s || nh > RC_MAX_N || nw > RC_MAX_N || ch < 0 || cw < 0 || ch > nh - s || cw > nw - s) return;
    const int y0 = (int)blockIdx.y * RC_TH, x0 = (int)blockIdx.x * RC_TW;       // tile origin in the (unflipped) window
    if (y0 >= s || x0 >= s) return;
    const int rows = min(RC_TH, s - y0), cols = min(RC_TW, s - x0);
    const uint8_t* img = src + off;
    const int tid = threadIdx.x;

    if (tid < RC_TW) {
        colp[tid] = rc_axis(w, nw, cw + x0 + min(tid, cols - 1));
    } else if (tid < RC_TW + RC_TH) {
        const int r = tid - RC_TW;
        rowp[r] = rc_axis(h, nh, ch + y0 + min(r, rows - 1));
    }
    __syncthreads();

    // source rows of the tile: the coordinate is monotonic in dst, so the first and last window rows bound them
    const int sy0 = rc_clamp(rowp[0].i0, h), sy1 = rc_clamp(rowp[rows - 1].i0 + 3, h);
    const int span = sy1 - sy0 + 1;
    float* out = dst + (long)b * 3 * s * s;
    const long cs = (long)s * s;

    if (span <= RC_ROWS) {
        for (int e = tid; e < span * cols; e += RC_THREADS) {
            const int r = e / cols, c = e - r * cols;
            float a0, a1, a2;
            rc_hsum<PLANAR>(img, lut, h, w, sy0 + r, colp[c], a0, a1, a2);
            hs[0][r][c] = a0, hs[1][r][c] = a1, hs[2][r][c] = a2;
        }
        __syncthreads();
        // one lane = 4 consecutive window columns of one (channel, window row)
        const int groups = (cols + 3) >> 2;
        for (int e = tid; e < 3 * rows * groups; e += RC_THREADS) {
            const int g = e % groups, t = e / groups;
            const int r = t % rows, k = t / rows;
            const RcAxis ry = rowp[r];
            const int q0 = rc_clamp(ry.i0, h) - sy0, q1 = rc_clamp(ry.i0 + 1, h) - sy0;
            const int q2 = rc_clamp(ry.i0 + 2, h) - sy0, q3 = rc_clamp(ry.i0 + 3, h) - sy0;
            const float4 a0 = *reinterpret_cast<const float4*>(&hs[k][q0][4 * g]), a1 = *reinterpret_cast<const float4*>(&hs[k][q1][4 * g]);
            const float4 a2 = *reinterpret_cast<const float4*>(&hs[k][q2][4 * g]), a3 = *reinterpret_cast<const float4*>(&hs[k][q3][4 * g]);
            const float o[4] = {rc_vsum(ry.w, a0.x, a1.x, a2.x, a3.x), rc_vsum(ry.w, a0.y, a1.y, a2.y, a3.y),
                                rc_vsum(ry.w, a0.z, a1.z, a2.z, a3.z), rc_vsum(ry.w, a0.w, a1.w, a2.w, a3.w)};
            const int oy = fv ? s - 1 - (y0 + r) : y0 + r;
            const int c = x0 + 4 * g;                                           // first window column of the group (x0 % 4 == 0)
            float* orow = out + k * cs + (long)oy * s;
            const int nv = min(4, x0 + cols - c);
            if (nv == 4 && (s & 3) == 0) {
                const float4 v = fh ? make_float4(o[3], o[2], o[1], o[0]) : make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(orow + (fh ? s - 4 - c : c)) = v;
            } else {
                for (int q = 0; q < nv; ++q) orow[fh ? s - 1 - c - q : c + q] = o[q];
            }
        }
    } else {
        for (int e = tid; e < rows * cols; e += RC_THREADS) {
            const int r = e / cols, c = e - r * cols;
            const RcAxis ry = rowp[r];
            const RcAxis cx = colp[c];
            float a[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) rc_hsum<PLANAR>(img, lut, h, w, rc_clamp(ry.i0 + j, h), cx, a[j][0], a[j][1], a[j][2]);
            const int oy = fv ? s - 1 - (y0 + r) : y0 + r, ox = fh ? s - 1 - (x0 + c) : x0 + c;
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k * cs + (long)oy * s + ox] = rc_vsum(ry.w, a[0][k], a[1][k], a[2][k], a[3][k]);
        }
    }
}

// the checks both entry points share; desc is the HOST copy of the descriptors
int rc_check(const char* name, const void* src, long src_bytes, const int* desc, const int* desc_dev, const float* lut, const float* dst,
             int B, int s) {
    SHG_CHECK_ARG(src && desc && desc_dev && lut && dst, "%s: null pointer", name);
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must lie in [1, 65535] (got %d)", name, B);
    SHG_CHECK_ARG(s >= 1 && s <= RC_MAX_S, "%s: s must lie in [1, %d] (got %d)", name, RC_MAX_S, s);
    SHG_CHECK_ARG(src_bytes >= 3 && src_bytes <= 0x7fffffffL, "%s: src_bytes must lie in [3, 2^31) (int32 offsets)", name);
    for (int b = 0; b < B; ++b) {
        const int* d = desc + (long)b * RC_DESC;
        const int h = d[0], w = d[1], off = d[2], nh = d[3], nw = d[4], ch = d[5], cw = d[6];
        SHG_CHECK_ARG(h >= 1 && w >= 1, "%s: image %d: h and w must be >= 1 (got %d x %d)", name, b, h, w);
        SHG_CHECK_ARG(off >= 0 && (long)off + 3L * h * w <= src_bytes, "%s: image %d: %d x %d x 3 bytes at offset %d lie outside src", name, b,
                      h, w, off);
        SHG_CHECK_ARG(nh >= s && nw >= s, "%s: image %d: nh and nw must be >= s (got %d x %d, s = %d)", name, b, nh, nw, s);
        SHG_CHECK_ARG(nh <= RC_MAX_N && nw <= RC_MAX_N, "%s: image %d: nh and nw must be <= %d (got %d x %d)", name, b, RC_MAX_N, nh, nw);
        SHG_CHECK_ARG(ch >= 0 && cw >= 0 && ch <= nh - s && cw <= nw - s, "%s: image %d: the window [%d:%d+s, %d:%d+s] lies outside %d x %d", name,
                      b, ch, ch, cw, cw, nh, nw);
        SHG_CHECK_ARG((d[7] == 0 || d[7] == 1) && (d[8] == 0 || d[8] == 1), "%s: image %d: flip flags must be 0 or 1", name, b);
    }
    return SHG_OK;
}

template <bool PLANAR>
int rc_launch(const void* src, long src_bytes, const int* desc_dev, const float* lut, float* dst, int B, int s, void* stream) {
    const dim3 grid(shg_cdiv(s, RC_TW), shg_cdiv(s, RC_TH), B);
    hipLaunchKernelGGL(randcrop_bicubic_kernel<PLANAR>, grid, dim3(RC_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, src_bytes,
                       desc_dev, lut, dst, s);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

}  // namespace

extern "C" int shg_randcrop_bicubic_ragged_f32(const void* src, long src_bytes, const int* desc, const int* desc_dev, const float* lut,
                                               float* dst, int B, int s, void* stream) {
    const int rc = rc_check("randcrop_bicubic_ragged_f32", src, src_bytes, desc, desc_dev, lut, dst, B, s);
    return rc != SHG_OK ? rc : rc_launch<false>(src, src_bytes, desc_dev, lut, dst, B, s, stream);
}

extern "C" int shg_randcrop_bicubic_planar_f32(const void* src, long src_bytes, const int* desc, const int* desc_dev, const float* lut,
                                               float* dst, int B, int s, void* stream) {
    const int rc = rc_check("randcrop_bicubic_planar_f32", src, src_bytes, desc, desc_dev, lut, dst, B, s);
    return rc != SHG_OK ? rc : rc_launch<true>(src, src_bytes, desc_dev, lut, dst, B, s, stream);
}
