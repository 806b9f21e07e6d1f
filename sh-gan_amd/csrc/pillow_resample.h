// Pillow's 8-bit bicubic resample of one workgroup tile, shared by csrc/resize.hip (Places2, OpenImages) and csrc/inpaint.hip
// (gather_windows).
//
// Pillow's 8-bit resample is integer arithmetic on fixed-point tables (22 fractional bits) built in double precision on the host
// (resize.py) and passed in `table`; here only integers are added, so the result is Pillow's byte for byte:
//   horizontal pass  mid = clip8((1 << 21 + sum_j src[y][xmin+j] * kh[x][j]) >> 22)    (uint8, as Pillow's intermediate image)
//   vertical pass    out = clip8((1 << 21 + sum_j mid[ymin+j][x] * kv[y][j]) >> 22)
// An axis that keeps its size carries the one-tap identity table (Pillow skips that pass: the same bytes).
//
// One workgroup = one (image, band of TB output rows, chunk of CW output columns): the band's source rows are resampled horizontally
// into LDS as three uint8 planes [rows][CW], then the vertical pass reads 4 columns per lane from LDS and writes them with one 4-byte
// store per plane row (byte stores when R % 4 != 0 or at a chunk's ragged end).  The host picks TB and CW per image so that the band
// fits lds_bytes (dynamic LDS, the batch's largest band).  No atomics, no inter-workgroup communication: deterministic, and an image's
// bytes do not depend on its neighbours in the batch.
//
// Per axis the table holds bounds [n][2] = (first tap, taps) and coefficients [n][K] at the offsets a descriptor names.  Every tap
// range is checked against the source extent and the staged rows: a malformed table leaves output bytes unwritten, it never reads or
// writes out of bounds.
#pragma once
#include "shg_common.h"

namespace {

constexpr int PIL_THREADS = 256;
constexpr int PRECISION_BITS = 22;

struct PilAxis {
    int bounds, coefs, K;            // table offsets of bounds [n][2] and coefficients [n][K], and K
};

// True when the tables of an axis with n output entries lie inside the table_elems ints of the table.
__device__ __forceinline__ bool pil_axis_ok(int bounds, int coefs, int K, long n, long tab_elems) {
    return K >= 1 && bounds >= 0 && coefs >= 0 && (long)bounds + 2 * n <= tab_elems && (long)coefs + n * K <= tab_elems;
}

__device__ __forceinline__ uint32_t clip8(int s) {
    s >>= PRECISION_BITS;
    return (uint32_t)min(max(s, 0), 255);
}

// Output rows [y0, y1) x columns [c0, c0 + cn) of one R x R plane triple at dst (c0 % 4 == 0 on the host's tiling), mirrored when flip
// is set, from the rows x cols HWC pixels at src (row pitch in bytes).  mid: the launch's lds_bytes of dynamic LDS.  Called by the whole
// workgroup (it holds a barrier; every return before it depends on blockIdx and table words only).  Returns false, with nothing stored,
// when the band's source rows do not fit lds_bytes.
// BOX: the canvas may be larger than the resized box (oh, ow) <= R that the tables describe.  A tile outside the box skips the horizontal
// pass, rows at or below oh take no taps (sum 1 << 21 -> 0), columns at or right of ow are stored as 0.
template <bool BOX>
__device__ __forceinline__ bool pil_resample_tile(uint8_t* mid, int lds_bytes, const int* __restrict__ tab, PilAxis H, PilAxis V,
                                                 const uint8_t* __restrict__ src, long pitch, int rows, int cols, int y0, int y1, int c0,
                                                 int cn, uint8_t* __restrict__ dst, int R, int flip, int oh, int ow) {
    const int cwp = (cn + 3) & ~3;                                  // LDS row pitch: 4-byte reads in the vertical pass
    const int cc = BOX ? min(c0 + cn, ow) - c0 : cn;                // columns of the tile inside the box (<= 0: none)
    const bool inside = !BOX || (y0 < oh && cc > 0);                // workgroup-uniform
    int sy0 = 0, span = 0;
    if (inside) {
        const int yl = (BOX ? min(y1, oh) : y1) - 1;                // last box row of the band
        sy0 = max(tab[V.bounds + 2 * y0], 0);
        const int sy1 = (int)min((long)tab[V.bounds + 2 * yl] + tab[V.bounds + 2 * yl + 1], (long)rows);
        span = sy1 - sy0;                                           // source rows of the band
        if (span < 1 || 3L * span * cwp > lds_bytes) return false;

        // horizontal pass: one lane = one (source row, output column), three channels
        for (int e = threadIdx.x; e < span * cc; e += PIL_THREADS) {
            const int r = e / cc, c = e - r * cc, x = c0 + c;
            int xmin = tab[H.bounds + 2 * x], n = tab[H.bounds + 2 * x + 1];
            if (xmin < 0 || n < 0 || n > H.K || (long)xmin + n > cols) xmin = 0, n = 0;
            const uint8_t* p = src + (long)(sy0 + r) * pitch + xmin * 3;
            const int* k = tab + H.coefs + (long)x * H.K;
            int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                s0 += (int)p[3 * j] * kj;
                s1 += (int)p[3 * j + 1] * kj;
                s2 += (int)p[3 * j + 2] * kj;
            }
            mid[(0 * span + r) * cwp + c] = (uint8_t)clip8(s0);
            mid[(1 * span + r) * cwp + c] = (uint8_t)clip8(s1);
            mid[(2 * span + r) * cwp + c] = (uint8_t)clip8(s2);
        }
        __syncthreads();
    }

    // vertical pass: one lane = 4 consecutive output columns of one (channel, output row)
    const int groups = cwp >> 2, nrow = y1 - y0;
    for (int e = threadIdx.x; e < 3 * nrow * groups; e += PIL_THREADS) {
        const int g = e % groups, t = e / groups;
        const int oy = y0 + t % nrow, ch = t / nrow;
        int rel = 0, n = 0;
        const int* k = tab;
        if (!BOX || (inside && oy < oh)) {
            rel = tab[V.bounds + 2 * oy] - sy0, n = tab[V.bounds + 2 * oy + 1];
            if (rel < 0 || n < 0 || n > V.K || (long)rel + n > span) rel = 0, n = 0;
            k = tab + V.coefs + (long)oy * V.K;
        }
        const uint8_t* m = mid + (ch * span + rel) * cwp + 4 * g;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < n; ++j) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(m + j * cwp);
            const int kj = k[j];
            a0 += (int)(v & 255u) * kj;
            a1 += (int)((v >> 8) & 255u) * kj;
            a2 += (int)((v >> 16) & 255u) * kj;
            a3 += (int)(v >> 24) * kj;
        }
        const int c = c0 + 4 * g;                                   // first output column of the group
        const uint32_t o0 = !BOX || c < ow ? clip8(a0) : 0u, o1 = !BOX || c + 1 < ow ? clip8(a1) : 0u;
        const uint32_t o2 = !BOX || c + 2 < ow ? clip8(a2) : 0u, o3 = !BOX || c + 3 < ow ? clip8(a3) : 0u;
        uint8_t* orow = dst + ((long)ch * R + oy) * R;
        const int nv = min(4, c0 + cn - c);
        if (nv == 4 && (R & 3) == 0 && (c & 3) == 0) {
            const uint32_t word = flip ? (o3 | o2 << 8 | o1 << 16 | o0 << 24) : (o0 | o1 << 8 | o2 << 16 | o3 << 24);
            *reinterpret_cast<uint32_t*>(orow + (flip ? R - 4 - c : c)) = word;
        } else {
            const uint32_t o[4] = {o0, o1, o2, o3};
            for (int q = 0; q < nv; ++q) orow[flip ? R - 1 - c - q : c + q] = (uint8_t)o[q];
        }
    }
    return true;
}

}  // namespace
