// Device functions shared by csrc/inpaint.hip (gather_windows, paste_back) and csrc/membrane.hip (the gradient-domain paste-back): the
// descriptor check, the feather weight of a tile, the float32 resample chain of `fake` and the blend.  Both files compute A and g through
// these functions, so the two paste-backs see the same bits.  The arithmetic is stated at the top of csrc/inpaint.hip.
#pragma once
#include "pillow_resample.h"

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_LDS_BYTES = 49152;      // inpaint.py LDS_BYTES: the most a launch may ask for
constexpr int IP_DESC = 16;              // inpaint.py DESC_INTS
constexpr int IP_MAX_FEATHER = 32;

__device__ __forceinline__ int ip_align16(int n) { return (n + 15) & ~15; }

struct IpDesc {
    int h, w, off, moff, wy0, wx0, ch, cw, hb, hk, KH, vb, vk, KV, TB, CW;
};

// The descriptor of image b, or false when anything in it points outside the buffers (n_h / n_v: entries of the horizontal / vertical table).
__device__ __forceinline__ bool ip_load_desc(const int* tab, long tab_elems, int b, long img_bytes, long msk_bytes, bool out_is_r, int R, IpDesc& d) {
    const int* p = tab + (long)b * IP_DESC;
    d.h = p[0], d.w = p[1], d.off = p[2], d.moff = p[3], d.wy0 = p[4], d.wx0 = p[5], d.ch = p[6], d.cw = p[7];
    d.hb = p[8], d.hk = p[9], d.KH = p[10], d.vb = p[11], d.vk = p[12], d.KV = p[13], d.TB = p[14], d.CW = p[15];
    if (d.h < 1 || d.w < 1 || d.off < 0 || d.moff < 0 || (long)d.off + (long)d.h * d.w * 3 > img_bytes || (long)d.moff + (long)d.h * d.w > msk_bytes)
        return false;
    if (d.wy0 < 0 || d.wx0 < 0 || d.ch < 1 || d.cw < 1 || (long)d.wy0 + d.ch > d.h || (long)d.wx0 + d.cw > d.w) return false;
    if (d.TB < 1 || d.CW < 1 || d.TB > 4096 || d.CW > 4096) return false;      // (tile products stay inside int)
    const long nh = out_is_r ? R : d.cw, nv = out_is_r ? R : d.ch;
    return pil_axis_ok(d.hb, d.hk, d.KH, nh, tab_elems) && pil_axis_ok(d.vb, d.vk, d.KV, nv, tab_elems);
}

// g = clamp(v * 127.5 + 127.5, 0, 255), every operation rounded on its own, as composite_u8_kernel writes it.
__device__ __forceinline__ float ip_scale(float v) {
#pragma clang fp contract(off)
    v = v * 127.5f;
    v = v + 127.5f;
    return fminf(fmaxf(v, 0.f), 255.f);
}

// (A g + (F - A) orig) / F truncated: every product, the sum and the quotient rounded on its own.
__device__ __forceinline__ uint32_t ip_mix(float g, float a, float fa, float orig, float f) {
#pragma clang fp contract(off)
    const float t1 = a * g;
    const float t2 = fa * orig;
    float s = t1 + t2;
    s = s / f;
    return (uint32_t)(uint8_t)(int)s;
}

// The tile of a paste-back workgroup: window rows [y0, y0 + rows), columns [c0, c0 + cn), and the carves of its dynamic LDS --
//   flag (16 bytes), A [rows][cn]  |  hole flags [th][twp], row distances [th][cn]   (ip_feather_tile)
//                                  |  horizontally resampled rows, float [span][3 cn] (ip_resample_rows, over the same bytes)
struct IpTile {
    int y0, c0, rows, cn, th, tw, twp, a_bytes, t_bytes, r_bytes;
    int* flag;
    uint8_t *A, *tile, *rowd;
    float* mid;
};

__device__ __forceinline__ void ip_tile_make(IpTile& t, uint8_t* lds, int y0, int c0, int rows, int cn, int feather) {
    t.y0 = y0, t.c0 = c0, t.rows = rows, t.cn = cn;
    t.th = rows + 2 * feather, t.tw = cn + 2 * feather, t.twp = (t.tw + 3) & ~3;
    t.a_bytes = 16 + ip_align16(rows * cn), t.t_bytes = ip_align16(t.th * t.twp), t.r_bytes = ip_align16(t.th * cn);
    t.flag = reinterpret_cast<int*>(lds);
    t.A = lds + 16;
    t.tile = lds + t.a_bytes;
    t.rowd = t.tile + t.t_bytes;
    t.mid = reinterpret_cast<float*>(lds + t.a_bytes);
}

// Steps 1-2 of paste_back: the hole flags of the tile and a halo of `feather` pixels (outside the window: not a hole), the row pass and
// the column pass -> A [rows][cn] in LDS.  Returns false (workgroup-uniform) when no hole lies within `feather` of the tile: A = 0
// everywhere, and t.A is NOT written.  On return true the flags and row distances are dead and every lane has passed a barrier.
// A pixel is a hole where its byte equals `key`: 0 on the native mask, a group's key (1..255) on an owner plane (csrc/hole_label.hip).
__device__ __forceinline__ bool ip_feather_tile(const IpTile& t, const uint8_t* __restrict__ msk, const IpDesc& d, int feather, uint32_t key) {
    const int F = feather + 1, HALO = feather, y0 = t.y0, c0 = t.c0, rows = t.rows, cn = t.cn, th = t.th, tw = t.tw, twp = t.twp;
    uint8_t *tile = t.tile, *rowd = t.rowd, *A = t.A;
    // 1. hole flags of the tile and its halo
    for (int e = threadIdx.x; e < t.t_bytes >> 2; e += IP_THREADS) reinterpret_cast<uint32_t*>(tile)[e] = 0u;
    if (threadIdx.x == 0) *t.flag = 0;
    __syncthreads();
    const uint8_t* mwin = msk + d.moff + (long)d.wy0 * d.w + d.wx0;
    const int ca = max(c0 - HALO, 0), cb = min(c0 + cn + HALO, d.cw), nbm = cb - ca;       // window columns staged
    const int um = (tw + 6) >> 2;                                                           // aligned words a staged row can touch
    int found = 0;
    for (int e = threadIdx.x; e < th * um; e += IP_THREADS) {
        const int tr = e / um, u = e - tr * um, wr = y0 - HALO + tr;
        if (wr < 0 || wr >= d.ch) continue;
        const uint8_t* p = mwin + (long)wr * d.w + ca;
        const int lo = 4 * u - (int)(reinterpret_cast<uintptr_t>(p) & 3);
        if (lo >= nbm || lo + 4 <= 0) continue;
        uint8_t* trow = tile + tr * twp + (ca - (c0 - HALO));
        if (lo >= 0 && lo + 4 <= nbm) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p + lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int hole = ((v >> (8 * q)) & 255u) == key;
                trow[lo + q] = (uint8_t)hole;
                found |= hole;
            }
        } else {
            for (int q = max(lo, 0); q < min(lo + 4, nbm); ++q) {
                const int hole = p[q] == key;
                trow[q] = (uint8_t)hole;
                found |= hole;
            }
        }
    }
    if (found) *t.flag = 1;                                         // (every writer stores the same value)
    __syncthreads();
    if (*t.flag == 0) return false;                                 // no hole within `feather` of the tile: A = 0

    // 2. row pass, column pass
    for (int e = threadIdx.x; e < th * cn; e += IP_THREADS) {
        const int tr = e / cn, c = e - tr * cn;
        const uint8_t* tt = tile + tr * twp + c + HALO;
        int rd = F;
        for (int dd = 0; dd <= HALO; ++dd)
            if (tt[-dd] | tt[dd]) {
                rd = dd;
                break;
            }
        rowd[tr * cn + c] = (uint8_t)rd;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * cn; e += IP_THREADS) {
        const int r = e / cn, c = e - r * cn;
        const uint8_t* q = rowd + (r + HALO) * cn + c;
        int best = q[0];
        for (int dd = 1; dd < best && dd <= HALO; ++dd) best = min(best, max(dd, min((int)q[-dd * cn], (int)q[dd * cn])));
        A[e] = (uint8_t)(F - best);
    }
    __syncthreads();                                                // A complete; the flags and row distances are dead from here on
    return true;
}

// The key of window b in a keyed launch (keys: device int [B], each in 1..255; anything else -> -1, the window is left alone), 0 in a
// launch on the native mask (keys == nullptr).
__device__ __forceinline__ int ip_load_key(const int* __restrict__ keys, int b) {
    if (!keys) return 0;
    const int k = keys[b];
    return k >= 1 && k <= 255 ? k : -1;
}

// A of the tile into `alpha` (packed-mask layout), one lane per aligned 4-byte word of a row.  keyed: several windows of one image
// write one plane and a window's tile may cover another group's ring, so only A > 0 is stored -- a word whole when its four bytes are
// non-zero, else its non-zero bytes singly (the rings of two groups are at least 3 bytes apart on a row).
__device__ __forceinline__ void ip_store_alpha(const IpTile& t, uint8_t* __restrict__ alpha, const IpDesc& d, bool keyed) {
    const int cn = t.cn, ua = (cn + 6) >> 2;
    for (int e = threadIdx.x; e < t.rows * ua; e += IP_THREADS) {
        const int r = e / ua, u = e - r * ua;
        uint8_t* p = alpha + d.moff + (long)(d.wy0 + t.y0 + r) * d.w + d.wx0 + t.c0;
        const int lo = 4 * u - (int)(reinterpret_cast<uintptr_t>(p) & 3);
        if (lo >= cn || lo + 4 <= 0) continue;
        const uint8_t* ar = t.A + r * cn;
        const bool whole = lo >= 0 && lo + 4 <= cn;
        if (whole && (!keyed || (ar[lo] && ar[lo + 1] && ar[lo + 2] && ar[lo + 3]))) {
            *reinterpret_cast<uint32_t*>(p + lo) = (uint32_t)ar[lo] | (uint32_t)ar[lo + 1] << 8 | (uint32_t)ar[lo + 2] << 16 | (uint32_t)ar[lo + 3] << 24;
        } else {
            for (int q = max(lo, 0); q < min(lo + 4, cn); ++q)
                if (!keyed || ar[q]) p[q] = ar[q];
        }
    }
}

// Step 3, horizontal pass: rows [sy0, sy0 + span) of one sample's `fake` (planes of R x R at fk), resampled to the tile's columns,
// into t.mid [span][3 cn] (pixel-interleaved).  The caller synchronises afterwards.
__device__ __forceinline__ void ip_resample_rows(const IpTile& t, const int* __restrict__ tab, const IpDesc& d, const float* __restrict__ fk, int R,
                                                 int sy0, int span) {
    const long RR = (long)R * R;
    const int cn = t.cn;
    for (int e = threadIdx.x; e < span * cn; e += IP_THREADS) {
        const int r = e / cn, c = e - r * cn, x = t.c0 + c;
        int xmin = tab[d.hb + 2 * x], n = tab[d.hb + 2 * x + 1];
        if (xmin < 0 || n < 0 || n > d.KH || (long)xmin + n > R) xmin = 0, n = 0;
        const float* p = fk + (long)(sy0 + r) * R + xmin;
        const int* wk = tab + d.hk + (long)x * d.KH;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j = 0; j < n; ++j) {
            const float wj = __int_as_float(wk[j]);
            s0 = fmaf(wj, p[j], s0);
            s1 = fmaf(wj, p[RR + j], s1);
            s2 = fmaf(wj, p[2 * RR + j], s2);
        }
        float* m = t.mid + (r * cn + c) * 3;
        m[0] = s0, m[1] = s1, m[2] = s2;
    }
}

// Step 3, vertical pass of one value: m points at the first tap's row of t.mid, q is the index inside a row of nb = 3 cn floats.
__device__ __forceinline__ float ip_resample_col(const int* __restrict__ wk, const float* __restrict__ m, int n, int nb, int q) {
    float v = 0.f;
    for (int j = 0; j < n; ++j) v = fmaf(__int_as_float(wk[j]), m[j * nb + q], v);
    return v;
}

}  // namespace
