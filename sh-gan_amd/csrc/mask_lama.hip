// Rasteriser of the LaMa thin / medium / thick masks: the device half of lib/data_factory/lama_mask_utils.py behind
// `LamaMaskFormatter` (ds_ffhq.py:352-381).  The host (sh-gan_amd/masks.py) makes the random draws in the reference's order and turns
// every mask into a list of 8-word integer records; this kernel draws them as OpenCV's `cv2.line(img, p0, p1, 1, t)` does for t > 1:
//   RECT (0, x0, x1, y0, y1)                 columns x0 <= x < x1 of rows y0 <= y < y1 (the box generator, plain slices)
//   LINE (1, x0, y0, x1, y1, t, dpx, dpy)    ThickLine: the convex quad [P0 + dp, P0 - dp, P1 - dp, P1 + dp] in 16.16 fixed point
//                                            (P = p << 16; dp = (cvRound(dy r), cvRound(dx r)) comes from the HOST: its sqrt and
//                                            round-half-even are the one step that is not exact integer arithmetic), filled by
//                                            FillConvexPoly = an outline walk (Line2 behind clipLine) + the two-walker scan, and a
//                                            filled midpoint circle of radius (t + 1) >> 1 at each end.  p0 == p1: the circles only.
// mask = 1 - painted (1 = keep, 0 = hole), holes = number of painted pixels.
//
// One workgroup per mask.  The mask lives in LDS as a bit plane (s*s/8 bytes: 8 KiB at 256, 32 KiB at 512).  Waves take records, lanes
// take the independent units of a record and OR their spans / points into the plane with LDS atomics (OR commutes: the bits do not
// depend on the order):
//   * a scan row of the quad.  FillConvexPoly's two edge walkers change state only at the rows where an edge ends (a budget of 4 edge
//     steps in all), and between those rows x is xs + (y - y_set) * dx in exact integers -- a lane replays the (at most four) events up
//     to its own row instead of walking the rows;
//   * a step k of an outline walk: pixel (x1 + k, (y1 + k * y_step) >> 16);
//   * a row of a circle, its half width read from a table [rmax+1][rmax+1] that the host computes with the integer midpoint walk.
// After a barrier the plane is counted (__popc, one plain store of the count per mask: `holes` needs no zeroing, there are no global
// atomics) and expanded to float4 stores.  clipLine's one double expression is evaluated as OpenCV writes it, the product and the
// quotient rounded separately (both IEEE: the host restatement computes the same bits; tests/test_gpu_lama.py runs every branch).
// NOT CHECKED AGAINST cv2 itself: the specification is the restatement in tests/lama_cv_ref.py.
#include "shg_common.h"

#define ML_REC 8
#define ML_XS 16
#define ML_HALF (1 << 15)
#define ML_THREADS 1024
#define ML_MAX_S 512
#define ML_MAX_T 1023
#define ML_MAX_COORD 2048      // |coordinate| bound of a record: every 16.16 vertex then fits an int (2^27 + 2^25)

typedef long long ml_i64;

struct LamaParams {
    const int* rec;          // [total][8]
    const int* off;          // [B+1] record offsets
    const int* circ;         // [rmax+1][rmax+1] half widths, -1 = no row
    int rmax;
    float* mask;             // [B,1,s,s]
    int* holes;              // [B] number of zero pixels (written, not added to)
    int B, s;
};

// columns [xa, xb] of row y (0 <= y < s), clipped to the canvas
__device__ __forceinline__ void ml_span(unsigned* bits, int wpr, int s, int y, int xa, int xb) {
    xa = max(xa, 0);
    xb = min(xb, s - 1);
    if (xa > xb) return;
    unsigned* row = bits + y * wpr;
    for (int w = xa >> 5; w <= (xb >> 5); ++w) {
        const int lo = max(xa - 32 * w, 0), hi = min(xb - 32 * w, 31);
        atomicOr(row + w, (0xffffffffu >> (31 - (hi - lo))) << lo);
    }
}

__device__ __forceinline__ void ml_point(unsigned* bits, int wpr, int s, int x, int y) {
    if (x >= 0 && x < s && y >= 0 && y < s) atomicOr(bits + y * wpr + (x >> 5), 1u << (x & 31));
}

__device__ __forceinline__ int ml_sel(const int (&v)[4], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// OpenCV's clipLine on a (w, h) canvas (here in 16.16 units)
__device__ __forceinline__ bool ml_clip_line(ml_i64 w, ml_i64 h, ml_i64& x1, ml_i64& y1, ml_i64& x2, ml_i64& y2) {
#pragma clang fp contract(off)
    const ml_i64 right = w - 1, bottom = h - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const ml_i64 a = c1 < 8 ? 0 : bottom;
            const double pr = (double)(a - y1) * (double)(x2 - x1);
            x1 += (ml_i64)(pr / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const ml_i64 a = c2 < 8 ? 0 : bottom;
            const double pr = (double)(a - y2) * (double)(x2 - x1);
            x2 += (ml_i64)(pr / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const ml_i64 a = c1 == 1 ? 0 : right;
                const double pr = (double)(a - x1) * (double)(y2 - y1);
                y1 += (ml_i64)(pr / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const ml_i64 a = c2 == 1 ? 0 : right;
                const double pr = (double)(a - x2) * (double)(y2 - y1);
                y2 += (ml_i64)(pr / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// OpenCV's Line2 between two 16.16 points, the steps of its walk spread over the lanes of the wave
__device__ __forceinline__ void ml_outline(unsigned* bits, int wpr, int s, int lane, int ax_, int ay_, int bx_, int by_) {
    ml_i64 x1 = ax_, y1 = ay_, x2 = bx_, y2 = by_;
    if (!ml_clip_line((ml_i64)s << ML_XS, (ml_i64)s << ML_XS, x1, y1, x2, y2)) return;
    ml_i64 dx = x2 - x1, dy = y2 - y1;
    const ml_i64 adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool xmajor = adx > ady;
    if (!xmajor) {                                   // the y-major walk is the x-major one with the axes exchanged
        ml_i64 t;
        t = x1; x1 = y1; y1 = t;
        t = x2; x2 = y2; y2 = t;
        t = dx; dx = dy; dy = t;
    }
    if (dx < 0) {
        ml_i64 t;
        t = x1; x1 = x2; x2 = t;
        t = y1; y1 = y2; y2 = t;
        dx = -dx; dy = -dy;
    }
    const ml_i64 step = (dy * (1 << ML_XS)) / (dx | 1);
    const int n = min((int)((x2 - x1) >> ML_XS), s);          // <= s - 1 behind clipLine
    const int u0 = (int)((x1 + ML_HALF) >> ML_XS);
    const ml_i64 v0 = y1 + ML_HALF;
    if (lane == 0) {
        const int pu = (int)((x2 + ML_HALF) >> ML_XS), pv = (int)((y2 + ML_HALF) >> ML_XS);
        ml_point(bits, wpr, s, xmajor ? pu : pv, xmajor ? pv : pu);
    }
    for (int k = lane; k <= n; k += 64) {
        const int pu = u0 + k, pv = (int)((v0 + k * step) >> ML_XS);
        ml_point(bits, wpr, s, xmajor ? pu : pv, xmajor ? pv : pu);
    }
}

// One edge walker of FillConvexPoly at row yc (yc >= its ye): step along the polygon while the shared budget lasts
__device__ __forceinline__ void ml_advance(const int (&vx)[4], const int (&vy)[4], int di, int yc, int& edges, int& idx, int& xs, int& dx,
                                           int& ye, int& ys) {
    int idx0 = idx, k = (idx0 + di) & 3;
    for (;;) {
        if (edges-- <= 0) break;
        const int ty = (ml_sel(vy, k) + ML_HALF) >> ML_XS;
        if (ty > yc) {
            const int x0 = ml_sel(vx, idx0), xe = ml_sel(vx, k);
            ye = ty;
            dx = ((xe - x0) * 2 + (ty - yc)) / (2 * (ty - yc));      // |xe - x0| < 2^29: the numerator fits an int
            xs = x0;
            ys = yc;
            idx = k;
            break;
        }
        idx0 = k;
        k = (k + di) & 3;
    }
}

// FillConvexPoly's scan of the quad, one lane per row
__device__ __forceinline__ void ml_quad_fill(unsigned* bits, int wpr, int s, int lane, const int (&vx)[4], const int (&vy)[4]) {
    int imin = 0, vymin = vy[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (vy[k] < vymin) { vymin = vy[k]; imin = k; }
    const int xmin = (min(min(vx[0], vx[1]), min(vx[2], vx[3])) + ML_HALF) >> ML_XS;
    const int xmax = (max(max(vx[0], vx[1]), max(vx[2], vx[3])) + ML_HALF) >> ML_XS;
    const int ymin = (vymin + ML_HALF) >> ML_XS;
    int ymax = (max(max(vy[0], vy[1]), max(vy[2], vy[3])) + ML_HALF) >> ML_XS;
    if (xmax < 0 || ymax < 0 || xmin >= s || ymin >= s) return;
    ymax = min(ymax, s - 1);
    for (int y = max(ymin, 0) + lane; y <= ymax; y += 64) {
        int idx[2] = {imin, imin}, xs[2] = {-(1 << ML_XS), -(1 << ML_XS)}, dx[2] = {0, 0}, ye[2] = {ymin, ymin}, ys[2] = {ymin, ymin};
        int edges = 4, yc = ymin;
        bool paint = false;
        for (int it = 0; it < 8; ++it) {             // every pass but the last spends budget: four passes at the most
            if (yc >= ye[0]) ml_advance(vx, vy, 1, yc, edges, idx[0], xs[0], dx[0], ye[0], ys[0]);
            if (yc >= ye[1]) ml_advance(vx, vy, 3, yc, edges, idx[1], xs[1], dx[1], ye[1], ys[1]);
            if (edges < 0) break;                    // the budget ran out at row yc: the polygon ends above it
            const int yn = min(ye[0], ye[1]);
            if (y < yn) { paint = true; break; }
            yc = yn;
        }
        if (!paint) continue;
        const ml_i64 xa = xs[0] + (ml_i64)(y - ys[0]) * dx[0], xb = xs[1] + (ml_i64)(y - ys[1]) * dx[1];
        const int xx1 = (int)((min(xa, xb) + ML_HALF) >> ML_XS), xx2 = (int)((max(xa, xb) + ML_HALF) >> ML_XS);
        if (xx2 >= 0 && xx1 < s) ml_span(bits, wpr, s, y, xx1, xx2);
    }
}

// One record, drawn by one wave
__device__ __forceinline__ void ml_record(unsigned* bits, int wpr, int s, int lane, const int* q, const int* circ, int rmax) {
    const int type = q[0], a0 = q[1], a1 = q[2], a2 = q[3], a3 = q[4];
    if (type == 0) {
        for (int y = max(a2, 0) + lane; y < min(a3, s); y += 64) ml_span(bits, wpr, s, y, a0, a1 - 1);
        return;
    }
    const int t = q[5], dpx = q[6], dpy = q[7];
    if (a0 != a2 || a1 != a3) {
        const int px0 = a0 * (1 << ML_XS), py0 = a1 * (1 << ML_XS), px1 = a2 * (1 << ML_XS), py1 = a3 * (1 << ML_XS);
        const int vx[4] = {px0 + dpx, px0 - dpx, px1 - dpx, px1 + dpx};
        const int vy[4] = {py0 + dpy, py0 - dpy, py1 - dpy, py1 + dpy};
        ml_outline(bits, wpr, s, lane, vx[3], vy[3], vx[0], vy[0]);
        ml_outline(bits, wpr, s, lane, vx[0], vy[0], vx[1], vy[1]);
        ml_outline(bits, wpr, s, lane, vx[1], vy[1], vx[2], vy[2]);
        ml_outline(bits, wpr, s, lane, vx[2], vy[2], vx[3], vy[3]);
        ml_quad_fill(bits, wpr, s, lane, vx, vy);
    }
    const int rad = min((t + 1) >> 1, rmax), rows = 2 * rad + 1;         // ((t << 15) + HALF) >> 16
    const int* hw = circ + (long)rad * (rmax + 1);
    for (int u = lane; u < 2 * rows; u += 64) {
        const int second = u >= rows, j = u - second * rows - rad;
        const int y = (second ? a3 : a1) + j;
        if (y < 0 || y >= s) continue;
        const int h = hw[j < 0 ? -j : j];
        const int cx = second ? a2 : a0;
        if (h >= 0) ml_span(bits, wpr, s, y, cx - h, cx + h);
    }
}

__global__ __launch_bounds__(ML_THREADS) void mask_lama_kernel(const LamaParams p) {
    __shared__ unsigned bits[ML_MAX_S * ML_MAX_S / 32];
    __shared__ int red[ML_THREADS / 64];
    const int b = blockIdx.x, s = p.s, wpr = s >> 5, nw = s * wpr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nw; i += ML_THREADS) bits[i] = 0u;
    __syncthreads();
    const int r0 = p.off[b], r1 = p.off[b + 1];
    for (int r = r0 + wave; r < r1; r += ML_THREADS / 64)          // wave-uniform record address
        ml_record(bits, wpr, s, lane, p.rec + (long)r * ML_REC, p.circ, p.rmax);
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < nw; i += ML_THREADS) cnt += __popc(bits[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < ML_THREADS / 64; ++w) total += red[w];
        p.holes[b] = total;
    }
    float4* out = reinterpret_cast<float4*>(p.mask + (long)b * s * s);
    for (int i = tid; i < (nw << 3); i += ML_THREADS) {          // pixel 4 i .. 4 i + 3 = bits 4 (i & 7) .. of word i >> 3
        const unsigned nb = bits[i >> 3] >> (4 * (i & 7));
        float4 v;
        v.x = nb & 1u ? 0.f : 1.f;
        v.y = nb & 2u ? 0.f : 1.f;
        v.z = nb & 4u ? 0.f : 1.f;
        v.w = nb & 8u ? 0.f : 1.f;
        out[i] = v;
    }
}

// records_host / offsets_host: the HOST copies of the two device arrays (the staging buffer the caller uploaded them from) -- every
// record is checked here, before the launch; records / offsets / circle_table [rmax+1][rmax+1] / mask [B,1,s,s] / holes [B]: device
// memory.  holes is written (it needs no zeroing).  s: multiple of 32 in [32, 512]; t in [2, 1023] with (t + 1) >> 1 <= rmax.
extern "C" int shg_mask_lama_f32(const int* records_host, const int* offsets_host, const int* records, const int* offsets,
                                 const int* circle_table, int rmax, float* mask, int* holes, int B, int total, int s, void* stream) {
    SHG_CHECK_ARG(records_host && offsets_host && records && offsets && circle_table && mask && holes, "mask_lama: null pointer");
    SHG_CHECK_ARG(s >= 32 && s <= ML_MAX_S && s % 32 == 0, "mask_lama: s must be a multiple of 32 in [32, 512] (got %d)", s);
    SHG_CHECK_ARG(B >= 1 && B <= 65535 && total >= 0 && rmax >= 1, "mask_lama: B must lie in [1, 65535], total >= 0, rmax >= 1");
    SHG_CHECK_ARG((reinterpret_cast<uintptr_t>(mask) & 15) == 0, "mask_lama: mask must be 16-byte aligned");
    SHG_CHECK_ARG(offsets_host[0] == 0 && offsets_host[B] == total, "mask_lama: offsets must run from 0 to the number of records");
    for (int b = 0; b < B; ++b) SHG_CHECK_ARG(offsets_host[b] <= offsets_host[b + 1], "mask_lama: offsets must not decrease");
    for (int r = 0; r < total; ++r) {
        const int* q = records_host + (long)r * ML_REC;
        SHG_CHECK_ARG(q[0] == 0 || q[0] == 1, "mask_lama: record %d has unknown type %d", r, q[0]);
        for (int k = 1; k <= 4; ++k)
            SHG_CHECK_ARG(q[k] >= -ML_MAX_COORD && q[k] <= ML_MAX_COORD, "mask_lama: record %d: coordinate %d beyond +-%d", r, q[k], ML_MAX_COORD);
        if (q[0] == 1) {
            SHG_CHECK_ARG(q[5] >= 2 && q[5] <= ML_MAX_T && ((q[5] + 1) >> 1) <= rmax,
                          "mask_lama: record %d: thickness %d outside [2, %d] or beyond the circle table", r, q[5], ML_MAX_T);
            SHG_CHECK_ARG(q[6] > -(1 << 26) && q[6] < (1 << 26) && q[7] > -(1 << 26) && q[7] < (1 << 26), "mask_lama: record %d: quad offset out of range", r);
        }
    }
    LamaParams p;
    p.rec = records; p.off = offsets; p.circ = circle_table; p.rmax = rmax; p.mask = mask; p.holes = holes; p.B = B; p.s = s;
    hipLaunchKernelGGL(mask_lama_kernel, dim3(B), dim3(ML_THREADS), 0, (hipStream_t)stream, p);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
