// Hole groups of a packed batch of masks (sh-gan_amd/inpaint.py label_holes / owner_plane): which holes of a
// photograph share one window.  Masks are uint8 HW packed back to back (0 = hole); `shapes` is device int32 [B][4] = {h, w, image byte
// offset (unused here), mask byte offset}.  With r = feather + 1 (1..33):
//   D     = the pixels within Chebyshev distance r of a hole pixel of the same image (clipped to the image),
//   group = an 8-connected component of D; its root is the smallest y w + x over its pixels,
//   labels (int32, packed-mask layout) = the root where the pixel lies in D, -1 elsewhere,
//   comps  (int32 [max_components][8]) = {image, root, ya, yb, xa, xb, hole pixels, 0}: the half-open bounding box of the group's HOLE
//           pixels and their count, one row per group in no particular order (rows that are not used hold zeros),
//   counter = {groups found, flags}: bit 0 = more groups than max_components (the ones beyond it are dropped from comps, labels is still
//           complete), bit 1 = a find / union loop ran into its cap (the result is then not to be used; the host raises).
//
// The sequence (launch boundaries are the only synchronisation between workgroups; no flags, no spinning, no cooperative launch):
//   1. hl_tile_kernel, one workgroup per HL_TILE x HL_TILE tile of an image: the hole flags of the tile and a halo of r in LDS, the
//      separable row / column "any hole within r" pass -> D, then a union-find over the tile in LDS (a pixel starts under the first pixel
//      of its run along the row; parents point at smaller indices, a union is an atomicMin on the larger root) and its flatten; the tile's provisional roots go out as image indices y w + x.  A tile
//      whose staged flags hold no hole stores -1 and is done.
//   2. hl_seam_kernel, one lane per pixel of the first row / first column of a tile: the unions with its three neighbours across the
//      border (corners included) in the global label plane.  Parents are read with agent-scope relaxed atomic loads and only the value an
//      atomicMin returns decides a union: L1 is per CU and may hold a stale parent, which is a former parent of the same set, so a find
//      that ends on it is put right by the atomicMin that follows.
//   3. hl_flatten_kernel: every pixel of D takes its root; a root draws a slot of comps and leaves the slot at its own position of the
//      scratch plane.
//   4. hl_reduce_kernel, one workgroup per tile: the hole pixels that share the tile's smallest root (nearly always all of them) reduce
//      their box and count in LDS and issue one set of atomics per workgroup; the others go to global memory singly.
// Integer atomicMin / atomicMax / atomicAdd only: the results do not depend on the order, and labels / boxes / counts are the same on
// every run.  Every find / union loop carries a cap (the pixels it could walk) and parents are checked to decrease, so no loop can spin.
// A descriptor that points outside the mask bytes, or is larger than max_h x max_w, leaves its image unwritten; nothing is read or
// written out of bounds.
//
// shg_hole_owner_u8: the owner plane (uint8, packed-mask layout): 0 at known pixels, at a hole pixel the key of its group from a device
// table int32 [n][3] = {image, root, key in 1..255}: roots clear their scratch entry, the table scatters its keys to the root positions,
// every hole pixel looks its root's entry up (a group the table does not name gets 0).
#include "shg_common.h"

namespace {

constexpr int HL_THREADS = 256;
constexpr int HL_TILE = 64;
constexpr int HL_PER_LANE = HL_TILE * HL_TILE / HL_THREADS;
constexpr int HL_MAX_R = 33;                                        // inpaint.py MAX_FEATHER + 1
constexpr int HL_OVERFLOW = 1, HL_CAP_HIT = 2;

struct HlImg {
    int h, w, moff;
};

__device__ __forceinline__ bool hl_load(const int* __restrict__ shapes, int b, long msk_bytes, int max_h, int max_w, HlImg& g) {
    const int* p = shapes + 4L * b;
    g.h = p[0], g.w = p[1], g.moff = p[3];
    return g.h >= 1 && g.w >= 1 && g.h <= max_h && g.w <= max_w && g.moff >= 0 && (long)g.moff + (long)g.h * g.w <= msk_bytes;
}

__host__ __device__ __forceinline__ int hl_align16(int n) { return (n + 15) & ~15; }

// LDS of hl_tile_kernel: D [T][T] | the larger of (flags [T + 2r][T + 2r] + row hits [T + 2r][T]) and (parents int [T][T], which take
// the bytes over once D stands)
__host__ __device__ __forceinline__ int hl_lds_bytes(int r) {
    const int th = HL_TILE + 2 * r;
    const int a = hl_align16(th * th) + hl_align16(th * HL_TILE), b = 4 * HL_TILE * HL_TILE;
    return HL_TILE * HL_TILE + (a > b ? a : b);
}

// The root of i in the parent array L of n entries, at most `cap` steps.  A parent outside [0, i] (never written by these kernels) or
// the cap sets `bad` and ends the walk.
template <int SCOPE>
__device__ __forceinline__ int hl_find(int* L, int i, int n, int cap, int& bad) {
    for (int it = 0; it < cap; ++it) {
        const int p = __hip_atomic_load(L + i, __ATOMIC_RELAXED, SCOPE);
        if (p == i) return i;
        if (p < 0 || p > i || p >= n) break;
        i = p;
    }
    bad = 1;
    return i;
}

// Unite the sets of a and b: the larger root goes under the smaller with an atomicMin; when the atomic returns another parent than the
// root itself, somebody else re-parented it meanwhile and the union goes on with that parent (which the atomicMin may have replaced).
template <int SCOPE>
__device__ __forceinline__ void hl_union(int* L, int a, int b, int n, int cap, int& bad) {
    for (int it = 0; it < cap; ++it) {
        a = hl_find<SCOPE>(L, a, n, cap, bad);
        b = hl_find<SCOPE>(L, b, n, cap, bad);
        if (bad || a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        if (old < 0 || old > a) break;
        a = old;
    }
    bad = 1;
}

__global__ __launch_bounds__(HL_THREADS) void hl_tile_kernel(const uint8_t* __restrict__ msk, long msk_bytes, const int* __restrict__ shapes,
                                                             int max_h, int max_w, int r, int* __restrict__ labels, int* __restrict__ counter) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hl_lds[];
    __shared__ int s_found;
    constexpr int T = HL_TILE;
    HlImg g;
    if (!hl_load(shapes, blockIdx.z, msk_bytes, max_h, max_w, g)) return;
    const int y0 = (int)blockIdx.y * T, x0 = (int)blockIdx.x * T;
    if (y0 >= g.h || x0 >= g.w) return;
    const int rows = min(T, g.h - y0), cols = min(T, g.w - x0), th = rows + 2 * r, twp = T + 2 * r;
    uint8_t* D = hl_lds;
    uint8_t* flags = hl_lds + T * T;
    uint8_t* rowhit = flags + hl_align16(twp * twp);
    int* L = reinterpret_cast<int*>(hl_lds + T * T);
    const uint8_t* m = msk + g.moff;
    int* lab = labels + g.moff;

    // 1. hole flags of the tile and its halo (outside the image: not a hole).  The flags are zeroed; then half a wave takes a staged row
    //    at a time and a lane one aligned 4-byte word of it (single bytes at the row's ragged ends)
    for (int e = threadIdx.x; e < hl_align16(twp * twp) >> 2; e += HL_THREADS) reinterpret_cast<uint32_t*>(flags)[e] = 0u;
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    const int ca = max(x0 - r, 0), cb = min(x0 + cols + r, g.w), nb = cb - ca;          // image columns staged
    const int um = (nb + 6) >> 2;                                                       // aligned words a staged row can touch
    int found = 0;
    for (int tr = threadIdx.x >> 5; tr < th; tr += HL_THREADS >> 5) {
        const int gy = y0 - r + tr;
        if (gy < 0 || gy >= g.h) continue;
        const uint8_t* p = m + (long)gy * g.w + ca;
        uint8_t* frow = flags + tr * twp + (ca - (x0 - r));
        const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        for (int u = threadIdx.x & 31; u < um; u += 32) {
            const int lo = 4 * u - mis;
            if (lo >= nb) break;
            if (lo >= 0 && lo + 4 <= nb) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(p + lo);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (((v >> (8 * q)) & 255u) == 0u) frow[lo + q] = 1, found = 1;
            } else {
                for (int q = max(lo, 0); q < min(lo + 4, nb); ++q)
                    if (p[q] == 0) frow[q] = 1, found = 1;
            }
        }
    }
    if (found) s_found = 1;                                         // (every writer stores the same value)
    __syncthreads();
    if (s_found == 0) {                                             // workgroup-uniform: no pixel of the tile lies in D
        for (int e = threadIdx.x; e < T * T; e += HL_THREADS) {
            const int rr = e / T, c = e - rr * T;
            if (rr < rows && c < cols) lab[(long)(y0 + rr) * g.w + x0 + c] = -1;
        }
        return;
    }

    // 2. D: a hole within r along the row, then within r along the column
    for (int e = threadIdx.x; e < th * T; e += HL_THREADS) {
        const int tr = e / T, c = e - tr * T;
        if (c >= cols) continue;
        const uint8_t* f = flags + tr * twp + c;
        int hit = 0;
        for (int dd = 0; dd <= 2 * r; ++dd) hit |= f[dd];
        rowhit[tr * T + c] = (uint8_t)hit;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * T; e += HL_THREADS) {
        const int rr = e / T, c = e - rr * T;
        int hit = 0;
        if (rr < rows && c < cols)
            for (int dd = 0; dd <= 2 * r; ++dd) hit |= rowhit[(rr + dd) * T + c];
        D[e] = (uint8_t)hit;
    }
    __syncthreads();                                                // D stands; flags and row hits are dead, L takes their bytes

    // 3. union-find over the tile
    // 3. union-find over the tile.  A pixel starts under the first pixel of its run along the row, so no union is needed along a row;
    //    a union with the row above is needed only where it is not implied by the neighbours' own: with N, unless W and NW are both
    //    in D (W hangs on NW, which shares N's run); without N, with NW unless W is in D (W's own N) and with NE unless E is (E's own N).
    for (int e = threadIdx.x; e < T * T; e += HL_THREADS) {
        int s = -1;
        if (D[e]) {
            s = e;
            for (int c = e % T; c > 0 && D[s - 1]; --c) --s;        // (at most T - 1 steps)
        }
        L[e] = s;
    }
    __syncthreads();
    int bad = 0;
    for (int e = threadIdx.x; e < T * T; e += HL_THREADS) {
        if (!D[e]) continue;
        const int rr = e / T, c = e - rr * T;
        if (rr == 0) continue;
        const bool W = c > 0 && D[e - 1], NW = c > 0 && D[e - T - 1];
        if (D[e - T]) {
            if (!(W && NW)) hl_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, e, e - T, T * T, T * T, bad);
        } else {
            if (NW && !W) hl_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, e, e - T - 1, T * T, T * T, bad);
            if (c < T - 1 && D[e - T + 1] && !D[e + 1]) hl_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, e, e - T + 1, T * T, T * T, bad);
        }
    }
    __syncthreads();
    int root[HL_PER_LANE];
#pragma unroll
    for (int i = 0; i < HL_PER_LANE; ++i) {
        const int e = threadIdx.x + i * HL_THREADS;
        root[i] = D[e] ? hl_find<__HIP_MEMORY_SCOPE_WORKGROUP>(L, e, T * T, T * T, bad) : -1;
    }
#pragma unroll
    for (int i = 0; i < HL_PER_LANE; ++i) {
        const int e = threadIdx.x + i * HL_THREADS, rr = e / T, c = e - rr * T;
        if (rr >= rows || c >= cols) continue;
        const int q = root[i];                                      // row-major inside the tile orders as row-major inside the image
        lab[(long)(y0 + rr) * g.w + x0 + c] = q < 0 ? -1 : (y0 + q / T) * g.w + x0 + q % T;
    }
    if (bad) atomicOr(counter + 1, HL_CAP_HIT);
}

// One lane per pixel of a seam line: blockIdx.y counts the image's row seams (y = T, 2T, ...), then its column seams.
__global__ __launch_bounds__(HL_THREADS) void hl_seam_kernel(long msk_bytes, const int* __restrict__ shapes, int max_h, int max_w, int* labels,
                                                             int* __restrict__ counter) {
    constexpr int T = HL_TILE;
    HlImg g;
    if (!hl_load(shapes, blockIdx.z, msk_bytes, max_h, max_w, g)) return;
    const int nrs = (g.h - 1) / T, ncs = (g.w - 1) / T, line = blockIdx.y, pos = (int)blockIdx.x * HL_THREADS + (int)threadIdx.x;
    const int n = g.h * g.w;
    int* L = labels + g.moff;
    int y, x, sy, sx;                                               // the pixel, and the step along the far side of the border
    if (line < nrs) {
        y = (line + 1) * T, x = pos, sy = 0, sx = 1;
    } else if (line - nrs < ncs) {
        x = (line - nrs + 1) * T, y = pos, sy = 1, sx = 0;
    } else {
        return;
    }
    if (y >= g.h || x >= g.w) return;
    const int p = y * g.w + x;
    if (__hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    int bad = 0;
    for (int dd = -1; dd <= 1; ++dd) {
        const int qy = sx ? y - 1 : y + dd * sy, qx = sx ? x + dd * sx : x - 1;
        if (qy < 0 || qy >= g.h || qx < 0 || qx >= g.w) continue;
        const int q = qy * g.w + qx;
        if (__hip_atomic_load(L + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        hl_union<__HIP_MEMORY_SCOPE_AGENT>(L, p, q, n, n, bad);
    }
    if (bad) atomicOr(counter + 1, HL_CAP_HIT);
}

// One lane per pixel: the root; a root draws its slot of comps.
__global__ __launch_bounds__(HL_THREADS) void hl_flatten_kernel(long msk_bytes, const int* __restrict__ shapes, int max_h, int max_w, int* labels,
                                                                int* __restrict__ scratch, int* __restrict__ comps, int max_components,
                                                                int* __restrict__ counter) {
    HlImg g;
    const int b = blockIdx.y;
    if (!hl_load(shapes, b, msk_bytes, max_h, max_w, g)) return;
    const long p = (long)blockIdx.x * HL_THREADS + threadIdx.x;
    const int n = g.h * g.w;
    if (p >= n) return;
    int* L = labels + g.moff;
    if (__hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    int bad = 0;
    const int root = hl_find<__HIP_MEMORY_SCOPE_AGENT>(L, (int)p, n, n, bad);
    if (bad) {
        atomicOr(counter + 1, HL_CAP_HIT);
        return;
    }
    if (root != (int)p) {                                           // (a root keeps its own entry: walks through p still end on it)
        __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int slot = atomicAdd(counter, 1);
    if (slot < max_components) {
        int* c = comps + 8L * slot;
        c[0] = b, c[1] = root, c[2] = g.h, c[3] = 0, c[4] = g.w, c[5] = 0, c[6] = 0, c[7] = 0;
        scratch[g.moff + p] = slot;
    } else {
        scratch[g.moff + p] = -1;
        atomicOr(counter + 1, HL_OVERFLOW);
    }
}

__device__ __forceinline__ void hl_box_atomics(int* c, int ya, int yb, int xa, int xb, int cnt) {
    atomicMin(c + 2, ya);
    atomicMax(c + 3, yb);
    atomicMin(c + 4, xa);
    atomicMax(c + 5, xb);
    atomicAdd(c + 6, cnt);
}

// One workgroup per tile: boxes and counts of the hole pixels onto their roots' slots.
__global__ __launch_bounds__(HL_THREADS) void hl_reduce_kernel(const uint8_t* __restrict__ msk, long msk_bytes, const int* __restrict__ shapes,
                                                               int max_h, int max_w, const int* __restrict__ labels,
                                                               const int* __restrict__ scratch, int* __restrict__ comps, int max_components) {
    constexpr int T = HL_TILE;
    __shared__ int s_root, s_box[8];                                // (s_box: a row of comps in LDS, words 2..6 used)
    HlImg g;
    if (!hl_load(shapes, blockIdx.z, msk_bytes, max_h, max_w, g)) return;
    const int y0 = (int)blockIdx.y * T, x0 = (int)blockIdx.x * T;
    if (y0 >= g.h || x0 >= g.w) return;
    const int n = g.h * g.w;
    if (threadIdx.x == 0) s_root = n, s_box[2] = g.h, s_box[3] = 0, s_box[4] = g.w, s_box[5] = 0, s_box[6] = 0;
    __syncthreads();
    int root[HL_PER_LANE], low = n;
#pragma unroll
    for (int i = 0; i < HL_PER_LANE; ++i) {
        const int e = threadIdx.x + i * HL_THREADS, y = y0 + e / T, x = x0 + e % T;
        root[i] = -1;
        if (y < g.h && x < g.w && msk[g.moff + (long)y * g.w + x] == 0) {
            const int q = labels[g.moff + (long)y * g.w + x];
            if (q >= 0 && q < n) root[i] = q, low = min(low, q);
        }
    }
    if (low < n) atomicMin(&s_root, low);
    __syncthreads();
    const int common = s_root;
    if (common >= n) return;                                        // workgroup-uniform: no hole pixel in the tile
    int ya = g.h, yb = 0, xa = g.w, xb = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < HL_PER_LANE; ++i) {
        if (root[i] < 0) continue;
        const int e = threadIdx.x + i * HL_THREADS, y = y0 + e / T, x = x0 + e % T;
        if (root[i] == common) {
            ya = min(ya, y), yb = max(yb, y + 1), xa = min(xa, x), xb = max(xb, x + 1), ++cnt;
        } else {
            const int slot = scratch[g.moff + root[i]];
            if (slot >= 0 && slot < max_components) hl_box_atomics(comps + 8L * slot, y, y + 1, x, x + 1, 1);
        }
    }
    if (cnt) hl_box_atomics(s_box, ya, yb, xa, xb, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int slot = scratch[g.moff + common];
        if (slot >= 0 && slot < max_components) hl_box_atomics(comps + 8L * slot, s_box[2], s_box[3], s_box[4], s_box[5], s_box[6]);
    }
}

// owner plane, step 1: every root clears its scratch entry
__global__ __launch_bounds__(HL_THREADS) void hl_owner_clear_kernel(long msk_bytes, const int* __restrict__ shapes, int max_h, int max_w,
                                                                    const int* __restrict__ labels, int* __restrict__ scratch) {
    HlImg g;
    if (!hl_load(shapes, blockIdx.y, msk_bytes, max_h, max_w, g)) return;
    const long p = (long)blockIdx.x * HL_THREADS + threadIdx.x;
    if (p >= (long)g.h * g.w) return;
    if (labels[g.moff + p] == (int)p) scratch[g.moff + p] = 0;
}

// step 2: the table's keys to the root positions
__global__ __launch_bounds__(HL_THREADS) void hl_owner_scatter_kernel(long msk_bytes, const int* __restrict__ shapes, int B, int max_h, int max_w,
                                                                      const int* __restrict__ labels, const int* __restrict__ table, int n_table,
                                                                      int* __restrict__ scratch) {
    const int i = (int)blockIdx.x * HL_THREADS + (int)threadIdx.x;
    if (i >= n_table) return;
    const int b = table[3L * i], root = table[3L * i + 1], key = table[3L * i + 2];
    HlImg g;
    if (b < 0 || b >= B || !hl_load(shapes, b, msk_bytes, max_h, max_w, g)) return;
    if (root < 0 || root >= g.h * g.w || key < 1 || key > 255 || labels[g.moff + root] != root) return;
    scratch[g.moff + root] = key;
}

// step 3: 0 at known pixels, the key of its root at a hole pixel
__global__ __launch_bounds__(HL_THREADS) void hl_owner_write_kernel(const uint8_t* __restrict__ msk, long msk_bytes, const int* __restrict__ shapes,
                                                                    int max_h, int max_w, const int* __restrict__ labels,
                                                                    const int* __restrict__ scratch, uint8_t* __restrict__ owner) {
    HlImg g;
    if (!hl_load(shapes, blockIdx.y, msk_bytes, max_h, max_w, g)) return;
    const long p = (long)blockIdx.x * HL_THREADS + threadIdx.x;
    const int n = g.h * g.w;
    if (p >= n) return;
    int key = 0;
    if (msk[g.moff + p] == 0) {
        const int root = labels[g.moff + p];
        if (root >= 0 && root < n && labels[g.moff + root] == root) key = scratch[g.moff + root];
    }
    owner[g.moff + p] = (uint8_t)key;
}

// blocks of a one-lane-per-pixel launch: an image has at most min(max_h max_w, mask_bytes) pixels
unsigned hl_px_blocks(long mask_bytes, int max_h, int max_w) {
    const long px = (long)max_h * max_w < mask_bytes ? (long)max_h * max_w : mask_bytes;
    return (unsigned)((px + HL_THREADS - 1) / HL_THREADS);
}

int hl_check_args(const char* who, long mask_bytes, int B, int max_h, int max_w) {
    SHG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must lie in [1, 65535] (got %d)", who, B);
    SHG_CHECK_ARG(mask_bytes >= 1 && mask_bytes <= 0x7fffffffL, "%s: mask_bytes must lie in [1, 2^31) (int32 offsets)", who);
    SHG_CHECK_ARG(max_h >= 1 && max_w >= 1 && max_h <= (1 << 21) && max_w <= (1 << 21), "%s: max_h and max_w must lie in [1, 2^21] (got %d, %d)", who,
                  max_h, max_w);
    return SHG_OK;
}

}  // namespace

extern "C" int shg_hole_label_tile(void) { return HL_TILE; }

// mask: uint8 [mask_bytes]; shapes: device int32 [B][4], every h <= max_h and w <= max_w; r in 1..33.  labels, scratch: int32
// [mask_bytes] each (scratch: contents irrelevant, written at root positions only); comps: int32 [max_components][8]; counter: int32 [2].
// Both comps and counter are zeroed here.  A memset and four launches (three when no image has a second tile) on `stream`.
extern "C" int shg_hole_label_i32(const void* mask, long mask_bytes, const int* shapes, int B, int max_h, int max_w, int r, int max_components,
                                  int* labels, int* scratch, int* comps, int* counter, void* stream) {
    SHG_CHECK_ARG(mask && shapes && labels && scratch && comps && counter, "hole_label: null pointer");
    if (int rc = hl_check_args("hole_label", mask_bytes, B, max_h, max_w)) return rc;
    SHG_CHECK_ARG(r >= 1 && r <= HL_MAX_R, "hole_label: r must lie in [1, %d] (got %d)", HL_MAX_R, r);
    SHG_CHECK_ARG(max_components >= 1 && max_components <= (1 << 24), "hole_label: max_components must lie in [1, 2^24] (got %d)", max_components);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(comps, 0, sizeof(int) * 8 * (size_t)max_components, st) != hipSuccess || hipMemsetAsync(counter, 0, 2 * sizeof(int), st) != hipSuccess) {
        shg_set_error("hole_label: hipMemsetAsync failed");
        return SHG_ERR_LAUNCH;
    }
    const dim3 tiles(shg_cdiv(max_w, HL_TILE), shg_cdiv(max_h, HL_TILE), B);
    const int lines = (max_h - 1) / HL_TILE + (max_w - 1) / HL_TILE;
    const unsigned px_blocks = hl_px_blocks(mask_bytes, max_h, max_w);
    hipLaunchKernelGGL(hl_tile_kernel, tiles, dim3(HL_THREADS), (size_t)hl_lds_bytes(r), st, (const uint8_t*)mask, mask_bytes, shapes, max_h, max_w, r,
                       labels, counter);
    if (lines > 0)
        hipLaunchKernelGGL(hl_seam_kernel, dim3(shg_cdiv(max_h > max_w ? max_h : max_w, HL_THREADS), lines, B), dim3(HL_THREADS), 0, st, mask_bytes,
                           shapes, max_h, max_w, labels, counter);
    hipLaunchKernelGGL(hl_flatten_kernel, dim3(px_blocks, B), dim3(HL_THREADS), 0, st, mask_bytes, shapes, max_h, max_w, labels, scratch, comps,
                       max_components, counter);
    hipLaunchKernelGGL(hl_reduce_kernel, tiles, dim3(HL_THREADS), 0, st, (const uint8_t*)mask, mask_bytes, shapes, max_h, max_w, labels, scratch, comps,
                       max_components);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}

// labels: what shg_hole_label_i32 wrote for the same mask and shapes; table: device int32 [n_table][3] = {image, root, key in 1..255}
// (a row that names no root of its image is skipped); scratch: int32 [mask_bytes], contents irrelevant; owner: uint8 [mask_bytes].
extern "C" int shg_hole_owner_u8(const void* mask, long mask_bytes, const int* shapes, int B, int max_h, int max_w, const int* labels,
                                 const int* table, int n_table, int* scratch, void* owner, void* stream) {
    SHG_CHECK_ARG(mask && shapes && labels && scratch && owner && (table || n_table == 0), "hole_owner: null pointer");
    if (int rc = hl_check_args("hole_owner", mask_bytes, B, max_h, max_w)) return rc;
    SHG_CHECK_ARG(n_table >= 0 && n_table <= (1 << 24), "hole_owner: n_table must lie in [0, 2^24] (got %d)", n_table);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(hl_px_blocks(mask_bytes, max_h, max_w), B);
    hipLaunchKernelGGL(hl_owner_clear_kernel, grid, dim3(HL_THREADS), 0, st, mask_bytes, shapes, max_h, max_w, labels, scratch);
    if (n_table > 0)
        hipLaunchKernelGGL(hl_owner_scatter_kernel, dim3(shg_cdiv(n_table, HL_THREADS)), dim3(HL_THREADS), 0, st, mask_bytes, shapes, B, max_h, max_w,
                           labels, table, n_table, scratch);
    hipLaunchKernelGGL(hl_owner_write_kernel, grid, dim3(HL_THREADS), 0, st, (const uint8_t*)mask, mask_bytes, shapes, max_h, max_w, labels, scratch,
                       (uint8_t*)owner);
    SHG_CHECK_LAUNCH();
    return SHG_OK;
}
