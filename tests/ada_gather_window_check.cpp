// Brute-force proof of the candidate window of the gather-form ADA adjoint (sh-gan_amd/csrc/ada_geom.h, compiled as host code; driven by
// tests/test_ada_gather_cpu.py).  stdin: one case per line, "H W mx0 my0 mx1 my1 g0 g1 g2 g3 g4 g5" (the six floats in any strtod form).
// For every sample (jx, jy) of the grid and each of the (up to four) upsampled pixels v its bilinear footprint touches -- floor(c) and
// floor(c) + 1 per axis, inside the upsampled image -- the sample must lie inside ada_gather_window(v).  stdout, per case:
// "ok touched violations largest_window"; a case the gather route does not take prints "0 0 0 0".
#include <cstdio>
#include <cstdlib>

#include "ada_geom.h"

int main() {
    int H, W, mg[4];
    char gs[6][64];
    while (std::scanf("%d %d %d %d %d %d %63s %63s %63s %63s %63s %63s", &H, &W, &mg[0], &mg[1], &mg[2], &mg[3], gs[0], gs[1], gs[2], gs[3],
                      gs[4], gs[5]) == 12) {
        float G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1};
        for (int i = 0; i < 6; ++i) G[i] = (float)std::strtod(gs[i], nullptr);
        const AdaGeo q = ada_geo(G, mg, 0, H, W);
        const AdaInv m = ada_gather_inverse(q, H, W);
        if (!m.ok) {
            std::printf("0 0 0 0\n");
            continue;
        }
        const int wp = W + q.mx0 + q.mx1, hp = H + q.my0 + q.my1;
        long touched = 0, bad = 0, largest = 0;
        for (int jy = 1; jy <= 2 * H + 10; ++jy)
            for (int jx = 1; jx <= 2 * W + 10; ++jx) {
                const int x0 = (int)floor(ada_coord(jx, jy, q.g[0], q.g[1], q.g[2], W, H, q.mx0, q.mx1));
                const int y0 = (int)floor(ada_coord(jy, jx, q.g[4], q.g[3], q.g[5], H, W, q.my0, q.my1));
                for (int k = 0; k < 4; ++k) {
                    const int vx = x0 + (k & 1), vy = y0 + (k >> 1);
                    if (vx < 0 || vx >= 2 * wp || vy < 0 || vy >= 2 * hp) continue;
                    int jx0, jx1, jy0, jy1;
                    ada_gather_window(m, vx, vy, H, W, jx0, jx1, jy0, jy1);
                    ++touched;
                    if (jx < jx0 || jx > jx1 || jy < jy0 || jy > jy1) ++bad;
                    const long size = (long)max(jx1 - jx0 + 1, 0) * max(jy1 - jy0 + 1, 0);
                    largest = size > largest ? size : largest;
                }
            }
        std::printf("1 %ld %ld %ld\n", touched, bad, largest);
    }
    return 0;
}
