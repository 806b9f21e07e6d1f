"""The transpose of the ADA geometry + colour operator written out factor by factor, ``P^T U^T S^T D^T C^T``, in the dtype of ``w`` on the CPU:
the index conventions of the gather-form adjoint (``csrc/ada.hip``: ada_cot_kernel, ada_gather_kernel) pinned against autograd of the
literal restatement (``tests/ada_f64.py``) by ``tests/test_ada_gather_cpu.py``.  Shares no code with the package.

    C^T   the colour matrix transposed on channels (first, count)
    D^T   sample j (1-based, 2n + 10 per axis) collects f[t] gy[(j - 1 - t) / 2] over the taps t of the parity of j - 1
    S^T   sample q at upsampled coordinate c adds 2 (1 - t) / 2 t per axis to the upsampled pixels floor(c) / floor(c) + 1 inside the image
    U^T   gP[i] = sum_o gU[o] f[o - 2 i + 5]
    P^T   source index y collects the padded indices m0 + y, m0 - y (y >= 1) and m0 + 2 (n - 1) - y (y <= n - 2) inside [0, n + m0 + m1)"""
import torch

from ada_f64 import hz_geom


def color_t(w, C34, channels):
    first, count = channels
    C34 = C34.to(w.dtype)
    g = w.clone()
    if count == 3:
        g[:, first:first + 3] = torch.einsum('nrj,nrhw->njhw', C34[:, :, :3], w[:, first:first + 3])
    else:
        g[:, first] = w[:, first] * C34[:, :, :3].sum(dim=2).mean(dim=1).reshape(-1, 1, 1)
    return g


def decimate_t(g, f):
    """[N,C,H,W] -> [N,C,2H+10,2W+10]; element s = j - 1."""
    N, C, H, W = g.shape
    a = g.new_zeros(N, C, 2 * H + 10, W)
    for t in range(12):
        a[:, :, t:t + 2 * H:2] += f[t] * g
    b = g.new_zeros(N, C, 2 * H + 10, 2 * W + 10)
    for t in range(12):
        b[:, :, :, t:t + 2 * W:2] += f[t] * a
    return b


def coords(G, H, W, margins):
    """upsampled-pixel coordinates of every sample of one image, (cx, cy) each [2H+10, 2W+10], in G's dtype, clamped as the kernels do."""
    mx0, my0, mx1, my1 = margins
    dt = G.dtype
    jx = torch.arange(1, 2 * W + 11, dtype=dt).reshape(1, -1)
    jy = torch.arange(1, 2 * H + 11, dtype=dt).reshape(-1, 1)
    ux, uy = 0.5 * (jx - W - 5), 0.5 * (jy - H - 5)
    wp, hp = W + mx0 + mx1, H + my0 + my1
    cx = 2 * (G[0, 0] * ux + G[0, 1] * uy + G[0, 2]) + (mx0 - mx1) + wp - 1
    cy = 2 * (G[1, 1] * uy + G[1, 0] * ux + G[1, 2]) + (my0 - my1) + hp - 1
    cx = torch.nan_to_num(cx, nan=-4.0).clamp(-4, 2 * wp + 4)
    cy = torch.nan_to_num(cy, nan=-4.0).clamp(-4, 2 * hp + 4)
    return cx, cy


def sample_t(gs, G, H, W, margins):
    """[C,2H+10,2W+10] of one image -> gU [C, 2 hp, 2 wp]."""
    mx0, my0, mx1, my1 = margins
    wp, hp = W + mx0 + mx1, H + my0 + my1
    cx, cy = coords(G, H, W, margins)
    fx, fy = cx.floor(), cy.floor()
    tx, ty = cx - fx, cy - fy
    x0, y0 = fx.long(), fy.long()
    C = gs.shape[0]
    gU = gs.new_zeros(C, 2 * hp * 2 * wp)
    for dy, wy in ((0, 2 * (1 - ty)), (1, 2 * ty)):
        for dx, wx in ((0, 2 * (1 - tx)), (1, 2 * tx)):
            vx, vy = x0 + dx, y0 + dy
            ok = (vx >= 0) & (vx < 2 * wp) & (vy >= 0) & (vy < 2 * hp)
            at = (vy.clamp(0, 2 * hp - 1) * (2 * wp) + vx.clamp(0, 2 * wp - 1)).reshape(-1)
            gU.index_add_(1, at, (gs * (wx * wy * ok)).reshape(C, -1))
    return gU.reshape(C, 2 * hp, 2 * wp)


def upsample_t(gU, f):
    """[C, 2 hp, 2 wp] -> gP [C, hp, wp]: gP[i] = sum_t gU[2 i - 5 + t] f[t]."""
    C, h2, w2 = gU.shape
    z = torch.nn.functional.pad(gU, [5, 6, 5, 6])
    a = gU.new_zeros(C, h2 // 2, w2 + 11)
    for t in range(12):
        a += f[t] * z[:, t:t + h2:2]
    b = gU.new_zeros(C, h2 // 2, w2 // 2)
    for t in range(12):
        b += f[t] * a[:, :, t:t + w2:2]
    return b


def _fold(gP, dim, n, m0, m1):
    npad = n + m0 + m1
    out = gP.narrow(dim, m0, n).clone()
    for y in range(n):
        for ok, i in ((y >= 1, m0 - y), (y <= n - 2, m0 + 2 * (n - 1) - y)):
            if ok and 0 <= i < npad:
                out.select(dim, y).add_(gP.select(dim, i))
    return out


def pad_t(gP, H, W, margins):
    mx0, my0, mx1, my1 = margins
    return _fold(_fold(gP, 1, H, my0, my1), 2, W, mx0, mx1)


def adjoint(w, G_inv=None, C34=None, channels=None, margins=None):
    """A^T w in w's dtype, the factors above in turn (geometry when G_inv is given, colour when C34 is)."""
    g = color_t(w, C34, channels) if C34 is not None else w
    if G_inv is None:
        return g
    N, C, H, W = w.shape
    f = hz_geom(w.dtype)
    gs = decimate_t(g, f)
    return torch.stack([pad_t(upsample_t(sample_t(gs[n], G_inv[n].to(w.dtype), H, W, margins), f), H, W, margins) for n in range(N)])
