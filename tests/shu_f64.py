"""Float64 restatement of the Spectral Hint Unit kernels, csrc/shu.hip (host only: numpy, no FFT library).

Written from the reference's SHU.forward (lib/model_zoo/shgan.py:312-336), its heterogeneous_filter (:143-160) and the header comments of
shu.hip, as explicit products with float64 cosine / sine matrices: nothing here calls ``torch.fft``, which tests/test_shu_f64_cpu.py uses
as the independent cross-check.  Every operator has a *magnitude twin* (``mag=True``): the same sums with |cos|, |sin|, |weights| applied to
|input| and every sign made a plus, i.e. the sum of the absolute values of the terms that meet in an output element, ``A_e``.  The GPU table
(tests/test_gpu_shu_edges.py) judges every element on its own:  |got - ref| <= k * 2^-24 * A_e  with k the number of float32 roundings on
the longest path to the element (``fwd_k`` / ``split_k`` / ``adjoint_k`` / ``spectral_bar`` below, counted from the kernels' arithmetic).
The cosine / sine tables hold exact 0 and +-1 at the quarter turns (as ``sincospif`` returns them), so an element whose terms all vanish
has A_e = 0 and must come back as an exact zero.

``defect=`` builds a float64 stand-in with one deliberate mistake; tests/test_shu_f64_cpu.py shows that each of them lies at least 100 bars
away from the restatement on a named case of the GPU table.  The defects:
  rowshift     forward: DC lands on row S/2 instead of S/2 - 1
  twiddle      forward: the table index (k * w) mod S is one too high at k = S/2, w = 1
  nyq_col      forward: column S/2 (the VALU column of the matrix-core kernels) is left at zero
  imoff        the Im planes sit one channel off (the plane offset C of [Re | Im]); invisible at C = 1
  c2r_im       split: Im of the DC and Nyquist columns is not dropped after the pass along y (with exact twiddles sin(0) = sin(pi x) = 0
               would hide a leak, so the stand-in lets them in with the cosine factor)
  colweight    split and adjoint: interior columns count once instead of twice
  crop         split and adjoint: the crop starts one row late
  unshift      split and adjoint: the un-shift is (j + r/2) mod r instead of (j + r/2 - 1) mod r
  band_drop    split and spectral: band B - 1 is left out of the band sum
  chan_order   split and spectral: flat channel k * O + o instead of o * B + k
  tail         spectral: the positions of a partial last tile of 64 are left at zero
  skip         split: a skipped scalar level does not advance the offset into the staged Gaussian tables (the levels after it read the
               slot before theirs) -- a skipped level that still counts
  acc_overwrite  split: ``accumulate`` stores the new value instead of adding it"""
import numpy as np

U32 = 2.0 ** -24                   # unit round-off of float32
TW = 4                             # a twiddle of the sincospif table is within 2 ulp = 4 units of 2^-24 of the true value


def f64(a):
    if a is None:
        return None
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def tables(size):
    """cos / sin of 2 pi m / size, m = 0 .. size-1, exact at the quarter turns."""
    m = np.arange(size)
    c, s = np.cos(2.0 * np.pi * m / size), np.sin(2.0 * np.pi * m / size)
    q = size // 4
    c[0], c[q], c[2 * q], c[3 * q] = 1.0, 0.0, -1.0, 0.0
    s[0], s[q], s[2 * q], s[3 * q] = 0.0, 1.0, 0.0, -1.0
    return c, s


def dft_mats(size, rows, cols, mag=False):
    """cos / sin of 2 pi rows[a] cols[b] / size as two [len(rows), len(cols)] matrices (the index is reduced mod size in integers)."""
    c, s = tables(size)
    idx = (np.asarray(rows)[:, None] * np.asarray(cols)[None, :]) % size
    return (np.abs(c[idx]), np.abs(s[idx])) if mag else (c[idx], s[idx])


# ------------------------------------------------------------------------------------------------
# forward transform
# ------------------------------------------------------------------------------------------------

def rfft2_shift(x, defect=None, mag=False):
    """x [N,C,S,S] -> [N,2C,S,S/2+1]: Re planes then Im planes of sum_hw x[h,w] e^{-2 pi i (u h + k w) / S} / S^2, frequency u on row
    (u + S/2 - 1) mod S (shgan.py:313-319)."""
    x = f64(x)
    size, nh = x.shape[-1], x.shape[-1] // 2 + 1
    c, s = tables(size)
    iw = (np.arange(nh)[:, None] * np.arange(size)[None, :]) % size            # [k, w]
    if defect == 'twiddle':
        iw[size // 2, 1] = (iw[size // 2, 1] + 1) % size
    iu = (np.arange(size)[:, None] * np.arange(size)[None, :]) % size          # [u, h]
    cw_, sw_, cu, su = c[iw], s[iw], c[iu], s[iu]
    sg = -1.0
    if mag:
        x, cw_, sw_, cu, su, sg = np.abs(x), np.abs(cw_), np.abs(sw_), np.abs(cu), np.abs(su), 1.0
    rr = np.einsum('nchw,kw->nchk', x, cw_)
    ri = sg * np.einsum('nchw,kw->nchk', x, sw_)
    tre = np.einsum('uh,nchk->ncuk', cu, rr) + np.einsum('uh,nchk->ncuk', su, ri)
    tim = np.einsum('uh,nchk->ncuk', cu, ri) + sg * np.einsum('uh,nchk->ncuk', su, rr)
    tre, tim = tre / (size * size), tim / (size * size)
    if defect == 'nyq_col':
        tre[..., size // 2] = 0.0
        tim[..., size // 2] = 0.0
    shift = size // 2 - 1 + (1 if defect == 'rowshift' else 0)
    tre, tim = np.roll(tre, shift, axis=2), np.roll(tim, shift, axis=2)
    if defect == 'imoff':
        tim = np.roll(tim, 1, axis=1)
    return np.concatenate([tre, tim], axis=1)


def fwd_k(size):
    """Roundings on the longest path of shu_rfft2_shift_kernel / shu_rfft2_shift_n_kernel<size>.
    size >= 64 (matrix cores): pass 1 one product + a chain of S additions + table = S + 1 + TW; pass 2 (K = 2S) 2S + 1 + TW; scale 1.
    size < 64 (scalar): pass 1 S + 1 + TW; pass 2 product, inner add, S additions + table = S + 2 + TW; scale 1."""
    return 3 * size + 3 + 2 * TW if size >= 64 else 2 * size + 4 + 2 * TW


# ------------------------------------------------------------------------------------------------
# spectral stage
# ------------------------------------------------------------------------------------------------

def _spectral_parts(t_in, w0, b0, w1, cw, defect=None):
    t_in, w0, b0, w1, cw = f64(t_in), f64(w0), f64(b0), f64(w1), f64(cw)
    n, ch = t_in.shape[:2]
    p = int(np.prod(t_in.shape[2:]))
    bands = cw.shape[0]
    w1r = w1.reshape(bands, ch, ch).transpose(1, 0, 2) if defect == 'chan_order' else w1.reshape(ch, bands, ch)       # [o, k, i]
    cwf = cw.reshape(bands, p).copy()
    if defect == 'band_drop':
        cwf[bands - 1] = 0.0
    return t_in.reshape(n, ch, p), w0, b0, w1r.reshape(ch, bands * ch), cwf, (n, ch, p, bands)


def _band_gemm(w1m, cwf, t):
    n, ch, p = t.shape
    z = (cwf[None, :, None, :] * t[:, None, :, :]).reshape(n, cwf.shape[0] * ch, p)            # [n, (k, i), p]
    return np.matmul(w1m[None], z)


def spectral(t_in, w0, b0, w1, cw, defect=None):
    """t_in [N,64,h,w]; w0 [64,64]; b0 [64]; w1 [64*B,64] with flat row o*B + k (shgan.py:157-158); cw [B,h,w] ->
    S[n,o,p] = sum_k cw[k,p] sum_i w1[o*B+k,i] relu(sum_j w0[i,j] T[n,j,p] + b0[i])   (shgan.py:320-321, :143-160)."""
    t, w0, b0, w1m, cwf, (n, ch, p, _) = _spectral_parts(t_in, w0, b0, w1, cw, defect)
    hid = np.maximum(np.matmul(w0[None], t) + b0[None, :, None], 0.0)
    out = _band_gemm(w1m, cwf, hid)
    if defect == 'tail':
        out[..., (p // 64) * 64:] = 0.0
    return out.reshape(np.shape(t_in))


def spectral_bar(t_in, w0, b0, w1, cw):
    """The bar of shu_spectral_kernel / shu_spectral_tail_kernel per element, in absolute units.  The ReLU is handled by carrying the first
    stage's bound through it (it is 1-Lipschitz), not by exact inputs:
      stage 1: K = 64 on the matrix cores, 64 + 1 roundings, the bias addition 1:  |t_gpu - t| <= E1 = 66 u (|w0| |T| + |b0|)
      stage 2: cw * t one rounding, K = 64 B on the matrix cores 64 B + 1:        (64 B + 2) u |w1| (|cw| (|t| + E1))  +  |w1| (|cw| E1)"""
    t, w0, b0, w1m, cwf, (n, ch, p, bands) = _spectral_parts(t_in, w0, b0, w1, cw)
    a1 = np.matmul(np.abs(w0)[None], np.abs(t)) + np.abs(b0)[None, :, None]
    e1 = 66 * U32 * a1
    hid = np.maximum(np.matmul(w0[None], t) + b0[None, :, None], 0.0)
    bar = (64 * bands + 2) * U32 * _band_gemm(np.abs(w1m), np.abs(cwf), hid + e1) + _band_gemm(np.abs(w1m), np.abs(cwf), e1)
    return bar.reshape(np.shape(t_in))


# ------------------------------------------------------------------------------------------------
# split stage and its adjoint
# ------------------------------------------------------------------------------------------------

def _colweight(r, defect=None):
    w = np.full(r // 2 + 1, 1.0 if defect == 'colweight' else 2.0)
    w[0] = w[r // 2] = 1.0
    return w


def _geometry(size, r, defect=None):
    """rows of the crop (index a = 0 .. r-1 -> row of the spectrum) and the un-shift j -> a."""
    crop = size // 2 - r // 2 + (1 if defect == 'crop' else 0)
    rows = (crop + np.arange(r)) % size
    a_of_j = (np.arange(r) + r // 2 - 1 + (1 if defect == 'unshift' else 0)) % r
    return rows, a_of_j


def band_sum(y, cw, defect=None, mag=False):
    """y [N,2C*B,S,S/2+1] (flat channel o*B + k, o = Re planes then Im planes) -> (Re, Im) [N,C,S,S/2+1] each."""
    y = f64(y)
    bands = 1 if cw is None else cw.shape[0]
    n, ch, size, nh = y.shape
    c = ch // (2 * bands)
    if defect == 'chan_order':
        yr = y.reshape(n, bands, 2, c, size, nh).transpose(0, 2, 3, 1, 4, 5)
    else:
        yr = y.reshape(n, 2, c, bands, size, nh)
    w = np.ones((1, size, nh)) if cw is None else f64(cw).copy()
    if defect == 'band_drop':
        w[bands - 1] = 0.0
    if mag:
        yr, w = np.abs(yr), np.abs(w)
    sre, sim = (yr[:, 0] * w[None, None]).sum(2), (yr[:, 1] * w[None, None]).sum(2)
    if defect == 'imoff':
        sim = np.roll(sim, 1, axis=1)
    return sre, sim


def split_irfft2(y, cw, gauss, res, accumulate_into=None, skip=(), defect=None, mag=False):
    """-> one [N,C,r,r] array per level of ``res`` (None where skipped): band sum, crop of rows S/2 - r/2 .. S/2 + r/2 and columns
    0 .. r/2, Gaussian weight, row un-shift, inverse DFT along y, c2r along x (Im of columns 0 and r/2 dropped, interior columns twice);
    no scale (norm='forward').  shgan.py:326-334.  With ``mag`` the |old| of ``accumulate_into`` is NOT included (the caller adds it)."""
    sre, sim = band_sum(y, cw, defect, mag)
    size = sre.shape[2]
    tabs = [f64(g) for g in gauss]
    if defect == 'skip':
        # the staged tables of the scalar levels, read at an offset that only the levels not skipped advance
        cnt = [r * (r // 2 + 1) if r < 64 else 0 for r in res]
        gl = np.concatenate([np.zeros(c_) if l in skip else tabs[l].reshape(-1)[:c_] for l, c_ in enumerate(cnt)] + [np.zeros(1)])
        off = 0
        for l, r in enumerate(res):
            if r < 64 and l not in skip:
                tabs[l] = gl[off:off + cnt[l]].reshape(r, r // 2 + 1)
                off += cnt[l]
    outs = []
    for l, r in enumerate(res):
        if l in skip:
            outs.append(None)
            continue
        rh = r // 2 + 1
        rows, a_of_j = _geometry(size, r, defect)
        g = np.abs(tabs[l]) if mag else tabs[l]
        vre, vim = (sre[:, :, rows, :rh] * g)[:, :, a_of_j], (sim[:, :, rows, :rh] * g)[:, :, a_of_j]        # [n, c, j, w]
        cy, sy = dft_mats(r, np.arange(r), np.arange(r), mag)                                              # [y, j]
        sg = 1.0 if mag else -1.0
        zre = np.einsum('yj,ncjw->ncyw', cy, vre) + sg * np.einsum('yj,ncjw->ncyw', sy, vim)                # e^{+i theta}
        zim = np.einsum('yj,ncjw->ncyw', sy, vre) + np.einsum('yj,ncjw->ncyw', cy, vim)
        cx, sx = dft_mats(r, np.arange(rh), np.arange(r), mag)                                             # [w, x]
        wre = _colweight(r, defect)
        wim = wre.copy()
        wim[0] = wim[r // 2] = 0.0
        out = np.einsum('ncyw,wx->ncyx', zre * wre, cx) + sg * np.einsum('ncyw,wx->ncyx', zim * wim, sx)
        if defect == 'c2r_im':
            out = out + zim[..., 0][..., None] + zim[..., r // 2][..., None] * cx[r // 2][None, None, None, :]
        if accumulate_into is not None and not mag and defect != 'acc_overwrite':
            out = f64(accumulate_into[l]) + out
        outs.append(out)
    return outs


def split_k(r, bands):
    """Roundings on the longest path of one level of shu_split_irfft2_kernel / shu_split_irfft2_n_kernel (accumulate's addition included).
    band sum: B products + B additions on a term's path = B + 1 (B == 1: the weight is 1.f and the sum starts at 0: nothing);
    r < 64 (scalar): along y product, subtraction, Gaussian weight, r additions + table = r + 3 + TW; along x product, subtraction, at most
                     r/2 additions + table = r/2 + 2 + TW (the factor 2 is exact); accumulate 1;
    r >= 64 (matrix cores): Gaussian weight 1; pass A (K = 2r) 2r + 1 + TW; pass B (K = r; the operand 2 cos is exact) r + 1 + TW;
                     accumulate 1."""
    band = bands + 1 if bands > 1 else 0
    if r < 64:
        return band + (r + 3 + TW) + (r // 2 + 2 + TW) + 1
    return band + 1 + (2 * r + 1 + TW) + (r + 1 + TW) + 1


def split_adjoint(grads, gauss, res, size=None, defect=None, mag=False, per_level=False):
    """The transpose of ``split_irfft2`` at bands = 1, as a formula of its own (header of shu_split_adjoint_kernel): with D = the forward
    DFT (e^{-i theta}) of the real gradient plane G_r along x (half spectrum) and y,
      GS[S/2 - r/2 + j][kx] += gauss_r[j][kx] * c_kx * D[ky][kx],   j = (ky + r/2 - 1) mod r,  c_0 = c_{r/2} = 1, else 2
    summed over the levels with a gradient -> [N,2C,S,S/2+1] (Re planes, Im planes).  ``per_level``: the list of the levels' shares."""
    size = res[-1] if size is None else size             # (the top level is the transform size)
    live = [f64(g) for g in grads if g is not None]
    n, c = live[0].shape[:2] if live else (0, 0)
    nh = size // 2 + 1
    total, shares = np.zeros((n, 2 * c, size, nh)), []
    for l, r in enumerate(res):
        if grads[l] is None:
            shares.append(None)
            continue
        g, rh = f64(grads[l]), r // 2 + 1
        tab = f64(gauss[l])
        if mag:
            g, tab = np.abs(g), np.abs(tab)
        sg = 1.0 if mag else -1.0
        cx, sx = dft_mats(r, np.arange(rh), np.arange(r), mag)                     # [kx, x]
        t1re, t1im = np.einsum('ncyx,kx->ncyk', g, cx), sg * np.einsum('ncyx,kx->ncyk', g, sx)
        cy, sy = dft_mats(r, np.arange(r), np.arange(r), mag)                      # [ky, y]
        dre = np.einsum('qy,ncyk->ncqk', cy, t1re) + np.einsum('qy,ncyk->ncqk', sy, t1im)
        dim = np.einsum('qy,ncyk->ncqk', cy, t1im) + sg * np.einsum('qy,ncyk->ncqk', sy, t1re)
        rows, a_of_j = _geometry(size, r, defect)                                  # j = a_of_j[ky]
        wgt = tab[a_of_j] * _colweight(r, defect)[None, :]                         # [ky, kx]
        share = np.zeros_like(total)
        share[:, :c, rows[a_of_j], :rh] = dre * wgt
        share[:, c:, rows[a_of_j], :rh] = dim * wgt
        if defect == 'imoff':
            share[:, c:] = np.roll(share[:, c:], 1, axis=1)
        shares.append(share)
        total += share
    return shares if per_level else total


def adjoint_k(r, levels):
    """Roundings on the longest path of one level's share in shu_split_adjoint_kernel / shu_split_adjoint_n_kernel (all levels scalar):
    along x product + r additions + table = r + 1 + TW; along y product, inner addition, r additions + table = r + 2 + TW; the weight
    (2 gauss is exact) 1; the sum over the levels in LDS at most ``levels`` additions."""
    return (r + 1 + TW) + (r + 2 + TW) + 1 + levels


def adjoint_bar(grads, gauss, res, size=None):
    """sum over the levels of adjoint_k * 2^-24 * A_level, per element of [N,2C,S,S/2+1]."""
    shares = split_adjoint(grads, gauss, res, size, mag=True, per_level=True)
    nl = sum(s is not None for s in shares)
    return sum(adjoint_k(r, nl) * U32 * s for r, s in zip(res, shares) if s is not None)


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------

def worst_ratio(got, ref, bar):
    """-> (max over the elements of |got - ref| / bar, its index); an element with bar == 0 must be exact (ratio inf otherwise)."""
    got, ref, bar = f64(got), f64(ref), np.broadcast_to(f64(bar), np.shape(ref))
    if not np.isfinite(got).all():
        bad = np.argwhere(~np.isfinite(got))[0]
        return float('inf'), tuple(int(v) for v in bad)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), tuple(int(v) for v in np.unravel_index(k, ratio.shape))
