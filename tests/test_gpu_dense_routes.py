"""Route table of the dense / style family, csrc/dense.hip (run with -m gpu on an MI355X).

Every entry point of the family at the edges of its kernels: both sides of each dispatch predicate (the kernel or instantiation that must
serve a case is named, the others forbidden), sizes off every tile multiple, the argument limits, pitched rows through the C ABI, every
null-operand branch, tied row maxima.  Results are compared with the float64 restatement tests/dense_f64.py (itself checked on the CPU by
tests/test_dense_f64_cpu.py):
  * linear products elementwise against c 2^-24 sum|a||b| with c the longest float32 addition chain of the kernel's summation order;
  * everything else per output and per row (max|diff| / max|ref| of the row) against the project's figures for the same quantities
    (1e-5 dense and demodulation, 2e-5 style factors, 1e-6 normalize_2nd_moment);
  * every output buffer is filled with a sentinel first: pad columns and guard rows must keep it, real elements must lose it.
The last test checks that the table covers every kernel and instantiation launched from dense.hip."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import dense_f64 as ref
from conftest import ROOT, rel_err
from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL_DENSE = 1e-5         # dense with activation, demodulated weights and their gradient (tests/test_gpu_ops.py, test_fused_demodulation_weight_kernel_vs_tensor_ops)
TOL_STYLE = 2e-5         # style factors and their gradients (test_fused_style_factors_vs_float64_autograd)
TOL_STYLE2 = 5e-5        # their closed double backward (test_closed_double_backward_of_the_style_factors_vs_float64_autograd)
TOL_NORM = 1e-6          # normalize_2nd_moment (test_dense_large_and_normalize)
SENT_BITS = 0x7A5C3B1D   # the sentinel: a finite float32 (2.86e35) no kernel here produces
SENT = float(np.array([SENT_BITS], np.uint32).view(np.float32)[0])


def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def _lib():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib as lib
    return lib


def rnd(seed, *shape, lo=None):
    rs = np.random.RandomState(seed)
    a = rs.rand(*shape) + lo if lo is not None else rs.standard_normal(shape)
    return torch.from_numpy(a.astype(np.float32))


class Out:
    """An output buffer of ``rows`` x ``cols`` floats with ``pad`` extra columns per row (the row pitch of the C ABI) and one guard row, all
    filled with the sentinel; ``view`` is what the kernel writes."""
    def __init__(self, rows, cols, pad=0):
        self.rows, self.cols, self.ld = rows, cols, cols + pad
        self.buf = torch.full((rows + 1, self.ld), SENT, device=DEV)
        self.view = self.buf[:rows, :cols]

    def check(self, name, written=True):
        bits = self.buf.cpu().view(torch.int32)
        keep = torch.ones_like(bits, dtype=torch.bool)
        keep[:self.rows, :self.cols] = False
        assert bool((bits[keep] == SENT_BITS).all()), f'{name}: written outside the output ({int((bits[keep] != SENT_BITS).sum())} elements)'
        real = self.buf[:self.rows, :self.cols].cpu()
        if written:
            assert bool(torch.isfinite(real).all()), f'{name}: not finite'
            assert bool((real.view(torch.int32) != SENT_BITS).all()), f'{name}: elements left unwritten'
        else:
            assert bool((real.view(torch.int32) == SENT_BITS).all()), f'{name}: written, but no output was requested'
        return real.double()


def pitched(t, pad):
    """t [R, C] on the GPU as a view of rows pitched by ``pad`` extra floats (NaN in the pad: a read of it poisons the result)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float('nan'), device=DEV)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cabi(name, *args):
    """One call of the C ABI on the current stream; a negative status raises ShgError."""
    lib = _lib()
    lib.check(getattr(lib.get_lib(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def lin(name, got, want, absprod, c, extra=None):
    ratio, _ = ref.linear_excess(got, want, absprod, c, extra)
    return (f'{name}|err/bound(c={c})', ratio, 1.0)


def row(name, got, want, tol, scale=None):
    e, _ = ref.row_rel_err(got, want, scale)
    return (name, e, tol)


# ------------------------------------------------------------------------------------------------
# case builders: each returns (call, judge); the inputs are built before the probe, ``call()`` enqueues the entry point(s) and returns
# the buffers they write (whole, guard rows and pad columns included), ``judge()`` reads the outputs back and returns the records
# (name, measured, bound)
# ------------------------------------------------------------------------------------------------

def dense_case(n, k, o, bias=True, act=False, bgain=1.0, pad_y=0, pad_x=0, gain=1.0):
    """kernels.dense into ``out=`` (a column slice of a wider buffer with pad_y); with pad_x through the C ABI (ldx > K)."""
    kk = _kk()
    x, w, b = rnd(1, n, k), rnd(2, o, k), (rnd(3, o) if bias else None)
    wgain = 0.7 / math.sqrt(k)
    y = Out(n, o, pad_y)
    xd, wd, bd = (pitched(x.to(DEV), pad_x) if pad_x else x.to(DEV)), w.to(DEV), (b.to(DEV) if bias else None)
    if pad_x:
        a, al, g, cl = kk._act_args(act, gain)

        def call():
            cabi('shg_dense_f32', ptr(xd), ptr(wd), ptr(bd), ptr(y.view), n, k, o, k + pad_x, y.ld, wgain, bgain, a, al, g, cl)
            return [y.buf]
    else:
        def call():
            assert kk.dense(xd, wd, bd, wgain=wgain, bgain=bgain, act=act, gain=gain, out=y.view).data_ptr() == y.view.data_ptr()
            return [y.buf]

    def judge():
        got, want = y.check('y'), ref.dense(x, w, b, wgain, bgain, act, gain)
        if act:
            return [row('y', got, want, TOL_DENSE)]
        # c: a lane adds ceil(K / 64) products, the shuffle tree 6 partial sums, then the gain and the bias: ceil(K / 64) + 8 roundings
        absprod = x.double().abs() @ w.double().abs().t() * abs(wgain * gain)
        extra = (b.double() * bgain * gain).abs() * ref.U32 if bias else None
        return [lin('y', got, want, absprod, -(-k // 64) + 8, extra)]
    return call, judge


def matmul_nn_case(n, m, k, scale=0.37, pad_a=0, pad_o=0):
    a, b = rnd(4, n, m), rnd(5, m, k)
    out = Out(n, k, pad_o)
    ad, bd = (pitched(a.to(DEV), pad_a) if pad_a else a.to(DEV)), b.to(DEV)

    def call():
        cabi('shg_matmul_nn_f32', ptr(ad), ptr(bd), ptr(out.view), n, m, k, m + pad_a, out.ld, scale)
        return [out.buf]

    def judge():
        # c: a wave adds its slice of ceil(M / 16) products, 16 wave sums meet in LDS, then the scale: ceil(M / 16) + 18 with two to spare
        absprod = a.double().abs() @ b.double().abs() * abs(scale)
        return [lin('out', out.check('out'), ref.matmul_nn(a, b, scale), absprod, -(-m // 16) + 18)]
    return call, judge


def matmul_tn_case(n, m, k, colsum=True, scale=-1.3, pad_a=0, pad_b=0):
    a, b = rnd(6, n, m), rnd(7, n, k)
    out, col = Out(m, k), Out(1, m)
    ad, bd = (pitched(a.to(DEV), pad_a) if pad_a else a.to(DEV)), (pitched(b.to(DEV), pad_b) if pad_b else b.to(DEV))
    cs = 0.6

    def call():
        cabi('shg_matmul_tn_f32', ptr(ad), ptr(bd), ptr(out.view), ptr(col.view) if colsum else None, n, m, k, m + pad_a, k + pad_b, scale, cs)
        return [out.buf, col.buf]

    def judge():
        want, wcol = ref.matmul_tn(a, b, scale, cs if colsum else None)
        # c: a thread walks the batch, N additions, then the scale: N + 2 with one to spare
        recs = [lin('out', out.check('out'), want, a.double().abs().t() @ b.double().abs() * abs(scale), n + 2)]
        got_col = col.check('colsum', written=colsum)
        if colsum:
            recs.append(lin('colsum', got_col[0], wcol, a.double().abs().sum(0) * abs(cs), n + 2))
        return recs
    return call, judge


def normalize_case(n, k, zero_row=None):
    kk = _kk()
    x = rnd(8, n, k)
    if zero_row is not None:
        x[zero_row] = 0
    y = Out(n, k)
    xd = x.to(DEV)

    def call():
        cabi('shg_normalize_2nd_moment_f32', ptr(xd), ptr(y.view), n, k, 1e-8)
        return [y.buf]

    def judge():
        got = y.check('y')
        if zero_row is not None:
            assert not got[zero_row].any(), 'an all-zero row must come back zero'
        return [row('y', got, ref.normalize_2nd_moment(x), TOL_NORM),
                row('wrapper', kk.normalize_2nd_moment(xd).cpu(), ref.normalize_2nd_moment(x), TOL_NORM)]
    return call, judge


def demod_case(o, i, k, prenorm, bwd='both'):
    """shg_demod_weight_f32, then shg_demod_weight_backward_f32 on its outputs with both gradients / gwn NULL / gwsq NULL."""
    w, gwn, gwsq = rnd(9, o, i, k), rnd(10, o, i, k), rnd(11, o, i)
    wn, wsq, sfac, gw = Out(o, i * k), Out(o, i), Out(1, o), Out(o, i * k)
    wd = w.to(DEV)
    gnd, gqd = (gwn.to(DEV) if bwd != 'gwsq' else None), (gwsq.to(DEV) if bwd != 'gwn' else None)

    def call():
        cabi('shg_demod_weight_f32', ptr(wd), ptr(wn.view), ptr(wsq.view), ptr(sfac.view), o, i, k, int(prenorm))
        cabi('shg_demod_weight_backward_f32', ptr(wn.view), ptr(sfac.view), ptr(gnd), ptr(gqd), ptr(gw.view), o, i, k)
        return [wn.buf, wsq.buf, sfac.buf, gw.buf]

    def judge():
        rn, rq, rs = ref.demod_weight(w, prenorm)
        rg = ref.demod_weight_backward(rn, rs, None if gnd is None else gwn, None if gqd is None else gwsq)
        scale = None
        if i * k == 1:
            # one element per channel: wn = +-1 whatever w, the gradient is G - wn (G wn) = 0 exactly; judged against the terms that cancel
            g = (0 if gnd is None else gwn.double()) + (0 if gqd is None else 2 * gwsq.double()[:, :, None] * rn)
            scale = (rs[:, None, None] * g).abs().reshape(o)
        return [row('wn', wn.check('wn'), rn.reshape(o, -1), TOL_DENSE), row('wsq', wsq.check('wsq'), rq, TOL_DENSE),
                row('sfac', sfac.check('sfac')[0], rs, TOL_DENSE), row('gw', gw.check('gw'), rg.reshape(o, -1), TOL_DENSE, scale)]
    return call, judge


def style_case(n, i, o, prenorm, bwd='both', want_wsq=True, ties=False, fwd_d=True):
    """shg_style_factors_f32 and shg_style_factors_backward_f32 on its outputs: gradients on both outputs / gsn NULL / gd NULL, gwsq NULL
    (want_wsq False), d NULL in the forward (fwd_d False: no backward).  ``ties``: the tie rows of dense_f64.tie_styles."""
    info = {}
    if ties:
        s, info = ref.tie_styles(n, i, seed=5)
    else:
        s = rnd(12, n, i) + 1.0
    wsq = rnd(13, o, i, lo=0.0) * (2.0 / i)
    # (one style per row: a row of the outputs is ONE element, a sum over the batch; incoming gradients of one sign keep that sum free of
    # cancellation, so that the per-row figure measures the kernel and not the conditioning of the input)
    gsn, gd = (rnd(14, n, i, lo=0.5), rnd(15, n, o, lo=0.5)) if i == 1 else (rnd(14, n, i), rnd(15, n, o))
    sb = (o + 63) // 64
    sn, d, aux, gs, gw, part = Out(n, i), Out(n, o), Out(1, n + 1), Out(n, i), Out(o, i), Out(sb * n, i)
    g1 = Out(n, i)
    sd, wd = s.to(DEV), wsq.to(DEV)
    gsd, gdd = (gsn.to(DEV) if bwd != 'gd' else None), (gd.to(DEV) if bwd != 'gsn' else None)

    def call():
        cabi('shg_style_factors_f32', ptr(sd), ptr(wd) if fwd_d else None, ptr(sn.view), ptr(d.view) if fwd_d else None, ptr(aux.view), n, i, o,
             int(prenorm))
        if fwd_d:
            cabi('shg_style_factors_backward_f32', ptr(sn.view), ptr(d.view), ptr(wd), ptr(aux.view), ptr(gsd), ptr(gdd), ptr(gs.view),
                 ptr(gw.view) if want_wsq else None, ptr(part.view), n, i, o, int(prenorm))
        return [sn.buf, d.buf, aux.buf, gs.buf, gw.buf, part.buf]

    def judge():
        rsn, rd, raux = ref.style_factors(s, wsq, prenorm)
        gsn_gpu, aux_gpu = sn.check('sn'), aux.check('aux')[0]
        recs = [row('sn', gsn_gpu, rsn, TOL_STYLE), row('aux', aux_gpu, raux, TOL_STYLE)]
        assert torch.equal(aux_gpu[:n], raux[:n]), 'the row maxima are exact'
        got_d = d.check('d', written=fwd_d)
        if not fwd_d:
            return recs
        recs.append(row('d', got_d, rd, TOL_STYLE))
        rgs, rgw = ref.style_factors_backward(rsn, rd, wsq, raux, None if gsd is None else gsn, None if gdd is None else gd, prenorm)
        scale = None
        if prenorm and i == 1:
            # one style per row: s / |s| = +-1 whatever s, the gradient g1 / M - sign R / M = 0 exactly; judged against the terms that cancel
            scale = (ref.style_factors_backward(rsn, rd, wsq, raux, None if gsd is None else gsn, None if gdd is None else gd, False)[0]
                     / raux[:n, None]).abs().reshape(n)
        recs.append(row('gs', gs.check('gs'), rgs, TOL_STYLE, scale))
        got_gw = gw.check('gwsq', written=want_wsq)
        if want_wsq:
            recs.append(row('gwsq', got_gw, rgw, TOL_STYLE))
        part.check('partq')
        if ties:
            # the same backward without the pre-normalisation gives g1; what is left of gs - g1 / M is the share of the maximum's derivative
            cabi('shg_style_factors_backward_f32', ptr(sn.view), ptr(d.view), ptr(wd), ptr(aux.view), ptr(gsd), ptr(gdd), ptr(g1.view), None,
                 ptr(part.view), n, i, o, 0)
            torch.cuda.synchronize()
            corr, share = ref.tie_corrections(gsn_gpu, aux_gpu, gs.check('gs'), g1.check('g1'))
            rg1 = ref.style_factors_backward(rsn, rd, wsq, raux, None if gsd is None else gsn, None if gdd is None else gd, False)[0]
            _, rshare = ref.tie_corrections(rsn, raux, rgs, rg1)
            worst = 0.0
            for r_, (tied, runner_up) in info.items():
                lim = TOL_STYLE * float(rgs[r_].abs().max())
                assert abs(float(rshare[r_])) > 100 * lim, 'the tie rows need a correction far above the tolerance'
                for p in tied:
                    assert abs(float(corr[r_, p]) - float(rshare[r_])) <= lim, f'row {r_}: tied position {p} got {float(corr[r_, p])}, its share is {float(rshare[r_])}'
                    assert abs(float(corr[r_, p]) - float(corr[r_, tied[0]])) <= lim, f'row {r_}: unequal shares'
                    worst = max(worst, abs(float(corr[r_, p]) - float(rshare[r_])) / lim)
                rest = corr[r_].clone()
                rest[list(tied)] = 0
                assert float(rest.abs().max()) <= lim, f'row {r_}: position {int(rest.abs().argmax())} is below the maximum and got a share (runner-up: {runner_up})'
                worst = max(worst, float(rest.abs().max()) / lim)
            recs.append(('tie shares|err/tol', worst, 1.0))
        return recs
    return call, judge


def _autograd_style(fn, dt, s64, w64, a64, b64, A64, B64, dev):
    s, w, a, b = (t.to(dev, dt).clone().requires_grad_(True) for t in (s64, w64, a64, b64))
    with torch.enable_grad():
        sn, d = fn(s, w)
        gs, gw = torch.autograd.grad([sn, d], [s, w], [a, b], create_graph=True)
        phi = (gs * A64.to(dev, dt)).sum() + (gw * B64.to(dev, dt)).sum()
        return [sn.detach(), d.detach(), gs.detach(), gw.detach()] + list(torch.autograd.grad(phi, [s, w, a, b]))


def style_fn_case(n, i, o, half):
    """``_StyleFactorsFn`` end to end: both outputs, both first-order gradients and the closed double backward against float64 autograd of
    the tensor-op formulation (the protocol and tolerances of tests/test_gpu_train_graph.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd.model_zoo import stylegan as sg
    g = torch.Generator().manual_seed(n * 977 + i + 3 * o)
    mk = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)          # noqa: E731
    s64, w64 = mk(n, i) + 1.0, torch.rand(o, i, generator=g, dtype=torch.float64) * 0.01
    rest = mk(n, i), mk(n, o), mk(n, i), mk(o, i)

    def composed(s, w):
        if half:
            s = s / s.norm(float('inf'), dim=1, keepdim=True)
        s = s * s.square().mean().rsqrt()
        return s, (s.square().matmul(w.t()) + 1e-8).rsqrt()
    want = _autograd_style(composed, torch.float64, s64, w64, *rest, 'cpu')
    got = []

    def call():
        assert sg.CLOSED_STYLE_FACTORS_BACKWARD
        got[:] = _autograd_style(lambda s, w: sg._StyleFactorsFn.apply(s, w, half), torch.float32, s64, w64, *rest, DEV)
        return list(got)

    def judge():
        names = ('sn', 'd', 'g_styles', 'g_wsq', '2nd:styles', '2nd:wsq', '2nd:g_sn', '2nd:g_d')
        return [(nm, rel_err(x.double().cpu(), y), TOL_STYLE if k < 4 else TOL_STYLE2) for k, (nm, x, y) in enumerate(zip(names, got, want))]
    return call, judge


def modulation_n33_case(half):
    """``_modulation_factors`` at N = 33, beyond the fused kernels' limit: the composed form serves it (under autograd), no style_factors kernel."""
    import shgan_amd  # noqa: F401
    from shgan_amd.model_zoo import stylegan as sg
    n, i, o = 33, 40, 9
    s, wsq, a, b = rnd(16, n, i) + 1.0, rnd(17, o, i, lo=0.0) * (2.0 / i), rnd(18, n, i), rnd(19, n, o)
    got = []

    def call():
        with torch.enable_grad():
            sd, wd = s.to(DEV).requires_grad_(True), wsq.to(DEV).requires_grad_(True)
            assert not _kk().style_factors_supported(sd, wd)
            _, sn, d = sg._modulation_factors(half, None, sd, True, wfac=(None, wd))
            got[:] = [sn.detach(), d.detach()] + list(torch.autograd.grad((sn * a.to(DEV)).sum() + (d * b.to(DEV)).sum(), [sd, wd]))
        return list(got)

    def judge():
        rsn, rd, raux = ref.style_factors(s, wsq, half)
        rgs, rgw = ref.style_factors_backward(rsn, rd, wsq, raux, a, b, half)
        return [row(nm, x.cpu(), y, TOL_STYLE) for nm, x, y in zip(('sn', 'd', 'gs', 'gwsq'), got, (rsn, rd, rgs, rgw))]
    return call, judge


def style_prep_case(n, i, o, demod=True, pre_gain=1.0, pad=0):
    """shg_modconv_style_prep_f32 on the [I][OP] table of kernels.conv_weight_prep (read back: the kernel's own input)."""
    kk = _kk()
    st = rnd(20, n, i) + 1.0
    pw = kk.conv_weight_prep(rnd(21, o, i, 1, 1).to(DEV), demod=True) if demod else None
    s_out, d_out = Out(n, i), Out(n, max(o, 1))
    sd = pitched(st.to(DEV), pad) if pad else st.to(DEV)
    op = pw.op if demod else 0

    def call():
        cabi('shg_modconv_style_prep_f32', ptr(sd), i + pad, ptr(pw.wsq) if demod else None, ptr(s_out.view), ptr(d_out.view) if demod else None, n, i,
             o if demod else 0, op, int(demod), pre_gain)
        return [s_out.buf, d_out.buf]

    def judge():
        table = pw.wsq.cpu().double().reshape(i, op) if demod else None
        rs, rd = ref.modconv_style_prep(st, table, o, demod, pre_gain)
        recs = [row('s', s_out.check('s'), rs, TOL_DENSE)]
        got_d = d_out.check('d', written=demod)
        if demod:
            w64 = ref.demod_weight(rnd(21, o, i, 1, 1))[1].t()                     # the table itself: sum_k wn^2, transposed
            recs += [row('d', got_d, rd, TOL_DENSE), row('wsq table', table[:, :o], w64, TOL_DENSE)]
            assert not table[:, o:].any(), 'pad columns of the table are zero'
            ws, wd_ = kk.modconv_style_prep(st.to(DEV), pw, demod=True, pre_gain=pre_gain)
            recs += [row('wrapper s', ws.cpu(), rs, TOL_DENSE), row('wrapper d', wd_.cpu(), rd, TOL_DENSE)]
        return recs
    return call, judge


def grouped_case(n, items=33):
    """kernels.dense_grouped and kernels.modconv_style_prep_grouped over ``items`` layers (more than 32: two launches each): the style rows
    are column slices of one buffer; every third group has no second source (x2 None, K2 = 0); group 1 has one output feature."""
    kk = _kk()
    k1, k2 = 48, 80
    ws, w0 = rnd(22, n, items, k1), rnd(23, n, k2)
    dims = [(1 if g == 1 else (5, 64, 33, 70)[g % 4], (9, 1, 65)[g % 3], g % 5 != 4) for g in range(items)]     # (I, O, demod)
    wsd, w0d = ws.to(DEV), w0.to(DEV)
    raw = Out(n, sum(d[0] for d in dims) + 2 * items)
    d_items, p_items, recs_in = [], [], []
    off = 1
    for g, (i_n, o_n, demod) in enumerate(dims):
        two = g % 3 != 2
        aw, ab = rnd(100 + g, i_n, k1 + (k2 if two else 0)), (rnd(200 + g, i_n) if g % 2 == 0 else None)
        pw = kk.conv_weight_prep(rnd(300 + g, o_n, i_n, 1, 1).to(DEV), demod=True) if demod else None
        st = raw.buf[:n, off:off + i_n]
        d_items.append(dict(x1=wsd[:, g, :], x2=w0d if two else None, w=aw.to(DEV), b=None if ab is None else ab.to(DEV), y=st, wgain=0.3, bgain=1.5))
        s_o, d_o = Out(n, i_n), (Out(n, o_n) if demod else None)
        p_items.append(dict(styles=st, pw=pw, demod=demod, pre_gain=1.0 if demod else 0.25, s=s_o.view[:, :], d=d_o.view[:, :] if demod else None))
        recs_in.append((off, i_n, o_n, demod, two, aw, ab, pw, s_o, d_o))
        off += i_n + 2
    # (s / d of an item must be contiguous: an Out without pad columns is, its guard row follows the last real row)

    def call():
        kk.dense_grouped(d_items)
        kk.modconv_style_prep_grouped(p_items)
        return [raw.buf] + [r[8].buf for r in recs_in] + [r[9].buf for r in recs_in if r[9] is not None]

    def judge():
        buf = raw.buf.cpu()
        bits = buf.view(torch.int32)
        keep = torch.ones_like(bits, dtype=torch.bool)
        worst = {'styles|err/bound': 0.0, 's': 0.0, 'd': 0.0}
        for g, (off_, i_n, o_n, demod, two, aw, ab, pw, s_o, d_o) in enumerate(recs_in):
            keep[:n, off_:off_ + i_n] = False
            x = torch.cat([ws[:, g, :], w0], 1) if two else ws[:, g, :]
            got = buf[:n, off_:off_ + i_n].double()
            assert bool(torch.isfinite(got).all()) and bool((bits[:n, off_:off_ + i_n] != SENT_BITS).all()), f'group {g}: styles unwritten'
            # c: as dense_kernel, the lane walk over both sources: ceil(K1 / 64) + ceil(K2 / 64) + 8
            c = -(-k1 // 64) + (-(-k2 // 64) if two else 0) + 8
            ratio, _ = ref.linear_excess(got, ref.dense(x, aw, ab, 0.3, 1.5), x.double().abs() @ aw.double().abs().t() * 0.3, c,
                                         None if ab is None else (ab.double() * 1.5).abs() * ref.U32)
            worst['styles|err/bound'] = max(worst['styles|err/bound'], ratio)
            table = pw.wsq.cpu().double().reshape(i_n, pw.op) if demod else None
            rs, rd = ref.modconv_style_prep(got, table, o_n, demod, 1.0 if demod else 0.25)        # (from the styles the kernel read)
            worst['s'] = max(worst['s'], ref.row_rel_err(s_o.check(f's{g}'), rs)[0])
            if demod:
                worst['d'] = max(worst['d'], ref.row_rel_err(d_o.check(f'd{g}'), rd)[0])
        assert bool((bits[keep] == SENT_BITS).all()), 'dense_grouped wrote between or after the style rows'
        return [('styles|err/bound', worst['styles|err/bound'], 1.0), ('s', worst['s'], TOL_DENSE), ('d', worst['d'], TOL_DENSE)]
    return call, judge


# ------------------------------------------------------------------------------------------------
# the table: id -> (builder, expect, forbid)
# ------------------------------------------------------------------------------------------------
D4, D8, D16 = 'dense_kernel<4>', 'dense_kernel<8>', 'dense_kernel<16>'
NN, TN, NORM = 'matmul_nn_kernel', 'matmul_tn_kernel', 'normalize_2nd_moment_kernel'
DW, DWB = 'demod_weight_kernel', 'demod_weight_backward_kernel'
SF, SB1, SB2 = 'style_factors_kernel', 'style_factors_backward1_kernel', 'style_factors_backward2_kernel'
PREP, PREPG, DG = 'modconv_style_prep_kernel', 'modconv_style_prep_grouped_kernel', 'dense_grouped_kernel'


def C(builder, expect, forbid=()):
    return (builder, tuple(expect), tuple(forbid))


def SFK(nb, backward=True):
    """(expect, forbid) of a style-factors case served by the <nb> instantiations."""
    others = [m for m in (8, 16, 32) if m != nb]
    exp = [f'{SF}<{nb}>'] + ([f'{SB1}<{nb}>', SB2] if backward else [])
    return exp, [f'{SF}<{m}>' for m in others] + [f'{SB1}<{m}>' for m in others] + ([] if backward else [SB1, SB2])


CASES = {
    # ---- dense: <4> to N = 4, <8> to N = 8, <16> in slabs of 16 rows beyond (rows past the batch re-read the last row)
    'dense_n1_k1_o1': C(lambda: dense_case(1, 1, 1, bias=False), [D4], [D8, D16]),
    'dense_n4_k63_o3_act': C(lambda: dense_case(4, 63, 3, act=True), [D4], [D8, D16]),
    'dense_n4_k64_o5_bgain': C(lambda: dense_case(4, 64, 5, bgain=0.5), [D4], [D8, D16]),
    'dense_n5_k64_o4_bgain': C(lambda: dense_case(5, 64, 4, bgain=0.5), [D8], [D4, D16]),
    'dense_n8_k65_o5_act': C(lambda: dense_case(8, 65, 5, act=True, bgain=2.0), [D8], [D4, D16]),
    'dense_n8_k130_o1_nobias': C(lambda: dense_case(8, 130, 1, bias=False, gain=0.8), [D8], [D4, D16]),
    'dense_n9_k130_o5_nobias_ldy': C(lambda: dense_case(9, 130, 5, bias=False, pad_y=3), [D16], [D4, D8]),
    'dense_n16_k64_o3_act_ldy': C(lambda: dense_case(16, 64, 3, act=True, pad_y=1), [D16], [D4, D8]),
    'dense_n17_k63_o4_bgain': C(lambda: dense_case(17, 63, 4, bgain=0.5), [D16], [D4, D8]),
    'dense_n17_k1_o5_act_nobias': C(lambda: dense_case(17, 1, 5, bias=False, act=True), [D16], [D4, D8]),
    'dense_n33_k130_o5_act': C(lambda: dense_case(33, 130, 5, act=True), [D16], [D4, D8]),
    'dense_n33_k65_o1': C(lambda: dense_case(33, 65, 1), [D16], [D4, D8]),
    'dense_cabi_n5_k65_o3_ldx_ldy': C(lambda: dense_case(5, 65, 3, bgain=0.5, pad_x=3, pad_y=2), [D8], [D4, D16]),
    'dense_cabi_n17_k1_o1_ldx': C(lambda: dense_case(17, 1, 1, pad_x=4), [D16], [D4, D8]),
    'dense_cabi_n4_k130_o4_act_ldx': C(lambda: dense_case(4, 130, 4, act=True, pad_x=1), [D4], [D8, D16]),
    # ---- matmul_nn: 64 columns x 16 slices of M per block, 8 batch rows per pass
    'nn_1_1_1': C(lambda: matmul_nn_case(1, 1, 1), [NN], [TN]),
    'nn_3_5_7': C(lambda: matmul_nn_case(3, 5, 7), [NN], [TN]),
    'nn_8_16_64': C(lambda: matmul_nn_case(8, 16, 64), [NN], [TN]),
    'nn_9_15_65': C(lambda: matmul_nn_case(9, 15, 65), [NN], [TN]),
    'nn_17_40_130': C(lambda: matmul_nn_case(17, 40, 130), [NN], [TN]),
    'nn_8_1536_64': C(lambda: matmul_nn_case(8, 1536, 64), [NN], [TN]),
    'nn_cabi_9_17_65_lda_ldo': C(lambda: matmul_nn_case(9, 17, 65, pad_a=3, pad_o=5), [NN], [TN]),
    # ---- matmul_tn: a thread owns 4 rows x 1 column, 256 columns per block; colsum on and off
    'tn_1_1_1': C(lambda: matmul_tn_case(1, 1, 1, colsum=False), [TN], [NN]),
    'tn_1_1_1_colsum': C(lambda: matmul_tn_case(1, 1, 1), [TN], [NN]),
    'tn_3_5_7': C(lambda: matmul_tn_case(3, 5, 7, colsum=False), [TN], [NN]),
    'tn_3_5_7_colsum': C(lambda: matmul_tn_case(3, 5, 7), [TN], [NN]),
    'tn_8_4_256': C(lambda: matmul_tn_case(8, 4, 256, colsum=False), [TN], [NN]),
    'tn_8_4_256_colsum': C(lambda: matmul_tn_case(8, 4, 256), [TN], [NN]),
    'tn_9_6_257': C(lambda: matmul_tn_case(9, 6, 257, colsum=False), [TN], [NN]),
    'tn_9_6_257_colsum': C(lambda: matmul_tn_case(9, 6, 257), [TN], [NN]),
    'tn_33_7_300': C(lambda: matmul_tn_case(33, 7, 300, colsum=False), [TN], [NN]),
    'tn_33_7_300_colsum': C(lambda: matmul_tn_case(33, 7, 300), [TN], [NN]),
    'tn_cabi_9_6_257_lda_ldb': C(lambda: matmul_tn_case(9, 6, 257, pad_a=2, pad_b=3), [TN], [NN]),
    # ---- normalize_2nd_moment: one block of 256 threads per row
    'norm_n1_k1': C(lambda: normalize_case(1, 1), [NORM]),
    'norm_n5_k255_zero_row': C(lambda: normalize_case(5, 255, zero_row=3), [NORM]),
    'norm_n1_k256': C(lambda: normalize_case(1, 256), [NORM]),
    'norm_n5_k257_zero_row': C(lambda: normalize_case(5, 257, zero_row=0), [NORM]),
    'norm_n5_k1000': C(lambda: normalize_case(5, 1000), [NORM]),
    'norm_n5_k1_zero_row': C(lambda: normalize_case(5, 1, zero_row=4), [NORM]),
    # ---- demod_weight and its backward: one block per output channel
    'demod_1_1_1': C(lambda: demod_case(1, 1, 1, False), [DW, DWB]),
    'demod_1_1_1_prenorm_gwn_null': C(lambda: demod_case(1, 1, 1, True, 'gwsq'), [DW, DWB]),
    'demod_3_5_9_gwsq_null': C(lambda: demod_case(3, 5, 9, False, 'gwn'), [DW, DWB]),
    'demod_3_5_9_prenorm': C(lambda: demod_case(3, 5, 9, True), [DW, DWB]),
    'demod_2_300_9': C(lambda: demod_case(2, 300, 9, False), [DW, DWB]),
    'demod_2_300_9_prenorm_gwsq_null': C(lambda: demod_case(2, 300, 9, True, 'gwn'), [DW, DWB]),
    'demod_70_13_9_gwn_null': C(lambda: demod_case(70, 13, 9, False, 'gwsq'), [DW, DWB]),
    'demod_70_13_9_prenorm': C(lambda: demod_case(70, 13, 9, True), [DW, DWB]),
    'demod_4_64_1_prenorm_gwn_null': C(lambda: demod_case(4, 64, 1, True, 'gwsq'), [DW, DWB]),
    'demod_4_64_1': C(lambda: demod_case(4, 64, 1, False), [DW, DWB]),
    # ---- style factors and their backward: <8> to N = 8, <16> to 16, <32> to 32; the backward sums ceil(O / 64) slices, 8 unrolled
    'style_n1_i63_o1': C(lambda: style_case(1, 63, 1, False), *SFK(8)),
    'style_n8_i1_o7': C(lambda: style_case(8, 1, 7, False), *SFK(8)),
    'style_n8_i1_o8_prenorm': C(lambda: style_case(8, 1, 8, True), *SFK(8)),
    'style_n8_i64_o8_prenorm_gsn_null': C(lambda: style_case(8, 64, 8, True, 'gd'), *SFK(8)),
    'style_n8_i256_o513_gwsq_null': C(lambda: style_case(8, 256, 513, False, want_wsq=False), *SFK(8)),
    'style_n9_i65_o9_gd_null': C(lambda: style_case(9, 65, 9, False, 'gsn'), *SFK(16)),
    'style_n9_i64_o64_prenorm_gwsq_null': C(lambda: style_case(9, 64, 64, True, want_wsq=False), *SFK(16)),
    'style_n9_i64_d_null': C(lambda: style_case(9, 64, 5, False, fwd_d=False), *SFK(16, backward=False)),
    'style_n16_i256_o65_prenorm': C(lambda: style_case(16, 256, 65, True), *SFK(16)),
    'style_n16_i63_o512': C(lambda: style_case(16, 63, 512, False), *SFK(16)),
    'style_n17_i65_o513_prenorm': C(lambda: style_case(17, 65, 513, True), *SFK(32)),
    'style_n17_i64_o7_gd_null': C(lambda: style_case(17, 64, 7, False, 'gsn'), *SFK(32)),
    'style_n32_i63_o65_prenorm_gsn_null': C(lambda: style_case(32, 63, 65, True, 'gd'), *SFK(32)),
    'style_n32_i256_o577': C(lambda: style_case(32, 256, 577, False), *SFK(32)),
    'style_n32_i1_o9_prenorm_d_null': C(lambda: style_case(32, 1, 9, True, fwd_d=False), *SFK(32, backward=False)),
    # (the limits of the entry point: N * I = 8192 fills 64 KB of dynamic LDS in the forward and in the second backward kernel)
    'style_limit_n8_i1024_o9_prenorm': C(lambda: style_case(8, 1024, 9, True), *SFK(8)),
    'style_limit_n8_i1024_o9': C(lambda: style_case(8, 1024, 9, False), *SFK(8)),
    'style_limit_n32_i256_o9_prenorm': C(lambda: style_case(32, 256, 9, True), *SFK(32)),
    # (tied row maxima: rows 1..3 belong to waves 1..3 of the forward and to workgroups 1..3 of the second backward kernel)
    'style_ties_n8_i256_o9': C(lambda: style_case(8, 256, 9, True, ties=True), *SFK(8)),
    'style_ties_n17_i65_o9': C(lambda: style_case(17, 65, 9, True, ties=True), *SFK(32)),
    'style_ties_n9_i3_o65_gd_null': C(lambda: style_case(9, 3, 65, True, 'gsn', ties=True), *SFK(16)),
    # ---- _StyleFactorsFn end to end (the closed double backward runs dense / matmul_nn / matmul_tn at N = 2 * 17 and 2 * 32 rows)
    'stylefn_n17_i64_o513': C(lambda: style_fn_case(17, 64, 513, False), [f'{SF}<32>', f'{SB1}<32>', SB2, NN, TN, D16], [f'{SF}<16>', f'{SB1}<16>']),
    'stylefn_n17_i64_o513_half': C(lambda: style_fn_case(17, 64, 513, True), [f'{SF}<32>', f'{SB1}<32>', SB2, NN, TN, D16], [f'{SF}<16>', f'{SB1}<16>']),
    'stylefn_n32_i64_o513': C(lambda: style_fn_case(32, 64, 513, False), [f'{SF}<32>', f'{SB1}<32>', SB2, NN, TN, D16], [f'{SF}<16>', f'{SB1}<16>']),
    'stylefn_n32_i64_o513_half': C(lambda: style_fn_case(32, 64, 513, True), [f'{SF}<32>', f'{SB1}<32>', SB2, NN, TN, D16], [f'{SF}<16>', f'{SB1}<16>']),
    # ---- beyond the limit: the composed form
    'modulation_n33_composed': C(lambda: modulation_n33_case(False), [D16], [SF, SB1, SB2]),
    'modulation_n33_composed_half': C(lambda: modulation_n33_case(True), [D16], [SF, SB1, SB2]),
    # ---- modconv_style_prep: block (sample, 64 output channels), 4 slices of the I reduction
    'prep_i1_o1': C(lambda: style_prep_case(3, 1, 1), [PREP], [PREPG]),
    'prep_i255_o63': C(lambda: style_prep_case(3, 255, 63), [PREP], [PREPG]),
    'prep_i257_o64_ld': C(lambda: style_prep_case(2, 257, 64, pad=3), [PREP], [PREPG]),
    'prep_i1000_o65': C(lambda: style_prep_case(3, 1000, 65), [PREP], [PREPG]),
    'prep_i255_o130_pre_gain': C(lambda: style_prep_case(5, 255, 130, pre_gain=0.5), [PREP], [PREPG]),
    'prep_i257_nodemod_pre_gain_ld': C(lambda: style_prep_case(3, 257, 0, demod=False, pre_gain=0.25, pad=2), [PREP], [PREPG]),
    # ---- the grouped forms
    'grouped_n17_33_items': C(lambda: grouped_case(17), [DG, PREPG], [D16, PREP]),
    'grouped_n33_33_items': C(lambda: grouped_case(33), [DG, PREPG], [D16, PREP]),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_route(case):
    builder, expect, forbid = CASES[case]
    call, judge = builder()
    torch.cuda.synchronize()
    _, names = launched(call, expect=expect)
    kern = sorted({re.sub(r'^void |\(.*$', '', n) for n in names if 'kernel' in n})
    for p in expect:
        assert any_hit(p, names), f'{case}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not any_hit(p, names), f'{case}: {p} must not run; ran {kern}'
    recs = judge()
    print(f'ROUTE {case} kernels={[k for k in kern if any(any_hit(p, [k]) for p in ROUTE_KERNELS)]} '
          + ' '.join(f'{nm}={e:.2e}/{b:.0e}' for nm, e, b in recs))
    for nm, e, b in recs:
        assert e <= b, f'{case}: {nm}: {e:.3e} exceeds {b:.0e}'


@pytest.mark.parametrize('n,i', [(33, 8), (4, 1025), (9, 911)])
def test_shapes_beyond_the_limits_are_rejected_before_launch(n, i):
    """N > 32, I > 1024 and N * I > 8192: ``style_factors_supported`` says no, both C entry points return an error, nothing is launched."""
    kk, lib = _kk(), _lib()
    o = 5
    s, wsq = torch.ones(n, i, device=DEV), torch.ones(o, i, device=DEV)
    assert not kk.style_factors_supported(s, wsq)
    outs = [torch.full(sh, SENT, device=DEV) for sh in ((n, i), (n, o), (n + 1,), (n, i), (o, i), (n, i))]
    torch.cuda.synchronize()

    def call():
        with pytest.raises(lib.ShgError):
            kk.style_factors(s, wsq)
        with pytest.raises(lib.ShgError):
            cabi('shg_style_factors_f32', ptr(s), ptr(wsq), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), n, i, o, 1)
        if n > 32 or n * i > 8192:
            with pytest.raises(lib.ShgError):
                cabi('shg_style_factors_backward_f32', ptr(s), ptr(outs[1]), ptr(wsq), ptr(outs[2]), ptr(s), ptr(outs[1]), ptr(outs[3]), ptr(outs[4]),
                     ptr(outs[5]), n, i, o, 1)
    _, names = launched(call)
    assert not any('style_factors' in k for k in names), names
    for t in outs:
        assert bool((t.cpu().view(torch.int32) == SENT_BITS).all())


# Every __global__ of dense.hip with each instantiation its host code can pick (the 18 hipLaunchKernelGGL sites).
ROUTE_KERNELS = [
    D4, D8, D16, NORM, NN, TN, DW, DWB,
    f'{SF}<8>', f'{SF}<16>', f'{SF}<32>', f'{SB1}<8>', f'{SB1}<16>', f'{SB1}<32>', SB2,
    PREP, DG, PREPG,
]


def test_route_table_covers_every_kernel():
    """Every kernel / instantiation dense.hip can launch is the expected route of at least one case, and the list names every __global__ of
    the source (host-only: no launch)."""
    expected = {p.replace(' ', '') for _, (_, exp, _) in CASES.items() for p in exp}
    missing = [k for k in ROUTE_KERNELS if k.replace(' ', '') not in expected]
    assert not missing, f'kernels without a route case: {missing}'
    assert len(set(ROUTE_KERNELS)) == len(ROUTE_KERNELS)
    with open(os.path.join(ROOT, 'sh-gan_amd', 'csrc', 'dense.hip')) as fh:
        src = fh.read()
    kernels = set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', src))
    listed = {k.split('<')[0] for k in ROUTE_KERNELS}
    assert kernels == listed, (sorted(kernels - listed), sorted(listed - kernels))
    assert len(re.findall(r'hipLaunchKernelGGL\(', src)) == len(ROUTE_KERNELS)
    # an O > 512 case (the rolled tail of the second backward kernel) on every instantiation's side of the table
    assert any('_o513' in c or '_o577' in c for c in CASES)
