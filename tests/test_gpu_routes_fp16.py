"""Route table of the float16 entry points of shgan_amd.kernels_f16 (run with -m gpu on an MI355X).

The counterpart of tests/test_gpu_routes_fp32.py for the fp16 sources (csrc/conv_f16*.hip, conv_wgrad_f16.hip, upfirdn2d_f16.hip,
pointwise_f16.hip): each case names the kernel (or template instantiation) that must serve its input and the ones that must not, sits one step either side of a
dispatch predicate or a loop bound (grid caps with grid-stride loops, the slice loop of the weight gradient, the trips of the tail's
backward), and compares the result with a float64 evaluation of the same operation on the same half-rounded operands.  The last two tests
are host-only: the table covers every launch site of those sources.

Bars (from the arithmetic, not from the code under test):
  * outputs rounded to half once from an fp32 accumulation (conv2d, conv_transpose2d, conv2d_wgrad, upfirdn2d):
    max|got - ref| / max|ref| < 6e-4 (2^-11 = 4.9e-4 + fp32 slack);
  * elementwise half outputs of the tails (gt, dx, y): every element |got - ref| <= 2^-10 |ref| + 2^-24 (one half rounding of an fp32
    value that carries fp32 rounding, + the smallest half denormal).  That holds for an fp32 value whose own error is relative to the
    VALUE; where a tail adds terms of both signs (t * d + noise + bias) the operands are therefore drawn from dyadic grids (t, noise,
    bias multiples of 1/64, d of 1/16), so that the fp32 sum is exact and only the activation's two multiplies and the half rounding remain;
    the second product of the double backward (gy * d + u * e) is drawn with u of the sign of gy and d, e > 0 for the same reason;
  * fp32 sums s1, s0, gnoise: |got - ref| <= 4e-5 * sum|terms| per output (at most 2 + 256 + 256 sequential fp32 adds: 514 * 2^-24 = 3.1e-5);
  * fused-tail convolution outputs: the reference of the f16 family of tests/fuzz_cases.py (intermediate rounded to half), 3e-3;
  * pure casts (relayout): bit-equal to torch's cast."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
SQRT2 = 2 ** 0.5
TOL_ACC = 6e-4           # one half rounding of an fp32-accumulated sum, relative to the largest output
TOL_FUSED = 3e-3         # fused-tail convolutions (tests/fuzz_cases.py _case_f16)
TOL_SUM = 4e-5           # fp32 sums, relative to the sum of absolute addends


def _kf():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels_f16
    return kernels_f16


def _lib():
    return _kf()._lib.get_lib()


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def hn(g, *shape, scale=1.0):
    """Normal halves [N,C,H,W] in channels_last memory."""
    t = (torch.randn(shape, generator=g, device=DEV) * scale).half()
    return t.contiguous(memory_format=CL) if t.ndim == 4 else t


def grid(g, lo, hi, step, *shape):
    """float32 multiples of 1/step in [lo, hi] (exact in half for the ranges used here)."""
    return torch.randint(int(lo * step), int(hi * step) + 1, shape, generator=g, device=DEV).float() / step


# ------------------------------------------------------------------------------------------------
# judges: got -> [(label, measured, bar, strict)]; ``strict``: measured < bar, otherwise measured <= bar
# ------------------------------------------------------------------------------------------------

def j_max(label, got, ref, bar):
    assert tuple(got.shape) == tuple(ref.shape), (label, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), label
    return (label, float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), bar, True)


def j_elem(label, got, ref):
    """Largest |got - ref| / (2^-10 |ref| + 2^-24) over the elements: at most 1."""
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float16, (label, tuple(got.shape), got.dtype)
    assert torch.isfinite(got).all(), label
    return (label, float(((got.double() - ref).abs() / (ref.abs() * 2.0 ** -10 + 2.0 ** -24)).max()), 1.0, False)


def j_sum(label, got, ref, absum):
    """Largest |got - ref| / (4e-5 sum|terms|); an output without addends must be exactly zero."""
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (label, tuple(got.shape), got.dtype)
    err = (got.double() - ref).abs()
    assert bool((err[absum == 0] == 0).all()), label
    return (label, float((err / (TOL_SUM * absum).clamp_min(1e-300)).max()), 1.0, False)


def j_equal(label, got, ref):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (label, got.dtype, tuple(got.shape))
    return (label, 0.0 if torch.equal(got, ref) else 1.0, 0.0, False)


# ------------------------------------------------------------------------------------------------
# case builders: each returns (call, judge); the inputs are built before the probe, so only the entry point's own launches are traced
# ------------------------------------------------------------------------------------------------

def wgrad(n, i, o, h, w, k=3, stride=1, pad=1, capped=False):
    """conv2d_wgrad against k*k float64 contractions over the shifted / strided windows of the zero-padded input.  ``capped``: the slice
    count is the workgroup-target cap, with several blocks per slice and a ragged count (asserted from the arithmetic of the case)."""
    kf = _kf()
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    g_ = gen(101 + n + i + o)
    x, gy = hn(g_, n, i, h, w), hn(g_, n, o, oh, ow)
    ip, op = cdiv(i, 8) * 8, cdiv(o, 8) * 8                       # the wrapper's channel pad
    IP, OP = cdiv(ip, 64) * 64, cdiv(op, 64) * 64
    tiles = (OP // 64) * (IP // 64)
    cap = cdiv(1024 if k == 1 else 512, tiles)
    wr = 8 if (k == 3 and stride == 1) else 4
    nblocks = n * cdiv(oh, wr) * cdiv(ow, 16)
    if capped:
        slices = _lib().shg_conv2d_wgrad_f16_workspace_bytes(n, ip, op, oh, ow, k) // (k * k * OP * IP * 4)
        assert slices == cap and nblocks > slices and nblocks % slices != 0, (slices, cap, nblocks)
    xd, gd = F.pad(x.double(), [pad] * 4), gy.double()
    ref = torch.stack([torch.einsum('noyx,niyx->oi', gd, xd[:, :, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride])
                       for ky in range(k) for kx in range(k)], dim=-1).reshape(o, i, k, k)
    return (lambda: kf.conv2d_wgrad(x, gy, k, stride, pad)), (lambda got: [j_max('dw', got, ref, TOL_ACC)])


def _slope64(y, act, gain, alpha, act_gain, clamp):
    """A'(y) read from the saved half output: 0 where |y| >= clamp, gain * act_gain where y > 0, times alpha otherwise (no activation: gain)."""
    yd = y.double()
    if not act:
        return torch.full_like(yd, gain)
    tot = act_gain * gain
    s = torch.where(yd > 0, torch.full_like(yd, tot), torch.full_like(yd, alpha * tot))
    return torch.where(yd.abs() >= clamp * gain, torch.zeros_like(yd), s)


def mtb(c, h, w, trips, ue=False, act=True, gain=1.0, clamp=256.0, yscale=100.0, td=True):
    """modtail_backward, N = 2, all four results.  ``trips``: iterations of the kernel's uniform loop (256 workgroups per sample at most)."""
    kf = _kf()
    n, alpha = 2, 0.2
    total = h * w * (c // 8)
    nblk = _lib().shg_modtail_backward_f16_blocks(h * w, c)
    assert nblk == min(256, cdiv(total, 256)) and cdiv(total, nblk * 256) == trips, (nblk, total)
    g_ = gen(211 + c + h)
    gy = hn(g_, n, c, h, w)
    y = (torch.randn(n, c, h, w, generator=g_, device=DEV) * yscale)
    y = (y.clamp(-clamp * gain, clamp * gain) if act else y).half().contiguous(memory_format=CL)
    t = hn(g_, n, c, h, w, scale=2.0) if td else None
    d = (torch.rand(n, c, generator=g_, device=DEV) + 0.5) if td else None
    u = e = None
    if ue:                                                    # sign(u) = sign(gy), e > 0: the two products never cancel (module docstring)
        u = (hn(g_, n, c, h, w).abs() * torch.where(gy < 0, -1.0, 1.0)).half().contiguous(memory_format=CL)
        e = torch.rand(n, c, generator=g_, device=DEV) + 0.5
    slope = _slope64(y, act, gain, alpha, SQRT2, clamp)
    if act:
        assert 0.002 < float((slope == 0).double().mean()) < 0.6              # a visible share of y sits on the clamp
    gz = gy.double() * slope
    d64 = d.double().view(n, c, 1, 1) if td else 1.0
    gt = gz * d64
    if ue:
        gt = gt + u.double() * slope * e.double().view(n, c, 1, 1)
    t64 = t.double() if td else torch.zeros_like(gz)
    s1, a1 = (gz * t64).sum((2, 3)), (gz * t64).abs().sum((2, 3))
    s0, a0 = gz.sum((2, 3)), gz.abs().sum((2, 3))
    gn, an = gz.sum(1, keepdim=True), gz.abs().sum(1, keepdim=True)

    def judge(got):
        ggt, gs1, gs0, ggn = got
        return [j_elem('gt', ggt, gt), j_sum('s1', gs1, s1, a1), j_sum('s0', gs0, s0, a0), j_sum('gnoise', ggn, gn, an)]
    return (lambda: kf.modtail_backward(gy, y, t, d, want_sums=True, want_noise=True, act=act, gain=gain, alpha=alpha, clamp=clamp, u=u, e=e)), judge


def _act64(z, act, gain, alpha, clamp):
    if not act:
        return z * gain
    z = torch.where(z < 0, z * alpha, z) * (SQRT2 * gain)
    return z.clamp(-clamp * gain, clamp * gain)


def modtail(c, h, w, noise='shared', n=2, clamp=4.0):
    """y = A(t * d + noise + bias) with every operand on a dyadic grid (module docstring): the fp32 sum is exact."""
    kf = _kf()
    g_ = gen(307 + c + h)
    t = grid(g_, -8, 8, 64, n, c, h, w).half().contiguous(memory_format=CL)
    d, b = grid(g_, 0.5, 1.5, 16, n, c), grid(g_, -1, 1, 64, c)
    nz = grid(g_, -2, 2, 64, *((h, w) if noise == 'shared' else (n, 1, h, w)))
    z = t.double() * d.double().view(n, c, 1, 1) + nz.double() + b.double().view(1, c, 1, 1)
    ref = _act64(z, True, 1.0, 0.2, clamp)
    assert 0.002 < float((ref.abs() == clamp).double().mean()) < 0.6
    return (lambda: kf.modtail(t, d, nz, b, act=True, clamp=clamp)), (lambda got: [j_elem('y', got, ref)])


def bias_act(c, h, w, n=2, clamp=4.0):
    kf = _kf()
    g_ = gen(401 + c + h)
    x = grid(g_, -8, 8, 64, n, c, h, w).half().contiguous(memory_format=CL)
    b = grid(g_, -1, 1, 64, c)
    ref = _act64(x.double() + b.double().view(1, c, 1, 1), True, 1.0, 0.2, clamp)
    assert 0.002 < float((ref.abs() == clamp).double().mean()) < 0.6
    return (lambda: kf.bias_act(x, b, act=True, clamp=clamp)), (lambda got: [j_elem('y', got, ref)])


def bias_act_bwd(n, c, h, w, clamp=4.0):
    kf = _kf()
    g_ = gen(503 + c + h)
    gy = hn(g_, n, c, h, w)
    y = (torch.randn(n, c, h, w, generator=g_, device=DEV) * 2.5).clamp(-clamp, clamp).half().contiguous(memory_format=CL)
    ref = gy.double() * _slope64(y, True, 1.0, 0.2, SQRT2, clamp)
    assert 0.002 < float((ref == 0).double().mean()) < 0.6
    return (lambda: kf.bias_act_backward(gy, y, act=True, clamp=clamp)), (lambda got: [j_elem('dx', got, ref)])


def relayout(n, c, h, w, to_half):
    """The block-boundary cast in either direction: bit-equal to torch's cast (values beyond the half range included)."""
    kf = _kf()
    x = torch.randn(n, c, h, w, generator=gen(601 + c + h), device=DEV) * 300
    x.view(-1)[::7] *= 1e3
    xh = x.to(dtype=torch.float16, memory_format=CL)
    if to_half:
        return (lambda: kf.relayout(x)), (lambda got: [j_equal('cast', got, xh)] if got.is_contiguous(memory_format=CL) else [('layout', 1.0, 0.0, False)])
    back = xh.to(torch.float32).contiguous()
    del x
    return (lambda: kf.relayout(xh)), (lambda got: [j_equal('cast', got, back)] if got.is_contiguous() else [('layout', 1.0, 0.0, False)])


F1331 = torch.tensor([1., 3., 3., 1.])
F_SEP = torch.outer(F1331, F1331) / 64
F_ASYM = torch.outer(torch.tensor([1., 2., -1., 0.5]), torch.tensor([0.25, 1., 3., -2.]))


def _frand(fh, fw):
    return torch.rand(fh, fw, generator=torch.Generator().manual_seed(fh * 10 + fw)) + 0.1


def fir(n, c, h, w, f, up=1, down=1, pad=(2, 1, 2, 1), flip=False, gain=1.0, rows=None, chunk=128):
    """upfirdn2d against a float64 sum of fh * fw shifted multiply-adds, in channel chunks.  ``rows``: the marching strip the documented rule
    (the longest of 32 / 16 / 8 / 4 rows with N ceil(OH / rows) ceil(OW / 2) C / 8 >= 524 288 lanes) gives this shape -- a runtime argument
    of the launch, asserted here from the rule alone."""
    kf = _kf()
    px0, px1, py0, py1 = pad
    fh, fw = f.shape
    oh, ow = (h * up + py0 + py1 - fh + down) // down, (w * up + px0 + px1 - fw + down) // down
    if rows is not None:
        r = 32
        while r > 4 and n * cdiv(oh, r) * cdiv(ow, 2) * (c // 8) < 524288:
            r //= 2
        assert r == rows and oh % rows != 0, (r, oh)
    x = hn(gen(701 + c + h), n, c, h, w)
    fd = f.to(DEV)
    fk = (fd if flip else fd.flip([0, 1])).double() * gain        # tap (ky, kx) of the gather form

    def judge(got):
        assert tuple(got.shape) == (n, c, oh, ow) and got.dtype == torch.float16 and torch.isfinite(got).all()
        dmax = rmax = 0.0
        for c0 in range(0, c, chunk):
            xc = x[:, c0:c0 + chunk].double()
            if up > 1:
                z = xc.new_zeros(n, xc.shape[1], h * up, w * up)
                z[:, :, ::up, ::up] = xc
                xc = z
            xc = F.pad(xc, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
            xc = xc[:, :, max(-py0, 0): xc.shape[2] - max(-py1, 0), max(-px0, 0): xc.shape[3] - max(-px1, 0)]
            ref = xc.new_zeros(n, xc.shape[1], oh, ow)
            for ky in range(fh):
                for kx in range(fw):
                    ref += fk[ky, kx] * xc[:, :, ky:ky + (oh - 1) * down + 1:down, kx:kx + (ow - 1) * down + 1:down]
            dmax = max(dmax, float((got[:, c0:c0 + chunk].double() - ref).abs().max()))
            rmax = max(rmax, float(ref.abs().max()))
            del xc, ref
        return [('y', dmax / rmax, TOL_ACC, True)]
    return (lambda: kf.upfirdn2d(x, fd, up, up, down, down, px0, px1, py0, py1, flip, gain)), judge


def conv(n, i, o, h, w, k=3, stride=1, pad=1, bias=False, in_scale=False, out_scale=False, noise=None, act=None, residual=False):
    """conv2d and its fused inference tail.  Plain (+ bias, + in_scale): one rounding of the fp32 sum, 6e-4; with a tail the reference of the
    f16 fuzz family (the convolution result rounded to half, the tail in float64, rounded, + residual), 3e-3."""
    kf = _kf()
    g_ = gen(809 + i + o + h + w)
    x = hn(g_, n, i, h, w)
    wt = (torch.randn(o, i, k, k, generator=g_, device=DEV) / math.sqrt(i * k * k)).half()
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    b = torch.randn(o, generator=g_, device=DEV) if bias else None
    si = (torch.rand(n, i, generator=g_, device=DEV) + 0.5) if in_scale else None
    so = (torch.rand(n, o, generator=g_, device=DEV) + 0.5) if out_scale else None
    nz = None if noise is None else torch.randn(*((oh, ow) if noise == 'shared' else (n, 1, oh, ow)), generator=g_, device=DEV)
    res = hn(g_, n, o, oh, ow) if residual else None
    xs = x if si is None else (x.float() * si.half().float().view(n, i, 1, 1)).half()          # half x half, rounded once
    ref = F.conv2d(xs.double(), wt.double(), None, stride=stride, padding=pad)
    tail = so is not None or nz is not None or act is not None or res is not None
    if not tail:
        if b is not None:
            ref = ref + b.double().view(1, -1, 1, 1)
        tol = TOL_ACC
    else:
        z = ref.half().double()
        if so is not None:
            z = z * so.double().view(n, o, 1, 1)
        if nz is not None:
            z = z + nz.double() * 0.5
        if b is not None:
            z = z + b.double().view(1, -1, 1, 1)
        if act:
            z = (F.leaky_relu(z, 0.2) * SQRT2).clamp(-256, 256)
        ref = z.half().double()
        if res is not None:
            ref = ref + res.double()
        tol = TOL_FUSED
    kw = {}
    if tail or si is not None:
        kw = dict(in_scale=si, out_scale=so, noise=nz, noise_strength=0.5, act=act, residual=res)
    return (lambda: kf.conv2d(x, wt, b, stride, pad, **kw)), (lambda got: [j_max('y', got, ref, tol)])


def convT(n, i, o, h, w, pad=0, bias=False):
    """conv_transpose2d (3x3, stride 2), the whole (2H+1-2 pad) x (2W+1-2 pad) result."""
    kf = _kf()
    g_ = gen(907 + i + o + h + w)
    x = hn(g_, n, i, h, w)
    wt = (torch.randn(i, o, 3, 3, generator=g_, device=DEV) / math.sqrt(i * 9 / 4)).half()
    b = torch.randn(o, generator=g_, device=DEV) if bias else None
    ref = F.conv_transpose2d(x.double(), wt.double(), None if b is None else b.double(), stride=2, padding=pad)
    return (lambda: kf.conv_transpose2d(x, wt, b, pad)), (lambda got: [j_max('y', got, ref, TOL_ACC)])


# ------------------------------------------------------------------------------------------------
# the table: id -> (builder, expect, forbid, switches); switches: routes = mask of shg_conv2d_f16_set_routes for the case, twice = run
# again and compare the bits
# ------------------------------------------------------------------------------------------------
GATHER, RING, UPRING, DOWN = 'conv_f16_kernel', 'conv_f16_ring_kernel', 'conv_f16_upring_kernel', 'conv_f16_down_kernel'
WG31, WG32, WG11 = 'conv_wgrad_f16_kernel<3, 1>', 'conv_wgrad_f16_kernel<3, 2>', 'conv_wgrad_f16_kernel<1, 1>'
RED = 'f16::wgrad_reduce_kernel'
MT, MTB, BA, BAB = 'modtail_f16_kernel', 'modtail_backward_f16_kernel', 'bias_act_f16_kernel', 'bias_act_backward_f16_kernel'
THIN, TO_H, TO_F = 'relayout_thin_kernel', 'relayout_to_half_kernel', 'relayout_to_float_kernel'
MARCH, SAME, UPDN, GENERIC = 'fir4_march_f16_kernel', 'fir_same_f16_kernel', 'updn4_f16_kernel', 'upfirdn2d_f16_kernel'


def K(mb, nt, nb, wl=False):
    return f'{GATHER}<{mb}, {nt}, {nb}, {"true" if wl else "false"}>'


# launch_conv<MB, NB> exists for (1,1) (2,1) (4,1) (1,2) (2,2), each with 1, 2, 4 or 9 taps, and with the LDS weight slab for 9 taps and MB <= 2
ALL_GATHER = ([K(mb, nt, nb) for mb, nb in ((1, 1), (2, 1), (4, 1), (1, 2), (2, 2)) for nt in (1, 2, 4, 9)]
              + [K(mb, 9, nb, True) for mb, nb in ((1, 1), (2, 1), (1, 2), (2, 2))])


def others(*kerns):
    return [k for k in ALL_GATHER if k not in kerns]


def C(builder, expect, forbid=(), **switches):
    return (builder, tuple(expect), tuple(forbid), dict(switches))


def W(builder, kern, g):
    """A weight-gradient case: its kernel instantiation and reduction, none of the others, bit-identical when run again."""
    return C(builder, [kern, f'{RED}<{g}>'], [k for k in (WG31, WG32, WG11) if k != kern] + [f'{RED}<{q}>' for q in (1, 2, 4, 8, 16) if q != g],
             twice=True)


def G9(builder, kern):
    """A 3x3 (or 1x1) gather case with every persistent route switched off: this instantiation and no other kernel of the family."""
    return C(builder, [kern], others(kern) + [RING, DOWN, UPRING], routes=0)


def T4(i, o, h, w, mb, nb):
    """The transposed form without the merged-phase kernel (bit 2 of the route mask off): four launches with 4, 2, 2 and 1 taps."""
    phases = [K(mb, 4, nb), K(mb, 2, nb), K(mb, 1, nb)]
    return C(lambda: convT(1, i, o, h, w), phases, others(*phases) + [UPRING], routes=5)


CASES = {
    # ---- conv2d_wgrad.  Channels after the wrapper's pad to 8; tiles = ceil(O/64) ceil(I/64); cap = ceil(512 / tiles) (1x1: 1024);
    # nblocks = N ceil(OH / wr) ceil(OW / 16), wr = 8 for 3x3 stride 1, else 4; slices = min(cap, nblocks).  The reduction takes the largest
    # G <= 16 with slices >= 8 (G / 2) at every doubling and ceil(total / (256 / (G / 2))) < 2048, total = k k O I.
    # 32 -> 32 at 8 x 16: one tile, one block per sample, slices = N, total = 9216 (36 workgroups at G = 1): G by slices >= 8 G alone
    'wgrad_reduce_n7_g1': W(lambda: wgrad(7, 32, 32, 8, 16), WG31, 1),
    'wgrad_reduce_n8_g2': W(lambda: wgrad(8, 32, 32, 8, 16), WG31, 2),
    'wgrad_reduce_n15_g2': W(lambda: wgrad(15, 32, 32, 8, 16), WG31, 2),
    'wgrad_reduce_n16_g4': W(lambda: wgrad(16, 32, 32, 8, 16), WG31, 4),
    'wgrad_reduce_n31_g4': W(lambda: wgrad(31, 32, 32, 8, 16), WG31, 4),
    'wgrad_reduce_n32_g8': W(lambda: wgrad(32, 32, 32, 8, 16), WG31, 8),
    'wgrad_reduce_n63_g8': W(lambda: wgrad(63, 32, 32, 8, 16), WG31, 8),
    'wgrad_reduce_n64_g16': W(lambda: wgrad(64, 32, 32, 8, 16), WG31, 16),
    # N = 2 at 32 x 32: 2 * 4 * 2 = 16 blocks, 16 tiles -> cap 32, slices 16.  256 -> 256: 9 * 256 * 256 / 256 = 2304 >= 2048 -> G = 1;
    # 224 -> 256: 9 * 256 * 224 / 256 = 2016 < 2048 and 16 >= 8 -> G = 2 (then 4032 >= 2048 stops it)
    'wgrad_reduce_2304_groups_g1': W(lambda: wgrad(2, 256, 256, 32, 32), WG31, 1),
    'wgrad_reduce_2016_groups_g2': W(lambda: wgrad(2, 224, 256, 32, 32), WG31, 2),
    # the same bound one channel step either side: 280 -> 208 (20 tiles, cap 26, slices 16): 9 * 208 * 280 = 524 160 -> ceil(/ 256) = 2048 -> G = 1;
    # 808 -> 72 (26 tiles, cap 20, slices 16): 9 * 72 * 808 = 523 584 -> 2046 < 2048 -> G = 2
    'wgrad_reduce_2048_groups_g1': W(lambda: wgrad(2, 280, 208, 32, 32), WG31, 1),
    'wgrad_reduce_2046_groups_g2': W(lambda: wgrad(2, 808, 72, 32, 32), WG31, 2),
    # 512 -> 512 at 20 x 40, N = 3: 64 tiles -> cap 8; 3 * ceil(20/8) * ceil(40/16) = 27 blocks on 8 slices: slices 0-2 run 4 blocks, 3-7 run 3;
    # the last row block has 4 of 8 rows, the last column block 8 of 16 columns; total / 256 = 9216 -> G = 1
    'wgrad_s1_27_blocks_on_8_slices': W(lambda: wgrad(3, 512, 512, 20, 40, capped=True), WG31, 1),
    # 136 -> 72 (192 x 128 padded: 6 tiles, ragged both ways) -> cap 86; 65 x 71 -> 32 x 35: 4 * 8 * 3 = 96 blocks on 86 slices (10 run two);
    # pad 1: 33 x 36 -> 4 * 9 * 3 = 108 blocks (22 run two).  total = 88128: 345 / 689 / 1377 groups < 2048, 86 >= 8, 16, 32 -> G = 8 (2754 stops)
    'wgrad_s2_96_blocks_on_86_slices': W(lambda: wgrad(4, 136, 72, 65, 71, stride=2, pad=0, capped=True), WG32, 8),
    'wgrad_s2_pad1_108_blocks_on_86_slices': W(lambda: wgrad(4, 136, 72, 65, 71, stride=2, pad=1, capped=True), WG32, 8),
    # 1x1 512 -> 512 at 12 x 40, N = 2: cap 1024 / 64 = 16; 2 * 3 * 3 = 18 blocks (2 slices run two); total / 256 = 1024 < 2048, 16 >= 8 -> G = 2
    'wgrad_1x1_18_blocks_on_16_slices': W(lambda: wgrad(2, 512, 512, 12, 40, k=1, pad=0, capped=True), WG11, 2),
    'wgrad_s1_one_block': W(lambda: wgrad(1, 8, 8, 4, 5), WG31, 1),
    'wgrad_1x1_one_block': W(lambda: wgrad(1, 8, 8, 1, 1, k=1, pad=0), WG11, 1),
    # ---- modtail_backward: 256 workgroups per sample at most, uniform trip count = ceil(HW C / 8 / 65536), masked lanes stay in the shuffle
    'mtb_c64_12x20_one_trip': C(lambda: mtb(64, 12, 20, 1), [MTB], [MT, BAB]),
    'mtb_c64_12x20_one_trip_ue': C(lambda: mtb(64, 12, 20, 1, ue=True), [MTB], [MT, BAB]),
    'mtb_c512_32x32_at_cap': C(lambda: mtb(512, 32, 32, 1), [MTB], [MT, BAB]),                   # 65 536 lanes: 256 full workgroups, one trip
    'mtb_c512_32x32_at_cap_ue': C(lambda: mtb(512, 32, 32, 1, ue=True), [MTB], [MT, BAB]),
    'mtb_c512_33x33_two_trips': C(lambda: mtb(512, 33, 33, 2), [MTB], [MT, BAB]),                # 69 696 lanes: workgroups 17-255 idle in trip 2
    'mtb_c512_33x33_two_trips_ue': C(lambda: mtb(512, 33, 33, 2, ue=True), [MTB], [MT, BAB]),
    'mtb_c64_91x91_two_trips': C(lambda: mtb(64, 91, 91, 2), [MTB], [MT, BAB]),                  # 66 248 lanes
    'mtb_c64_91x91_two_trips_ue': C(lambda: mtb(64, 91, 91, 2, ue=True), [MTB], [MT, BAB]),
    'mtb_c8_257x257_two_trips': C(lambda: mtb(8, 257, 257, 2), [MTB], [MT, BAB]),                # 66 049 lanes, one lane per pixel
    'mtb_c8_257x257_two_trips_ue': C(lambda: mtb(8, 257, 257, 2, ue=True), [MTB], [MT, BAB]),
    'mtb_c64_91x91_linear_gain': C(lambda: mtb(64, 91, 91, 2, act=False, gain=0.6), [MTB], [MT, BAB]),
    'mtb_c64_91x91_small_clamp': C(lambda: mtb(64, 91, 91, 2, clamp=1.0, yscale=1.0), [MTB], [MT, BAB]),
    'mtb_c64_91x91_no_t_no_d': C(lambda: mtb(64, 91, 91, 2, td=False), [MTB], [MT, BAB]),
    # ---- modtail / bias_act forward: <true> keeps the per-channel operands in registers when 256 % (C / 8) == 0, <false> reloads them
    **{f'modtail_c{c}_{nz}_noise': C(lambda c=c, nz=nz: modtail(c, 9, 7, noise=nz), [f'{MT}<{"true" if 256 % (c // 8) == 0 else "false"}>'],
                                     [f'{MT}<{"false" if 256 % (c // 8) == 0 else "true"}>', BA])
       for c in (16, 24, 40, 64, 72) for nz in ('shared', 'per')},
    **{f'bias_act_c{c}': C(lambda c=c: bias_act(c, 9, 7), [f'{BA}<{"true" if 256 % (c // 8) == 0 else "false"}>'],
                           [f'{BA}<{"false" if 256 % (c // 8) == 0 else "true"}>', MT])
       for c in (16, 24, 40, 64, 72)},
    # past the grid caps, the last trip not full: modtail 2048 workgroups = 524 288 lanes (725^2 = 525 625; 419^2 * 3 = 526 683), bias_act
    # 4096 = 1 048 576 (1025^2 = 1 050 625), bias_act_backward 8192 = 2 097 152 (2 097 229 eight-element groups)
    'modtail_c8_725x725_past_cap': C(lambda: modtail(8, 725, 725, noise='per', n=1), [f'{MT}<true>'], [f'{MT}<false>']),
    'modtail_c24_419x419_past_cap': C(lambda: modtail(24, 419, 419, noise='shared', n=1), [f'{MT}<false>'], [f'{MT}<true>']),
    'bias_act_c8_1025x1025_past_cap': C(lambda: bias_act(8, 1025, 1025, n=1), [f'{BA}<true>'], [f'{BA}<false>']),
    'bias_act_bwd_c8_2097229_past_cap': C(lambda: bias_act_bwd(1, 8, 1, 2097229), [BAB], [BA, MTB]),
    'bias_act_bwd_c24_9x7': C(lambda: bias_act_bwd(2, 24, 9, 7), [BAB], [BA, MTB]),
    # ---- relayout: C % 8 != 0 takes the thin kernels (a lane per pixel), C % 8 == 0 the 64 x 64 LDS tiles; H W = 65: two pixel tiles, the
    # second with one pixel; 4100^2 = 16 810 000 pixels > 65 536 * 256 = 16 777 216: a second, ragged trip
    'relayout_thin_c3_to_half': C(lambda: relayout(2, 3, 5, 13, True), [f'{THIN}<true>'], [f'{THIN}<false>', TO_H, TO_F]),
    'relayout_thin_c3_to_float': C(lambda: relayout(2, 3, 5, 13, False), [f'{THIN}<false>'], [f'{THIN}<true>', TO_H, TO_F]),
    'relayout_thin_c12_to_half': C(lambda: relayout(2, 12, 5, 13, True), [f'{THIN}<true>'], [f'{THIN}<false>', TO_H, TO_F]),
    'relayout_thin_c12_to_float': C(lambda: relayout(2, 12, 5, 13, False), [f'{THIN}<false>'], [f'{THIN}<true>', TO_H, TO_F]),
    'relayout_thin_c3_4100x4100_past_cap': C(lambda: relayout(1, 3, 4100, 4100, True), [f'{THIN}<true>'], [f'{THIN}<false>', TO_H, TO_F]),
    **{f'relayout_tiled_c{c}_to_half': C(lambda c=c: relayout(2, c, 5, 13, True), [TO_H], [THIN, TO_F]) for c in (8, 16, 72, 128)},
    **{f'relayout_tiled_c{c}_to_float': C(lambda c=c: relayout(2, c, 5, 13, False), [TO_F], [THIN, TO_H]) for c in (8, 16, 72, 128)},
    # ---- upfirdn2d: 4x4 same-size -> marching; any other same-size filter -> fir_same; 4x4 with ONE factor of two -> updn4; else generic
    'fir_4x4_same_march': C(lambda: fir(2, 16, 9, 11, F_SEP), [MARCH], [SAME, UPDN, GENERIC]),
    'fir_3x4_same': C(lambda: fir(2, 16, 9, 11, _frand(3, 4), pad=(2, 1, 1, 1)), [SAME], [MARCH, UPDN, GENERIC]),
    'fir_4x4_down2': C(lambda: fir(2, 16, 10, 12, F_ASYM, down=2, pad=(1, 1, 1, 1), flip=True), [f'{UPDN}<1, 2>'], [f'{UPDN}<2, 1>', MARCH, SAME, GENERIC]),
    'fir_4x4_up2': C(lambda: fir(2, 16, 5, 7, F_ASYM, up=2, pad=(2, 1, 2, 1), gain=4.0), [f'{UPDN}<2, 1>'], [f'{UPDN}<1, 2>', MARCH, SAME, GENERIC]),
    'fir_4x4_up2_down2_generic': C(lambda: fir(2, 16, 9, 11, F_ASYM, up=2, down=2, pad=(2, 1, 2, 1)), [GENERIC], [UPDN, MARCH, SAME]),
    'fir_3x3_down2_generic': C(lambda: fir(2, 16, 9, 11, _frand(3, 3), down=2, pad=(1, 1, 1, 1)), [GENERIC], [UPDN, MARCH, SAME]),
    # marching strips at C = 512, OH = 250, OW = 512 (256 column pairs, 64 channel groups): lanes(r) = N * ceil(250 / r) * 16 384:
    #   N = 4: lanes(32) = 4 * 8 * 16 384 = 524 288 -> 32 rows;   N = 2: lanes(32) = 262 144, lanes(16) = 2 * 16 * 16 384 = 524 288 -> 16;
    #   N = 1: lanes(16) = 262 144, lanes(8) = 32 * 16 384 = 524 288 -> 8;   N = 1, OW = 510: lanes(8) = 32 * 255 * 64 = 522 240 -> 4
    'fir_march_32_row_strips': C(lambda: fir(4, 512, 250, 512, F_SEP, rows=32), [MARCH], [SAME]),
    'fir_march_16_row_strips': C(lambda: fir(2, 512, 250, 512, F_SEP, rows=16, flip=True, gain=4.0), [MARCH], [SAME]),
    'fir_march_8_row_strips': C(lambda: fir(1, 512, 250, 512, F_ASYM, rows=8), [MARCH], [SAME]),
    'fir_march_4_row_strips_below_threshold': C(lambda: fir(1, 512, 250, 510, _frand(4, 4), rows=4), [MARCH], [SAME]),
    # past the 8192-workgroup cap (2 097 152 lanes): down 2 at 64 ch, 513^2 outputs * 8 = 2 105 352 lanes; 3x4 same-size at 32 ch, a lane
    # = 2 rows x 4 columns x 8 channels: ceil(1025 / 2) * ceil(4093 / 4) * 4 = 513 * 1024 * 4 = 2 101 248 lanes
    'fir_down2_past_cap': C(lambda: fir(1, 64, 1026, 1026, F_SEP, down=2, pad=(1, 1, 1, 1)), [f'{UPDN}<1, 2>'], [GENERIC]),
    'fir_3x4_same_past_cap': C(lambda: fir(1, 32, 1025, 4093, _frand(3, 4), pad=(2, 1, 1, 1)), [SAME], [MARCH]),
    # ---- the gather convolution conv_f16_kernel<MB, taps, NB, WL>, persistent routes off.  OB = ceil(O / 32): MB = 4 for OB > 2, 2 for
    # OB > 1 (NB = 1); NB = 2 (8 x 32 pixel tiles) when the stride-1 grid is wider than 16, then MB = 2 for OB > 1
    **{f'conv_w16_o{o}': G9(lambda o=o: conv(1, 32, o, 8, 16), K(mb, 9, 1)) for o, mb in ((32, 1), (33, 2), (64, 2), (65, 4), (96, 4), (97, 4))},
    **{f'conv_w17_o{o}': G9(lambda o=o: conv(1, 32, o, 8, 17), K(mb, 9, 2)) for o, mb in ((32, 1), (33, 2), (64, 2), (65, 2), (96, 2), (97, 2))},
    # I >= 384: the weight slab of a chunk goes through LDS, for MB <= 2 only
    'conv_i352_o64_w16': G9(lambda: conv(1, 352, 64, 8, 16), K(2, 9, 1)),
    'conv_i384_o64_w16_wlds': G9(lambda: conv(1, 384, 64, 8, 16), K(2, 9, 1, True)),
    'conv_i352_o64_w17': G9(lambda: conv(1, 352, 64, 8, 17), K(2, 9, 2)),
    'conv_i384_o64_w17_wlds': G9(lambda: conv(1, 384, 64, 8, 17), K(2, 9, 2, True)),
    'conv_i352_o128_w16': G9(lambda: conv(1, 352, 128, 8, 16), K(4, 9, 1)),
    'conv_i384_o128_w16_no_wlds': G9(lambda: conv(1, 384, 128, 8, 16), K(4, 9, 1)),
    'conv_i384_o32_w16_wlds': G9(lambda: conv(1, 384, 32, 8, 16, bias=True), K(1, 9, 1, True)),
    'conv_i384_o32_w17_wlds': G9(lambda: conv(1, 384, 32, 8, 17, bias=True), K(1, 9, 2, True)),
    'conv_1x1_w16': G9(lambda: conv(2, 32, 32, 9, 16, k=1, pad=0, bias=True), K(1, 1, 1)),
    'conv_1x1_w17': G9(lambda: conv(2, 32, 32, 9, 17, k=1, pad=0, bias=True), K(1, 1, 2)),
    'conv_s2_routes_off': G9(lambda: conv(1, 64, 64, 17, 37, stride=2, pad=0), K(2, 9, 1)),      # stride-2 reads keep 8 x 16 tiles at any width
    # the transposed form per phase: grids of W + 1 and W columns (W = 8: NB = 1 everywhere; W = 20: NB = 2 everywhere)
    'convT_phases_w8_o32': T4(32, 32, 5, 8, 1, 1),
    'convT_phases_w8_o64': T4(32, 64, 5, 8, 2, 1),
    'convT_phases_w8_o128': T4(32, 128, 5, 8, 4, 1),
    'convT_phases_w20_o32': T4(32, 32, 5, 20, 1, 2),
    'convT_phases_w20_o64': T4(64, 64, 5, 20, 2, 2),
    # ---- eligibility of the persistent kernels, every route on.  Ring (3x3 stride 1): O % 8 == 0, no in_scale, no residual, noise only
    # with OW % 4 == 0
    'ring_o40': C(lambda: conv(1, 32, 40, 8, 16), [RING], [GATHER], routes=7),
    'ring_o36_gather': C(lambda: conv(1, 32, 36, 8, 16), [K(2, 9, 1)], others(K(2, 9, 1)) + [RING], routes=7),
    'ring_out_scale_bias_act': C(lambda: conv(2, 32, 40, 8, 16, bias=True, out_scale=True, act=True), [RING], [GATHER], routes=7),
    'ring_in_scale_gather': C(lambda: conv(2, 32, 40, 8, 16, in_scale=True), [K(2, 9, 1)], others(K(2, 9, 1)) + [RING], routes=7),
    'ring_residual_gather': C(lambda: conv(2, 32, 40, 8, 16, bias=True, act=True, residual=True), [K(2, 9, 1)], others(K(2, 9, 1)) + [RING], routes=7),
    'ring_noise_ow20': C(lambda: conv(2, 32, 40, 8, 20, noise='per', bias=True, act=True), [RING], [GATHER], routes=7),
    'ring_noise_ow18_gather': C(lambda: conv(2, 32, 40, 8, 18, noise='per', bias=True, act=True), [K(2, 9, 2)], others(K(2, 9, 2)) + [RING], routes=7),
    # down (3x3 stride 2): I <= 128, no noise
    'down_i128': C(lambda: conv(1, 128, 32, 17, 19, stride=2, pad=0), [DOWN], [GATHER], routes=7),
    'down_i160_gather': C(lambda: conv(1, 160, 32, 17, 19, stride=2, pad=0), [K(1, 9, 1)], others(K(1, 9, 1)) + [DOWN], routes=7),
    'down_i128_bias_act': C(lambda: conv(2, 128, 32, 17, 19, stride=2, pad=1, bias=True, act=True), [DOWN], [GATHER], routes=7),
    'down_i128_noise_gather': C(lambda: conv(2, 128, 32, 17, 19, stride=2, pad=1, noise='shared', bias=True, act=True), [K(1, 9, 1)], others(K(1, 9, 1)) + [DOWN], routes=7),
    # upring (the transposed form in one launch): no bias, I <= 512
    'upring_i512': C(lambda: convT(1, 512, 32, 5, 8), [UPRING], [GATHER], routes=7),
    'upring_i544_gather': C(lambda: convT(1, 544, 32, 5, 8), [K(1, 4, 1), K(1, 2, 1), K(1, 1, 1)], others(K(1, 4, 1), K(1, 2, 1), K(1, 1, 1)) + [UPRING], routes=7),
    'upring_i512_pad1': C(lambda: convT(2, 512, 40, 5, 8, pad=1), [UPRING], [GATHER], routes=7),
    'upring_bias_gather': C(lambda: convT(1, 512, 32, 5, 8, bias=True), [K(1, 4, 1), K(1, 2, 1), K(1, 1, 1)], others(K(1, 4, 1), K(1, 2, 1), K(1, 1, 1)) + [UPRING], routes=7),
}


def mangled(pattern):
    """The Itanium fragment of ``name<ints / bools>`` (namespaces as ``a::b``): the profiler reports kernels whose signature has a
    ``_Float16`` pointer by their mangled symbol (``_ZN3f1619bias_act_f16_kernelILb1EEEvPKDF16_...``)."""
    m = re.fullmatch(r'([\w:]+)(?:<(.*)>)?', pattern.replace(' ', ''))
    s = ''.join(f'{len(p)}{p}' for p in m.group(1).split('::'))
    if m.group(2) is not None:
        s += 'I' + ''.join({'true': 'Lb1E', 'false': 'Lb0E'}.get(a, f'Li{a}E') for a in m.group(2).split(',')) + 'E'
    return s


def _ok(pattern, names):
    frag = mangled(pattern)
    return any_hit(pattern, names) or any(n.startswith('_Z') and frag in n for n in names)


def _tensors(out):
    return [t for t in (out if isinstance(out, (list, tuple)) else [out]) if t is not None]


@pytest.mark.parametrize('case', sorted(CASES))
def test_route(case):
    builder, expect, forbid, switches = CASES[case]
    lib = _lib()
    old = lib.shg_conv2d_f16_set_routes(switches['routes']) if 'routes' in switches else None
    try:
        call, judge = builder()
        for _ in range(3):                                   # (the tracer occasionally drops the events of a short region: route_probe)
            got, names = launched(call)
            if all(_ok(p, names) for p in expect):
                break
        again = call() if switches.get('twice') else None
        torch.cuda.synchronize()
    finally:
        if old is not None:
            lib.shg_conv2d_f16_set_routes(old)
    kern = sorted(n for n in names if 'kernel' in n)
    for p in expect:
        assert _ok(p, names), f'{case}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not _ok(p, names), f'{case}: {p} must not run; ran {kern}'
    if again is not None:
        assert all(torch.equal(a, b) for a, b in zip(_tensors(got), _tensors(again))), f'{case}: two runs differ'
    records = judge(got)
    print(f'ROUTE {case} ' + ' '.join(f'{label}: rel_err={v:.3e} (bar {bar:.0e})' for label, v, bar, _ in records))
    for label, v, bar, strict in records:
        assert (v < bar) if strict else (v <= bar), f'{case}: {label} {v:.3e} exceeds {bar:.0e}'


# Every kernel launched from the fp16 sources (F16_SOURCES: their hipLaunchKernelGGL sites, and the persistent_launch<kernel> sites of the
# three persistent convolutions), with the instantiation where the site picks one.
ROUTE_KERNELS = (
    ALL_GATHER
    + [RING, UPRING, DOWN, WG31, WG32, WG11] + [f'{RED}<{g}>' for g in (1, 2, 4, 8, 16)]
    + [MARCH, SAME, f'{UPDN}<1, 2>', f'{UPDN}<2, 1>', GENERIC]
    + [f'{THIN}<true>', f'{THIN}<false>', TO_H, TO_F, f'{BA}<true>', f'{BA}<false>', BAB, f'{MT}<true>', f'{MT}<false>', MTB]
)

# launched from those files but left out of the table, and why
NOT_ROUTED = {
    'pack_weight_f16_kernel': 'weight preparation from the staged [T][O][I] copy: one kernel, no choice; test_direct_weight_pack_equals_the_staged_pack '
                              '(test_gpu_fp16.py) compares its operand tensor with the direct pack',
    'pack_weight_oihw_f16_kernel': 'weight preparation straight from the torch layout: one kernel, no choice; every convolution case above consumes '
                                   'its output, and test_direct_weight_pack_equals_the_staged_pack covers its transposed / rotated forms',
}

F16_SOURCES = ('conv_f16.hip', 'conv_wgrad_f16.hip', 'upfirdn2d_f16.hip', 'pointwise_f16.hip', 'conv_f16_ring.hip', 'conv_f16_upring.hip', 'conv_f16_down.hip')


def test_route_table_covers_every_kernel():
    """Every kernel / instantiation the float16 entry points can launch is the expected route of at least one case (host-only: no launch)."""
    expected = {p.replace(' ', '') for _, (_, exp, _, _) in CASES.items() for p in exp}
    missing = [k for k in ROUTE_KERNELS if k.replace(' ', '') not in expected]
    assert not missing, f'kernels without a route case: {missing}'
    assert len(set(ROUTE_KERNELS)) == len(ROUTE_KERNELS)


def test_route_table_names_every_launch_site():
    """Every launch site of the fp16 sources launches a kernel of ROUTE_KERNELS or of NOT_ROUTED, and the table names no kernel those
    sources do not launch (host-only: reads the sources)."""
    sites = set()
    for name in F16_SOURCES:
        with open(os.path.join(ROOT, 'sh-gan_amd', 'csrc', name)) as fh:
            sites |= {m.split('::')[-1] for m in re.findall(r'(?:hipLaunchKernelGGL\(\(?|persistent_launch<)\s*([\w:]+)', fh.read())}
    assert len(sites) >= 19, sorted(sites)
    table = {re.match(r'[\w:]+', k).group(0).split('::')[-1] for k in ROUTE_KERNELS} | set(NOT_ROUTED)
    assert sites == table, (sorted(sites - table), sorted(table - sites))
