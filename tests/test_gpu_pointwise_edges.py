"""The single-kernel pointwise entry points of csrc/pointwise.hip at their edges (run with -m gpu on an MI355X).

These kernels sit behind no dispatch predicate, so the route tables leave them out (NOT_ROUTED of tests/test_gpu_routes_fp32.py); they still
have edges: a capped grid with a grid-stride loop for the rest, unrolled loops with tails, channel slices, stride plans with a fallback and
argument checks.  One case per edge, at the smallest size that reaches it.

Bars.  Whatever only moves or sums data runs on integer-valued float32 in [-8, 8] with dyadic activation constants (act_gain 1, gain 2,
alpha 0.25, an integer clamp): every product and partial sum is exact in float32 in any order (all sums stay far below 2^24), so the bar
is ``torch.equal`` with the float64 reference rounded to float32 -- no tolerance; a misindexed block changes about 94 % of its elements.
Where the arithmetic itself is under test the data is random normal and the bars are the project's existing ones: TOL_PW = 1e-5 for
elementwise passes, 2e-5 for the tail backward, bit equality with torch's CPU operators for the casts, the uint8 composite and the input
assembly, as the kernels' comments claim.  ``test_second_trip_cases_exceed_the_caps`` (host-only) reads the caps out of the source, so a
changed cap cannot quietly turn a second-trip case into a one-trip case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from route_probe import any_hit, launched
from test_gpu_routes_fp32 import TOL_PW, _on_clamp_values, act64, dev, rnd

gpu = pytest.mark.gpu
DEV = 'cuda:0'
TOL_TAIL = 2e-5                                   # the tail backward (the round5 fuzz family, tests/test_gpu_alloc_fill.py)
ACT = dict(act_gain=1.0, gain=2.0, alpha=0.25)    # dyadic: an integer stays a multiple of 1/8

# Sizes of the second-trip cases, in the unit one lane handles per trip (elements, float4, units of four pixels; outputs for the workgroup
# mapping of mul_reduce, where a workgroup owns one output): entry point -> sizes in the order of its capped launch sites in the source.
SECOND_TRIP = {
    'shg_fma_f32': [4096 * 256 + 3],
    'shg_fma_bcast': [8192 * 256 + 257],
    'shg_scale_channels_f32': [3 * 349527],
    'shg_scale_cast_f32_f16': [2048 * 256 + 1],
    'shg_composite_u8': [6 * 3 * 512 * 512 // 4],
    'shg_minibatch_std_f32': [4 * (16 + 1) * 128 * 128],
    'shg_bias_act_f32': [4096 * 256 + 1, 4096 * 256 + 3],           # the float4 kernel's site comes first
    'shg_bias_act_backward_f32': [4096 * 256 + 3],
    'shg_mul_reduce': [65537],
}
LANES = {'shg_mul_reduce': 1}                     # units per workgroup and trip (256 lanes everywhere else)


def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def _lib():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib
    return _lib


def ints(seed, *shape, dtype=torch.float32, lo=-8, hi=8):
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi + 1, size=shape)).to(dtype)


def same_bits(got, ref64, what=''):
    """torch.equal with the float64 reference rounded to the result's dtype."""
    got = got.detach().cpu()
    ref = ref64.to(got.dtype)
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).reshape(-1)
        first = int(bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {ref.numel()} elements differ, first at flat index {first}: '
                             f'{got.reshape(-1)[first].item()!r} for {ref.reshape(-1)[first].item()!r}')


def ran(call, kernel):
    """call() under the profiler: its result, after asserting that ``kernel`` ran (the tracer does not demangle symbols with _Float16 parameters:
    those are named by the head of the mangled symbol)."""
    out, names = launched(call, expect=[kernel])
    assert any_hit(kernel, names), f'expected {kernel}; ran {sorted(n for n in names if "kernel" in n)}'
    return out


def raises_without_launch(call, kernel, match):
    """call() must raise ShgError before anything of ``kernel`` is enqueued."""
    def guarded():
        with pytest.raises(_lib().ShgError, match=match):
            call()
    _, names = launched(guarded)
    assert not any_hit(kernel, names), f'{kernel} was launched although the arguments were refused'


# ------------------------------------------------------------------------------------------------
# fma through kernels.fma (fma_bcast_kernel<float|double>) and the public op
# ------------------------------------------------------------------------------------------------
SEVEN = ((2, 3, 2, 3, 2, 3, 2), (1, 3, 1, 3, 1, 3, 1), (2, 1, 2, 1, 2, 1, 2))
BCAST = {torch.float32: 'fma_bcast_kernel<float>', torch.float64: 'fma_bcast_kernel<double>'}


def _fma_check(ops, dtype, what):
    kk = _kk()
    d = [None if t is None else t.to(DEV) for t in ops]
    ref = ops[0].double() * ops[1].double()
    if ops[2] is not None:
        ref = ref + ops[2].double()
    got = ran(lambda: kk.fma(*d), BCAST[dtype])
    assert got.dtype == dtype and got.is_contiguous()
    same_bits(got, ref, what)


def fma_second_trip(dtype):
    n = SECOND_TRIP['shg_fma_bcast'][0]
    _fma_check([ints(1, n, dtype=dtype), ints(2, 1, dtype=dtype), ints(3, n, dtype=dtype)], dtype, 'second trip, ragged tail')


def fma_six_dims(dtype):
    _fma_check([ints(4, 2, 3, 2, 3, 2, 3, dtype=dtype), ints(5, 1, 3, 1, 3, 1, 3, dtype=dtype), ints(6, 2, 1, 2, 1, 2, 1, dtype=dtype)], dtype, 'six dimensions')
    plan = _kk().fma_plan(torch.zeros(2, 3, 2, 3, 2, 3), torch.zeros(1, 3, 1, 3, 1, 3), torch.zeros(2, 1, 2, 1, 2, 1))
    assert len(plan.cshape) == 6


def fma_seven_dims(dtype):
    """The fallback above six dimensions, forward and all three gradients through the public op, against float64 autograd of a*b+c."""
    import shgan_amd  # noqa: F401
    from shgan_amd.model_zoo.stylegan_utils import fma as fma_mod
    ops = [ints(7 + k, *s, dtype=dtype) for k, s in enumerate(SEVEN)]
    go = ints(10, *SEVEN[0], dtype=dtype)
    assert len(_kk().fma_plan(*ops).cshape) == 1 and _kk().fma_plan(*ops).ops[1].numel() == ops[0].numel()
    _fma_check(ops, dtype, 'seven dimensions')
    with torch.enable_grad():
        r = [t.double().requires_grad_(True) for t in ops]
        rg = torch.autograd.grad(r[0] * r[1] + r[2], r, go.double())
        d = [t.to(DEV).requires_grad_(True) for t in ops]
        y = fma_mod.fma(*d)
        same_bits(y, (r[0] * r[1] + r[2]).detach(), 'public op, seven dimensions')
        grads = torch.autograd.grad(y, d, go.to(DEV))
    for name, got, want in zip('abc', grads, rg):
        same_bits(got, want, f'd{name}, seven dimensions')


def fma_c_none(dtype):
    _fma_check([ints(11, 4, 1, 3, dtype=dtype), ints(12, 2, 1, 5, 1, dtype=dtype), None], dtype, 'c = None')


def fma_sliced_view(dtype):
    a = ints(13, 3, 6, 23, dtype=dtype)[:, 1:5, 3:21:2]                  # storage offset 26, strides (138, 23, 2)
    b = ints(14, 4, 40, dtype=dtype)[:, 5:23:2]
    c = ints(15, 9, 4, dtype=dtype).t()[None]                            # transposed: strides (.., 1, 4)
    assert a.storage_offset() == 26 and a.stride(-1) == 2 and not a.is_contiguous()
    kk = _kk()
    ad, bd, cd = (t.to(DEV) for t in (ints(13, 3, 6, 23, dtype=dtype), ints(14, 4, 40, dtype=dtype), ints(15, 9, 4, dtype=dtype)))
    ad, bd, cd = ad[:, 1:5, 3:21:2], bd[:, 5:23:2], cd.t()[None]
    assert ad.storage_offset() == 26 and ad.stride() == a.stride() and kk.fma_plan(ad, bd, cd).ops[0].data_ptr() == ad.data_ptr()
    same_bits(ran(lambda: kk.fma(ad, bd, cd), BCAST[dtype]), a.double() * b.double() + c.double(), 'sliced view, inner stride 2')


def fma_zero_elements(dtype):
    kk = _kk()
    a, b, c = torch.zeros(3, 0, 2, dtype=dtype, device=DEV), torch.ones(1, 2, dtype=dtype, device=DEV), torch.ones(3, 1, 1, dtype=dtype, device=DEV)
    y, names = launched(lambda: kk.fma(a, b, c))
    assert tuple(y.shape) == (3, 0, 2) and y.dtype == dtype and not any_hit('fma_bcast_kernel', names)
    # an empty batch through the public op: the gradients of the broadcast operands are sums of no terms
    from shgan_amd.model_zoo.stylegan_utils import fma as fma_mod
    shapes = ((0, 3, 2), (1, 3, 1), (2,))
    with torch.enable_grad():
        r = [ints(22 + k, *s, dtype=torch.float64).requires_grad_(True) for k, s in enumerate(shapes)]
        rg = torch.autograd.grad(r[0] * r[1] + r[2], r, torch.zeros(0, 3, 2, dtype=torch.float64))
        d = [t.detach().to(dtype).to(DEV).requires_grad_(True) for t in r]
        y = fma_mod.fma(*d)
        assert tuple(y.shape) == (0, 3, 2)
        grads = torch.autograd.grad(y, d, torch.zeros(0, 3, 2, dtype=dtype, device=DEV))
    for name, got, want in zip('abc', grads, rg):
        same_bits(got, want, f'd{name}, empty batch')


def _cancellation(seed, n):
    """a, b normal; c = -float32(a * b): a fused multiply-add returns the exact residual of the float32 product, an unfused one 0."""
    a, b = rnd(seed, n), rnd(seed + 1, n)
    p = a.double() * b.double()                                           # exact: 48 significant bits
    c = -(p.float())
    want = p + c.double()                                                 # exact: the residual of a rounding is representable
    assert torch.equal(want.float().double(), want) and float((want != 0).float().mean()) > 0.9
    return a, b, c, want


def fma_cancellation(dtype):
    assert dtype == torch.float32
    a, b, c, want = _cancellation(16, 4099)
    kk = _kk()
    ad, bd, cd = a.to(DEV), b.to(DEV), c.to(DEV)
    same_bits(ran(lambda: kk.fma(ad, bd, cd), BCAST[dtype]), want, 'one rounding (fused)')


def fma_f32_entry_second_trip(dtype):
    """shg_fma_f32 (fma_kernel) has no Python wrapper: through the C interface."""
    assert dtype == torch.float32
    lm = _lib()
    lib = lm.get_lib()
    n = SECOND_TRIP['shg_fma_f32'][0]
    a, b, c = ints(18, n), ints(19, n), ints(20, n)
    ca, cb, cc, want = _cancellation(21, n)

    def call(x, y, z):
        xd, yd, zd = x.to(DEV), y.to(DEV), z.to(DEV)
        out = torch.empty(n, device=DEV)
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in (xd, yd, zd, out)]

        def go():
            lm.check(lib.shg_fma_f32(*ptr, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'fma_f32')
            return out
        return ran(go, 'fma_kernel')
    same_bits(call(a, b, c), a.double() * b.double() + c.double(), 'fma_kernel second trip')
    same_bits(call(ca, cb, cc), want, 'fma_kernel: one rounding (fused)')


# ------------------------------------------------------------------------------------------------
# mul_reduce
# ------------------------------------------------------------------------------------------------
MULRED = {torch.float32: 'mul_reduce_kernel<float>', torch.float64: 'mul_reduce_kernel<double>'}


def _unbroadcast64(g, b, shape):
    p = g.double() * b.double() if b is not None else g.double()
    full = (1,) * (g.ndim - len(shape)) + tuple(shape)
    dims = [i for i in range(g.ndim) if full[i] == 1]
    return (p.sum(dims, keepdim=True) if dims else p).reshape(tuple(shape))


def _mul_reduce_check(g, b, shape, what, inner_kept=None, dtype=torch.float32):
    kk = _kk()
    gd, bd = g.to(DEV), (None if b is None else b.to(DEV))
    if inner_kept is not None:
        assert kk.mul_reduce_plan(gd, bd, shape).inner_kept == inner_kept, what
    got = ran(lambda: kk.mul_reduce(gd, bd, shape), MULRED[dtype])
    assert got.dtype == dtype
    same_bits(got, _unbroadcast64(g, b, shape), what)


def mul_reduce_workgroup_lengths():
    """A workgroup per output, 3 outputs, reduced length below, at and past the 256 lanes; length 1 can only be asked of the C interface
    (the plan of a size-1 reduction has nothing to reduce and takes the thread mapping)."""
    for r in (255, 256, 257, 513):
        _mul_reduce_check(ints(30 + r, 3, r), ints(31 + r, 1, r), (3, 1), f'workgroup mapping, reduced length {r}', inner_kept=0)
    lm = _lib()
    g, b = ints(32, 3, 1), ints(33, 3, 1)
    gd, bd, out = g.to(DEV), b.to(DEV), torch.empty(3, device=DEV)
    arr = lambda *v: (ctypes.c_long * len(v))(*v)                        # noqa: E731

    def go():
        lm.check(lm.get_lib().shg_mul_reduce(ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(out.data_ptr()), 2, 1, arr(3, 1),
                                              arr(1, 1), arr(1, 1), 0, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mul_reduce')
        return out
    same_bits(ran(go, MULRED[torch.float32]), (g.double() * b.double()).reshape(3), 'workgroup mapping, reduced length 1')


def mul_reduce_workgroup_second_trip():
    n = SECOND_TRIP['shg_mul_reduce'][0]
    _mul_reduce_check(ints(34, n, 2), ints(35, 1, 2), (n, 1), 'workgroup mapping, 65537 outputs', inner_kept=0)


def mul_reduce_thread_mapping():
    _mul_reduce_check(ints(36, 3, 257), ints(37, 3, 1), (1, 257), 'thread mapping, 257 outputs, reduced length 3', inner_kept=1)
    _mul_reduce_check(ints(38, 1, 257), ints(39, 1, 257), (1, 257), 'thread mapping, 257 outputs, reduced length 1', inner_kept=1)
    _mul_reduce_check(ints(40, 2, 257), None, (257,), 'thread mapping, leading dimension dropped', inner_kept=1)


def mul_reduce_interleaved():
    g, b = ints(41, 2, 3, 2, 3, 2, 3), ints(42, 1, 3, 1, 3, 1, 3)
    assert len(_kk().mul_reduce_plan(g, b, (2, 1, 2, 1, 2, 1)).cshape) == 6
    _mul_reduce_check(g, b, (2, 1, 2, 1, 2, 1), 'three kept dimensions between three reduced ones')
    _mul_reduce_check(g, ints(43, 2, 1, 2, 1, 2, 1), (1, 3, 1, 3, 1, 3), 'three reduced dimensions between three kept ones')


def mul_reduce_permuted_fallback():
    g, a = ints(44, *SEVEN[0]), ints(45, *SEVEN[0])
    plan = _kk().mul_reduce_plan(g, a, SEVEN[1])
    assert plan.cshape == [27, 16] and plan.nk == 1
    _mul_reduce_check(g, a, SEVEN[1], 'seven dimensions: kept in front', inner_kept=0)
    _mul_reduce_check(g.permute(6, 5, 4, 3, 2, 1, 0), ints(46, *SEVEN[2]).permute(6, 5, 4, 3, 2, 1, 0), SEVEN[2][::-1], 'seven dimensions, transposed')


def mul_reduce_b_none():
    _mul_reduce_check(ints(47, 3, 5, 300), None, (3, 1, 1), 'b = None, workgroup mapping', inner_kept=0)
    _mul_reduce_check(ints(48, 3, 5, 300), None, (5, 300), 'b = None, thread mapping', inner_kept=1)


def mul_reduce_float64():
    f64 = torch.float64
    _mul_reduce_check(ints(49, 3, 257, dtype=f64), ints(50, 1, 257, dtype=f64), (3, 1), 'float64, workgroup mapping', inner_kept=0, dtype=f64)
    _mul_reduce_check(ints(51, 3, 257, dtype=f64), ints(52, 3, 1, dtype=f64), (257,), 'float64, thread mapping', inner_kept=1, dtype=f64)
    _mul_reduce_check(ints(53, *SEVEN[0], dtype=f64), ints(54, *SEVEN[0], dtype=f64), SEVEN[1], 'float64, seven dimensions', dtype=f64)


def mul_reduce_empty_to_zeros():
    kk = _kk()
    for dtype in (torch.float32, torch.float64):
        g = torch.zeros(0, 3, dtype=dtype, device=DEV)
        for b in (None, torch.ones(1, 3, dtype=dtype, device=DEV)):
            for _ in range(4):
                junk = torch.full((1, 3), float('nan'), dtype=dtype, device=DEV)          # what a recycled block may hold
                del junk
                out = kk.mul_reduce(g, b, (1, 3))
                same_bits(out, _unbroadcast64(g.cpu(), None if b is None else b.cpu(), (1, 3)), 'empty reduction')
                assert out.dtype == dtype and float(out.abs().sum()) == 0.0
        assert tuple(kk.mul_reduce(g, None, (0, 3)).shape) == (0, 3)


# ------------------------------------------------------------------------------------------------
# sum_partials
# ------------------------------------------------------------------------------------------------

def sum_partials_tails():
    """B on both sides of the 16-row unrolled loop and of its 4-row tail, K on both sides of the 64 columns of a workgroup."""
    kk = _kk()
    for b in (1, 3, 4, 5, 13, 16, 17, 29, 33):
        for k in (1, 63, 64, 65):
            part = ints(60 + b * 100 + k, 2, b, k)
            pd = part.to(DEV)
            same_bits(kk.sum_partials(pd), part.double().sum(1), f'B={b} K={k}')
    part = ints(61, 2, 17, 2, 5)                                          # trailing dimensions are one run of K = 10
    pd = part.to(DEV)
    same_bits(ran(lambda: kk.sum_partials(pd), 'sum_partials_kernel'), part.double().sum(1), 'B=17, K = 2 x 5')


# ------------------------------------------------------------------------------------------------
# modtail_backward
# ------------------------------------------------------------------------------------------------
CLAMP = 4.0                                       # x gain 2: |y| >= 8 has zero slope


def _tail_case(n, c, h, w, seed, t=True, d=True, u=False, e=False, act=True, normal=False):
    mk = (lambda s, *shape: rnd(s, *shape)) if normal else (lambda s, *shape: ints(s, *shape))
    gy = mk(seed, n, c, h, w)
    y = _on_clamp_values(n * c * h * w, CLAMP * ACT['gain']).view(n, c, h, w)
    if n * c * h * w > 64:                                                # the edge values into other channels and blocks as well
        flat = y.view(-1)
        flat[-6:] = flat[:6]
        flat[flat.numel() // 2:flat.numel() // 2 + 6] = flat[:6]
    ops = dict(t=mk(seed + 1, n, c, h, w) if t else None, d=mk(seed + 2, n, c) if d else None, u=mk(seed + 3, n, c, h, w) if u else None,
               e=mk(seed + 4, n, c) if e else None)
    yd = y.double()
    if act:
        g_, a_ = ACT['gain'] * ACT['act_gain'], ACT['alpha']
        slope = torch.where(yd.abs() >= CLAMP * ACT['gain'], torch.zeros_like(yd), torch.where(yd > 0, torch.full_like(yd, g_), torch.full_like(yd, a_ * g_)))
    else:
        slope = torch.full_like(yd, ACT['gain'])
    gz = gy.double() * slope
    gt = gz * (ops['d'].double().view(n, c, 1, 1) if d else 1.0)
    if u:
        gt = gt + ops['u'].double() * slope * (ops['e'].double().view(n, c, 1, 1) if e else 1.0)
    tt = ops['t'].double() if t else torch.zeros_like(gz)
    ref = dict(gt=gt, s1=(gz * tt).sum([2, 3]), s0=gz.sum([2, 3]), gnoise=gz.sum(1, keepdim=True))
    return gy, y, ops, ref


def _tail_run(n, c, h, w, seed, slices=None, want_sums=True, want_noise=True, what='', normal=False, **opt):
    kk = _kk()
    gy, y, ops, ref = _tail_case(n, c, h, w, seed, normal=normal, **opt)
    if slices is not None:
        assert _lib().get_lib().shg_modtail_backward_f32_cslices(n, c, h * w) == slices, what
    act = opt.get('act', True)
    kw = dict(act=act, clamp=CLAMP, **ACT) if act else dict(act=False, gain=ACT['gain'])
    dv = {k: (None if v is None else v.to(DEV)) for k, v in ops.items()}
    gyd, ydv = gy.to(DEV), y.to(DEV)
    out = ran(lambda: kk.modtail_backward(gyd, ydv, dv['t'], dv['d'], want_sums=want_sums, want_noise=want_noise, u=dv['u'], e=dv['e'], **kw),
              'modtail_backward_f32_kernel')
    for name, got in zip(('gt', 's1', 's0', 'gnoise'), out):
        wanted = name == 'gt' or (want_sums if name in ('s1', 's0') else want_noise)
        assert (got is not None) == wanted, (what, name)
        if got is None:
            continue
        if normal:
            err = rel_err(got.double().cpu().numpy(), ref[name].numpy())
            print(f'EDGE modtail {what} {name} rel_err={err:.3e}')
            assert tuple(got.shape) == tuple(ref[name].shape) and err < TOL_TAIL, (what, name, err)
        else:
            same_bits(got, ref[name], f'{what}: {name}')


def modtail_hw_4():
    _tail_run(2, 5, 2, 2, 70, slices=1, what='HW = 4', u=True, e=True)


def modtail_two_blocks():
    assert _lib().get_lib().shg_modtail_backward_f32_blocks(4 * 257) == 2
    _tail_run(2, 5, 4, 257, 71, slices=1, what='HW = 4 * 257', u=True, e=True)


def modtail_two_slices():
    _tail_run(1, 16, 4, 4, 72, slices=2, what='C = 16: two slices', u=True, e=True)


def modtail_last_slice_empty():
    _tail_run(1, 81, 4, 4, 73, slices=10, what='C = 81: ten slices, the last empty', u=True, e=True)
    _tail_run(1, 89, 4, 4, 74, slices=11, what='C = 89: eleven slices, the last starts past C', u=True, e=True)


def modtail_full_table():
    _tail_run(1, 512, 2, 2, 75, slices=64, what='C = 512: 64 slices', u=True, e=True)
    _tail_run(3, 512, 2, 6, 76, what='C = 512, N = 3', u=True, e=True)
    assert _lib().get_lib().shg_modtail_backward_f32_cslices(512, 512, 4) == 1
    _tail_run(512, 512, 2, 2, 77, slices=1, what='C = 512 in one slice: the whole LDS table')


def modtail_optional_operands():
    shape = (2, 5, 4, 6)
    _tail_run(*shape, 78, what='t = None', t=False)
    _tail_run(*shape, 79, what='d = None', d=False)
    _tail_run(*shape, 80, what='u without e', u=True)
    _tail_run(*shape, 81, what='u with e', u=True, e=True)
    _tail_run(*shape, 82, what='act = False', act=False, u=True, e=True)
    _tail_run(*shape, 83, what='sums alone', want_noise=False)
    _tail_run(*shape, 84, what='noise alone', want_sums=False)
    _tail_run(*shape, 85, what='gt alone', want_sums=False, want_noise=False)


def modtail_arithmetic():
    """Random normal operands at the sliced and the two-block shape: the existing 2e-5 bar of the tail backward."""
    _tail_run(1, 81, 4, 4, 86, what='normal, C = 81', normal=True, u=True, e=True)
    _tail_run(2, 5, 4, 257, 87, what='normal, HW = 4 * 257', normal=True, u=True, e=True)


def modtail_refusals():
    kk = _kk()
    gy, y = torch.zeros(1, 513, 2, 2, device=DEV), torch.zeros(1, 513, 2, 2, device=DEV)
    raises_without_launch(lambda: kk.modtail_backward(gy, y), 'modtail_backward_f32_kernel', 'C <= 512')
    g1, y1 = dev(ints(88, 2, 5, 4, 6), offset=1), ints(89, 2, 5, 4, 6).to(DEV)
    assert g1.is_contiguous() and g1.data_ptr() % 16 == 4
    raises_without_launch(lambda: kk.modtail_backward(g1, y1), 'modtail_backward_f32_kernel', '16-byte aligned')
    raises_without_launch(lambda: kk.modtail_backward(y1, y1, t=g1), 'modtail_backward_f32_kernel', '16-byte aligned')


# ------------------------------------------------------------------------------------------------
# scale_cast
# ------------------------------------------------------------------------------------------------

def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _placed_for_half(gain):
    """float32 inputs whose product with ``gain`` (a power of two: exact) is: every halfway point between adjacent halves around 1, 2048
    and the largest normals (ties to even, both ways) and one float32 ulp either side; 65504, 65520 (the first value that rounds to
    infinity) and their neighbours; the half denormals, halfway points between them and the smallest normal; +-0."""
    f32 = np.float32
    hs = np.array([1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, 1.5, 2.0 - 2.0 ** -10, 2047.0, 2048.0, 2050.0, 65472.0, 65504.0 - 32.0, 2.0 ** -14, 2.0 ** -14 + 2.0 ** -24], np.float16)
    nxt = np.nextafter(hs, np.float16(np.inf))
    mid = (hs.astype(f32) + nxt.astype(f32)) / f32(2)
    den = np.array([1, 2, 3, 512, 1022, 1023, 1024], f32) * f32(2.0 ** -24)           # denormals and the smallest normal (1024 * 2^-24 = 2^-14)
    den_mid = (np.array([0, 1, 2, 3, 1022, 1023], f32) + f32(0.5)) * f32(2.0 ** -24)    # 2^-25: ties to 0; 3 * 2^-25: ties to 2^-23
    top = np.array([65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e6], f32)
    v = np.concatenate([mid, hs.astype(f32), den, den_mid, top])
    v = np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(0))])
    v = np.concatenate([v, -v, np.array([0.0, -0.0], f32)])
    x = (v / f32(gain)).astype(f32)
    assert np.array_equal(x * f32(gain), v)
    return torch.from_numpy(x)


def scale_cast_to_half():
    """Bit equality with ``(x * gain).to(torch.float16)`` of torch's CPU operators, the signs of zero included.  (This case found the
    one class on which the kernel used to differ: a product of exactly -0 came back as +0, and only for the elements the remainder of
    the compiler's unrolled loop handled -- there the multiplication and the conversion were one v_fma_mixlo_f16 with a +0 addend.  The
    kernel now keeps the product in a register of its own.)"""
    kk = _kk()
    n = SECOND_TRIP['shg_scale_cast_f32_f16'][0]
    placed = _placed_for_half(0.5)
    for gain, what in ((0.5, 'placed values'), (0.37, 'any gain')):
        x = rnd(90, n) * 30
        x[:placed.numel()] = placed
        x[-placed.numel():] = placed                                      # in the second trip as well, the last element included
        ref = (x * gain).to(torch.float16)                                # torch's CPU operators: one float32 product, one rounding to half
        xd = x.to(DEV)
        got = ran(lambda: kk.scale_cast(xd, gain, True), '_Z25scale_cast_to_half_kernel')
        assert got.dtype == torch.float16 and got.is_contiguous()
        diff = (_bits(got) != _bits(ref)).nonzero().reshape(-1)
        assert diff.numel() == 0, (f'{what}: {diff.numel()} of {n} halves differ in their bits, first at {int(diff[0])}: x = {float(x[diff[0]])!r}, '
                                   f'got {float(got[diff[0]])!r} for {float(ref[diff[0]])!r}')


def scale_cast_to_float():
    kk = _kk()
    n = SECOND_TRIP['shg_scale_cast_f32_f16'][0]
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    every = every[~torch.isnan(every)]                                    # every half there is, the infinities included
    for gain in (1.0, 1.7, 2.0 ** -113):                                  # the last: products among the float32 denormals
        h = (rnd(91, n) * 30).to(torch.float16)
        h[:every.numel()] = every
        h[-every.numel():] = every
        ref = h.float() * gain
        hd = h.to(DEV)
        got = ran(lambda: kk.scale_cast(hd, gain, False), '_Z26scale_cast_to_float_kernel')
        assert got.dtype == torch.float32
        diff = (_bits(got) != _bits(ref)).nonzero().reshape(-1)
        assert diff.numel() == 0, (f'gain {gain}: {diff.numel()} of {n} floats differ in their bits, first at {int(diff[0])}: h = {float(h[diff[0]])!r}, '
                                   f'got {float(got[diff[0]])!r} for {float(ref[diff[0]])!r}')


# ------------------------------------------------------------------------------------------------
# scale_channels, planes_to_image
# ------------------------------------------------------------------------------------------------

def scale_channels_edges():
    kk = _kk()
    for nc, hw in ((3, 349527), (5, 1)):
        x, s = ints(92, 1, nc, 1, hw), ints(93, nc)
        xd, sd = x.to(DEV), s.to(DEV)
        same_bits(ran(lambda: kk.scale_channels(xd, sd), 'scale_channels_kernel'), x.double() * s.double().view(1, nc, 1, 1), f'NC={nc} HW={hw}')
    x, s = ints(94, 2, 3, 5, 7), ints(95, 6)
    same_bits(kk.scale_channels(x.to(DEV), s.to(DEV)), x.double() * s.double().view(2, 3, 1, 1), 'N=2 C=3')


def _planes_ref(mid, lo, oh, ow, bias):
    _, n, c, hp, wp = mid.shape
    h, w = hp - 1, wp - 1
    pad = 4
    canvas = torch.zeros(n, c, 2 * h + 1 + 2 * pad + oh, 2 * w + 1 + 2 * pad + ow, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            canvas[:, :, pad + a:pad + 2 * h + 1:2, pad + b:pad + 2 * w + 1:2] = mid[a * 2 + b][:, :, :h + 1 - a, :w + 1 - b].double()
    out = canvas[:, :, pad + lo:pad + lo + oh, pad + lo:pad + lo + ow]
    return out + bias.double().view(1, c, 1, 1) if bias is not None else out


def planes_to_image_edges():
    kk = _kk()
    rows = [('H = W = 1', 1, 1, 1, 1, 0, 3, 3, False), ('H = W = 1 with bias', 2, 3, 1, 1, 1, 2, 2, True),
            ('two column blocks', 1, 2, 2, 130, 1, 4, 260, True), ('257 columns', 2, 3, 1, 128, 0, 3, 257, True)]
    rows += [(f'lo = {lo}: past both ends', 2, 3, 2, 3, lo, 9, 11, bias) for lo in (-1, 0, 1, 2) for bias in (False, True)]
    for what, n, c, h, w, lo, oh, ow, with_bias in rows:
        mid, bias = ints(96, 4, n, c, h + 1, w + 1, lo=1), (ints(97, c) if with_bias else None)
        md, bd = mid.to(DEV), (bias.to(DEV) if with_bias else None)
        got = ran(lambda: kk.planes_to_image(md, lo, oh, ow, bias=bd), 'planes_to_image_kernel')
        ref = _planes_ref(mid, lo, oh, ow, bias)
        same_bits(got, ref, what)
        if lo == -1 and not with_bias:
            assert float(ref[:, :, 0].abs().sum()) == 0 and float(ref[:, :, :, -1].abs().sum()) == 0 and float(ref[:, :, 1, 1:8].abs().min()) > 0


# ------------------------------------------------------------------------------------------------
# composite_u8, assemble_input
# ------------------------------------------------------------------------------------------------

def _composite_inputs(n, h, w, seed, placed=False):
    rs = np.random.RandomState(seed)
    mask = torch.from_numpy((rs.rand(n, 1, h, w) < 0.6).astype(np.float32))
    real = torch.from_numpy(rs.randint(0, 256, (n, 3, h, w)).astype(np.float32)) / 127.5 - 1.0
    img = torch.from_numpy((rs.standard_normal((n, 3, h, w)) * 0.7).astype(np.float32))
    known = real * mask
    if placed:
        # v * 127.5 + 127.5 on every integer 0 .. 255 (as nearly as float32 has it), one ulp either side, below 0 and above 255: through
        # the known pixels where the mask is 1 and through the generated image where it is 0
        f32 = np.float32
        k = ((np.arange(-3, 260, dtype=np.float64) - 127.5) / 127.5).astype(f32)
        k = np.concatenate([k, np.nextafter(k, f32(-9)), np.nextafter(k, f32(9)), np.array([-1.5, 1.5, -0.0, 0.0, 1e3, -1e3], f32)])
        assert k.size * 2 <= h * w
        kt = torch.from_numpy(k)
        for ch in range(3):
            mask[0, 0].view(-1)[:k.size] = 1.0
            known[0, ch].view(-1)[:k.size] = kt
            mask[-1, 0].view(-1)[-k.size:] = 0.0
            known[-1, ch].view(-1)[-k.size:] = 0.0
            img[-1, ch].view(-1)[-k.size:] = kt
    return torch.cat([mask - 0.5, known], dim=1), img


def composite_u8_edges():
    from oracle import shgan_oracle as orc
    kk = _kk()
    for what, (n, h, w), placed in (('second trip', (6, 512, 512), True), ('2 x 2', (3, 2, 2), False), ('placed values', (2, 36, 60), True)):
        assert what != 'second trip' or n * 3 * h * w // 4 == SECOND_TRIP['shg_composite_u8'][0]
        x, img = _composite_inputs(n, h, w, 98, placed)
        want = orc.composite_u8(x, img)
        xd, imd = x.to(DEV), img.to(DEV)
        got = ran(lambda: kk.composite_u8(xd, imd), 'composite_u8_kernel')
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 3, h, w)
        diff = (got.cpu() != want).reshape(-1).nonzero().reshape(-1)
        assert diff.numel() == 0, f'{what}: {diff.numel()} of {want.numel()} bytes differ from the oracle, first at flat index {int(diff[0])}'
        if placed:
            assert int(want.min()) == 0 and int(want.max()) == 255 and len(torch.unique(want[0, 0].view(-1)[:800])) == 256


def assemble_input_edges():
    kk = _kk()
    for what, (n, h, w) in (('H W = 4', (3, 2, 2)), ('257 float4', (1, 2, 514)), ('two samples, 257 float4 each', (2, 2, 514))):
        rs = np.random.RandomState(99)
        real = torch.from_numpy(rs.uniform(-1, 1, (n, 3, h, w)).astype(np.float32))
        u8 = torch.from_numpy(rs.randint(0, 256, (n, 3, h, w)).astype(np.uint8))
        u8.view(-1)[:4] = torch.tensor([0, 255, 255, 0], dtype=torch.uint8)
        u8.view(-1)[-2:] = torch.tensor([255, 0], dtype=torch.uint8)
        mask = torch.from_numpy((rs.rand(n, 1, h, w) < 0.6).astype(np.float32))
        mask.view(-1)[:4] = 1.0
        mask.view(-1)[-2:] = 1.0
        rd, ud, md = real.to(DEV), u8.to(DEV), mask.to(DEV)
        got = ran(lambda: kk.assemble_input(rd, md), 'assemble_input_kernel')
        assert torch.equal(got.cpu(), torch.cat([mask - 0.5, real * mask], dim=1)), what
        got = ran(lambda: kk.assemble_input(ud, md[:, 0]), 'assemble_input_u8_kernel')
        want = torch.cat([mask - 0.5, kk.u8_value_table('cpu')[u8.long()] * mask], dim=1)
        assert torch.equal(got.cpu(), want), what
        assert float(want[0, 1].view(-1)[0]) == -1.0 and float(want[0, 1].view(-1)[1]) == 1.0
    buf = torch.zeros(2 * 3 * 4 * 4 + 4, dtype=torch.uint8, device=DEV)
    off = buf[1:1 + 96].view(2, 3, 4, 4)
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    mk = torch.ones(2, 1, 4, 4, device=DEV)
    raises_without_launch(lambda: kk.assemble_input(off, mk), 'assemble_input_u8_kernel', '4-byte aligned')


# ------------------------------------------------------------------------------------------------
# minibatch_std
# ------------------------------------------------------------------------------------------------

def _mbstd_check(n, c, h, w, group, f, what):
    kk = _kk()
    x = rnd(100, n, c, h, w)
    g = n if group is None else min(group, n)
    s = x.double().reshape(g, -1, f, c // f, h, w)
    s = (s - s.mean(dim=0)).square().mean(dim=0)
    s = (s + 1e-8).sqrt().mean(dim=[2, 3, 4]).reshape(-1, f, 1, 1).repeat(g, 1, h, w)
    xd = x.to(DEV)
    got = ran(lambda: kk.minibatch_std(xd, group, f), 'mbstd_write_kernel').cpu()
    assert tuple(got.shape) == (n, c + f, h, w)
    assert torch.equal(got[:, :c], x), f'{what}: the copied channels are not the input'
    err = rel_err(got[:, c:].double().numpy(), s.numpy())
    print(f'EDGE mbstd {what} rel_err={err:.3e}')
    assert err < TOL_PW, (what, err)
    assert float((got[:, c:] - got[:, c:, :1, :1]).abs().max()) == 0.0, f'{what}: the statistic is not constant over its plane'


def mbstd_second_trip():
    assert 4 * 17 * 128 * 128 == SECOND_TRIP['shg_minibatch_std_f32'][0]
    _mbstd_check(4, 16, 128, 128, 2, 1, 'N=4 C=16 128x128')


def mbstd_small_and_groups():
    _mbstd_check(4, 3, 5, 5, 2, 1, 'c HW = 75')
    _mbstd_check(4, 6, 7, 7, 4, 2, 'c HW = 147, F = 2')
    _mbstd_check(3, 4, 4, 4, 1, 1, 'group size 1')
    _mbstd_check(4, 8, 9, 9, 2, 2, 'F = 2, c HW = 324')
    kk = _kk()
    x = torch.zeros(6, 4, 4, 4, device=DEV)
    raises_without_launch(lambda: kk.minibatch_std(x, 4, 1), 'mbstd_', 'not a multiple of the group size')


# ------------------------------------------------------------------------------------------------
# bias_act, bias_act_backward
# ------------------------------------------------------------------------------------------------

def _bias_act_check(n, c, h, w, kernel, forbid, what, x_off=0):
    kk = _kk()
    x, sc, bi = ints(101, n, c, h, w), ints(102, n * c, lo=-2, hi=2), ints(103, c)
    nz, res = ints(104, n, 1, h, w), ints(105, n, c, h, w)
    z = x.double() * sc.double().view(n, c, 1, 1) + nz.double() * 0.5 + bi.double().view(1, c, 1, 1)
    ref = act64(z, True, clamp=8.0, **ACT) + res.double()
    assert float((ref - res.double()).abs().max()) == 16.0 and float(z.abs().max()) > 8.0          # the clamp is reached
    xd, sd, bd, nd, rd = dev(x, x_off), sc.to(DEV), bi.to(DEV), nz.to(DEV), res.to(DEV)
    call = lambda: kk.bias_act(xd, bias=bd, scale=sd, noise=nd, noise_strength=0.5, residual=rd, act=True, clamp=8.0, **ACT)   # noqa: E731
    got, names = launched(call, expect=[kernel])
    assert any_hit(kernel, names) and not any_hit(forbid, names), (what, sorted(k for k in names if 'kernel' in k))
    same_bits(got, ref, what)


def bias_act_scalar_second_trip():
    total = SECOND_TRIP['shg_bias_act_f32'][1]
    assert total == 7 * 149797
    _bias_act_check(7, 1, 149797, 1, 'bias_act_kernel', 'bias_act_v4_kernel', 'scalar kernel, 4096 * 256 + 3 elements, HW odd')
    _bias_act_check(2, 3, 174763, 1, 'bias_act_kernel', 'bias_act_v4_kernel', 'scalar kernel, N=2 C=3, HW = 174763')


def bias_act_v4_second_trip():
    total4 = SECOND_TRIP['shg_bias_act_f32'][0]
    assert total4 == 17 * 61681
    _bias_act_check(17, 1, 61681, 4, 'bias_act_v4_kernel', 'bias_act_kernel', 'float4 kernel, 4096 * 256 + 1 float4')
    _bias_act_check(2, 3, 174763, 4, 'bias_act_v4_kernel', 'bias_act_kernel', 'float4 kernel, N=2 C=3, HW = 4 * 174763')


def bias_act_backward_second_trip():
    kk = _kk()
    n = SECOND_TRIP['shg_bias_act_backward_f32'][0]
    g = ints(106, n)
    y = _on_clamp_values(n, CLAMP * ACT['gain'])
    y[-6:] = y[:6]
    yd = y.double()
    g_, a_ = ACT['gain'], ACT['alpha']
    slope = torch.where(yd.abs() >= CLAMP * g_, torch.zeros_like(yd), torch.where(yd > 0, torch.full_like(yd, g_), torch.full_like(yd, a_ * g_)))
    gd, ydv = g.to(DEV), y.to(DEV)
    same_bits(ran(lambda: kk.bias_act_backward(gd, ydv, act=True, clamp=CLAMP, **ACT), 'bias_act_backward_kernel'), g.double() * slope, 'backward, 4096 * 256 + 3')
    same_bits(ran(lambda: kk.bias_act_backward(gd, ydv, act=False, gain=0.5), 'bias_act_backward_kernel'), g.double() * 0.5, 'backward, linear')


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
F32, F64 = torch.float32, torch.float64
CASES = {
    'fma_second_trip_f32': lambda: fma_second_trip(F32), 'fma_second_trip_f64': lambda: fma_second_trip(F64),
    'fma_six_dims_f32': lambda: fma_six_dims(F32), 'fma_six_dims_f64': lambda: fma_six_dims(F64),
    'fma_seven_dims_f32': lambda: fma_seven_dims(F32), 'fma_seven_dims_f64': lambda: fma_seven_dims(F64),
    'fma_c_none_f32': lambda: fma_c_none(F32), 'fma_c_none_f64': lambda: fma_c_none(F64),
    'fma_sliced_view_f32': lambda: fma_sliced_view(F32), 'fma_sliced_view_f64': lambda: fma_sliced_view(F64),
    'fma_zero_elements_f32': lambda: fma_zero_elements(F32), 'fma_zero_elements_f64': lambda: fma_zero_elements(F64),
    'fma_cancellation_f32': lambda: fma_cancellation(F32),
    'fma_f32_entry_second_trip': lambda: fma_f32_entry_second_trip(F32),
    'mul_reduce_workgroup_lengths': mul_reduce_workgroup_lengths,
    'mul_reduce_workgroup_second_trip': mul_reduce_workgroup_second_trip,
    'mul_reduce_thread_mapping': mul_reduce_thread_mapping,
    'mul_reduce_interleaved': mul_reduce_interleaved,
    'mul_reduce_permuted_fallback': mul_reduce_permuted_fallback,
    'mul_reduce_b_none': mul_reduce_b_none,
    'mul_reduce_float64': mul_reduce_float64,
    'mul_reduce_empty_to_zeros': mul_reduce_empty_to_zeros,
    'sum_partials_tails': sum_partials_tails,
    'modtail_hw_4': modtail_hw_4,
    'modtail_two_blocks': modtail_two_blocks,
    'modtail_two_slices': modtail_two_slices,
    'modtail_last_slice_empty': modtail_last_slice_empty,
    'modtail_full_table': modtail_full_table,
    'modtail_optional_operands': modtail_optional_operands,
    'modtail_arithmetic': modtail_arithmetic,
    'modtail_refusals': modtail_refusals,
    'scale_cast_to_half': scale_cast_to_half,
    'scale_cast_to_float': scale_cast_to_float,
    'scale_channels_edges': scale_channels_edges,
    'planes_to_image_edges': planes_to_image_edges,
    'composite_u8_edges': composite_u8_edges,
    'assemble_input_edges': assemble_input_edges,
    'mbstd_second_trip': mbstd_second_trip,
    'mbstd_small_and_groups': mbstd_small_and_groups,
    'bias_act_scalar_second_trip': bias_act_scalar_second_trip,
    'bias_act_v4_second_trip': bias_act_v4_second_trip,
    'bias_act_backward_second_trip': bias_act_backward_second_trip,
}


@gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_edge(case):
    CASES[case]()


# ------------------------------------------------------------------------------------------------
# host-only: the second-trip sizes against the caps in the source
# ------------------------------------------------------------------------------------------------

def caps_in_source():
    """entry point -> the grid caps of its launch sites, in source order: ``if (grid > A * B) grid = ...``, ``if (blocks > A) ...`` and the
    ``n_out < A ? n_out : A`` of the workgroup mapping of mul_reduce."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sh-gan_amd', 'csrc', 'pointwise.hip')
    with open(path) as f:
        src = f.read()
    parts = re.split(r'extern "C" int (\w+)\(', src)
    caps = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        found = []
        for m in re.finditer(r'if \((grid|blocks) > ([0-9 *]+)\) \1 = ([0-9 *]+);|n_out < (\d+) \? n_out : (\d+)', body):
            a, b = (m.group(2), m.group(3)) if m.group(1) else (m.group(4), m.group(5))
            va, vb = (int(np.prod([int(t) for t in e.split('*')])) for e in (a, b))
            assert va == vb, (name, m.group(0))
            found.append(va)
        if found:
            caps[name] = found
    return caps


def test_second_trip_cases_exceed_the_caps():
    caps = caps_in_source()
    assert set(caps) == set(SECOND_TRIP), f'capped launch sites of pointwise.hip: {sorted(caps)}; cases: {sorted(SECOND_TRIP)}'
    for name, sizes in SECOND_TRIP.items():
        assert len(sizes) == len(caps[name]), (name, caps[name])
        for size, cap in zip(sizes, caps[name]):
            assert size > cap * LANES.get(name, 256), f'{name}: a case of {size} units is one trip of a grid capped at {cap} workgroups'
    assert caps['shg_fma_f32'] == [4096] and caps['shg_fma_bcast'] == [8192] and caps['shg_mul_reduce'] == [65536]      # the scan reads numbers
