"""Bits of the fused layer tail of the float32 forward convolution kernels (run with -m gpu on an MI355X).

Every kernel route is run twice on the same random finite input.  Run 1 has the identity tail (no bias, noise or out_scale, no activation,
gain 1) and yields the raw convolution bits r.  Run 2 has the full tail: bias, activation on and off, gain 1 and sqrt(2), clamp off, 256 and
0.5 (small enough to bite).  Its expected value is computed on the host in numpy.float32 FROM r -- r + b, then x < 0 ? x * alpha : x,
then * gain, then the clip: lrelu_agc as common/utils.py:135-143 defines it, plain float32 arithmetic and not the code under test -- and the
int32 views must be EQUAL.  Without out_scale and noise the tail holds no contracted multiply-add (v * 1 + 0 is exact), so equality is the
right condition whatever the compiler fuses.  The contract is for finite values (a NaN goes through a clamp and through v_med3_f32
differently); no NaN is fed.

The routes and their shapes sit on the dispatch boundaries of tests/test_gpu_routes_fp32.py (F(4x4) tile shapes from W = 32 / 128 / 256,
F(2x2) at 16 rows, the direct kernel below, the polyphase form from 128 input channels and 32 output pixels per side); every case checks
with the launch probe that the kernel it names did run.  N = 2, I = 16 (128 for the polyphase form), O = 64 and 72: 72 has a padded last
channel tile with masked stores.

Modulated cases (in_scale, out_scale, per-sample noise), on the routes that take those operands:
  * `fma`: noise_strength 0.25 (the noise term is then exact), no bias, no activation: the tail is the ONE fused multiply-add r * osc +
    nzterm, correctly rounded, compared with its float64 evaluation at <= 1 ulp (half an ulp is what a fused multiply-add may differ by; a
    separate multiply and add would exceed one under cancellation);
  * `full`: the same plus bias, lrelu, gain sqrt(2), clamp 256, against float64 within a bound worked out per element from the roundings
    the chain has: the product (half an ulp of r * osc, if it is not fused), the sum t = r * osc + nzterm and the sum x = t + b (half an ulp
    each, scaled by the slope and the gain that follow), then the two multiplies (half an ulp of the result each, and half an ulp of slack
    for the spacing being taken at the float64 value): |got - ref| <= slope * gain * (ulp(r osc) + ulp(t) + ulp(x)) / 2 + 1.5 ulp(ref).
    The `fma` bound is asserted on the routes whose source fuses the operation (shg_conv_tail); the direct kernel's figure is printed."""
import numpy as np
import pytest
import torch

from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALPHA = 0.2
SQRT2 = 2 ** 0.5
GAINS = (1.0, SQRT2)
CLAMPS = (None, 256.0, 0.5)          # None: clamping off (the C entry points take -1)
OS = (64, 72)
WINO, WINO4, MFMA, POLY_DOWN = 'conv_wino_kernel', 'conv_wino4_kernel', 'conv_mfma_kernel', 'conv_poly_down_kernel'


def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def rnd(seed, *shape, lo=None):
    rs = np.random.RandomState(seed)
    a = rs.rand(*shape) + lo if lo is not None else rs.standard_normal(shape)
    return torch.from_numpy(a.astype(np.float32))


def expected_f32(r, b, act, gain, clamp):
    """lrelu_agc of common/utils.py:135-143 on r + b, every step rounded to float32; without activation the layer does x * gain."""
    x = (r + b.reshape(1, -1, 1, 1)).astype(np.float32)
    g = np.float32(gain)
    if not act:
        return (x * g).astype(np.float32)
    y = np.where(x < 0, (x * np.float32(ALPHA)).astype(np.float32), x)
    y = (y * g).astype(np.float32)
    if clamp is not None:
        y = np.clip(y, np.float32(-clamp), np.float32(clamp))
    return y.astype(np.float32)


def tail_cases():
    for gain in GAINS:
        yield False, gain, None
        for clamp in CLAMPS:
            yield True, gain, clamp


# route id -> (builder of run(**tail) on N = 2 and `o` output channels, kernels that must run, kernels that must not)
def _conv2d_route(h, w, i=16, k=3, mode='same', nb=2):
    def build(o):
        kk = _kk()
        x, wt = rnd(1, nb, i, h, w).to(DEV), rnd(2, o, i, k, k)
        pw = kk.conv_weight_prep(wt.to(DEV), gain=1.0 / np.sqrt(i * k * k))
        kw = dict(mode=kk.MODE_SAME, pad=k // 2) if mode == 'same' else dict(mode=kk.MODE_DOWN2, pad=1)
        return lambda **tail: kk.conv2d(x, pw, **kw, **tail)
    return build


def _down_poly_route(o):
    kk = _kk()
    from oracle import shgan_oracle as orc
    x, wt = rnd(1, 2, 128, 64, 64).to(DEV), rnd(2, o, 128, 3, 3)
    f = orc.setup_filter([1, 3, 3, 1]).to(DEV)
    pw = kk.conv_weight_prep(wt.to(DEV), gain=1.0 / np.sqrt(128 * 9))
    assert kk.down_poly_supported(x, pw)                        # (not forced: the smallest shape the layer itself sends this way)
    return lambda **tail: kk.fir_conv_down2(x, f, pw, **tail)


ROUTES = {
    'wino4_4x8': (_conv2d_route(32, 32), [f'{WINO4}<4, 8>'], [MFMA, WINO]),
    'wino4_2x16': (_conv2d_route(32, 128), [f'{WINO4}<2, 16>'], [MFMA, WINO]),
    'wino4_1x32': (_conv2d_route(32, 256), [f'{WINO4}<1, 32>'], [MFMA, WINO]),
    'wino_f2x2': (_conv2d_route(16, 16), [WINO], [MFMA, WINO4]),
    'mfma_stride1': (_conv2d_route(8, 8), [MFMA], [WINO, WINO4]),
    'mfma_stride2': (_conv2d_route(16, 16, mode='down'), [MFMA], [WINO, WINO4]),
    'c1x1_gemm': (_conv2d_route(64, 64, k=1, nb=16), ['conv1x1_gemm_kernel'], [MFMA]),      # (16 images: one tile per CU, below that it is not chosen)
    'down_poly': (_down_poly_route, [f'{POLY_DOWN}<2', f'{POLY_DOWN}<3'], [MFMA]),
}
MODULATED = ['wino4_4x8', 'wino4_2x16', 'wino4_1x32', 'wino_f2x2', 'mfma_stride1', 'mfma_stride2']
FUSED = ['wino4_4x8', 'wino4_2x16', 'wino4_1x32', 'wino_f2x2']      # shg_conv_tail: the multiply-add is fused in the source, not by the compiler's choice


def _bits(t):
    a = t.detach().cpu().numpy()
    assert a.dtype == np.float32 and np.isfinite(a).all()
    return a


def _raw(route, o):
    """(run, r): the route's launcher and its identity-tail output; the probe confirms the kernels by name."""
    build, expect, forbid = ROUTES[route]
    if route == 'c1x1_gemm' and o % 64:
        expect, forbid = [MFMA], ['conv1x1_gemm_kernel']         # 72 channels are no whole GEMM tile: the tap-list kernel serves them
    run = build(o)
    r, names = launched(lambda: run(act=False, gain=1.0), expect=expect)
    kern = sorted(n for n in names if 'kernel' in n)
    for p in expect:
        assert any_hit(p, names), f'{route}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not any_hit(p, names), f'{route}: {p} must not run; ran {kern}'
    return run, _bits(r)


@pytest.mark.parametrize('o', OS)
@pytest.mark.parametrize('route', sorted(ROUTES))
def test_tail_bits(route, o):
    run, r = _raw(route, o)
    assert np.array_equal(_bits(run(act=False, gain=1.0)).view(np.int32), r.view(np.int32)), f'{route}: the identity run does not repeat'
    b = rnd(3, o)
    bd = b.to(DEV)
    for act, gain, clamp in tail_cases():
        # total gain = act_gain * gain and total clamp = clamp * gain (kernels._act_args): gain goes in as act_gain so that both stay as listed
        tail = dict(act=True, alpha=ALPHA, act_gain=gain, gain=1.0, clamp=clamp) if act else dict(act=False, gain=gain)
        got = _bits(run(bias=bd, **tail))
        want = expected_f32(r, b.numpy(), act, gain, clamp)
        diff = got.view(np.int32) != want.view(np.int32)
        print(f'TAILBITS {route} O={o} act={int(act)} gain={gain:.4f} clamp={clamp} differing={int(diff.sum())} of {diff.size}')
        if clamp == 0.5:
            assert (np.abs(want) == np.float32(0.5)).any(), 'clamp 0.5 is meant to bite'
        assert not diff.any(), (f'{route} O={o} act={act} gain={gain} clamp={clamp}: {int(diff.sum())} of {diff.size} values differ, first at '
                                f'{np.argwhere(diff)[0].tolist()}: got {got[diff][0]!r}, want {want[diff][0]!r}')


def _ulp32(v):
    """Spacing of float32 at |v| (v float64)."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('route', MODULATED)
def test_tail_modulated(route):
    o, ns = 72, 0.25
    run, _ = _raw(route, o)
    y0 = run(act=False, gain=1.0)
    n, _, oh, ow = y0.shape
    i = 16
    s, osc, nz, b = rnd(4, n, i, lo=0.5), rnd(5, n, o, lo=0.5), rnd(6, n, 1, oh, ow), rnd(7, o)
    sd, od, nd, bd = s.to(DEV), osc.to(DEV), nz.to(DEV), b.to(DEV)
    r = _bits(run(in_scale=sd, act=False, gain=1.0)).astype(np.float64)           # raw bits of the modulated convolution
    prod = r * osc.numpy().astype(np.float64).reshape(n, o, 1, 1)
    t = prod + nz.numpy().astype(np.float64) * ns
    # fma: one correctly rounded operation
    got = _bits(run(in_scale=sd, out_scale=od, noise=nd, noise_strength=ns, act=False, gain=1.0)).astype(np.float64)
    err = np.abs(got - t) / _ulp32(t)
    print(f'TAILMOD {route} fma: max {err.max():.3f} ulp')
    if route in FUSED:
        assert err.max() <= 1.0, f'{route}: fused tail {err.max():.3f} ulp from float64'
    # full: bias, lrelu, gain sqrt(2), clamp 256
    g = float(np.float32(SQRT2))
    x = t + b.numpy().astype(np.float64).reshape(1, o, 1, 1)
    slope = np.where(x < 0, float(np.float32(ALPHA)), 1.0)
    ref = np.clip(x * slope * g, -256.0, 256.0)
    got = _bits(run(in_scale=sd, out_scale=od, noise=nd, noise_strength=ns, bias=bd, act=True, alpha=ALPHA, act_gain=SQRT2, gain=1.0,
                    clamp=256.0)).astype(np.float64)
    e_x = (_ulp32(prod) + _ulp32(t) + _ulp32(x)) / 2
    # (a sum that lands within its own rounding error of zero may take the other slope on the device: |x| (1 - alpha) gain <= gain e_x)
    bound = np.where(np.abs(x) <= e_x, 1.0, slope) * g * e_x + 1.5 * _ulp32(ref)
    ratio = np.abs(got - ref) / bound
    print(f'TAILMOD {route} full: max {ratio.max():.3f} of the bound')
    assert ratio.max() <= 1.0, f'{route}: full modulated tail {ratio.max():.3f} x its rounding bound from float64'
