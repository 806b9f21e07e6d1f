"""conv_wino4: the two routes of the weight operands -- register ring and wave-private LDS ring -- must give the same bits.

Every case runs the same convolution under ``kernels.WINO4_U = 'reg'`` and ``'lds'`` (and as shipped, ``None``) and checks
  * by kernel name that the two arms really are the two routes (one runs as ``conv_wino4_kernel<TY, TX>``, the other as
    ``conv_wino4_alt_kernel<TY, TX>``); the 4 x 128 px shape has no room for the ring, both arms are its only kernel;
  * that the outputs of the arms are bit-identical: the same operand values reach the same MFMAs in the same order;
  * that the shipped route agrees with float64 torch CPU ``conv2d`` + the layer tail within 1e-4 of the output range, the
    tolerance of the F(4x4,3x3) cases of test_gpu_ops.py (test_wino4_conv_vs_torch_cpu_and_direct).
The shapes are the smallest at which the ring can go wrong: one chunk (the peeled first chunk alone), a masked channel tail,
an odd chunk count (the two-slot ring wraps inside a chunk boundary), two output tiles with masked channels, the K split with
its reduction, all tail operands present / absent, each tile shape, extents that are no multiple of the tile."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4              # test_gpu_ops.py::test_wino4_conv_vs_torch_cpu_and_direct
K, ALT, WSPLIT = 'conv_wino4_kernel', 'conv_wino4_alt_kernel', 'wino_split_reduce_kernel'

# name: (n, ci, co, h, w, tile, fused tail, WINO_SPLIT, the launch splits along K)
CASES = {
    'i8_one_chunk': (2, 8, 64, 32, 32, '<4, 8>', True, True, False),
    'i12_masked_channels': (2, 12, 64, 32, 32, '<4, 8>', True, True, False),
    'i24_odd_chunks': (2, 24, 64, 32, 32, '<4, 8>', True, True, False),
    'i40': (2, 40, 64, 32, 32, '<4, 8>', True, True, False),
    'o72_two_otiles': (2, 16, 72, 32, 32, '<4, 8>', True, True, False),
    'ksplit_on': (1, 256, 64, 32, 32, '<4, 8>', True, True, True),
    'ksplit_off': (1, 256, 64, 32, 32, '<4, 8>', True, False, False),
    'no_tail': (2, 24, 64, 32, 32, '<4, 8>', False, True, False),
    'ragged_36x40': (1, 20, 70, 36, 40, '<4, 8>', True, True, False),
    'tile_8x64': (1, 24, 72, 32, 128, '<2, 16>', True, True, False),
    'tile_8x64_ragged': (1, 12, 64, 36, 132, '<2, 16>', False, True, False),
    'tile_4x128': (1, 16, 64, 32, 256, '<1, 32>', True, True, False),
}


@pytest.fixture(scope='module')
def kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def _problem(kk, n, ci, co, h, w, tail):
    """-> (call(), float64 reference) of one stride-1 3x3 convolution, with or without every operand of the fused tail."""
    from oracle import shgan_oracle as orc
    rs = np.random.RandomState(7 * n + ci + 3 * co + h + w)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    x, wt = t(n, ci, h, w), t(co, ci, 3, 3)
    if not tail:
        ref = F.conv2d(x.double(), wt.double() * 0.1, padding=1)
        args = dict(mode=0, pad=1)
    else:
        s_in = torch.from_numpy(rs.rand(n, ci).astype(np.float32) + 0.5)
        s_out = torch.from_numpy(rs.rand(n, co).astype(np.float32) + 0.5)
        bias, noise, res = t(co), t(n, 1, h, w), t(n, co, h, w)
        ref = F.conv2d((x * s_in[:, :, None, None]).double(), wt.double() * 0.1, padding=1) * s_out[:, :, None, None].double() + noise.double() * 0.25
        ref = orc.lrelu_agc((ref + bias.view(1, -1, 1, 1).double()).float(), gain=0.5) + res
        args = dict(mode=0, pad=1, in_scale=s_in.to(DEV), out_scale=s_out.to(DEV), bias=bias.to(DEV), noise=noise.to(DEV),
                    noise_strength=0.25, act=True, gain=0.5, residual=res.to(DEV))
    pw = kk.conv_weight_prep(wt.to(DEV), gain=0.1)
    xd = x.to(DEV)
    return (lambda: kk.conv2d(xd, pw, **args)), ref


@pytest.mark.parametrize('case', sorted(CASES))
def test_wino4_weight_routes_agree(kk, case):
    n, ci, co, h, w, tile, tail, split, splits = CASES[case]
    old = kk.WINO, kk.WINO4, kk.WINO_SPLIT, kk.WINO4_U
    out, names = {}, {}
    try:
        kk.WINO, kk.WINO4, kk.WINO_SPLIT = True, True, split
        call, ref = _problem(kk, n, ci, co, h, w, tail)
        for route in ('reg', 'lds', None):
            kk.WINO4_U = route
            out[route], names[route] = launched(call, expect=[f'{K}{tile}'] if route is None else ['conv_wino4_'])
    finally:
        kk.WINO, kk.WINO4, kk.WINO_SPLIT, kk.WINO4_U = old
    ran = {r: sorted(k for k in names[r] if 'wino' in k) for r in names}
    assert any_hit(f'{K}{tile}', names[None]), f'{case}: the shipped route runs as {K}{tile}; ran {ran[None]}'
    if tile == '<1, 32>':       # no room for the ring beside the 6 x 136 windows
        assert all(any_hit(f'{K}{tile}', names[r]) and not any_hit(ALT, names[r]) for r in ('reg', 'lds')), ran
    else:
        alt = [r for r in ('reg', 'lds') if any_hit(f'{ALT}{tile}', names[r])]
        std = [r for r in ('reg', 'lds') if any_hit(f'{K}{tile}', names[r])]
        assert len(alt) == 1 and len(std) == 1 and alt != std, f'{case}: one arm per kernel name; ran {ran}'
    for r in names:
        assert any_hit(WSPLIT, names[r]) == splits, f'{case}: K split expected {splits}; ran {ran[r]}'
    e = rel_err(out[None].double().cpu().numpy(), ref.numpy())
    same = torch.equal(out['reg'], out['lds'])
    print(f'uring {case}: shipped route vs fp64 {e:.2e}; reg == lds bitwise: {same}; shipped == reg bitwise: {torch.equal(out[None], out["reg"])}')
    assert torch.isfinite(out['lds']).all()
    assert same, f'{case}: register ring and LDS ring differ (max abs {float((out["reg"] - out["lds"]).abs().max()):.3e})'
    assert torch.equal(out[None], out['reg']), f'{case}: the shipped route differs from its own arm'
    assert e < TOL, f'{case}: rel err {e:.3e} >= {TOL:.0e}'


def test_wino4_ring_on_narrow_tiles_for_wide_images(kk):
    """``WINO4_U = 'lds_8x64'``: W >= 256 on the 8 x 64 px tiles with the LDS ring (the A/B arm against the 4 x 128 px shape).  Every 4 x 4
    output block is computed from the same 6 x 6 patch by the same sums whatever tile it belongs to, so the bits are those of the
    shipped route as long as neither launch is split along K."""
    n, ci, co, h, w = 1, 16, 64, 32, 256
    old = kk.WINO, kk.WINO4, kk.WINO4_U
    try:
        kk.WINO, kk.WINO4 = True, True
        call, ref = _problem(kk, n, ci, co, h, w, True)
        kk.WINO4_U = 'lds_8x64'
        y, names = launched(call, expect=['conv_wino4_'])
        kk.WINO4_U = None
        y0 = call()
    finally:
        kk.WINO, kk.WINO4, kk.WINO4_U = old
    ran = sorted(k for k in names if 'wino' in k)
    assert any_hit('conv_wino4_kernel<2, 16>', names) or any_hit('conv_wino4_alt_kernel<2, 16>', names), ran
    assert not any_hit('conv_wino4_kernel<1, 32>', names) and not any_hit(WSPLIT, names), ran
    e = rel_err(y.double().cpu().numpy(), ref.numpy())
    print(f'uring lds_8x64: vs fp64 {e:.2e}; bitwise equal to the shipped route: {torch.equal(y, y0)}')
    assert e < TOL
    assert torch.equal(y, y0)


@pytest.mark.parametrize('ci,tile', [(63, '<1, 32>'), (64, '<2, 16>')])
def test_wino4_wide_images_take_the_ring_tiles_from_64_channels(kk, ci, tile):
    """W >= 256 as shipped: the 8 x 64 px tiles (with the ring) from 64 input channels on, the 4 x 128 px tiles below -- both sides of the
    rule, against the register-ring arm (4 x 128 px tiles on either side: same bits) and float64."""
    other = '<1, 32>' if tile == '<2, 16>' else '<2, 16>'
    old = kk.WINO, kk.WINO4, kk.WINO4_U
    try:
        kk.WINO, kk.WINO4 = True, True
        call, ref = _problem(kk, 1, ci, 64, 32, 256, True)
        kk.WINO4_U = None
        y, names = launched(call, expect=[f'{K}{tile}'])
        kk.WINO4_U = 'reg'
        y0, names0 = launched(call, expect=['conv_wino4_'])
    finally:
        kk.WINO, kk.WINO4, kk.WINO4_U = old
    ran = sorted(k for k in names | names0 if 'wino' in k)
    assert any_hit(f'{K}{tile}', names) and not any_hit(f'{K}{other}', names) and not any_hit(ALT, names), ran
    assert any_hit(f'{K}<1, 32>', names0) and not any_hit('<2, 16>', names0), ran
    assert not any_hit(WSPLIT, names | names0), ran
    e = rel_err(y.double().cpu().numpy(), ref.numpy())
    print(f'uring wide i{ci}: {tile} vs fp64 {e:.2e}; bitwise equal to the register-ring arm: {torch.equal(y, y0)}')
    assert e < TOL
    assert torch.equal(y, y0)
