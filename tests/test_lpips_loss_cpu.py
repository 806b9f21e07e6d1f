"""CPU (no GPU): the algebra csrc/lpips_bwd.hip implements, against float64 autograd (tests/lpips_grad_f64.py), and the argument
validation of ``Lpips.loss``, ``kernels.l1_mean`` and ``InpaintingLoss(perceptual=...)`` as far as it runs before a device is touched."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import lpips_grad_f64 as y64
import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, kernels, losses, lpips
from shgan_amd._lib import ShgError

F64 = torch.float64


def _taps(seed, B=2, C=8, h=5, w=7, dead=True):
    g = torch.Generator().manual_seed(seed)
    f = F.relu(torch.randn(B, C, h, w, generator=g, dtype=F64))
    fr = F.relu(torch.randn(B, C, h, w, generator=g, dtype=F64))
    if dead:
        f[0, :, 1, 2] = 0                     # an all-zero pred vector: s = 0
        fr[1, :, 0, 0] = 0                    # and an all-zero real vector
    return f, fr, torch.rand(C, generator=g, dtype=F64) * 2 / C, torch.tensor([0.75, -1.5][:B], dtype=F64)


def test_head_closed_form_equals_float64_autograd():
    f, fr, w, g = _taps(0)
    want = y64.head_grad_autograd(f, fr, w, g)
    got = y64.head_grad_closed_form(f, fr, w, g)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(got[0, :, 1, 2].abs().max()) == 0.0 and float(want[0, :, 1, 2].abs().max()) == 0.0     # the all-zero position: exact zeros


def test_head_yardstick_normaliser_is_the_forward_heads():
    """clamp_min(1e-300) changes no value: the yardstick's head equals tests/lpips_f64.py's wherever that one is finite (everywhere)."""
    import lpips_f64
    f, fr, w, _ = _taps(1)
    assert torch.equal(y64.head(f, fr, w), lpips_f64.head_f64(f, fr, w))


@pytest.mark.parametrize('k,p,i,o', [(3, 1, 5, 7), (5, 2, 4, 3), (3, 1, 16, 3)])
def test_dgrad_is_the_forward_convolution_with_transposed_flipped_weights(k, p, i, o):
    g = torch.Generator().manual_seed(k * 10 + i)
    w = torch.randn(o, i, k, k, generator=g, dtype=F64)
    gy = torch.randn(2, o, 6, 9, generator=g, dtype=F64)
    want = y64.conv_input_grad_autograd(gy, w, (2, i, 6, 9), 1, p)
    got = F.conv2d(gy, w.transpose(0, 1).flip(2, 3), padding=p)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize('k,H,W', [(2, 6, 8), (2, 7, 5), (2, 9, 9), (3, 7, 7), (3, 8, 10), (3, 15, 6), (3, 3, 3)])
def test_gather_pool_rule_equals_max_pool2d_backward(k, H, W):
    g = torch.Generator().manual_seed(H * 100 + W + k)
    x = F.relu(torch.randn(2, 3, H, W, generator=g, dtype=F64))                # zeros tie; positive maxima are distinct
    x[0, 0, :2, :2] = 0                                                        # a window of zeros: the tie goes to the first, then the select
    gy = torch.randn(2, 3, (H - k) // 2 + 1, (W - k) // 2 + 1, generator=g, dtype=F64)
    want = y64.pool_grad_autograd(x, gy, k)
    got = y64.pool_grad_gather(x, gy, k)
    assert torch.equal(got, want) or float((got - want).abs().max()) <= 1e-15 * float(want.abs().max())
    if H % 2 == 1 and k == 2:
        assert float(got[:, :, -1].abs().max()) == 0.0                         # the dropped last row


def test_gather_pool_rule_gives_a_tied_maximum_to_the_first():
    x = torch.tensor([[[[1.0, 1.0], [1.0, 0.5]]]], dtype=F64)
    gy = torch.tensor([[[[2.0]]]], dtype=F64)
    want = y64.pool_grad_autograd(x, gy, 2)
    assert torch.equal(y64.pool_grad_gather(x, gy, 2), want) and float(want[0, 0, 0, 0]) == 2.0


def test_alex_conv1_input_gradient_leaves_unreached_pixels_zero():
    """33 x 46: (W + 4 - 11) % 4 = 3, one more than the padding: the last column lies in no window and autograd's gradient is 0 there (the
    rows' remainder of 2 is all padding)."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(4, 3, 11, 11, generator=g, dtype=F64)
    H, W = 33, 46
    OH, OW = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    dx = y64.conv_input_grad_autograd(torch.randn(1, 4, OH, OW, generator=g, dtype=F64), w, (1, 3, H, W), 4, 2)
    reached_h, reached_w = 4 * (OH - 1) - 2 + 11, 4 * (OW - 1) - 2 + 11
    assert reached_h == H and reached_w == W - 1
    assert float(dx[:, :, :, reached_w:].abs().max()) == 0.0
    assert float(dx[:, :, :, :reached_w].abs().min()) > 0.0


@pytest.mark.parametrize('net,B,H,W', y64.CASES)
def test_yardstick_cases_meet_their_conditions(net, B, H, W):
    """The cases of tests/test_gpu_lpips_loss.py: conditions (a) and (b) hold on the float64 run (asserted inside), the gradient is finite,
    and the sample whose upstream gradient is 0 has an exactly zero image gradient."""
    sd = y64.state_dict(net, y64.WEIGHT_SEED)
    fake, real = y64.images(net, B, H, W, y64.IMAGE_SEED)
    value, grad = y64.loss_and_grad(net, sd, fake, real, y64.upstream(B), conditions=True)
    assert torch.isfinite(value).all() and torch.isfinite(grad).all() and float(value.min()) > 0
    assert float(grad[0].abs().max()) > 0 and (B == 1 or float(grad[1].abs().max()) == 0.0)


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.get_lib()
    for name in ('shg_lpips_dgrad_f32', 'shg_lpips_maxpool_bwd_f32', 'shg_lpips_head_bwd_f32', 'shg_lpips_conv1_pm1_f32', 'shg_lpips_scale_pm1_f32',
                 'shg_lpips_conv1_dgrad_f32', 'shg_l1_mean_f32', 'shg_l1_mean_bwd_f32'):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.get_lib()
    p = 16                                                                     # a non-null, aligned address that is never dereferenced
    assert lib.shg_lpips_dgrad_f32(p, p, None, p, 1, 8, 8, 4, 4, 4, 2, None) != 0          # even kernel
    assert lib.shg_lpips_dgrad_f32(p, p, None, p, 1, 8, 8, 4, 4, 3, 0, None) != 0          # not 'same' padding
    assert lib.shg_lpips_dgrad_f32(None, p, None, p, 1, 8, 8, 4, 4, 3, 1, None) != 0
    assert lib.shg_lpips_maxpool_bwd_f32(p, p, p, 1, 1, 8, 8, 4, None) != 0
    assert lib.shg_lpips_maxpool_bwd_f32(p, p, p, 1, 1, 2, 8, 3, None) != 0
    assert lib.shg_lpips_head_bwd_f32(p, p, p, p, p, 1, 0, 4, 4, 0, None) != 0
    assert lib.shg_lpips_conv1_dgrad_f32(p, p, p, 1, 6, 31, None) != 0
    assert lib.shg_l1_mean_f32(p, p, p, 0, 5, None) != 0
    assert lib.shg_l1_mean_bwd_f32(p, p, p, p, 1, 0, None) != 0


class _Net:
    mapping = None


def _lpips_stub(net='vgg'):
    """An ``Lpips`` without a device: the checks under test run before any kernel."""
    return lpips.Lpips(None, [], [], lpips.SHIFT, lpips.SCALE, 'cpu', net=net)


def test_inpainting_loss_validates_the_perceptual_arguments():
    kw = dict(composite_fake=True, noise_mode='const')
    with pytest.raises(ShgError, match='perceptual_weight'):
        losses.InpaintingLoss('cpu', _Net(), None, perceptual_weight=0.5, **kw)
    with pytest.raises(ShgError, match='must be an lpips.Lpips'):
        losses.InpaintingLoss('cpu', _Net(), None, perceptual=object(), perceptual_weight=0.5, **kw)
    with pytest.raises(ShgError, match='must be an lpips.Lpips'):
        losses.InpaintingLoss('cpu', _Net(), None, perceptual=lambda a, b: a, **kw)
    net = _lpips_stub()
    L = losses.InpaintingLoss('cpu', _Net(), None, perceptual=net, perceptual_weight=0.5, l1_weight=2, **kw)
    assert L.perceptual is net and L.perceptual_weight == 0.5 and L.l1_weight == 2.0
    L = losses.InpaintingLoss('cpu', _Net(), None, **kw)
    assert L.perceptual is None and L.perceptual_weight == 0.0 and L.l1_weight == 0.0 and L.stats == {}
    assert set(L.state_dict()) == {'pl_mean'}
    with pytest.raises(TypeError):
        losses.InpaintingLoss('cpu', _Net(), None, True, 'const', net)          # keyword-only


@pytest.mark.parametrize('net', ['vgg', 'alex'])
def test_lpips_loss_validates_its_operands(net):
    n = _lpips_stub(net)
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ShgError, match='one shape'):
        n.loss(x, x[:1])
    with pytest.raises(ShgError, match='one shape'):
        n.loss(x[:, :2], x[:, :2])
    with pytest.raises(ShgError, match='no CPU path'):
        n.loss(x, x)
    with pytest.raises(ShgError, match='one shape'):
        n.loss(x, None)
    assert n.loss_calls == 0


def test_l1_mean_validates_its_operands():
    with pytest.raises(ShgError, match='one shape'):
        kernels.l1_mean(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ShgError, match='one shape'):
        kernels.l1_mean(torch.zeros(4), torch.zeros(4))
    with pytest.raises(ShgError, match='HIP'):
        kernels.l1_mean(torch.zeros(2, 3), torch.zeros(2, 3))
