"""GPU: ``Lpips.loss`` (value and d loss / d fake) and every kernel of csrc/lpips_bwd.hip on its own against float64 (tests/
lpips_grad_f64.py), ``kernels.l1_mean``, and the perceptual / L1 terms of ``InpaintingLoss``.

Error of a tensor: ``||x - x64||_inf / ||x64||_inf``.  Bar: the rule of tests/second_order_f64.py, ``max(LAYER_FACTOR * e_ref, LAYER_FLOOR)``
= ``max(3 e_ref, 5e-5)``, ``e_ref`` = the error of torch's own float32 CPU autograd of the same model (or operator) to the same float64
yardstick, measured here.  Every comparison prints its two figures before it asserts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_grad_f64 as y64
from second_order_f64 import LAYER_FLOOR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def judge(what, got, ref32, ref64):
    """Print the HIP and the torch-float32 error to the float64 yardstick, then hold the HIP one to max(3 e_ref, 5e-5)."""
    e_hip, e_ref = y64.rel_inf(got, ref64), y64.rel_inf(ref32, ref64)
    print(f'[lpips_loss] {what}: hip {e_hip:.3e}  torch-f32 {e_ref:.3e}  bar {y64.bar(e_ref):.3e}')
    assert torch.isfinite(got).all(), what
    assert e_hip <= y64.bar(e_ref), (what, e_hip, e_ref)


@functools.lru_cache(maxsize=None)
def device_net(net):
    import shgan_amd  # noqa: F401
    from shgan_amd import lpips
    return lpips.Lpips.from_state_dict(y64.state_dict(net, y64.WEIGHT_SEED), device=DEV, net=net)


@functools.lru_cache(maxsize=None)
def reference(net, B, H, W):
    """The float64 yardstick (conditions asserted) and torch's float32 CPU autograd of one case: computed once, shared, never changed."""
    sd = y64.state_dict(net, y64.WEIGHT_SEED)
    fake, real = y64.images(net, B, H, W, y64.IMAGE_SEED)
    g = y64.upstream(B)
    v64, g64 = y64.loss_and_grad(net, sd, fake, real, g, F64, conditions=True)
    v32, g32 = y64.loss_and_grad(net, sd, fake, real, g, torch.float32)
    return dict(fake=fake, real=real, g=g, v64=v64, g64=g64, v32=v32, g32=g32)


def hip_loss_and_grad(net, ref):
    n = device_net(net)
    with torch.enable_grad():
        fake = ref['fake'].to(DEV).requires_grad_(True)
        value = n.loss(fake, ref['real'].to(DEV))
        (grad,) = torch.autograd.grad((value * ref['g'].to(DEV)).sum(), fake)
    return value.detach(), grad


@pytest.mark.parametrize('net,B,H,W', y64.CASES)
def test_loss_and_image_gradient_against_float64(net, B, H, W):
    ref = reference(net, B, H, W)
    value, grad = hip_loss_and_grad(net, ref)
    assert value.dtype == torch.float32 and tuple(value.shape) == (B,) and tuple(grad.shape) == (B, 3, H, W)
    judge(f'{net} {B}x{H}x{W} loss', value, ref['v32'], ref['v64'])
    judge(f'{net} {B}x{H}x{W} d loss / d fake', grad, ref['g32'], ref['g64'])
    if B > 1:                                                  # the sample whose upstream gradient is 0
        assert float(ref['g'][1]) == 0.0 and float(grad[1].abs().max()) == 0.0 and float(grad[0].abs().max()) > 0
    if (net, W) == ('alex', 46):                               # the column no conv1 window reaches
        assert float(ref['g64'][:, :, :, 45].abs().max()) == 0.0 and float(grad[:, :, :, 45].abs().max()) == 0.0
    # the value is __call__'s distance: the same trunk and heads, the operands apart ([0, 1] steps there, straight in here)
    n = device_net(net)
    same = n((ref['fake'].to(DEV) + 1) / 2, ref['real'].to(DEV))
    assert y64.rel_inf(value, same) <= 1e-4
    # a fake that does not require grad saves nothing and gives the same bits
    assert bits_equal(n.loss(ref['fake'].to(DEV), ref['real'].to(DEV)), value)


@pytest.mark.parametrize('net,B,H,W', [('vgg', 3, 35, 37), ('alex', 3, 33, 46)])
def test_two_runs_and_a_graph_replay_give_the_same_bits(net, B, H, W):
    ref = reference(net, B, H, W)
    v0, g0 = hip_loss_and_grad(net, ref)
    v1, g1 = hip_loss_and_grad(net, ref)
    assert bits_equal(v0, v1) and bits_equal(g0, g1)
    n = device_net(net)
    real, up = ref['real'].to(DEV), ref['g'].to(DEV)
    fake = torch.zeros_like(real).requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.enable_grad(), torch.cuda.graph(graph):       # a synchronisation or an allocation outside the pool fails the capture
        value = n.loss(fake, real)
        (grad,) = torch.autograd.grad((value * up).sum(), fake)
    with torch.no_grad():
        fake.copy_(ref['fake'].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert bits_equal(value.detach(), v0) and bits_equal(grad, g0)
    graph.replay()
    torch.cuda.synchronize()
    assert bits_equal(value.detach(), v0) and bits_equal(grad, g0)


@pytest.mark.parametrize('net', ['vgg', 'alex'])
def test_second_order_raises(net):
    from shgan_amd import kernels
    ref = reference(net, 1, *(y64.CASES[0][2:] if net == 'vgg' else y64.CASES[5][2:]))
    n = device_net(net)
    with torch.enable_grad():
        fake = ref['fake'].to(DEV).requires_grad_(True)
        (grad,) = torch.autograd.grad(n.loss(fake, ref['real'].to(DEV)).sum(), fake, create_graph=True)
        with pytest.raises(RuntimeError, match='first order only'):
            torch.autograd.grad(grad.square().sum(), fake)
        a = ref['fake'].to(DEV).requires_grad_(True)
        (ga,) = torch.autograd.grad(kernels.l1_mean(a, ref['real'].to(DEV)).sum(), a, create_graph=True)
        with pytest.raises(RuntimeError, match='first order only'):
            torch.autograd.grad(ga.square().sum(), a)


# ---- every kernel on its own -----------------------------------------------------------------------------------------------------------

def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('B,C,h,w', [(2, 24, 9, 11), (3, 8, 1, 1), (1, 70, 13, 5)])
def test_head_backward(B, C, h, w, accumulate):
    """99 positions = two 64-lane tiles with a partial one; 1 x 1 (the last vgg tap at 16 x 16); all-zero pred and real vectors."""
    from shgan_amd import lpips
    f, fr = F.relu(rnd(1, B, C, h, w)), F.relu(rnd(2, B, C, h, w))
    f[0, :, 0, 0] = 0
    fr[B - 1, :, h - 1, w - 1] = 0
    wl, g = torch.rand(C, generator=torch.Generator().manual_seed(3)) * 2 / C, y64.upstream(B)
    prev = rnd(4, B, C, h, w) if accumulate else torch.zeros(B, C, h, w)
    ref64 = prev.to(F64) + y64.head_grad_autograd(f.to(F64), fr.to(F64), wl, g)
    ref32 = prev + y64.head_grad_autograd(f, fr, wl, g)
    df = prev.to(DEV).clone() if accumulate else None
    got = lpips.head_bwd(f.to(DEV), fr.to(DEV), wl.to(DEV), g.to(DEV), df=df)
    assert (got is df) == accumulate
    judge(f'head_bwd {B}x{C}x{h}x{w} accumulate={accumulate}', got, ref32, ref64)
    assert bits_equal(got[0, :, 0, 0].cpu(), prev[0, :, 0, 0])             # the all-zero position: exactly 0 added
    if B > 1 and not accumulate:
        assert float(got[1].abs().max()) == 0.0


@pytest.mark.parametrize('k,B,C,H,W', [(2, 2, 5, 8, 6), (2, 1, 3, 35, 37), (2, 2, 2, 17, 8), (3, 2, 5, 7, 7), (3, 1, 3, 15, 26), (3, 2, 2, 3, 5), (3, 1, 2, 8, 10)])
def test_maxpool_backward(k, B, C, H, W):
    """Odd sizes (a dropped last row / column at k = 2; rows outside every window at k = 3 and even sizes), more than one block, the
    minimum 3 x 3 -> 1 output, zeros (masked) tying inside a window."""
    from shgan_amd import lpips
    x = F.relu(rnd(5, B, C, H, W))
    gy = rnd(6, B, C, (H - k) // 2 + 1, (W - k) // 2 + 1)
    ref64 = y64.pool_grad_autograd(x.to(F64), gy.to(F64), k)
    assert torch.equal(ref64, y64.pool_grad_gather(x.to(F64), gy.to(F64), k)) or y64.rel_inf(y64.pool_grad_gather(x.to(F64), gy.to(F64), k), ref64) < 1e-15
    got = lpips.maxpool_bwd(x.to(DEV), gy.to(DEV), k)
    judge(f'maxpool_bwd k={k} {B}x{C}x{H}x{W}', got, y64.pool_grad_autograd(x, gy, k), ref64)
    assert bits_equal((got != 0).cpu().to(torch.int32), (ref64 != 0).to(torch.int32))
    if k == 2 and H % 2:
        assert float(got[:, :, -1].abs().max()) == 0.0


@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('k,B,I,O,H,W', [(3, 2, 24, 16, 13, 9), (3, 1, 32, 70, 8, 8), (5, 2, 16, 5, 7, 9), (5, 1, 20, 64, 6, 5), (3, 3, 8, 3, 5, 5)])
def test_masked_dgrad(k, B, I, O, H, W, masked):
    """3 x 3 and 5 x 5; forward outputs I a multiple of 16 (a K step inside one tap) and not; forward inputs O = 3 (the image), 70 (two
    channel tiles, the second partial) and 64; 234 pixels = four pixel tiles with a partial one."""
    from shgan_amd import lpips
    w = rnd(7, I, O, k, k) * (2.0 / (O * k * k)) ** 0.5           # the FORWARD weight [out = I][in = O]
    g = rnd(8, B, I, H, W)
    y_prev = F.relu(rnd(9, B, O, H, W))
    sel = (lambda t: torch.where(y_prev > 0, t, torch.zeros_like(t))) if masked else (lambda t: t)
    ref64 = sel(y64.conv_input_grad_autograd(g.to(F64), w.to(F64), (B, O, H, W), 1, k // 2).to(F64))
    ref32 = sel(y64.conv_input_grad_autograd(g, w, (B, O, H, W), 1, k // 2))
    wp = lpips.pack_dgrad_weight(w.to(DEV))
    got = lpips.dgrad(g.to(DEV), wp, O, k, y_prev.to(DEV) if masked else None)
    judge(f'dgrad {k}x{k} {B}x{I}->{O}x{H}x{W} masked={masked}', got, ref32, ref64)
    if masked:
        assert float(got.cpu()[y_prev <= 0].abs().max()) == 0.0
    # the packed operand round-trips through the forward packing
    from shgan_amd import inception
    fw = inception.pack_weight(w.to(DEV), torch.zeros(I, device=DEV))[0]
    assert bits_equal(lpips.unpack_weight(fw, I, O, k, k).cpu(), w)


@pytest.mark.parametrize('B,H,W', [(1, 31, 31), (2, 33, 46), (1, 67, 35)])
def test_alex_conv1_forward_and_dgrad(B, H, W):
    from shgan_amd import lpips
    import lpips_f64
    n = device_net('alex')
    sd = y64.state_dict('alex', y64.WEIGHT_SEED)
    w = sd['net.slice1.0.weight']
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(10)) * 2 - 1
    ref64 = lpips_f64.conv1_f64(sd, x)
    sd32 = {k: v for k, v in sd.items()}
    ref32 = F.relu(F.conv2d(y64.scaling(x, torch.float32), w, sd32['net.slice1.0.bias'], stride=4, padding=2))
    judge(f'conv1_pm1 {B}x{H}x{W}', lpips.conv1_pm1(x.to(DEV), *n.conv1_wb, n.shift, n.scale), ref32, ref64)
    OH, OW = ref64.shape[2:]
    g = rnd(11, B, 64, OH, OW)
    inv = (1 / torch.tensor(lpips_f64.SCALE, dtype=torch.float32).to(F64)).reshape(1, 3, 1, 1)
    ref64 = y64.conv_input_grad_autograd(g.to(F64), w.to(F64), (B, 3, H, W), 4, 2) * inv
    ref32 = y64.conv_input_grad_autograd(g, w, (B, 3, H, W), 4, 2) * inv.to(torch.float32)
    n._dgrad_weights()
    got = lpips.conv1_dgrad(g.to(DEV), n._conv1_wt, H, W)
    judge(f'conv1_dgrad {B}x{H}x{W}', got, ref32, ref64)
    assert bits_equal((got != 0).cpu().to(torch.int32), (ref64 != 0).to(torch.int32))         # unreached pixels: 0


@pytest.mark.parametrize('B,shape', [(1, (1,)), (3, (3, 7, 5)), (2, (3, 37, 41)), (2, (5000,))])
def test_l1_mean_both_ways(B, shape):
    """One element, fewer elements than threads, more than the 1024 threads of a workgroup; a == b at some elements (sign gives 0)."""
    from shgan_amd import kernels
    a, b = rnd(12, B, *shape), rnd(13, B, *shape)
    b.reshape(B, -1)[:, ::3] = a.reshape(B, -1)[:, ::3]
    g = y64.upstream(B)
    with torch.enable_grad():
        ad = a.to(DEV).requires_grad_(True)
        bd = b.to(DEV).requires_grad_(True)
        out = kernels.l1_mean(ad, bd)
        ga, gb = torch.autograd.grad((out * g.to(DEV)).sum(), (ad, bd))

    def ref(dtype):
        with torch.enable_grad():
            x = a.to(dtype).requires_grad_(True)
            v = (x - b.to(dtype)).abs().reshape(B, -1).mean(dim=1)
            (gx,) = torch.autograd.grad((v * g.to(dtype)).sum(), x)
        return v.detach(), gx
    (v64, g64), (v32, g32) = ref(F64), ref(torch.float32)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B,)
    judge(f'l1_mean {B}x{shape}', out.detach(), v32, v64)
    judge(f'l1_mean_bwd {B}x{shape}', ga, g32, g64)
    assert bits_equal(gb, -ga)
    assert float(ga.reshape(B, -1)[:, ::3].abs().max()) == 0.0                               # a == b: sign gives 0
    if B > 1:
        assert float(ga[1].abs().max()) == 0.0


def test_l1_mean_with_strided_operands():
    """Both operands as channel slices of a 4-channel batch (the form ``InpaintingLoss`` passes ``real_img[:, 1:4]`` in), B = 3: the value
    and both gradients equal, bit for bit, those of the contiguous copies."""
    from shgan_amd import kernels
    B = 3
    a4, b4 = rnd(14, B, 4, 9, 7).to(DEV), rnd(15, B, 4, 9, 7).to(DEV)
    g = y64.upstream(B).to(DEV) + 0.5

    def run(a, b):
        with torch.enable_grad():
            a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
            out = kernels.l1_mean(a, b)
            return (out.detach(),) + torch.autograd.grad((out * g).sum(), (a, b))
    want = run(a4[:, 1:4].contiguous(), b4[:, 1:4].contiguous())
    for a, b in ((a4[:, 1:4], b4[:, 1:4]), (a4[:, 1:4].contiguous(), b4[:, 1:4]), (a4[:, 1:4], b4[:, 1:4].contiguous())):
        assert not (a.is_contiguous() and b.is_contiguous())
        got = run(a, b)
        assert all(bits_equal(x, y) for x, y in zip(got, want))
    ref = torch.sign(a4[:, 1:4] - b4[:, 1:4]) * (g / (3 * 9 * 7)).reshape(B, 1, 1, 1)
    assert y64.rel_inf(want[1], ref.to(F64)) <= 2.0 ** -22 and float(want[1][2].abs().max()) > 0


@pytest.mark.parametrize('net,small', [('vgg', 15), ('alex', 30)])
def test_too_small_images_and_a_second_backward_raise(net, small):
    from shgan_amd._lib import ShgError
    n = device_net(net)
    x = torch.zeros(1, 3, small, 64, device=DEV)
    with pytest.raises(ShgError, match='too small'):
        n.loss(x, x)
    with pytest.raises(ShgError, match='too small'):
        n.loss(x.transpose(2, 3), x.transpose(2, 3))
    with pytest.raises(ShgError, match='float32'):
        n.loss(torch.zeros(1, 3, 64, 64, device=DEV, dtype=torch.float64), torch.zeros(1, 3, 64, 64, device=DEV, dtype=torch.float64))
    ref = reference(net, *(y64.CASES[0][1:] if net == 'vgg' else y64.CASES[5][1:]))
    with torch.enable_grad():
        fake = ref['fake'].to(DEV).requires_grad_(True)
        value = n.loss(fake, ref['real'].to(DEV)).sum()
        torch.autograd.grad(value, fake, retain_graph=True)
        with pytest.raises(ShgError, match='freed by its first backward'):
            torch.autograd.grad(value, fake)


# ---- InpaintingLoss ----------------------------------------------------------------------------------------------------------------------

TODAY = {'Gmain': {'Loss/scores/fake', 'Loss/G/loss'}, 'Greg': {'Loss/pl_penalty', 'Loss/G/reg'},
         'Dmain': {'Loss/scores/fake', 'Loss/scores/real', 'Loss/signs/real', 'Loss/D/loss'}, 'Dreg': {'Loss/scores/real', 'Loss/r1_penalty', 'Loss/D/reg'}}
PW, LW = 0.7, 1.3


@pytest.fixture(scope='module')
def stage():
    from test_gpu_optim import real_batch, small_networks
    G, D = small_networks(5)
    real4 = real_batch(2, 6)
    z = torch.from_numpy(np.random.RandomState(3).standard_normal((2, 64)).astype(np.float32)).to(DEV)
    return G, D, real4, z, torch.zeros(2, 0, device=DEV)


def make_loss(stage, **kw):
    from shgan_amd import losses
    G, D = stage[:2]
    return losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0, **kw)


def run_phase(stage, L, phase, gain=1.0):
    """One phase call -> ([gradient of every parameter of the phase's module], the stats keys the call wrote)."""
    G, D, real4, z, cnd = stage
    mod = G if phase.startswith('G') else D
    G.zero_grad(set_to_none=True), D.zero_grad(set_to_none=True)
    L.stats.clear()
    mod.requires_grad_(True)
    try:
        L.accumulate_gradients(phase, real4, cnd, z, cnd, sync=True, gain=gain)
    finally:
        mod.requires_grad_(False)
    return [None if p.grad is None else p.grad.detach().clone() for p in mod.parameters()], set(L.stats)


def test_inpainting_loss_with_weights_zero_is_todays_loss(stage):
    net = device_net('vgg')
    calls = net.loss_calls
    want, keys = run_phase(stage, make_loss(stage), 'Gmain')
    for L in (make_loss(stage, perceptual=net), make_loss(stage, perceptual=net, perceptual_weight=0.0, l1_weight=0.0), make_loss(stage, l1_weight=0)):
        got, got_keys = run_phase(stage, L, 'Gmain')
        assert got_keys == keys == TODAY['Gmain']
        assert len(got) == len(want) and all((a is None and b is None) or bits_equal(a, b) for a, b in zip(got, want))
    assert net.loss_calls == calls and any(g is not None and float(g.abs().max()) > 0 for g in want)


@pytest.mark.parametrize('net', ['vgg', 'alex'])
def test_inpainting_loss_terms_add_up(stage, net):
    """Gmain with both terms against three separately taken backward passes (adversarial, perceptual, L1).

    1. The image gradient of the ``InpaintingLoss`` call itself (a hook on ``run_G``'s output) against the sum of the three image
       gradients taken separately: autograd adds the three float32 addends with two additions, each rounding once (relative 2^-24), so
       elementwise |joint - sum| <= 2 * 2^-24 * (|g_adv| + |g_lp| + |g_l1|), the bound from the number of addends (asserted with 2.5
       units: the sum is formed in float64 here and the first addition's result is bounded by the sum of the magnitudes, which leaves a
       second-order term).
    2. The parameter gradients the call leaves are BIT-EQUAL to one backward of the objective written out here with the same association.
    3. The parameter gradients against the sum of the three passes': the joint pass and the three separate ones are four float32 passes
       of one linear map (the generator's adjoint) applied to the joint image gradient and to its three addends; each pass is within
       LAYER_FLOOR of exact relative to its own result's max-norm (the bar the suite holds every layer's backward to), so per parameter
       tensor |joint - sum| <= LAYER_FLOOR (|joint| + |adv| + |lp| + |l1|) in max-norms.
    The statistics equal the directly computed values."""
    from shgan_amd import kernels
    G, D, real4, z, cnd = stage
    n = device_net(net)
    gain = 0.5
    L = make_loss(stage, perceptual=n, perceptual_weight=PW, l1_weight=LW)
    calls = n.loss_calls
    hooked, run_G = [], L.run_G

    def run_G_hooked(*args, **kw):
        img, ws = run_G(*args, **kw)
        img.register_hook(lambda g: hooked.append(g.detach().clone()))
        return img, ws
    L.run_G = run_G_hooked
    try:
        joint, keys = run_phase(stage, L, 'Gmain', gain)
    finally:
        del L.run_G
    assert keys == TODAY['Gmain'] | {'Loss/G/perceptual', 'Loss/G/l1'} and n.loss_calls == calls + 1 and len(hooked) == 1
    stat_lp, stat_l1 = L.stats['Loss/G/perceptual'].clone(), L.stats['Loss/G/l1'].clone()
    real = real4[:, 1:4].contiguous()
    terms = {'adv': lambda img: F.softplus(-L.run_D(img, cnd)).mean(), 'lp': lambda img: n.loss(img, real).mean() * PW,
             'l1': lambda img: kernels.l1_mean(img, real).mean() * LW}

    def passes(which):
        """One generator forward, the objective of ``which`` terms, one backward -> (parameter gradients, d objective / d img, img)."""
        G.zero_grad(set_to_none=True)
        G.requires_grad_(True)
        L._m05 = real4[:, 0:1].detach()
        L._x = torch.cat([L._m05, real4[:, 1:4].detach() * (L._m05 + 0.5)], dim=1)
        try:
            with torch.enable_grad():
                img, _ = L.run_G(z, cnd)
                img.retain_grad()
                vals = [terms[k](img) for k in which]
                total = vals[0] if len(vals) == 1 else vals[0] + (vals[1] + vals[2])         # the loss's own association
                total.mul(gain).backward()
        finally:
            G.requires_grad_(False)
            L._m05 = L._x = None
        return [None if p.grad is None else p.grad.detach().clone() for p in G.parameters()], img.grad.detach().clone(), img.detach()
    written, g_written, img = passes(('adv', 'lp', 'l1'))
    assert bits_equal(stat_lp, n.loss(img, real)) and bits_equal(stat_l1, kernels.l1_mean(img, real))    # the directly computed values
    direct = (img.to(F64) - real.to(F64)).abs().mean(dim=(1, 2, 3))
    assert y64.rel_inf(stat_l1, direct) <= 2.0 ** -23                              # float64 inside, rounded once
    parts = [passes((k,)) for k in ('adv', 'lp', 'l1')]
    addends = [p[1].to(F64) for p in parts]
    assert all(float(a.abs().max()) > 0 for a in addends)
    slack = 2.5 * 2.0 ** -24 * (addends[0].abs() + addends[1].abs() + addends[2].abs())                 # 1: three addends, two roundings
    diff = (hooked[0].to(F64) - (addends[0] + addends[1] + addends[2])).abs()
    print(f'[lpips_loss] InpaintingLoss {net}: image gradient |joint - sum| / bound, worst element = {float((diff / slack.clamp_min(1e-300)).max()):.3f}')
    assert bool((diff <= slack).all())
    assert bits_equal(hooked[0], g_written)                                                             # 2
    assert len(written) == len(joint) and all((a is None and b is None) or bits_equal(a, b) for a, b in zip(joint, written))
    worst = 0.0
    for j, a, p, q in zip(joint, parts[0][0], parts[1][0], parts[2][0]):                                # 3
        if j is None:
            assert a is None and p is None and q is None
            continue
        three = [t if t is not None else torch.zeros_like(j) for t in (a, p, q)]
        bound = LAYER_FLOOR * float(j.abs().max() + sum(t.abs().max() for t in three))
        err = float((j.to(F64) - (three[0].to(F64) + three[1].to(F64) + three[2].to(F64))).abs().max())
        worst = max(worst, err / max(bound, 1e-300))
    print(f'[lpips_loss] InpaintingLoss {net}: parameter gradients |joint - sum| / bound, worst tensor = {worst:.3e}')
    assert worst <= 1.0
    assert any(p is not None and float(p.abs().max()) > 0 for p in parts[1][0]) and any(q is not None and float(q.abs().max()) > 0 for q in parts[2][0])


def test_other_phases_never_see_the_terms(stage):
    n = device_net('vgg')
    L = make_loss(stage, perceptual=n, perceptual_weight=PW, l1_weight=LW)
    calls = n.loss_calls
    for phase in ('Dmain', 'Dreg', 'Greg'):
        grads, keys = run_phase(stage, L, phase)
        assert keys == TODAY[phase], (phase, keys)
        assert n.loss_calls == calls and any(g is not None for g in grads)
    assert set(L.state_dict()) == {'pl_mean'}
