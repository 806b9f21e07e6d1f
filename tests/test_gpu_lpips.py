"""GPU: LPIPS (sh-gan_amd/lpips.py, csrc/lpips.hip + the detector's convolution and pool kernels) against the float64 CPU model of
tests/lpips_f64.py with random weights -- the first convolution in all operand forms, the distance head on every tap shape, the whole
network per image, exact zero / symmetry / batch invariance, and ``EvalLoop(lpips=net)``.

Bounds: convolution and head, max error / max |reference| <= 1e-5 (the bound tests/test_gpu_inception.py holds the shared convolution
kernel to); whole network, |value - float64| <= 1e-5 * float64 value per image (a plain float32 torch model of this network stays within
1.6e-7 of float64 on this input family, values 8e-4 .. 1.7e-2, so the bound leaves float32 arithmetic about 60 x)."""
import numpy as np
import pytest
import torch

import lpips_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TAPS = {256: (63, 31, 15, 15, 15), 512: (127, 63, 31, 31, 31)}
CHANNELS = (64, 192, 384, 256, 256)


def _rel(a, b):
    a, b = a.detach().cpu().to(torch.float64), b.detach().cpu().to(torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope='module')
def sd():
    return ref.random_state_dict(11)


@pytest.fixture(scope='module')
def net(sd):
    from shgan_amd import lpips
    return lpips.Lpips.from_state_dict(sd, device=DEV)


def _forms(pred_u8, real_u8, kind):
    """(pred, gt, gt_range) of one operand pairing: 'u8u8' composite / decoded pixels, 'u8f' composite / float32 real in [-1, 1],
    'ff' float32 pred in [0, 1] / float32 real in [-1, 1]."""
    real = real_u8.to(torch.float32).div(255) * 2 - 1
    if kind == 'u8u8':
        return pred_u8, real_u8
    if kind == 'u8f':
        return pred_u8, real
    return pred_u8.to(torch.float32) / 255, real


@pytest.mark.parametrize('size', [256, 512, (200, 300), 64, 7])
def test_conv1_against_float64(sd, net, size):
    """Operand load + scaling layer + conv 11 x 11 stride 4 pad 2 + bias + ReLU, all four operand forms (and the two 'unit' ones)."""
    from shgan_amd import lpips
    h, w = (size, size) if isinstance(size, int) else size
    g = torch.Generator().manual_seed(h * 5 + w)
    u8 = torch.randint(0, 256, (2, 3, h, w), generator=g, dtype=torch.uint8)
    unit = torch.rand(2, 3, h, w, generator=g)
    pm1 = torch.rand(2, 3, h, w, generator=g) * 2 - 1
    oh, ow = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    for img, operand, rng in ((u8, 'pred', 'pm1'), (unit, 'pred', 'pm1'), (pm1, 'gt', 'pm1'), (u8, 'gt', 'pm1'), (unit, 'gt', 'unit'),
                              (u8, 'gt', 'unit')):
        got = lpips.conv1(img.to(DEV), *net.conv1_wb, operand, rng)
        v = ref.pred_values_f32(img) if operand == 'pred' else ref.gt_values_f32(img, rng)
        want = ref.conv1_f64(sd, v)
        assert got.shape == want.shape == (2, 64, oh, ow)
        err = _rel(got, want)
        print(f'conv1 {size} {operand} {rng} {img.dtype}: {err:.2e}')
        assert err <= 1e-5, (size, operand, rng, img.dtype, err)


def test_conv1_weight_prep_gives_the_detectors_packing():
    """shg_lpips_conv1_weight_prep_f32 on a seeded [64,3,11,11] weight against ``inception.pack_weight``: both outputs, bit for bit.
    ``shg_inception_weight_prep_f32`` refuses kernels beyond 7 x 7 (tests/test_inception_cpu.py pins that refusal), so ``pack_weight`` cannot
    be handed the 11 x 11 weight itself; it packs the same 363 columns as a 1 x 1 convolution over 363 channels laid out in the packing's
    own K order, k = (ky*11 + kx)*3 + c -- for a 1 x 1 kernel the detector's k IS the channel index, so the two [368][64] tables and the
    two [64] biases must agree element for element.  ``lpips.pack_conv1`` is that entry point and is held to the same bits."""
    import ctypes
    from shgan_amd import _lib, inception, kernels, lpips
    g = torch.Generator().manual_seed(363)
    w, b = torch.randn(64, 3, 11, 11, generator=g).to(DEV), torch.randn(64, generator=g).to(DEV)
    wp, bp = torch.full((368 * 64,), float('nan'), device=DEV), torch.full((64,), float('nan'), device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(_lib.get_lib().shg_lpips_conv1_weight_prep_f32(kernels._ptr(w), kernels._ptr(b), kernels._ptr(wp), kernels._ptr(bp), stream),
               'lpips_conv1_weight_prep')
    with pytest.raises(_lib.ShgError, match='bad shape'):
        inception.pack_weight(w, b)
    want_wp, want_bp = inception.pack_weight(w.permute(0, 2, 3, 1).reshape(64, 363, 1, 1).contiguous(), b)
    assert want_wp.shape == wp.shape and want_bp.shape == bp.shape
    assert torch.equal(wp, want_wp) and torch.equal(bp, want_bp)
    # and a table built on the host, which shares no kernel with either side: rows k = (ky*11 + kx)*3 + c, columns o, zero rows to 368
    host = torch.zeros(368, 64)
    host[:363] = w.cpu().permute(2, 3, 1, 0).reshape(363, 64)
    assert torch.equal(wp.cpu().reshape(368, 64), host) and torch.equal(bp.cpu(), b.cpu())
    assert float(wp.reshape(368, 64)[363:].abs().max()) == 0 and bool((wp.reshape(368, 64)[:363] != 0).all())
    again = lpips.pack_conv1(w, b)
    assert torch.equal(again[0], want_wp) and torch.equal(again[1], want_bp)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('res', [256, 512])
def test_head_against_float64(res, B):
    """The five tap shapes; ReLU-like features (many zeros) with a block of pixels whose features are ALL zero in both images (0, not NaN)
    and one where only the pred's are; ``out`` is added to."""
    from shgan_amd import lpips
    for k, (c, s) in enumerate(zip(CHANNELS, TAPS[res])):
        g = torch.Generator().manual_seed(res + 10 * B + k)
        fp = torch.relu(torch.randn(B, c, s, s, generator=g))
        fg = torch.relu(fp + 0.3 * torch.randn(B, c, s, s, generator=g))
        fp[:, :, 2:6, 1:5] = 0
        fg[:, :, 2:6, 1:5] = 0
        fp[:, :, 8:10, 3:9] = 0
        w = torch.rand(c, generator=g) * 2 / c
        out = torch.full((B,), 1.5, dtype=torch.float64, device=DEV)
        lpips.head(fp.to(DEV), fg.to(DEV), w.to(DEV), out)
        want = ref.head_f64(fp, fg, w)
        got = out.cpu() - 1.5
        assert bool(torch.isfinite(got).all())
        err = _rel(got, want)
        print(f'head {res} tap {k} B={B}: {err:.2e}')
        assert err <= 1e-5, (res, k, B, err)


@pytest.mark.parametrize('kind', ['u8u8', 'u8f', 'ff'])
@pytest.mark.parametrize('size,B', [(256, 3), (512, 2), ((200, 300), 2), (1024, 1)])
def test_network_against_float64_model(net, sd, size, B, kind):
    h, w = (size, size) if isinstance(size, int) else size
    pred_u8, real_u8 = ref.image_pairs(B, h, w, seed=h + B)
    pred, gt = _forms(pred_u8, real_u8, kind)
    got = net(pred.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    want = ref.lpips_f64(sd, pred, gt)
    assert got.shape == (B,) and got.dtype == torch.float64
    err = ((got.cpu() - want).abs() / want).tolist()
    print(f'lpips {size} x {B} {kind}: values {[f"{v:.4e}" for v in want.tolist()]} rel err {[f"{e:.2e}" for e in err]}')
    assert float(want.min()) > 0
    assert max(err) <= 1e-5, (size, B, kind, err)


def test_identical_float_images_give_exactly_zero_and_the_value_is_symmetric(net):
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 256, 256, generator=g).to(DEV)
    assert torch.equal(net(x, x, gt_range='unit'), torch.zeros(2, dtype=torch.float64, device=DEV))
    a, b = x, torch.rand(2, 3, 256, 256, generator=g).to(DEV)
    ab, ba = net(a, b, gt_range='unit'), net(b, a, gt_range='unit')
    assert torch.equal(ab, ba) and float(ab.min()) > 0


def test_a_pair_has_the_same_bits_alone_and_inside_a_batch(net):
    pred_u8, real_u8 = ref.image_pairs(8, 256, 256, seed=9)
    pred, real = pred_u8.to(DEV), (real_u8.to(torch.float32).div(255) * 2 - 1).to(DEV)
    v8, v1 = net(pred, real), net(pred[5:6], real[5:6])
    torch.cuda.synchronize()
    assert torch.equal(v8[5:6], v1) and float(v1) > 0
    again = net(pred, real)
    assert torch.equal(again, v8)                              # run to run


def test_python_api_refusals_on_the_device(net):
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError, match='too small'):
        net(torch.zeros(1, 3, 30, 64, dtype=torch.uint8, device=DEV), torch.zeros(1, 3, 30, 64, device=DEV))
    with pytest.raises(_lib.ShgError, match='uint8 or float32'):
        net(torch.zeros(1, 3, 64, 64, dtype=torch.float64, device=DEV), torch.zeros(1, 3, 64, 64, device=DEV))
    with pytest.raises(_lib.ShgError, match='float64'):
        net(torch.zeros(1, 3, 64, 64, device=DEV), torch.zeros(1, 3, 64, 64, device=DEV), out=torch.zeros(1, device=DEV))
    v = net(torch.zeros(1, 3, 31, 31, dtype=torch.uint8, device=DEV), torch.full((1, 3, 31, 31), 0.25, device=DEV))   # the smallest image
    assert v.shape == (1,) and bool(torch.isfinite(v).all())


@pytest.fixture(scope='module')
def small_g():
    from shgan_amd import configs
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1)
    return G.eval().requires_grad_(False).to(DEV)


def _latents(ids, b, z_dim=64):
    out = torch.empty(b, z_dim)
    g = torch.Generator()
    for k, i in enumerate(ids):
        g.manual_seed(500 + int(i))
        out[k].normal_(generator=g)
    return out.to(DEV)


def test_eval_loop_lpips_per_image(small_g, net, sd):
    """EvalLoop(..., depth=4, feature_fn=det, metrics=('psnr', 'ssim'), lpips=net) over 48 items: ``lpips_per_image`` equals the float64
    model on the kept composites and the loader's reals; images, FID moments, PSNR and SSIM are the same bits as the run without lpips."""
    import inception_f64
    from shgan_amd import eval_harness as hz
    from shgan_amd import inception
    det = inception.InceptionFeatures.from_state_dict(inception_f64.random_state_dict(7), device=DEV)
    n_items, b, R = 48, 8, 256
    runs = []
    for kw in ({'lpips': net}, {}):
        loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=4, feature_fn=det, latent_fn=_latents, metrics=('psnr', 'ssim'),
                           **kw)
        np.random.seed(21)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
        images, fid = loop.gather()
        torch.cuda.synchronize()
        runs.append((images, fid, loop.image_metrics))
    (images, fid, im), (images0, fid0, im0) = runs
    assert sorted(im) == ['lpips', 'lpips_per_image', 'psnr', 'psnr_per_image', 'ssim', 'ssim_per_image']
    assert sorted(im0) == ['psnr', 'psnr_per_image', 'ssim', 'ssim_per_image']
    assert torch.equal(images, images0) and torch.equal(fid.S, fid0.S)
    for k in im0:
        assert torch.equal(im[k], im0[k]) if torch.is_tensor(im0[k]) else im[k] == im0[k], k
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)])
    want = ref.lpips_f64(sd, images.cpu(), reals)
    got = im['lpips_per_image'].cpu()
    assert got.shape == (n_items,) and got.dtype == torch.float64
    err = float(((got - want).abs() / want).max())
    print(f'EvalLoop lpips: mean {im["lpips"]:.6f} (float64 {float(want.mean()):.6f}), worst per-image rel err {err:.2e}')
    assert err <= 1e-5
    assert abs(im['lpips'] - float(want.mean())) <= 1e-5 * float(want.mean())
    # lpips alone, without the image buffer
    lean = hz.EvalLoop(small_g, DEV, R, 16, noise_mode='const', depth=4, latent_fn=_latents, keep_images=False, lpips=net)
    np.random.seed(21)
    lean.run(hz.PinnedU8Loader(lean.ids, b, R, seed=13))
    imgs, _ = lean.gather()
    assert imgs is None and sorted(lean.image_metrics) == ['lpips', 'lpips_per_image']
    assert torch.equal(lean.image_metrics['lpips_per_image'], im['lpips_per_image'][:16])
