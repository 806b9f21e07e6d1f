"""GPU: per-image PSNR and SSIM on the device (sh-gan_amd/image_metrics.py, csrc/image_metrics.hip) against the reference's own outputs
(tests/golden/image_metrics.npz) and the float64 restatement of tests/test_image_metrics_cpu.py over a shape / window / operand-form
sweep; reproducibility; and ``EvalLoop(metrics=...)`` on a reduced-width 256^2 generator."""
import numpy as np
import pytest
import torch

from test_image_metrics_cpu import golden_cases, reference_metrics_f64

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PSNR_TOL, SSIM_TOL = 1e-5, 2e-5


def _pair(shape, seed, pred_u8=True, gt_u8=False):
    """A decoded-pixel image and a composite close to it (noise + a rectangular region of unrelated pixels), in the requested forms:
    pred uint8 or float32 in [0, 1]; gt float32 in [-1, 1] (ToTensor * 2 - 1) or uint8 decoded pixels."""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    yy = torch.arange(h, dtype=torch.float32)[:, None]
    xx = torch.arange(w, dtype=torch.float32)[None, :]
    base = 128 + 60 * torch.sin(xx / 5.0) * torch.cos(yy / 7.0)
    real_u8 = (base + torch.randint(-40, 41, shape, generator=g)).clamp(0, 255).to(torch.uint8)
    pred = real_u8.to(torch.int32) + torch.randint(-8, 9, shape, generator=g)
    pred[:, :, h // 4:h // 2 + 1, w // 4:w // 2 + 1] = torch.randint(0, 256, (b, c, h // 2 + 1 - h // 4, w // 2 + 1 - w // 4), generator=g)
    pred = pred.clamp(0, 255).to(torch.uint8)
    if not pred_u8:
        pred = (pred.to(torch.float32) / 255 + torch.rand(shape, generator=g) * 0.003).clamp(0, 1)
    gt = real_u8 if gt_u8 else real_u8.to(torch.float32).div(255) * 2 - 1
    return pred, gt


def _check(pred, gt, ws, what):
    from shgan_amd.image_metrics import image_metrics
    psnr, ssim = image_metrics(pred.to(DEV), gt.to(DEV), window_size=ws)
    p_ref, s_ref = reference_metrics_f64(pred, gt, ws)
    dp = float((psnr.cpu() - p_ref).abs().max())
    ds = float((ssim.cpu() - s_ref).abs().max())
    assert dp <= PSNR_TOL and ds <= SSIM_TOL, f'{what}: psnr err {dp:.3e}, ssim err {ds:.3e}'
    return dp, ds


def test_matches_the_reference_evaluators():
    from shgan_amd.image_metrics import image_metrics
    for name, pred_u8, real_u8, real, ws, psnr_ref, ssim_ref in golden_cases():
        for gt in (real, real_u8):
            psnr, ssim = image_metrics(pred_u8.to(DEV), gt.to(DEV), window_size=ws)
            assert np.abs(psnr.cpu().numpy() - psnr_ref).max() <= PSNR_TOL, name
            assert np.abs(ssim.cpu().numpy() - ssim_ref).max() <= SSIM_TOL, name


SWEEP = [  # (H, W, C, windows, pred_u8, gt_u8)
    (1, 1, 3, (1, 3, 11, 31), True, False),
    (1, 1, 1, (7,), False, True),
    (5, 300, 3, (1, 7, 11, 31), True, True),
    (5, 300, 1, (3, 11), False, False),
    (37, 53, 3, (1, 3, 7, 11, 31), False, True),
    (37, 53, 1, (7, 11, 31), True, False),
    (64, 64, 3, (3, 7, 11, 31), True, False),
    (64, 64, 1, (11,), True, True),
    (257, 257, 3, (7, 11), True, False),
    (257, 257, 1, (31,), False, False),
    (512, 512, 3, (11,), True, False),
    (512, 512, 3, (3,), False, True),
]


@pytest.mark.parametrize('h,w,c,windows,pred_u8,gt_u8', SWEEP)
def test_shape_window_form_sweep_against_float64(h, w, c, windows, pred_u8, gt_u8):
    pred, gt = _pair((16, c, h, w), seed=h * 1000 + w + c, pred_u8=pred_u8, gt_u8=gt_u8)
    for ws in windows:
        _check(pred, gt, ws, f'{h}x{w} C={c} ws={ws} pred_u8={pred_u8} gt_u8={gt_u8}')


def test_identical_operands_give_ssim_one_and_infinite_psnr():
    from shgan_amd.image_metrics import image_metrics
    for shape in ((3, 3, 37, 53), (2, 1, 5, 300)):
        u8 = _pair(shape, 11)[0].to(DEV)
        f = u8.float() / 255
        psnr, ssim = image_metrics(f, f, gt_range='unit')
        assert torch.isinf(psnr).all() and (psnr > 0).all()
        assert float((ssim - 1).abs().max()) <= 1e-6
        # uint8 pixels: PSNR compares pred as float64 u8/255 with gt in float32 (the reference's evaluator batch) -- finite, ~155 dB
        psnr, ssim = image_metrics(u8, u8, gt_range='unit')
        assert float((ssim - 1).abs().max()) <= 1e-6 and bool((psnr > 140).all()) and bool(torch.isfinite(psnr).all())


def test_results_are_batch_invariant_and_reproducible():
    from shgan_amd.image_metrics import image_metrics
    pred, gt = _pair((16, 3, 257, 257), 3)
    pred, gt = pred.to(DEV), gt.to(DEV)
    for ws in (11, 7):
        p1, s1 = image_metrics(pred, gt, window_size=ws)
        p2, s2 = image_metrics(pred, gt, window_size=ws)
        assert torch.equal(p1, p2) and torch.equal(s1, s2)
        for i in (0, 5, 15):
            pi, si = image_metrics(pred[i:i + 1], gt[i:i + 1], window_size=ws)
            assert torch.equal(pi, p1[i:i + 1]) and torch.equal(si, s1[i:i + 1])
        pp, _ = image_metrics(pred, gt, window_size=ws, psnr_only=True)
        assert torch.equal(pp, p1)


def test_bad_arguments_raise():
    from shgan_amd._lib import ShgError
    from shgan_amd.image_metrics import image_metrics
    pred, gt = _pair((1, 3, 16, 16), 1)
    pred, gt = pred.to(DEV), gt.to(DEV)
    for ws in (10, 0, 33):
        with pytest.raises(ShgError, match='window_size'):
            image_metrics(pred, gt, window_size=ws)
    with pytest.raises(ShgError, match='device'):
        image_metrics(pred.cpu(), gt)
    with pytest.raises(ShgError):
        image_metrics(pred, gt[:, :2])


def test_eval_loop_metrics_match_the_gathered_images_and_leave_them_unchanged():
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, eval_harness as hz
    from shgan_amd.image_metrics import image_metrics
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1).eval().requires_grad_(False).to(DEV)
    n_items, b, R = 11, 4, 256

    def latents(ids, bb):
        out = torch.empty(bb, 64)
        g = torch.Generator()
        for k, i in enumerate(ids):
            g.manual_seed(500 + int(i))
            out[k].normal_(generator=g)
        return out.to(DEV)

    def run(metrics):
        loop = hz.EvalLoop(G, DEV, R, n_items, noise_mode='const', seed=3, latent_fn=latents, metrics=metrics)
        np.random.seed(77)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=9))
        images, _ = loop.gather()
        torch.cuda.synchronize()
        return loop, images

    on, images = run(('psnr', 'ssim'))
    off, images_off = run(None)
    assert off.image_metrics is None
    assert torch.equal(images, images_off), 'the metrics must not change the uint8 images'
    real = hz.PinnedU8Loader(list(range(n_items)), n_items, R, seed=9)._draw(list(range(n_items))).to(DEV)
    psnr, ssim = image_metrics(images, real)
    im = on.image_metrics
    assert torch.equal(im['psnr_per_image'], psnr) and torch.equal(im['ssim_per_image'], ssim)
    assert im['psnr'] == float(psnr.mean()) and im['ssim'] == float(ssim.mean())
    assert np.isfinite(im['psnr']) and 0 < im['ssim'] < 1
