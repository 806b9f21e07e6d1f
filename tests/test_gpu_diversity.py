"""GPU: the diversity of pluralistic completions -- ``diversity.pairwise_lpips`` against the existing pair API of ``lpips.Lpips`` (random
weights) and ``EvalLoop(samples_per_input=K, diversity=net)`` at the reduced 256 generator.  On the commit before this feature every test
fails at ``from shgan_amd import diversity`` or at the EvalLoop options."""
import numpy as np
import pytest
import torch

import lpips_f64
import ppl_f64

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def alex():
    from shgan_amd import lpips
    return lpips.LPIPS(net='alex', state_dict=lpips_f64.random_state_dict(11), device=DEV)


@pytest.fixture(scope='module')
def vgg():
    from shgan_amd import lpips
    return lpips.LPIPS(net='vgg', state_dict=ppl_f64.vgg_random_state_dict(ppl_f64.NARROW, seed=3), device=DEV)


def _by_pair_api(net, imgs):
    """Mean over the pairs of net(imgs[n, a], imgs[n, b]): K - 1 trunk passes per sample; float64, pairs added in table order."""
    from shgan_amd import diversity
    N, K = imgs.shape[:2]
    pairs = diversity.pair_table(K)
    out = torch.zeros(N, dtype=torch.float64, device=imgs.device)
    for n in range(N):
        vals = [net(imgs[n, a][None].contiguous(), imgs[n, b][None].contiguous(), gt_range='unit')[0] for a, b in pairs]
        acc = vals[0].clone()
        for v in vals[1:]:
            acc += v
        out[n] = acc / len(pairs)
    return out


@pytest.mark.parametrize('which', ['alex', 'vgg'])
def test_pairwise_lpips_is_the_pair_api_bit_for_bit(which, alex, vgg):
    from shgan_amd import diversity
    net = alex if which == 'alex' else vgg
    imgs = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)           # N = 2, K = 3, float32 in [0, 1]
    got = diversity.pairwise_lpips(net, imgs)
    want = _by_pair_api(net, imgs)
    print(f'pairwise lpips ({which}): {got.tolist()}')
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and float(got.min()) > 0
    assert torch.equal(got, want)
    out = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    assert diversity.pairwise_lpips(net, imgs, out=out) is out and torch.equal(out, want)
    assert torch.equal(diversity.pairwise_lpips(net, imgs[1:]), want[1:])                            # an input's value does not depend on N
    same = imgs[:, :1].expand(-1, 3, -1, -1, -1).contiguous()
    assert torch.equal(diversity.pairwise_lpips(net, same), torch.zeros(2, dtype=torch.float64, device=DEV))


def test_pairwise_lpips_does_not_depend_on_fresh_contents_and_stays_inside_its_buffers(alex):
    """('diversity.py', 'pairwise_lpips') has no entry in the site tables of tests/test_gpu_alloc_fill.py / test_gpu_alloc_guard.py (it is
    newer than they are): its fill and guard runs are here -- the same bits with every fresh allocation pre-filled with NaN bytes and with
    large values, and no guard band touched with every buffer, the images included, housed between poisoned bands."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import diversity
    host = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    want = diversity.pairwise_lpips(alex, host.to(DEV))
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got = diversity.pairwise_lpips(alex, host.to(DEV))
            torch.cuda.synchronize()
        assert ('diversity.py', 'pairwise_lpips') in rec.sites and ('lpips.py', 'head_pairs') in rec.sites
        assert torch.equal(got, want), pattern
    with alloc_guard.guarded() as rec:
        got = diversity.pairwise_lpips(alex, host.to(DEV))
        bad = rec.violations()
        assert ('diversity.py', 'pairwise_lpips') in rec.sites and not bad, bad
        assert torch.equal(got, want)


def test_pairwise_lpips_edges(alex):
    from shgan_amd import _lib, diversity
    imgs = torch.rand(2, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(DEV)
    assert torch.equal(diversity.pairwise_lpips(alex, imgs), torch.zeros(2, dtype=torch.float64, device=DEV))       # K = 1
    u8 = torch.randint(0, 256, (1, 2, 3, 64, 64), generator=torch.Generator().manual_seed(7), dtype=torch.uint8).to(DEV)
    v = diversity.pairwise_lpips(alex, u8)                                                           # uint8 composites: the 'pred' table for both
    assert tuple(v.shape) == (1,) and float(v) > 0 and bool(torch.isfinite(v).all())
    with pytest.raises(_lib.ShgError, match='too small'):
        diversity.pairwise_lpips(alex, torch.zeros(1, 2, 3, 16, 16, device=DEV))
    with pytest.raises(_lib.ShgError, match=r'\[N,K,3,R,R\]'):
        diversity.pairwise_lpips(alex, torch.zeros(2, 3, 64, 64, device=DEV))
    with pytest.raises(_lib.ShgError, match='lpips.Lpips'):
        diversity.pairwise_lpips(lambda a, b: a, imgs)


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


def _run(G, metrics=('psnr',), **kw):
    from shgan_amd import eval_harness as hz
    loop = hz.EvalLoop(G, DEV, 256, 8, noise_mode='const', depth=2, latent_fn=_latents, metrics=metrics, **kw)
    np.random.seed(21)
    loop.run(hz.PinnedU8Loader(loop.ids, 4, 256, seed=13))
    images, _ = loop.gather()
    torch.cuda.synchronize()
    return loop, images


def test_eval_loop_diversity_per_image(small_g, alex):
    """8 synthetic items in two batches, K = 3: ``diversity_per_image`` in dataset order equals pairwise_lpips on the kept samples; the
    gathered images are sample 0 and differ from the K = 1 run of the same seed by at most 1 LSB on a share of pixels below 2e-3 (the
    allowance test_generator_small_golden makes for route differences: the synthesis batch is 12 rows instead of 4)."""
    from shgan_amd import diversity
    loop, images = _run(small_g, samples_per_input=3, diversity=alex, keep_samples=True)
    im = loop.image_metrics
    assert sorted(im) == ['diversity', 'diversity_per_image', 'psnr', 'psnr_per_image']
    per = im['diversity_per_image']
    assert per.dtype == torch.float64 and tuple(per.shape) == (8,) and bool(torch.isfinite(per).all()) and float(per.min()) > 0
    assert tuple(loop.samples.shape) == (8, 3, 3, 256, 256) and loop.samples.dtype == torch.uint8
    assert torch.equal(per, diversity.pairwise_lpips(alex, loop.samples))
    assert loop.diversity_value() == im['diversity'] == float(per.mean())
    assert torch.equal(images, loop.samples[:, 0])
    for k in (1, 2):
        assert not torch.equal(loop.samples[:, k], loop.samples[:, 0])
    loop1, images1 = _run(small_g)
    d = (images.to(torch.int32) - images1.to(torch.int32)).abs()
    share = float((d > 0).float().mean())
    print(f'sample 0 vs the K = 1 run: max diff {int(d.max())} LSB on a share of {share:.2e}; diversity {im["diversity"]:.5f}')
    assert int(d.max()) <= 1 and share < 2e-3
    # diversity alone, nothing kept
    lean, _ = _run(small_g, metrics=None, keep_images=False, samples_per_input=3, diversity=alex)
    assert lean.samples is None and sorted(lean.image_metrics) == ['diversity', 'diversity_per_image']
    assert torch.equal(lean.image_metrics['diversity_per_image'], per)


def test_eval_loop_with_the_option_off_is_the_plain_loop(small_g):
    """K = 1 (the default) takes the loop's usual path: no evaluator, buffer or generator of the feature exists, and stating the default
    explicitly changes no bit.  Both runs here go through this commit's loop, so this is no comparison with the parent commit's: what pins
    the K = 1 loop to its earlier outputs are the unchanged tests of tests/test_gpu_eval_loop.py, test_gpu_lpips.py, test_gpu_kid_is.py and
    test_gpu_pr.py, which run it against float64 references and fixed expectations."""
    loop_a, images_a = _run(small_g)
    loop_b, images_b = _run(small_g, samples_per_input=1)
    assert torch.equal(images_a, images_b)
    assert torch.equal(loop_a.image_metrics['psnr_per_image'], loop_b.image_metrics['psnr_per_image'])
    for loop in (loop_a, loop_b):
        assert sorted(loop.image_metrics) == ['psnr', 'psnr_per_image'] and sorted(loop.evaluators) == ['columns']
        assert loop.samples is None and loop._extra_rng is None and loop.diversity_per_image is None
