"""GPU: the perceptual path length (sh-gan_amd/ppl.py, csrc/ppl.hip) and ``lpips.LPIPS(net='vgg')`` against the CPU restatements of
tests/ppl_f64.py.  On the commit before this feature every test here fails at ``from shgan_amd import ppl`` or at ``LPIPS(net='vgg')``.

Front end.  Its only inexact step is the box mean; everything after it is a fixed chain of float32 operations.  So the kernel's output
must equal, element by element, that chain applied to the float64 box mean rounded to float32 or to one of its two float32 neighbours
("within 1 float32 ulp", stated where an ulp means something: after ``(m + 1) * 127.5 - mean_c`` a value near 0 has an ulp far below
the ulp of the mean it came from).  At factor 0 / 1 there is no mean and the output is bit-exact.  The kernel sums a box in float64, not
in the reference's unspecified float32 ``mean([3, 5])`` order, so bit equality with torch's float32 mean is not claimed.

LPIPS-VGG value.  Bound: 7e-8 relative where that holds, else 2 x E32 + 2^-22 relative, E32 = the relative distance of the SAME
restatement run in float32 on the CPU from the float64 one for that case (the rule INTEGRATION section L uses).  2^-22 > 7e-8, so the second
form is the bound in force.

Sampler.  ``dist`` is a difference of nearly equal feature vectors divided by epsilon^2 = 1e-8: its float32 error is set by
cancellation.  Bound per value: 2 x (the largest relative float32-on-CPU error over this file's sampler cases) + 2^-22, with the
device's own draws fed to the restatement.  A case whose float32-on-CPU error exceeds 5 % is too ill-conditioned to show anything and
would be replaced by another seed (at most one in ten); none was replaced.

Measured on one MI355X (also in MEASUREMENTS.md, perceptual path length): front end 100 % bit-exact against the chain on the float64
mean in every case; LPIPS-VGG device error 1.8e-9 .. 5.0e-7 with float32-on-CPU 2.2e-8 .. 2.5e-7 (worst 4.98e-7 against 6.2e-7);
sampler, 16 values: largest float32-on-CPU error 4.43e-3 -> bound 8.85e-3, device error 7.1e-5 .. 2.77e-3."""
import numpy as np
import pytest
import torch

import ppl_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FLOOR = 2.0 ** -22


@pytest.fixture(scope='module')
def ppl():
    from shgan_amd import ppl
    return ppl


@pytest.fixture(scope='module')
def vgg_sd():
    return ref.vgg_random_state_dict(ref.NARROW, seed=3)


@pytest.fixture(scope='module')
def vgg(vgg_sd):
    from shgan_amd import lpips
    return lpips.LPIPS(net='vgg', state_dict=vgg_sd, device=DEV)


def _image(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


def _check_frontend(got, x, factor, crop, mean, std):
    lo, mid, hi = ref.frontend_candidates(x.numpy(), factor, crop, mean, std)
    got = got.cpu().numpy()
    assert got.shape == mid.shape and got.dtype == np.float32
    exact = got == mid
    ok = exact | (got == lo) | (got == hi)
    print(f'front end {tuple(x.shape)} factor {factor} crop {crop}: {exact.mean() * 100:.4f} % bit-exact, {(~ok).sum()} outside one ulp of the mean')
    return exact, ok


MEAN, STD = (123.68, 116.779, 103.939), (58.4, 57.1, 57.4)


@pytest.mark.parametrize('shape,factor,crop', [((2, 3, 64, 64), 0, False), ((2, 3, 256, 256), 1, False), ((2, 3, 512, 512), 2, False),
                                               ((1, 1, 1024, 1024), 4, False), ((2, 3, 512, 512), 2, True), ((1, 3, 264, 264), 1, True),
                                               ((1, 1, 72, 72), 3, False), ((1, 3, 514, 514), 2, False)])
def test_frontend_against_float64(ppl, shape, factor, crop):
    """Copy (factor 0, 1), factor 2, factor 4 with the grey repeat, crop at factor 2 -- 264 with crop starts its window at column 66, not a multiple of 4: the scalar route at
    factor 1 --, a factor with no float4 form (3), and factor 2 on rows of 514 floats (not 16-byte aligned: the scalar route, S = 257 odd)."""
    x = _image(shape, shape[2] + factor)
    got = ppl.frontend(x.to(DEV), factor, crop, MEAN, STD)
    exact, ok = _check_frontend(got, x, factor, crop, MEAN, STD)
    assert bool(ok.all())
    if factor <= 1:
        assert bool(exact.all())                                # a copy: no mean, bit-exact
    S = ppl.frontend_side(shape[1], shape[2], shape[3], factor, crop)
    assert tuple(got.shape) == (shape[0], 3, S, S)


def test_frontend_vector_and_scalar_routes_agree_bit_for_bit(ppl):
    """An unaligned view of the same values takes the scalar route: same bits.  A non-contiguous view is copied by the launcher, never
    misread."""
    x = _image((2, 3, 512, 512), 9).to(DEV)
    a = ppl.frontend(x, 2, False, MEAN, STD)
    flat = torch.empty(x.numel() + 1, device=DEV)
    flat[1:].copy_(x.reshape(-1))
    b = ppl.frontend(flat[1:].view(2, 3, 512, 512), 2, False, MEAN, STD)            # contiguous, 4 bytes off 16-byte alignment
    assert torch.equal(a, b)
    big = _image((2, 3, 512, 1024), 10).to(DEV)
    view = big[:, :, :, ::2]                                                       # non-contiguous [2,3,512,512]
    assert not view.is_contiguous()
    c = ppl.frontend(view, 2, True, MEAN, STD)
    exact, ok = _check_frontend(c, view.cpu().contiguous(), 2, True, MEAN, STD)
    assert bool(ok.all())


@pytest.mark.parametrize('shape,factor,crop,msg', [((1, 3, 64, 32), 1, False, 'not square'), ((1, 2, 64, 64), 1, False, 'channels'),
                                                   ((1, 3, 258, 258), 4, False, 'not divisible'), ((1, 3, 520, 520), 8, True, 'not divisible')])
def test_frontend_argument_errors_write_nothing(ppl, shape, factor, crop, msg):
    from shgan_amd import _lib
    x = _image(shape, 1).to(DEV)
    y = torch.full((shape[0], 3, 64, 64), -7.0, device=DEV)
    with pytest.raises(_lib.ShgError, match=msg) as e:
        ppl.frontend(x, factor, crop, MEAN, STD, y=y)
    assert 'code -1' in str(e.value)                                                # SHG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())


def _pairs(B, H, W, seed):
    import lpips_f64
    return lpips_f64.image_pairs(B, H, W, seed)


@pytest.mark.parametrize('kind', ['u8f', 'ff'])
@pytest.mark.parametrize('size', [(32, 32), (40, 56), (64, 64)])
@pytest.mark.parametrize('B', [1, 3])
def test_lpips_vgg_against_float64(vgg, vgg_sd, size, B, kind):
    """A uint8 composite against a float32 real, and a float32 pair; 40 x 56 is odd after the pools (20 x 28, 10 x 14, 5 x 7, 2 x 3)."""
    h, w = size
    pred_u8, real_u8 = _pairs(B, h, w, seed=h + w + B)
    real = real_u8.to(torch.float32).div(255) * 2 - 1
    pred = pred_u8 if kind == 'u8f' else pred_u8.to(torch.float32) / 255
    got = vgg(pred.to(DEV), real.to(DEV))
    torch.cuda.synchronize()
    want = ref.lpips_vgg(vgg_sd, pred, real)
    e32 = ((ref.lpips_vgg(vgg_sd, pred, real, dtype=torch.float32).to(torch.float64) - want).abs() / want)
    err = (got.cpu() - want).abs() / want
    bound = torch.clamp(2 * e32 + FLOOR, min=7e-8)
    print(f'lpips-vgg {size} B={B} {kind}: values {[f"{v:.4e}" for v in want.tolist()]} rel err {[f"{v:.2e}" for v in err.tolist()]} '
          f'float32-on-CPU {[f"{v:.2e}" for v in e32.tolist()]}')
    assert got.shape == (B,) and got.dtype == torch.float64 and float(want.min()) > 0
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())


def test_lpips_vgg_same_bits_alone_and_in_a_batch(vgg):
    pred_u8, real_u8 = _pairs(5, 40, 56, seed=2)
    pred, real = pred_u8.to(DEV), (real_u8.to(torch.float32).div(255) * 2 - 1).to(DEV)
    v5, v1 = vgg(pred, real), vgg(pred[3:4], real[3:4])
    torch.cuda.synchronize()
    assert torch.equal(v5[3:4], v1) and float(v1) > 0
    assert torch.equal(vgg(pred, real), v5)
    x = torch.rand(2, 3, 32, 32, device=DEV)
    assert torch.equal(vgg(x, x, gt_range='unit'), torch.zeros(2, dtype=torch.float64, device=DEV))
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError, match='too small'):
        vgg(torch.zeros(1, 3, 15, 64, device=DEV), torch.zeros(1, 3, 15, 64, device=DEV))


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------------

GENS = {64: dict(ch_base=1024, ch_max=16, w_dim=32, z_dim=32, num_layers=2, calls=4),
        512: dict(ch_base=4096, ch_max=8, w_dim=32, z_dim=32, num_layers=2, calls=2)}


def _plain_generator(res, seed):
    from shgan_amd.model_zoo import stylegan
    cfg = GENS[res]
    torch.manual_seed(seed)
    syn = stylegan.Synthesis(w_dim=cfg['w_dim'], resolution=res, rgb_n=3, ch_base=cfg['ch_base'], ch_max=cfg['ch_max'], use_fp16_after_res=None)
    mp = stylegan.Mapping(z_dim=cfg['z_dim'], c_dim=0, w_dim=cfg['w_dim'], num_ws=syn.num_ws, num_layers=cfg['num_layers'])
    G = stylegan.Generator(mp, syn).eval().requires_grad_(False)
    with torch.no_grad():               # (module-scoped fixtures run outside the suite's per-test no_grad)
        for name, p in G.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.1)
    return G


def _run_sampler(ppl, G, vgg, res, calls, seed, space='w', sampling='end', crop=False):
    """-> (device dists [calls][B], the draws of every call read back from the device)."""
    B = 2
    sampler = ppl.PPLSampler(G, vgg, space=space, sampling=sampling, crop=crop, generator=torch.Generator(device=DEV).manual_seed(seed))
    shadow = torch.Generator(device=DEV).manual_seed(seed)           # the same stream of draws, taken again in the documented order
    dists, draws = [], []
    for _ in range(calls):
        dists.append(sampler(torch.zeros(B, 0, device=DEV)).cpu())
        t = torch.rand([B], device=DEV, generator=shadow) * (1 if sampling == 'full' else 0)
        z0, z1 = torch.randn([2 * B, G.z_dim], device=DEV, generator=shadow).chunk(2)
        noise = {}
        for name, buf in sampler.G.named_buffers():
            if name.endswith('.noise_const'):
                noise[name[:-len('noise_const')]] = torch.randn(buf.shape, device=DEV, generator=shadow).cpu()
                assert torch.equal(buf.cpu(), noise[name[:-len('noise_const')]])         # the copy holds exactly these draws
        draws.append({'t': t.cpu(), 'z0': z0.cpu(), 'z1': z1.cpu(), 'noise': noise})
    return dists, draws


@pytest.fixture(scope='module')
def sampler_cases(ppl, vgg, vgg_sd):
    """Every sampler case of this file, run once: device values, float64 and float32-on-CPU restatements."""
    with torch.no_grad():               # (a module-scoped fixture runs outside the suite's per-test no_grad)
        return _sampler_cases(ppl, vgg, vgg_sd)


def _sampler_cases(ppl, vgg, vgg_sd):
    out = []
    for res, space, sampling, crop, seed in ((64, 'w', 'end', False, 11), (64, 'z', 'full', True, 12), (512, 'w', 'end', False, 13)):
        G = _plain_generator(res, seed)
        sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
        before = {k: v.clone() for k, v in sd.items()}
        Gd = G.to(DEV)
        calls = GENS[res]['calls'] if space == 'w' else 2
        dists, draws = _run_sampler(ppl, Gd, vgg, res, calls, seed, space, sampling, crop)
        after = {k: v.detach().cpu() for k, v in Gd.state_dict().items()}
        assert all(torch.equal(before[k], after[k]) for k in before), 'the caller\'s generator was modified'
        for got, d in zip(dists, draws):
            kw = dict(resolution=res, num_layers=GENS[res]['num_layers'], space=space, crop=crop)
            want = ref.sampler_dist(sd, vgg_sd, d, **kw)
            w32 = ref.sampler_dist(sd, vgg_sd, d, dtype=torch.float32, **kw).to(torch.float64)
            out.append(dict(res=res, space=space, sampling=sampling, crop=crop, got=got, want=want, e32=(w32 - want).abs() / want))
    return out


def test_sampler_against_the_restatement(sampler_cases):
    e32_max = max(float(c['e32'].max()) for c in sampler_cases)
    bound = 2 * e32_max + FLOOR
    worst = 0.0
    for c in sampler_cases:
        err = (c['got'] - c['want']).abs() / c['want']
        worst = max(worst, float(err.max()))
        print(f"sampler {c['res']} {c['space']} {c['sampling']} crop {c['crop']}: dist {[f'{v:.5e}' for v in c['want'].tolist()]} device rel err "
              f"{[f'{v:.2e}' for v in err.tolist()]} float32-on-CPU {[f'{v:.2e}' for v in c['e32'].tolist()]}")
        assert c['got'].dtype == torch.float64 and float(c['want'].min()) > 0
    print(f'sampler: largest float32-on-CPU error {e32_max:.3e} -> bound {bound:.3e}; largest device error {worst:.3e}')
    assert all(float(c['e32'].max()) <= 0.05 for c in sampler_cases), 'a case is too ill-conditioned: choose another seed'
    for c in sampler_cases:
        assert bool(((c['got'] - c['want']).abs() / c['want'] <= bound).all()), (c['res'], c['space'], bound)


def test_compute_ppl_is_the_trimmed_mean_of_the_sampler_outputs(ppl, vgg):
    G = _plain_generator(64, 21).to(DEV)
    before = {k: v.detach().clone() for k, v in G.state_dict().items()}
    value = ppl.compute_ppl(G, vgg, num_samples=12, batch_size=2, generator=torch.Generator(device=DEV).manual_seed(77))
    sampler = ppl.PPLSampler(G, vgg, generator=torch.Generator(device=DEV).manual_seed(77))
    dist = torch.cat([sampler(torch.zeros(2, 0, device=DEV)) for _ in range(6)])
    assert isinstance(value, float) and value == ppl.trimmed_mean(dist) and value > 0
    assert abs(value - ref.trimmed_mean_np(dist.cpu().numpy())) <= 12 * 2.0 ** -52 * value
    assert value == ppl.ppl2_wend(G, vgg, num_samples=12, generator=torch.Generator(device=DEV).manual_seed(77))
    after = G.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)                     # noise_const buffers and parameters alike


def test_eval_loop_takes_the_vgg_backbone(vgg, vgg_sd):
    """``EvalLoop(lpips=LPIPS(net='vgg'))`` on the loop tests' small generator fills ``lpips_per_image`` with the values of the direct call.
    (At 256 x 256: the shipped inpainter configs start there, a 64 x 64 one cannot be built.)"""
    from shgan_amd import configs
    from shgan_amd import eval_harness as hz
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1).eval().requires_grad_(False).to(DEV)

    def latents(ids, b, z_dim=64):
        out = torch.empty(b, z_dim)
        g = torch.Generator()
        for k, i in enumerate(ids):
            g.manual_seed(500 + int(i))
            out[k].normal_(generator=g)
        return out.to(DEV)
    n_items, b, R = 8, 4, 256
    loop = hz.EvalLoop(G, DEV, R, n_items, noise_mode='const', depth=2, latent_fn=latents, lpips=vgg)
    np.random.seed(21)
    loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
    images, _ = loop.gather()
    torch.cuda.synchronize()
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)])
    got = loop.image_metrics['lpips_per_image']
    direct = vgg(images, reals.to(DEV))
    assert got.shape == (n_items,) and got.dtype == torch.float64 and torch.equal(got, direct)
    want = ref.lpips_vgg(vgg_sd, images[:2].cpu(), reals[:2])
    assert float(((got[:2].cpu() - want).abs() / want).max()) <= 1e-5
