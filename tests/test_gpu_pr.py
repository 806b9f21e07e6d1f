"""GPU: the improved precision / recall metric on the device -- the fp16-MFMA manifold kernels of csrc/pr.hip, the VGG16 detector of
sh-gan_amd/vgg16.py (front end and 2 x 2 pool of csrc/vgg16.hip) and EvalLoop's ``pr`` option -- against the float64 yardsticks of
tests/pr_f64.py.

Tolerances.  Exact case: rows from {0, 1, 2}, D = 64 -- every squared distance is an integer <= 256, exact in fp32 under any summation
order; for integers up to 16 384 the square root rounded through float32 and through float64 gives the same half, and for integers
<= 256 no square root lies closer than 7e-6 relative to an fp16 rounding midpoint: radii and flags equal the restatement BIT FOR BIT.
General case: radii within 1e-3 relative of the float64 radii (one fp16 ulp: half an ulp is the rounding itself, fp32 accumulation is
orders of magnitude below); flags bracketed by the float64 test with every radius shrunk / grown by 2e-3, the probes between the brackets
at most 5 % of the case, precision / recall within open / m of the restatement's.  One listed case cannot meet that cap whatever the
kernel does: at (257, 64, 4096) the float64 restatement itself leaves 8 of 64 and 39 of 257 probes between the brackets (12.5 % and
15.2 %, measured on the CPU without the product: distances of 4096 independent coordinates concentrate, so many probes sit within 2e-3
of a radius).  The cap is a property of the data and the yardstick, not of the code under test; for that case alone the share is printed
instead of capped, and the precision / recall it would have bounded are held to min(open / m, 5 %) -- what the cap grants at most.
Detector: 1e-5 of each image's largest feature, the
bound INTEGRATION section I holds the LPIPS stack to."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pr_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# (n manifold, m probes): just past / at the edges of the 128-row tiles; 64 x 5 below one tile; 128 x 128 whole tiles; 385 x 257: three
# slices, a ragged tile on both sides
EXACT_CASES = [(200, 150), (129, 65), (64, 5), (128, 128), (385, 257)]
# the issue's three, then D = 72 (a full chunk of 64 and a ragged one) and 2100 rows (17 tiles: two tiles per slice, the last slice short)
GENERAL_CASES = [(300, 337, 64), (700, 737, 128), (257, 64, 4096), (150, 90, 72), (2100, 300, 128)]
OPEN_CAP = 0.05
CAP_UNREACHABLE = {(257, 64, 4096)}         # see the module docstring
BOUND = 1e-5


@functools.lru_cache(maxsize=None)
def _ints(n, seed):
    return np.random.RandomState(seed).randint(0, 3, (n, 64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _general(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.relu(torch.randn(n, D, generator=g)) * 3).to(torch.float16)


@functools.lru_cache(maxsize=None)
def _exact_ref(n, m, k):
    man, probes = _ints(n, 10 + n), _ints(m, 20 + m)
    r = ref.radii16(man, k)
    d = ref.dist16(probes, man)
    return r, (d <= r[None]).any(axis=1), (d < r[None]).any(axis=1), int((d == r[None]).any(axis=1).sum())


@pytest.mark.parametrize('k', [1, 3, 15])
@pytest.mark.parametrize('n,m', EXACT_CASES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_exact_case_radii_and_flags_bit_for_bit(n, m, k, dtype):
    from shgan_amd import precision_recall as prm
    man, probes = torch.from_numpy(_ints(n, 10 + n)).to(dtype).to(DEV), torch.from_numpy(_ints(m, 20 + m)).to(dtype).to(DEV)
    want_r, want_in, strict_in, ties = _exact_ref(n, m, k)
    r = prm.radii(man, k)
    assert r.dtype == torch.float16 and r.shape == (n,)
    got_r = r.cpu().numpy()
    assert np.array_equal(got_r.view(np.uint16), want_r.view(np.uint16))
    flags = prm.inside(probes, man, r)
    assert flags.dtype == torch.bool and flags.shape == (m,)
    print(f'exact n={n} m={m} k={k}: {ties} probes sit exactly on a radius, {int(want_in.sum())} inside')
    assert np.array_equal(flags.cpu().numpy(), want_in)
    if (n, m, k) == (200, 150, 3):
        assert ties > 10 and not np.array_equal(want_in, strict_in)          # this case tells `<=` from `<`


@functools.lru_cache(maxsize=None)
def _general_ref(n, m, D, k):
    """Both directions of one case: (manifold, probes) -> float64 radii, the two brackets and the restatement's flags."""
    a, b = _general(n, D, 1).numpy(), _general(m, D, 2).numpy()
    out = {}
    for name, man, probes in (('fwd', a, b), ('rev', b, a)):
        must, may = ref.inside_brackets(probes, man, k, 2e-3)
        out[name] = (ref.radii_f64(man, k), must, may, ref.inside16(probes, man, ref.radii16(man, k)))
    return out


@pytest.mark.parametrize('direction', ['fwd', 'rev'])
@pytest.mark.parametrize('n,m,D', GENERAL_CASES)
def test_general_case_against_float64(n, m, D, direction):
    from shgan_amd import precision_recall as prm
    k = 3
    a, b = _general(n, D, 1), _general(m, D, 2)
    man, probes = (a, b) if direction == 'fwd' else (b, a)
    want_r, must, may, want_in = _general_ref(n, m, D, k)[direction]
    r = prm.radii(man.to(DEV), k)
    got_r = r.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got_r - want_r) / want_r))
    flags = prm.inside(probes.to(DEV), man.to(DEV), r).cpu().numpy()
    open_ = int((may & ~must).sum())
    share = open_ / len(probes)
    got, want = float(flags.mean()), float(want_in.mean())
    print(f'general n={len(man)} m={len(probes)} D={D}: radii rel err {err:.2e}; open {open_} / {len(probes)}; inside {got:.4f} vs {want:.4f}')
    assert err <= 1e-3
    if (n, m, D) not in CAP_UNREACHABLE:
        assert share <= OPEN_CAP
    assert np.all(flags[must]) and np.all(may[flags])
    assert abs(got - want) <= min(share, OPEN_CAP)


def test_pr_from_features_equals_the_restatement_on_the_exact_case():
    from shgan_amd import precision_recall as prm
    real, fake = _ints(200, 210), _ints(150, 170)
    got = prm.pr_from_features(torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV), nhood_size=3)
    assert got == ref.pr16(real, fake, 3) and 0 < got[0] < 1


def test_a_set_against_itself_gives_one_also_with_duplicated_rows():
    from shgan_amd import precision_recall as prm
    x = _general(300, 128, 5)
    dup = torch.cat([x, x[:40], x[:7], x[:7], x[:7], x[:7]])           # rows with 2 and with 6 copies (more than nhood_size + 1)
    for feats in (x, dup):
        f = feats.to(DEV)
        assert prm.pr_from_features(f, f.clone(), nhood_size=3) == (1.0, 1.0)
    assert bool(prm.inside(dup.to(DEV), dup.to(DEV), prm.radii(dup.to(DEV), 1)).all())


def test_calls_repeat_bit_for_bit_and_flags_do_not_depend_on_later_probes():
    from shgan_amd import precision_recall as prm
    man, probes = _general(700, 128, 1).to(DEV), _general(737, 128, 2).to(DEV)
    r1, r2 = prm.radii(man, 3), prm.radii(man, 3)
    assert torch.equal(r1, r2)
    f1, f2 = prm.inside(probes, man, r1), prm.inside(probes, man, r1)
    assert torch.equal(f1, f2)
    for m0 in (100, 128, 300):
        assert torch.equal(prm.inside(probes[:m0], man, r1), f1[:m0]), m0


def test_rejected_arguments_raise():
    from shgan_amd import _lib, precision_recall as prm
    x = _general(64, 64, 9).to(DEV)
    r = prm.radii(x, 3)
    for bad in (0, 16, -1):
        with pytest.raises(_lib.ShgError, match='nhood_size'):
            prm.radii(x, bad)
    with pytest.raises(_lib.ShgError, match='rows'):
        prm.radii(x[:3], 3)
    with pytest.raises(_lib.ShgError, match='multiple of 8'):
        prm.radii(x[:, :60], 3)
    with pytest.raises(_lib.ShgError, match='multiple of 8'):
        prm.radii(torch.zeros(16, 68, device=DEV), 3)
    with pytest.raises(_lib.ShgError, match='multiple of 8'):
        prm.radii(torch.zeros(16, 32, device=DEV), 3)
    with pytest.raises(_lib.ShgError, match='float32 or float16'):
        prm.radii(x.double(), 3)
    with pytest.raises(_lib.ShgError, match='HIP'):
        prm.radii(x.cpu(), 3)
    with pytest.raises(_lib.ShgError, match='share D'):
        prm.inside(torch.zeros(8, 128, device=DEV), x, r)
    with pytest.raises(_lib.ShgError, match='radii must be'):
        prm.inside(x, x, r[:10])
    with pytest.raises(_lib.ShgError, match='radii'):
        prm.inside(x, x, r.float())
    with pytest.raises(ValueError, match='rows'):
        prm.pr_from_features(x, x[:3], nhood_size=3)
    assert bool(prm.inside(x, x, r).all())                              # the library is still usable after the rejections


# ---- the detector

@pytest.fixture(scope='module')
def sd():
    return ref.random_state_dict(3)


@pytest.fixture(scope='module')
def det(sd):
    from shgan_amd import vgg16
    return vgg16.Vgg16Features.from_state_dict(sd, device=DEV)


def _images(B, H, W, seed, pm1=False):
    g = torch.Generator().manual_seed(seed)
    if pm1:
        return torch.rand(B, 3, H, W, generator=g) * 2 - 1
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    img[:, :, :H // 2] = (torch.arange(B, dtype=torch.uint8) * 60 + 30)[:, None, None, None]       # images that differ in the large
    return img


def _rel_per_image(got, want):
    got, want = got.double().cpu().reshape(len(want), -1), want.reshape(len(want), -1)
    return float(((got - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())


@pytest.mark.parametrize('B,H,W,pm1', [(1, 224, 224, False), (3, 224, 224, False), (2, 256, 256, False), (2, 160, 288, True)])
def test_detector_against_float64(det, sd, B, H, W, pm1):
    img = _images(B, H, W, 11 + B + H, pm1)
    rng = 'pm1' if pm1 else None
    got = det(img.to(DEV), input_range=rng)
    assert got.shape == (B, 128) and got.dtype == torch.float32 and det.dim == 128
    want = ref.features_f64(sd, img, rng)
    assert float(want.amax(dim=1).min()) > 0 and float((want > 0).double().mean()) > 0.2
    err = _rel_per_image(got, want)
    print(f'vgg16 B={B} {H}x{W} pm1={pm1}: rel err {err:.2e}')
    assert err <= BOUND


@pytest.mark.parametrize('size', [256, 299, 512, 1024, 160, 288, 224])
@pytest.mark.parametrize('form', ['u8', 'f255', 'pm1', 'u8pm1'])
def test_front_end_against_float64(size, form):
    from shgan_amd import kernels, vgg16
    H, W = size, (size if size != 160 else 288)
    mean, std = (123.68, 116.779, 103.939), (58.4, 57.1, 57.4)
    if form in ('u8', 'u8pm1'):
        img = _images(2, H, W, size)
    elif form == 'f255':
        img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(size)) * 255
    else:
        img = _images(2, H, W, size, pm1=True)
    rng = 'pm1' if form in ('pm1', 'u8pm1') else None
    got = vgg16.frontend(img.to(DEV), rng, mean, std)
    assert got.shape == (2, 3, 224, 224)
    if form == 'u8pm1':                 # a loader's decoded pixels: the value table first, then the float rule
        want = ref.frontend_f64(kernels.u8_value_table('cpu')[img.long()], 'pm1', mean, std)
    else:
        want = ref.frontend_f64(img, rng, mean, std)
    err = _rel_per_image(got, want)
    print(f'vgg16 front end {form} {H}x{W}: rel err {err:.2e}')
    assert err <= BOUND


@pytest.mark.parametrize('shape', [(2, 5, 8, 8), (1, 3, 7, 10), (3, 2, 9, 5), (1, 64, 224, 224)])
def test_maxpool2_is_bit_exact(shape):
    from shgan_amd import vgg16
    x = torch.randn(shape, generator=torch.Generator().manual_seed(shape[2]))
    got = vgg16.maxpool2(x.to(DEV)).cpu()
    assert torch.equal(got, F.max_pool2d(x, 2))


def test_bgr_equals_rgb_on_the_flipped_image(sd):
    from shgan_amd import vgg16
    mean, std = (123.68, 116.779, 103.939), (58.4, 57.1, 57.4)
    rgb = vgg16.Vgg16Features.from_state_dict(sd, device=DEV, mean=mean, std=std)
    bgr = vgg16.Vgg16Features.from_state_dict(sd, device=DEV, mean=mean, std=std, bgr=True)
    img = _images(2, 224, 224, 77)
    a, b = bgr(img.to(DEV)), rgb(img.flip(1).to(DEV))
    want = ref.features_f64(sd, img.flip(1), None, mean, std)
    assert _rel_per_image(a, b.double().cpu()) <= BOUND and _rel_per_image(a, want) <= BOUND
    assert _rel_per_image(rgb(img.to(DEV)), want) > 1e-3                 # the flip matters on this image


def test_features_are_the_same_bits_in_any_batch(det):
    img = _images(3, 256, 256, 5).to(DEV)
    batch = det(img)
    for i in range(3):
        assert torch.equal(det(img[i:i + 1])[0], batch[i]), i
    assert torch.equal(det(img), batch)


# ---- the loop

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


def test_eval_loop_precision_recall(small_g, det):
    """40 items, batch 8, two streams: pr_value() equals pr_from_features on features recomputed outside the loop from the kept images
    (and the loader's reals); with pr=None the images, the image metrics and the FID moments are those of a loop without the argument."""
    from shgan_amd import eval_harness as hz, kernels, precision_recall as prm
    n_items, b, R = 40, 8, 256

    def feats(img, input_range='0_255'):
        if input_range == 'pm1':
            img = (kernels.u8_value_table(DEV)[img.long()] if img.dtype == torch.uint8 else img) * 127.5 + 127.5
        return hz.standin_features(img, 64)

    def run(**kw):
        loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=2, latent_fn=_latents, feature_fn=feats, fid_dim=64, fid_real=True,
                           metrics=('psnr', 'ssim'), **kw)
        np.random.seed(21)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
        return loop, loop.gather()
    loop, (images, fid) = run(pr=dict(detector=det, nhood_size=3))
    none, (images_n, fid_n) = run(pr=None)
    plain, (images_p, fid_p) = run()
    torch.cuda.synchronize()
    assert none.pr_features is None and 'pr' not in none.evaluators and 'pr' not in plain.evaluators and 'pr' in loop.evaluators
    for other, im, fd in ((none, images_n, fid_n), (loop, images, fid)):
        assert torch.equal(im, images_p) and torch.equal(fd.S, fid_p.S) and torch.equal(other.fid_real.S, plain.fid_real.S)
        assert set(other.image_metrics) == set(plain.image_metrics)
        for key, v in plain.image_metrics.items():
            assert np.array_equal(np.asarray(torch.as_tensor(other.image_metrics[key]).cpu()), np.asarray(torch.as_tensor(v).cpu())), key
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)]).to(DEV)
    f_fake = torch.cat([det(images[k:k + b]) for k in range(0, n_items, b)])
    f_real = torch.cat([det(reals[k:k + b], input_range='pm1') for k in range(0, n_items, b)])
    fake16, real16 = loop.pr_features
    assert fake16.shape == (n_items, 128) and fake16.dtype == torch.float16
    assert torch.equal(fake16, f_fake.to(torch.float16)) and torch.equal(real16, f_real.to(torch.float16))
    got = loop.pr_value()
    want = prm.pr_from_features(f_real, f_fake, nhood_size=3)
    print(f'loop precision / recall {got} (restatement {ref.pr16(f_real.cpu().numpy(), f_fake.cpu().numpy(), 3)})')
    assert got == want and all(0.0 <= v <= 1.0 for v in got)
