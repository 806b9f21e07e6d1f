"""GPU: the FID detector (sh-gan_amd/inception.py, csrc/inception.hip) against the float64 CPU model of tests/inception_f64.py -- every
convolution geometry of the network, the pools, the front end, the whole detector at several input sizes, batch invariance, and
EvalLoop with the detector on both the fakes and the reals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _rel(a, b):
    a, b = a.detach().cpu().to(torch.float64), b.detach().cpu().to(torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _geometries():
    from shgan_amd import inception
    seen, out = set(), []
    for name, (i, o, k, s, p, h) in inception.LAYERS.items():
        key = (i, o, k, s, p, h)
        if key not in seen:
            seen.add(key)
            out.append((name,) + key)
    return out


@pytest.fixture(scope='module')
def sd():
    return ref.random_state_dict(7)


@pytest.fixture(scope='module')
def det(sd):
    from shgan_amd import inception
    return inception.InceptionFeatures.from_state_dict(sd, device=DEV)


@pytest.mark.parametrize('B', [1, 3])
def test_every_convolution_geometry_against_float64(B):
    """Each distinct (kernel, stride, pad, I, O, grid) of the 94 layers, written at a channel offset of a wider buffer from a channel slice
    of a wider input (the concat-buffer form); the launch plan splits K where the grid is small.  Max error / max |output| <= 1e-5."""
    from shgan_amd import inception
    g = torch.Generator().manual_seed(B)
    worst = 0.0
    for name, i, o, k, s, p, h in _geometries():
        w = torch.randn(o, i, *k, generator=g, dtype=torch.float64) * np.sqrt(2.0 / (i * k[0] * k[1]))
        b = torch.randn(o, generator=g, dtype=torch.float64) * 0.1
        x = torch.randn(B, i + 5, h, h, generator=g).to(torch.float32)
        wp, bp = inception.pack_weight(w.to(torch.float32).to(DEV), b.to(torch.float32).to(DEV))
        op = inception.ConvOp(name, wp, bp, i, o, k, s, p)
        oh, ow = inception.out_size(h, k[0], s[0], p[0]), inception.out_size(h, k[1], s[1], p[1])
        y = torch.full((B, o + 24, oh, ow), 7.0, device=DEV)
        inception.conv_group([(op, x.to(DEV), 3, y, 17)])
        want = F.relu(F.conv2d(x[:, 3:3 + i].to(torch.float64), w.to(torch.float32).to(torch.float64), b.to(torch.float32).to(torch.float64),
                               stride=s, padding=p))
        got = y.cpu()
        assert torch.all(got[:, :17] == 7.0) and torch.all(got[:, 17 + o:] == 7.0), name      # nothing outside [y_coff, y_coff + O)
        err = _rel(got[:, 17:17 + o], want)
        worst = max(worst, err)
        assert err <= 1e-5, (name, B, err)
    print(f'worst conv error B={B}: {worst:.2e}')


def test_grouped_launch_and_split_k_agree_with_separate_launches():
    """A grouped launch (the branches of a Mixed block) == one launch per convolution; the split-K plan agrees with float64 as closely as
    the unsplit sums do (the two differ by rounding: 1.7e-6 measured at K = 1280); the split launches do need a workspace."""
    from shgan_amd import _lib, inception
    g = torch.Generator().manual_seed(3)
    ops, ws = [], []
    x = torch.randn(2, 1280, 8, 8, generator=g).to(DEV)
    for name, o in (('a', 320), ('b', 384), ('c', 448), ('d', 192)):
        w = torch.randn(o, 1280, 1, 1, generator=g) * 0.04
        ws.append(w)
        wp, bp = inception.pack_weight(w.to(DEV), torch.zeros(o, device=DEV))
        ops.append(inception.ConvOp(name, wp, bp, 1280, o, (1, 1), (1, 1), (0, 0)))
    ref_out = torch.empty(2, 1344, 8, 8, device=DEV)
    off = 0
    for op in ops:
        inception.conv_group([(op, x, 0, ref_out, off)], split_k=False)
        off += op.O
    split_out = torch.empty_like(ref_out)
    items, off = [], 0
    for op in ops:
        items.append((op, x, 0, split_out, off))
        off += op.O
    inception.conv_group(items, split_k=True)
    grouped = torch.empty_like(ref_out)
    inception.conv_group([(op, x, 0, grouped, o) for (op, _, _, _, o) in items], split_k=False)
    torch.cuda.synchronize()
    assert torch.equal(grouped, ref_out)                        # same plan, same bits
    want = F.relu(F.conv2d(x.cpu().double(), torch.cat(ws).double()))
    assert _rel(split_out, want) <= 1e-5 and _rel(ref_out, want) <= 1e-5 and _rel(split_out, ref_out) <= 1e-5
    d = (_lib.IncConv * 1)(ops[0].desc(x, split_out, 0, 0, 4))
    assert _lib.get_lib().shg_inception_conv_workspace_bytes(d, 1, 2) == 4 * 320 * 2 * 64 * 4


@pytest.mark.parametrize('mode,stride,pad,C,h,coff', [('max', 2, 0, 64, 147, 0), ('max', 2, 0, 192, 71, 0), ('max', 2, 0, 288, 35, 480),
                                                      ('max', 2, 0, 768, 17, 512), ('avg', 1, 1, 192, 35, 0), ('avg', 1, 1, 288, 35, 0),
                                                      ('avg', 1, 1, 768, 17, 0), ('avg', 1, 1, 1280, 8, 0), ('max', 1, 1, 2048, 8, 0)])
def test_pools(mode, stride, pad, C, h, coff):
    """Max pools bit-exact against float32 torch; average pools (count_include_pad=False) within 1e-6 of float64."""
    from shgan_amd import inception
    for B in (1, 3):
        x = torch.randn(B, C, h, h, generator=torch.Generator().manual_seed(C + B))
        oh = inception.out_size(h, 3, stride, pad)
        y = torch.full((B, C + coff + 8, oh, oh), 5.0, device=DEV)
        inception.pool(x.to(DEV), mode, stride, pad, y=y, y_coff=coff)
        got = y.cpu()
        assert torch.all(got[:, :coff] == 5.0) and torch.all(got[:, coff + C:] == 5.0)
        got = got[:, coff:coff + C]
        if mode == 'max':
            assert torch.equal(got, F.max_pool2d(x, 3, stride, pad))
        else:
            assert _rel(got, F.avg_pool2d(x.double(), 3, stride, pad, count_include_pad=False)) <= 1e-6


def test_global_mean():
    from shgan_amd import inception
    x = torch.rand(3, 2048, 8, 8, generator=torch.Generator().manual_seed(2))
    assert _rel(inception.global_mean(x.to(DEV)), x.double().mean(dim=(2, 3))) <= 1e-6


@pytest.mark.parametrize('size', [256, 512, 1024, 299, (200, 300)])
def test_front_end_against_float64(size):
    """uint8 composite, float 0..255, float [-1, 1] reals and uint8 reals -> resize + (x - 128) / 128 within 1e-6 of float64."""
    from shgan_amd import inception
    h, w = (size, size) if isinstance(size, int) else size
    g = torch.Generator().manual_seed(h * 7 + w)
    u8 = torch.randint(0, 256, (2, 3, h, w), generator=g, dtype=torch.uint8)
    f255 = torch.rand(2, 3, h, w, generator=g) * 255
    pm1 = torch.rand(2, 3, h, w, generator=g) * 2 - 1
    for img, rng in ((u8, '0_255'), (f255, '0_255'), (pm1, 'pm1'), (u8, 'pm1')):
        got = inception.frontend(img.to(DEV), rng)
        want = ref.frontend_f64(img, rng)
        assert got.shape == (2, 3, 299, 299)
        assert _rel(got, want) <= 1e-6, (size, rng, img.dtype)


@pytest.mark.parametrize('size,B,kind', [(299, 2, 'f255'), (256, 3, 'u8'), (512, 2, 'pm1'), (1024, 2, 'u8pm1')])
def test_detector_against_float64_model(det, sd, size, B, kind):
    g = torch.Generator().manual_seed(size + B)
    if kind in ('u8', 'u8pm1'):
        img = torch.randint(0, 256, (B, 3, size, size), generator=g, dtype=torch.uint8)
        # some structure on top of the noise, so that the features differ between the images
        img[:, :, : size // 2] = (torch.arange(B, dtype=torch.uint8) * 60)[:, None, None, None]
    elif kind == 'f255':
        img = torch.rand(B, 3, size, size, generator=g) * 255
    else:
        img = torch.rand(B, 3, size, size, generator=g) * 2 - 1
    rng = 'pm1' if kind in ('pm1', 'u8pm1') else '0_255'
    got = det(img.to(DEV), return_features=True, input_range=rng)
    torch.cuda.synchronize()
    want = ref.detector_f64(sd, img, rng)
    assert got.shape == (B, 2048) and got.dtype == torch.float32
    err = _rel(got, want)
    print(f'detector {size} x {B} {kind}: {err:.2e}')
    assert err <= 1e-4


def test_batch_invariance(det, sd):
    """Without split-K the launch plan does not depend on B: an image's features are the same bits in batch 1 and batch 8.  The default
    plan splits K in the small late-layer launches at batch 1 and not at batch 8, so there the features agree to rounding (1e-6)."""
    from shgan_amd import inception
    img = torch.randint(0, 256, (8, 3, 256, 256), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).to(DEV)
    fixed = inception.InceptionFeatures(det.ops, DEV, split_k=False)
    a8, a1 = fixed(img), fixed(img[5:6])
    s8, s1 = det(img), det(img[5:6])
    torch.cuda.synchronize()
    assert torch.equal(a8[5:6], a1)
    assert _rel(s1, s8[5:6]) <= 1e-6 and _rel(s8, a8) <= 1e-6


def test_fid_stats_add_images_takes_the_detector(det, sd):
    from shgan_amd.fid_stats import FidStats
    img = torch.randint(0, 256, (3, 3, 128, 128), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(DEV)
    st = FidStats(2048, device=DEV)
    f = st.add_images(det, img)
    assert f.shape == (3, 2048) and st.mean_cov()[0] == 3
    assert _rel(f, ref.detector_f64(sd, img.float().cpu())) <= 1e-4
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError):
        det(img, return_features=False)


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


def _moments(f):
    f = f.numpy()
    mu = f.mean(0)
    return mu, f.T @ f / len(f) - np.outer(mu, mu)


def test_eval_loop_fid_fake_and_real_sides(small_g, det, sd):
    """EvalLoop(feature_fn=det, fid_real=True) on four streams, 48 items: both sides' moments equal float64 moments of the float64 model's
    features of the kept uint8 composites and of the loader's reals; fid_value() equals fid_from_stats on those; fid_real=False gives the
    same fake moments as a run without the keyword."""
    from shgan_amd import eval_harness as hz
    from shgan_amd.fid_stats import fid_from_stats
    n_items, b, R = 48, 8, 256
    loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=4, feature_fn=det, latent_fn=_latents, fid_real=True)
    np.random.seed(21)
    loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
    images, fid = loop.gather()
    torch.cuda.synchronize()
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)])
    f_fake = ref.detector_f64(sd, images.cpu())
    f_real = ref.detector_f64(sd, reals, 'pm1')
    for st, f in ((fid, f_fake), (loop.fid_real, f_real)):
        n, mu, sg = st.mean_cov()
        mu0, sg0 = _moments(f)
        assert n == n_items
        e_mu, e_sg = np.abs(mu - mu0).max() / np.abs(mu0).max(), np.abs(sg - sg0).max() / np.abs(sg0).max()
        print(f'moments: mean {e_mu:.2e} cov {e_sg:.2e}')
        assert e_mu <= 1e-5 and e_sg <= 1e-4
    want = fid_from_stats(*_moments(f_fake), *_moments(f_real))
    got = loop.fid_value()
    print(f'fid {got:.6f} vs float64 {want:.6f}')
    assert abs(got - want) <= 1e-3 * abs(want)
    # fid_real=False: the loop of before (same streams, same values)
    runs = []
    for kw in ({}, {'fid_real': False}):
        lp = hz.EvalLoop(small_g, DEV, R, 16, noise_mode='const', depth=4, feature_fn=det, latent_fn=_latents, **kw)
        np.random.seed(21)
        lp.run(hz.PinnedU8Loader(lp.ids, b, R, seed=13))
        runs.append(lp.gather())
        assert lp.fid_real is None
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1].S, runs[1][1].S)
