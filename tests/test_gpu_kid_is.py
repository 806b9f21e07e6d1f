"""GPU: KID and the Inception Score on the device -- the fp64-MFMA polynomial-kernel sums and the in-place IS accumulator of csrc/kid.hip,
the classifier head of csrc/inception.hip, and EvalLoop's ``kid`` / ``inception_score`` options -- against the float64 yardsticks of
tests/kid_is_f64.py.

Tolerances.  KID sums: fp64 products and sums, relative round-off of order (D + m^2 / tiles) * 2^-53 ~ 1e-12 at D = 2048, m = 100; each
sum is held to 1e-11 relative, the KID to 1e-11 * (|a_xx| + |a_yy|) / (m - 1) / m absolute (it is a difference of large sums).  Head: the
distance of torch's CPU float32 softmax(linear) from float64 on the test's own inputs (relative to the row's largest probability) is
measured in the test; the kernel gets 4 x that (another summation order over 2048 terms), and never more than the project's 1e-3.  IS
accumulator: fp64 sums of float32 inputs, 1e-12 relative per entry; mean and std 1e-10 relative, each to itself."""
import numpy as np
import pytest
import torch

import inception_f64 as inc_ref
import kid_is_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KID_CASES = [(70, 90, 37, 3), (64, 64, 64, 2), (130, 101, 100, 4), (5, 7, 2, 1)]      # (n_f, n_r, m, S)


def _features(n, D, seed, dtype):
    """Non-negative rows like pooled activations, of unequal norms."""
    g = np.random.RandomState(seed)
    f = g.rand(n, D) * g.rand(n, 1) * 2 + 0.05 * g.randn(n, D) ** 2
    return torch.from_numpy(f).to(dtype)


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [64, 2048])
@pytest.mark.parametrize('n_f,n_r,m,S', KID_CASES)
def test_kid_sums_against_float64(n_f, n_r, m, S, D, dtype):
    """Ragged last tile (37), whole tiles with m == n (64), two tiles per side (100), the minimum (2); D of one chunk row and of 128."""
    from shgan_amd import kid
    fake, real = _features(n_f, D, 1, dtype), _features(n_r, D, 2, dtype)
    idx_f, idx_r, mm = kid.kid_subsets(n_f, n_r, S, m, seed=4)
    assert mm == m
    got = kid.kid_sums(fake.to(DEV), real.to(DEV), torch.from_numpy(idx_f).to(DEV), torch.from_numpy(idx_r).to(DEV))
    assert got.shape == (S, 3) and got.dtype == torch.float64
    want = ref.kid_sums_f64(fake.numpy(), real.numpy(), idx_f, idx_r)
    err = _rel(got.cpu().numpy(), want)
    print(f'kid sums ({n_f},{n_r},{m},{S}) D={D} {dtype}: {err:.2e}')
    assert err <= 1e-11


def test_kid_gather_follows_hand_built_tables():
    """Subset 0 is the identity, subset 1 a permutation of it (the same three sums up to summation order), subset 2 shares rows with
    both and reaches the rows past m; the real side uses other tables than the fake side."""
    from shgan_amd import kid
    n, m, D = 12, 8, 64
    fake, real = _features(n, D, 3, torch.float32), _features(n, D, 4, torch.float32)
    idx_f = np.array([np.arange(8), [7, 6, 5, 4, 3, 2, 1, 0], [11, 3, 5, 0, 9, 2, 10, 8]], dtype=np.int32)
    idx_r = np.array([np.arange(8), [3, 1, 0, 2, 7, 5, 6, 4], [0, 1, 2, 3, 11, 10, 9, 8]], dtype=np.int32)
    got = kid.kid_sums(fake.to(DEV), real.to(DEV), torch.from_numpy(idx_f).to(DEV), torch.from_numpy(idx_r).to(DEV)).cpu().numpy()
    want = ref.kid_sums_f64(fake.numpy(), real.numpy(), idx_f, idx_r)
    assert _rel(got, want) <= 1e-11
    assert _rel(got[1], got[0]) <= 1e-11 and _rel(got[2], got[0]) > 1e-3


def test_kid_same_rows_on_both_sides():
    """x == y: the xx term equals the xy term minus its diagonal, and equals the yy term bit for bit."""
    from shgan_amd import kid
    n, m, D, S = 90, 70, 64, 2
    f = _features(n, D, 5, torch.float64)
    idx, _, _ = kid.kid_subsets(n, n, S, m, seed=6)
    t = torch.from_numpy(idx).to(DEV)
    got = kid.kid_sums(f.to(DEV), f.to(DEV), t, t).cpu().numpy()
    assert np.array_equal(got[:, 0], got[:, 1])
    for s in range(S):
        x = f.numpy()[idx[s]]
        diag = ((np.sum(x * x, axis=1) / D + 1) ** 3).sum()
        assert abs(got[s, 0] - (got[s, 2] - diag)) <= 1e-11 * abs(got[s, 2])


def test_kid_sums_repeat_bit_for_bit_and_do_not_depend_on_the_other_subsets():
    from shgan_amd import kid
    n_f, n_r, m, S, D = 130, 101, 100, 4, 2048
    fake, real = _features(n_f, D, 7, torch.float32).to(DEV), _features(n_r, D, 8, torch.float32).to(DEV)
    idx_f, idx_r, _ = kid.kid_subsets(n_f, n_r, S, m, seed=2)
    tf, tr = torch.from_numpy(idx_f).to(DEV), torch.from_numpy(idx_r).to(DEV)
    a, b = kid.kid_sums(fake, real, tf, tr), kid.kid_sums(fake, real, tf, tr)
    assert torch.equal(a, b)
    for s in (0, 2, 3):
        alone = kid.kid_sums(fake, real, tf[s:s + 1].contiguous(), tr[s:s + 1].contiguous())
        assert torch.equal(alone[0], a[s]), s
    pair = kid.kid_sums(fake, real, tf[[3, 1]].contiguous(), tr[[3, 1]].contiguous())
    assert torch.equal(pair[0], a[3]) and torch.equal(pair[1], a[1])


def test_kid_out_of_range_index_gives_nan_for_its_subset_only():
    from shgan_amd import kid
    fake, real = _features(9, 64, 1, torch.float32).to(DEV), _features(9, 64, 2, torch.float32).to(DEV)
    idx_f = torch.tensor([[0, 1, 2, 3], [4, 9, 6, 7], [8, 1, 0, 2]], dtype=torch.int32, device=DEV)       # row 9 does not exist
    idx_r = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7], [8, 1, -1, 2]], dtype=torch.int32, device=DEV)
    got = kid.kid_sums(fake, real, idx_f, idx_r).cpu().numpy()
    assert np.all(np.isfinite(got[0])) and np.isnan(got[1, 0]) and np.isnan(got[1, 2]) and np.isfinite(got[1, 1])
    assert np.isfinite(got[2, 0]) and np.isnan(got[2, 1]) and np.isnan(got[2, 2])


@pytest.mark.parametrize('n_f,n_r,cap,S', [(130, 101, 100, 4), (70, 90, 37, 3)])
def test_kid_from_features_against_float64(n_f, n_r, cap, S):
    from shgan_amd import kid
    D = 2048
    fake, real = _features(n_f, D, 11, torch.float32), _features(n_r, D, 12, torch.float32) * 1.1
    got = kid.kid_from_features(fake.to(DEV), real.to(DEV), num_subsets=S, max_subset_size=cap, seed=5)
    idx_f, idx_r, m = kid.kid_subsets(n_f, n_r, S, cap, 5)
    want = ref.kid_f64(fake.numpy(), real.numpy(), idx_f, idx_r)
    sums = ref.kid_sums_f64(fake.numpy(), real.numpy(), idx_f, idx_r)
    bound = 1e-11 * float(np.mean(np.abs(sums[:, 0]) + np.abs(sums[:, 1]))) / (m - 1) / m
    print(f'kid {got:.12e} vs float64 {want:.12e}: |diff| {abs(got - want):.2e}, bound {bound:.2e}')
    assert isinstance(got, float) and abs(got - want) <= bound


def _head_inputs(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.rand(B, 2048, generator=g) * torch.rand(B, 1, generator=g)
    w = torch.randn(C, 2048, generator=g) * 0.05            # logits of standard deviation ~1: no probability underflows
    b = torch.randn(C, generator=g) * 0.5
    return feats, w, b


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('B', [1, 5, 16])
@pytest.mark.parametrize('C', [1008, 1000])
def test_head_probabilities_against_float64(C, B, bias):
    from shgan_amd import inception
    feats, w, b = _head_inputs(B, C, C + B)
    got = inception.head_probs(feats.to(DEV), w.to(DEV), b.to(DEV) if bias else None)
    assert got.shape == (B, C) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    want = ref.softmax_head_f64(feats.numpy(), w.numpy(), b.numpy() if bias else None)
    assert want.min() > 1e-30
    top = want.max(axis=1, keepdims=True)
    cpu = torch.softmax(torch.nn.functional.linear(feats, w, b if bias else None), dim=1).numpy().astype(np.float64)
    d_torch = float(np.max(np.abs(cpu - want) / top))
    d_kernel = float(np.max(np.abs(got - want) / top))
    print(f'head C={C} B={B} bias={bias}: torch CPU float32 {d_torch:.2e}, kernel {d_kernel:.2e}')
    assert d_kernel <= min(4 * d_torch, 1e-3)
    # rows sum to 1 within float32 round-off: the divisor is a float32 sum of C terms through at most 16 roundings (2 per thread, 6
    # butterfly steps, 8 wave partials) and each quotient is rounded once
    assert float(np.max(np.abs(got.sum(axis=1) - 1))) <= 17 * 2.0 ** -24


@pytest.fixture(scope='module')
def sd():
    d = inc_ref.random_state_dict(7)
    g = torch.Generator().manual_seed(70)
    d['fc.weight'] = torch.randn(1008, 2048, generator=g) * 0.05
    d['fc.bias'] = torch.randn(1008, generator=g) * 0.5
    return d


@pytest.fixture(scope='module')
def det(sd):
    """The seeded random-weight detector of tests/test_gpu_inception.py with a classifier head; split_k=False: an image's features are
    the same bits in any batch."""
    from shgan_amd import inception
    return inception.InceptionFeatures.from_state_dict(sd, device=DEV, split_k=False)


def test_detector_probabilities_and_unchanged_features(det, sd):
    img = torch.randint(0, 256, (5, 3, 256, 256), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    img[:, :, :128] = (torch.arange(5, dtype=torch.uint8) * 50)[:, None, None, None]
    img = img.to(DEV)
    assert det.num_classes == 1008
    before = det(img, return_features=True)
    probs = det(img, return_features=False)
    biased = det(img, return_features=False, no_output_bias=False)
    feats2, probs2 = det(img, with_probs=True)
    after = det(img, return_features=True)
    torch.cuda.synchronize()
    assert torch.equal(before, after) and torch.equal(before, feats2) and torch.equal(probs, probs2)
    assert probs.shape == (5, 1008) and probs.dtype == torch.float32 and not torch.equal(probs, biased)
    f = before.cpu().numpy()
    for got, b in ((probs, None), (biased, sd['fc.bias'].numpy())):
        want = ref.softmax_head_f64(f, sd['fc.weight'].numpy(), b)
        top = want.max(axis=1, keepdims=True)
        cpu = torch.softmax(torch.nn.functional.linear(before.cpu(), sd['fc.weight'], None if b is None else sd['fc.bias']), dim=1).numpy()
        d_torch, d_kernel = float(np.max(np.abs(cpu - want) / top)), float(np.max(np.abs(got.cpu().numpy() - want) / top))
        print(f'detector head: torch CPU float32 {d_torch:.2e}, kernel {d_kernel:.2e}')
        assert d_kernel <= min(4 * d_torch, 1e-3)


def _probs(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(n, C, generator=g) * 2, dim=1)


@pytest.mark.parametrize('C', [1008, 1000])
def test_is_accumulator_against_float64(C):
    """Batches of 5 and 16 into one buffer, two padded duplicates (-1) among them; the splits follow the slice rule over the 19 counted
    images, so the direct formula applies to them in order."""
    from shgan_amd import inception_score as isc
    S, N = 3, 19
    probs = _probs(21, C, C)
    splits = np.empty(21, dtype=np.int32)
    skip = (3, 12)
    keep = [i for i in range(21) if i not in skip]
    splits[list(skip)] = -1
    splits[keep] = [isc.split_of(j, N, S) for j in range(N)]
    acc = isc.new_accumulator(S, C, DEV)
    t = torch.from_numpy(splits).to(DEV)
    isc.is_accumulate(acc, probs[:5].to(DEV), t[:5])
    isc.is_accumulate(acc, probs[5:].to(DEV), t[5:])
    again = isc.new_accumulator(S, C, DEV)
    isc.is_accumulate(again, probs[:5].to(DEV), t[:5])
    isc.is_accumulate(again, probs[5:].to(DEV), t[5:])
    assert torch.equal(acc, again)
    got = acc.cpu().numpy()
    want = ref.is_accumulator_f64(probs.numpy(), splits, S)
    assert np.array_equal(got[:, C + 1], want[:, C + 1]) and got[:, C + 1].sum() == N
    err = _rel(got[:, :C + 1], want[:, :C + 1])
    print(f'IS accumulator C={C}: {err:.2e}')
    assert err <= 1e-12
    mean, std = isc.is_from_accumulator(acc)
    wm, ws = ref.is_f64(probs.numpy()[keep], S)
    print(f'IS {mean:.12f} +- {std:.12f} vs float64 {wm:.12f} +- {ws:.12f}')
    assert abs(mean - wm) <= 1e-10 * wm and abs(std - ws) <= 1e-10 * ws


def test_is_accumulator_zero_probability_contributes_zero():
    from shgan_amd import inception_score as isc
    C = 1008
    probs = _probs(5, C, 3)
    probs[2, 7] = 0.0
    probs[4, :500] = 0.0
    splits = torch.tensor([0, 0, 1, -1, 1], dtype=torch.int32)
    acc = isc.is_accumulate(isc.new_accumulator(2, C, DEV), probs.to(DEV), splits.to(DEV)).cpu().numpy()
    assert np.all(np.isfinite(acc))
    want = ref.is_accumulator_f64(probs.numpy(), splits.numpy(), 2)
    assert np.array_equal(acc[:, :C] == 0, want[:, :C] == 0)
    nz = want != 0
    assert _rel(acc[nz], want[nz]) <= 1e-12
    assert np.all(np.isfinite(isc.is_from_accumulator(acc)))


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


def test_eval_loop_kid_and_inception_score(small_g, det):
    """24 items, batch 8, two streams: kid_value() and is_value() equal the yardsticks on the features / probabilities of the detector
    run directly on the gathered images (and the loader's reals); images and FID moments are the same bits with the options off."""
    from shgan_amd import eval_harness as hz, kid
    n_items, b, R = 24, 8, 256
    kid_opts = dict(num_subsets=4, max_subset_size=16, seed=1)

    def run(**kw):
        loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=2, feature_fn=det, latent_fn=_latents, fid_real=True, **kw)
        np.random.seed(21)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
        return loop, loop.gather()
    loop, (images, fid) = run(kid=kid_opts, inception_score=dict(num_splits=3))
    plain, (images0, fid0) = run()
    torch.cuda.synchronize()
    assert plain.kid_features is None and plain.is_acc is None
    assert torch.equal(images, images0) and torch.equal(fid.S, fid0.S) and torch.equal(loop.fid_real.S, plain.fid_real.S)
    reals = torch.cat([img for img, _ in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=13)]).to(DEV)
    f_fake, p_fake, f_real = [], [], []
    for k in range(0, n_items, b):
        f, p = det(images[k:k + b], with_probs=True)
        f_fake.append(f)
        p_fake.append(p)
        f_real.append(det(reals[k:k + b], input_range='pm1'))
    f_fake, p_fake, f_real = (torch.cat(t).cpu().numpy() for t in (f_fake, p_fake, f_real))
    assert loop.kid_features[0].shape == (n_items, 2048)
    assert np.array_equal(loop.kid_features[0].cpu().numpy(), f_fake) and np.array_equal(loop.kid_features[1].cpu().numpy(), f_real)
    idx_f, idx_r, m = kid.kid_subsets(n_items, n_items, **kid_opts)
    want = ref.kid_f64(f_fake, f_real, idx_f, idx_r)
    sums = ref.kid_sums_f64(f_fake, f_real, idx_f, idx_r)
    bound = 1e-11 * float(np.mean(np.abs(sums[:, 0]) + np.abs(sums[:, 1]))) / (m - 1) / m
    got = loop.kid_value()
    print(f'loop kid {got:.12e} vs float64 {want:.12e} (bound {bound:.2e})')
    assert abs(got - want) <= bound
    wm, ws = ref.is_f64(p_fake, 3)
    mean, std = loop.is_value()
    print(f'loop IS {mean:.12f} +- {std:.12f} vs float64 {wm:.12f} +- {ws:.12f}')
    assert float(loop.is_acc[:, -1].sum()) == n_items
    assert abs(mean - wm) <= 1e-10 * wm and abs(std - ws) <= 1e-10 * ws
