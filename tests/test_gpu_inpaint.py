"""GPU: sh-gan_amd/inpaint.py on csrc/inpaint.hip against the numpy yardstick of tests/inpaint_f64.py -- ``gather_windows`` byte for byte,
the feather weight exactly, ``paste_back`` under the byte rule stated (and derived) there, ``Inpainter`` end to end, and the fill / guard
runs of the new allocation sites (they are newer than the site tables of tests/test_gpu_alloc_fill.py / test_gpu_alloc_guard.py).
R = 16 planes (``gather_windows`` also at 37 and 144) and random ``fake``; no generator except in the end-to-end test."""
import numpy as np
import pytest
import torch

import inpaint_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
R = 16
FEATHERS = (0, 1, 5, 32)
_CACHE = {}


def _batch(ids, k=1, R=R):
    """The cases ``ids`` of ref.CASES as one ragged launch: (cases, packed, packed_mask, shapes [B,4], windows [B,4], fake [B k,3,R,R])."""
    key = (tuple(ids), k, R)
    if key not in _CACHE:
        from shgan_amd import inpaint, resize
        cases = [ref.make_case(i, R, k) for i in ids]
        packed, shapes = resize.pack_images([c[0] for c in cases])
        packed_mask, moffs = inpaint.pack_masks([c[1] for c in cases])
        shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
        windows = np.array([c[2] for c in cases], np.int64)
        fake = torch.from_numpy(np.concatenate([c[3] for c in cases]))
        _CACHE[key] = (cases, packed, packed_mask, shapes, windows, fake)
    cases, packed, packed_mask, shapes, windows, fake = _CACHE[key]
    return cases, packed.to(DEV), packed_mask.to(DEV), shapes, windows, fake.to(DEV)


ALL = tuple(range(len(ref.CASES)))


def _images(out, shapes):
    """out uint8 [K, bytes] -> [[h, w, 3] per image] per sample."""
    out = out.cpu().numpy()
    return [[row[off:off + 3 * h * w].reshape(h, w, 3) for h, w, off in shapes[:, :3]] for row in out]


def _single(i, k=1, R=R):
    return _batch((i,), k, R)


def test_packed_offsets_are_ragged():
    _, _, _, shapes, _, _ = _batch(ALL)
    assert (shapes[:, 2] % 4 != 0).any() and (shapes[:, 3] % 4 != 0).any()


@pytest.mark.parametrize('R', [16, 37, 144])
def test_gather_windows_equals_the_reference_in_a_ragged_batch_and_alone(R):
    """R = 16: one band, one chunk, every store a packed word; 37: 3 bands and byte stores (R % 4 != 0); 144: 9 bands and 2 chunks
    (128 + a ragged 16), up-sampling on both axes for the small cases and mixed up / down for 150 x 201."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, _ = _batch(ALL, R=R)
    real, mask = inpaint.gather_windows(packed, pm, shapes, windows, R)
    assert real.shape == (len(cases), 3, R, R) and real.dtype == torch.uint8 and mask.shape == (len(cases), 1, R, R) and mask.dtype == torch.float32
    real, mask = real.cpu().numpy(), mask.cpu().numpy()
    for i, (img, m, window, _) in enumerate(cases):
        want_real, want_mask = ref.gather_reference(img, m, window, R)
        assert np.array_equal(real[i], want_real), i
        assert np.array_equal(mask[i, 0], want_mask), i
        _, p1, m1, s1, w1, _ = _single(i, R=R)
        r1, k1 = inpaint.gather_windows(p1, m1, s1, w1, R)
        assert np.array_equal(r1.cpu().numpy()[0], real[i]) and np.array_equal(k1.cpu().numpy()[0], mask[i]), i
    if R == 16:                                                     # the identity: a 16 x 16 image under its full window is its own bytes
        assert np.array_equal(real[0], cases[0][0].transpose(2, 0, 1))


@pytest.mark.parametrize('feather', FEATHERS)
def test_alpha_out_equals_the_reference(feather):
    """Holes on the window's edges and corners, a one-pixel hole, a window several tiles wide and tall with holes across the tile seams,
    a hole outside the window (it does not feather): A exactly, and 0 outside the windows."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake = _batch(ALL)
    alpha = torch.full((pm.numel(),), 77, dtype=torch.uint8, device=DEV)
    inpaint.paste_back(packed, pm, shapes, windows, fake, feather=feather, alpha_out=alpha)
    alpha = alpha.cpu().numpy()
    for (img, m, (y0, x0, ch, cw), _), (h, w, _, moff) in zip(cases, shapes):
        want = np.zeros((h, w), np.uint8)
        want[y0:y0 + ch, x0:x0 + cw] = ref.feather_reference(m[y0:y0 + ch, x0:x0 + cw], feather)
        assert np.array_equal(alpha[moff:moff + h * w].reshape(h, w), want), (h, w, feather)


@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('feather', (0, 5, 32))
def test_paste_back_obeys_the_byte_rule(k, feather):
    """Every case, every sample: within 1 of the float64 byte, the original's wherever A = 0 (so: outside the feather band and outside the
    window), the float64 byte wherever its pre-truncation value is farther than eps from an integer, at most 1 % of the window pixels
    left out.  Row j of ``out`` holds sample j of every image at the image's offset."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake = _batch(ALL, k)
    out = inpaint.paste_back(packed, pm, shapes, windows, fake, k=k, feather=feather)
    assert out.shape == (k, packed.numel()) and out.dtype == torch.uint8
    got = _images(out, shapes)
    worst, differ = 0.0, 0
    for i, (img, m, window, f) in enumerate(cases):
        for j in range(k):
            share, nd = ref.byte_rule(got[j][i], img, m, window, f[j], feather)
            worst, differ = max(worst, share), differ + nd
    print(f'k = {k}, feather = {feather}: at most {worst:.4%} of a window within eps of an integer; {differ} bytes differ from float64 in all')


def test_paste_back_clamps():
    """fake = +1.5 / -1.5 / +1.5 per channel: g is 255 / 0 / 255 exactly, and so is every blend's numerator an integer: the float64 bytes."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, _ = _batch(ALL)
    fake = torch.tensor([1.5, -1.5, 1.5], device=DEV).view(1, 3, 1, 1).expand(len(cases), 3, R, R).contiguous()
    got = _images(inpaint.paste_back(packed, pm, shapes, windows, fake, feather=5), shapes)[0]
    for i, (img, m, window, _) in enumerate(cases):
        want = ref.paste_reference(img, m, window, fake[i].cpu().numpy(), 5, np.float64)[0]
        assert np.array_equal(got[i], want), i


def test_the_identity_case_is_composite_u8():
    """An R x R image under its full window with feather = 0: one tap of weight 1 per axis, A in {0, 1} -- the bits of
    ``kernels.composite_u8`` on the assembled input."""
    from shgan_amd import eval_harness, inpaint, kernels
    (case,), packed, pm, shapes, windows, fake = _single(0)
    real, mask = inpaint.gather_windows(packed, pm, shapes, windows, R)
    x = eval_harness.assemble_input(real, mask)
    want = kernels.composite_u8(x, fake).cpu().numpy()[0]
    got = _images(inpaint.paste_back(packed, pm, shapes, windows, fake, feather=0), shapes)[0][0]
    assert np.array_equal(got.transpose(2, 0, 1), want)
    assert not np.array_equal(got, case[0])


def test_two_runs_and_batch_versus_single_are_bit_equal():
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake = _batch(ALL, 3)
    a = inpaint.paste_back(packed, pm, shapes, windows, fake, k=3, feather=5)
    out = torch.full_like(a, 9)
    b = inpaint.paste_back(packed, pm, shapes, windows, fake, k=3, feather=5, out=out)
    assert b is out and torch.equal(a, b)
    got = _images(a, shapes)
    for i in range(len(cases)):
        _, p1, m1, s1, w1, f1 = _single(i, 3)
        alone = _images(inpaint.paste_back(p1, m1, s1, w1, f1, k=3, feather=5), s1)
        for j in range(3):
            assert np.array_equal(alone[j][0], got[j][i]), (i, j)


def test_refusals():
    from shgan_amd import _lib, inpaint
    _, packed, pm, shapes, windows, fake = _single(1)
    with pytest.raises(_lib.ShgError):
        inpaint.paste_back(packed.cpu(), pm, shapes, windows, fake)
    with pytest.raises(_lib.ShgError):
        inpaint.paste_back(packed, pm, shapes, windows, fake, feather=33)
    with pytest.raises(_lib.ShgError):
        inpaint.paste_back(packed, pm, shapes, windows, fake, k=2)
    with pytest.raises(_lib.ShgError):
        inpaint.paste_back(packed, pm, shapes, windows, fake, out=torch.zeros(2, packed.numel(), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='does not lie inside'):
        inpaint.gather_windows(packed, pm, shapes, windows + 30, R)
    with pytest.raises(_lib.ShgError, match='does not lie inside packed'):
        inpaint.gather_windows(packed[:-1], pm, shapes, windows, R)


@pytest.fixture(scope='module')
def small_g():
    from shgan_amd import configs
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1)
    return G.eval().requires_grad_(False).to(DEV)


def test_inpainter_end_to_end(small_g):
    """Reduced-width seeded generator (``configs.build_generator`` + ``seeded_init_``) at R = 256, the smallest resolution the synthesis
    network is defined for (256 / 512 / 1024), three images with holes, of different sizes (one shorter than R), and one without a hole
    between them, given z.  The random weights saturate (|fake| reaches 20): see the two refinements of the byte rule.  The output
    obeys the byte rule against ``paste_reference`` fed the device's own ``fake``, so the generator's float error does not enter;
    ``samples = 2`` has the stated shape and layout."""
    from shgan_amd import inpaint
    rng = np.random.RandomState(7)
    sizes = [(300, 420), (90, 64), (200, 500), (481, 333)]
    images = [ref.random_image(rng, h, w) for h, w in sizes]
    masks = [ref.mask_with_holes(300, 420, [(100, 180, 150, 260)]), np.ones((90, 64), np.uint8), ref.mask_with_holes(200, 500, [(0, 60, 440, 500)]),
             ref.mask_with_holes(481, 333, [(200, 230, 100, 120), (260, 262, 140, 141)])]
    z = torch.from_numpy(rng.standard_normal((4, 2, 64)).astype(np.float32))
    seen = []

    def paste(packed, pm, shapes, windows, fake, k=1, feather=8):
        seen.append((shapes.copy(), windows.copy(), fake.cpu().numpy(), k))
        return inpaint.paste_back(packed, pm, shapes, windows, fake, k=k, feather=feather)

    inp = inpaint.Inpainter(small_g, 256, DEV, feather=8, batch=2, paste_fn=paste)
    res = inp(images, masks, z=z[:, 0])
    assert len(res) == 4 and np.array_equal(res[1], images[1]) and res[1] is not images[1]
    assert [len(s[0]) for s in seen] == [2, 1] and all(s[3] == 1 for s in seen)
    holed = [0, 2, 3]
    fakes = np.concatenate([s[2] for s in seen])
    windows = np.concatenate([s[1] for s in seen])
    for n, i in enumerate(holed):
        window = tuple(int(v) for v in windows[n])
        assert window == inpaint.plan_window(masks[i], 256, 0.5, 8) and res[i].shape == images[i].shape
        share, nd = ref.byte_rule(res[i], images[i], masks[i], window, fakes[n], 8)
        print(f'image {i} {sizes[i]}, window {window}: {share:.4%} within eps, {nd} bytes differ from float64')
        assert not np.array_equal(res[i], images[i])
    del seen[:]
    res2 = inp(images, masks, z=z, samples=2)
    assert [r.shape for r in res2] == [(2,) + im.shape for im in images] and np.array_equal(res2[1], np.stack([images[1]] * 2))
    assert [s[3] for s in seen] == [2, 2] and seen[0][2].shape == (4, 3, 256, 256)
    fakes2 = np.concatenate([s[2] for s in seen])
    for n, i in enumerate(holed):
        for j in range(2):
            ref.byte_rule(res2[i][j], images[i], masks[i], tuple(int(v) for v in windows[n]), fakes2[n * 2 + j], 8)
        assert not np.array_equal(fakes2[n * 2], fakes2[n * 2 + 1])             # (so the rule above tells the samples' rows apart)


def test_new_sites_do_not_depend_on_fresh_contents_and_stay_inside_their_buffers():
    """('inpaint.py', 'gather_windows') and ('inpaint.py', 'paste_back'): the same bits with every fresh allocation pre-filled with NaN
    bytes and with large values, and no guard band touched with every buffer, the operands included, housed between poisoned bands.  The
    batch ends with a window at the bottom-right corner of the last image: its last loads and stores end at the buffers' last bytes."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import inpaint
    sites = {('inpaint.py', 'gather_windows'), ('inpaint.py', 'paste_back')}
    ids = (1, 4, 6, 11, 8)
    cases, _, _, shapes, windows, _ = _batch(ids, 2)
    host = _CACHE[(ids, 2, R)]

    def run():
        packed, pm, fake = host[1].to(DEV), host[2].to(DEV), host[5].to(DEV)
        real, mask = inpaint.gather_windows(packed, pm, shapes, windows, R)
        alpha = torch.empty(pm.numel(), dtype=torch.uint8, device=DEV)
        out = inpaint.paste_back(packed, pm, shapes, windows, fake, k=2, feather=5, alpha_out=alpha)
        return [real, mask, out, alpha]
    want = run()
    torch.cuda.synchronize()
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got = run()
            torch.cuda.synchronize()
        assert sites <= rec.sites, rec.sites
        assert all(torch.equal(x, y) for x, y in zip(got, want)), pattern
    with alloc_guard.guarded() as rec:
        got = run()
        bad = rec.violations()
        assert sites <= rec.sites and not bad, bad
        assert all(torch.equal(x, y) for x, y in zip(got, want))
