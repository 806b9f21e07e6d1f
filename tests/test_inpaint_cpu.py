"""No GPU: the host side of sh-gan_amd/inpaint.py and the numpy yardstick tests/inpaint_f64.py that the GPU tests hold the kernels to --
the window planner's properties, the references against Pillow / brute force / torch, the byte rule on the float32 restatement, the
table builders, the two new C entry points' argument checks, and ``Inpainter`` with injected reference functions and a stand-in G."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import inpaint_f64 as ref
from shgan_amd import _lib, inpaint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('shg_inpaint_gather_u8', 'shg_inpaint_paste_u8')
R = 16


# ------------------------------------------------------------------------------------------------
# planner
# ------------------------------------------------------------------------------------------------

def test_planner_sweep():
    rng = np.random.RandomState(0)
    n_rect = 0
    for _ in range(400):
        H, W = (int(v) for v in rng.randint(5, 140, 2))
        Rr = int(rng.choice([8, 16, 32, 64]))
        feather = int(rng.choice([0, 1, 8, 32]))
        context = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        ya, xa = int(rng.randint(0, H)), int(rng.randint(0, W))
        yb, xb = int(rng.randint(ya + 1, H + 1)), int(rng.randint(xa + 1, W + 1))
        mask = ref.mask_with_holes(H, W, [(ya, yb, xa, xb)])
        if rng.rand() < 0.3:                                                   # a second hole: the box is the union's
            mask[rng.randint(0, H), rng.randint(0, W)] = 0
        window = inpaint.plan_window(mask, Rr, context, feather)
        ref.check_window(mask, window, Rr, context, feather)
        n_rect += window[2] != window[3]
    assert n_rect > 20                                                         # the sweep reaches rectangular windows


def test_planner_edges():
    assert inpaint.plan_window(np.ones((30, 40), np.uint8), 16) is None
    for mask, Rr in ((ref.mask_with_holes(50, 60, [(0, 3, 0, 4)]), 16), (ref.mask_with_holes(50, 60, [(47, 50, 55, 60)]), 16),      # corners
                     (np.zeros((50, 60), np.uint8), 16),                                                                          # all hole
                     (ref.mask_with_holes(10, 60, [(2, 5, 20, 30)]), 16), (ref.mask_with_holes(9, 7, [(4, 5, 3, 4)]), 16)):        # H < R; both < R
        window = inpaint.plan_window(mask, Rr, 0.5, 8)
        ref.check_window(mask, window, Rr, 0.5, 8)
    assert inpaint.plan_window(ref.mask_with_holes(50, 60, [(0, 3, 0, 4)]), 16, 0.5, 8) == (0, 0, 24, 24)
    assert inpaint.plan_window(np.zeros((50, 60), np.uint8), 16) == (0, 0, 50, 60)
    assert inpaint.plan_window(ref.mask_with_holes(9, 7, [(4, 5, 3, 4)]), 16) == (0, 0, 9, 7)
    assert inpaint.plan_window(ref.mask_with_holes(100, 100, [(40, 50, 45, 55)]), 16, 0.5, 2) == (35, 40, 20, 20)
    with pytest.raises(ValueError):
        inpaint.plan_window(np.ones((3, 4, 1)), 16)


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('idx', range(len(ref.CASES)))
def test_gather_reference_is_pillow_and_the_pooling_a_brute_force_loop(idx):
    img, mask, (y0, x0, ch, cw), _ = ref.make_case(idx)
    real, m = ref.gather_reference(img, mask, (y0, x0, ch, cw), R)
    pil = np.asarray(Image.fromarray(img).crop((x0, y0, x0 + cw, y0 + ch)).resize((R, R), Image.BICUBIC))
    assert np.array_equal(real, pil.transpose(2, 0, 1))
    mw = mask[y0:y0 + ch, x0:x0 + cw]
    assert np.array_equal(m, ref.pool_mask_bruteforce(mw, R))
    # conservative: every native hole pixel lies under a low-resolution hole pixel
    ys, xs = np.nonzero(mw == 0)
    assert np.all(m[ys * R // ch, xs * R // cw] == 0)


@pytest.mark.parametrize('feather', (0, 1, 5, 32))
def test_separable_feather_is_the_brute_force(feather):
    for idx in (1, 2, 3, 4, 5, 8, 10, 11):                                     # (the windows small enough for the per-pixel loop)
        _, mask, (y0, x0, ch, cw), _ = ref.make_case(idx)
        mw = mask[y0:y0 + ch, x0:x0 + cw]
        A = ref.feather_reference(mw, feather)
        assert np.array_equal(A, ref.feather_bruteforce(mw, feather)), idx
        assert np.array_equal(A == feather + 1, mw == 0) and A.max() <= feather + 1
    if feather == 0:
        assert set(np.unique(A)) <= {0, 1}


def test_paste_reference_keeps_the_bytes_outside_the_window_and_the_feather_band():
    img, mask, window, fake = ref.make_case(7)
    y0, x0, ch, cw = window
    for dtype in (np.float64, np.float32):
        out, t, A, _ = ref.paste_reference(img, mask, window, fake[0], 5, dtype)
        keep = np.ones(img.shape[:2], bool)
        keep[y0:y0 + ch, x0:x0 + cw] = A == 0
        assert t.dtype == dtype and np.array_equal(out[keep], img[keep]) and not np.array_equal(out[~keep], img[~keep])


def test_paste_reference_identity_is_the_torch_composite():
    """R x R image, full window, feather 0: ((x m + img (1 - m)) 127.5 + 127.5).clamp(0, 255).to(uint8) in float32, bit for bit."""
    from shgan_amd import kernels
    rng = np.random.RandomState(3)
    img = ref.random_image(rng, R, R)
    mask = ref.mask_with_holes(R, R, [(3, 9, 2, 12), (15, 16, 15, 16)])
    fake = rng.uniform(-1.3, 1.3, (3, R, R)).astype(np.float32)
    out, _, _, _ = ref.paste_reference(img, mask, (0, 0, R, R), fake, 0, np.float32)
    real = kernels.u8_value_table('cpu')[torch.from_numpy(img.transpose(2, 0, 1).copy()).long()]
    m = torch.from_numpy(mask.astype(np.float32))[None]
    want = ((real * m + torch.from_numpy(fake) * (1 - m)) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)
    assert np.array_equal(out.transpose(2, 0, 1), want.numpy())


@pytest.mark.parametrize('idx', range(len(ref.CASES)))
def test_the_float32_restatement_obeys_the_byte_rule(idx):
    img, mask, window, fake = ref.make_case(idx)
    for feather in (0, 5, 32):
        out32 = ref.paste_reference(img, mask, window, fake[0], feather, np.float32)[0]
        share, differ = ref.byte_rule(out32, img, mask, window, fake[0], feather)
        print(f'case {idx}, feather {feather}: eps {ref.eps_of(R, window[2], window[3]):.3e}, {share:.4%} of the window within eps, {differ} bytes differ')
        assert share <= ref.CAP
    bad = out32.copy()
    ys, xs = np.nonzero(mask == 0)
    bad[ys[0], xs[0], 1] ^= 2                                                  # the rule notices one wrong byte
    with pytest.raises(AssertionError):
        ref.byte_rule(bad, img, mask, window, fake[0], 32)


def test_paste_reference_clamps():
    img, mask, window, _ = ref.make_case(3)
    fake = np.broadcast_to(np.array([1.5, -1.5, 1.5], np.float32)[:, None, None], (3, R, R))
    out64, t, A, raw = ref.paste_reference(img, mask, window, fake, 5, np.float64)
    out32 = ref.paste_reference(img, mask, window, fake, 5, np.float32)[0]
    y0, x0, ch, cw = window
    assert np.array_equal(out32, out64)
    hole = A == 6
    assert np.all(out64[y0:y0 + ch, x0:x0 + cw][hole] == np.array([255, 0, 255], np.uint8))
    assert raw[..., 0].min() > 255 and raw[..., 1].max() < 0


# ------------------------------------------------------------------------------------------------
# host side of the launches
# ------------------------------------------------------------------------------------------------

def test_weight_and_table_builders_stay_inside_their_bounds():
    from shgan_amd import resize
    for n_in, n_out in ((16, 53), (16, 9), (16, 16), (512, 1400), (64, 7)):
        bounds, w = inpaint.bicubic_weights(n_in, n_out)
        assert bounds.shape == (n_out, 2) and w.shape[0] == n_out and w.dtype == np.float64
        assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] >= 1) and np.all(bounds[:, 0] + bounds[:, 1] <= n_in) and bounds[:, 1].max() <= w.shape[1]
        assert np.allclose(w.sum(1), 1.0, atol=1e-12)
        if n_in != n_out:                                                      # the same taps the fixed-point table rounds
            kb, k = resize.bicubic_coeffs(n_in, n_out)
            assert np.array_equal(kb, bounds) and np.array_equal(k, np.where(w < 0, np.trunc(-0.5 + w * 2.0 ** 22), np.trunc(0.5 + w * 2.0 ** 22)).astype(np.int32))
    shapes = np.array([[37, 53, 0], [150, 201, 37 * 53 * 3]])
    windows = np.array([[5, 13, 32, 40], [0, 0, 150, 201]])
    for feather in (0, 8, 32):
        table, chunks, bands, lds = inpaint.build_paste_table(shapes, windows, R, feather)
        desc = table[:2 * inpaint.DESC_INTS].reshape(2, inpaint.DESC_INTS)
        assert table.dtype == np.int32 and lds <= inpaint.LDS_BYTES and lds % 16 == 0
        assert desc[1, 3] == 37 * 53                                           # the masks lie back to back
        for (h, w, off, moff, y0, x0, ch, cw, hb, hk, KH, vb, vk, KV, TB, CW) in desc:
            assert max(hb + 2 * cw, hk + cw * KH, vb + 2 * ch, vk + ch * KV) <= table.size
            assert chunks >= -(-cw // CW) and bands >= -(-ch // TB)
            hbounds = table[hb:hb + 2 * cw].reshape(cw, 2)
            assert np.all(hbounds[:, 0] + hbounds[:, 1] <= R)
            wts = table[hk:hk + cw * KH].view(np.float32).reshape(cw, KH)
            assert np.array_equal(wts, inpaint.bicubic_weights(R, cw)[1].astype(np.float32))
    table, chunks, bands, lds = inpaint.build_gather_table(shapes, windows, R)
    assert table.dtype == np.int32 and 12 <= lds <= inpaint.LDS_BYTES and chunks >= 1 and bands >= 1
    with pytest.raises(ValueError, match='image 1'):
        inpaint.build_paste_table(shapes, np.array([[5, 13, 32, 40], [0, 0, 151, 201]]), R, 8)
    with pytest.raises(ValueError, match='image 1.*do not fit'):                 # an extreme downscale on the way back
        inpaint.build_paste_table(np.array([[40, 40, 0], [2, 300, 4800]]), np.array([[0, 0, 40, 40], [0, 0, 2, 300]]), 2048, 8)
    with pytest.raises(ValueError, match='feather'):
        inpaint.build_paste_table(shapes, windows, R, 33)


def test_pack_masks():
    masks = [np.array([[1, 0, 7]], np.uint8), np.array([[True], [False]])]
    packed, offs = inpaint.pack_masks(masks)
    assert packed.dtype == torch.uint8 and packed.tolist() == [1, 0, 1, 1, 0] and offs.tolist() == [0, 3]


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    p = ctypes.c_void_p(4096)

    def gather(src=p, mask=p, table=p, dst=p, mdst=p, B=1, Rr=16, chunks=1, bands=1, lds=1024):          # (every call fails a check: nothing is launched)
        return lib.shg_inpaint_gather_u8(src, 4096, mask, 4096, table, 4096, dst, mdst, B, Rr, chunks, bands, lds, None)

    def paste(out=p, mask=p, table=p, fake=p, B=1, K=1, Rr=16, feather=8, chunks=1, bands=1, lds=1024):
        return lib.shg_inpaint_paste_u8(out, 4096, mask, 4096, table, 4096, fake, None, B, K, Rr, feather, chunks, bands, lds, None)
    for kw in (dict(src=None), dict(mask=None), dict(table=None), dict(dst=None), dict(mdst=None)):
        assert gather(**kw) == -1 and 'null' in err(), kw
    for kw in (dict(out=None), dict(mask=None), dict(table=None), dict(fake=None)):
        assert paste(**kw) == -1 and 'null' in err(), kw
    assert gather(Rr=0) == -1 and 'R must' in err() and paste(Rr=0) == -1 and 'R must' in err()
    assert paste(K=0) == -1 and 'K must' in err()
    for f in (-1, 33):
        assert paste(feather=f) == -1 and 'feather' in err()
    assert gather(B=0) == -1 and paste(B=0) == -1 and 'B must' in err()
    assert gather(lds=49153) == -1 and paste(lds=49153) == -1 and 'lds_bytes' in err()
    assert gather(B=300) == -1 and 'descriptors' in err() and paste(B=300) == -1 and 'descriptors' in err()


# ------------------------------------------------------------------------------------------------
# Inpainter on the host
# ------------------------------------------------------------------------------------------------

class StandInG:
    """A generator of nothing: the image channels of x scaled, plus a z-dependent offset -- enough to tell samples and images apart."""
    z_dim, c_dim = 4, 0

    def __init__(self):
        self.calls = []

    def __call__(self, x, z, c, noise_mode='const'):
        self.calls.append(('single', x.shape[0], noise_mode))
        assert c.shape == (x.shape[0], 0)
        return x[:, 1:] * 0.5 + z[:, :1, None, None] * 0.2

    def sample_many(self, x, z, c=None, noise_mode='random'):
        self.calls.append(('many', x.shape[0], z.shape[1]))
        return x[:, None, 1:] * 0.5 + z[:, :, :1, None, None] * 0.2


def _gather_ref(packed, packed_mask, shapes, windows, Rr):
    pk, pm = packed.numpy(), packed_mask.numpy()
    real, mask = [], []
    for (h, w, off, moff), window in zip(shapes, windows):
        r, m = ref.gather_reference(pk[off:off + 3 * h * w].reshape(h, w, 3), pm[moff:moff + h * w].reshape(h, w), tuple(window), Rr)
        real.append(r)
        mask.append(m[None])
    return torch.from_numpy(np.stack(real)), torch.from_numpy(np.stack(mask))


def _paste_ref(packed, packed_mask, shapes, windows, fake, k=1, feather=8):
    pk, pm, fake = packed.numpy(), packed_mask.numpy(), fake.numpy()
    out = np.stack([pk] * k)
    for n, ((h, w, off, moff), window) in enumerate(zip(shapes, windows)):
        for j in range(k):
            res = ref.paste_reference(pk[off:off + 3 * h * w].reshape(h, w, 3), pm[moff:moff + h * w].reshape(h, w), tuple(int(v) for v in window),
                                      fake[n * k + j], feather, np.float32)[0]
            out[j, off:off + 3 * h * w] = res.reshape(-1)
    return torch.from_numpy(out)


def test_inpainter_on_the_host_with_reference_functions():
    rng = np.random.RandomState(4)
    sizes = [(37, 53), (20, 20), (9, 70), (33, 35), (64, 40)]
    images = [ref.random_image(rng, h, w) for h, w in sizes]
    masks = [ref.mask_with_holes(37, 53, [(10, 18, 11, 29)]), np.ones((20, 20), np.uint8), ref.mask_with_holes(9, 70, [(2, 5, 30, 41)]),
             ref.mask_with_holes(33, 35, [(16, 17, 17, 18)]), ref.mask_with_holes(64, 40, [(0, 5, 30, 40)])]
    G = StandInG()
    inp = inpaint.Inpainter(G, R, 'cpu', feather=2, batch=2, gather_fn=_gather_ref, paste_fn=_paste_ref)
    z = torch.from_numpy(rng.standard_normal((5, 3, 4)).astype(np.float32))
    res = inp(images, masks, z=z[:, 0])
    assert G.calls == [('single', 2, 'const'), ('single', 2, 'const')]          # four holed images in chunks of two; the hole-free one never sent
    assert np.array_equal(res[1], images[1]) and res[1] is not images[1]
    for i in (0, 2, 3, 4):                                                      # order kept: each result is its own image outside the hole's band
        window = inpaint.plan_window(masks[i], R, 0.5, 2)
        alone = inpaint.Inpainter(StandInG(), R, 'cpu', feather=2, gather_fn=_gather_ref, paste_fn=_paste_ref)([images[i]], [masks[i]], z=z[i:i + 1, 0])[0]
        assert res[i].shape == images[i].shape and res[i].dtype == np.uint8 and np.array_equal(res[i], alone)
        A = ref.feather_reference(masks[i][window[0]:window[0] + window[2], window[1]:window[1] + window[3]], 2)
        keep = np.ones(sizes[i], bool)
        keep[window[0]:window[0] + window[2], window[1]:window[1] + window[3]] = A == 0
        assert np.array_equal(res[i][keep], images[i][keep]) and not np.array_equal(res[i], images[i])
    G.calls.clear()
    res3 = inp(images, masks, z=z, samples=3)
    assert G.calls == [('many', 2, 3), ('many', 2, 3)]
    assert [r.shape for r in res3] == [(3,) + im.shape for im in images]
    assert np.array_equal(res3[1], np.stack([images[1]] * 3))
    for i in (0, 2, 3, 4):
        assert np.array_equal(res3[i][0], res[i])                              # sample 0 drew z[:, 0]
        assert not np.array_equal(res3[i][0], res3[i][1]) and not np.array_equal(res3[i][1], res3[i][2])
    # without z: seeded per image, independent of the chunking
    a = inp(images, masks, seed=3)
    b = inpaint.Inpainter(StandInG(), R, 'cpu', feather=2, batch=16, gather_fn=_gather_ref, paste_fn=_paste_ref)(images, masks, seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    n_calls = len(G.calls)
    assert np.array_equal(inp([images[1]], [masks[1]])[0], images[1]) and len(G.calls) == n_calls
    with pytest.raises(ValueError):
        inp(images, masks[:2])
    with pytest.raises(ValueError):
        inp(images, masks, z=z[:2])
