"""CPU (no GPU): the host side of the OpenImages evaluation input (lib/data_factory/ds_openimages.py:20-81,148-166 with the resize and
the padding left to the device): ``resize.fit_size`` / ``fit_reference`` / ``build_fit_table``, the ``OpenImages`` dataset against the
reference's own loader + formatter (tests/golden/openimages_fit.npz), listing, collate, the host masks at 1024 and the C argument checks
of the two new entry points."""
import ctypes
import os

import numpy as np
import numpy.random as npr
import pytest
import torch
from PIL import Image

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import _lib, data, datasets, masks
from shgan_amd import resize as rz


def _pillow_fit(img, R, flip=False):
    """FixResolutionLoader + the formatter's flip, written with Pillow as the reference does (uint8 [3, R, R])."""
    im = Image.fromarray(img)
    w, h = im.size
    if w > R or h > R:
        ratio = R / w if w > h else R / h
        im = im.resize((R, int(h * ratio)) if w > h else (int(w * ratio), R), resample=Image.BICUBIC)
    canvas = np.zeros((R, R, 3), np.uint8)
    canvas[:im.size[1], :im.size[0]] = np.asarray(im)
    out = canvas.transpose(2, 0, 1)
    return np.ascontiguousarray(out[:, :, ::-1] if flip else out)


def test_fit_size_is_the_float_expression():
    """The reference's float64 expression, not h * R // w: the square sizes whose box is one column short are among the sweep."""
    short = 0
    for R in (48, 64, 256, 1024):
        for h in list(range(1, 3 * R, 7)) + [R - 1, R, R + 1, 2 * R, 1122, 8000]:
            for w in (1, 3, R // 2, R - 1, R, R + 1, h, 2 * h + 1, 4000):
                if w > R or h > R:
                    ratio = R / w if w > h else R / h
                    ww, hh = (R, int(h * ratio)) if w > h else (int(w * ratio), R)
                    if ww <= 0 or hh <= 0:
                        with pytest.raises(ValueError, match='height and width must be > 0'):
                            rz.fit_size(h, w, R)
                        continue
                    want = (hh, ww)
                else:
                    want = (h, w)
                assert rz.fit_size(h, w, R) == want, (h, w, R)
                short += h == w and want != (R, R) and h > R
    assert short > 0
    assert rz.fit_size(1122, 1122, 1024) == (1024, 1023)            # one black column, as the reference
    assert rz.fit_size(561, 1122, 1024) == (511, 1024) and 561 * 1024 // 1122 == 512
    assert rz.fit_size(644, 1288, 1024) == (511, 1024) and 644 * 1024 // 1288 == 512
    assert rz.fit_size(94, 94, 48) == (48, 47) and rz.fit_size(98, 98, 64) == (64, 63)
    n = sum(rz.fit_size(s, s, 1024) == (1024, 1023) for s in range(1025, 8001))
    assert n == 968
    with pytest.raises(ValueError, match='height and width must be > 0'):
        rz.fit_size(3000, 1, 1024)


def test_fit_reference_is_bit_identical_to_pillow():
    rs = np.random.RandomState(17)
    n = 0
    for i in range(160):
        R = int(rs.choice([48, 64, 96, 128]))
        kind = i % 5
        if kind == 0:                                          # smaller than R: pad only
            h, w = rs.randint(1, R + 1, size=2)
        elif kind == 1:                                        # landscape
            w = rs.randint(R + 1, 4 * R)
            h = rs.randint(max(1, w // 12), w + 1)
        elif kind == 2:                                        # portrait
            h = rs.randint(R + 1, 4 * R)
            w = rs.randint(max(1, h // 12), h + 1)
        elif kind == 3:                                        # square
            h = w = rs.randint(R - 2, 4 * R)
        else:                                                  # one side at R
            h, w = (R, rs.randint(1, 3 * R)) if i % 2 else (rs.randint(1, 3 * R), R)
        img = rs.randint(0, 256, size=(int(h), int(w), 3)).astype(np.uint8)
        flip = bool(rs.rand() < 0.5)
        assert np.array_equal(rz.fit_reference(img, R, flip), _pillow_fit(img, R, flip)), (h, w, R, flip)
        n += 1
    assert n == 160


def test_build_fit_table_keys_tables_by_size_pair():
    R = 64
    shapes = np.array([(98, 98, 0), (30, 200, 1), (200, 30, 2), (20, 33, 3), (98, 98, 4), (6000 // 16, 4000 // 16, 5)])
    table, chunks, bands, lds = rz.build_fit_table(shapes, R, flip=[0, 1, 0, 1, 0, 1])
    assert table.dtype == np.int32 and 12 <= lds <= rz.LDS_BYTES
    desc = table[:len(shapes) * rz.FIT_DESC_INTS].reshape(-1, rz.FIT_DESC_INTS)
    assert list(desc[:, 3]) == [0, 1, 0, 1, 0, 1]
    assert np.array_equal(desc[0, 4:10], desc[4, 4:10])                       # the same (in, out) pairs are placed once
    for (h, w, off, fl, hb, hk, kh, vb, vk, kv, tb, cw, oh, ow) in desc:
        assert (oh, ow) == rz.fit_size(h, w, R)
        assert np.array_equal(table[hb:hb + 2 * ow].reshape(ow, 2), rz.bicubic_coeffs(w, ow)[0])
        assert np.array_equal(table[hk:hk + ow * kh].reshape(ow, kh), rz.bicubic_coeffs(w, ow)[1])
        assert np.array_equal(table[vb:vb + 2 * oh].reshape(oh, 2), rz.bicubic_coeffs(h, oh)[0])
        assert np.array_equal(table[vk:vk + oh * kv].reshape(oh, kv), rz.bicubic_coeffs(h, oh)[1])
        assert -(-R // tb) <= bands and -(-R // cw) <= chunks and (cw == R or cw % 4 == 0)
        vbnd = table[vb:vb + 2 * oh].reshape(oh, 2)
        for y0 in range(0, oh, tb):
            y1 = min(y0 + tb, oh)
            span = vbnd[y1 - 1, 0] + vbnd[y1 - 1, 1] - vbnd[y0, 0]
            assert 3 * span * ((min(cw, R) + 3) // 4 * 4) <= lds
    # a pad-only image carries identity tables of its own size
    d = desc[3]
    assert tuple(d[12:]) == (20, 33) and d[6] == 1 and d[9] == 1


@pytest.mark.parametrize('h,w', [(4000, 6000), (6000, 4000), (3000, 40), (40, 3000), (8000, 8000), (1025, 1025)])
def test_fit_tiling_fits_lds_for_heavy_downscales_at_1024(h, w):
    table, chunks, bands, lds = rz.build_fit_table(np.array([(h, w, 0)]), 1024)
    assert lds <= rz.LDS_BYTES and chunks <= 1024 and bands <= 1024


def _save(path, h, w, seed, fmt='PNG'):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    img = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    Image.fromarray(img).save(path, format=fmt)
    return img


def test_items_equal_the_reference_loader_and_formatter(tmp_path):
    """Golden: the reference's FixResolutionLoader + FreeFormMaskFormatter with seeded npr.  The item's image through fit_reference with
    its flip is the formatter's canvas; the item's mask (drawn after the flip, then filled with the UNFLIPPED box) is the formatter's."""
    g = load_golden('openimages_fit')
    cases = g['cases']
    for i, (h, w, R, random_flip, seed) in enumerate(cases.tolist()):
        root = tmp_path / f'c{i}'
        d = root / 'validation'
        d.mkdir(parents=True)
        Image.fromarray(g[f'in{i}']).save(str(d / f'im{i}.png'))
        ds = datasets.OpenImages(str(root), 'val', resolution=R, random_flip=bool(random_flip), host_masks=True)
        npr.seed(seed)
        it = ds[0]
        assert np.array_equal(it['image'], g[f'in{i}'])
        assert tuple(it['content_size']) == tuple(g[f'content{i}'].tolist()), i
        assert it['flip'] == bool(g[f'flip{i}']), i
        assert np.array_equal(rz.fit_reference(it['image'], R, it['flip']), g[f'x{i}']), i
        assert np.array_equal(it['mask'].astype(np.uint8), g[f'mask{i}']), i
    # the quirk is covered: a flipped item whose box is narrower than R (content at the right edge, keep fill at the left box's right)
    quirk = [i for i in range(len(cases)) if bool(g[f'flip{i}']) and g[f'content{i}'][1] < cases[i][2]]
    assert quirk
    for i in quirk:
        R, cw = int(cases[i][2]), int(g[f'content{i}'][1])
        assert (g[f'mask{i}'][:, cw:] == 1).all() and (g[f'x{i}'][:, :, :R - cw] == 0).all()


def test_host_random_mask_records_at_1024_match_the_reference():
    """masks.mask_attempt_records at s = 1024 rasterised by the numpy oracle == the reference's RandomMask(1024) (golden, 3 seeds)."""
    from oracle import mask_raster_oracle as mo
    g = load_golden('openimages_fit')
    tab = masks.disc_span_table()
    for k, seed in enumerate(g['mask_seeds'].tolist()):
        want = np.unpackbits(g[f'rm1024_{k}'])[:1024 * 1024].reshape(1024, 1024)
        np.random.seed(seed)
        while True:                                         # the reference's rejection loop (hole_range [0, 1])
            rec, f0, f1 = masks.mask_attempt_records(1024, [0.0, 1.0])
            m = mo.rasterize(rec, f0, f1, 1024, tab)
            ratio = 1 - m.mean()
            if 0.0 < ratio < 1.0:
                break
        assert np.array_equal(m.astype(np.uint8), want), seed
        np.random.seed(seed)
        assert np.array_equal(data.RandomMask(1024, [0.0, 1.0])[0].astype(np.uint8), want), seed


def test_listing_unique_ids_sort_and_modes(tmp_path):
    """unique_id = '-'.join(subdir.split('/')[4:] + [stem]) with no main tag; sorted; 'train' -> train/, 'val' -> validation/."""
    root = str(tmp_path)
    _save(os.path.join(root, 'validation', 'b.jpg'), 20, 30, 1, 'JPEG')
    _save(os.path.join(root, 'validation', 'a.png'), 20, 30, 2)
    _save(os.path.join(root, 'validation', 'sub', 'c.jpg'), 20, 30, 3, 'JPEG')
    _save(os.path.join(root, 'train', 'z.png'), 10, 10, 4)
    with open(os.path.join(root, 'validation', 'readme.txt'), 'w') as fh:
        fh.write('x')
    parts = root.split('/')
    uid = lambda sub, stem: '-'.join((parts + sub)[4:] + [stem])      # noqa: E731
    val = datasets.openimages_list(root, 'val')
    assert [e['unique_id'] for e in val] == sorted([uid(['validation'], 'a'), uid(['validation'], 'b'), uid(['validation', 'sub'], 'c')])
    assert [e['idx'] for e in val] == [0, 1, 2] and {e['filename'] for e in val} == {'a.png', 'b.jpg', 'c.jpg'}
    tr = datasets.openimages_list(root, 'train')
    assert [e['unique_id'] for e in tr] == [uid(['train'], 'z')]
    with pytest.raises(ValueError):
        datasets.openimages_list(root, 'test')
    ds = datasets.OpenImages(root, 'val', resolution=32, try_sample=2, repeat=3)
    assert len(ds) == 6 and ds[5]['unique_id'] == ds[1]['unique_id']


def test_literal_ids_under_a_four_component_root(monkeypatch):
    walked = [('/data/x/y/oi/validation', ['k'], ['b.jpg', 'a.png', 'c.txt']), ('/data/x/y/oi/validation/k', [], ['z.jpg'])]
    monkeypatch.setattr(datasets.os, 'walk', lambda d: iter(walked) if d == '/data/x/y/oi/validation' else iter([]))
    lst = datasets.openimages_list('/data/x/y/oi', 'val')
    assert [e['unique_id'] for e in lst] == ['oi-validation-a', 'oi-validation-b', 'oi-validation-k-z']


def test_items_draw_order_constructors_and_the_bomb_check(tmp_path):
    from PIL import Image as PILImage
    root = str(tmp_path)
    _save(os.path.join(root, 'validation', 'a.png'), 90, 40, 1)
    _save(os.path.join(root, 'train', 'a.png'), 90, 40, 1)
    ds = datasets.OpenImages(root, 'val', resolution=32, random_flip=True, host_masks=True)
    npr.seed(4)
    it = ds[0]
    npr.seed(4)
    flip = npr.rand() < 0.5
    m = data.RandomMask(32, [0, 1])[0]
    m[:, 14:] = 1
    m[32:, :] = 1
    assert it['flip'] == flip and it['content_size'] == (32, 14) and np.array_equal(it['mask'], m)
    st = npr.get_state()[1].copy()
    it = datasets.OpenImages(root, 'val', resolution=32)[0]          # no flip draw, no mask draw
    assert it['flip'] is False and 'mask' not in it and np.array_equal(npr.get_state()[1], st)
    v, t = datasets.openimages_val_1024(root), datasets.openimages_train_1024(root)
    assert (v.resolution, v.random_flip, v.hole_range) == (1024, False, [0.0, 1.0])
    assert (t.resolution, t.random_flip, t.hole_range) == (1024, True, [0.0, 1.0])
    # the decompression-bomb limit is off for this decode only
    limit = PILImage.MAX_IMAGE_PIXELS
    try:
        PILImage.MAX_IMAGE_PIXELS = 100                     # 90 x 40 = 3600 > 2 x 100: Pillow would refuse it
        assert datasets.OpenImages(root, 'val', resolution=32)[0]['image'].shape == (90, 40, 3)
        assert PILImage.MAX_IMAGE_PIXELS == 100
        with pytest.raises(PILImage.DecompressionBombError):
            PILImage.open(os.path.join(root, 'validation', 'a.png'))
    finally:
        PILImage.MAX_IMAGE_PIXELS = limit
    # a box of zero pixels: Pillow's error, naming the file
    _save(os.path.join(root, 'validation', 'thin.png'), 1, 90, 2)
    with pytest.raises(ValueError, match='thin.png.*height and width must be > 0'):
        ds = datasets.OpenImages(root, 'val', resolution=32)
        ds[[e['filename'] for e in ds.load_info].index('thin.png')]


def test_collate_fit_and_content_size(tmp_path):
    root = str(tmp_path)
    for k, (h, w) in enumerate([(90, 40), (20, 20), (33, 70)]):
        _save(os.path.join(root, 'validation', f'i{k}.png'), h, w, k)
    ds = datasets.OpenImages(root, 'val', resolution=32, random_flip=True, host_masks=True)
    npr.seed(1)
    items = [ds[i] for i in range(len(ds))]
    b = datasets.collate_ragged(items)
    assert b.fit is True and b.content_size.dtype == torch.int32
    assert b.content_size.tolist() == [list(it['content_size']) for it in items] == [[32, 14], [20, 20], [15, 32]]
    assert tuple(b.masks.shape) == (3, 32, 32) and b.flip.tolist() == [it['flip'] for it in items]
    for k, it in enumerate(items):
        h, w, o = b.shapes[k].tolist()
        assert np.array_equal(b.data.numpy()[o:o + h * w * 3].reshape(h, w, 3), it['image'])
    # Places2 batches stay as they were
    p = datasets.collate_ragged([{k: v for k, v in it.items() if k != 'content_size'} for it in items])
    assert p.fit is False and p.content_size is None
    with pytest.raises(ValueError, match='mixes'):
        datasets.collate_ragged([items[0], {k: v for k, v in items[1].items() if k != 'content_size'}])
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0, collate_fn=datasets.collate_ragged)
    assert [bb.fit for bb in loader] == [True, True]


def test_fill_outside_box():
    m = np.zeros((6, 6), np.float32)
    datasets.fill_outside_box(m, (4, 3))
    want = np.ones((6, 6), np.float32)
    want[:4, :3] = 0
    assert np.array_equal(m, want)
    t = torch.zeros(2, 6, 6)
    datasets.fill_outside_box(t[1], (6, 5))
    assert t[0].sum() == 0 and t[1, :, 5].sum() == 6 and t[1].sum() == 6


def test_c_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.get_lib()
    P = ctypes.c_void_p(256)
    f = lib.shg_resize_fit_pad_u8
    assert f(None, 100, P, 100, P, 1, 64, 1, 4, 1024, None) == -1 and b'null' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 0, 64, 1, 4, 1024, None) == -1 and b'B must' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 0, 1, 4, 1024, None) == -1 and b'R must' in lib.shg_last_error()
    assert f(P, 2, P, 100, P, 1, 64, 1, 4, 1024, None) == -1 and b'src_bytes' in lib.shg_last_error()
    assert f(P, 100, P, 27, P, 2, 64, 1, 4, 1024, None) == -1 and b'descriptors of 14' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 0, 4, 1024, None) == -1 and b'chunks' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 1, 65, 1024, None) == -1 and b'bands' in lib.shg_last_error()
    assert f(P, 100, P, 100, P, 1, 64, 1, 4, 49153, None) == -1 and b'lds_bytes' in lib.shg_last_error()
    A = ctypes.c_void_p(4096)
    g = lib.shg_mask_raster_box_f32
    assert g(A, A, A, A, 32, None, A, A, 2, 1024, None) == -1 and b'null' in lib.shg_last_error()
    assert g(A, A, A, A, 32, A, None, A, 2, 1024, None) == -1 and b'null' in lib.shg_last_error()
    assert g(A, A, A, A, 32, A, A, A, 2, 1056, None) == -1 and b'[32, 1024]' in lib.shg_last_error()
    assert g(A, A, A, A, 32, A, A, A, 2, 1000, None) == -1 and b'[32, 1024]' in lib.shg_last_error()
    assert g(A, A, A, A, 32, A, ctypes.c_void_p(4100), A, 2, 1024, None) == -1 and b'aligned' in lib.shg_last_error()
    h = lib.shg_mask_raster_f32
    assert h(A, A, A, A, 32, A, A, 2, 1056, None) == -1 and b'[32, 1024]' in lib.shg_last_error()
    assert h(A, A, A, A, 32, A, A, 0, 512, None) == -1
    with pytest.raises(_lib.ShgError):
        rz.resize_fit_pad_u8(torch.zeros(12, dtype=torch.uint8), [[2, 2, 0]], 4)
    with pytest.raises(_lib.ShgError, match='1024'):
        masks.rasterize(np.zeros((0, 8), np.int32), [0, 0], [(0, 0)], 1056, device='cpu')
