"""Host side of the random-scale crop training input (resize.randcrop_reference, datasets.draw_scale_crop / Texture / the 'adv'
formatters, collate_ragged's crop, the C entry points' argument checks) against tests/golden/randcrop.npz -- the reference's own
formatters, tools/gen_golden_randcrop.py -- live torch and the float64 restatement of tests/randcrop_f64.py.  No GPU."""
import ctypes
import os

import numpy as np
import numpy.random as npr
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import _lib, datasets as dsx, resize as rz

import randcrop_f64 as ref


@pytest.fixture(scope='module')
def gold():
    g = load_golden('randcrop')
    n = len(g['datasets'])
    return {'s': int(g['s']), 'cases': [dict(ds=str(g['datasets'][i]), seed=int(g['cases'][i][2]), img=g[f'in{i}'], loaded=g[f'loaded{i}'],
                                             params=tuple(int(v) for v in g[f'params{i}']), x=g[f'x{i}'], mask=g[f'mask{i}'])
                                        for i in range(n)]}


def _check(name, got, img, s, params, stats=None):
    """got within 2 E_ref + 2^-22 of the float64 restatement (the bound of randcrop_f64.py); prints the figures first."""
    lim, e_ref, f64 = ref.bound(img, s, params)
    dev = float(np.abs(np.asarray(got, np.float64) - f64).max())
    print(f'{name}: E_ref {e_ref:.3e}  deviation {dev:.3e}  bound {lim:.3e}')
    if stats is not None:
        stats.append((e_ref, dev))
    assert got.dtype == np.float32 and got.shape == (3, s, s)
    assert dev <= lim, f'{name}: deviation {dev:.3e} from the float64 restatement exceeds 2 x {e_ref:.3e} + 2^-22'


def test_value_table_is_the_references_float32_steps():
    t = (torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255) - 0.5) * 2
    assert np.array_equal(rz.randcrop_value_table(), t.numpy()) and np.array_equal(ref.value_table(), t.numpy())


def test_reference_matches_the_fixture_x(gold):
    """the fixture's x is the reference formatter's output: it is torch's result, so it sits within E_ref of the float64 window and the
    numpy restatement within the bound of it"""
    s = gold['s']
    for i, c in enumerate(gold['cases']):
        f64 = ref.window_f64(c['loaded'], s, c['params'])
        live = ref.window_torch(c['loaded'], s, c['params'])
        e_fix = float(np.abs(c['x'].astype(np.float64) - f64).max())
        lim, e_ref, _ = ref.bound(c['loaded'], s, c['params'], f64)
        print(f'case {i} ({c["ds"]}): fixture vs f64 {e_fix:.3e}, live torch vs f64 {e_ref:.3e}')
        assert e_fix <= lim                                     # the recorded x and this machine's torch agree to the same bound
        assert float(np.abs(c['x'] - live).max()) <= lim
        _check(f'case {i}', rz.randcrop_reference(c['loaded'], s, c['params']), c['loaded'], s, c['params'])


def test_reference_matches_live_interpolate_on_fuzz_cases():
    stats = []
    for i, (img, s, params) in enumerate(ref.fuzz_cases()):
        _check(f'fuzz {i} {img.shape[:2]} s={s} {params}', rz.randcrop_reference(img, s, params), img, s, params, stats)
    print('largest E_ref %.3e, largest deviation %.3e' % (max(e for e, _ in stats), max(d for _, d in stats)))


@pytest.mark.parametrize('fv,fh', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_reference_identity_is_bit_exact(fv, fh):
    img = ref.synthetic_image(np.random.RandomState(3), 21, 34)
    want = ref.value_table()[img].transpose(2, 0, 1)[:, 2:18, 5:21]
    want = want[:, ::-1] if fv else want
    want = want[:, :, ::-1] if fh else want
    got = rz.randcrop_reference(img, 16, (21, 34, 2, 5, fv, fh))
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_reference_rejects_bad_windows():
    img = np.zeros((8, 8, 3), np.uint8)
    for s, params in [(0, (8, 8, 0, 0, 0, 0)), (9, (8, 9, 0, 0, 0, 0)), (4, (8, 8, 5, 0, 0, 0)), (4, (8, 8, 0, -1, 0, 0))]:
        with pytest.raises(ValueError):
            rz.randcrop_reference(img, s, params)


def test_draw_scale_crop_makes_the_references_draws(gold):
    s = gold['s']
    for c in gold['cases']:
        oh, ow = c['loaded'].shape[:2]
        npr.seed(c['seed'])
        assert dsx.draw_scale_crop(oh, ow, s, flips=c['ds'] == 'texture') == c['params']
    npr.seed(5)
    a = dsx.draw_scale_crop(40, 50, 32, flips=False)
    assert a[4:] == (0, 0) and 32 <= a[0] <= 40 and 32 <= a[1] <= 50 and a[2] <= a[0] - 32 and a[3] <= a[1] - 32
    with pytest.raises(ValueError):
        dsx.draw_scale_crop(10, 10, 0)


def test_items_carry_the_references_parameters_and_mask_bits(tmp_path, gold):
    for name, (ds, idx) in ref.make_trees(tmp_path, gold).items():
        assert len(ds) == len(idx)
        for k, i in enumerate(idx):
            c = gold['cases'][i]
            npr.seed(c['seed'])
            item = ds[k]
            assert np.array_equal(item['image'], c['img']) and item['flip'] is False
            assert tuple(item['crop']) == c['params'], (name, i)
            assert np.array_equal(np.asarray(item['mask']).astype(np.uint8), c['mask']), (name, i)
            assert bool(item.get('preresize', False)) == (name != 'texture')
        batch = dsx.collate_ragged([ds[k] for k in range(len(idx))])
        assert batch.crop.dtype == torch.int32 and tuple(batch.crop.shape) == (len(idx), 6) and batch.preresize == (name != 'texture')
        assert batch.fit == (name == 'openimages') and not bool(batch.flip.any()) and batch.masks.shape == (len(idx), gold['s'], gold['s'])


def test_the_loaders_resize_feeds_the_adv_window(gold):
    """Places2 / OpenImages: the formatter sees the loader's R x R output, which the existing host references reproduce from the file"""
    s = gold['s']
    for c in gold['cases']:
        if c['ds'] == 'places2':
            assert np.array_equal(rz.resize_reference(c['img'], s).transpose(1, 2, 0), c['loaded'])
        elif c['ds'] == 'openimages':
            assert np.array_equal(rz.fit_reference(c['img'], s).transpose(1, 2, 0), c['loaded'])
        else:
            assert np.array_equal(c['img'], c['loaded'])


def test_texture_lists_modes_and_mixed_order(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'dtd', 'labels'))
    lists = {'train1': ['banded/banded_0002.jpg', 'banded/banded_0005.jpg', 'dotted/dotted_0001.jpg', 'banded/banded_0009.jpg'],
             'val1': ['zigzagged/zigzagged_0003.jpg', 'dotted/dotted_0007.jpg'], 'anything': ['woven/woven_0001.jpg']}
    for name, lines in lists.items():
        with open(os.path.join(root, 'dtd', 'labels', name + '.txt'), 'w') as f:
            f.write(''.join(li + ' \n' for li in lines))                       # trailing blanks are stripped, as the reference strips
    info = dsx.texture_list(root, 'train1')
    assert [e['unique_id'] for e in info] == ['banded_0002', 'banded_0005', 'banded_0009', 'dotted_0001']     # ds_base sorts by id
    assert info[3]['texture_type'] == 'dotted' and info[3]['filename'] == 'dotted_0001.jpg' and [e['idx'] for e in info] == [0, 1, 2, 3]
    assert info[3]['image_path'] == os.path.join(root, 'dtd', 'images', 'dotted', 'dotted_0001.jpg')
    both = dsx.texture_list(root, 'train1+val1')
    assert [e['unique_id'] for e in both] == ['banded_0002', 'banded_0005', 'banded_0009', 'dotted_0001', 'dotted_0007', 'zigzagged_0003']
    assert [e['unique_id'] for e in dsx.texture_list(root, 'anything')] == ['woven_0001']         # the mode check never raises
    mixed = dsx.texture_list(root, 'train1+val1', mixed_order=True)
    assert [e['unique_id'] for e in mixed] == ['00000_banded_0002', '00001_dotted_0001', '00002_zigzagged_0003', '00003_banded_0005',
                                                '00004_dotted_0007', '00005_banded_0009']
    with pytest.raises(FileNotFoundError):
        dsx.texture_list(root, 'train2')

    rs = np.random.RandomState(0)
    for e in both:
        ref.write_png(e['image_path'].replace('.jpg', '.png'), rs.randint(0, 256, (11, 17, 3)).astype(np.uint8))
        os.rename(e['image_path'].replace('.jpg', '.png'), e['image_path'])    # PNG bytes under the list's name: Pillow sniffs the content
    ds = dsx.Texture(root, 'train1+val1', 16, (0.0, 1.0), mixed_order=True, try_sample=4, repeat=2)
    assert len(ds) == 8
    npr.seed(1)
    item = ds[5]
    assert item['unique_id'] == '00001_dotted_0001' and item['image'].shape == (11, 17, 3) and 'mask' not in item
    npr.seed(1)
    assert tuple(item['crop']) == dsx.draw_scale_crop(11, 17, 16, flips=True)
    assert dsx.texture_train_256.__doc__ and dsx.texture_train_512.__doc__
    assert dsx.places2_train256_adv_inpainting.__doc__ and dsx.places2_train512_adv_inpainting.__doc__ and dsx.openimages_train_1024_adv.__doc__


def test_collate_without_crop_is_unchanged_and_mixing_raises():
    a = {'image': np.zeros((4, 5, 3), np.uint8), 'flip': True, 'unique_id': 'a'}
    b = {'image': np.ones((3, 2, 3), np.uint8), 'flip': False, 'unique_id': 'b', 'crop': (4, 4, 0, 0, 0, 1)}
    plain = dsx.collate_ragged([a, dict(a, unique_id='c')])
    assert plain.crop is None and plain.preresize is False and not plain.fit and plain.ids == ['a', 'c']
    got = dsx.collate_ragged([b, dict(b, crop=(5, 6, 1, 2, 1, 0))])
    assert got.crop.tolist() == [[4, 4, 0, 0, 0, 1], [5, 6, 1, 2, 1, 0]] and got.preresize is False
    with pytest.raises(ValueError):
        dsx.collate_ragged([a, b])
    with pytest.raises(ValueError):
        dsx.collate_ragged([b, dict(b, preresize=True)])
    with pytest.raises(ValueError):
        dsx.Places2('/nonexistent', 'val', formatter='lama')


def test_device_feeder_without_crop_is_unchanged_on_the_cpu_path():
    feeder = dsx.DeviceFeeder('cpu', resolution=8)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(-1, 1, (2, 3, 8, 8)).astype(np.float32))
    m = torch.from_numpy((rs.uniform(size=(2, 8, 8)) > 0.5).astype(np.float32))
    xd, md, ids, ev, boxes = feeder._stage((x, m, ['a', 'b']))
    assert torch.equal(xd, x) and torch.equal(md[:, 0], m) and ids == ['a', 'b'] and ev is None and boxes is None
    item = {'image': np.zeros((4, 5, 3), np.uint8), 'flip': False, 'unique_id': 'a', 'crop': (8, 8, 0, 0, 0, 0)}
    with pytest.raises(ValueError):                                # ragged batches, with or without crop, have no host path
        feeder._stage(dsx.collate_ragged([item]))


@pytest.mark.parametrize('name', ['shg_randcrop_bicubic_ragged_f32', 'shg_randcrop_bicubic_planar_f32'])
def test_c_entry_points_validate_their_arguments_without_a_gpu(name):
    lib = _lib.get_lib()
    f = getattr(lib, name)
    P = ctypes.c_void_p(256)

    def call(desc, src=P, nbytes=3 * 20 * 30, dd=P, lut=P, dst=P, B=1, s=8):
        d = None if desc is None else (ctypes.c_int * len(desc))(*desc)
        return f(src, nbytes, d, dd, lut, dst, B, s, None), lib.shg_last_error()

    good = [20, 30, 0, 10, 12, 2, 4, 0, 1]
    for kw in (dict(src=None), dict(dd=None), dict(lut=None), dict(dst=None)):
        rc, msg = call(good, **kw)
        assert rc == -1 and b'null' in msg
    rc, msg = call(None)
    assert rc == -1 and b'null' in msg
    for bad, word in [(dict(s=0), b's must'), (dict(s=-3), b's must'), (dict(B=0), b'B must'), (dict(nbytes=2), b'src_bytes'),
                      (dict(nbytes=1 << 31), b'src_bytes')]:
        rc, msg = call(good, **bad)
        assert rc == -1 and word in msg, (bad, msg)
    for i, v, word in [(0, 0, b'h and w'), (1, -1, b'h and w'), (2, -1, b'outside src'), (2, 1, b'outside src'), (3, 7, b'>= s'),
                       (4, 7, b'>= s'), (5, 3, b'window'), (5, -1, b'window'), (6, 5, b'window'), (6, -1, b'window'), (7, 2, b'flip'),
                       (8, -1, b'flip'), (3, (1 << 20) + 1, b'<=')]:
        desc = list(good)
        desc[i] = v
        rc, msg = call(desc)
        assert rc == -1 and word in msg, (i, v, msg)
    rc, msg = call(good + [20, 30, 1, 10, 12, 2, 4, 0, 0], B=2)          # the second image runs past src
    assert rc == -1 and b'image 1' in msg
    with pytest.raises(_lib.ShgError):
        rz.randcrop_bicubic(torch.zeros(12, dtype=torch.uint8), [[2, 2, 0]], 2, [[2, 2, 0, 0, 0, 0]])


def test_abi_version_and_symbols():
    lib = _lib.get_lib()
    assert lib.shg_abi_version() == 40 and _lib.ABI_VERSION == 40
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'shgan_hip.h')).read()
    for name in ('shg_randcrop_bicubic_ragged_f32', 'shg_randcrop_bicubic_planar_f32'):
        assert name + '(' in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert rz.randcrop_desc([[4, 5, 0], [2, 3, 60]], [[8, 8, 0, 0, 0, 1], [9, 9, 1, 1, 1, 0]]).tolist() == \
        [[4, 5, 0, 8, 8, 0, 0, 0, 1], [2, 3, 60, 9, 9, 1, 1, 1, 0]]
