"""LaMa thin / medium / thick masks (reference: lib/data_factory/lama_mask_utils.py behind ``LamaMaskFormatter``, ds_ffhq.py:352-381), the
host half.  Three pins: the DRAWS against the reference's own generator (tests/golden/lama_masks.npz: its ``cv2.line`` calls recorded
through a stand-in, tools/gen_golden_lama.py), the RASTERISER against the restatement of OpenCV's thick line (tests/lama_cv_ref.py), and
a geometric condition that holds whatever the restatement's details: every pixel within t/2 - 0.5 of the segment is painted, none
beyond t/2 + 1.5.  The comparison with ``cv2`` itself runs only where ``cv2`` imports; if it ever fails, the restatement is what gets
corrected."""
import os
import re

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
import lama_cv_ref as cv
from conftest import load_golden
from shgan_amd import _lib, data, datasets, masks

SETTINGS = [(kind, res) for res in (256, 512) for kind in ('thin', 'medium', 'thick')]


def golden_calls(g, key, i):
    o = g['offs_' + key]
    return g['calls_' + key][o[i]:o[i + 1]]


def golden_painted(g, key, i, s):
    """Painted pixels of golden mask i: its box mask OR the restatement's composite of its recorded line calls."""
    box = np.unpackbits(g['boxes_' + key][i])[: s * s].reshape(s, s)
    return box | cv.draw(golden_calls(g, key, i), s)


@pytest.fixture(scope='module')
def golden_masks():
    """{(kind, res): uint8 [24, s, s] painted} -- computed once, shared, left unchanged."""
    g = load_golden('lama_masks')
    return {(kind, res): np.stack([golden_painted(g, f'{kind}{res}', i, res) for i in range(24)]) for kind, res in SETTINGS}


@pytest.mark.parametrize('kind,res', SETTINGS)
def test_draws_equal_the_reference_generator(kind, res):
    """Every ``cv2.line`` call, every box mask, every flip decision and the RNG state afterwards, for the seed of the golden file."""
    g = load_golden('lama_masks')
    key = f'{kind}{res}'
    np.random.seed(int(g['seed']) + [f'{k}{r}' for r in (256, 512) for k in ('thin', 'medium', 'thick')].index(key))
    setting = masks.LAMA_SETTINGS[(kind, res)]
    for i in range(24):
        assert int(np.random.rand() < 0.5) == int(g['flips_' + key][i]), i        # the formatter's flip draw comes first
        rec = masks.lama_mask_records(res, setting)
        assert rec.dtype == np.int32 and rec.shape[1] == 8
        lines = rec[rec[:, 0] == masks.LAMA_LINE]
        assert np.array_equal(lines[:, 1:6], golden_calls(g, key, i)), (key, i)
        box = np.zeros((res, res), np.uint8)
        for _, x0, x1, y0, y1, *_ in rec[rec[:, 0] == masks.LAMA_RECT].tolist():
            box[y0:y1, x0:x1] = 1
        assert np.array_equal(np.packbits(box.reshape(-1)), g['boxes_' + key][i]), (key, i)
        assert len(lines) == 0 or not box.any()                                   # one generator per mask
    assert int(np.random.randint(2 ** 31)) == int(g['witness_' + key])
    assert list(g['argtypes']) == ['int32']                                       # the reference hands cv2 numpy int32 end points


def test_golden_covers_what_the_issue_observed():
    g = load_golden('lama_masks')
    calls = np.concatenate([g[f'calls_{k}{r}'] for k, r in SETTINGS])
    assert calls[:, 4].min() == 5 and calls[:, 4].max() == 254
    assert (calls[:, :4].max() == 512) and calls[:, :4].min() == 0                # end points one past the canvas occur
    assert ((calls[:, 0] == calls[:, 2]) & (calls[:, 1] == calls[:, 3])).any()    # zero-length segments occur


@pytest.mark.parametrize('kind,res', SETTINGS)
def test_host_path_equals_the_restatement_on_the_golden_calls(kind, res, golden_masks):
    g = load_golden('lama_masks')
    key = f'{kind}{res}'
    np.random.seed(int(g['seed']) + SETTINGS.index((kind, res)))
    for i in range(24):
        np.random.rand()
        m = data.LamaMask(res, kind)
        assert m.dtype == np.float32 and m.shape == (1, res, res)
        assert np.array_equal(1 - m[0].astype(np.uint8), golden_masks[(kind, res)][i]), (key, i)


def test_capsule_condition_on_800_segments():
    """d = distance of a pixel centre to the segment: painted wherever d <= t/2 - 0.5, never where d > t/2 + 1.5.  No case excluded.
    The host path paints the same pixels as the restatement on each of them."""
    worst_out, worst_in = 0.0, np.inf
    for s, x0, y0, x1, y1, t in cv.random_segments():
        img = cv.draw([(x0, y0, x1, y1, t)], s)
        d = cv.capsule_distance(s, (x0, y0), (x1, y1))
        assert img[d <= t / 2 - 0.5].all(), (s, x0, y0, x1, y1, t)
        assert not img[d > t / 2 + 1.5].any(), (s, x0, y0, x1, y1, t)
        if img.any():
            worst_out = max(worst_out, float((d[img == 1] - t / 2).max()))
        if not img.all():
            worst_in = min(worst_in, float((d[img == 0] - t / 2).min()))
        host = masks.lama_draw_host(np.array([[masks.LAMA_LINE, x0, y0, x1, y1, t, 0, 0]], np.int32), s)
        assert np.array_equal(host, img), (s, x0, y0, x1, y1, t)
    print(f'farthest painted pixel: t/2 + {worst_out:.3f}; nearest unpainted: t/2 + {worst_in:.3f}')


def test_zero_length_segment_is_two_circles():
    for t, (x, y) in ((5, (10, 12)), (8, (0, 0)), (33, (64, 64)), (40, (63, 1)), (254, (30, 30))):
        want = np.zeros((64, 64), np.uint8)
        cv.circle(want, x, y, (t + 1) >> 1)
        assert np.array_equal(cv.draw([(x, y, x, y, t)], 64), want)
        assert np.array_equal(masks.lama_draw_host(np.array([[1, x, y, x, y, t, 0, 0]], np.int32), 64), want)


def test_circle_table_is_symmetric_and_equals_the_walk():
    tab = masks.lama_circle_table()
    assert tab.shape == (513, 513) and tab.dtype == np.int32
    for r in (0, 1, 2, 3, 7, 20, 53, 127, 512):
        n = 2 * r + 3
        img = np.zeros((n, n), np.uint8)
        cv.circle(img, r + 1, r + 1, r)
        assert np.array_equal(img, img.T) and np.array_equal(img, img[::-1]) and np.array_equal(img, img[:, ::-1])
        assert not img[0].any() and not img[:, 0].any() and img[1, r + 1] and img[r + 1, 1]
        hw = tab[r, :r + 1]
        assert (hw >= 0).all() and (tab[r, r + 1:] == -1).all()
        assert np.array_equal(img[r + 1:r + 2 + r].sum(axis=1), 2 * hw + 1)      # rows 0 .. r below the centre


def test_segment_off_canvas_paints_nothing():
    for rec in ([1, -300, -300, -200, -250, 9, 0, 0], [1, 200, 30, 260, 50, 20, 0, 0], [1, 10, 300, 50, 290, 40, 0, 0],
                [1, -40, 10, -40, 10, 12, 0, 0]):
        assert not masks.lama_draw_host(np.array([rec], np.int32), 64).any()
        assert not cv.draw([rec[1:6]], 64).any()


def test_refusals():
    S = masks.LAMA_SETTINGS[('medium', 256)]
    for extra in ({'segm_proba': 0.1}, {'squares_proba': 0.2}, {'superres_proba': 0.5}, {'outpainting_proba': 1}, {'invert_proba': 0.5},
                  {'squares_kwargs': {}}, {'irregular_kwargs': dict(S['irregular_kwargs'], ramp_kwargs={})}):
        with pytest.raises(_lib.ShgError):
            masks.lama_mask_records(256, dict(S, **extra))
    for t in (1, 0, -3, 1024):
        with pytest.raises(_lib.ShgError):
            masks.lama_draw_host(np.array([[1, 3, 3, 9, 9, t, 0, 0]], np.int32), 64)
    with pytest.raises(_lib.ShgError):
        masks.lama_draw_host(np.array([[2, 3, 3, 9, 9, 5, 0, 0]], np.int32), 64)          # unknown record type
    for s in (48, 1024, 16):
        with pytest.raises(_lib.ShgError):
            masks.lama_draw_host(np.zeros((0, 8), np.int32), s)
    with pytest.raises(_lib.ShgError):
        masks.lama_masks(2, 128, 'thin', device='cpu')                                    # no setting at 128
    with pytest.raises(_lib.ShgError):
        masks.lama_rasterize(np.zeros((0, 8), np.int32), [0, 0], 64, device='cpu')         # the rasteriser is the device's


def test_formatter_draws_the_flip_first_then_the_mask():
    img = ((torch.arange(256, dtype=torch.float32) + 1) / 512).expand(3, 256, 256).contiguous()
    el = {'image': img, 'unique_id': 'u7'}
    for seed in (0, 1, 2, 3):
        np.random.seed(seed)
        x, m, uid = datasets.LamaMaskFormatter(random_flip=True, resolution=256, type='medium')(el)
        after = int(np.random.randint(2 ** 31))
        np.random.seed(seed)
        flip = np.random.rand() < 0.5
        want = data.LamaMask(256, 'medium')[0]
        assert int(np.random.randint(2 ** 31)) == after and uid == 'u7'
        assert torch.equal(x, (img * 2 - 1).flip(-1) if flip else img * 2 - 1)
        assert m.shape == (256, 256) and m.dtype == np.float32 and np.array_equal(m, want) and set(np.unique(m)) <= {0.0, 1.0}
    np.random.seed(5)
    _, m, _ = datasets.LamaMaskFormatter(random_flip=False, resolution=256, type='thin')(el)       # no flip draw without random_flip
    np.random.seed(5)
    assert np.array_equal(m, data.LamaMask(256, 'thin')[0])
    for ty, res in (('thin', 128), ('huge', 256), ('lama_thin', 256), ('thick', 1024), (None, 512)):
        with pytest.raises(ValueError):
            datasets.LamaMaskFormatter(resolution=res, type=ty)


def test_mask_kind_plumbing(tmp_path):
    from PIL import Image
    with pytest.raises(ValueError):
        datasets.Places2('/nonexistent', 'val', formatter='lama')
    with pytest.raises(ValueError):
        datasets.Places2('/nonexistent', 'val', mask_kind='lama')
    with pytest.raises(ValueError):
        datasets.Places2('/nonexistent', 'val', resolution=128, mask_kind='lama_thin')
    with pytest.raises(ValueError):
        datasets.Places2('/nonexistent', 'train', formatter='adv', mask_kind='lama_thin')
    with pytest.raises(ValueError):
        datasets.DeviceFeeder('cpu', 256, mask_kind='thin')
    d = tmp_path / 'val_large'
    d.mkdir()
    rs = np.random.RandomState(2)
    for k in range(3):
        Image.fromarray(rs.randint(0, 256, size=(40 + k, 50, 3)).astype(np.uint8)).save(str(d / f'im{k}.png'))
    ds = datasets.places2_val256_inpainting_lama2(str(tmp_path), host_masks=True)
    assert ds.mask_kind == 'lama_medium' and ds.resolution == 256 and len(ds) == 3
    np.random.seed(8)
    items = [ds[k] for k in range(3)]
    np.random.seed(8)
    want = [data.LamaMask(256, 'medium')[0] for _ in range(3)]                   # random_flip is off in these configs: no flip draw
    assert all(np.array_equal(it['mask'], w) for it, w in zip(items, want))
    assert datasets.places2_val512_inpainting_lama1(str(tmp_path)).mask_kind == 'lama_thin'
    assert datasets.places2_val512_inpainting_lama3(str(tmp_path)).resolution == 512
    np.random.seed(9)
    assert 'mask' not in datasets.Places2(str(tmp_path), 'val', resolution=256)[0]            # the default path is untouched
    # DeviceFeeder on the CPU with host LaMa masks stages them unchanged
    x = torch.zeros(3, 3, 256, 256)
    m = torch.from_numpy(np.stack(want))
    feeder = datasets.DeviceFeeder('cpu', 256, mask_kind='lama_medium')
    (x4, xd, md, ids), = list(feeder([(x, m, ['a', 'b', 'c'])]))
    assert torch.equal(md[:, 0], m) and ids == ['a', 'b', 'c'] and tuple(x4.shape) == (3, 4, 256, 256)
    assert torch.equal(x4[:, 0], m - 0.5)


def test_abi_is_unchanged_and_the_symbol_is_declared():
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 == lib.shg_abi_version()
    assert hasattr(lib, 'shg_mask_lama_f32') and 'shg_mask_lama_f32' in _lib.exported_symbols()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'shgan_hip.h')).read()
    assert re.search(r'\bint\s+shg_mask_lama_f32\s*\(', hdr)
    # the host-side checks of the entry point itself, none of which reaches a launch
    rec = np.array([[1, 3, 3, 9, 9, 5, 100, 100]], np.int32)
    off = np.array([0, 1], np.int32)
    fake = 4096                                                                  # a non-null, 16-byte aligned stand-in for device memory

    def call(rec_, off_, s, mask=fake, total=1):
        return lib.shg_mask_lama_f32(rec_.ctypes.data, off_.ctypes.data, fake, fake, fake, 512, mask, fake, 1, total, s, None)
    assert call(rec, off, 48) == -1 and b'multiple of 32' in lib.shg_last_error()
    assert call(rec, off, 1024) == -1
    assert call(rec, off, 64, mask=fake + 4) == -1 and b'aligned' in lib.shg_last_error()
    assert call(rec, off, 64, mask=0) == -1 and b'null' in lib.shg_last_error()
    for t in (1, 1024):
        bad = rec.copy()
        bad[0, 5] = t
        assert call(bad, off, 64) == -1 and b'thickness' in lib.shg_last_error()
    bad = rec.copy()
    bad[0, 0] = 7
    assert call(bad, off, 64) == -1 and b'unknown type' in lib.shg_last_error()
    assert call(rec, np.array([0, 2], np.int32), 64) == -1


def test_restatement_equals_cv2_where_cv2_imports():
    """Skipped where ``cv2`` is not installed.  If it fails, the restatement (tests/lama_cv_ref.py, and with it the kernel) is wrong."""
    cv2 = pytest.importorskip('cv2')
    for s, x0, y0, x1, y1, t in cv.random_segments():
        ref = np.zeros((s, s), np.float32)
        cv2.line(ref, (np.int32(x0), np.int32(y0)), (np.int32(x1), np.int32(y1)), 1.0, t)
        assert np.array_equal(ref.astype(np.uint8), cv.draw([(x0, y0, x1, y1, t)], s)), (s, x0, y0, x1, y1, t)
