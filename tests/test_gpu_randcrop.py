"""The random-scale crop kernel (csrc/randcrop.hip) and the training input it serves, on the device: every case against the float64
restatement of tests/randcrop_f64.py within 2 x E_ref + 2^-22 (E_ref: torch's own CPU result of that case, computed live), bit
equality where the arithmetic is exact or the same (identity, batch independence, planar against ragged), and the fixture of the
reference's formatters (tests/golden/randcrop.npz) through DeviceFeeder end to end."""
import numpy as np
import numpy.random as npr
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import datasets as dsx, resize as rz

import randcrop_f64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _run(imgs, s, params):
    """ragged launch of a list of HWC images -> float32 numpy [B,3,s,s]"""
    packed, shapes = rz.pack_images(imgs)
    out = rz.randcrop_bicubic(packed.to(DEV), shapes, s, np.asarray(params, np.int64).reshape(-1, 6))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(imgs), 3, s, s)
    return out.cpu().numpy()


def _check(name, got, img, s, params, stats=None):
    lim, e_ref, f64 = ref.bound(img, s, params)
    dev = float(np.abs(got.astype(np.float64) - f64).max())
    print(f'{name}: E_ref {e_ref:.3e}  deviation {dev:.3e}  bound {lim:.3e}')
    if stats is not None:
        stats.append((e_ref, dev))
    assert np.isfinite(got).all()
    assert dev <= lim, f'{name}: deviation {dev:.3e} from the float64 restatement exceeds 2 x {e_ref:.3e} + 2^-22'
    return lim


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def gold():
    g = load_golden('randcrop')
    n = len(g['datasets'])
    return {'s': int(g['s']), 'cases': [dict(ds=str(g['datasets'][i]), seed=int(g['cases'][i][2]), img=g[f'in{i}'], loaded=g[f'loaded{i}'],
                                             params=tuple(int(v) for v in g[f'params{i}']), x=g[f'x{i}'], mask=g[f'mask{i}'])
                                        for i in range(n)]}


@pytest.mark.parametrize('name', ['texture', 'places2', 'openimages'])
def test_fixture_through_the_feeder(tmp_path, gold, name):
    """dataset -> collate_ragged -> DeviceFeeder: x within the bound of the float64 window of the loader's output and of the reference
    formatter's recorded x; host masks are the reference's bits; the generator input is cat([mask - 0.5, x * mask])"""
    s = gold['s']
    ds, idx = ref.make_trees(tmp_path, gold)[name]
    items = []
    for k, i in enumerate(idx):
        npr.seed(gold['cases'][i]['seed'])
        items.append(ds[k])
    feeder = dsx.DeviceFeeder(DEV, resolution=s, device_masks=False)
    (x4, real, mask, ids), = list(feeder([dsx.collate_ragged(items)]))
    torch.cuda.synchronize()
    assert real.dtype == torch.float32 and tuple(real.shape) == (len(idx), 3, s, s) and ids == [it['unique_id'] for it in items]
    real_h, mask_h = real.cpu().numpy(), mask.cpu().numpy()
    for k, i in enumerate(idx):
        c = gold['cases'][i]
        lim = _check(f'{name} case {i}', real_h[k], c['loaded'], s, c['params'])
        assert float(np.abs(real_h[k] - c['x']).max()) <= lim
        assert np.array_equal(mask_h[k, 0], c['mask'].astype(np.float32))
    want4 = torch.cat([mask - 0.5, real * mask], dim=1)
    assert torch.equal(x4, want4)

    # the same batch with masks drawn on the device: same x bits, masks of the right shape (no box fill on the adv formatter)
    feeder = dsx.DeviceFeeder(DEV, resolution=s, device_masks=True)
    npr.seed(7)
    (x4d, reald, maskd, _), = list(feeder([dsx.collate_ragged(items)]))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(reald.cpu().numpy()), _bits(real_h))
    md = maskd.cpu().numpy()
    assert md.shape == (len(idx), 1, s, s) and set(np.unique(md)) <= {0.0, 1.0}


@pytest.mark.parametrize('corner', ['top_left', 'bottom_right'])
def test_borders_clamp_on_all_four_sides(corner):
    img = ref.synthetic_image(np.random.RandomState(1), 9, 13)
    s, nh, nw = 32, 41, 47
    ch, cw = (0, 0) if corner == 'top_left' else (nh - s, nw - s)
    for fv, fh in ((0, 0), (1, 1)):
        params = (nh, nw, ch, cw, fv, fh)
        _check(f'border {corner} flips {fv}{fh}', _run([img], s, [params])[0], img, s, params)
    params = (s, s, 0, 0, 0, 0)                                      # nh = nw = s: the window is the whole resample, both borders at once
    _check('border whole', _run([img], s, [params])[0], img, s, params)


@pytest.mark.parametrize('h,w,nh,nw', [(150, 97, 32, 32), (93, 64, 32, 32), (96, 64, 32, 32), (100, 200, 34, 40), (60, 33, 32, 32)])
def test_downsampling(h, w, nh, nw):
    """150 x 97 -> 32 x 32 shrinks beyond 2x (16 point-sampled taps, the direct path); 93 / 96 / 100 rows sit on both sides of the
    48-source-row limit between the staged and the direct path; 60 rows stay on the staged one"""
    img = ref.synthetic_image(np.random.RandomState(h), h, w)
    params = (nh, nw, nh - 32, nw - 32, 0, 1)
    _check(f'down {h}x{w}->{nh}x{nw}', _run([img], 32, [params])[0], img, 32, params)


@pytest.mark.parametrize('fv,fh', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_identity_is_bit_exact(fv, fh):
    """nh = h, nw = w: t = 0, weights (0, 1, 0, 0) -> the table values of the source bytes themselves"""
    img = ref.synthetic_image(np.random.RandomState(3), 37, 70)
    s, ch, cw = 33, 3, 36
    want = ref.value_table()[img].transpose(2, 0, 1)[:, ch:ch + s, cw:cw + s]
    want = want[:, ::-1] if fv else want
    want = want[:, :, ::-1] if fh else want
    got = _run([img], s, [(37, 70, ch, cw, fv, fh)])[0]
    assert np.array_equal(_bits(got), _bits(want))


def test_unaligned_ragged_batch_is_batch_independent():
    """widths 5, 7 and 33: byte offsets and row lengths that are no multiple of 4; one launch and one image at a time give the same bits"""
    rs = np.random.RandomState(5)
    imgs = [ref.synthetic_image(rs, 6, 5), ref.synthetic_image(rs, 9, 7), ref.synthetic_image(rs, 11, 33)]
    s = 16
    params = [(19, 17, 2, 1, 0, 0), (16, 19, 0, 3, 1, 0), (18, 33, 1, 9, 0, 1)]
    _, shapes = rz.pack_images(imgs)
    assert [int(v) % 4 for v in shapes[:, 2]] == [0, 2, 3]
    together = _run(imgs, s, params)
    for k in range(3):
        alone = _run([imgs[k]], s, [params[k]])[0]
        assert np.array_equal(_bits(alone), _bits(together[k]))
        _check(f'ragged {k}', together[k], imgs[k], s, params[k])
    swapped = _run(imgs[::-1], s, params[::-1])
    assert np.array_equal(_bits(swapped[::-1]), _bits(together))


@pytest.mark.parametrize('s', [1, 24, 65])
def test_tile_edges(s):
    """s = 24 and 65 are multiples of neither tile side (16 rows x 64 columns): partial tiles, scalar stores at 65; s = 1"""
    img = ref.synthetic_image(np.random.RandomState(s), 50, 71)
    for params in [(s + 9, s + 14, 4, 11, 1, 1), (max(50, s), max(71, s), 0, 0, 0, 0)]:
        _check(f'tile s={s} {params}', _run([img], s, [params])[0], img, s, params)


def test_planar_source_matches_the_ragged_path():
    """the output of resize_bicubic_u8 at 64 x 64, fed as it is (planar) and as HWC bytes (ragged): the same bits"""
    rs = np.random.RandomState(9)
    imgs = [ref.synthetic_image(rs, 80, 101), ref.synthetic_image(rs, 50, 64)]
    packed, shapes = rz.pack_images(imgs)
    u8 = rz.resize_bicubic_u8(packed.to(DEV), shapes, 64)
    params = [(70, 76, 3, 10, 0, 0), (64, 64, 0, 0, 0, 0)]
    planar = rz.randcrop_bicubic(u8, None, 64, params)
    torch.cuda.synchronize()
    hwc = [np.ascontiguousarray(u8[k].permute(1, 2, 0).cpu().numpy()) for k in range(2)]
    ragged = _run(hwc, 64, params)
    assert np.array_equal(_bits(planar.cpu().numpy()), _bits(ragged))
    assert np.array_equal(_bits(ragged[1]), _bits(ref.value_table()[hwc[1]].transpose(2, 0, 1)))
    _check('planar', ragged[0], hwc[0], 64, params[0])


@pytest.mark.parametrize('s,h,w', [(256, 300, 400), (512, 600, 800)])
def test_full_size_launch_geometry(s, h, w):
    """B = 2 at the training sizes, nh = int(1.2 s): the grid of a real batch, against the float64 window and randcrop_reference (each
    within the bound of the float64 window, hence within twice the bound of each other)"""
    rs = np.random.RandomState(s)
    imgs = [ref.synthetic_image(rs, h, w), ref.synthetic_image(rs, h - 37, w - 111)]
    n = int(1.2 * s)
    params = [(n, n + 5, n - s, 3, 0, 1), (n, n, 0, n - s, 1, 0)]
    got = _run(imgs, s, params)
    for k in range(2):
        lim = _check(f'full s={s} image {k}', got[k], imgs[k], s, params[k])
        host = rz.randcrop_reference(imgs[k], s, params[k])
        d = float(np.abs(got[k] - host).max())
        print(f'  vs randcrop_reference: max diff {d:.3e}, {int((_bits(got[k]) != _bits(host)).sum())} of {host.size} values differ')
        assert d <= 2 * lim


def test_fuzz():
    stats = []
    for i, (img, s, params) in enumerate(ref.fuzz_cases()):
        _check(f'fuzz {i} {img.shape[:2]} s={s} {params}', _run([img], s, [params])[0], img, s, params, stats)
    print('largest E_ref %.3e, largest kernel deviation %.3e' % (max(e for e, _ in stats), max(d for _, d in stats)))
