"""CPU (no GPU): the Places2 dataset side (datasets.places2_list / Places2 / collate_ragged = lib/data_factory/ds_places2.py:19-77,90-103,
214-229 with the resize left to the device): listing and unique ids, modes, try_sample, the formatter's draw order, the ragged collate."""
import os

import numpy as np
import numpy.random as npr
import pytest
import torch
from PIL import Image

import shgan_amd  # noqa: F401
from shgan_amd import data, datasets


def _save(path, h, w, seed, fmt='JPEG'):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    img = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    Image.fromarray(img).save(path, format=fmt)
    return img


def _tree(root):
    _save(os.path.join(root, 'val_large', 'Places365_val_00000002.jpg'), 40, 52, 1)
    _save(os.path.join(root, 'val_large', 'Places365_val_00000001.jpg'), 33, 30, 2)
    _save(os.path.join(root, 'val_large', 'x', 'y', 'deep.png'), 20, 24, 3, 'PNG')
    _save(os.path.join(root, 'places2_small', 'val_512', 'b', 'img7.jpg'), 16, 17, 4)
    _save(os.path.join(root, 'places2_small', 'val_512', 'a.png'), 18, 16, 5, 'PNG')
    with open(os.path.join(root, 'val_large', 'notes.txt'), 'w') as fh:
        fh.write('not an image')


def test_listing_unique_ids_and_order(tmp_path):
    """unique_id = '-'.join([maintag] + subdir.split('/')[4:] + [stem]) on the path string as given; sorted by unique_id."""
    root = str(tmp_path)
    _tree(root)
    parts = root.split('/')                 # the reference's [4:] counts components of the path string as given
    uid = lambda sub, stem: '-'.join(['50val'] + (parts + sub)[4:] + [stem])      # noqa: E731
    val = datasets.places2_list(root, 'val')
    want = sorted([uid(['val_large'], 'Places365_val_00000001'), uid(['val_large'], 'Places365_val_00000002'),
                   uid(['val_large', 'x', 'y'], 'deep')])
    assert [e['unique_id'] for e in val] == want
    assert [e['idx'] for e in val] == [0, 1, 2]
    # written out literally for a root of a known depth: /<a>/<b>/<c>/<d>/...
    root2 = os.path.join(root, 'deep', 'er')
    _save(os.path.join(root2, 'places2_small', 'val_512', 'b', 'img7.jpg'), 8, 9, 6)
    _save(os.path.join(root2, 'places2_small', 'val_512', 'a.png'), 8, 9, 7, 'PNG')
    lst = datasets.places2_list(root2, 'sval512')
    base = root2.split('/')[4:]
    assert [e['unique_id'] for e in lst] == sorted(['-'.join(['52val'] + base + ['places2_small', 'val_512', 'a']),
                                                    '-'.join(['52val'] + base + ['places2_small', 'val_512', 'b', 'img7'])])
    assert [e['filename'] for e in lst] == ['a.png', 'img7.jpg']


def test_literal_ids_under_a_four_component_root(tmp_path, monkeypatch):
    """The id for a root /data/x/y/places2, written out: split('/') starts with '', so [4:] keeps 'places2' and everything below it."""
    walked = [('/data/x/y/places2/val_large', ['k'], ['b.jpg', 'a.png', 'c.txt']), ('/data/x/y/places2/val_large/k', [], ['z.jpg'])]
    monkeypatch.setattr(datasets.os, 'walk', lambda d: iter(walked) if d == '/data/x/y/places2/val_large' else iter([]))
    lst = datasets.places2_list('/data/x/y/places2', 'val')
    assert [e['unique_id'] for e in lst] == ['50val-places2-val_large-a', '50val-places2-val_large-b', '50val-places2-val_large-k-z']
    assert lst[2]['image_path'] == '/data/x/y/places2/val_large/k/z.jpg'


def test_joined_modes_try_sample_and_errors(tmp_path):
    root = str(tmp_path)
    _tree(root)
    both = datasets.places2_list(root, 'val+sval512')
    assert len(both) == 5 and [e['unique_id'] for e in both] == sorted(e['unique_id'] for e in both)
    assert sum(e['unique_id'].startswith('52val') for e in both) == 2
    ds = datasets.Places2(root, 'val+sval512', try_sample=3, repeat=2)
    assert len(ds) == 6 and ds[4]['unique_id'] == ds[1]['unique_id']
    with pytest.raises(ValueError):
        datasets.places2_list(root, 'nope')


def test_items_decode_and_draw_in_the_formatter_order(tmp_path):
    """Item = decoded uint8 HWC at its own size (convert('RGB')); the flip draw, then RandomMask, per item (FreeFormMaskFormatter)."""
    root = str(tmp_path)
    _tree(root)
    ds = datasets.Places2(root, 'val', resolution=32, random_flip=True, host_masks=True)
    npr.seed(13)
    items = [ds[i] for i in range(len(ds))]
    npr.seed(13)
    for e, it in zip(ds.load_info, items):
        flip = npr.rand() < 0.5
        m = data.RandomMask(32, [0, 1])[0]
        ref = np.asarray(Image.open(e['image_path']).convert('RGB'))
        assert it['flip'] == flip and np.array_equal(it['mask'], m) and np.array_equal(it['image'], ref) and it['image'].dtype == np.uint8
    assert items[1]['image'].shape == (40, 52, 3) and items[2]['image'].shape == (20, 24, 3)
    # val: no flip draw, no host masks by default
    npr.seed(13)
    st = npr.get_state()[1].copy()
    it = datasets.Places2(root, 'val')[0]
    assert it['flip'] is False and 'mask' not in it and np.array_equal(npr.get_state()[1], st)


def test_named_constructors(tmp_path):
    root = str(tmp_path)
    _tree(root)
    os.makedirs(os.path.join(root, 'data_challenge'))
    _save(os.path.join(root, 'data_challenge', 'q.jpg'), 10, 12, 9)
    for fn, R, flip, mode_tag in [(datasets.places2_val256_inpainting, 256, False, '50val'), (datasets.places2_val512_inpainting, 512, False, '50val'),
                                  (datasets.places2_challenge256_inpainting, 256, True, '01challenge'),
                                  (datasets.places2_challenge512_inpainting, 512, True, '01challenge')]:
        ds = fn(root)
        assert ds.resolution == R and ds.random_flip is flip and ds.hole_range == [0.0, 1.0] and ds.load_info[0]['unique_id'].startswith(mode_tag)


def test_ragged_collate_packs_bytes_and_offsets(tmp_path):
    root = str(tmp_path)
    _tree(root)
    ds = datasets.Places2(root, 'val+sval512', resolution=16, random_flip=True, host_masks=True)
    npr.seed(2)
    items = [ds[i] for i in range(len(ds))]
    batch = datasets.collate_ragged(items)
    assert isinstance(batch, datasets.RaggedU8Batch) and len(batch) == 5
    assert batch.shapes.dtype == torch.int32 and tuple(batch.shapes.shape) == (5, 3) and batch.data.dtype == torch.uint8
    off = 0
    for k, it in enumerate(items):
        h, w, o = batch.shapes[k].tolist()
        assert (h, w, o) == (it['image'].shape[0], it['image'].shape[1], off)
        assert np.array_equal(batch.data.numpy()[o:o + h * w * 3].reshape(h, w, 3), it['image'])
        off += h * w * 3
    assert batch.data.numel() == off
    assert batch.flip.tolist() == [it['flip'] for it in items] and batch.ids == [it['unique_id'] for it in items]
    assert tuple(batch.masks.shape) == (5, 16, 16) and np.array_equal(batch.masks[3].numpy(), items[3]['mask'])
    nomask = datasets.collate_ragged([{k: v for k, v in it.items() if k != 'mask'} for it in items])
    assert nomask.masks is None
    # the DataLoader route
    npr.seed(2)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, collate_fn=datasets.collate_ragged)
    got = list(loader)
    assert [len(b) for b in got] == [2, 2, 1] and sum((b.ids for b in got), []) == batch.ids
    assert torch.equal(torch.cat([b.data for b in got]), batch.data)


def test_device_feeder_refuses_ragged_batches_on_the_host(tmp_path):
    root = str(tmp_path)
    _tree(root)
    ds = datasets.Places2(root, 'val', resolution=16)
    batch = datasets.collate_ragged([ds[0], ds[1]])
    with pytest.raises(ValueError, match='HIP device'):
        list(datasets.DeviceFeeder('cpu', 16, device_masks=True)([batch]))
