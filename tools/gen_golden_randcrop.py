#!/usr/bin/env python3
"""Golden vectors of the "random scale, random crop" training formatters: runs the reference's own ``InpaintingFormatter``
(lib/data_factory/ds_texture.py:121-149) and the two ``AdvInpaintingFormatter`` (ds_places2.py:183-207, ds_openimages.py:117-141) behind
their loaders on the CPU and writes tests/golden/randcrop.npz (data only: inputs, the drawn parameters and the reference's outputs).

Per case, at s = 32 and from a seeded numpy RNG: the source image (a small synthetic PNG of its own size), the seed, the loader's output
as uint8 codes (the image itself for DTD, the R x R resize / padded canvas for Places2 / OpenImages), the formatter's draws
(nh, nw, ch, cw, flip_v, flip_h) -- replayed here from the same seed with the formatter's own calls -- and its ``x`` (float32) and mask.

The reference imports ``torchvision.transforms`` for ``ToTensor``, which is not installed here: a stub with the same uint8 -> float / 255
conversion stands in; ``cv2`` / ``pyspng`` / ``lib.visual_service`` are stubbed as in tools/gen_golden.py and tools/gen_golden_openimages.py
(never called on these paths).

Runs ONLY where the reference tree exists; nothing here is imported by the product or by the tests.

Usage:  python tools/gen_golden_randcrop.py
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SHGAN_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'randcrop.npz')

import torch  # noqa: E402


def _to_tensor(pic):
    a = np.asarray(pic)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)


for _name in ['torchvision', 'torchvision.models', 'torchvision.transforms', 'pyspng', 'cv2', 'lib.visual_service']:
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['torchvision'].models = sys.modules['torchvision.models']
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
sys.modules['torchvision.transforms'].ToTensor = lambda: _to_tensor
if not hasattr(torch.functional, 'align_tensors'):          # ds_texture.py:6 imports it and never uses it
    torch.functional.align_tensors = None
sys.path.insert(0, REF)

from PIL import Image  # noqa: E402

import lib  # noqa: E402
lib.visual_service = sys.modules['lib.visual_service']

from lib.data_factory import ds_openimages, ds_places2, ds_texture  # noqa: E402

S = 32
# (dataset, h, w, seed): DTD images keep their size (smaller than s, between s and 1.2 s, larger; both orientations; shrinking beyond
# 2x); Places2 / OpenImages images go through the loader's resize to S x S first
CASES = [
    ('texture', 40, 52, 1), ('texture', 9, 13, 2), ('texture', 70, 30, 3), ('texture', 36, 33, 4), ('texture', 150, 97, 5),
    ('texture', 32, 32, 6),
    ('places2', 45, 60, 11), ('places2', 32, 32, 12), ('places2', 20, 77, 13),
    ('openimages', 48, 64, 21), ('openimages', 20, 25, 22), ('openimages', 90, 40, 23),
]


def _draws(oh, ow, s, flips):
    """the formatter's calls (ds_texture.py:138-147), to read the parameters it drew back from the same seed"""
    npr = np.random
    nh = npr.randint(s, max(oh, int(s * 1.2)) + 1)
    nw = npr.randint(s, max(ow, int(s * 1.2)) + 1)
    ch, cw = npr.randint(0, nh - s + 1), npr.randint(0, nw - s + 1)
    fv = fh = False
    if flips:
        fv = npr.random() < 0.5
        fh = npr.random() < 0.5
    return [nh, nw, ch, cw, int(fv), int(fh)]


def main():
    out = {'datasets': np.array([c[0] for c in CASES]), 'cases': np.array([c[1:] for c in CASES], np.int32), 's': np.array(S, np.int32)}
    rs = np.random.RandomState(20261018)
    with tempfile.TemporaryDirectory() as tmp:
        for i, (ds, h, w, seed) in enumerate(CASES):
            # smooth structure plus noise: a resample of pure noise says little about the coordinates
            yy, xx = np.mgrid[0:h, 0:w]
            base = 127.5 + 90 * np.sin(yy[..., None] / 3.1 + np.arange(3)) * np.cos(xx[..., None] / 4.3 - np.arange(3))
            img = np.clip(base + rs.randint(-35, 36, size=(h, w, 3)), 0, 255).astype(np.uint8)
            path = os.path.join(tmp, f'im{i}.png')
            Image.fromarray(img).save(path)
            element = {'image_path': path, 'unique_id': f'im{i}'}
            if ds == 'texture':
                element = ds_texture.DefaultLoader()(element)
                fmt = ds_texture.InpaintingFormatter(resolution=S, hole_range=[0.0, 1.0])
            elif ds == 'places2':
                element = ds_places2.FixResolutionLoader(resolution=S)(element)
                fmt = ds_places2.AdvInpaintingFormatter(resolution=S, hole_range=[0.0, 1.0])
            else:
                element = ds_openimages.FixResolutionLoader(resolution=S)(element)
                fmt = ds_openimages.AdvInpaintingFormatter(resolution=S, hole_range=[0.0, 1.0])
            _, oh, ow = element['image'].shape
            np.random.seed(seed)
            params = _draws(oh, ow, S, flips=ds == 'texture')
            np.random.seed(seed)
            x, mask, uid = fmt(element)
            assert uid == f'im{i}' and tuple(x.shape) == (3, S, S) and x.dtype == torch.float32
            loaded = np.rint(element['image'].numpy().astype(np.float64) * 255)
            out[f'in{i}'] = img
            out[f'loaded{i}'] = loaded.astype(np.uint8).transpose(1, 2, 0)                # HWC codes of the loader's output
            out[f'params{i}'] = np.array(params, np.int32)
            out[f'x{i}'] = x.numpy().copy()
            out[f'mask{i}'] = np.asarray(mask).astype(np.uint8)
            print(ds, (h, w), '->', (oh, ow), 'seed', seed, 'params', params)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
