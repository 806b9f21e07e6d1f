#!/usr/bin/env python3
"""Golden vectors of the OpenImages evaluation input: runs the reference's own ``FixResolutionLoader`` and ``FreeFormMaskFormatter``
(lib/data_factory/ds_openimages.py:63-81,148-166) and ``RandomMask`` (ds_ffhq.py:199-217) on the CPU and writes
tests/golden/openimages_fit.npz (data only: inputs and the reference's outputs).

  * items at small R (48 / 64), each from a seeded numpy RNG: landscape, portrait, the square sizes whose box comes out one column
    short (94 x 94 at R = 48 and 98 x 98 at R = 64), images smaller than R, exactly R, and flips.  Per item: the input image, the
    formatter's x as uint8 codes (the canvas after the flip), its mask, the content size and the flip decision;
  * ``RandomMask(1024)`` for three seeds, bit-packed.

The reference imports ``torchvision.transforms`` for ``ToTensor``, which is not installed here: a stub with the same uint8 -> float /255
conversion stands in; ``cv2`` / ``pyspng`` are stubbed as in tools/gen_golden.py, and ``lib.visual_service``, which does not exist in the
reference tree, as in tools/gen_golden_metrics.py (never called on these paths).

Runs ONLY where the reference tree exists; nothing here is imported by the product or by the tests.

Usage:  python tools/gen_golden_openimages.py
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SHGAN_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'openimages_fit.npz')

import torch  # noqa: E402


def _to_tensor(pic):
    a = np.asarray(pic)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)


for _name in ['torchvision', 'torchvision.models', 'torchvision.transforms', 'pyspng', 'cv2', 'lib.visual_service']:
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['torchvision'].models = sys.modules['torchvision.models']
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
sys.modules['torchvision.transforms'].ToTensor = lambda: _to_tensor
sys.path.insert(0, REF)

from PIL import Image  # noqa: E402

import lib  # noqa: E402
lib.visual_service = sys.modules['lib.visual_service']

from lib.data_factory.ds_ffhq import RandomMask  # noqa: E402
from lib.data_factory.ds_openimages import FixResolutionLoader, FreeFormMaskFormatter  # noqa: E402

# (h, w, R, random_flip, seed)
CASES = [
    (40, 70, 48, True, 1), (70, 30, 48, True, 2), (94, 94, 48, True, 3), (94, 94, 48, True, 4), (20, 33, 48, True, 5),
    (48, 48, 48, False, 6), (120, 61, 48, False, 7), (98, 98, 64, True, 8), (98, 98, 64, True, 9), (64, 200, 64, True, 10),
    (33, 17, 64, True, 11), (150, 64, 64, False, 12), (64, 64, 64, True, 13), (65, 64, 64, True, 14),
]
MASK_SEEDS = [101, 102, 103]


def main():
    out = {'cases': np.array([(h, w, R, int(fl), sd) for h, w, R, fl, sd in CASES], np.int32), 'mask_seeds': np.array(MASK_SEEDS, np.int32)}
    rs = np.random.RandomState(20261016)
    with tempfile.TemporaryDirectory() as tmp:
        for i, (h, w, R, random_flip, seed) in enumerate(CASES):
            img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
            path = os.path.join(tmp, f'im{i}.png')
            Image.fromarray(img).save(path)
            element = FixResolutionLoader(resolution=R)({'image_path': path, 'unique_id': f'im{i}'})
            np.random.seed(seed)
            flip = bool(random_flip and np.random.rand() < 0.5)
            np.random.seed(seed)
            x, mask, _ = FreeFormMaskFormatter(random_flip=random_flip, resolution=R, hole_range=[0.0, 1.0])(element)
            codes = np.rint((x.numpy().astype(np.float64) + 1) / 2 * 255)
            assert codes.min() >= 0 and codes.max() <= 255
            out[f'in{i}'] = img
            out[f'x{i}'] = codes.astype(np.uint8)
            out[f'mask{i}'] = np.asarray(mask).astype(np.uint8)
            out[f'content{i}'] = np.array(element['content_size'], np.int32)
            out[f'flip{i}'] = np.array(flip)
    for k, seed in enumerate(MASK_SEEDS):
        np.random.seed(seed)
        m = RandomMask(1024, [0.0, 1.0])[0]
        out[f'rm1024_{k}'] = np.packbits(m.astype(np.uint8).reshape(-1))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
