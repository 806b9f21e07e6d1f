"""Writes tests/golden/places2_resize.npz: seeded uint8 RGB images of Places2-like (and awkward) sizes and Pillow's
``Image.resize([R, R], BICUBIC)`` of each (FixResolutionLoader, ds_places2.py:90-103) -- the GPU test pins the device resize to these bytes
independently of the Pillow version installed where it runs."""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(72, 96, 48), (48, 36, 48), (48, 48, 48), (48, 150, 48), (150, 100, 24), (58, 38, 24), (31, 97, 20), (6, 5, 40)]


def main():
    rs = np.random.RandomState(20261015)
    out = {'cases': np.array(CASES, np.int32)}
    for i, (h, w, R) in enumerate(CASES):
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        out[f'in{i}'] = img
        out[f'out{i}'] = np.ascontiguousarray(np.asarray(Image.fromarray(img).resize([R, R], Image.BICUBIC)).transpose(2, 0, 1))
    path = os.path.join(ROOT, 'tests', 'golden', 'places2_resize.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
