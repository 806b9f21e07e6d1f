#!/usr/bin/env python3
"""Golden draws of the LaMa thin / medium / thick masks -> tests/golden/lama_masks.npz.

Runs the reference's own ``LamaMaskFormatter`` (lib/data_factory/ds_ffhq.py:352-381, drawing through lama_mask_utils.py) with a recording
stand-in for ``cv2`` (tools/lama_cv2_standin/cv2.py): the ``cv2.line`` calls are the fixture, not pixels -- ``cv2`` is not installed
where this runs, and the rasteriser is pinned elsewhere (tests/lama_cv_ref.py).  Runs only where the reference tree exists
(``SHGAN_REFERENCE``); the file it writes holds data only and is committed, nothing here is imported by the product or the tests.

Per setting (thin / medium / thick x 256 / 512), ``np.random.seed(SEED + k)`` then 24 formatter calls with ``random_flip=True``:
  calls_<key>   int32 [n, 5]   (x0, y0, x1, y1, thickness) of every ``cv2.line`` call, in order
  offs_<key>    int32 [25]     calls of mask i = calls[offs[i]:offs[i+1]]
  boxes_<key>   uint8 [24, s*s/8]   np.packbits of the painted pixels without the lines: the rectangle generator's masks
  flips_<key>   uint8 [24]     whether the formatter flipped the image
  witness_<key> int64          one np.random.randint(2**31) drawn after the last mask: the RNG-state witness
  argtypes      the type names the end points arrived with (the reference passes numpy int32 scalars)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SHGAN_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'lama_masks.npz')
SEED, N = 20240, 24

for _name in ['torchvision', 'torchvision.models', 'torchvision.transforms', 'pyspng']:
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['torchvision'].models = sys.modules['torchvision.models']
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'lama_cv2_standin'))

import cv2  # noqa: E402  (the stand-in)
import torch  # noqa: E402
from lib.data_factory.ds_ffhq import LamaMaskFormatter  # noqa: E402


def main():
    out, types_seen = {}, set()
    k = 0
    for res in (256, 512):
        for kind in ('thin', 'medium', 'thick'):
            key = f'{kind}{res}'
            fmt = LamaMaskFormatter(random_flip=True, resolution=res, type=kind)
            image = ((torch.arange(res, dtype=torch.float32) + 1) / (2 * res)).expand(3, res, res).contiguous()
            np.random.seed(SEED + k)
            k += 1
            calls, offs, boxes, flips = [], [0], [], []
            for i in range(N):
                del cv2.calls[:]
                x, mask, uid = fmt({'image': image, 'unique_id': str(i)})
                flips.append(int(bool(x[0, 0, 0] > x[0, 0, -1])))
                types_seen.update(c[5] for c in cv2.calls)
                calls.extend(c[:5] for c in cv2.calls)
                offs.append(len(calls))
                painted = (1 - np.asarray(mask)).astype(np.uint8)
                assert painted.shape == (res, res) and set(np.unique(painted)) <= {0, 1}
                boxes.append(np.packbits(painted.reshape(-1)))
            out['calls_' + key] = np.asarray(calls, dtype=np.int32).reshape(-1, 5)
            out['offs_' + key] = np.asarray(offs, dtype=np.int32)
            out['boxes_' + key] = np.stack(boxes)
            out['flips_' + key] = np.asarray(flips, dtype=np.uint8)
            out['witness_' + key] = np.int64(np.random.randint(2 ** 31))
            c = out['calls_' + key]
            print(f'  {key}: {len(c)} line calls (max {int(np.diff(offs).max())} per mask), thickness {c[:, 4].min() if len(c) else "-"}..'
                  f'{c[:, 4].max() if len(c) else "-"}, {int(sum(b.any() for b in boxes))} box masks, {sum(flips)} flips')
    out['seed'], out['argtypes'] = np.int64(SEED), np.asarray(sorted(types_seen))
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)')


if __name__ == '__main__':
    main()
