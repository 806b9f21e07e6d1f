#!/usr/bin/env python3
"""Golden vectors of the image-quality evaluators: runs the reference's own ``psnr_evaluator`` (lib/evaluator/eva_psnr.py,
``for_dataset=None, rgb_range=1``) and ``compute_ssim(..., size_average=False)`` (lib/evaluator/eva_ssim.py) on the CPU and writes
tests/golden/image_metrics.npz (data only: inputs and the reference's outputs).

The inputs are what the evaluation loop hands its evaluators (shgan_default.py:279-291): ``pred = fake_u8 / 255`` (numpy float64) and
``gt = (real + 1) / 2`` with ``real = ToTensor(u8) * 2 - 1`` (float32) built from decoded uint8 pixels.  The reference modules import
``lib.nputils``, which does not exist in the reference tree: a stub module stands in (it is never called on these paths).

Runs ONLY where the reference tree exists; nothing here is imported by the product or by the tests.

Usage:  python tools/gen_golden_metrics.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SHGAN_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'image_metrics.npz')

for _name in ['cv2', 'lib.nputils']:
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.path.insert(0, REF)

import torch  # noqa: E402

import lib  # noqa: E402
lib.nputils = sys.modules['lib.nputils']
from lib.evaluator import eva_psnr, eva_ssim  # noqa: E402

# (name, shape, window_size, seed, pred == gt pixels)
CASES = [
    ('a64_w11', (4, 3, 64, 64), 11, 1, False),
    ('a64_w7', (4, 3, 64, 64), 7, 2, False),
    ('b37x53_w11', (2, 3, 37, 53), 11, 3, False),
    ('b37x53_w7', (2, 3, 37, 53), 7, 4, False),
    ('same37x53_w11', (2, 3, 37, 53), 11, 5, True),
]


def synth(shape, seed, same):
    """Decoded pixels (smooth gradients + texture, so that SSIM is neither ~0 nor ~1) and a composite that differs from them in a
    rectangular 'hole' plus a little noise elsewhere."""
    rs = np.random.RandomState(seed)
    b, c, h, w = shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    base = 128 + 60 * np.sin(xx[None, None] / (3.0 + rs.rand(b, c, 1, 1) * 5)) * np.cos(yy[None, None] / (4.0 + rs.rand(b, c, 1, 1) * 5))
    real_u8 = np.clip(base + rs.randint(-40, 41, size=shape), 0, 255).astype(np.uint8)
    if same:
        return real_u8.copy(), real_u8
    pred = real_u8.astype(np.int32) + rs.randint(-6, 7, size=shape)
    for i in range(b):
        y0, x0 = rs.randint(0, h // 2), rs.randint(0, w // 2)
        pred[i, :, y0:y0 + h // 3, x0:x0 + w // 3] = rs.randint(0, 256, size=(c, len(range(y0, min(h, y0 + h // 3))), len(range(x0, min(w, x0 + w // 3)))))
    return np.clip(pred, 0, 255).astype(np.uint8), real_u8


def main():
    out = {}
    for name, shape, ws, seed, same in CASES:
        pred_u8, real_u8 = synth(shape, seed, same)
        real = (torch.from_numpy(real_u8).to(torch.float32).div(255) * 2 - 1).numpy()     # ToTensor() * 2 - 1
        pred = pred_u8 / 255                                                                # torch_to_numpy(fake) / 255: float64
        gt = (real + 1) / 2                                                                 # float32
        ev = eva_psnr.psnr_evaluator(for_dataset=None, rgb_range=1)
        ev.add_batch(pred=pred, gt=gt, fn=None)
        ev.set_sample_n(shape[0])
        mean_psnr = ev.compute()
        per_psnr = np.concatenate(ev.data_psnr, axis=0)
        ssim = eva_ssim.compute_ssim(torch.FloatTensor(pred), torch.FloatTensor(gt), window_size=ws, size_average=False)
        out[name + '/pred_u8'] = pred_u8
        out[name + '/real_u8'] = real_u8
        out[name + '/window'] = np.int64(ws)
        out[name + '/psnr'] = per_psnr.astype(np.float64)
        out[name + '/psnr_mean'] = np.float64(mean_psnr)
        out[name + '/ssim'] = ssim.numpy().astype(np.float64)
        print(f'{name}: psnr {per_psnr} ssim {out[name + "/ssim"]}')
    out['cases'] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print('wrote', OUT)


if __name__ == '__main__':
    main()
