#!/usr/bin/env python3
"""Timing of the image-quality metrics (sh-gan_amd/image_metrics.py) on one MI355X.

  --mode kernel   image_metrics at B x 3 x R x R, uint8 composite + float32 real (the evaluation loop's operands): device-event
                  time per call (both launches) and its share of the HBM roof (operand bytes / 8.0 TB/s).  Run it under
                  ``rocprofv3 --kernel-trace --stats`` for the per-kernel split.
  --mode loop     EvalLoop images/s with metrics=('psnr', 'ssim') and with metrics=None, alternated in one process, on the
                  full 512 generator (the bench.py evaluation loop: uint8 loader, device masks, stand-in FID features); the
                  steady-state rate from the per-batch device events, middle half of the batches.
Prints one JSON line per mode."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def kernel_mode(a):
    from shgan_amd.image_metrics import image_metrics
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (a.batch, 3, a.res, a.res)
    pred = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
    real = torch.rand(shape, device=dev, generator=g) * 2 - 1
    psnr = torch.empty(a.batch, dtype=torch.float64, device=dev)
    ssim = torch.empty_like(psnr)
    for _ in range(a.warmup):
        image_metrics(pred, real, window_size=a.window, psnr_out=psnr, ssim_out=ssim)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        image_metrics(pred, real, window_size=a.window, psnr_out=psnr, ssim_out=ssim)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1e3
    nbytes = pred.numel() * 1 + real.numel() * 4
    roof_us = nbytes / HBM_PEAK * 1e6
    return {'mode': 'kernel', 'shape': list(shape), 'window': a.window, 'us_per_call': round(us, 2), 'operand_bytes': nbytes,
            'hbm_roof_us': round(roof_us, 2), 'fraction_of_hbm_roof': round(roof_us / us, 3),
            'ssim_fma_per_pixel_channel': 10 * a.window + 10, 'note': 'device events around back-to-back calls (both launches + scratch alloc)'}


def loop_mode(a):
    from shgan_amd import configs, eval_harness as hz
    dev = 'cuda:0'
    G = configs.seeded_init_(configs.build_generator(a.res), seed=0).eval().requires_grad_(False).to(dev)
    n = a.batch * a.steps

    def once(metrics, seed):
        loop = hz.EvalLoop(G, dev, a.res, n, noise_mode='random', seed=0, feature_fn=hz.standin_features, timing=True, metrics=metrics)
        loader = hz.PinnedU8Loader(loop.ids, a.batch, a.res, seed=1000, pool=4)
        np.random.seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(loader)
        loop.gather()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        evs = loop.batch_done_events
        k0, k1 = len(evs) // 4, len(evs) - 1 - len(evs) // 4
        steady = evs[k0].elapsed_time(evs[k1]) / (k1 - k0)
        return n / dt, a.batch / steady * 1e3
    once(None, 1)
    once(('psnr', 'ssim'), 1)                      # warm-up of both forms
    on, off = [], []
    for r in range(a.rounds):
        off.append(once(None, 100 + r))
        on.append(once(('psnr', 'ssim'), 100 + r))
    med = lambda v, i: float(np.median([x[i] for x in v]))   # noqa: E731
    return {'mode': 'loop', 'res': a.res, 'batch': a.batch, 'batches': a.steps, 'rounds': a.rounds,
            'images_per_s_off': round(med(off, 0), 1), 'images_per_s_on': round(med(on, 0), 1),
            'steady_images_per_s_off': round(med(off, 1), 1), 'steady_images_per_s_on': round(med(on, 1), 1),
            'ratio_whole_loop': round(med(on, 0) / med(off, 0), 4), 'ratio_steady': round(med(on, 1) / med(off, 1), 4),
            'all_off': [round(x[1], 1) for x in off], 'all_on': [round(x[1], 1) for x in on]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['kernel', 'loop'], default='kernel')
    p.add_argument('--res', type=int, default=512)
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--window', type=int, default=11)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--steps', type=int, default=24)
    p.add_argument('--rounds', type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('image_metrics_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    print(json.dumps(kernel_mode(a) if a.mode == 'kernel' else loop_mode(a)))


if __name__ == '__main__':
    main()
