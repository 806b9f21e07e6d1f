#!/usr/bin/env python3
"""Timing of the perceptual path length (sh-gan_amd/ppl.py) on one MI355X, random weights (the rate does not depend on their values).

  --mode metric    ``ppl2_wend`` samples/s at every resolution in --res: a plain StyleGAN2 ``Generator`` of the shipped widths and a
                   full-width VGG16 with random weights; device events around --iters back-to-back ``sampler(c)`` calls (batch 2: four
                   synthesis images, one front-end launch, one trunk run, five head launches), after --warmup calls.
  --mode frontend  ``shg_ppl_frontend_f32`` alone at every resolution in --res (batch --batch): microseconds per launch and the achieved
                   bandwidth against the bytes it must move (the window of x once, y once).
Stand-alone timing only.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

FULL = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _vgg(dev):
    from shgan_amd import lpips
    import ppl_f64
    return lpips.LPIPS(net='vgg', state_dict=ppl_f64.vgg_random_state_dict(FULL, seed=0), device=dev)


def _generator(res, dev):
    from shgan_amd.model_zoo import stylegan
    torch.manual_seed(0)
    syn = stylegan.Synthesis(w_dim=512, resolution=res, rgb_n=3, ch_base=32768, ch_max=512, use_fp16_after_res=None)
    mp = stylegan.Mapping(z_dim=512, c_dim=0, w_dim=512, num_ws=syn.num_ws, num_layers=8)
    return stylegan.Generator(mp, syn).eval().requires_grad_(False).to(dev)


def metric_mode(a):
    from shgan_amd import lpips, ppl
    dev = 'cuda:0'
    vgg = _vgg(dev)
    for res in a.res:
        sampler = ppl.PPLSampler(_generator(res, dev), vgg, generator=torch.Generator(device=dev).manual_seed(0))
        c = torch.zeros(2, 0, device=dev)
        ms = _time(lambda: sampler(c), a.warmup, a.iters)
        side = ppl.frontend_side(3, res, res, res // 256, False)
        print(json.dumps({'mode': 'metric', 'res': res, 'batch': 2, 'ms_per_call': round(ms, 3), 'samples_per_s': round(2 / ms * 1e3, 2),
                          'hours_for_50000': round(50000 / (2 / ms * 1e3) / 3600, 3),
                          'vgg_macs_per_image': lpips.vgg_macs_per_image(FULL, side, side)}), flush=True)


def frontend_mode(a):
    from shgan_amd import ppl
    dev = 'cuda:0'
    for res in a.res:
        for crop in (False, True):
            x = torch.rand(a.batch, 3, res, res, device=dev) * 2 - 1
            factor = res // 256
            side = ppl.frontend_side(3, res, res, factor, crop)
            y = torch.empty(a.batch, 3, side, side, device=dev)
            ms = _time(lambda: ppl.frontend(x, factor, crop, y=y), a.warmup, a.iters)
            nbytes = 4 * a.batch * 3 * (side * max(factor, 1)) ** 2 + 4 * y.numel()
            print(json.dumps({'mode': 'frontend', 'res': res, 'batch': a.batch, 'crop': crop, 'factor': factor, 'us_per_launch': round(ms * 1e3, 2),
                              'bytes_moved': nbytes, 'gb_per_s': round(nbytes / (ms * 1e-3) / 1e9, 1)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['metric', 'frontend'], default='metric')
    p.add_argument('--res', type=int, nargs='+', default=[256, 512])
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--iters', type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ppl_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    with torch.no_grad():
        metric_mode(a) if a.mode == 'metric' else frontend_mode(a)


if __name__ == '__main__':
    main()
