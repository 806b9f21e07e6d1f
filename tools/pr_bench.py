#!/usr/bin/env python3
"""Timing of the improved precision / recall metric (sh-gan_amd/precision_recall.py, vgg16.py) on one MI355X, random data and random
weights (the rates do not depend on their values).

  --mode manifold  ``radii`` and ``inside`` at --n rows x --dim (default 50 000 x 4096, float16 rows; device events around back-to-back
                   calls): ms per call, the 2 n^2 D flop of the sweep as TFLOP/s and as a share of the fp16 MFMA peak (2.5 PF dense);
                   one ``pr50k3_full`` is two calls of each.
  --mode detector  images/s of ``Vgg16Features`` (full-width VGG16, fc 4096) for every (size, batch) in --cases, its multiply-adds per
                   image and the share of the fp32 matrix peak (157.3 TF); the front end, the thirteen convolutions with their pools,
                   and the two fc layers on their own.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

FP32_PEAK = 157.3e12
FP16_PEAK = 2.5e15


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


def manifold_mode(a):
    from shgan_amd import precision_recall as prm
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    man = (torch.relu(torch.randn(a.n, a.dim, device=dev, generator=g)) * 3).to(torch.float16)
    probes = (torch.relu(torch.randn(a.n, a.dim, device=dev, generator=g)) * 3).to(torch.float16)
    r = prm.radii(man, a.nhood)
    flop = 2.0 * a.n * a.n * a.dim
    out = {'mode': 'manifold', 'n': a.n, 'dim': a.dim, 'nhood_size': a.nhood}
    for name, fn in (('radii', lambda: prm.radii(man, a.nhood)), ('inside', lambda: prm.inside(probes, man, r))):
        ms = _time(fn, a.warmup, a.iters)
        out[name] = {'ms': round(ms, 2), 'tflops': round(flop / ms / 1e9, 1), 'share_of_fp16_peak': round(flop / (ms * 1e-3) / FP16_PEAK, 4)}
    out['pr_ms'] = round(2 * (out['radii']['ms'] + out['inside']['ms']), 2)
    out['inside_share'] = round(float(prm.inside(probes, man, r).float().mean()), 4)
    print(json.dumps(out), flush=True)


def detector_mode(a):
    from shgan_amd import vgg16
    import pr_f64
    dev = 'cuda:0'
    det = vgg16.Vgg16Features.from_state_dict(pr_f64.random_state_dict(0, div=1, fc=4096), device=dev)
    macs = vgg16.macs_per_image(det.widths, 4096, 4096)
    for size, b in a.cases:
        img = torch.randint(0, 256, (b, 3, size, size), dtype=torch.uint8, device=dev)
        ms = _time(lambda: det(img), a.warmup, a.iters)
        rate = b / ms * 1e3
        out = {'mode': 'detector', 'size': size, 'batch': b, 'ms_per_batch': round(ms, 3), 'images_per_s': round(rate, 1), 'macs_per_image': macs,
               'tflops': round(2 * macs * rate / 1e12, 2), 'share_of_fp32_peak': round(2 * macs * rate / FP32_PEAK, 3)}
        x = vgg16.frontend(img, None, det.mean, det.std)
        flat = torch.rand(b, det.fcs[0][0].shape[1], device=dev)

        def convs():
            return vgg16.conv_trunk(det.ops, x)

        def fcs():
            y = flat
            for w, bias in det.fcs:
                y = vgg16.fc_relu(y, w, bias)
            return y
        fc_macs = sum(w.numel() for w, _ in det.fcs)
        for name, fn, m in (('front_end', lambda: vgg16.frontend(img, None, det.mean, det.std), 0), ('convs_and_pools', convs, (macs - fc_macs) * b),
                            ('fc1_fc2', fcs, fc_macs * b)):
            t = _time(fn, a.warmup, a.iters)
            out[name] = {'ms': round(t, 3)}
            if m:
                out[name]['share_of_fp32_peak'] = round(2 * m / (t * 1e-3) / FP32_PEAK, 3)
        out['fc_weight_gb_per_s'] = round(4 * fc_macs / (out['fc1_fc2']['ms'] * 1e-3) / 1e9 * -(-b // 16), 1)
        print(json.dumps(out), flush=True)


def _case(s):
    size, b = s.split('x')
    return int(size), int(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['manifold', 'detector'], default='manifold')
    p.add_argument('--n', type=int, default=50000)
    p.add_argument('--dim', type=int, default=4096)
    p.add_argument('--nhood', type=int, default=3)
    p.add_argument('--cases', type=_case, nargs='+', default=[(512, 16)], help='SIZExBATCH')
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--iters', type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pr_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    manifold_mode(a) if a.mode == 'manifold' else detector_mode(a)


if __name__ == '__main__':
    main()
