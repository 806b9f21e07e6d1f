#!/usr/bin/env python3
"""Timing of the FID detector (sh-gan_amd/inception.py) on one MI355X, random weights (the rate does not depend on their values).

  --mode detector  images/s of ``det(u8 images)`` for every batch in --batches and input size in --sizes (device events around
                   back-to-back calls: front end + 94 convolutions + pools + mean), the multiply-adds of the 94 convolutions per image
                   (computed from the layer shapes) and the achieved share of the fp32 matrix peak (157.3 TF).  Run it alone under
                   ``rocprofv3 --kernel-trace --stats`` for the per-kernel split (--classes summarises the resulting kernel_stats.csv).
  --mode loop      EvalLoop images/s at --res x --batch (the full 512 generator, uint8 loader, device masks, random noise) with the
                   stand-in features, with the detector on the fakes only, and on fakes + reals (fid_real=True), alternated in one
                   process; whole-loop rate and the steady-state rate from the per-batch device events (middle half of the batches).
  --classes CSV    kernel classes of a rocprofv3 kernel_stats.csv: total / per-call time and share.
Prints one JSON line per measurement."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP32_PEAK = 157.3e12
CLASSES = (('conv', 'inc_conv_kernel'), ('splitk_reduce', 'inc_splitk_reduce_kernel'), ('frontend', 'inc_frontend_kernel'),
           ('pool', 'inc_pool_kernel'), ('mean', 'inc_mean_kernel'), ('weight_prep', 'inc_weight_prep_kernel'))


def _detector(dev, split_k=True):
    from shgan_amd import inception
    import inception_f64
    return inception.InceptionFeatures.from_state_dict(inception_f64.random_state_dict(0), device=dev, split_k=split_k)


def detector_mode(a):
    from shgan_amd import inception
    dev = 'cuda:0'
    det = _detector(dev)
    macs = inception.macs_per_image()
    out = []
    for b in a.batches:
        for r in a.sizes:
            img = torch.randint(0, 256, (b, 3, r, r), dtype=torch.uint8, device=dev)
            for _ in range(a.warmup):
                det(img)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                det(img)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            rate = b / ms * 1e3
            out.append({'mode': 'detector', 'batch': b, 'size': r, 'ms_per_batch': round(ms, 3), 'images_per_s': round(rate, 1),
                        'macs_per_image': macs, 'conv_tflops': round(2 * macs * rate / 1e12, 2),
                        'share_of_fp32_peak': round(2 * macs * rate / FP32_PEAK, 3)})
            print(json.dumps(out[-1]), flush=True)
    return out


def loop_mode(a):
    from shgan_amd import configs, eval_harness as hz
    dev = 'cuda:0'
    G = configs.seeded_init_(configs.build_generator(a.res), seed=0).eval().requires_grad_(False).to(dev)
    det = _detector(dev)
    n = a.batch * a.steps
    forms = {'standin': dict(feature_fn=hz.standin_features), 'detector_fake': dict(feature_fn=det),
             'detector_fake_real': dict(feature_fn=det, fid_real=True)}

    def once(kw, seed):
        loop = hz.EvalLoop(G, dev, a.res, n, noise_mode='random', seed=0, timing=True, **kw)
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
    for kw in forms.values():
        once(kw, 1)                                  # warm-up of every form
    res = {k: [] for k in forms}
    for r in range(a.rounds):
        for k, kw in forms.items():
            res[k].append(once(kw, 100 + r))
    med = lambda v, i: float(np.median([x[i] for x in v]))   # noqa: E731
    out = {'mode': 'loop', 'res': a.res, 'batch': a.batch, 'batches': a.steps, 'rounds': a.rounds}
    for k in forms:
        out[f'{k}_images_per_s'] = round(med(res[k], 0), 1)
        out[f'{k}_steady_images_per_s'] = round(med(res[k], 1), 1)
    print(json.dumps(out), flush=True)
    return out


def classes(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    out = {'mode': 'classes', 'csv': os.path.basename(path)}
    for cls, key in CLASSES + (('other', None),):
        sel = [r for r in rows if (key is not None and key in r['Name']) or
               (key is None and not any(k in r['Name'] for _, k in CLASSES))]
        ns = sum(float(r['TotalDurationNs']) for r in sel)
        calls = sum(int(r['Calls']) for r in sel)
        out[cls] = {'total_ms': round(ns / 1e6, 3), 'calls': calls, 'us_per_call': round(ns / 1e3 / max(calls, 1), 2),
                    'share': round(ns / max(total, 1), 4)}
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['detector', 'loop'], default='detector')
    p.add_argument('--batches', type=int, nargs='+', default=[16, 32])
    p.add_argument('--sizes', type=int, nargs='+', default=[256, 512, 1024])
    p.add_argument('--res', type=int, default=512)
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--steps', type=int, default=16)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--classes', default=None, help='summarise a rocprofv3 kernel_stats.csv instead of measuring')
    a = p.parse_args()
    if a.classes:
        classes(a.classes)
        return
    if not torch.cuda.is_available():
        raise SystemExit('inception_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    detector_mode(a) if a.mode == 'detector' else loop_mode(a)


if __name__ == '__main__':
    main()
