#!/usr/bin/env python3
"""Timing of LPIPS (sh-gan_amd/lpips.py) on one MI355X, random weights (the rate does not depend on their values).

  --mode network  pairs/s of ``net(pred_u8, real)`` for every (size, batch) in --cases (device events around back-to-back calls: two
                  conv1 launches, two pools, four convolutions, five head launch pairs), the multiply-adds of the ten convolutions per
                  pair and the achieved share of the fp32 matrix peak (157.3 TF); the time of every stage on its own (same buffers,
                  back-to-back launches of that stage only) with the convolutions' own share of peak; and the same network as
                  ``torch.nn.functional`` float32 calls on the same GPU.
  --mode loop     EvalLoop images/s at --res x --batch (the full generator, uint8 loader, device masks, random noise, PSNR + SSIM on)
                  with and without ``lpips=net``, alternated in one process; whole-loop rate and the steady-state rate from the
                  per-batch device events (middle half of the batches).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FP32_PEAK = 157.3e12


def _net(dev):
    from shgan_amd import lpips
    import lpips_f64
    sd = lpips_f64.random_state_dict(0)
    return lpips.Lpips.from_state_dict(sd, device=dev), sd


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


def _torch_f32(sd, dev):
    """The same network as plain float32 torch calls (rocBLAS / MIOpen behind them)."""
    import lpips_f64
    w = {k: v.to(dev) for k, v in sd.items()}
    shift = torch.tensor(lpips_f64.SHIFT, device=dev)[None, :, None, None]
    scale = torch.tensor(lpips_f64.SCALE, device=dev)[None, :, None, None]

    def run(pred_u8, real):
        x = torch.cat([(pred_u8.to(torch.float32) / 255 - 0.5) * 2, ((real + 1) / 2 - 0.5) * 2])
        x = (x - shift) / scale
        b, total = pred_u8.shape[0], 0
        for n, (key, _, _, _, s, p) in enumerate(lpips_f64.CONVS):
            if n in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w[f'{key}.weight'], w[f'{key}.bias'], stride=s, padding=p))
            f = x / (torch.sqrt((x * x).sum(dim=1, keepdim=True)) + 1e-10)
            total = total + (w[f'lin{n}.model.1.weight'] * (f[:b] - f[b:]) ** 2).sum(dim=1).mean(dim=(1, 2))
        return total
    return run


def network_mode(a):
    from shgan_amd import inception, lpips
    dev = 'cuda:0'
    net, sd = _net(dev)
    ref = _torch_f32(sd, dev)
    for size, b in a.cases:
        pred = torch.randint(0, 256, (b, 3, size, size), dtype=torch.uint8, device=dev)
        real = torch.rand(b, 3, size, size, device=dev) * 2 - 1
        ms = _time(lambda: net(pred, real), a.warmup, a.iters)
        ms_t = _time(lambda: ref(pred, real), a.warmup, a.iters)
        macs = lpips.macs_per_pair(size, size)
        rate = b / ms * 1e3
        out = {'mode': 'network', 'size': size, 'batch': b, 'ms_per_batch': round(ms, 3), 'pairs_per_s': round(rate, 1), 'macs_per_pair': macs,
               'conv_tflops': round(2 * macs * rate / 1e12, 2), 'share_of_fp32_peak': round(2 * macs * rate / FP32_PEAK, 3),
               'torch_f32_ms_per_batch': round(ms_t, 3), 'torch_f32_pairs_per_s': round(b / ms_t * 1e3, 1)}
        print(json.dumps(out), flush=True)
        # every stage on its own
        taps = net.features(pred, real)
        hs = lpips.out_sizes(size)
        stages = {}
        y0 = torch.empty_like(taps[0])
        stages['conv1_u8'] = (lambda: lpips.conv1(pred, *net.conv1_wb, 'pred', y=y0[:b]), b * hs[0] ** 2 * 64 * 363)
        stages['conv1_f32'] = (lambda: lpips.conv1(real, *net.conv1_wb, 'gt', y=y0[b:]), b * hs[0] ** 2 * 64 * 363)
        stages['pool1'] = (lambda: inception.pool(taps[0], 'max', 2, 0), 0)
        stages['pool2'] = (lambda: inception.pool(taps[1], 'max', 2, 0), 0)
        x = inception.pool(taps[0], 'max', 2, 0)
        for k, op in enumerate(net.ops, start=1):
            y = torch.empty_like(taps[k])
            i, o, ks, _, _ = lpips.CONVS[k]
            stages[f'conv{k + 1}'] = ((lambda op=op, x=x, y=y: inception.conv_group([(op, x, 0, y, 0)], split_k=False)),
                                      2 * b * hs[k] ** 2 * o * i * ks * ks)
            x = inception.pool(taps[1], 'max', 2, 0) if k == 1 else taps[k]
        val = torch.zeros(b, dtype=torch.float64, device=dev)
        for k in range(5):
            stages[f'head{k}'] = ((lambda k=k: lpips.head(taps[k][:b], taps[k][b:], net.lins[k], val)), 0)
        per = {'mode': 'stages', 'size': size, 'batch': b}
        for name, (fn, m) in stages.items():
            t = _time(fn, a.warmup, a.iters)
            per[name] = {'us': round(t * 1e3, 1)}
            if m:
                per[name]['share_of_fp32_peak'] = round(2 * m / (t * 1e-3) / FP32_PEAK, 3)
        print(json.dumps(per), flush=True)


def loop_mode(a):
    from shgan_amd import configs, eval_harness as hz
    dev = 'cuda:0'
    G = configs.seeded_init_(configs.build_generator(a.res), seed=0).eval().requires_grad_(False).to(dev)
    net, _ = _net(dev)
    n = a.batch * a.steps
    forms = {'lpips_off': {}, 'lpips_on': {'lpips': net}}

    def once(kw, seed):
        loop = hz.EvalLoop(G, dev, a.res, n, noise_mode='random', seed=0, timing=True, metrics=('psnr', 'ssim'), **kw)
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
        out[f'{k}_steady_all'] = [round(x[1], 1) for x in res[k]]
    print(json.dumps(out), flush=True)


def _case(s):
    size, b = s.split('x')
    return int(size), int(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['network', 'loop'], default='network')
    p.add_argument('--cases', type=_case, nargs='+', default=[(256, 32), (512, 16)], help='SIZExBATCH')
    p.add_argument('--res', type=int, default=512)
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--steps', type=int, default=16)
    p.add_argument('--rounds', type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    network_mode(a) if a.mode == 'network' else loop_mode(a)


if __name__ == '__main__':
    main()
