#!/usr/bin/env python
"""Measure pluralistic sampling on one MI355X (a tool, not part of bench.py):

  * images/s of ``G.sample_many(x[N], z[N,K])`` next to ``G(x.repeat_interleave(K, 0), z.flatten(0, 1))`` at the same N*K rows (default:
    full-width 512^2, N*K = 16, K = 1, 2, 4, 8), both in this process, alternating, after a warm-up of every shape;
  * the time of the expansion launch alone (``G.expand_encoding`` on a finished encoding) and the bytes it moves;
  * pairs/s of the LPIPS pair head (``diversity.pairwise_lpips`` on finished taps is what it serves: all five AlexNet taps of N*K images at
    256^2, K = 8) and of the whole ``pairwise_lpips`` call.

Times are HIP events around ``reps`` calls on one stream (no pipelining), the median of ``rounds`` such windows; the ``piped_*`` figures
are the same two calls plus the uint8 composite as independent batches on three streams (``eval_harness.StreamPipeline``), by the host clock.  Prints one JSON line.
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shgan_amd  # noqa: E402,F401
from shgan_amd import configs, diversity, eval_harness, lpips  # noqa: E402


def timed(fn, reps, rounds):
    """Median over ``rounds`` windows of (ms per call over ``reps`` back-to-back calls)."""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def piped(dev, step, args, batches, rounds):
    """ms per batch of ``batches`` independent batches issued round-robin on three streams (eval_harness.StreamPipeline, the evaluation loop's
    way), host clock around work that ends in a device synchronise; median over ``rounds``."""
    out = []
    for _ in range(rounds):
        pipe = eval_harness.StreamPipeline(dev, depth=3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            pipe.run(step, *args)
        pipe.join()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / batches * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--rows', type=int, default=16, help='N*K synthesis rows')
    ap.add_argument('--ks', type=int, nargs='*', default=[1, 2, 4, 8])
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--widths', type=int, nargs=5, default=None, metavar=('CH_BASE', 'CH_MAX', 'W_DIM', 'Z_DIM', 'W0_DIM'),
                    help='reduced widths (rehearsals); default: the shipped full width')
    ap.add_argument('--noise-mode', default='random')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('plural_bench: needs a GPU (there is no CPU path)')
    dev = 'cuda:0'
    kw = dict(zip(('ch_base', 'ch_max', 'w_dim', 'z_dim', 'w0_dim'), a.widths)) if a.widths else {}
    G = configs.seeded_init_(configs.build_generator(a.resolution, **kw), seed=1, noise_strength=0.05).eval().requires_grad_(False).to(dev)
    res = dict(tool='plural_bench', device=torch.cuda.get_device_name(0), resolution=a.resolution, rows=a.rows, reps=a.reps, rounds=a.rounds,
               noise_mode=a.noise_mode, sample_many=[])
    with torch.no_grad():
        for k in a.ks:
            n = a.rows // k
            x, z, _, _ = eval_harness.synthetic_batch(n, a.resolution, G.z_dim, seed=3, device=dev, masks='bernoulli')
            zk = torch.randn(n, k, G.z_dim, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
            xr, zr, c = x.repeat_interleave(k, 0), zk.flatten(0, 1).contiguous(), torch.zeros(n * k, 0, device=dev)
            many = lambda: G.sample_many(x, zk, noise_mode=a.noise_mode)                          # noqa: E731
            rep = lambda: G(x=xr, z=zr, c=c, noise_mode=a.noise_mode)                             # noqa: E731
            for _ in range(a.warmup):
                many(), rep()
            torch.cuda.synchronize()
            tm, tr = [], []
            for _ in range(a.rounds):                                                             # alternate the two within the call
                tm.append(timed(many, a.reps, 1)[0])
                tr.append(timed(rep, a.reps, 1)[0])
            pm = piped(dev, lambda x_, z_: eval_harness.run_generator_many(G, x_, z_, noise_mode=a.noise_mode), (x, zk), 3 * a.reps, a.rounds)
            pr = piped(dev, lambda x_, z_: eval_harness.run_generator(G, x_, z_, noise_mode=a.noise_mode), (xr, zr), 3 * a.reps, a.rounds)
            enc = G.encode(x)
            expand = lambda: G.expand_encoding(enc, k)                                            # noqa: E731
            for _ in range(a.warmup):
                expand()
            te = timed(expand, 4 * a.reps, a.rounds)
            per_image = sum(t[0].numel() * t.element_size() for t in [enc[0]] + list(enc[1].values()))
            m, r = statistics.median(tm), statistics.median(tr)
            res['sample_many'].append(dict(K=k, N=n, sample_many_ms=round(m, 3), repeated_ms=round(r, 3), sample_many_ms_range=[round(min(tm), 3), round(max(tm), 3)],
                                           repeated_ms_range=[round(min(tr), 3), round(max(tr), 3)], sample_many_img_s=round(n * k / m * 1e3, 1),
                                           repeated_img_s=round(n * k / r * 1e3, 1), speedup=round(r / m, 3), piped_sample_many_ms=round(pm, 3),
                                           piped_repeated_ms=round(pr, 3), piped_speedup=round(pr / pm, 3),
                                           bound=round(1 / (0.505 + 0.495 / k), 3), expand_ms=round(te[0], 4), expand_ms_range=[round(te[1], 4), round(te[2], 4)],
                                           expand_bytes_written=per_image * n * k, expand_gb_s=round(per_image * n * (k + 1) / te[0] / 1e6, 1)))
            print('[plural_bench]', json.dumps(res['sample_many'][-1]), file=sys.stderr, flush=True)
            del x, z, zk, xr, zr, enc
            torch.cuda.empty_cache()
        # the pair head: N*K = rows images at 256^2, K = 8
        shapes = lpips._conv_shapes(lpips.PACKAGE_CONV_KEYS)
        shapes.update(lpips._lin_shapes())
        g = torch.Generator().manual_seed(11)
        sd = {key: torch.randn(shape, generator=g).mul_(0.05).abs_() if key.startswith('lin') else torch.randn(shape, generator=g).mul_(0.05)
              for key, shape in shapes.items()}
        net = lpips.LPIPS(net='alex', state_dict=sd, device=dev)                                  # random weights: the timing does not depend on them
        k, n = 8, max(1, a.rows // 8)
        imgs = torch.randint(0, 256, (n, k, 3, 256, 256), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        taps = net.taps_of(imgs.view(n * k, 3, 256, 256))
        ia, ib = (t.to(dev) for t in diversity.pair_tables(n, k))
        vals = torch.zeros(ia.numel(), dtype=torch.float64, device=dev)

        def heads():
            for t, w in zip(taps, net.lins):
                lpips.head_pairs(t, ia, ib, w, vals)
        whole = lambda: diversity.pairwise_lpips(net, imgs)                                       # noqa: E731
        for _ in range(a.warmup):
            heads(), whole()
        th, tw = timed(heads, 4 * a.reps, a.rounds), timed(whole, 4 * a.reps, a.rounds)
        res['pair_head'] = dict(resolution=256, K=k, N=n, pairs=int(ia.numel()), heads_ms=round(th[0], 4), heads_ms_range=[round(th[1], 4), round(th[2], 4)],
                                pairs_per_s=round(ia.numel() / th[0] * 1e3, 1), pairwise_lpips_ms=round(tw[0], 4),
                                pairwise_lpips_pairs_per_s=round(ia.numel() / tw[0] * 1e3, 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
