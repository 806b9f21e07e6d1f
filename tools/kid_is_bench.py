#!/usr/bin/env python3
"""Timing of KID and the Inception Score pieces (sh-gan_amd/kid.py, inception_score.py, the head of inception.py) on one MI355X.

  --mode kernels  the KID launch pair at (S, m, D) = (100, 1000, 2048) and (100, 100, 2048) on float32 features (device events around
                  back-to-back calls; --rounds timed windows per shape, the two shapes alternating, median and min..max reported),
                  its fp64 operations computed from the shapes (2 D per kernel-matrix entry over the tiles the
                  kernel walks), the achieved rate and the share of the fp64 matrix peak (78.6 TF: AMD's published MI355X figure);
                  numpy on the host for the same KID in float64 and in the reference's float32, with their distance from each other
                  and the kernel's distance from float64 (--host-subsets of the 100 subsets, the time scaled); the classifier head plus
                  the IS accumulation at batch 16 and 64.
  --mode loop     EvalLoop images/s at --res x --batch (the full generator, uint8 loader, device masks, random noise, the random-weight
                  detector on fakes and reals) with and without ``kid`` + ``inception_score``, alternated in one process; whole-loop and
                  steady-state rate (per-batch device events, middle half of the batches).
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

FP64_MFMA_PEAK = 78.6e12


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


def _spread(v):
    return {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3), 'all': [round(x, 3) for x in v]}


def kid_flops(S, m, D, tile=64):
    """(fp64 operations of the tiles the kernel walks, those of the three full m x m products the reference forms)."""
    T = -(-m // tile)
    return S * (T * (T + 1) + T * T) * tile * tile * 2 * D, S * 3 * m * m * 2 * D


def _host_kid(fake, real, idx_f, idx_r, dtype):
    """kernel_inception_distance.py:36-43 in numpy at ``dtype`` with the draws given -> (kid, seconds)."""
    x_all, y_all = fake.astype(dtype), real.astype(dtype)
    n, m = x_all.shape[1], idx_f.shape[1]
    t0 = time.perf_counter()
    t = 0
    for s in range(len(idx_f)):
        x, y = x_all[idx_f[s]], y_all[idx_r[s]]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return float(t / len(idx_f) / m), time.perf_counter() - t0


def kernels_mode(a):
    from shgan_amd import inception, inception_score as isc, kid
    dev = 'cuda:0'
    g = np.random.RandomState(0)
    shapes, data, times = ((100, 1000, 2048), (100, 100, 2048)), {}, {}
    for S, m, D in shapes:
        n = max(2 * m, 1000)
        fake = (g.rand(n, D) * g.rand(n, 1) * 2).astype(np.float32)
        real = (g.rand(n, D) * g.rand(n, 1) * 2.2).astype(np.float32)
        idx_f, idx_r, _ = kid.kid_subsets(n, n, S, m, seed=0)
        data[m] = (n, fake, real, idx_f, idx_r, [torch.from_numpy(t).to(dev) for t in (fake, real, idx_f, idx_r)])
        times[m] = []
    for _ in range(a.rounds):                      # the shapes alternate: a drift of the clock shows as spread, not as a difference
        for S, m, D in shapes:
            dv = data[m][5]
            times[m].append(_time(lambda: kid.kid_sums(*dv), a.warmup, a.iters if m >= 1000 else a.iters * 20))
    for S, m, D in shapes:
        n, fake, real, idx_f, idx_r, dv = data[m]
        ms = float(np.median(times[m]))
        walked, full = kid_flops(S, m, D)
        sums = kid.kid_sums(*dv).cpu().numpy()
        got = kid.kid_from_sums(sums, m)
        hs = min(a.host_subsets, S)
        k64, t64 = _host_kid(fake, real, idx_f[:hs], idx_r[:hs], np.float64)
        k32, t32 = _host_kid(fake, real, idx_f[:hs], idx_r[:hs], np.float32)
        part = kid.kid_from_sums(sums[:hs], m)
        scale = float(np.mean(np.abs(sums[:hs, 0]) + np.abs(sums[:hs, 1]))) / (m - 1) / m
        print(json.dumps({'mode': 'kid', 'S': S, 'm': m, 'D': D, 'n_rows': n, 'ms': round(ms, 3), 'ms_rounds': _spread(times[m]), 'fp64_flop_walked': walked, 'fp64_flop_full': full,
                          'tflops_walked': round(walked / ms / 1e9, 2), 'share_of_fp64_mfma_peak': round(walked / (ms * 1e-3) / FP64_MFMA_PEAK, 3),
                          'floor_ms_at_peak': round(walked / FP64_MFMA_PEAK * 1e3, 3), 'kid': got, 'host_subsets': hs,
                          'host_f64_s_scaled_to_S': round(t64 * S / hs, 2), 'host_f32_s_scaled_to_S': round(t32 * S / hs, 2),
                          'host_threads': torch.get_num_threads(), 'kid_host_f64': k64, 'kid_host_f32': k32, 'kid_kernel_same_subsets': part,
                          'abs_kernel_minus_f64': abs(part - k64), 'abs_host_f32_minus_f64': abs(k32 - k64),
                          'kid_scale_(axx+ayy)/(m-1)/m': scale}), flush=True)
    C = 1008
    w, b = torch.randn(C, 2048, device=dev) * 0.05, torch.randn(C, device=dev) * 0.5
    for B in (16, 64):
        feats = torch.rand(B, 2048, device=dev)
        acc = isc.new_accumulator(10, C, dev)
        splits = (torch.arange(B, device=dev) % 10).to(torch.int32)
        probs = inception.head_probs(feats, w, None)
        t_head, t_acc, t_both = [], [], []
        for _ in range(a.rounds):
            t_head.append(_time(lambda: inception.head_probs(feats, w, None), a.warmup, a.iters * 40) * 1e3)
            t_acc.append(_time(lambda: isc.is_accumulate(acc, probs, splits), a.warmup, a.iters * 40) * 1e3)
            t_both.append(_time(lambda: isc.is_accumulate(acc, inception.head_probs(feats, w, None), splits), a.warmup, a.iters * 40) * 1e3)
        print(json.dumps({'mode': 'head_is', 'batch': B, 'classes': C, 'head_us': _spread(t_head), 'is_accumulate_us': _spread(t_acc),
                          'head_plus_is_us': _spread(t_both), 'head_weight_bytes_read_per_image': C * 2048 * 4}), flush=True)


def loop_mode(a):
    import inception_f64
    from shgan_amd import configs, eval_harness as hz, inception
    dev = 'cuda:0'
    G = configs.seeded_init_(configs.build_generator(a.res), seed=0).eval().requires_grad_(False).to(dev)
    sd = inception_f64.random_state_dict(0)
    sd['fc.weight'], sd['fc.bias'] = torch.randn(1008, 2048) * 0.05, torch.zeros(1008)
    det = inception.InceptionFeatures.from_state_dict(sd, device=dev)
    n = a.batch * a.steps
    forms = {'off': {}, 'kid_is_on': {'kid': True, 'inception_score': dict(num_splits=10)}}

    def once(kw, seed):
        loop = hz.EvalLoop(G, dev, a.res, n, noise_mode='random', seed=0, timing=True, feature_fn=det, fid_real=True, **kw)
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
        once(kw, 1)
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['kernels', 'loop'], default='kernels')
    p.add_argument('--res', type=int, default=512)
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--iters', type=int, default=5)
    p.add_argument('--steps', type=int, default=16)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--host-subsets', type=int, default=4)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('kid_is_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    kernels_mode(a) if a.mode == 'kernels' else loop_mode(a)


if __name__ == '__main__':
    main()
