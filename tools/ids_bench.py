#!/usr/bin/env python3
"""Timing of U-IDS / P-IDS (sh-gan_amd/ids_score.py, csrc/svm.hip) on one MI355X at the sizes CoModGAN fits: N = 50 000 (FFHQ) and 36 500
(Places2) rows per side, D = 2048, float32.  The features come from the recipe of tests/ids_f64.py (--sep moves U-IDS).

  passes   one 'hv' and one 'grad' call of svm_pass = the pass kernel, the reduction launch and the wrapper's allocations (device events
           around --iters back-to-back calls, 32 ms a window at the defaults; --rounds windows, hv and grad and the two sizes alternating;
           median and min..max; the kernels' own durations come from a kernel trace of this tool run with --fits 0), the bytes of X they
           read computed from the shapes, the achieved rate and its share of the 6.0-6.3 TB/s of an in-order HBM sweep
  fit      the whole ids_from_features (host clock around a call that ends in a device synchronise), its Newton steps and passes, the
           scores; with --sklearn and where sklearn imports, LinearSVC(dual=False) at its default tol on the same arrays, ONE reading
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

HBM_SWEEP = (6.0e12, 6.3e12)


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
    return e0.elapsed_time(e1) / iters * 1e3          # us


def _spread(v):
    return {'median': round(float(np.median(v)), 1), 'min': round(min(v), 1), 'max': round(max(v), 1), 'all': [round(x, 1) for x in v]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', type=int, nargs='+', default=[50000, 36500])
    p.add_argument('--dim', type=int, default=2048)
    p.add_argument('--sep', type=float, default=0.35)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--iters', type=int, default=200)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--fits', type=int, default=3)
    p.add_argument('--sklearn', action='store_true')
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ids_bench: needs a GPU')
    import ids_f64
    import shgan_amd  # noqa: F401
    from shgan_amd import ids_score
    dev, D = 'cuda:0', a.dim
    data, times = {}, {}
    for N in a.sizes:
        real, fake = ids_f64.features(N, D, a.sep, seed=0)
        dr, df = torch.from_numpy(real).to(dev), torch.from_numpy(fake).to(dev)
        v = torch.from_numpy(np.random.RandomState(1).standard_normal(D + 1) / np.sqrt(D)).to(dev)
        act = ids_score.svm_pass(dr, df, v, 'grad')[2]
        data[N], times[N] = (real, fake, dr, df, v, act), {'hv': [], 'grad': []}
    for _ in range(a.rounds):                       # sizes and modes alternate: a drift of the clock shows as spread, not as a difference
        for N in a.sizes:
            _, _, dr, df, v, act = data[N]
            times[N]['hv'].append(_time(lambda: ids_score.svm_pass(dr, df, v, 'hv', a=act), a.warmup, a.iters))
            times[N]['grad'].append(_time(lambda: ids_score.svm_pass(dr, df, v, 'grad'), a.warmup, a.iters))
    for N in a.sizes:
        nbytes = 2 * N * D * 4
        out = {'mode': 'passes', 'N_per_side': N, 'D': D, 'x_bytes': nbytes, 'floor_us_at_6.0_6.3_TBps': [round(nbytes / r * 1e6, 1) for r in HBM_SWEEP]}
        for m in ('hv', 'grad'):
            us = float(np.median(times[N][m]))
            out[f'{m}_us'] = _spread(times[N][m])
            out[f'{m}_TBps'] = round(nbytes / us / 1e6, 3)
            out[f'{m}_share_of_sweep'] = [round(nbytes / (us * 1e-6) / r, 3) for r in HBM_SWEEP]
        print(json.dumps(out), flush=True)
    for N in a.sizes if a.fits > 0 else ():
        real, fake, dr, df, _, _ = data[N]
        ids_score.ids_from_features(dr, df)
        secs = []
        for _ in range(a.fits):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ids_score.ids_from_features(dr, df)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        out = {'mode': 'fit', 'N_per_side': N, 'D': D, 'sep': a.sep, 'ids_from_features_ms': _spread([s * 1e3 for s in secs]), 'newton_iters': res['newton_iters'],
               'passes': res['passes'], 'uids': res['uids'], 'pids': res['pids'], 'grad_norm_over_grad_norm0': res['grad_norm'] / res['grad_norm0']}
        if a.sklearn:
            try:
                from sklearn.svm import LinearSVC
                X, y = np.concatenate([real, fake]), np.concatenate([np.ones(N), -np.ones(N)])
                t0 = time.perf_counter()
                clf = LinearSVC(dual=False).fit(X, y)
                out['sklearn_default_tol_s_single_reading'] = round(time.perf_counter() - t0, 2)
                out['sklearn_uids'] = float(1.0 - clf.score(X, y))
                out['sklearn_pids'] = float(np.mean(clf.decision_function(fake) > clf.decision_function(real)))
                out['host_threads'] = torch.get_num_threads()
            except ImportError:
                out['sklearn_default_tol_s_single_reading'] = 'sklearn does not import on this host'
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
