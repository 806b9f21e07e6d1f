#!/usr/bin/env python3
"""Timing of the tail of FID on one MI355X at the shipped size, D = 2048 (sh-gan_amd/fid_stats.py, csrc/gemm_f64.hip), on synthetic
statistics from the recipe of tests/fid_f64.py (N = 6000 rows per side, decay 12), accumulated by ``FidStats``.

  tail      host: ``mean_cov()`` of both sides (the 2 x 33.6 MB copies included) + ``fid_from_stats`` (scipy's sqrtm), ONE reading;
            device: ``mean_cov_device()`` of both sides + ``frechet_device`` (host clock around calls that end in the read of the last
            trace), --reps readings after one warm-up, the step count and the stop reason; both values against ``frechet_eigh``
  gemm      ``gemm_f64`` alone at n = 2048, batch 1 and batch 2 (the launch of a Newton-Schulz step), device events around --iters calls,
            --rounds windows: TFLOP/s = 2 n^3 batch / time
  matmul    ``torch.matmul`` in float64 at the same size on the same device (rocBLAS), the same windows          } the outside yardsticks: the
  eigvalsh  ``torch.linalg.eigvalsh`` of a symmetric 2048 x 2048 float64 matrix on the device, ONE reading       } product path uses neither

Every step runs in a process of its own under a time limit of its own (--limit seconds).  A step that ends by a signal or at its limit
ends the tool: nothing more is started on a device that may have faulted.  A yardstick that merely cannot run (an exception) is printed
and the tool goes on.  No rate is reported as a share of a peak: no fp64-MFMA rate of this part has been published or measured here, so
the GEMM stands next to rocBLAS.  Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ('tail', 'gemm', 'matmul', 'eigvalsh')
YARDSTICKS = ('matmul', 'eigvalsh')


def _spread(v, nd=3):
    import numpy as np
    return {'median': round(float(np.median(v)), nd), 'min': round(min(v), nd), 'max': round(max(v), nd), 'all': [round(x, nd) for x in v]}


def _windows(fn, a):
    """-> ms per call over --rounds windows of --iters calls between device events."""
    import torch
    for _ in range(a.warmup):
        fn()
    out = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / a.iters)
    return out


def _rate(ms, n, batch):
    return round(2.0 * n ** 3 * batch / (ms * 1e-3) / 1e12, 2)


def step_tail(a):
    import numpy as np
    import torch
    import fid_f64 as ref
    from shgan_amd import fid_stats
    dev, D = 'cuda:0', a.dim
    fake, real = ref.features(D, a.rows, a.decay, 0)
    sides = []
    for x in (fake, real):
        st = fid_stats.FidStats(D, device=dev)
        for k in range(0, a.rows, 1500):
            st.add(torch.from_numpy(x[k:k + 1500]).to(dev))
        sides.append(st)
    torch.cuda.synchronize()

    def device_tail():
        (_, mf, sf), (_, mr, sr) = (s.mean_cov_device() for s in sides)
        return fid_stats.frechet_device(mf, sf, mr, sr)
    device_tail()
    secs = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = device_tail()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    st = sides[0].mean_cov()[1:] + sides[1].mean_cov()[1:]
    t1 = time.perf_counter()
    host = fid_stats.fid_from_stats(*st)
    t2 = time.perf_counter()
    fid, _ = ref.frechet_eigh(*st)
    scale = float(np.trace(st[1]) + np.trace(st[3]))
    dev_ms = _spread([s * 1e3 for s in secs])
    print(json.dumps({'mode': 'tail', 'D': D, 'rows': a.rows, 'decay': a.decay, 'host_threads': torch.get_num_threads(),
                      'host_tail_s_single_reading': round(t2 - t0, 3), 'host_mean_cov_s': round(t1 - t0, 3), 'host_sqrtm_s': round(t2 - t1, 3),
                      'device_tail_ms': dev_ms, 'iterations': res['iterations'], 'stop': res['stop'],
                      'host_over_device': round((t2 - t0) * 1e3 / dev_ms['median'], 1), 'fid_eigh': fid, 'fid_host': host, 'fid_device': res['fid'],
                      'host_minus_eigh_over_traces': abs(host - fid) / scale, 'device_minus_eigh_over_traces': abs(res['fid'] - fid) / scale}), flush=True)


def _operands(a, batch):
    import torch
    g = torch.Generator(device='cuda:0').manual_seed(1)
    shape = (batch, a.dim, a.dim) if batch > 1 else (a.dim, a.dim)
    return (torch.randn(shape, dtype=torch.float64, device='cuda:0', generator=g) for _ in range(3))


def step_gemm(a):
    from shgan_amd import fid_stats
    for batch in (1, 2):
        x, y, out = _operands(a, batch)
        ms = _windows(lambda: fid_stats.gemm_f64(x, y, out=out), a)
        print(json.dumps({'mode': 'gemm_f64', 'n': a.dim, 'batch': batch, 'ms': _spread(ms), 'TFLOPs': _rate(float(sorted(ms)[len(ms) // 2]), a.dim, batch)}),
              flush=True)


def step_matmul(a):
    import torch
    for batch in (1, 2):
        x, y, out = _operands(a, batch)
        ms = _windows(lambda: torch.matmul(x, y, out=out), a)
        print(json.dumps({'mode': 'torch.matmul float64', 'n': a.dim, 'batch': batch, 'ms': _spread(ms),
                          'TFLOPs': _rate(float(sorted(ms)[len(ms) // 2]), a.dim, batch)}), flush=True)


def step_eigvalsh(a):
    import torch
    x, _, _ = _operands(a, 1)
    sym = x @ x.t() / a.dim
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = torch.linalg.eigvalsh(sym)
    torch.cuda.synchronize()
    print(json.dumps({'mode': 'torch.linalg.eigvalsh float64 on the device', 'n': a.dim, 's_single_reading': round(time.perf_counter() - t0, 3),
                      'smallest': float(ev[0]), 'largest': float(ev[-1])}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dim', type=int, default=2048)
    p.add_argument('--rows', type=int, default=6000)
    p.add_argument('--decay', type=float, default=12.0)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--iters', type=int, default=100)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--limit', type=int, default=240, help='seconds per step')
    p.add_argument('--steps', nargs='+', default=list(STEPS), choices=STEPS)
    p.add_argument('--step', choices=STEPS, help='run this one step in this process (what the tool starts for each step)')
    a = p.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('fid_tail_bench: needs a GPU')
        import shgan_amd  # noqa: F401
        globals()['step_' + a.step](a)
        return 0
    passed = [f'--{k}={getattr(a, k)}' for k in ('dim', 'rows', 'decay', 'reps', 'warmup', 'iters', 'rounds')]
    for step in a.steps:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + passed, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({'mode': step, 'error': f'no end within {a.limit} s: stopping'}), flush=True)
            return 124
        if rc < 0 or rc >= 124:                   # a signal (abort, segmentation fault, kill): the device may have faulted
            print(json.dumps({'mode': step, 'error': f'exit status {rc}: stopping'}), flush=True)
            return 1
        if rc != 0:
            print(json.dumps({'mode': step, 'error': f'exit status {rc}' + (' (an outside yardstick: not fatal)' if step in YARDSTICKS else '')}), flush=True)
            if step not in YARDSTICKS:
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
