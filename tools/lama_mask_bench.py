"""Micro-benchmark of the LaMa mask path: masks/s of ``masks.lama_masks`` for thin / medium / thick at 256^2 x 32 and 512^2 x 16, with the
host-side record time and the device time apart, beside the freeform sibling ``masks.random_masks`` at the same size and batch and
the host path ``data.LamaMask``, all in one process.  Every figure is the mean over ``reps`` batches after two warm-up batches; the
RNG is re-seeded before each timed window so that the three LaMa rows of a size time the same masks whichever row runs first.
usage: python tools/lama_mask_bench.py [--reps N] [--loop]      (--loop: one EvalLoop reading at 512^2 x 16 per mask kind)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import shgan_amd  # noqa: F401
from shgan_amd import data, masks

dev = 'cuda'


def wall(fn, reps, seed):
    """Mean wall time of fn() in ms, the device drained before the clock starts and before it stops."""
    for _ in range(2):
        fn()
    np.random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def lama_rows(s, n, reps):
    rows = []
    for kind in ('thin', 'medium', 'thick'):
        setting = masks.lama_setting(kind, s)
        total_ms = wall(lambda: masks.lama_masks(n, s, kind, device=dev), reps, seed=1)
        # host: the draws alone (no device work at all)
        np.random.seed(1)
        t0 = time.perf_counter()
        nrec = 0
        batches = []
        for _ in range(reps):
            recs = [masks.lama_mask_records(s, setting) for _ in range(n)]
            nrec += sum(len(r) for r in recs)
            batches.append((np.concatenate(recs), np.cumsum([0] + [len(r) for r in recs])))
        draw_ms = (time.perf_counter() - t0) / reps * 1e3
        # host: checks, quad offsets, staging and the launch call (records ready)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for rec, off in batches:
            masks.lama_rasterize(rec, off, s, dev)
        issue_ms = (time.perf_counter() - t0) / reps * 1e3
        torch.cuda.synchronize()
        # device: copy + kernel of the same batches, HIP events around each call
        evs = []
        for rec, off in batches:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            masks.lama_rasterize(rec, off, s, dev)
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        dev_ms = float(np.median([a.elapsed_time(b) for a, b in evs]))
        # the host path
        np.random.seed(1)
        t0 = time.perf_counter()
        k = max(2, min(n, 8))
        for _ in range(k):
            data.LamaMask(s, kind)
        host_ms = (time.perf_counter() - t0) / k * 1e3
        rows.append(dict(kind='lama_' + kind, s=s, batch=n, masks_per_s=n / total_ms * 1e3, batch_ms=total_ms, host_draw_ms=draw_ms,
                         host_issue_ms=issue_ms, device_event_ms=dev_ms, records_per_mask=nrec / (reps * n), host_path_masks_per_s=1e3 / host_ms))
    return rows


def freeform_row(s, n, reps):
    ms = wall(lambda: masks.random_masks(n, s, (0, 1), device=dev), reps, seed=1)
    return dict(kind='freeform', s=s, batch=n, masks_per_s=n / ms * 1e3, batch_ms=ms)


def loop_rows(reps):
    """EvalLoop at 512^2 x 16 on the full-width generator, default masks and lama_thin, alternating (two readings each), images/s from a host clock around
    run() + synchronise."""
    from shgan_amd import configs, eval_harness as hz
    R, b = 512, 16
    G = configs.seeded_init_(configs.build_generator(R), seed=5).eval().requires_grad_(False).to(dev)
    n_items = b * reps
    out = []
    for rnd in range(3):
        for kind in ('freeform', 'lama_thin'):
            loop = hz.EvalLoop(G, dev, R, n_items, mask_kind=kind, keep_images=True)
            np.random.seed(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=9, pool=4))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:                                   # the first round warms every shape up
                out.append(dict(loop=kind, s=R, batch=b, batches=reps, images_per_s=n_items / dt))
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'lama_mask_bench needs a GPU'
    for s, n in ((256, 32), (512, 16)):
        for row in lama_rows(s, n, a.reps) + [freeform_row(s, n, a.reps)]:
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    if a.loop:
        for row in loop_rows(a.reps):
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
