"""What the maintenance of a training run costs (MEASUREMENTS.md, "Training run maintenance").  Not part of bench.py.

  --part adam   the fused Adam + health pass (shg_adam_buckets_health_f32 + shg_health_reduce_f64) against the plain pass
                (shg_adam_buckets_f32) over the full-width FFHQ-512 G and D parameter sets: arms alternated in one process, device events,
                ``--rounds`` rounds of ``--reps`` steps each.
  --part step   the config-5 step in graph form (train_stage.PhaseGraphs, ShgAdam; Gmain + Dmain) with and without collector + health,
                fp32 and (``--fp16``) fp16 blocks, the same alternation.
  --part tick   single readings: Collector.update(), one snapshot, one 8 x 6 sample grid at 512^2.
The rule printed with every pair: the observed arm is accepted when its median is no slower than the plain arm's median by more than the
plain arm's own max - min in this job.  One JSON line per result."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import shgan_amd  # noqa: E402,F401
from shgan_amd import configs, losses, optim, train_stage as ts, training_stats as tstats  # noqa: E402
from shgan_amd.model_zoo import stylegan  # noqa: E402

DEV = 'cuda:0'


def networks(fp16=False, res=512):
    G = configs.seeded_init_(configs.build_generator(res, **(dict(use_fp16_before_res=64, use_fp16_after_res=32) if fp16 else {})),
                             seed=0).to(DEV).train().requires_grad_(False)
    D = stylegan.Discriminator(resolution=res, ic_n=4, ch_base=32768, ch_max=512, use_fp16_before_res=(32 if fp16 else None),
                               mbstd_group_size=4, mbstd_c_n=1).to(DEV).train().requires_grad_(False)
    return G, D


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def verdict(plain, observed):
    mp, mo = statistics.median(plain), statistics.median(observed)
    spread = max(plain) - min(plain)
    return {'plain_ms_median': round(mp, 4), 'observed_ms_median': round(mo, 4), 'plain_ms_min': round(min(plain), 4),
            'plain_ms_max': round(max(plain), 4), 'observed_ms_min': round(min(observed), 4), 'observed_ms_max': round(max(observed), 4),
            'ratio': round(mo / mp, 4), 'accepted': bool(mo - mp <= spread), 'rounds': len(plain)}


def part_adam(a):
    for name, module in zip(('G', 'D'), networks()):
        arms = {}
        for health in (False, True):
            params = [torch.nn.Parameter(p.detach().clone()) for p in module.parameters()]
            opt = optim.ShgAdam(params, lr=0.002, betas=(0.0, 0.99), eps=1e-8, health=health)
            for b in opt.sync.buckets:
                b.normal_()
            opt.sync._touched = {id(p) for p in params}          # every parameter has a gradient (the buckets were filled directly)

            def step(opt=opt, ids=frozenset(id(p) for p in params)):
                opt.sync._touched = set(ids)
                opt.step_from_buckets()
            step()
            arms[health] = step
        torch.cuda.synchronize()
        t = {False: [], True: []}
        for _ in range(a.rounds):
            for health in (False, True):
                t[health].append(events_ms(arms[health], a.reps))
        n = sum(p.numel() for p in module.parameters())
        print(json.dumps(dict(verdict(t[False], t[True]), part='adam', net=name, params=n, reps=a.reps,
                              what='ShgAdam.step_from_buckets: tick + pass (+ health reduce)')), flush=True)
        del arms


def part_step(a):
    b = a.batch
    real = torch.rand(b, 3, 512, 512, device=DEV) * 2 - 1
    mask = (torch.rand(b, 1, 512, 512, device=DEV) < 0.7).float()
    real4 = torch.cat([mask - 0.5, real], dim=1)
    arms = {}
    for observe in (False, True):
        torch.manual_seed(1234)
        G, D = networks(a.fp16)
        c = tstats.Collector(DEV) if observe else None
        L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='random', style_mixing_prob=0.9, collector=c)
        kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8, health=observe)
        phases = ts.make_phases(G, D, kw, kw, g_reg_interval=4, d_reg_interval=16, opt_class=optim.ShgAdam)
        pg = ts.PhaseGraphs(phases, L, b, 512, tuple(real4.shape), DEV)
        for _ in range(3):
            pg.run(real4, 0)
        for i in (1, 2):
            pg.run(real4, i)
        arms[observe] = pg
    torch.cuda.synchronize()
    t = {False: [], True: []}
    idx = [1, 2, 3]
    for _ in range(a.rounds):
        for observe in (False, True):
            k = iter(idx * a.reps)
            t[observe].append(events_ms(lambda: arms[observe].run(real4, next(k)), a.reps))
    print(json.dumps(dict(verdict(t[False], t[True]), part='step', dtype='f16 blocks + f32' if a.fp16 else 'f32', batch=b, reps=a.reps,
                          what='config-5 step (Gmain + Dmain) as HIP graphs, ShgAdam; observed = collector in the loss + health=True')), flush=True)


def part_tick(a):
    G, D = networks()
    G_ema = networks()[0].eval()
    kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
    phases = ts.make_phases(G, D, kw, kw, opt_class=optim.ShgAdam)
    L = losses.InpaintingLoss(DEV, G, D, composite_fake=True)
    c = tstats.Collector(DEV)
    c.report('x', torch.randn(64, device=DEV))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.update()
    upd = (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        ts.save_snapshot(os.path.join(d, 'network-snapshot-000000.pt'), G, D, G_ema, phases=phases, loss=L, device=DEV,
                         progress=dict(cur_nimg=0, batch_idx=0, cur_tick=0, tick_start_nimg=0))
        snap = (time.perf_counter() - t0) * 1e3
        size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        img = torch.rand(48, 3, 512, 512, device=DEV) * 2 - 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u8 = ts.image_grid(img, (8, 6), (-1, 1))
        torch.cuda.synchronize()
        grid_dev = (time.perf_counter() - t0) * 1e3
        ts.save_image_grid(u8, os.path.join(d, 'fakes000000.png'))
        grid_all = (time.perf_counter() - t0) * 1e3
    print(json.dumps({'part': 'tick', 'single_readings': True, 'collector_update_ms': round(upd, 3), 'snapshot_ms': round(snap, 1),
                      'snapshot_bytes': size, 'grid_8x6_512_kernel_ms': round(grid_dev, 3), 'grid_8x6_512_with_png_ms': round(grid_all, 1)}),
          flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['adam', 'step', 'tick'], required=True)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--fp16', action='store_true')
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error('--rounds >= 5')
    with torch.no_grad():
        {'adam': part_adam, 'step': part_step, 'tick': part_tick}[args.part](args)
