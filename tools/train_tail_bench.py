#!/usr/bin/env python3
"""The tail of a training iteration on one MI355X, old against new, on the FFHQ-512 parameter sets with random gradients in the buckets.

  old   BucketedAllReduce.finish() (div_ + nan_to_num per bucket; the divide only with --world > 1) + torch.optim.Adam(fused=True,
        capturable=True).step(), and train_stage.update_ema (the per-parameter lerp + copy loop) for G
  new   optim.ShgAdam.step_from_buckets() (shg_adam_tick + shg_adam_buckets_f32), and optim.EmaUpdater.update() (shg_ema_lerp_f32)

Device events around --iters back-to-back calls after --warmup, old and new alternated --rounds times in one process (the median round
is reported, the spread beside it).  GB/s = the bytes a fused pass must move (Adam: read and write g, p, m, v = 32 B/param; EMA: read
p and p_ema, write p_ema = 12 B/param, buffers 8 B/word) over the measured time, for BOTH forms, and its share of the 6.29 TB/s that a
float4 copy kernel reaches on this part.  Every parameter has a gradient (the Gmain / Dmain case).  Prints one JSON line per measurement."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

COPY_CEILING = 6.29e12


def timed(fn, warmup, iters):
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


def report(name, which, times, nbytes, **extra):
    ms = statistics.median(times)
    print(json.dumps(dict(bench='train_tail', case=name, form=which, ms=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                          fused_pass_GBps=round(nbytes / ms / 1e6, 1), share_of_copy_ceiling=round(nbytes / (ms * 1e-3) / COPY_CEILING, 3), **extra)),
          flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--world', type=int, default=1, help='divisor of the gradient average (the arithmetic only: no collective runs)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, optim, train_stage as ts
    from shgan_amd.grad_sync import BucketedAllReduce
    from shgan_amd.model_zoo import stylegan
    dev = torch.device('cuda:0')
    G = configs.seeded_init_(configs.build_generator(a.resolution), seed=0).to(dev).train().requires_grad_(False)
    D = stylegan.Discriminator(resolution=a.resolution, ic_n=4, ch_base=32768, ch_max=512, mbstd_group_size=4, mbstd_c_n=1).to(dev).train().requires_grad_(False)
    kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
    totals = {}
    for name, net in (('G', G), ('D', D)):
        nets = [net, copy.deepcopy(net)]
        n = sum(p.numel() for p in net.parameters())
        syncs = [BucketedAllReduce(list(m.parameters())) for m in nets]
        for s in syncs:
            s.world = a.world
            s._touched = {id(p) for p in s.params}               # every parameter has a gradient
            for b in s.buckets:
                b.normal_()
        old_opt = torch.optim.Adam(list(nets[0].parameters()), fused=True, capturable=True, **kw)
        new_opt = optim.ShgAdam(list(nets[1].parameters()), sync=syncs[1], **kw)
        touched = set(syncs[1]._touched)

        def old():
            syncs[0].finish(reduced=True)
            old_opt.step()

        def new():
            syncs[1]._touched = touched
            new_opt.step_from_buckets(reduced=True)
        to, tn = [], []
        for _ in range(a.rounds):
            to.append(timed(old, a.warmup, a.iters))
            tn.append(timed(new, a.warmup, a.iters))
        nbytes = 32 * n
        mo = report(f'{name} adam ({n / 1e6:.1f} M parameters, {len(syncs[0].buckets)} buckets, world {a.world})', 'old', to, nbytes)
        mn = report(f'{name} adam ({n / 1e6:.1f} M parameters, {len(syncs[0].buckets)} buckets, world {a.world})', 'new', tn, nbytes, speedup=round(mo / statistics.median(tn), 2))
        totals[name] = (mo, mn)
        for s in syncs:
            s.remove()
        if name == 'G':
            ema_old, ema_new = copy.deepcopy(net), copy.deepcopy(net)
            up = optim.EmaUpdater(ema_new, net)
            nb = 12 * n + 8 * sum(b.numel() * b.element_size() // 4 for b in net.buffers())
            to, tn = [], []
            for _ in range(a.rounds):
                to.append(timed(lambda: ts.update_ema(ema_old, net, 32, 100000, 10.0, 0.05), a.warmup, a.iters))
                tn.append(timed(lambda: up.update(32, 100000, 10.0, 0.05), a.warmup, a.iters))
            launches = len(list(net.parameters())) * 2 + len(list(net.buffers()))
            mo = report(f'G_ema update ({launches} launches in the loop)', 'old', to, nb)
            mn = report('G_ema update (1 launch)', 'new', tn, nb, speedup=round(mo / statistics.median(tn), 2))
            totals['ema'] = (mo, mn)
            up.capture()
            tg = [timed(lambda: up.update(32, 100000, 10.0, 0.05), a.warmup, a.iters) for _ in range(a.rounds)]
            report('G_ema update (1 captured launch, replayed)', 'new', tg, nb)
        del nets, syncs, old_opt, new_opt
        torch.cuda.empty_cache()
    old_total, new_total = (sum(v[i] for v in totals.values()) for i in (0, 1))
    print(json.dumps(dict(bench='train_tail', case='G adam + D adam + G_ema', old_ms=round(old_total, 3), new_ms=round(new_total, 3),
                          speedup=round(old_total / new_total, 2))), flush=True)


if __name__ == '__main__':
    main()
