#!/usr/bin/env python3
"""Timing of LPIPS as a training loss (``Lpips.loss``: sh-gan_amd/lpips.py, csrc/lpips_bwd.hip) on one MI355X, full-width networks with
random weights (the rate does not depend on their values).  Stand-alone timing only; one JSON line per measurement.

  --mode loss    per net in --nets and side in --res at batch --batch: forward alone, forward + backward (device events around --iters
                 back-to-back calls after --warmup), their ratio backward / forward; then ONE extra pass with device events around every
                 backward launch, summed per class (dgrad, pool, head, conv1 dgrad); the executed fraction of the fp32-MFMA peak of the
                 dgrad class (the flops of the tile launches, padding not counted, over their time); and the same network through torch's
                 float32 autograd on the device as the baseline.
  --mode gmain   the Gmain phase of the config-5 step (FFHQ-512 SH-GAN, batch --batch, fp32, random-init weights, synthetic data) through
                 ``InpaintingLoss`` without the term, with the VGG perceptual term, and with the perceptual and L1 terms."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FULL = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
PEAK_F32_MFMA = 157.3e12


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


def _state_dict(net):
    import lpips_f64
    import ppl_f64
    return ppl_f64.vgg_random_state_dict(FULL, seed=0) if net == 'vgg' else lpips_f64.random_state_dict(0)


def _torch_loss(net, sd, fake, real):
    """The same network in plain torch float32 on the device (the baseline)."""
    import lpips_f64
    import ppl_f64
    sh = torch.tensor(lpips_f64.SHIFT, device=fake.device).reshape(1, 3, 1, 1)
    sc = torch.tensor(lpips_f64.SCALE, device=fake.device).reshape(1, 3, 1, 1)

    def taps(x):
        x, out = (x - sh) / sc, []
        if net == 'vgg':
            for k, (s, i) in enumerate(zip(ppl_f64.VGG_SLICE_OF, ppl_f64.VGG_CONV_IDS)):
                x = F.relu(F.conv2d(x, sd[f'net.slice{s}.{i}.weight'], sd[f'net.slice{s}.{i}.bias'], padding=1))
                if k in ppl_f64.VGG_TAPS:
                    out.append(x)
                    if k != ppl_f64.VGG_TAPS[-1]:
                        x = F.max_pool2d(x, 2, 2)
            return out
        for n, (key, _, _, _, s, p) in enumerate(lpips_f64.CONVS):
            if n in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, sd[f'{key}.weight'], sd[f'{key}.bias'], stride=s, padding=p))
            out.append(x)
        return out

    def norm(f):
        return f / ((f ** 2).sum(dim=1, keepdim=True).clamp_min(1e-30).sqrt() + 1e-10)
    with torch.no_grad():
        tr = taps(real)
    return sum((sd[f'lin{n}.model.1.weight'] * (norm(a) - norm(b)) ** 2).sum(dim=1).mean(dim=(1, 2)) for n, (a, b) in enumerate(zip(taps(fake), tr)))


def _dgrad_flops(net, n, B, H, W):
    """Flops of the dgrad launches on the tile for ONE backward: 2 * the multiply-adds of the pred half's stride-1 convolutions."""
    from shgan_amd import lpips
    if net == 'vgg':
        return 2 * B * lpips.vgg_macs_per_image(n.widths, H, W)
    hs, ws = lpips.out_sizes(H), lpips.out_sizes(W)
    return 2 * B * sum(hs[k] * ws[k] * o * i * ks * ks for k, (i, o, ks, _, _) in enumerate(lpips.CONVS) if k > 0)


def loss_mode(a):
    from shgan_amd import lpips
    dev = 'cuda:0'
    for net in a.nets:
        sd = _state_dict(net)
        n = lpips.LPIPS(net=net, state_dict=sd, device=dev)
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        for res in a.res:
            g = torch.Generator(device=dev).manual_seed(0)
            real = torch.rand(a.batch, 3, res, res, device=dev, generator=g) * 2 - 1
            fake = (real + 0.3 * torch.randn(a.batch, 3, res, res, device=dev, generator=g)).clamp(-1, 1).requires_grad_(True)

            def fwd():
                with torch.no_grad():
                    return n.loss(fake, real)

            def both(loss_fn=n.loss):
                with torch.enable_grad():
                    (gr,) = torch.autograd.grad(loss_fn(fake, real).mean(), fake)
                return gr
            ms_f, ms_fb = _time(fwd, a.warmup, a.iters), _time(both, a.warmup, a.iters)
            # one more pass with events around every backward launch
            spans, names = [], ('dgrad', 'maxpool_bwd', 'head_bwd', 'conv1_dgrad')
            keep = {name: getattr(lpips, name) for name in names}

            def timed(name):
                def call(*args, **kw):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = keep[name](*args, **kw)
                    e1.record()
                    spans.append((name, e0, e1))
                    return out
                return call
            try:
                for name in names:
                    setattr(lpips, name, timed(name))
                both()
                torch.cuda.synchronize()
            finally:
                for name in names:
                    setattr(lpips, name, keep[name])
            cls = {name: round(sum(e0.elapsed_time(e1) for k, e0, e1 in spans if k == name), 3) for name in names}
            flops = _dgrad_flops(net, n, a.batch, res, res)
            row = {'mode': 'loss', 'net': net, 'res': res, 'batch': a.batch, 'ms_forward': round(ms_f, 3), 'ms_forward_backward': round(ms_fb, 3),
                   'ms_backward': round(ms_fb - ms_f, 3), 'backward_over_forward': round((ms_fb - ms_f) / ms_f, 3), 'ms_backward_classes': cls,
                   'ms_backward_rest': round(ms_fb - ms_f - sum(cls.values()), 3), 'dgrad_flops': flops,
                   'dgrad_fraction_of_fp32_mfma_peak': round(flops / (cls['dgrad'] * 1e-3) / PEAK_F32_MFMA, 4)}
            print(json.dumps(row), flush=True)
            ms_t = _time(lambda: both(lambda x, y: _torch_loss(net, sd_dev, x, y)), a.warmup, a.iters)
            print(json.dumps({'mode': 'loss', 'net': net, 'res': res, 'batch': a.batch, 'ms_forward_backward_torch_f32': round(ms_t, 3),
                              'hip_over_torch': round(ms_fb / ms_t, 3)}), flush=True)


def gmain_mode(a):
    from shgan_amd import configs, losses, lpips
    from shgan_amd.model_zoo import stylegan
    dev = 'cuda:0'
    G = configs.seeded_init_(configs.build_generator(a.resolution), seed=0).to(dev).train()
    for m in G.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    D = stylegan.Discriminator(resolution=a.resolution, ic_n=4, ch_base=32768, ch_max=512, mbstd_group_size=4, mbstd_c_n=1).to(dev).train()
    G.requires_grad_(True)
    D.requires_grad_(False)
    n = lpips.LPIPS(net='vgg', state_dict=_state_dict('vgg'), device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    real = torch.rand(a.batch, 3, a.resolution, a.resolution, device=dev, generator=g) * 2 - 1
    mask = (torch.rand(a.batch, 1, a.resolution, a.resolution, device=dev, generator=g) < 0.7).float()
    real4 = torch.cat([mask - 0.5, real], dim=1)
    z, cnd = torch.randn(a.batch, 512, device=dev, generator=g), torch.zeros(a.batch, 0, device=dev)
    base = None
    for what, kw in (('adversarial', {}), ('adversarial + perceptual', dict(perceptual=n, perceptual_weight=1.0)),
                     ('adversarial + perceptual + l1', dict(perceptual=n, perceptual_weight=1.0, l1_weight=1.0))):
        L = losses.InpaintingLoss(dev, G, D, composite_fake=True, noise_mode='random', **kw)

        def phase():
            G.zero_grad(set_to_none=True)
            L.accumulate_gradients('Gmain', real4, cnd, z, cnd, sync=True, gain=1)
        ms = _time(phase, a.warmup, a.iters)
        base = ms if base is None else base
        print(json.dumps({'mode': 'gmain', 'resolution': a.resolution, 'batch': a.batch, 'terms': what, 'ms_per_phase': round(ms, 3),
                          'over_adversarial': round(ms / base, 3)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['loss', 'gmain'], default='loss')
    p.add_argument('--nets', nargs='+', default=['vgg', 'alex'])
    p.add_argument('--res', type=int, nargs='+', default=[512, 256])
    p.add_argument('--resolution', type=int, default=512)
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--iters', type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_loss_bench: needs a GPU')
    import shgan_amd  # noqa: F401
    loss_mode(a) if a.mode == 'loss' else gmain_mode(a)


if __name__ == '__main__':
    main()
