"""Times the ADA pipe (shgan_amd.ada) on the GPU: the fused forward and the adjoint against ADA's literal sequence written with torch's own
operators in float32 on the same device (reflect pad -> zero insertion + conv2d -> affine_grid + grid_sample -> conv2d + stride -> colour
matmul; its backward by torch autograd), and -- with ``--step`` -- Gmain + Dmain of BASELINE config 5 without a pipe, with the ``bgc`` pipe
and with the ``bgc`` pipe on the deterministic (gather-form) adjoint.  The two adjoint routes are timed alternately, ``--rounds`` times
each, in the same process and on the same draws: the scatter kernel with the zero fill of its output, the gather route as all of its
launches (its workspace comes from the caching allocator, as in training).

    python tools/ada_bench.py [--shapes 16x4x512x512,8x4x512x512] [--reps 20] [--warmup 5] [--rounds 5] [--step] [--train-batch 8] [--out FILE]

Both sides get the same matrices and the same margins (the yardstick is handed the integers: ADA's host read-back that sizes the pad is NOT
in its time).  HIP events around ``reps`` back-to-back launches after ``warmup`` untimed ones; one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds


def _fir(x, f, axis):
    n, c, h, w = x.shape
    k = f.reshape(1, 1, -1, 1) if axis == 2 else f.reshape(1, 1, 1, -1)
    return F.conv2d(x.reshape(n * c, 1, h, w), k).reshape(n, c, *([h - 11, w] if axis == 2 else [h, w - 11]))


def torch_sequence(x, G_inv, Cm, margins, f, color):
    """ADA's forward, literally, with torch operators on x's device."""
    n, c, h, w = x.shape
    mx0, my0, mx1, my1 = margins
    dev = x.device

    def mat(rows):
        return torch.tensor(rows, dtype=torch.float32, device=dev)
    x = F.pad(x, [mx0, mx1, my0, my1], mode='reflect')
    G = mat([[1, 0, (mx0 - mx1) / 2], [0, 1, (my0 - my1) / 2], [0, 0, 1]]) @ G_inv
    hp, wp = x.shape[2:]
    z = F.pad(x.reshape(n, c, hp, 1, wp, 1), [0, 1, 0, 0, 0, 1]).reshape(n, c, hp * 2, wp * 2)
    z = F.pad(z, [6, 5, 6, 5])
    fu = (f * 2).flip(0)
    x = _fir(_fir(z, fu, 2), fu, 3)
    G = mat([[2, 0, 0], [0, 2, 0], [0, 0, 1]]) @ G @ mat([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]])
    G = mat([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1]]) @ G @ mat([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]])
    shape = [n, c, (h + 6) * 2, (w + 6) * 2]
    G = mat([[2 / x.shape[3], 0, 0], [0, 2 / x.shape[2], 0], [0, 0, 1]]) @ G @ mat([[shape[3] / 2, 0, 0], [0, shape[2] / 2, 0], [0, 0, 1]])
    grid = F.affine_grid(G[:, :2, :], shape, align_corners=False)
    x = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    x = x[:, :, 1:-1, 1:-1]
    x = _fir(_fir(x, f, 2), f, 3)[:, :, ::2, ::2]
    first, count = color
    img = x[:, first:first + count].reshape(n, count, h * w)
    img = Cm[:, :, :3] @ img + Cm[:, :, 3:]
    return torch.cat([x[:, :first], img.reshape(n, count, h, w), x[:, first + count:]], dim=1)


def bench_ops(shape, reps, warmup, emit, rounds=5):
    from shgan_amd import ada
    n, c, h, w = shape
    dev = 'cuda:0'
    torch.manual_seed(0)
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(dev)
    x = torch.randn(shape, device=dev)
    wgt = torch.randn(shape, device=dev)
    draws = pipe.draw(n, dev)
    G, Cm, margins, color = pipe.params(draws, c, h, w)
    m = [int(v) for v in margins.cpu()]
    f = pipe.Hz_geom
    with torch.no_grad():
        y = ada.ada_apply(x, G, Cm, margins, color)
        ref = torch_sequence(x, G, Cm, m, f, color)
        err = float((y - ref).abs().max())
        t_params = timed(lambda: pipe.params(draws, c, h, w), reps, warmup)
        t_fwd = timed(lambda: ada.ada_apply(x, G, Cm, margins, color), reps, warmup)
        t_adj = timed(lambda: ada.ada_apply_adjoint(wgt, G, Cm, margins, color), reps, warmup)
        t_ref = timed(lambda: torch_sequence(x, G, Cm, m, f, color), max(reps // 4, 2), 2)
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        yr = torch_sequence(xr, G, Cm, m, f, color)
        t_ref_bwd = timed(lambda: torch.autograd.grad(yr, xr, wgt, retain_graph=True), max(reps // 4, 2), 2)
        (gref,) = torch.autograd.grad(yr, xr, wgt)
    gerr = float((ada.ada_apply_adjoint(wgt, G, Cm, margins, color) - gref).abs().max())
    with torch.no_grad():
        det = ada.ada_apply_adjoint(wgt, G, Cm, margins, color, deterministic=True)
        det_err = float((det - gref).abs().max())
        same_bits = bool(torch.equal(det, ada.ada_apply_adjoint(wgt, G, Cm, margins, color, deterministic=True)))
        scatter, gather = [], []
        for _ in range(rounds):
            scatter.append(round(timed(lambda: ada.ada_apply_adjoint(wgt, G, Cm, margins, color), reps, warmup), 1))
            gather.append(round(timed(lambda: ada.ada_apply_adjoint(wgt, G, Cm, margins, color, deterministic=True), reps, warmup), 1))
    from shgan_amd import _lib
    emit(dict(what='ada_adjoint_routes', shape=list(shape), margins=m, scatter_us=scatter, gather_us=gather,
              scatter_median_us=sorted(scatter)[rounds // 2], gather_median_us=sorted(gather)[rounds // 2],
              gather_over_scatter=round(sorted(gather)[rounds // 2] / sorted(scatter)[rounds // 2], 3),
              workspace_bytes=int(_lib.get_lib().shg_ada_adjoint_gather_workspace_bytes(n, c, h, w)), max_abs_diff_gather=det_err,
              gather_same_bits_twice=same_bits, readings=f'{rounds} x {reps} launches, alternating'))
    floor_bytes = 2 * n * c * h * w * 4
    emit(dict(what='ada_ops', shape=list(shape), margins=m, params_us=round(t_params, 1), forward_us=round(t_fwd, 1), adjoint_us=round(t_adj, 1),
              adjoint_includes='zero fill of gx', torch_forward_us=round(t_ref, 1), torch_backward_us=round(t_ref_bwd, 1),
              forward_speedup=round(t_ref / t_fwd, 2), adjoint_speedup=round(t_ref_bwd / t_adj, 2), floor_bytes=floor_bytes,
              forward_floor_GBps=round(floor_bytes / t_fwd / 1e3, 1), max_abs_diff_forward=err, max_abs_diff_adjoint=gerr, readings='single'))


def bench_step(batch, reps, warmup, emit):
    """Gmain + Dmain of config 5 (bench.py train_block's networks and loss) through train_stage.PhaseGraphs, with and without the pipe."""
    from shgan_amd import ada, configs, losses, train_stage as ts
    from shgan_amd.model_zoo import stylegan
    dev = 'cuda:0'
    for spec, det in ((None, False), ('bgc', False), ('bgc', True)):
        torch.manual_seed(1234)
        G = configs.seeded_init_(configs.build_generator(512), seed=0).to(dev).train().requires_grad_(False)
        D = stylegan.Discriminator(resolution=512, ic_n=4, ch_base=32768, ch_max=512, mbstd_group_size=4, mbstd_c_n=1).to(dev).train().requires_grad_(False)
        real = torch.rand(batch, 3, 512, 512, device=dev) * 2 - 1
        mask = (torch.rand(batch, 1, 512, 512, device=dev) < 0.7).float()
        real4 = torch.cat([mask - 0.5, real], dim=1)
        pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS[spec], deterministic=det).to(dev) if spec else None
        L = losses.InpaintingLoss(dev, G, D, composite_fake=True, noise_mode='random', style_mixing_prob=0.9, augment_pipe=pipe)
        kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8, capturable=True, fused=True)
        phases = [ph for ph in ts.make_phases(G, D, kw, kw, g_reg_interval=4, d_reg_interval=16) if ph.name in ('Gmain', 'Dmain')]
        pg = ts.PhaseGraphs(phases, L, batch, 512, tuple(real4.shape), dev)
        for i in range(3):                                   # two eager runs per phase, then capture + first replay
            pg.run(real4, i)
        t = timed(lambda: pg.run(real4, 1), reps, warmup)
        emit(dict(what='config5_Gmain+Dmain', batch=batch, pipe=spec, deterministic=det, ms_per_step=round(t / 1e3, 2), graphs=sorted(pg.graphs), readings='single'))
        for ph in phases:
            if ph.sync is not None:
                ph.sync.remove()
        del pg, L, G, D, phases
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='16x4x512x512,8x4x512x512')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--train-batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import shgan_amd  # noqa: F401
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
    for s in [v for v in a.shapes.split(',') if v]:
        bench_ops(tuple(int(v) for v in s.split('x')), a.reps, a.warmup, emit, a.rounds)
    if a.step:
        bench_step(a.train_batch, max(a.reps // 2, 3), 2, emit)


if __name__ == '__main__':
    main()
