"""The training tail on the device (sh-gan_amd/optim.py, csrc/optim.hip): ShgAdam and EmaUpdater against the float64 yardstick
(tests/adam_f64.py) with torch's own float32 arithmetic as the measure of what float32 allows, the exact properties (gradient written
back, untouched parameters, repeatability, buffer copies), the prepared-weight cache contract, and the training stage end to end.

Tolerance rule of the float32 results (p, exp_avg, exp_avg_sq, p_ema): the figure of a run is the worst per-tensor ``max |x - ref| /
max |ref|`` over all tensors against the float64 yardstick fed with the same float32 inputs; ours must be <= 2 x the figure of torch's
float32 implementation in the same test (a different but equally valid rounding order; a wrong formula is off by orders of magnitude)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_f64

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAZY = 0.99 ** (16 / 17)            # lazy-regularisation beta2 of the discriminator (d_reg_interval 16)
SHAPES = [(1,), (3,), (4,), (5,), (7, 9), (1023,), (1,), (1025,), ((1 << 20) + 3,), (33, 31), (2, 4096)]


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def special_grad(shape, rs):
    g = rs.standard_normal(shape).astype(np.float32) * np.float32(10.0 ** rs.uniform(-6, 2))
    f = g.reshape(-1)
    vals = np.array([np.nan, np.inf, -np.inf, 1e-41, -3e-39, 0.0, -0.0, 1.17549435e-38], np.float32)
    idx = rs.permutation(f.size)[:min(f.size, len(vals))]
    f[idx] = vals[rs.permutation(len(vals))[:len(idx)]]
    if f.size > 64:
        f[rs.permutation(f.size)[:f.size // 8]] = 0.0             # exact zeros
    return g


def adam_run(world, betas, steps=5, seed=0):
    """ShgAdam over SHAPES for ``steps`` steps; returns what the checks need.  Gradients reach the buckets through autograd
    (sum(p * c) has gradient c exactly, whatever c holds)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim
    from shgan_amd.grad_sync import BucketedAllReduce
    rs = np.random.RandomState(seed)
    init = [rs.standard_normal(s).astype(np.float32) for s in SHAPES]
    params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    ref_params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    sync = BucketedAllReduce(params, bucket_bytes=1 << 21)
    assert len(sync.buckets) >= 3 and any(sync.slot(p)[1] % 2 for p in params)       # a split layout with odd offsets
    lr, eps = 0.002 * 16 / 17, 1e-8
    opt = optim.ShgAdam(params, lr=lr, betas=betas, eps=eps, sync=sync)
    ref = torch.optim.Adam(ref_params, lr=lr, betas=betas, eps=eps, foreach=True, fused=False)
    y = [dict(p=a.astype(np.float64), m=np.zeros(a.shape), v=np.zeros(a.shape), t=0) for a in init]
    for step in range(steps):
        touched = [i for i in range(len(params)) if (i + step) % 3 != 0]         # every parameter sits out one or two steps
        grads = {i: special_grad(SHAPES[i], rs) for i in touched}
        sync.zero_grad()
        with torch.enable_grad():
            sum((params[i] * torch.from_numpy(grads[i]).to(DEV)).sum() for i in touched).backward()
        g_in = {i: params[i].grad.detach().clone() for i in touched}            # what the bucket holds: the input of all three
        for i in touched:
            assert torch.equal(torch.nan_to_num(g_in[i], nan=7.0), torch.nan_to_num(torch.from_numpy(grads[i]).to(DEV), nan=7.0)), i
            assert int(torch.isnan(g_in[i]).sum()) == int(np.isnan(grads[i]).sum())
        before = [b.clone() for b in sync.buckets]
        keep = {i: [t.clone() for t in (params[i], opt.state[params[i]]['exp_avg'], opt.state[params[i]]['exp_avg_sq'], opt.state[params[i]]['step'])]
                for i in range(len(params)) if i not in touched}
        opt.step_from_buckets(world=world)
        # exact: the gradient written back is what finish() leaves
        for b0, b1 in zip(before, sync.buckets):
            want = b0.div_(world) if world > 1 else b0
            want = torch.nan_to_num(want, nan=0.0, posinf=1e5, neginf=-1e5)
            assert torch.equal(bits(want), bits(b1)), f'gradient write-back differs from nan_to_num(bucket.div_({world}))'
        # exact: untouched parameters and their state
        for i, (p0, m0, v0, t0) in keep.items():
            st = opt.state[params[i]]
            assert params[i].grad is None
            assert torch.equal(bits(p0), bits(params[i])) and torch.equal(bits(m0), bits(st['exp_avg'])), i
            assert torch.equal(bits(v0), bits(st['exp_avg_sq'])) and float(t0) == float(st['step']), i
        # torch's float32 Adam and the float64 yardstick on the same float32 bucket values
        for i in range(len(params)):
            ref_params[i].grad = None
        for i in touched:
            g32 = g_in[i].clone()
            g32 = torch.nan_to_num(g32.div_(world) if world > 1 else g32, nan=0.0, posinf=1e5, neginf=-1e5)
            ref_params[i].grad = g32
            g64 = adam_f64.sanitize_f64(g_in[i].cpu().numpy(), world)
            y[i]['p'], y[i]['m'], y[i]['v'], y[i]['t'] = adam_f64.adam_step_f64(y[i]['p'], g64, y[i]['m'], y[i]['v'], y[i]['t'], lr, betas[0], betas[1], eps)
        ref.step()
    torch.cuda.synchronize()
    return params, opt, ref_params, ref, y


@pytest.mark.parametrize('world', [1, 3])
@pytest.mark.parametrize('betas', [(0.0, LAZY), (0.9, 0.999)], ids=['beta1_0_lazy', 'beta1_0.9'])
def test_adam_parity_over_several_steps(world, betas):
    """Five steps over 11 parameters (1 ... 2^20 + 3 elements, three buckets, odd offsets), gradients seeded with NaN, the infinities,
    denormals and zeros, a third of the parameters without a gradient in every step; world divisor driven directly.  The exact checks
    run inside ``adam_run``; here the float32 results against the float64 yardstick under the 2 x rule of the module docstring."""
    params, opt, ref_params, ref, y = adam_run(world, betas)
    ours, theirs = {}, {}
    for key, name in (('p', None), ('m', 'exp_avg'), ('v', 'exp_avg_sq')):
        eo = et = 0.0
        for i, p in enumerate(params):
            a = (p if name is None else opt.state[p][name]).detach().cpu().numpy()
            b = (ref_params[i] if name is None else ref.state[ref_params[i]][name]).detach().cpu().numpy()
            assert np.isfinite(a).all()
            eo, et = max(eo, adam_f64.rel_err(a, y[i][key])), max(et, adam_f64.rel_err(b, y[i][key]))
            assert float(opt.state[p]['step']) == y[i]['t'] == float(ref.state[ref_params[i]]['step'])
        ours[key], theirs[key] = eo, et
        print(f'Adam world={world} betas={betas} {key}: ShgAdam {eo:.3e}, torch float32 {et:.3e} (vs float64 yardstick)')
    for key in ours:
        assert ours[key] <= 2 * theirs[key], (key, ours[key], theirs[key])


def test_adam_two_runs_are_bit_identical():
    a = adam_run(3, (0.9, 0.999), steps=3, seed=4)
    b = adam_run(3, (0.9, 0.999), steps=3, seed=4)
    for p, q in zip(a[0], b[0]):
        assert torch.equal(bits(p), bits(q))
        assert torch.equal(bits(a[1].state[p]['exp_avg']), bits(b[1].state[q]['exp_avg']))
        assert torch.equal(bits(a[1].state[p]['exp_avg_sq']), bits(b[1].state[q]['exp_avg_sq']))


def test_adam_state_dict_loads_into_torch_on_the_device_and_hyper_parameters_follow():
    """After two steps our state dict loads into torch.optim.Adam and both continue alike; a changed lr reaches the device block."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim
    torch.manual_seed(3)
    pa = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in [(5,), (300, 7)]]
    ours = optim.ShgAdam(pa, lr=0.01, betas=(0.9, 0.99))
    for k in range(3):
        ours.zero_grad()
        with torch.enable_grad():
            sum((p * (k + 1.5)).square().sum() for p in pa).backward()
        if k == 2:
            pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
            theirs = torch.optim.Adam(pb, lr=1.0)
            theirs.load_state_dict(ours.state_dict())
            for g in ours.param_groups + theirs.param_groups:
                g['lr'] = 0.05
            for p, q in zip(pa, pb):
                q.grad = p.grad.clone()
            theirs.step()
        ours.step()
    for p, q in zip(pa, pb):
        assert float(ours.state[p]['step']) == 3 == float(theirs.state[q]['step'])
        assert adam_f64.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 1e-6      # (the last step moved them by ~0.05)


class _Net(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES])
        self.register_buffer('f', torch.randn(1029, generator=g))
        self.register_buffer('i32', torch.randint(-2 ** 31, 2 ** 31 - 1, (37,), generator=g, dtype=torch.int64).to(torch.int32))
        self.register_buffer('i64', torch.randint(-2 ** 62, 2 ** 62, (5,), generator=g, dtype=torch.int64))
        self.register_buffer('nanbits', torch.tensor([0x7fc00001, 0x7f800001, -1], dtype=torch.int64).to(torch.int32).view(torch.float32))


def test_ema_one_captured_launch_follows_the_ramp_up():
    """EmaUpdater on a pair of modules (parameters of 1 ... 2^20 + 3 elements; float32, int32, int64 buffers and NaN payloads): ONE
    captured launch replayed with the betas of the ramp-up (0 at the start, then 0.5 ** (batch / (cur_nimg * rampup)), then the
    ema_kimg cap), G moving between the calls.  p_ema against the float64 lerp under the 2 x rule with torch's float32
    ``p.lerp(p_ema, beta)`` as the comparison; buffers bit for bit."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim, train_stage as ts
    G, G_ema, G_ref = _Net(1).to(DEV), _Net(2).to(DEV), _Net(2).to(DEV)
    y = [p.detach().cpu().numpy().astype(np.float64) for p in G_ema.parameters()]
    ema = optim.EmaUpdater(G_ema, G)
    ema.set_beta(0.0)
    ema.capture()
    betas = []
    rs = torch.Generator(device='cpu').manual_seed(9)
    for k, cur_nimg in enumerate([0, 32, 640, 6400, 400000]):
        versions = [p._version for p in G_ema.parameters()]
        beta = ema.update(32, cur_nimg, ema_kimg=10.0, ema_rampup=0.05)
        assert beta == ts.ema_beta(32, cur_nimg, 10.0, 0.05) == ts.update_ema(G_ref, G, 32, cur_nimg, 10.0, 0.05)
        betas.append(beta)
        assert all(p._version > v for p, v in zip(G_ema.parameters(), versions))
        b32 = float(np.float32(beta))
        for i, p in enumerate(G.parameters()):
            y[i] = adam_f64.ema_f64(y[i], p.detach().cpu().numpy(), b32)
        for (n, b), (_, b_ema) in zip(G.named_buffers(), G_ema.named_buffers()):
            assert torch.equal(b.view(torch.int32) if b.element_size() == 4 else b, b_ema.view(torch.int32) if b.element_size() == 4 else b_ema), n
        with torch.no_grad():                            # G moves on
            for p in G.parameters():
                p.add_(torch.randn(p.shape, generator=rs).to(DEV) * 0.01)
            G.f.mul_(1.5)
            G.i64.add_(k)
    assert betas[0] == 0.0 and 0 < betas[1] < 0.5 < betas[3] < betas[4] and len(set(betas)) == 5
    eo = max(adam_f64.rel_err(p.detach().cpu().numpy(), y[i]) for i, p in enumerate(G_ema.parameters()))
    et = max(adam_f64.rel_err(p.detach().cpu().numpy(), y[i]) for i, p in enumerate(G_ref.parameters()))
    print(f'EMA after 5 updates: EmaUpdater {eo:.3e}, torch float32 lerp {et:.3e} (vs float64 yardstick)')
    assert eo <= 2 * et, (eo, et)


def small_networks(seed):
    import shgan_amd  # noqa: F401
    from shgan_amd import configs
    from shgan_amd.model_zoo import stylegan
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=seed,
                             noise_strength=0.1, bias_std=0.1).to(DEV).train().requires_grad_(False)
    for m in G.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    torch.manual_seed(seed + 1)
    D = stylegan.Discriminator(resolution=256, ic_n=4, ch_base=2048, ch_max=32, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train().requires_grad_(False)
    return G, D


def real_batch(n, seed):
    rs = np.random.RandomState(seed)
    real = torch.from_numpy(rs.uniform(-1, 1, size=(n, 3, 256, 256)).astype(np.float32))
    mask = torch.from_numpy((rs.uniform(size=(n, 1, 256, 256)) < 0.7).astype(np.float32))
    return torch.cat([mask - 0.5, real], dim=1).to(DEV)


def gen_forward(G, real4):
    x = torch.cat([real4[:, 0:1], real4[:, 1:4] * (real4[:, 0:1] + 0.5)], dim=1)
    z = torch.from_numpy(np.random.RandomState(1).standard_normal((real4.shape[0], 64)).astype(np.float32)).to(DEV)
    return G(x=x, z=z, c=torch.zeros(real4.shape[0], 0, device=DEV), noise_mode='const')


def test_prepared_weight_caches_follow_the_kernels_writes():
    """The kernels write parameters behind autograd's back.  With ``_ParamCache.guard`` on (every cache hit is checked against the
    parameters' bytes and raises when stale): a forward of G_ema after ``EmaUpdater.update()`` and a forward of G after
    ``ShgAdam.step_from_buckets()`` do not raise and equal the forward after dropping every cache -- the new weights are used."""
    import shgan_amd  # noqa: F401
    from shgan_amd import losses, optim, train_stage as ts
    from shgan_amd.model_zoo.stylegan import _ParamCache
    G, D = small_networks(5)
    G_ema = copy.deepcopy(G).eval()
    real4 = real_batch(2, 6)
    keep, phases = _ParamCache.guard, []
    _ParamCache.guard = True
    try:
        g_before, e_before = gen_forward(G, real4).clone(), gen_forward(G_ema, real4).clone()
        kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
        phases = ts.make_phases(G, D, kw, kw, g_reg_interval=None, d_reg_interval=None, opt_class=optim.ShgAdam)
        L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0)
        torch.manual_seed(3)
        ts.run_phases(real4, 64, phases, batch_idx=0, loss=L, batch_gpu=2, device=DEV)
        g_after = gen_forward(G, real4).clone()                    # guard on: raises if a prepared weight is stale
        ema = optim.EmaUpdater(G_ema, G)
        ema.update(32, 20000, ema_kimg=0.02)                       # beta = 0.5 ** 1.6
        e_after = gen_forward(G_ema, real4).clone()
        _ParamCache.invalidate_all()
        assert torch.equal(g_after, gen_forward(G, real4)) and torch.equal(e_after, gen_forward(G_ema, real4))
        assert not torch.equal(g_after, g_before) and not torch.equal(e_after, e_before) and not torch.equal(e_after, g_after)
    finally:
        _ParamCache.guard = keep
        for ph in phases:
            ph.sync.remove()


ORDER = [0, 1, 2, 4]


def run_stage(opt_class, graphed, order=ORDER, seed=5, nudge=False):
    """``nudge``: every parameter starts one float32 round-off away (each element moved to a neighbouring float32 value, up or down)."""
    from shgan_amd import losses, train_stage as ts
    G, D = small_networks(seed)
    if nudge:
        gen = torch.Generator(device='cpu').manual_seed(99)
        for p in list(G.parameters()) + list(D.parameters()):
            up = (torch.rand(p.shape, generator=gen) < 0.5).to(DEV)
            p.copy_(torch.where(up, torch.nextafter(p, torch.full_like(p, float('inf'))), torch.nextafter(p, torch.full_like(p, float('-inf')))))
    real4 = real_batch(4, 6)
    kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8, capturable=True)
    torch.manual_seed(11)
    L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0)
    phases = ts.make_phases(G, D, kw, kw, g_reg_interval=4, d_reg_interval=16, opt_class=opt_class)
    pg = ts.PhaseGraphs(phases, L, 4, 64, tuple(real4.shape), DEV, warmup=1) if graphed else None
    ran = [pg.run(real4, idx) if graphed else ts.run_phases(real4, 64, phases, batch_idx=idx, loss=L, batch_gpu=4, device=DEV) for idx in order]
    torch.cuda.synchronize()
    out = {n: p.detach().clone() for n, p in list(G.named_parameters()) + [('D.' + n, p) for n, p in D.named_parameters()]}
    for ph in phases:
        ph.sync.remove()
    return out, ran, pg


def test_training_stage_with_shg_adam_follows_torch_adam():
    """Four iterations of all four phases (Greg at 0 and 4, Dreg at 0) from equal seeds with ShgAdam and with torch.optim.Adam.

    Bound.  One ShgAdam step differs from torch's float32 step by round-off (the parity test above: ~1e-7 of a tensor's largest value, no
    more than 2 x torch's own error).  What a perturbation of that size becomes over the following phases is a property of the training
    dynamics, not of the optimiser: with beta1 = 0 an element's update is lr * g / (sqrt(v) + eps), of size lr whatever the size of g,
    so elements whose gradient is near its own round-off noise (zero-initialised biases, the SHU's spectral weights) take steps whose
    direction a one-ulp change upstream decides.  The reference measures that amplification itself: the same torch.optim.Adam stage run
    again with every initial parameter moved to a NEIGHBOURING float32 value (one round-off, once).  The figures are the per-tensor
    ``max |a - b| / max |a|`` against the un-nudged torch run, summarised as median, 90th percentile and worst over the tensors;
    ShgAdam's must be <= 2 x the nudged reference's, each (measured on MI355X: ShgAdam 4.7e-4 / 5.1e-3 / 0.25, nudged torch 1.8e-3 /
    1.7e-2 / 0.40; two torch runs without the nudge are bit-identical).  A wrong formula or wiring (learning rate, bias correction, a
    missed parameter) moves every tensor by ~lr per step and lifts the median by orders of magnitude."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim
    a, ran_a, _ = run_stage(torch.optim.Adam, False)
    b, ran_b, _ = run_stage(optim.ShgAdam, False)
    c, _, _ = run_stage(torch.optim.Adam, False, nudge=True)
    assert ran_a == ran_b and ran_a[0] == ['Gmain', 'Greg', 'Dmain', 'Dreg'] and ran_a[1] == ['Gmain', 'Dmain']
    G0, D0 = small_networks(5)
    init = {n: p.detach() for n, p in list(G0.named_parameters()) + [('D.' + n, p) for n, p in D0.named_parameters()]}
    moved = sum(int(not torch.equal(b[n], init[n])) for n in b)
    assert all(torch.isfinite(t).all() for t in b.values()) and moved > 50

    def figures(x):
        r = sorted(float((a[n] - x[n]).abs().max() / (a[n].abs().max() + 1e-12)) for n in a)
        return r[len(r) // 2], r[int(len(r) * 0.9)], r[-1]
    ours, ref = figures(b), figures(c)
    print(f'after {len(ORDER)} iterations, per-tensor relative difference to torch Adam (median, p90, worst): ShgAdam '
          + ', '.join(f'{v:.2e}' for v in ours) + '; torch Adam from parameters one round-off away ' + ', '.join(f'{v:.2e}' for v in ref)
          + f'; {moved} of {len(b)} tensors moved')
    for o, r in zip(ours, ref):
        assert o <= 2 * r, (ours, ref)


def test_phase_graphs_replay_with_shg_adam_equals_the_eager_loop_bit_for_bit():
    """``PhaseGraphs`` accepts ShgAdam (device step counters by construction): one eager visit per phase, then capture and replays,
    against the eager ShgAdam loop on the same data -- bit-identical parameters."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim
    order = [0, 1, 2, 3, 4, 5]
    a, _, _ = run_stage(optim.ShgAdam, False, order)
    b, _, pg = run_stage(optim.ShgAdam, True, order)
    assert set(pg.graphs) == {'Gmain', 'Dmain', 'Greg'}
    diff = [n for n in a if not torch.equal(bits(a[n]), bits(b[n]))]
    worst = max(float((a[n] - b[n]).abs().max() / (a[n].abs().max() + 1e-12)) for n in a)
    print(f'PhaseGraphs + ShgAdam vs eager ShgAdam: {len(diff)} of {len(a)} tensors differ, worst relative difference {worst:.2e}')
    assert not diff, diff[:5]


def test_phase_graphs_two_ranks_split_form_with_shg_adam():
    """Two ranks (gloo, both on the test box's one device, each with its own data): the split two-graph form (backward graph,
    host-side all-reduce, graph of ShgAdam's tick + stream with the divide by 2 inside) against the eager ShgAdam loop with hook-launched
    reductions: parameters to round-off (the bound of the torch-Adam form of this test in tests/test_gpu_train_graph.py), both ranks
    bit-identical in both forms."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import copy, os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd
from shgan_amd import losses, optim, train_stage as ts
from test_gpu_optim import small_networks, real_batch, DEV
r = int(os.environ["RANK"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=r, world_size=2)
G, D = small_networks(5)
g0, d0 = copy.deepcopy(G.state_dict()), copy.deepcopy(D.state_dict())
init = torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone()
real4 = real_batch(4, 60 + r)                          # per-rank data
kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
order = [0, 1, 2, 4, 5, 8, 9]
out = []
for graphed in (False, True):
    G.load_state_dict(g0); D.load_state_dict(d0)
    torch.manual_seed(11 + r)
    L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode="const", style_mixing_prob=0)
    phases = ts.make_phases(G, D, kw, kw, g_reg_interval=4, d_reg_interval=16, bucket_bytes=1 << 16, opt_class=optim.ShgAdam)
    assert all(ph.sync is ph.opt.sync and ph.sync.reduce and ph.sync.world == 2 and len(ph.sync.buckets) > 1 for ph in phases)
    pg = ts.PhaseGraphs(phases, L, 4, 64, tuple(real4.shape), DEV) if graphed else None
    assert pg is None or pg.split
    for idx in order:
        pg.run(real4, idx) if graphed else ts.run_phases(real4, 64, phases, batch_idx=idx, loss=L, batch_gpu=4, device=DEV)
    torch.cuda.synchronize()
    if graphed:
        assert set(pg.graphs) == {"Gmain", "Greg", "Dmain"} and all(isinstance(g, tuple) and len(g) == 2 for g in pg.graphs.values())
    out.append(torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone())
    for ph in phases:
        ph.sync.remove()
worst = float(((out[0] - out[1]).abs().max() / out[0].abs().max()))
moved = float((out[1] - init).abs().max())
for form in out:                                       # both ranks hold the same parameters, bit for bit
    both = [torch.zeros_like(form.cpu()) for _ in range(2)]
    dist.all_gather(both, form.cpu())
    assert torch.equal(both[0], both[1]), "ranks diverged"
assert torch.isfinite(out[1]).all() and worst < 1e-4 and moved > 0, (worst, moved)
dist.destroy_process_group()
print("rank", r, "ok", "worst %.2e" % worst)
'''
    port = str(40500 + os.getpid() % 2000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), SHG_ROOT=root, SHG_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for rank, p in enumerate(procs):
        o, _ = p.communicate(timeout=1200)
        assert p.returncode == 0 and f'rank {rank} ok'.encode() in o, o.decode()[-3000:]
        print(o.decode().strip().splitlines()[-1])
