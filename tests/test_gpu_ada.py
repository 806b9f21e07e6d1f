"""The ADA pipe on the device (shgan_amd.ada, csrc/ada.hip) against the literal restatement of ADA's sequence (tests/ada_f64.py, checked
on the CPU by tests/test_ada_cpu.py).

Tolerance rule (not fixed in advance): every comparison runs the restatement twice on the CPU, in float64 and in float32;
``e32 = max |f32 - f64|`` is the reference's own float32 error on that case, and the device must lie within ``4 e32 + 2^-22 max|y|`` of the
float64 result (4: the fused weights and the LDS-staged adjoint sum in another order than torch's five passes).  Each test prints the
observed ratio device / e32."""
import numpy as np
import pytest
import torch

import ada_f64 as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(3, 1, 16, 16), (2, 3, 16, 24), (2, 4, 24, 16), (2, 3, 64, 64), (1, 4, 40, 72)]
_REF = {}


@pytest.fixture(scope='module')
def ada():
    import shgan_amd  # noqa: F401
    from shgan_amd import ada as mod
    return mod


def bound(y64, y32):
    e32 = float((y32.double() - y64).abs().max())
    return 4 * e32 + 2.0 ** -22 * float(y64.abs().max()), e32


def check(name, dev, y64, y32):
    b, e32 = bound(y64, y32)
    err = float((dev.detach().double().cpu() - y64).abs().max())
    print(f'{name}: device error {err:.2e}, reference float32 error {e32:.2e}, ratio {err / max(e32, 1e-30):.2f}, bound {b:.2e}')
    assert err <= b, (name, err, e32, b)
    return b


def channels_of(C):
    return {1: (0, 1), 3: (0, 3), 4: (1, 3)}[C]


def case(shape, kind):
    """Inputs and both reference runs of one (shape, matrix) case, computed once: x, w, G_inv, colour matrix, margins; y, A^T w and
    2 A A^T w in float64 and float32."""
    key = (shape, kind)
    if key not in _REF:
        N, C, H, W = shape
        rs = np.random.RandomState(sum(shape) + len(kind))
        x = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        w = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        G = R.affine(kind, N, H, W).float()                     # the float32 matrices are THE inputs of both sides
        Cm = (torch.eye(4)[:3].expand(N, 3, 4) + 0.1 * torch.from_numpy(rs.standard_normal((N, 3, 4)).astype(np.float32))).contiguous()
        ch = channels_of(C)
        m = tuple(int(v) for v in R.margins_pre(G.double(), H, W).ceil())
        ref = {}
        for dt in (torch.float64, torch.float32):
            kw = dict(G_inv=G.to(dt), C34=Cm.to(dt), channels=ch, margins=m)
            ref[dt] = dict(y=R.apply(x.to(dt), **kw), geo=R.apply(x.to(dt), G_inv=G.to(dt), margins=m), atw=R.adjoint(w.to(dt), shape, **kw),
                           g2=R.second_order_wgrad(w.to(dt), shape, **kw))
        _REF[key] = dict(x=x, w=w, G=G, Cm=Cm, ch=ch, m=m, ref=ref)
    return _REF[key]


def dev_args(c):
    return dict(G_inv=c['G'].to(DEV), Cm=c['Cm'].to(DEV), margins=torch.tensor(c['m'], dtype=torch.int32, device=DEV), color_channels=c['ch'])


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
PARAM_CASES = [(k,) for k in R.GEOM_KEYS + R.COLOR_KEYS] + [R.GEOM_KEYS + R.COLOR_KEYS]
LATTICE = {('xflip',), ('rotate90',), ('xint',)} | {(k,) for k in R.COLOR_KEYS}       # G_inv is a signed permutation + integer shift
PARAM_SEED = 0


def _draws(seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.uniform(size=(8, 24)).astype(np.float32)), torch.from_numpy(rs.standard_normal((8, 8)).astype(np.float32))


def _away(v):
    """distance of every element of v from the nearest multiple of 0.5"""
    v = np.asarray(v, dtype=np.float64) * 2
    return np.abs(v - np.round(v)) / 2


@pytest.mark.parametrize('keys', PARAM_CASES, ids=lambda k: '+'.join(k) if len(k) < 3 else 'all')
def test_params_kernel_matches_the_restatement(ada, keys):
    """16 x 24, N = 8 fixed draws, p = 1 and multiplier 1 (every gate open), each transform alone and all together: G_inv and the colour
    matrix within the tolerance rule, the margins equal.

    Integer decisions.  The draws (PARAM_SEED, chosen on the CPU) keep the float64 restatement's pre-``round`` integer-translation products
    and pre-``ceil`` margins at least 1e-3 away from an integer and from a half wherever a continuous transform takes part.  Where the
    geometry is a pure blit (flip, quarter turns, integer shift alone -- and the colour-only cases, whose geometry is the identity) G_inv
    is a signed permutation with an integer shift and the margin IS an integer up to the float64 rounding of cos(pi / 2) = 6e-17: no
    choice of draws moves it away, so those cases assert instead that the value sits within 1e-9 of an integer; the kernel evaluates the
    same float64 expression and must take the same ``ceil``."""
    H, W = 16, 24
    u, g = _draws(PARAM_SEED)
    cfg = {k: 1 for k in keys}
    r64, r32 = R.params(u, g, 1.0, cfg, H, W, torch.float64), R.params(u, g, 1.0, cfg, H, W, torch.float32)
    pre = R.margins_pre(r64['G_inv'], H, W).numpy()
    unclamped = (pre > 0) & (pre < np.array([W - 1, H - 1] * 2))
    if tuple(keys) in LATTICE:
        assert np.abs(pre - np.round(pre)).max() <= 1e-9, pre
    else:
        assert _away(pre[unclamped]).min(initial=1.0) >= 1e-3, pre
    fired = r64['xint_pre'].numpy()
    assert _away(fired[fired != 0]).min(initial=1.0) >= 1e-3, fired
    pipe = ada.AugmentPipe(**cfg).to(DEV)
    G, Cm, margins, color = pipe.params((u.to(DEV), g.to(DEV)), 3, H, W)
    assert color == (0, 3)
    assert [int(v) for v in margins.cpu()] == [int(v) for v in np.ceil(pre)]
    check('G_inv ' + '+'.join(keys), G, r64['G_inv'], r32['G_inv'])
    check('colour ' + '+'.join(keys), Cm, r64['C'], r32['C'])
    # one colour channel: hue and saturation do not exist
    G1, Cm1, _, _ = pipe.params((u.to(DEV), g.to(DEV)), 1, H, W)
    c64, c32 = R.params(u, g, 1.0, cfg, H, W, torch.float64, color_count=1), R.params(u, g, 1.0, cfg, H, W, torch.float32, color_count=1)
    check('colour (1 channel) ' + '+'.join(keys), Cm1, c64['C'], c32['C'])
    assert torch.equal(G1, G)


def test_params_gates_closed_at_p_zero(ada):
    u, g = _draws(PARAM_SEED)
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    pipe.p.zero_()
    G, Cm, margins, _ = pipe.params((u.to(DEV), g.to(DEV)), 3, 16, 24)
    assert torch.equal(G.cpu(), torch.eye(3).expand(8, 3, 3)) and torch.equal(Cm.cpu(), torch.eye(4)[:3].expand(8, 3, 4))
    assert [int(v) for v in margins.cpu()] == [6, 6, 6, 6]


# ---- the image operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.AFFINE_KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_apply_forward(ada, shape, kind):
    c = case(shape, kind)
    a = dev_args(c)
    x = c['x'].to(DEV)
    y = ada.ada_apply(x, **a)
    check(f'forward {shape} {kind}', y, c['ref'][torch.float64]['y'], c['ref'][torch.float32]['y'])
    geo = ada.ada_apply(x, G_inv=a['G_inv'], margins=a['margins'])
    check(f'geometry alone {shape} {kind}', geo, c['ref'][torch.float64]['geo'], c['ref'][torch.float32]['geo'])
    first, count = c['ch']
    other = [i for i in range(shape[1]) if not first <= i < first + count]
    assert torch.equal(y[:, other], geo[:, other])                       # the mask channel of C = 4: colour leaves its bits alone


def test_pass_through_paths_are_bit_exact(ada):
    c = case((2, 4, 24, 16), 'identity')
    x = c['x'].to(DEV)
    assert ada.ada_apply(x) is x
    off = ada.AugmentPipe().to(DEV)
    assert off(x) is x
    col = ada.ada_apply(x, Cm=c['Cm'].to(DEV), color_channels=(1, 3))    # geometry off: every other channel is copied
    assert torch.equal(col[:, 0], x[:, 0])
    for dt in (torch.float64, torch.float32):
        c['ref'][dt]['col'] = R.color(c['x'].to(dt), c['Cm'].to(dt), (1, 3))
    check('colour alone', col, c['ref'][torch.float64]['col'], c['ref'][torch.float32]['col'])
    one = ada.ada_apply(x, Cm=c['Cm'].to(DEV), color_channels=(2, 1))
    assert torch.equal(one[:, [0, 1, 3]], x[:, [0, 1, 3]])
    check('colour alone, one channel', one, R.color(c['x'].double(), c['Cm'].double(), (2, 1)), R.color(c['x'], c['Cm'], (2, 1)))
    geo_only = ada.AugmentPipe(xflip=1, rotate90=1, xint=1).to(DEV)      # colour multipliers 0: the colour stage is skipped
    u, g = _draws(3)
    u, g = u[:2].to(DEV), g[:2].to(DEV)
    G, _, margins, _ = geo_only.params((u, g), 4, 24, 16)
    assert torch.equal(geo_only(x, (u, g)), ada.ada_apply(x, G_inv=G, margins=margins))
    col_only = ada.AugmentPipe(brightness=1, contrast=1, saturation=1).to(DEV)
    assert torch.equal(col_only(x, (u, g))[:, 0], x[:, 0])


@pytest.mark.parametrize('kind', R.AFFINE_KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adjoint(ada, shape, kind):
    """A^T w against float64 autograd of the restatement, and <A x, w> = <x, A^T w> on the device results summed in float64: each side is
    within its tolerance of the exact operator, for which the identity holds, so they differ by at most sum|w| b_y + sum|x| b_g."""
    c = case(shape, kind)
    a = dev_args(c)
    x, w = c['x'].to(DEV), c['w'].to(DEV)
    r64, r32 = c['ref'][torch.float64], c['ref'][torch.float32]
    atw = ada.ada_apply_adjoint(w, **a)
    b_g = check(f'adjoint {shape} {kind}', atw, r64['atw'], r32['atw'])
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((ada.ada_apply(xr, **a) * w).sum(), xr)
    check(f'backward {shape} {kind}', gx, r64['atw'], r32['atw'])
    lin64 = R.apply(c['x'].double(), G_inv=c['G'].double(), C34=c['Cm'].double(), channels=c['ch'], margins=c['m'], bias=False)
    lin32 = R.apply(c['x'], G_inv=c['G'], C34=c['Cm'], channels=c['ch'], margins=c['m'], bias=False)
    b_y, _ = bound(lin64, lin32)
    zero_bias = c['Cm'].clone()
    zero_bias[:, :, 3] = 0
    y_lin = ada.ada_apply(x, **dict(a, Cm=zero_bias.to(DEV)))
    lhs, rhs = float((y_lin.double() * w.double()).sum()), float((x.double() * atw.double()).sum())
    lim = float(w.double().abs().sum()) * b_y + float(x.double().abs().sum()) * b_g
    print(f'<Ax, w> - <x, A^T w> = {lhs - rhs:.3e} (limit {lim:.3e})')
    assert abs(lhs - rhs) <= lim


@pytest.mark.parametrize('shape,kind', [(s, 'rot_aniso_frac') for s in SHAPES] + [((2, 3, 16, 24), k) for k in R.AFFINE_KINDS if k != 'rot_aniso_frac'],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_second_order(ada, shape, kind):
    """g = grad((pipe(x) * w).sum(), x, create_graph=True); g.square().sum().backward(): w.grad = 2 A A^T w (the backward of the adjoint node
    is the forward kernel) against the restatement (tests/ada_f64.second_order_wgrad), the shape of the R1 regulariser."""
    c = case(shape, kind)
    a = dev_args(c)
    with torch.enable_grad():
        x = c['x'].to(DEV).requires_grad_(True)
        w = c['w'].to(DEV).requires_grad_(True)
        (g,) = torch.autograd.grad((ada.ada_apply(x, **a) * w).sum(), x, create_graph=True)
        assert g.requires_grad and type(g.grad_fn).__name__.startswith('_AdaAdjointFn')
        g.square().sum().backward()
    assert x.grad is None or float(x.grad.abs().max()) == 0.0           # linear in x: nothing of second order flows into it
    check(f'second order {shape} {kind}', w.grad, c['ref'][torch.float64]['g2'], c['ref'][torch.float32]['g2'])


# ---- the losses -----------------------------------------------------------------------------------------------------------------------
def _pinned(ada, n_max, seed):
    rs = np.random.RandomState(seed)
    u = torch.from_numpy(rs.uniform(size=(n_max, 24)).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rs.standard_normal((n_max, 8)).astype(np.float32)).to(DEV)
    return lambda n: (u[:n], g[:n])


def test_stylegan2_loss_with_the_pipe(ada):
    from shgan_amd import losses
    from shgan_amd.model_zoo import stylegan as sg
    torch.manual_seed(3)
    mp = sg.Mapping(z_dim=32, c_dim=0, w_dim=32, num_ws=8, num_layers=3, lr_multiplier=0.01, w_avg_beta=0.995)
    syn = sg.Synthesis(w_dim=32, resolution=32, rgb_n=3, ch_base=256, ch_max=16, use_fp16_after_res=32)
    G = sg.Generator(mp, syn).to(DEV).train()
    D = sg.Discriminator(resolution=32, ic_n=3, ch_base=256, ch_max=16, use_fp16_before_res=None, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train()
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    L = losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=pipe, style_mixing_prob=0)
    assert L.draw_fn == pipe.draw
    L.draw_fn = _pinned(ada, 8, 5)
    z, real, cnd = torch.randn(4, 32, device=DEV), torch.randn(4, 3, 32, 32, device=DEV), torch.zeros(4, 0, device=DEV)
    fake = torch.randn(4, 3, 32, 32, device=DEV)
    assert torch.equal(L.run_D(real, cnd), D(pipe(real, L.draw_fn(4)), cnd))
    gl, rl = L.run_D_pair(fake, cnd, real, cnd)
    both = D(pipe(torch.cat([fake, real]), L.draw_fn(8)), torch.cat([cnd, cnd]), segments=2)
    assert torch.equal(gl, both[:4]) and torch.equal(rl, both[4:])
    assert not torch.equal(L.run_D(real, cnd), D(real, cnd))
    for phase in losses.PHASES:
        G.zero_grad(set_to_none=True), D.zero_grad(set_to_none=True)
        mod = G if phase.startswith('G') else D
        G.requires_grad_(mod is G), D.requires_grad_(mod is D)
        L.stats.clear()
        L.accumulate_gradients(phase, real, cnd, z, cnd, sync=True, gain=1)
        grads = [p.grad for p in mod.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(t).all()) for t in grads) and any(float(t.abs().max()) > 0 for t in grads), phase
        if phase in ('Dmain', 'Dboth'):
            s = L.stats['Loss/signs/real']
            assert s.shape == (4, 1) and torch.equal(s, L.stats['Loss/scores/real'].sign())
    L2 = losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=pipe, style_mixing_prob=0, batch_critic=False)
    D.requires_grad_(True)
    L2.accumulate_gradients('Dmain', real, cnd, z, cnd)
    assert 'Loss/signs/real' in L2.stats
    with pytest.raises(NotImplementedError):
        losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=object())


def test_inpainting_loss_with_the_pipe(ada):
    from shgan_amd import configs, losses
    from shgan_amd.model_zoo import stylegan
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1).to(DEV).train().requires_grad_(False)
    torch.manual_seed(6)
    D = stylegan.Discriminator(resolution=256, ic_n=4, ch_base=2048, ch_max=32, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train().requires_grad_(False)
    rs = np.random.RandomState(7)
    real = torch.from_numpy(rs.uniform(-1, 1, size=(2, 3, 256, 256)).astype(np.float32))
    mask = torch.from_numpy((rs.uniform(size=(2, 1, 256, 256)) < 0.7).astype(np.float32))
    real4 = torch.cat([mask - 0.5, real], dim=1).to(DEV)
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0, augment_pipe=pipe)
    L.draw_fn = _pinned(ada, 4, 8)
    cnd = torch.zeros(2, 0, device=DEV)
    fake = torch.randn(2, 3, 256, 256, device=DEV)
    L._m05 = real4[:, 0:1]
    fake4 = torch.cat([real4[:, 0:1], fake], dim=1)
    assert torch.equal(L.run_D(fake, cnd), D(pipe(fake4, L.draw_fn(2)), cnd))              # the mask channel is prepended first
    assert torch.equal(L.run_D(real4, cnd), D(pipe(real4, L.draw_fn(2)), cnd))
    gl, rl = L.run_D_pair(fake, cnd, real4, cnd)
    both = D(pipe(torch.cat([fake4, real4]), L.draw_fn(4)), torch.cat([cnd, cnd]), segments=2)
    assert torch.equal(gl, both[:2]) and torch.equal(rl, both[2:])
    L._m05 = None
    z = torch.randn(2, 64, device=DEV)
    for phase in losses.PHASES:
        G.zero_grad(set_to_none=True), D.zero_grad(set_to_none=True)
        mod = G if phase.startswith('G') else D
        mod.requires_grad_(True)
        L.accumulate_gradients(phase, real4, cnd, z, cnd, sync=True, gain=1)
        mod.requires_grad_(False)
        grads = [p.grad for p in mod.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(t).all()) for t in grads), phase
    assert 'Loss/signs/real' in L.stats


# ---- graph capture --------------------------------------------------------------------------------------------------------------------
def test_pipe_forward_and_backward_replay_from_one_graph(ada):
    """One ``torch.cuda.graph`` of pipe forward + backward (one stream, no branches): replays draw again, and read ``p`` from the device --
    after ``p.zero_()`` a replay is the identity transform, held to the tolerance rule on the restatement's identity case."""
    shape = (4, 3, 32, 32)
    rs = np.random.RandomState(9)
    x0, w0 = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)), torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    x = x0.to(DEV).requires_grad_(True)
    w = w0.to(DEV)

    def step():
        with torch.enable_grad():
            y = pipe(x)
            (gx,) = torch.autograd.grad((y * w).sum(), x)
        return y.detach(), gx
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, gx = step()
    graph.replay()
    y1, g1 = y.clone(), gx.clone()
    graph.replay()
    y2, g2 = y.clone(), gx.clone()
    assert not torch.equal(y1, y2) and not torch.equal(g1, g2)          # fresh draws
    assert bool(torch.isfinite(y1).all() and torch.isfinite(g1).all())
    pipe.p.zero_()
    graph.replay()
    eye = torch.eye(3, dtype=torch.float64).expand(4, 3, 3)
    i64, i32 = R.geometry(x0.double(), eye)[0], R.geometry(x0, eye.float())[0]
    check('replay at p = 0, forward', y, i64, i32)
    a64, a32 = R.adjoint(w0.double(), shape, G_inv=eye), R.adjoint(w0, shape, G_inv=eye.float())
    check('replay at p = 0, backward', gx, a64, a32)
    assert float((y.cpu() - x0).abs().max()) <= 4 * float((i32 - x0).abs().max()) + 2.0 ** -22 * float(x0.abs().max())
