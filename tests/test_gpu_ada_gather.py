"""The gather-form adjoint of the ADA geometry (``deterministic=True``: shgan_amd.ada, csrc/ada.hip ada_cot_kernel + ada_gather_kernel) on the
device: the values against the float64 restatement under the tolerance rule of tests/test_gpu_ada.py (``4 e32 + 2^-22 max|y|``), and what
the route is for -- the same bits on every run, under every content of a fresh allocation, for every batch a sample is part of, through
autograd, the pipes, a loss phase and a captured graph.  The cases, inputs and references are those of tests/test_gpu_ada.py."""
import numpy as np
import pytest
import torch

import ada_f64 as R
import ada_tail_f64 as RT
from alloc_fill import filled
from test_gpu_ada import SHAPES, _pinned, bound, case, check, dev_args
from test_gpu_ada_tail import _pinned as _pinned_full

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v       # noqa: E731


@pytest.fixture(scope='module')
def ada():
    import shgan_amd  # noqa: F401
    from shgan_amd import ada as mod
    return mod


# ---- values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.AFFINE_KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_values(ada, shape, kind):
    """A^T w of the gather route against float64 autograd of the restatement, and <A x, w> = <x, A^T w> with the forward kernel (the limit of
    test_gpu_ada.test_adjoint: each side within its bound of the exact operator)."""
    c = case(shape, kind)
    a = dev_args(c)
    x, w = c['x'].to(DEV), c['w'].to(DEV)
    r64, r32 = c['ref'][torch.float64], c['ref'][torch.float32]
    atw = ada.ada_apply_adjoint(w, deterministic=True, **a)
    b_g = check(f'gather adjoint {shape} {kind}', atw, r64['atw'], r32['atw'])
    geo = ada.ada_apply_adjoint(w, G_inv=a['G_inv'], margins=a['margins'], deterministic=True)            # geometry alone
    first, count = c['ch']
    other = [i for i in range(shape[1]) if not first <= i < first + count]
    assert torch.equal(atw[:, other], geo[:, other])
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


def test_colour_alone_is_the_colour_kernel(ada):
    c = case((2, 3, 16, 24), 'identity')
    w = c['w'].to(DEV)
    kw = dict(Cm=c['Cm'].to(DEV), color_channels=c['ch'])
    assert torch.equal(ada.ada_apply_adjoint(w, deterministic=True, **kw), ada.ada_apply_adjoint(w, **kw))


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
BIT_KINDS = ('rot_aniso_frac', 'zoom_out4', 'zoom_in2', 'mixed')


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_bits_do_not_depend_on_the_run_or_on_stale_memory(ada, shape):
    """Two calls are bit-equal; so is the call under each fill of tests/alloc_fill.py (the output and the workspace are ``torch.empty``:
    both are read only where written) and the call whose output lands in a block that held NaN."""
    for kind in BIT_KINDS:
        c = case(shape, kind)
        a = dev_args(c)
        w = c['w'].to(DEV)
        first = ada.ada_apply_adjoint(w, deterministic=True, **a)
        assert torch.equal(first, ada.ada_apply_adjoint(w, deterministic=True, **a)), kind
        for pattern in ('zero', 'nan', 'big'):
            with filled(pattern) as rec:
                got = ada.ada_apply_adjoint(w, deterministic=True, **a)
                torch.cuda.synchronize()
            assert ('ada.py', '_launch') in rec.sites and rec.count == 2            # the output and the workspace
            assert torch.equal(got, first), (kind, pattern)
        del got
        torch.cuda.synchronize()
        stale = torch.full(shape, float('nan'), device=DEV)                       # the allocator hands this block to the next output
        del stale
        assert torch.equal(ada.ada_apply_adjoint(w, deterministic=True, **a), first), kind
        assert bool(torch.isfinite(first).all())


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[0] > 1], ids=ids)
def test_a_sample_has_the_same_bits_alone_as_in_the_batch(ada, shape):
    c = case(shape, 'mixed')
    a = dev_args(c)
    w = c['w'].to(DEV)
    full = ada.ada_apply_adjoint(w, deterministic=True, **a)
    for n in range(shape[0]):
        one = ada.ada_apply_adjoint(w[n:n + 1].contiguous(), G_inv=a['G_inv'][n:n + 1], Cm=a['Cm'][n:n + 1], margins=a['margins'],
                                    color_channels=a['color_channels'], deterministic=True)
        assert torch.equal(one, full[n:n + 1]), n


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,kind', [(s, 'rot_aniso_frac') for s in SHAPES] + [((2, 4, 24, 16), 'zoom_out4'), ((2, 3, 16, 24), 'mixed')], ids=ids)
def test_backward_is_the_adjoint_call_and_the_forward_is_unchanged(ada, shape, kind):
    c = case(shape, kind)
    a = dev_args(c)
    x, w = c['x'].to(DEV), c['w'].to(DEV)
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        y = ada.ada_apply(xr, deterministic=True, **a)
        (gx,) = torch.autograd.grad((y * w).sum(), xr)
    assert torch.equal(y.detach(), ada.ada_apply(x, **a)) and torch.equal(y.detach(), ada.ada_apply(x, deterministic=False, **a))
    assert torch.equal(gx, ada.ada_apply_adjoint(w, deterministic=True, **a))


@pytest.mark.parametrize('shape,kind', [(s, 'rot_aniso_frac') for s in SHAPES] + [((2, 3, 16, 24), k) for k in R.AFFINE_KINDS if k != 'rot_aniso_frac'],
                         ids=ids)
def test_second_order(ada, shape, kind):
    """test_gpu_ada.test_second_order on the deterministic route: the backward of the adjoint node is still the forward kernel."""
    c = case(shape, kind)
    a = dev_args(c)
    with torch.enable_grad():
        x = c['x'].to(DEV).requires_grad_(True)
        w = c['w'].to(DEV).requires_grad_(True)
        (g,) = torch.autograd.grad((ada.ada_apply(x, deterministic=True, **a) * w).sum(), x, create_graph=True)
        assert g.requires_grad and type(g.grad_fn).__name__.startswith('_AdaAdjointFn')
        assert torch.equal(g.detach(), ada.ada_apply_adjoint(c['w'].to(DEV), deterministic=True, **a))
        g.square().sum().backward()
    assert x.grad is None or float(x.grad.abs().max()) == 0.0
    check(f'second order, gather {shape} {kind}', w.grad, c['ref'][torch.float64]['g2'], c['ref'][torch.float32]['g2'])


# ---- routing ----------------------------------------------------------------------------------------------------------------------------
def _routing_matrix(name):
    if name == 'far':                                     # beyond ADA_GATHER_HMAX: a 64-fold magnification
        return R.scale2d(1 / 64, 1 / 64, torch.float64)
    if name == 'singular':
        return torch.tensor([[1.0, 2.0, 0.5], [0.5, 1.0, -0.25], [0.0, 0.0, 1.0]], dtype=torch.float64)
    m = torch.eye(3, dtype=torch.float64)
    m[0, 1] = float('nan')
    return m


@pytest.mark.parametrize('name', ['far', 'singular', 'nan'])
def test_samples_the_gather_does_not_take(ada, name):
    """A matrix whose window is unbounded, mixed into a batch with an ordinary sample: the scatter kernel behind the gather handles it.
    Finite, within the rule of the restatement (a NaN matrix: exact zeros, as the forward gives), and the ordinary sample keeps the bits it
    has alone."""
    shape = (2, 3, 16, 16)
    rs = np.random.RandomState(41)
    w = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    Cm = (torch.eye(4)[:3].expand(2, 3, 4) + 0.1 * torch.from_numpy(rs.standard_normal((2, 3, 4)).astype(np.float32))).contiguous()
    G = torch.stack([R.affine('rot_aniso_frac', 1, 16, 16)[0], _routing_matrix(name)]).float()
    finite = G[:1] if name == 'nan' else G
    m = tuple(int(v) for v in R.margins_pre(finite.double(), 16, 16).ceil())
    a = dict(G_inv=G.to(DEV), Cm=Cm.to(DEV), margins=torch.tensor(m, dtype=torch.int32, device=DEV), color_channels=(0, 3))
    got = ada.ada_apply_adjoint(w.to(DEV), deterministic=True, **a)
    assert bool(torch.isfinite(got).all())
    keep = 1 if name == 'nan' else 2
    ref = [R.adjoint(w[:keep].to(dt), (keep, 3, 16, 16), G_inv=G[:keep].to(dt), C34=Cm[:keep].to(dt), channels=(0, 3), margins=m)
           for dt in (torch.float64, torch.float32)]
    check(f'routing {name}', got[:keep], ref[0], ref[1])
    if name == 'nan':
        assert float(got[1].abs().max()) == 0.0
        y = ada.ada_apply(w.to(DEV), **dict(a, Cm=None, color_channels=None))
        assert float(y[1].abs().max()) == 0.0                                    # the forward: every weight zero
    else:
        assert float(got[1].abs().max()) > 0.0
    alone = ada.ada_apply_adjoint(w[:1].to(DEV), G_inv=a['G_inv'][:1], Cm=a['Cm'][:1], margins=a['margins'], color_channels=(0, 3),
                                  deterministic=True)
    assert torch.equal(alone, got[:1])
    assert torch.equal(ada.ada_apply_adjoint(w.to(DEV), deterministic=True, **a)[:1], got[:1])


# ---- the pipes and a loss ---------------------------------------------------------------------------------------------------------------
def _pipe_grad(pipe, x, w, draws):
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((pipe(xr, draws) * w).sum(), xr)
    return gx


def test_pipe_gradients_are_the_same_bits_twice(ada):
    """``AugmentPipe`` (bgc) and ``FullAugmentPipe`` (bgcfnc) with ``deterministic=True`` on pinned draws: the input gradient is bit-equal
    in two runs and within the rule of the float64 transpose built from the parameters the device computed (the reference the default
    route's gradient is held to as well)."""
    shape = (4, 4, 32, 24)
    rs = np.random.RandomState(51)
    x0, w0 = (torch.from_numpy(rs.standard_normal(shape).astype(np.float32)) for _ in range(2))
    x, w = x0.to(DEV), w0.to(DEV)
    for full in (False, True):
        if full:
            pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc'], deterministic=True).to(DEV)
            draws = _pinned_full(4, 22, (3, 32, 24))(4)
        else:
            pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc'], deterministic=True).to(DEV)
            draws = _pinned(ada, 4, 5)(4)
        assert pipe.deterministic
        g1, g2 = _pipe_grad(pipe, x, w, draws), _pipe_grad(pipe, x, w, draws)
        assert torch.equal(g1, g2) and float(g1.abs().max()) > 0
        G, Cm, margins, color = pipe.params(draws, 4, 32, 24)
        m = tuple(int(v) for v in margins.cpu())
        tail = {}
        if full:
            Hz, _, cut = pipe.tail_params(draws)
            tail = dict(Hz=Hz.cpu(), cut=cut.cpu())
        ref = []
        for dt in (torch.float64, torch.float32):
            wt = w0.to(dt)
            if full:
                wt = RT.adjoint(wt, Hz=tail['Hz'].to(dt), cut=tail['cut'], channels=color)
            ref.append(R.adjoint(wt, shape, G_inv=G.cpu().to(dt), C34=Cm.cpu().to(dt), channels=color, margins=m))
        check(f'pipe gradient, full={full}', g1, ref[0], ref[1])
        off = type(pipe)(**(ada.AUGPIPE_SPECS_FULL['bgcfnc'] if full else ada.AUGPIPE_SPECS['bgc'])).to(DEV)
        assert torch.equal(off(x, draws), pipe(x, draws))                       # the forward does not know the flag
        check(f'pipe gradient of the default route, full={full}', _pipe_grad(off, x, w, draws), ref[0], ref[1])


def test_stylegan2_gmain_gradients_are_bit_reproducible(ada):
    """``StyleGAN2Loss`` on the 32 x 32 toy networks of test_gpu_ada.test_stylegan2_loss_with_the_pipe, the deterministic pipe, pinned draws:
    Gmain twice from the same state (same seed for the latents' path) gives every parameter gradient bit for bit."""
    from shgan_amd import losses
    from shgan_amd.model_zoo import stylegan as sg
    torch.manual_seed(3)
    mp = sg.Mapping(z_dim=32, c_dim=0, w_dim=32, num_ws=8, num_layers=3, lr_multiplier=0.01, w_avg_beta=0.995)
    syn = sg.Synthesis(w_dim=32, resolution=32, rgb_n=3, ch_base=256, ch_max=16, use_fp16_after_res=32)
    G = sg.Generator(mp, syn).to(DEV).train()
    D = sg.Discriminator(resolution=32, ic_n=3, ch_base=256, ch_max=16, use_fp16_before_res=None, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train()
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc'], deterministic=True).to(DEV)
    L = losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=pipe, style_mixing_prob=0)
    L.draw_fn = _pinned(ada, 8, 5)
    z, real, cnd = torch.randn(4, 32, device=DEV), torch.randn(4, 3, 32, 32, device=DEV), torch.zeros(4, 0, device=DEV)
    G.requires_grad_(True), D.requires_grad_(False)
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    runs = []
    for _ in range(2):
        G.load_state_dict(state)
        G.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        L.stats.clear()
        L.accumulate_gradients('Gmain', real, cnd, z, cnd, sync=True, gain=1)
        runs.append({n: p.grad.detach().clone() for n, p in G.named_parameters() if p.grad is not None})
    assert runs[0] and sorted(runs[0]) == sorted(runs[1]) and any(float(t.abs().max()) > 0 for t in runs[0].values())
    differ = [n for n in runs[0] if not torch.equal(runs[0][n], runs[1][n])]
    assert not differ, differ


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_the_same_bits_from_one_graph(ada):
    """One ``torch.cuda.graph`` of the deterministic pipe's forward + backward on static draws (one stream; the workspace comes from the
    graph's pool): two replays are bit-equal, and equal to the eager result."""
    shape = (4, 3, 32, 32)
    rs = np.random.RandomState(9)
    x = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(DEV).requires_grad_(True)
    w = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(DEV)
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc'], deterministic=True).to(DEV)
    draws = _pinned(ada, 4, 13)(4)

    def step():
        with torch.enable_grad():
            y = pipe(x, draws)
            (gx,) = torch.autograd.grad((y * w).sum(), x)
        return y.detach(), gx
    y0, g0 = (t.clone() for t in step())
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
    gx.fill_(float('nan'))
    graph.replay()
    y2, g2 = y.clone(), gx.clone()
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    assert torch.equal(y1, y0) and torch.equal(g1, g0) and float(g0.abs().max()) > 0
