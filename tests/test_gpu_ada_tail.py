"""The tail of the ADA pipe on the device (shgan_amd.ada.FullAugmentPipe, csrc/ada_tail.hip: image-space filter, noise, cutout) against
the literal restatement of ADA's sequence (tests/ada_tail_f64.py, checked on the CPU by tests/test_ada_tail_cpu.py).

Tolerance rule, the one of tests/test_gpu_ada.py: every comparison runs the restatement twice on the CPU, in float64 and in float32;
``e32 = max |f32 - f64|`` is the reference's own float32 error on that case, and the device must lie within ``4 e32 + 2^-22 max|y|`` of the
float64 result.  Each test prints the observed ratio device / e32.  The float32 parameters (taps, sigma, box, noise field) are THE inputs
of both sides; which pixels a cutout erases is decided by ADA's float32 compares on both sides, and the cases keep every compare at least
1e-6 away from equality (asserted in float64)."""
import numpy as np
import pytest
import torch

import ada_tail_f64 as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(2, 3, 22, 22), (3, 1, 24, 40), (2, 4, 32, 24), (1, 3, 70, 90), (1, 4, 130, 66)]
KINDS = ('filter', 'noise', 'cutout', 'all', 'mixed')
_REF = {}


def ids(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


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


def cut_margin(cut, H, W):
    """the smallest distance of a cutout compare from equality, in float64"""
    dx, dy = R.cutout_terms(cut.double(), H, W, torch.float64)
    return min(float(dx.abs().min()), float(dy.abs().min()))


def case(shape, kind):
    """Inputs and both reference runs of one (shape, kind) case, computed once: x, w, the float32 parameters; y, A^T w and 2 A A^T w in
    float64 and float32.  ``mixed``: the filter with the last sample's band gates all closed (its taps are the exact impulse)."""
    key = (shape, kind)
    if key not in _REF:
        N, C, H, W = shape
        rs = np.random.RandomState(sum(shape) + len(kind))
        x = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        w = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        ch = channels_of(C)
        ut = torch.from_numpy(rs.uniform(size=(N, 8)))
        gt = torch.from_numpy(rs.standard_normal((N, 5)))
        if kind == 'mixed':
            ut[N - 1, :4] = 2.0                                   # no band gate of the last sample fires
        pr = R.params(ut, gt, 1.0, dict(imgfilter=1, noise=1, cutout=1, cutout_size=0.45), torch.float64)
        Hz = pr['Hz'].float()
        closed = ~pr['fired'].any(dim=1)
        Hz[closed] = torch.eye(R.TAPS)[R.PAD]                     # what the parameter kernel writes for such a sample
        a = dict(Hz=None, sigma=None, z=None, cut=None)
        if kind in ('filter', 'all', 'mixed'):
            a['Hz'] = Hz
        if kind in ('noise', 'all'):
            a['sigma'] = pr['sigma'].float()
            a['z'] = torch.from_numpy(rs.standard_normal((N, ch[1], H, W)).astype(np.float32))
        if kind in ('cutout', 'all'):
            a['cut'] = pr['cut'].float()
            assert cut_margin(a['cut'], H, W) >= 1e-6
        lin = dict(Hz=a['Hz'], cut=a['cut'])
        ref = {}
        for dt in (torch.float64, torch.float32):
            def to(t):
                return None if t is None else t.to(dt)
            ref[dt] = dict(y=R.apply(x.to(dt), Hz=to(a['Hz']), sigma=to(a['sigma']), z=to(a['z']), cut=a['cut'], channels=ch))
            if kind != 'noise':
                kw = dict(Hz=to(lin['Hz']), cut=lin['cut'], channels=ch)
                ref[dt].update(lin=R.apply(x.to(dt), bias=False, **kw), atw=R.adjoint(w.to(dt), **kw), g2=R.second_order_wgrad(w.to(dt), **kw))
        _REF[key] = dict(x=x, w=w, ch=ch, a=a, lin=lin, closed=closed, ref=ref)
    return _REF[key]


def dev(d):
    return {k: (None if v is None else v.to(DEV)) for k, v in d.items()}


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
PARAM_CASES = {
    'filter': (1.0, dict(imgfilter=1)),
    'noise': (1.0, dict(noise=1)),
    'cutout': (1.0, dict(cutout=1)),
    'all': (1.0, dict(imgfilter=1, noise=1, cutout=1)),
    'bands_p_half': (0.5, dict(imgfilter=1, imgfilter_bands=(1, 0, 0.5, 1), noise=1, cutout=1)),
}
PARAM_SEED = 0


def _draws(seed, n=8):
    """fixed draws; the uniform ones stay inside [0.002, 0.998] (a gate threshold of 0 or 1 is at least 1e-3 away)"""
    rs = np.random.RandomState(seed)
    ut = torch.from_numpy(rs.uniform(0.002, 0.998, size=(n, 8)).astype(np.float32))
    return ut, torch.from_numpy(rs.standard_normal((n, 5)).astype(np.float32))


@pytest.mark.parametrize('name', list(PARAM_CASES))
def test_params_kernel_matches_the_restatement(ada, name):
    """N = 8 fixed draws, every gate draw at least 1e-3 from its threshold (asserted first): taps, sigma and the box under the tolerance
    rule; a sample none of whose band gates fired has the exact impulse."""
    p, cfg = PARAM_CASES[name]
    ut, gt = _draws(PARAM_SEED)
    thr = np.array(R.thresholds(p, cfg))
    assert np.abs(ut[:, :6].double().numpy() - thr[None, :]).min() >= 1e-3
    r64, r32 = R.params(ut, gt, p, cfg, torch.float64), R.params(ut, gt, p, cfg, torch.float32)
    assert torch.equal(r64['fired'], r32['fired'])
    pipe = ada.FullAugmentPipe(**cfg).to(DEV)
    pipe.p.fill_(p)
    Hz, sigma, cut = pipe.tail_params((None, None, ut.to(DEV), gt.to(DEV)))
    assert Hz.shape == (8, 43) and sigma.shape == (8,) and cut.shape == (8, 4)
    check(f'Hz {name}', Hz, r64['Hz'], r32['Hz'])
    check(f'sigma {name}', sigma, r64['sigma'], r32['sigma'])
    check(f'cut {name}', cut, r64['cut'], r32['cut'])
    closed = ~r64['fired'].any(dim=1)
    if name == 'bands_p_half':
        assert 0 < int(closed.sum()) < 8 and not bool(r64['fired'][:, 1].any()) and 0 < int((r64['sigma'] > 0).sum()) < 8
        assert 0 < int((r64['cut'][:, 2] > 0).sum()) < 8
    if 'imgfilter' not in cfg:
        assert bool(closed.all())
    assert torch.equal(Hz.cpu()[closed], torch.eye(43)[21].expand(int(closed.sum()), 43))
    assert torch.equal((sigma.cpu() == 0), (r64['sigma'] == 0)) and torch.equal((cut.cpu()[:, 2:] == 0), (r64['cut'][:, 2:] == 0))


def test_params_gates_closed_at_p_zero(ada):
    ut, gt = _draws(PARAM_SEED)
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc']).to(DEV)
    pipe.p.zero_()
    Hz, sigma, cut = pipe.tail_params((None, None, ut.to(DEV), gt.to(DEV)))
    assert torch.equal(Hz.cpu(), torch.eye(43)[21].expand(8, 43))
    assert torch.equal(sigma.cpu(), torch.zeros(8)) and torch.equal(cut.cpu()[:, 2:], torch.zeros(8, 2))
    assert torch.equal(cut.cpu()[:, :2], ut[:, 6:8])


# ---- the image operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_apply_forward(ada, shape, kind):
    c = case(shape, kind)
    x = c['x'].to(DEV)
    y = ada.ada_tail_apply(x, color_channels=c['ch'], **dev(c['a']))
    check(f'forward {shape} {kind}', y, c['ref'][torch.float64]['y'], c['ref'][torch.float32]['y'])
    N, C, H, W = shape
    first, count = c['ch']
    if kind == 'mixed':                                                  # all band gates closed: the sample's bits pass
        n = N - 1
        assert bool(c['closed'][n]) and torch.equal(y[n], x[n])
        if N > 1:
            assert not torch.equal(y[0, first:first + count], x[0, first:first + count])
    if C == 4:
        if kind in ('filter', 'noise', 'mixed'):
            assert torch.equal(y[:, 0], x[:, 0])                          # the mask channel is neither filtered nor given noise
        if kind in ('cutout', 'all'):
            m = R.cutout_mask(c['a']['cut'], H, W, torch.float32)[:, 0].to(DEV)
            assert int((m == 0).sum()) > 0 and torch.equal(y[:, 0], x[:, 0] * m)
            assert torch.equal(y[:, 0] == 0, m == 0)


def test_pass_through_paths(ada):
    c = case((2, 4, 32, 24), 'all')
    x = c['x'].to(DEV)
    assert ada.ada_tail_apply(x) is x and ada.ada_tail_apply_adjoint(x) is x
    off = ada.FullAugmentPipe().to(DEV)
    assert off(x) is x
    with pytest.raises(ValueError):
        ada.ada_tail_apply(x, sigma=c['a']['sigma'].to(DEV))
    # the linear part (what the second-order route runs): the kernel with bias = 0 drops the noise term
    a = dev(c['a'])
    y_lin = ada._AdaTailApplyFn.apply(x, a['Hz'], a['sigma'], a['z'], a['cut'], c['ch'], False)
    check('linear part', y_lin, c['ref'][torch.float64]['lin'], c['ref'][torch.float32]['lin'])
    assert torch.equal(y_lin, ada.ada_tail_apply(x, Hz=a['Hz'], cut=a['cut'], color_channels=c['ch']))


@pytest.mark.parametrize('shape', [(2, 4, 32, 24), (1, 3, 70, 90)], ids=ids)
def test_kernels_write_every_element_of_their_results(ada, shape):
    """The three entry points called on result buffers that hold NaN: every element is written, and with the bits a zero-filled buffer gets
    (filtered planes, copied planes and the ragged last tiles alike).  ``ada.py`` hands them zero-filled buffers; nothing relies on that."""
    import ctypes
    from shgan_amd import _lib
    lib = _lib.get_lib()
    N, C, H, W = shape
    c = case(shape, 'mixed' if C == 4 else 'all')
    a = dev(case(shape, 'all')['a'])
    a['Hz'] = c['a']['Hz'].to(DEV)
    x = c['x'].to(DEV)
    first, count = c['ch']
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    res = {}
    for fill in (0.0, float('nan')):
        y, gx = torch.full_like(x, fill), torch.full_like(x, fill)
        _lib.check(lib.shg_ada_tail_apply_f32(p(x), p(a['Hz']), p(a['sigma']), p(a['z']), p(a['cut']), p(y), N, C, H, W, first, count, 1, st), 'apply')
        _lib.check(lib.shg_ada_tail_adjoint_f32(p(x), p(a['Hz']), p(a['cut']), p(gx), N, C, H, W, first, count, st), 'adjoint')
        Hz, sigma, cut = (torch.full(s, fill, device=DEV) for s in ((N, 43), (N,), (N, 4)))
        pipe = ada.FullAugmentPipe(imgfilter=1, noise=1, cutout=1).to(DEV)
        ut, gt = _draws(PARAM_SEED, N)
        ut, gt = ut.to(DEV), gt.to(DEV)
        _lib.check(lib.shg_ada_tail_params_f32(p(ut), p(gt), p(pipe.p.reshape(1)), ctypes.byref(pipe._tail_config()), p(Hz), p(sigma), p(cut),
                                               N, st), 'params')
        res[fill == 0.0] = (y, gx, Hz, sigma, cut)
    for zero, poisoned in zip(res[True], res[False]):
        assert bool(torch.isfinite(poisoned).all()) and torch.equal(zero, poisoned)
    assert torch.equal(res[True][0], ada.ada_tail_apply(x, color_channels=c['ch'], **a))


def test_cutout_decisions(ada):
    """Boxes over every image edge, one inside, one closed gate: the set of zeroed pixels equals the restatement's mask exactly."""
    N, C, H, W = 6, 3, 24, 40
    half = np.float32(0.5) / 2
    cut = torch.tensor([[0.0613, 0.5127, half, half], [0.9441, 0.4713, half, half], [0.5219, 0.0331, half, half],
                        [0.4877, 0.9907, half, half], [0.5127, 0.4713, half, half], [0.3, 0.7, 0.0, 0.0]], dtype=torch.float32)
    assert cut_margin(cut, H, W) >= 1e-6
    dx, dy = R.cutout_terms(cut.double(), H, W, torch.float64)
    inside_x, inside_y = dx < 0, dy < 0
    assert bool(inside_x[0, 0]) and bool(inside_x[1, W - 1]) and bool(inside_y[2, 0]) and bool(inside_y[3, H - 1])       # over each edge
    assert not bool(inside_x[4, 0] or inside_x[4, W - 1] or inside_y[4, 0] or inside_y[4, H - 1]) and not bool(inside_x[5].any())
    rs = np.random.RandomState(11)
    x = torch.from_numpy((rs.uniform(0.5, 1.5, size=(N, C, H, W)) * rs.choice([-1.0, 1.0], size=(N, C, H, W))).astype(np.float32))
    assert int((x == 0).sum()) == 0
    mask = R.cutout_mask(cut, H, W, torch.float32)
    assert torch.equal(mask, R.cutout_mask(cut, H, W, torch.float64).float())
    assert torch.equal(mask == 0, (inside_x[:, None, None, :] & inside_y[:, None, :, None]))
    y = ada.ada_tail_apply(x.to(DEV), cut=cut.to(DEV)).cpu()
    assert torch.equal(y == 0, (mask == 0).expand(N, C, H, W))
    assert torch.equal(y, x * mask)
    erased = (mask == 0).flatten(1).sum(dim=1)
    assert int(erased[5]) == 0 and all(int(v) > 0 for v in erased[:5]) and int(erased[4]) > int(erased[0])


LINEAR = [(s, k) for s in SHAPES for k in ('all', 'mixed')] + [((2, 3, 22, 22), 'filter'), ((2, 4, 32, 24), 'cutout'), ((1, 3, 70, 90), 'filter')]


@pytest.mark.parametrize('shape,kind', LINEAR, ids=ids)
def test_adjoint(ada, shape, kind):
    """A^T w against float64 autograd of the restatement, and <A x, w> = <x, A^T w> on the device results summed in float64: each side is
    within its tolerance of the exact operator, for which the identity holds, so they differ by at most sum|w| b_y + sum|x| b_g.  The
    adjoint is a gather: two runs give the same bits."""
    c = case(shape, kind)
    a = dev(c['lin'])
    x, w = c['x'].to(DEV), c['w'].to(DEV)
    r64, r32 = c['ref'][torch.float64], c['ref'][torch.float32]
    atw = ada.ada_tail_apply_adjoint(w, color_channels=c['ch'], **a)
    b_g = check(f'adjoint {shape} {kind}', atw, r64['atw'], r32['atw'])
    assert torch.equal(atw, ada.ada_tail_apply_adjoint(w, color_channels=c['ch'], **a))
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((ada.ada_tail_apply(xr, color_channels=c['ch'], **dev(c['a'])) * w).sum(), xr)
    assert torch.equal(gx, atw)                                          # the noise term does not reach the gradient
    b_y, _ = bound(r64['lin'], r32['lin'])
    y_lin = ada.ada_tail_apply(x, color_channels=c['ch'], **a)
    lhs, rhs = float((y_lin.double() * w.double()).sum()), float((x.double() * atw.double()).sum())
    lim = float(w.double().abs().sum()) * b_y + float(x.double().abs().sum()) * b_g
    print(f'<Ax, w> - <x, A^T w> = {lhs - rhs:.3e} (limit {lim:.3e})')
    assert abs(lhs - rhs) <= lim
    if kind in ('filter', 'all'):                                        # not self-adjoint: the reflected pad folds back
        assert float((r64['atw'] - R.apply(c['w'].double(), bias=False, Hz=c['lin']['Hz'].double(), cut=c['lin']['cut'],
                                           channels=c['ch'])).abs().max()) > 1e-3


@pytest.mark.parametrize('shape,kind', [(s, 'all') for s in SHAPES] + [((2, 3, 22, 22), 'mixed')], ids=ids)
def test_second_order(ada, shape, kind):
    """g = grad((tail(x) * w).sum(), x, create_graph=True); g.square().sum().backward(): w.grad = 2 A A^T w (the backward of the adjoint node
    is the forward kernel without the noise term) against the restatement, the shape of the R1 regulariser."""
    c = case(shape, kind)
    with torch.enable_grad():
        x = c['x'].to(DEV).requires_grad_(True)
        w = c['w'].to(DEV).requires_grad_(True)
        (g,) = torch.autograd.grad((ada.ada_tail_apply(x, color_channels=c['ch'], **dev(c['a'])) * w).sum(), x, create_graph=True)
        assert g.requires_grad and type(g.grad_fn).__name__.startswith('_AdaTailAdjointFn')
        g.square().sum().backward()
    assert x.grad is None or float(x.grad.abs().max()) == 0.0           # linear in x: nothing of second order flows into it
    check(f'second order {shape} {kind}', w.grad, c['ref'][torch.float64]['g2'], c['ref'][torch.float32]['g2'])


def test_noise_alone_differentiates_as_the_identity(ada):
    """Without filter and cutout the linear part is the identity: the gradient is ``w`` and the R1-shaped ``w.grad`` is ``2 w``, bit for bit,
    on the operator and through the pipe (the named set ``noise``, and ``color`` + noise, whose base stage hands a differentiable input on)."""
    shape = (2, 4, 32, 24)
    c = case(shape, 'noise')
    a = dev(c['a'])
    assert a['Hz'] is None and a['cut'] is None and float(a['sigma'].max()) > 0
    draws = _pinned(2, 31, (3, 32, 24))(2)
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['noise']).to(DEV)
    for fn in (lambda t: ada.ada_tail_apply(t, color_channels=c['ch'], **a), lambda t: pipe(t, draws), lambda t: pipe(t)):
        with torch.enable_grad():
            x = c['x'].to(DEV).requires_grad_(True)
            w = c['w'].to(DEV).requires_grad_(True)
            y = fn(x)
            assert not torch.equal(y[:, 1:], x[:, 1:]) and torch.equal(y[:, 0], x[:, 0])
            (g,) = torch.autograd.grad((y * w).sum(), x, create_graph=True)
            assert torch.equal(g, w)
            g.square().sum().backward()
        assert torch.equal(w.grad, 2 * w.detach()) and (x.grad is None or float(x.grad.abs().max()) == 0.0)
    both = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['color'], noise=1).to(DEV)           # (the colour adjoint has no atomics)
    base = ada.AugmentPipe(**ada.AUGPIPE_SPECS['color']).to(DEV)
    with torch.enable_grad():
        x = c['x'].to(DEV).requires_grad_(True)
        w = c['w'].to(DEV)
        (g,) = torch.autograd.grad((both(x, draws) * w).sum(), x)
        xb = c['x'].to(DEV).requires_grad_(True)
        (gb,) = torch.autograd.grad((base(xb, draws[:2]) * w).sum(), xb)
    assert torch.equal(g, gb) and float(g.abs().max()) > 0


# ---- the whole pipe -------------------------------------------------------------------------------------------------------------------
def _pinned(n_max, seed, z_shape=None):
    rs = np.random.RandomState(seed)

    def t(a):
        return torch.from_numpy(a.astype(np.float32)).to(DEV)
    u, g = t(rs.uniform(size=(n_max, 24))), t(rs.standard_normal((n_max, 8)))
    ut, gt = t(rs.uniform(size=(n_max, 8))), t(rs.standard_normal((n_max, 5)))
    if z_shape is None:
        return lambda n: (u[:n], g[:n], ut[:n], gt[:n])
    z = t(rs.standard_normal((n_max,) + tuple(z_shape)))
    return lambda n: (u[:n], g[:n], ut[:n], gt[:n], z[:n])


def test_full_pipe_is_the_base_pipe_followed_by_the_tail(ada):
    shape = (4, 4, 32, 24)
    x = torch.from_numpy(np.random.RandomState(21).standard_normal(shape).astype(np.float32)).to(DEV)
    draws = _pinned(4, 22, (3, 32, 24))(4)
    full = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc']).to(DEV)
    base = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    Hz, sigma, cut = full.tail_params(draws)
    assert float(sigma.max()) > 0 and float(cut[:, 2].max()) > 0 and not torch.equal(Hz, torch.eye(43, device=DEV)[21].expand(4, 43))
    want = ada.ada_tail_apply(base(x, draws[:2]), Hz, sigma, draws[4], cut, (1, 3))
    assert torch.equal(full(x, draws), want) and not torch.equal(want, base(x, draws[:2]))
    # without a noise field one is drawn: the other stages are unchanged where sigma is 0, and two calls differ where it is not
    y1, y2 = full(x, draws[:4]), full(x, draws[:4])
    assert not torch.equal(y1, y2) and torch.equal(y1[sigma == 0], y2[sigma == 0])
    # tail multipliers 0: the base pipe bit for bit, on either form of the draws
    plain = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgc']).to(DEV)
    assert not plain.tail_on
    assert torch.equal(plain(x, draws), base(x, draws[:2])) and torch.equal(plain(x, draws[:2]), base(x, draws[:2]))
    assert len(full.draw(3)) == 4 and [tuple(t.shape) for t in full.draw(3)] == [(3, 24), (3, 8), (3, 8), (3, 5)]
    with pytest.raises(ValueError):
        full(x, draws[:2])                                               # the tail is on: its draws are required
    # each single category runs alone
    for name in ('filter', 'noise', 'cutout'):
        one = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL[name]).to(DEV)
        y = one(x, draws)
        kw = dict(filter=dict(Hz=Hz), noise=dict(sigma=sigma, z=draws[4]), cutout=dict(cut=cut))[name]
        assert torch.equal(y, ada.ada_tail_apply(x, color_channels=(1, 3), **kw)) and not torch.equal(y, x)


def test_sizes_the_filter_cannot_pad_are_rejected(ada):
    from shgan_amd import _lib
    Hz = torch.eye(43, device=DEV)[20:22].contiguous()
    for h, w in ((21, 32), (32, 21)):
        x = torch.zeros(2, 3, h, w, device=DEV)
        with pytest.raises(_lib.ShgError, match=f'{h} x {w}'):
            ada.ada_tail_apply(x, Hz=Hz)
        with pytest.raises(_lib.ShgError, match=f'{h} x {w}'):
            ada.ada_tail_apply_adjoint(x, Hz=Hz)
        pipe = ada.FullAugmentPipe(imgfilter=1).to(DEV)
        with pytest.raises(_lib.ShgError, match=f'{h} x {w}'):
            pipe(x)
        cut = torch.tensor([[0.5, 0.5, 0.2, 0.2]] * 2, device=DEV)       # the cutout alone has no such limit
        assert ada.ada_tail_apply(x + 1, cut=cut).shape == x.shape


# ---- the losses -----------------------------------------------------------------------------------------------------------------------
def test_stylegan2_loss_with_the_full_pipe(ada):
    from shgan_amd import losses
    from shgan_amd.model_zoo import stylegan as sg
    torch.manual_seed(3)
    mp = sg.Mapping(z_dim=32, c_dim=0, w_dim=32, num_ws=8, num_layers=3, lr_multiplier=0.01, w_avg_beta=0.995)
    syn = sg.Synthesis(w_dim=32, resolution=32, rgb_n=3, ch_base=256, ch_max=16, use_fp16_after_res=32)
    G = sg.Generator(mp, syn).to(DEV).train()
    D = sg.Discriminator(resolution=32, ic_n=3, ch_base=256, ch_max=16, use_fp16_before_res=None, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train()
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc']).to(DEV)
    L = losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=pipe, style_mixing_prob=0)
    assert L.draw_fn == pipe.draw
    L.draw_fn = _pinned(8, 5, (3, 32, 32))
    z, real, cnd = torch.randn(4, 32, device=DEV), torch.randn(4, 3, 32, 32, device=DEV), torch.zeros(4, 0, device=DEV)
    fake = torch.randn(4, 3, 32, 32, device=DEV)
    assert torch.equal(L.run_D(real, cnd), D(pipe(real, L.draw_fn(4)), cnd))
    gl, rl = L.run_D_pair(fake, cnd, real, cnd)
    both = D(pipe(torch.cat([fake, real]), L.draw_fn(8)), torch.cat([cnd, cnd]), segments=2)
    assert torch.equal(gl, both[:4]) and torch.equal(rl, both[4:])
    base = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)
    assert not torch.equal(L.run_D(real, cnd), D(base(real, L.draw_fn(4)[:2]), cnd))       # the tail took part
    for phase in losses.PHASES:
        G.zero_grad(set_to_none=True), D.zero_grad(set_to_none=True)
        mod = G if phase.startswith('G') else D
        G.requires_grad_(mod is G), D.requires_grad_(mod is D)
        L.stats.clear()
        L.accumulate_gradients(phase, real, cnd, z, cnd, sync=True, gain=1)
        grads = [p.grad for p in mod.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(t).all()) for t in grads) and any(float(t.abs().max()) > 0 for t in grads), phase
    L.draw_fn = pipe.draw                                                # the pipe's own draws, noise field included
    D.requires_grad_(True)
    L.accumulate_gradients('Dmain', real, cnd, z, cnd, sync=True, gain=1)
    assert 'Loss/signs/real' in L.stats


@pytest.mark.parametrize('spec', ['noise', 'cutout', 'filter'])
def test_stylegan2_loss_phases_with_a_single_tail_category(ada, spec):
    """Every phase, the ones that differentiate through the pipe (Gmain; R1 with ``create_graph``) included, with each tail category alone."""
    from shgan_amd import losses
    from shgan_amd.model_zoo import stylegan as sg
    torch.manual_seed(4)
    mp = sg.Mapping(z_dim=32, c_dim=0, w_dim=32, num_ws=8, num_layers=3, lr_multiplier=0.01, w_avg_beta=0.995)
    syn = sg.Synthesis(w_dim=32, resolution=32, rgb_n=3, ch_base=256, ch_max=16, use_fp16_after_res=32)
    G = sg.Generator(mp, syn).to(DEV).train()
    D = sg.Discriminator(resolution=32, ic_n=3, ch_base=256, ch_max=16, use_fp16_before_res=None, mbstd_group_size=4, mbstd_c_n=1).to(DEV).train()
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL[spec]).to(DEV)
    L = losses.StyleGAN2Loss(DEV, G.mapping, G.synthesis, D, augment_pipe=pipe, style_mixing_prob=0)
    z, real, cnd = torch.randn(4, 32, device=DEV), torch.randn(4, 3, 32, 32, device=DEV), torch.zeros(4, 0, device=DEV)
    assert not torch.equal(L.run_D(real, cnd), D(real, cnd))
    for phase in losses.PHASES:
        G.zero_grad(set_to_none=True), D.zero_grad(set_to_none=True)
        mod = G if phase.startswith('G') else D
        G.requires_grad_(mod is G), D.requires_grad_(mod is D)
        L.accumulate_gradients(phase, real, cnd, z, cnd, sync=True, gain=1)
        grads = [p.grad for p in mod.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(t).all()) for t in grads) and any(float(t.abs().max()) > 0 for t in grads), phase


def test_inpainting_loss_with_the_full_pipe(ada):
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
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc']).to(DEV)
    L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0, augment_pipe=pipe)
    L.draw_fn = _pinned(2, 8, (3, 256, 256))
    cnd = torch.zeros(2, 0, device=DEV)
    fake = torch.randn(2, 3, 256, 256, device=DEV)
    L._m05 = real4[:, 0:1]
    fake4 = torch.cat([real4[:, 0:1], fake], dim=1)
    assert torch.equal(L.run_D(fake, cnd), D(pipe(fake4, L.draw_fn(2)), cnd))              # the mask channel is prepended first
    assert torch.equal(L.run_D(real4, cnd), D(pipe(real4, L.draw_fn(2)), cnd))
    aug = pipe(real4, L.draw_fn(2))
    base = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc']).to(DEV)(real4, L.draw_fn(2)[:2])
    _, _, cut = pipe.tail_params(L.draw_fn(2))
    m = R.cutout_mask(cut.cpu(), 256, 256, torch.float32)[:, 0].to(DEV)
    assert torch.equal(aug[:, 0], base[:, 0] * m) and not torch.equal(aug[:, 1:], base[:, 1:])    # the mask channel: erased, never filtered


# ---- graph capture --------------------------------------------------------------------------------------------------------------------
def test_tail_forward_and_backward_replay_from_one_graph(ada):
    """One ``torch.cuda.graph`` of a tail-only pipe's forward + backward (one stream, no branches): replays draw again -- parameters and noise
    field -- and read ``p`` from the device: after ``p.zero_()`` a replay returns x, and the gradient w, bit for bit."""
    shape = (4, 3, 32, 32)
    rs = np.random.RandomState(9)
    x0, w0 = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)), torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['filter'], noise=1, cutout=1).to(DEV)
    assert pipe.tail_on and not pipe.geometry_on and not pipe.color_on
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
    assert not torch.equal(y1, y2) and not torch.equal(g1, g2)          # fresh draws, fresh noise field
    assert bool(torch.isfinite(y1).all() and torch.isfinite(g1).all())
    pipe.p.zero_()
    graph.replay()
    assert torch.equal(y, x.detach()) and torch.equal(gx, w)
