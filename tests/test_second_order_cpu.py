"""The references and the table of tests/second_order_f64.py are themselves right (CPU only).

* every float64 reference expression passes ``torch.autograd.gradcheck`` and ``gradgradcheck`` at a small shape of its family, on inputs the
  case's own constructor / seed selector produced (so the numerical differences never straddle a slope jump);
* the input constructor and the seed selector run for EVERY table entry and the kink margins are asserted: a mis-specified case fails here,
  before it reaches a GPU;
* every ``torch.autograd.Function`` of the operator modules is either a required node of some case or named in ``NOT_HERE`` with the test
  that pins its second derivative."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import second_order_f64 as so
from conftest import ROOT
from oracle import shgan_oracle as orc


def _leaves(P):
    return {k: so.leaf64(v) for k, v in P.items()}


def _check(fn, P, fast=False):
    """gradcheck and gradgradcheck of fn(**P) in float64 with respect to every input (``fast``: torch's random-projection mode, for the
    layers, whose full Jacobians take tens of seconds)."""
    names = list(P)
    leaves = [so.leaf64(P[k]) for k in names]

    def f(*a):
        return fn(**dict(zip(names, a)))
    with torch.enable_grad():
        assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=fast)
        assert torch.autograd.gradgradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=fast)


F4 = so.FIR4
SMALL = {
    # family / expression -> (make, ref, pre | None, clear): a small instance of the family built by the table's own constructors
    'conv2d_s1': (so._conv_make(1, 2, 2, 3, 4, 3), lambda x, w, b: F.conv2d(x, w, b, stride=1, padding=1), None, None),
    'conv2d_s2': (so._conv_make(1, 2, 2, 6, 5, 3), lambda x, w, b: F.conv2d(x, w, b, stride=2, padding=0), None, None),
    'conv_transpose2d': (lambda seed: {k: (v.transpose(0, 1).contiguous() if k == 'w' else v) for k, v in so._conv_make(1, 2, 2, 3, 4, 3)(seed).items()},
                         lambda x, w, b: F.conv_transpose2d(x, w, b, stride=2, padding=1), None, None),
    'conv2d_bias_act': (so._conv_make(1, 2, 2, 3, 4, 3), lambda x, w, b: so.ref_conv_act(x, w, b, stride=1, padding=1),
                        lambda x, w, b: so.ref_conv_act(x, w, b, stride=1, padding=1, pre=True), so.clear_of_kinks),
    'conv2d_bias_act_linear_residual': (so._conv_make(1, 2, 2, 3, 4, 3, res_shape=(1, 2, 3, 4)),
                                        lambda x, w, b, r: so.ref_conv_act(x, w, b, r, stride=1, padding=1, act=False, gain=0.7), None, None),
    'conv2d_resample_up2': (so._rs_make(1, 1, 2, 3, 4), lambda x, w: orc.conv2d_resample(x, w, f=F4, up=2, padding=1, flip_weight=False), None, None),
    'conv2d_resample_down2': (so._rs_make(1, 1, 2, 4, 6), lambda x, w: orc.conv2d_resample(x, w, f=F4, down=2, padding=1), None, None),
    'conv2d_down_bias_act': (so._rs_make(1, 1, 2, 4, 6, bias=True), lambda x, w, b: so.ref_down_act(x, w, b, F4),
                             lambda x, w, b: so.ref_down_act(x, w, b, F4, pre=True), so.clear_of_kinks),
    'bias_act': (lambda seed: so.tail_inputs(seed, (3, 5), d=False, noise=None, bias=True, names=('x', None, None, 'bias')),
                 lambda x, bias: so.ref_tail(x, bias=bias), None, None),
    'modconv_tail': (lambda seed: so.tail_inputs(seed, (2, 3, 2, 4), d=True, noise='n1hw', bias=True),
                     lambda t, d, noise, bias: so.ref_tail(t, d, noise, bias), None, None),
    'modconv_tail_shared_noise_linear': (lambda seed: so.tail_inputs(seed, (2, 3, 2, 4), d=True, noise='hw', bias=False),
                                         lambda t, d, noise: so.ref_tail(t, d, noise, act=False, gain=0.7), None, None),
}


@pytest.mark.parametrize('name', sorted(SMALL))
def test_reference_expression_gradcheck_and_gradgradcheck(name):
    make, ref, pre, clear = SMALL[name]
    seed = 5 if pre is None else so.select_seed(make, pre, clear, 5)
    _check(ref, make(seed))


@pytest.mark.parametrize('name', [u[0] for u in so.UPFIRDN])
def test_upfirdn2d_reference_gradcheck_and_gradgradcheck(name):
    (_, f, up, down, pad, flip, gain), = [u for u in so.UPFIRDN if u[0] == name]
    x = torch.from_numpy(np.random.RandomState(3).standard_normal((1, 1, 4, 5)).astype(np.float32))
    _check(lambda x: orc.upfirdn2d(x, f, up=up, down=down, padding=pad, flip_filter=flip, gain=gain), dict(x=x))


@pytest.mark.parametrize('kind,ci,co,k,h,w,kw', [('synthesis', 3, 4, 3, 4, 4, {}), ('synthesis', 2, 3, 3, 2, 2, dict(up=2)), ('torgb', 4, 3, 1, 3, 4, {}),
                                                 ('conv2d', 3, 4, 3, 4, 6, dict(down=2))])
def test_layer_reference_gradcheck_and_gradgradcheck(kind, ci, co, k, h, w, kw):
    case = so.layer_case('small', kind, ci, co, k, h, w, need=(), **kw)
    _check(case.ref, case.inputs(), fast=True)


def test_third_order_functional_on_the_reference_is_consistent():
    """The third-order functional: its g3 with respect to gy equals the directional derivative of g2 (a finite difference in float64)."""
    (case,) = [k for k in so.CASES if k.order == 3]
    P = case.inputs()
    gy, U, _ = so.aux_data(case.seed(), P, tuple(P['t'].shape))
    _, V, _ = so.aux_data(case.seed() + 1, dict(P, gy=gy), tuple(P['t'].shape))
    U, V = {k: v.double() for k, v in U.items()}, {k: v.double() for k, v in V.items()}

    def l3(gy_):
        _, g2, _ = so.third_order(case.ref, _leaves(P), so.leaf64(gy_), U, V)
        return sum(float((g2[k] * V[k]).sum()) for k in g2)
    _, _, g3 = so.third_order(case.ref, _leaves(P), so.leaf64(gy), U, V)
    dirn = torch.from_numpy(np.random.RandomState(1).standard_normal(tuple(gy.shape)))
    h = 1e-5
    fd = (l3(gy.double() + h * dirn) - l3(gy.double() - h * dirn)) / (2 * h)
    an = float((g3['gy'] * dirn).sum())
    assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0), (fd, an)
    assert all(g3[k] is not None and float(g3[k].abs().max()) > 0 for k in ('t', 'd', 'gy'))


# ------------------------------------------------------------------------------------------------
# every table entry: constructor / seed selector and kink margins
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', [k.id for k in so.CASES])
def test_table_entry_is_well_specified(cid):
    case = so.BY_ID[cid]
    seed = case.seed()                         # (raises for a case none of whose 16 seeds qualifies)
    P = case.inputs()
    assert all(torch.isfinite(v).all() for v in P.values())
    assert set(case.wrt1 or P) <= set(P) and set(case.only or ()) <= set(P) and set(case.skip1) <= set(P)
    if case.half:
        assert all((v.dtype == torch.float16) == (k in so.HALF_KEYS) for k, v in P.items())
    else:
        assert all(v.dtype == torch.float32 for v in P.values())
    P64 = {k: v.double() for k, v in P.items()}
    if case.constructed:
        # pointwise cases: the argument of the activation, from the ROUNDED operands, at least KINK_MARGIN from 0 and from the clamp
        z = so.ref_tail(P64[next(k for k in P if k in so.HALF_KEYS)], P64.get('d'), P64.get('noise'), P64.get('bias'), pre=True)
        a = so.act_argument(z).abs()
        assert float(a.min()) >= so.KINK_MARGIN and float((a - so.CLAMP).abs().min()) >= so.KINK_MARGIN, (float(a.min()), float((a - so.CLAMP).abs().min()))
        clamped = float((a > so.CLAMP).double().mean())
        assert 0.15 <= clamped <= 0.45, clamped
    if case.pre is not None:
        assert case.base_seed <= seed < case.base_seed + so.SEEDS
        z = case.pre(**P64)
        assert case.clear(z)
        if not case.layer:
            # the fused convolution cases: the margin in units of z, and roughly a quarter of the elements clamped
            assert so.kink_distance(z) > so.TOL_CONV * float(z.abs().max())
            assert z.numel() <= 9000
            clamped = float((so.act_argument(z).abs() > so.CLAMP).double().mean())
            assert 0.1 <= clamped <= 0.45, clamped


def test_bars_are_the_projects_first_order_bars():
    """TOL_CONV and TOL_PW are those of tests/test_gpu_routes_fp32.py (read as text: that module needs the device library)."""
    with open(os.path.join(ROOT, 'tests', 'test_gpu_routes_fp32.py')) as fh:
        src = fh.read()
    for name in ('TOL_CONV', 'TOL_PW'):
        (val,) = re.findall(rf'^{name} = (\S+)', src, flags=re.M)
        assert float(val) == getattr(so, name), (name, val)


def test_kink_distance_and_selector():
    hi, lo = so.CLAMP / so.SQRT2, -so.CLAMP / (so.ALPHA * so.SQRT2)
    z = torch.tensor([0.5, hi + 0.01, lo - 0.3, -0.02], dtype=torch.float64)
    assert math.isclose(so.kink_distance(z), 0.01, rel_tol=1e-9)
    assert math.isclose(so.kink_distance(z[2:]), 0.02, rel_tol=1e-9)
    # lrelu_agc really changes slope exactly there
    for j in (0.0, hi, lo):
        a, b = (orc.lrelu_agc(torch.tensor([j + s, j + 2 * s], dtype=torch.float64), clamp=so.CLAMP) for s in (-1e-3, 1e-3))
        assert abs(float((a[1] - a[0]) - (b[1] - b[0]))) > 1e-4
    # a selector none of whose seeds qualifies fails, it does not skip
    with pytest.raises(AssertionError, match='mis-specified'):
        so.select_seed(lambda s: dict(x=torch.zeros(3)), lambda x: x, so.clear_of_kinks, 0)


def test_functional_sees_a_wrong_second_derivative():
    """The functional and rel_err turn red for two defects of the kind the table is there to catch, stated on the reference itself: a gain
    dropped from the weight gradient (seen in g1_w and in every g2), and a cotangent that never reaches the backward node."""
    from conftest import rel_err
    case = so.BY_ID['conv2d_bias_act-linear']
    P = case.inputs()
    with torch.no_grad():
        shape = tuple(case.ref(**{k: v.double() for k, v in P.items()}).shape)
    gy, U, q = so.aux_data(case.seed(), P, shape)
    U, q = {k: v.double() for k, v in U.items()}, q.double()
    _, g1, g2 = so.functional(case.ref, _leaves(P), so.leaf64(gy), U, q)

    class NoGainOnGw(torch.autograd.Function):
        @staticmethod
        def forward(ctx, w):
            return w * 0.7

        @staticmethod
        def backward(ctx, g):
            return g                  # (should be 0.7 g)

    def broken(x, w, b):
        return F.conv2d(x, NoGainOnGw.apply(w), b * 0.7, padding=1)
    _, h1, h2 = so.functional(broken, _leaves(P), so.leaf64(gy), U, q)
    assert rel_err(h1['x'].detach(), g1['x'].detach()) < 1e-12 and rel_err(h1['w'].detach(), g1['w'].detach()) > 0.1
    assert min(rel_err(h2[k], g2[k]) for k in ('x', 'w', 'gy')) > 1e-2
    _, _, k2 = so.functional(case.ref, _leaves(P), so.leaf64(gy), U, q, only=['x'])
    assert rel_err(k2['gy'], g2['gy']) > 1e-3                 # a cotangent that never reached the backward node


# ------------------------------------------------------------------------------------------------
# coverage: every autograd Function of the operator modules
# ------------------------------------------------------------------------------------------------

def test_every_autograd_function_is_pinned_to_second_order():
    pkg = os.path.join(ROOT, 'sh-gan_amd', 'model_zoo')
    files = sorted(glob.glob(os.path.join(pkg, 'stylegan_utils', '*.py'))) + [os.path.join(pkg, 'stylegan.py')]
    assert len(files) > 5
    found = {}
    for path in files:
        with open(path) as fh:
            for name in re.findall(r'^class\s+(\w+)\(torch\.autograd\.Function\)', fh.read(), flags=re.M):
                found[name] = os.path.relpath(path, ROOT)
    assert len(found) >= 20, found
    required = set().union(*(k.need | k.fwd for k in so.CASES))
    missing = [f'{n} ({p})' for n, p in sorted(found.items()) if n + 'Backward' not in required and n not in so.NOT_HERE]
    assert not missing, f'autograd Functions with no second-order case and no NOT_HERE entry: {missing}'
    both = [n for n in found if n + 'Backward' in required and n in so.NOT_HERE]
    stale = [n for n in so.NOT_HERE if n not in found]
    assert not both and not stale, (both, stale)
    # the tests NOT_HERE points to exist
    for n, where in so.NOT_HERE.items():
        m = re.match(r'(tests/\w+\.py)(?:::(\w+))?', where)
        if m:
            path = os.path.join(ROOT, m.group(1))
            assert os.path.exists(path), where
            if m.group(2):
                with open(path) as fh:
                    assert f'def {m.group(2)}(' in fh.read(), where
    # and every node a case names is a Function that exists
    unknown = sorted(n for n in required | set().union(*(k.forbid for k in so.CASES)) if n[:-len('Backward')] not in found)
    assert not unknown, unknown
