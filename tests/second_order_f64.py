"""Second derivatives of every differentiable HIP operator: the float64 references, the functional and the case table.

The yardstick of tests/test_gpu_second_order.py (itself checked on the CPU by tests/test_second_order_cpu.py).  Every case is one operator
``op`` with differentiable inputs ``P`` and fixed random data -- a cotangent ``gy`` (a leaf that requires grad: d/dgy of the backward node is
exercised, as inside a network), one probe ``u_p`` per input and a weight ``q`` shaped like y:

    y   = op(*P)
    g1  = autograd.grad((y * gy).sum(), P, create_graph=True)
    pen = sum_p (g1_p * u_p).square().sum() + (y.square() * q).sum()
    g2  = autograd.grad(pen, P + [gy], allow_unused=True)

(``functional``) -- the shape of the path-length and R1 regularisers.  The reference side evaluates it in float64 on the CPU with the plain
expression (``F.conv2d``, ``F.conv_transpose2d``, the oracle's ``upfirdn2d`` / ``conv2d_resample`` / ``lrelu_agc`` / layer functions, tensor
arithmetic), the device side through the public entry point.  Every array is generated in the test's dtype (float32, or half for the
activation of the half cases), so both sides start from the same numbers: the reference is evaluated on the rounded operands.

Activation kinks.  lrelu_agc has slope jumps at z = 0 and at the clamp; an element whose float32 pre-activation lands on the other side of a
jump than the float64 one changes every sum over it by O(1).  This is kept out by construction, never by tolerance: every case with an
activation uses ``clamp = 1.5`` (about a quarter of the elements clamped; at 256 none is), the pointwise cases construct their inputs from a
target pre-activation at least 0.2 from both jumps (``tail_inputs``), and the fused convolution cases take the first of 16 consecutive seeds
whose float64 pre-activation keeps every element farther than TOL_CONV * max|z| from both jumps (``select_seed``) -- the margin the kernel is
allowed to be off by.  A case for which none of the 16 qualifies is mis-specified and FAILS (on the CPU, before it reaches a GPU).

The table is also a route table of the ``create_graph`` compositions: each case names the autograd nodes that must appear under g1 on the device
(what the backward built under ``create_graph``) and under y (the forward route), and those that must appear under neither."""
import contextlib
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import shgan_oracle as orc

SQRT2 = math.sqrt(2.0)
TOL_CONV = 2e-5          # convolutions, resampling convolutions, weight gradients: y and g1 (tests/test_gpu_routes_fp32.py)
TOL_PW = 1e-5            # FIR and pointwise passes: y and g1 (tests/test_gpu_routes_fp32.py)
G2_FACTOR = 2.0          # g2: two kernels of the family in sequence, each allowed its bar, errors add at most linearly
G3_FACTOR = 3.0          # the third-order case: three in sequence, by the same argument
TOL_H_ELEM, TOL_H_SUM, TOL_H_G2 = 2e-3, 5e-3, 4e-3      # half tail: tests/test_gpu_fp16.py (elementwise, reduced gradients, second order)
LAYER_FACTOR, LAYER_FLOOR = 3.0, 5e-5                   # layers: max(3 e_ref, 5e-5) (test_gpu_backward.py, test_gpu_shu_geometry.py)
CLAMP = 1.5
ALPHA = 0.2
KINK_MARGIN = 0.2        # constructed inputs: distance of A's argument (after the gains) from 0 and from the clamp
SEEDS = 16
HALF_KEYS = ('t', 'x')   # the inputs that are half tensors in a half case (activations; d, noise, bias stay float32 as in the layers)


# ------------------------------------------------------------------------------------------------
# the functional
# ------------------------------------------------------------------------------------------------

def _wide(t):
    return t.float() if t.dtype == torch.float16 else t


def functional(op, P, gy, U, q, wrt1=None, only=None, ctx=None, skip1=()):
    """-> (y, g1 {name: tensor | None}, g2 {name | 'gy': tensor | None}).  ``wrt1``: the inputs of the first derivative (default: all);
    ``only``: the g1 that enter the penalty (default: all of wrt1); ``ctx``: a context manager factory around the first ``grad``
    (no_weight_gradients); ``skip1``: inputs left out of the first derivative (how the reference states what no_weight_gradients does)."""
    names = list(P)
    wrt1 = [k for k in (wrt1 or names) if k not in skip1]
    with torch.enable_grad():
        y = op(**P)
        with (ctx() if ctx is not None else contextlib.nullcontext()):
            g1 = torch.autograd.grad((_wide(y) * _wide(gy)).sum(), [P[k] for k in wrt1], create_graph=True, allow_unused=True)
        g1 = dict(zip(wrt1, g1))
        pen = (_wide(y).square() * _wide(q)).sum()
        for k in (only or wrt1):
            if g1.get(k) is not None:
                pen = pen + (_wide(g1[k]) * _wide(U[k])).square().sum()
        g2 = torch.autograd.grad(pen, [P[k] for k in names] + [gy], allow_unused=True)
    return y, g1, dict(zip(names + ['gy'], g2))


def third_order(op, P, gy, U, V):
    """grad(grad(grad)) of the term trilinear in (gy, t, d): g1 = d<y, gy>/d(t, d); g2 = d sum (g1 u)^2 / d(t, d, gy), itself differentiable;
    g3 = d sum <g2, v> / d(t, d, gy)."""
    names = list(P)
    with torch.enable_grad():
        y = op(**P)
        g1 = torch.autograd.grad((y * gy).sum(), [P[k] for k in names], create_graph=True)
        pen = sum((g * U[k]).square().sum() for k, g in zip(names, g1))
        g2 = torch.autograd.grad(pen, [P[k] for k in names] + [gy], create_graph=True)
        l3 = sum((g * V[k]).sum() for k, g in zip(names + ['gy'], g2))
        g3 = torch.autograd.grad(l3, [P[k] for k in names] + [gy], allow_unused=True)
    return y, dict(zip(names + ['gy'], g2)), dict(zip(names + ['gy'], g3))


def graph_nodes(*tensors):
    """The type names of every autograd node reachable from the tensors through ``next_functions``."""
    seen, names, stack = set(), set(), [t.grad_fn for t in tensors if t is not None and t.grad_fn is not None]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        stack.extend(g for g, _ in f.next_functions)
    return names


# ------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------

def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dtype)


def leaf64(t):
    return t.detach().to('cpu', torch.float64).clone().requires_grad_(True)


def aux_data(seed, P, y_shape, half=False):
    """(gy, {name: probe}, q) for a case: gy ~ N(0,1), probes ~ N(0,1) scaled by sqrt(numel(p) / numel(y)) where an input is smaller than
    the output (its gradient is a sum over numel(y) / numel(p) terms), q ~ U(0.5, 1.5); in the dtype of the tensors they multiply."""
    rs = np.random.RandomState(seed + 7919)
    ydt = torch.float16 if half else torch.float32
    ny = int(np.prod(y_shape))
    gy = _t(rs.standard_normal(y_shape), ydt)
    q = _t(rs.rand(*y_shape) + 0.5, ydt)
    U = {}
    for k, p in P.items():
        s = 1.0 / math.sqrt(max(1.0, ny / max(p.numel(), 1)))
        U[k] = _t(rs.standard_normal(tuple(p.shape)) * s, p.dtype)
    return gy, U, q


def act_argument(z, gain=1.0, alpha=ALPHA, act_gain=SQRT2):
    """The value lrelu_agc clamps: leaky_relu(z) * act_gain * gain."""
    return torch.where(z < 0, z * alpha, z) * (act_gain * gain)


def kink_distance(z, gain=1.0, alpha=ALPHA, act_gain=SQRT2, clamp=CLAMP):
    """min over the elements of the distance of z from the three slope jumps of lrelu_agc, in units of z: 0, +clamp / act_gain (the gain
    cancels: the argument and the clamp both carry it) and -clamp / (alpha act_gain)."""
    z = z.detach().double()
    hi, lo = clamp / act_gain, -clamp / (alpha * act_gain)
    return float(torch.minimum(z.abs(), torch.minimum((z - hi).abs(), (z - lo).abs())).min())


def target_preactivation(rs, shape, alpha=ALPHA):
    """z* with |A-argument| / sqrt2 drawn from [0.3, 0.9] (70 %) or [1.3, 2.5] (30 %: clamped at 1.5), either sign, the negative side scaled
    by 1 / alpha: sqrt2 z* (positive side) and sqrt2 alpha z* (negative side) are at least 0.2 from 0 and from +-1.5."""
    mag = np.where(rs.rand(*shape) < 0.7, 0.3 + 0.6 * rs.rand(*shape), 1.3 + 1.2 * rs.rand(*shape))
    neg = rs.rand(*shape) < 0.5
    return np.where(neg, -mag / alpha, mag)


def tail_inputs(seed, shape, half=False, d=True, noise=None, bias=True, names=('t', 'd', 'noise', 'bias')):
    """Constructed inputs of y = A(t d[n,c] + noise + bias[c]): d ~ U(0.5, 1.5), noise and bias ~ N(0, 1/4), t solved in float64 from the
    target pre-activation and rounded to the test dtype.  ``noise``: None | 'hw' ([H,W]) | 'n1hw' ([N,1,H,W]); ``shape`` may be [N,C]
    (the dense form of bias_act).  -> {name: tensor} of the operands present, under ``names``."""
    rs = np.random.RandomState(seed)
    n, c = shape[0], shape[1]
    sp = tuple(shape[2:])
    one = (1,) * len(sp)
    z = target_preactivation(rs, tuple(shape))
    dv = (rs.rand(n, c) + 0.5).astype(np.float32)
    nv = (0.5 * rs.standard_normal(sp if noise == 'hw' else (n, 1) + sp)).astype(np.float32)
    bv = (0.5 * rs.standard_normal(c)).astype(np.float32)
    num = z
    if noise:
        num = num - nv.astype(np.float64)
    if bias:
        num = num - bv.astype(np.float64).reshape((1, c) + one)
    if d:
        num = num / dv.astype(np.float64).reshape((n, c) + one)
    out = {names[0]: _t(num, torch.float16 if half else torch.float32)}
    if d:
        out[names[1]] = _t(dv)
    if noise:
        out[names[2]] = _t(nv)
    if bias:
        out[names[3]] = _t(bv)
    return out


def ref_tail(t, d=None, noise=None, bias=None, act=True, gain=1.0, clamp=CLAMP, pre=False):
    n, c = t.shape[0], t.shape[1]
    one = (1,) * (t.ndim - 2)
    z = t if d is None else t * d.reshape((n, c) + one)
    if noise is not None:
        z = z + noise
    if bias is not None:
        z = z + bias.reshape((1, c) + one)
    if pre:
        return z
    return orc.lrelu_agc(z, gain=gain, alpha=ALPHA, act_gain=SQRT2, clamp=clamp) if act else z * gain


def ref_conv_act(x, w, b=None, r=None, stride=1, padding=0, act=True, gain=1.0, clamp=CLAMP, pre=False):
    z = F.conv2d(x, w, b, stride=stride, padding=padding)
    if pre:
        return z
    y = orc.lrelu_agc(z, gain=gain, alpha=ALPHA, act_gain=SQRT2, clamp=clamp) if act else z * gain
    return y if r is None else y + r


def ref_down_act(x, w, b, f, act=True, gain=1.0, clamp=CLAMP, pre=False):
    z = orc.conv2d_resample(x, w, f=f, down=2, padding=1) + b.reshape(1, -1, 1, 1)
    if pre:
        return z
    return orc.lrelu_agc(z, gain=gain, alpha=ALPHA, act_gain=SQRT2, clamp=clamp) if act else z * gain


def clear_of_kinks(z):
    """Every element of the float64 pre-activation farther than TOL_CONV max|z| from the three jumps (clamp = CLAMP, gain 1)."""
    return kink_distance(z) > TOL_CONV * float(z.abs().max())


def clear_of_zero(y):
    """The layers (their own activation: clamp 256, never reached here, so the one jump is z = 0), judged from the float64 OUTPUT: y = 0 iff
    z = 0 and y is z times a constant on either side, so |y| > TOL_CONV max|y| keeps z as far from the jump as the convolution that forms it
    is allowed to be off by."""
    y = y.detach().abs()
    return float(y.min()) > TOL_CONV * float(y.max()) and float(y.max()) < 200.0


def qualifying_seeds(make, pre, clear, base):
    with torch.no_grad():
        return [s for s in range(base, base + SEEDS) if clear(pre(**{k: v.double() for k, v in make(s).items()}))]


def select_seed(make, pre, clear, base):
    """The first of SEEDS consecutive seeds from ``base`` whose float64 pre-activation ``pre(**make(seed))`` is ``clear``.  None: AssertionError
    (the case is mis-specified; it never skips)."""
    with torch.no_grad():
        for s in range(base, base + SEEDS):
            if clear(pre(**{k: v.double() for k, v in make(s).items()})):
                return s
    raise AssertionError(f'mis-specified case: none of the seeds {base} .. {base + SEEDS - 1} keeps the pre-activation clear of the kinks')


# ------------------------------------------------------------------------------------------------
# the product side, imported on first use (tests/test_second_order_cpu.py never calls it)
# ------------------------------------------------------------------------------------------------

_PRODUCT = None


def product():
    global _PRODUCT
    if _PRODUCT is None:
        import shgan_amd  # noqa: F401
        from shgan_amd.model_zoo import stylegan
        from shgan_amd.model_zoo.stylegan_utils import conv2d_gradfix, conv2d_resample, grad_ops, upfirdn2d
        _PRODUCT = types.SimpleNamespace(stylegan=stylegan, gf=conv2d_gradfix, cr=conv2d_resample, go=grad_ops, up=upfirdn2d)
    return _PRODUCT


@contextlib.contextmanager
def switched(switches):
    """Module-level A/B switches {'gf.LINEAR_GAIN_ON_WEIGHTS': False, ...} flipped for the block and restored whatever happens."""
    m, old = product(), []
    try:
        for key, val in (switches or {}).items():
            mod, attr = key.split('.')
            old.append((getattr(m, mod), attr, getattr(getattr(m, mod), attr)))
            setattr(getattr(m, mod), attr, val)
        yield
    finally:
        for mod, attr, val in reversed(old):
            setattr(mod, attr, val)


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------

class Case:
    """One row.  ``make(seed) -> {name: tensor}`` (the differentiable inputs, in the test's dtypes); ``ref(**P)`` the plain expression;
    ``dev(m, **P)`` the public entry point (m = ``product()``); ``pre`` the pre-activation of ``ref`` for the seed selection (None: no kinks,
    or constructed inputs); node names on the device: ``need`` in the graph of g1 (what the create_graph backward built), ``fwd`` in the graph
    of y (the forward route), ``forbid`` in neither."""
    def __init__(self, family, name, make, ref, dev, need=(), forbid=(), fwd=(), tol=TOL_CONV, seed=0, pre=None, clear=clear_of_kinks, wrt1=None, only=None,
                 nowg=False, skip1=(), switches=None, half=False, constructed=False, order=2, refkey=None, layer=None):
        self.family, self.name, self.make, self.ref, self.dev = family, name, make, ref, dev
        self.need, self.forbid, self.fwd, self.tol, self.base_seed, self.pre, self.clear = set(need), set(forbid), set(fwd), tol, seed, pre, clear
        self.wrt1, self.only, self.nowg, self.skip1, self.switches = wrt1, only, nowg, tuple(skip1), dict(switches or {})
        self.half, self.constructed, self.order, self.layer = half, constructed, order, layer
        self.refkey = refkey or name          # cases that share a reference (the same functional of the same data) share this key
        self._seed = None

    @property
    def id(self):
        return f'{self.family}-{self.name}'

    def seed(self):
        if self._seed is None:
            self._seed = self.base_seed if self.pre is None else select_seed(self.make, self.pre, self.clear, self.base_seed)
        return self._seed

    def inputs(self):
        return self.make(self.seed())

    def bars(self, tensor, order):
        """The bar of one tensor: 'y', an input's name (order 1, 2 or 3) or 'gy'."""
        if self.half:
            if order >= 2:
                return TOL_H_G2
            return TOL_H_ELEM if tensor in ('y',) + HALF_KEYS else TOL_H_SUM
        return self.tol * {0: 1.0, 1: 1.0, 2: G2_FACTOR, 3: G3_FACTOR}[order]


CASES = []
FIR4 = orc.setup_filter((1, 3, 3, 1))


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- 1. conv2d_gradfix.conv2d, with bias ----------------------------------------------------------------------------------------------

def _conv_make(n, ci, co, h, w, k, res_shape=None):
    def make(seed):
        rs = np.random.RandomState(seed)
        P = dict(x=_t(rs.standard_normal((n, ci, h, w))), w=_t(rs.standard_normal((co, ci, k, k)) / math.sqrt(ci * k * k)),
                 b=_t(rs.standard_normal(co)))
        if res_shape is not None:
            P['r'] = _t(rs.standard_normal(res_shape))
        return P
    return make


CONV_GEOM = [
    # n, ci, co, h, w, k, stride, pad
    (2, 5, 7, 8, 12, 3, 1, 1), (2, 24, 40, 9, 12, 3, 1, 1), (2, 6, 10, 10, 13, 3, 1, 0), (3, 8, 12, 8, 12, 1, 1, 0),
    # stride 2, parity x padding: _fit crops (17x21 p0 exact, p1 crops), passes through and zero-extends (16x20 p0: 7x9 out, the transposed
    # result is one short)
    (2, 6, 10, 17, 21, 3, 2, 0), (2, 6, 10, 16, 20, 3, 2, 0), (2, 6, 10, 16, 20, 3, 2, 1), (2, 6, 10, 17, 21, 3, 2, 1),
    # the FIR-padded model form
    (2, 64, 64, 33, 33, 3, 2, 0),
]
for (n, ci, co, h, w, k, s, p) in CONV_GEOM:
    nm = f'{n}x{ci}to{co}_{h}x{w}_k{k}s{s}p{p}'
    kw = dict(stride=s, padding=p)
    ref = (lambda kw: lambda x, w, b: F.conv2d(x, w, b, **kw))(kw)
    dev = (lambda kw: lambda m, x, w, b: m.gf.conv2d(x, w, b, **kw))(kw)
    t2 = {'_ConvTranspose2dFnBackward'} if s == 2 else {'_Conv2dFnBackward'}      # the input gradient's operator
    _add('conv2d', nm, _conv_make(n, ci, co, h, w, k), ref, dev, need={'_WgradFnBackward'} | t2, fwd={'_Conv2dFnBackward'}, seed=11)
    _add('conv2d', nm + '_nowg', _conv_make(n, ci, co, h, w, k), ref, dev, need=t2, fwd={'_Conv2dFnBackward'}, forbid={'_WgradFnBackward'},
         seed=11, nowg=True, skip1=('w',))

# ---- 2. conv2d_gradfix.conv_transpose2d -------------------------------------------------------------------------------------------------

for (n, ci, co, h, w, p) in [(2, 5, 7, 6, 9, 0), (2, 24, 40, 8, 5, 1)]:
    def _mk(seed, n=n, ci=ci, co=co, h=h, w=w):
        rs = np.random.RandomState(seed)
        return dict(x=_t(rs.standard_normal((n, ci, h, w))), w=_t(rs.standard_normal((ci, co, 3, 3)) / math.sqrt(ci * 9 / 4)),
                    b=_t(rs.standard_normal(co)))
    _add('conv_transpose2d', f'{n}x{ci}to{co}_{h}x{w}_p{p}', _mk, (lambda p: lambda x, w, b: F.conv_transpose2d(x, w, b, stride=2, padding=p))(p),
         (lambda p: lambda m, x, w, b: m.gf.conv_transpose2d(x, w, b, stride=2, padding=p))(p),
         need={'_Conv2dFnBackward', '_WgradFnBackward'}, fwd={'_ConvTranspose2dFnBackward'}, seed=21)

# ---- 3. conv2d_gradfix.conv2d_bias_act --------------------------------------------------------------------------------------------------

CBA_ACT = [
    # name, (n, ci, co, h, w, k), stride, pad
    ('s1p1', (2, 5, 12, 8, 12, 3), 1, 1), ('s1p1_block', (2, 24, 40, 9, 12, 3), 1, 1), ('s2p0', (2, 8, 12, 17, 21, 3), 2, 0),
    ('k1_thin', (2, 4, 16, 8, 12, 1), 1, 0), ('k1', (2, 9, 16, 8, 12, 1), 1, 0),
]
for nm, g, s, p in CBA_ACT:
    kw = dict(stride=s, padding=p, act=True, gain=1.0, clamp=CLAMP)
    _add('conv2d_bias_act', 'act_' + nm, _conv_make(*g), (lambda kw: lambda x, w, b: ref_conv_act(x, w, b, **kw))(kw),
         (lambda kw: lambda m, x, w, b: m.gf.conv2d_bias_act(x, w, b, kw['padding'], stride=kw['stride'], act=True, gain=1.0, alpha=ALPHA,
                                                             act_gain=SQRT2, clamp=CLAMP))(kw),
         need={'_BiasActBwdFnBackward', '_WgradFnBackward', '_ConvTranspose2dFnBackward' if s == 2 else '_Conv2dFnBackward'},
         fwd={'_ConvBiasActFnBackward'},
         seed=100, pre=(lambda kw: lambda x, w, b: ref_conv_act(x, w, b, pre=True, **kw))(kw))
for res in (False, True):
    for on_w in (True, False):
        g = (2, 5, 12, 8, 12, 3)
        kw = dict(stride=1, padding=1, act=False, gain=0.7)
        nm = 'linear' + ('_residual' if res else '') + ('' if on_w else '_gain_elementwise')
        if res:
            ref = (lambda kw: lambda x, w, b, r: ref_conv_act(x, w, b, r, **kw))(kw)
            dev = lambda m, x, w, b, r: m.gf.conv2d_bias_act(x, w, b, 1, stride=1, act=False, gain=0.7, residual=r)      # noqa: E731
        else:
            ref = (lambda kw: lambda x, w, b: ref_conv_act(x, w, b, **kw))(kw)
            dev = lambda m, x, w, b: m.gf.conv2d_bias_act(x, w, b, 1, stride=1, act=False, gain=0.7)      # noqa: E731
        _add('conv2d_bias_act', nm, _conv_make(*g, res_shape=(2, 12, 8, 12) if res else None), ref, dev,
             need={'_Conv2dFnBackward', '_WgradFnBackward'} | (set() if on_w else {'_BiasActBwdFnBackward'}), fwd={'_ConvBiasActFnBackward'},
             forbid={'_BiasActBwdFnBackward'} if on_w else set(), seed=31, switches={'gf.LINEAR_GAIN_ON_WEIGHTS': on_w},
             refkey='linear' + ('_residual' if res else ''))

# ---- 4. conv2d_resample and conv2d_down_bias_act, the 4x4 [1,3,3,1] filter ----------------------------------------------------------------


def _rs_make(n, ci, co, h, w, bias=False):
    def make(seed):
        rs = np.random.RandomState(seed)
        P = dict(x=_t(rs.standard_normal((n, ci, h, w))), w=_t(rs.standard_normal((co, ci, 3, 3)) / math.sqrt(ci * 9)))
        if bias:
            P['b'] = _t(rs.standard_normal(co))
        return P
    return make


_AK = dict(act=True, gain=1.0, alpha=ALPHA, act_gain=SQRT2, clamp=CLAMP)
for way, nowg, sw in (('wg', False, {}), ('nowg', True, {}), ('unfused', False, {'cr.FUSED_TRAIN_RESAMPLE': False})):
    skip = ('w',) if nowg else ()
    wg = set() if nowg else {'_WgradFnBackward'}
    nwg = {'_WgradFnBackward'} if nowg else set()
    fused = not sw
    # up = 2: _UpConvFirFn; backward = FIR transpose, strided convolution, weight gradient with the tensors exchanged
    _add('conv2d_resample', 'up2_' + way, _rs_make(2, 6, 10, 6, 8), lambda x, w: orc.conv2d_resample(x, w, f=FIR4, up=2, padding=1, flip_weight=False),
         lambda m, x, w: m.cr.conv2d_resample(x=x, w=w, f=FIR4.to(x.device), up=2, padding=1, flip_weight=False),
         need={'_UpfirdnFnBackward', '_Conv2dFnBackward'} | wg, fwd={'_UpConvFirFnBackward'} if fused else {'_ConvTranspose2dFnBackward', '_UpfirdnFnBackward'},
         forbid=nwg | (set() if fused else {'_UpConvFirFnBackward'}), seed=41, nowg=nowg, skip1=skip, switches=sw, refkey='up2_' + ('nowg' if nowg else 'wg'))
    # down = 2: _FirDownConvFn; with weight gradients on, create_graph re-filters x (the branch no shipped loss reaches)
    _add('conv2d_resample', 'down2_' + way, _rs_make(2, 6, 10, 12, 16), lambda x, w: orc.conv2d_resample(x, w, f=FIR4, down=2, padding=1),
         lambda m, x, w: m.cr.conv2d_resample(x=x, w=w, f=FIR4.to(x.device), down=2, padding=1),
         need={'_UpfirdnFnBackward', '_ConvTranspose2dFnBackward'} | wg, fwd={'_FirDownConvFnBackward'} if fused else {'_Conv2dFnBackward', '_UpfirdnFnBackward'},
         forbid=nwg | (set() if fused else {'_FirDownConvFnBackward'}), seed=42, nowg=nowg, skip1=skip, switches=sw, refkey='down2_' + ('nowg' if nowg else 'wg'))
    _add('conv2d_resample', 'down2_act_' + way, _rs_make(2, 6, 10, 12, 16, bias=True), lambda x, w, b: ref_down_act(x, w, b, FIR4),
         lambda m, x, w, b: m.cr.conv2d_down_bias_act(x, w, FIR4.to(x.device), b, dict(_AK)),
         need={'_UpfirdnFnBackward', '_ConvTranspose2dFnBackward', '_BiasActBwdFnBackward'} | wg,
         fwd={'_FirDownConvFnBackward'} if fused else {'_ConvBiasActFnBackward', '_UpfirdnFnBackward'},
         forbid=nwg | (set() if fused else {'_FirDownConvFnBackward'}), seed=120, nowg=nowg, skip1=skip, switches=sw,
         pre=lambda x, w, b: ref_down_act(x, w, b, FIR4, pre=True), refkey='down2_act_' + ('nowg' if nowg else 'wg'))
# odd input: the generic composition (the fused node takes even extents only)
_add('conv2d_resample', 'down2_odd_13x16', _rs_make(2, 6, 10, 13, 16), lambda x, w: orc.conv2d_resample(x, w, f=FIR4, down=2, padding=1),
     lambda m, x, w: m.cr.conv2d_resample(x=x, w=w, f=FIR4.to(x.device), down=2, padding=1),
     need={'_UpfirdnFnBackward', '_ConvTranspose2dFnBackward', '_WgradFnBackward'}, fwd={'_Conv2dFnBackward', '_UpfirdnFnBackward'},
     forbid={'_FirDownConvFnBackward'}, seed=43)

# ---- 5. upfirdn2d, float32 (linear: g2 pins d pen / d gy) ---------------------------------------------------------------------------------

FIR_ASYM2 = orc.setup_filter((1, 3, 2, 0.5))                       # 2-D 4x4, not symmetric: flip_filter changes the result
FIR_ASYM1 = orc.setup_filter((1, 3, 2, 0.5), separable=True)       # separable 4-tap
FIR_ODD = orc.setup_filter((1, 2, 1), separable=True)              # rank-1, odd
UPFIRDN = [
    # name, f, up, down, padding [x0, x1, y0, y1], flip, gain
    ('up2_2d', FIR4, 2, 1, [2, 1, 2, 1], False, 4.0), ('up2_2d_asym_flip', FIR_ASYM2, 2, 1, [2, 1, 2, 1], True, 4.0),
    ('up2_sep_asym', FIR_ASYM1, 2, 1, [2, 1, 2, 1], False, 4.0),
    ('down2_2d_asym', FIR_ASYM2, 1, 2, [1, 1, 1, 1], False, 1.0), ('down2_sep_asym_flip', FIR_ASYM1, 1, 2, [1, 1, 1, 1], True, 1.0),
    ('same_2d_asym_flip', FIR_ASYM2, 1, 1, [2, 1, 2, 1], True, 1.0), ('same_sep', FIR_ASYM1, 1, 1, [2, 1, 2, 1], False, 1.0),
    ('same_pad2_2d', FIR4, 1, 1, [2, 2, 2, 2], False, 1.0),
    ('odd_sep_unequal_pad', FIR_ODD, 1, 1, [2, 0, 1, 3], False, 1.0), ('odd_sep_unequal_pad_up2_flip', FIR_ODD, 2, 1, [2, 0, 1, 3], True, 1.0),
]
for nm, f, up, down, pad, flip, gain in UPFIRDN:
    kw = dict(up=up, down=down, padding=pad, flip_filter=flip, gain=gain)
    _add('upfirdn2d', nm, lambda seed: dict(x=_t(np.random.RandomState(seed).standard_normal((2, 3, 9, 14)))),
         (lambda f, kw: lambda x: orc.upfirdn2d(x, f, **kw))(f, kw), (lambda f, kw: lambda m, x: m.up.upfirdn2d(x, f.to(x.device), **kw))(f, kw),
         need={'_UpfirdnFnBackward'}, fwd={'_UpfirdnFnBackward'}, tol=TOL_PW, seed=51)

# ---- 6. grad_ops.bias_act (constructed inputs) -------------------------------------------------------------------------------------------

for nm, shape, half in (('rank4', (2, 37, 5, 7), False), ('rank2_dense', (5, 37), False), ('half_nhwc_c16', (2, 16, 6, 10), True)):
    for act in (True, False):
        gain = 1.0 if act else 0.7
        _add('bias_act', f'{nm}_{"act" if act else "linear"}',
             (lambda shape, half: lambda seed: tail_inputs(seed, shape, half=half, d=False, noise=None, bias=True, names=('x', None, None, 'bias')))(shape, half),
             (lambda act, gain: lambda x, bias: ref_tail(x, bias=bias, act=act, gain=gain))(act, gain),
             (lambda act, gain: lambda m, x, bias: m.go.bias_act(x, bias, act=act, gain=gain, alpha=ALPHA, act_gain=SQRT2, clamp=CLAMP))(act, gain),
             need={'_BiasActBwdFnBackward'}, fwd={'_BiasActFnBackward'}, tol=TOL_PW, seed=61, half=half, constructed=act)

# ---- 7. grad_ops.modconv_tail (constructed inputs) -----------------------------------------------------------------------------------------
# A shape with H W % 4 != 0 (float32) is not served: ``modtail_supported`` is False there and callers fall back to the per-operation form
# (stylegan._modulated_conv2d_train); the fallback is tested through the 5x5 synthesis layer below.
TAIL_UNSUPPORTED_SHAPE = (2, 8, 5, 5)


def _tail_case(nm, shape, half, d, noise, bias, act, closed, only=None, seed=71):
    gain = 1.0 if act else 0.7

    def ref(t, d=None, noise=None, bias=None):
        return ref_tail(t, d, noise, bias, act=act, gain=gain)

    def dev(m, t, d=None, noise=None, bias=None):
        return m.go.modconv_tail(t, d=d, noise=noise, bias=bias, act=act, gain=gain, alpha=ALPHA, act_gain=SQRT2, clamp=CLAMP)
    _add('modconv_tail', nm + ('' if closed else '_composed'), lambda seed: tail_inputs(seed, shape, half=half, d=d, noise=noise, bias=bias), ref, dev,
         need={'_ModTailBwdFnBackward'} if closed else {'_BiasActBwdFnBackward'}, fwd={'_ModTailFnBackward'},
         forbid=set() if closed else {'_ModTailBwdFnBackward'}, tol=TOL_PW, seed=seed, half=half, only=only, constructed=act,
         switches={'go.CLOSED_TAIL_BACKWARD': closed}, refkey=nm)


for closed in (True, False):
    # the presence grid, float32 (3, 37, 6x10)
    for d in (True, False):
        for noise in (None, 'hw', 'n1hw'):
            for bias in (True, False):
                for act in (True, False):
                    _tail_case(f'f32_37_d{int(d)}_n{noise or "0"}_b{int(bias)}_{"act" if act else "lin"}', (3, 37, 6, 10), False, d, noise, bias, act, closed)
    # which cotangents carry a value into the backward node (all four operands present).  These rows pin VALUES, not branches: no Function
    # here switches ``set_materialize_grads`` off, so autograd hands _ModTailBwdFn.backward a zero tensor, never None, for every output the
    # penalty does not use -- with ``d`` given the one-pass u / e form and the ``extra`` pass through the bias and noise sums run in every
    # row, and the ``ggt``-only / ``ggd``-only branches of that function are reached only without ``d`` (ggd is then dropped).
    for only in (('t',), ('d',), ('t', 'd'), ('bias',), ('noise',)):
        _tail_case('f32_37_only_' + '_'.join(only), (3, 37, 6, 10), False, True, 'n1hw', True, True, closed, only=only)
    _tail_case('f32_64_4x4_all', (2, 64, 4, 4), False, True, 'hw', True, True, closed, seed=72)
    # half, channels-last (3, 32, 6x10)
    for d, noise, bias, act in ((True, 'hw', True, True), (True, 'n1hw', True, False), (False, None, True, True), (True, None, False, True)):
        _tail_case(f'f16_32_d{int(d)}_n{noise or "0"}_b{int(bias)}_{"act" if act else "lin"}', (3, 32, 6, 10), True, d, noise, bias, act, closed, seed=73)
    for only in (('t',), ('d',), ('t', 'd'), ('bias',), ('noise',)):
        _tail_case('f16_32_only_' + '_'.join(only), (3, 32, 6, 10), True, True, 'n1hw', True, True, closed, only=only, seed=73)

# the third-order case: grad(grad(grad)) of the term trilinear in (gy, t, d); runs the is_grad_enabled() branch of _ModTailBwdFn.backward
_add('modconv_tail', 'f32_8_4x4_third_order', lambda seed: tail_inputs(seed, (2, 8, 4, 4), d=True, noise=None, bias=False),
     lambda t, d: ref_tail(t, d, act=True), lambda m, t, d: m.go.modconv_tail(t, d=d, act=True, gain=1.0, alpha=ALPHA, act_gain=SQRT2, clamp=CLAMP),
     need={'_ModTailBwdFnBackward', '_BiasActBwdFnBackward'}, fwd={'_ModTailFnBackward'}, tol=TOL_PW, seed=74, constructed=True, order=3)

# ---- 8. layers, against the oracle on a flat state dict ----------------------------------------------------------------------------------
# (the layers' own activation: clamp 256, so the only jump is z = 0; the seed is chosen from the float64 output alone, ``clear_of_zero``)

W_DIM = 16
LRELU = 'lrelu_agc(alpha=0.2, gain=sqrt_2)'


def _layer_sd(kind, seed, ci, co, k):
    rs = np.random.RandomState(seed)
    sd = dict(weight=_t(rs.standard_normal((co, ci, k, k))), bias=_t(0.5 * rs.standard_normal(co)))
    if kind in ('synthesis', 'torgb'):
        sd['affine.weight'] = _t(rs.standard_normal((ci, W_DIM)))
        sd['affine.bias'] = _t(1.0 + 0.2 * rs.standard_normal(ci))
    if kind == 'synthesis':
        sd['noise_strength'] = _t(np.asarray(0.3))
    return sd


BUFFERS = ('noise_const', 'resample_filter')


def _noise_const(res):
    return _t(np.random.RandomState(4242).standard_normal((res, res)))


def layer_case(nm, kind, ci, co, k, h, w, need, fwd=(), forbid=(), up=1, down=1, wrt1=('wlat',), nowg=False, seed=200):
    res = h * up if kind == 'synthesis' else None

    def make(seed):
        rs = np.random.RandomState(seed + 1)
        P = dict(x=_t(rs.standard_normal((2, ci, h, w))))
        if kind != 'conv2d':
            P['wlat'] = _t(rs.standard_normal((2, W_DIM)))
        P.update(_layer_sd(kind, seed, ci, co, k))
        return P

    def ref(**P):
        sd = {k_: v for k_, v in P.items() if k_ not in ('x', 'wlat')}
        sd['resample_filter'] = FIR4
        if kind == 'synthesis':
            sd['noise_const'] = _noise_const(res).to(P['x'].dtype)
            return orc.synthesis_layer(sd, '', P['x'], P['wlat'], res, up=up, noise_mode='const')
        if kind == 'torgb':
            return orc.torgb_layer(sd, '', P['x'], P['wlat'])
        return orc.conv2d_layer(sd, '', P['x'], k, down=down, use_filter=True, act=True)

    def dev(m, **P):
        sg = m.stylegan
        if kind == 'synthesis':
            mod = sg.synthesis_layer(ci, co, k, W_DIM, res, up=up)
            mod.noise_const.copy_(_noise_const(res))
        elif kind == 'torgb':
            mod = sg.torgb_layer(ci, co, k, W_DIM)
        else:
            mod = sg.conv2d_layer(ci, co, k, bias=True, activation=LRELU, down=down)
        mod = mod.to(P['x'].device)
        args = (P['x'],) if kind == 'conv2d' else (P['x'], P['wlat'])
        kwargs = dict(noise_mode='const') if kind == 'synthesis' else {}
        return torch.func.functional_call(mod, {k_: v for k_, v in P.items() if k_ not in ('x', 'wlat')}, args, kwargs)

    return Case('layer', nm, make, ref, dev, need=need, fwd=fwd, forbid=forbid, seed=seed, wrt1=list(wrt1), nowg=nowg, layer=kind,
                pre=None if kind == 'torgb' else ref, clear=clear_of_zero)


CASES.append(layer_case('synthesis_8x8_pathlength', 'synthesis', 8, 12, 3, 8, 8, need={'_ModTailBwdFnBackward', '_Conv2dFnBackward'},
                        fwd={'_ModTailFnBackward', '_Conv2dFnBackward'}))
# ... with the weight in the first derivative: the create_graph branch of stylegan._DemodWeightFn.backward (no shipped loss takes it)
CASES.append(layer_case('synthesis_8x8_weight_and_latent', 'synthesis', 8, 12, 3, 8, 8, wrt1=('wlat', 'weight'),
                        need={'_ModTailBwdFnBackward', '_Conv2dFnBackward', '_WgradFnBackward', '_DemodWeightFnBackward'},
                        fwd={'_ModTailFnBackward', '_Conv2dFnBackward', '_DemodWeightFnBackward'}))
CASES.append(layer_case('synthesis_up2_8x8_pathlength', 'synthesis', 8, 12, 3, 8, 8, up=2, need={'_ModTailBwdFnBackward', '_UpfirdnFnBackward', '_Conv2dFnBackward'},
                        fwd={'_ModTailFnBackward', '_UpConvFirFnBackward'}))
CASES.append(layer_case('synthesis_5x5_fallback_pathlength', 'synthesis', 8, 12, 3, 5, 5, need={'_BiasActBwdFnBackward', '_Conv2dFnBackward'},
                        fwd={'_BiasActFnBackward', '_Conv2dFnBackward'}, forbid={'_ModTailFnBackward', '_ModTailBwdFnBackward'}))
CASES.append(layer_case('torgb_6x10_pathlength', 'torgb', 12, 3, 1, 6, 10, need={'_Conv2dFnBackward', '_ModTailBwdFnBackward'},
                        fwd={'_ChannelBiasFnBackward', '_Conv2dFnBackward'}))
CASES.append(layer_case('conv2d_down2_8x12_r1', 'conv2d', 8, 12, 3, 8, 12, down=2, wrt1=('x',), nowg=True,
                        need={'_BiasActBwdFnBackward', '_ConvTranspose2dFnBackward', '_UpfirdnFnBackward'}, fwd={'_FirDownConvFnBackward'},
                        forbid={'_WgradFnBackward'}))
CASES.append(layer_case('conv2d_down2_8x12_all', 'conv2d', 8, 12, 3, 8, 12, down=2, wrt1=('x', 'weight', 'bias'),
                        need={'_BiasActBwdFnBackward', '_ConvTranspose2dFnBackward', '_UpfirdnFnBackward', '_WgradFnBackward'},
                        fwd={'_FirDownConvFnBackward'}))


BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), 'duplicate case ids'

# Functions whose second derivative is pinned elsewhere (or that have none by design): class name -> where
NOT_HERE = {
    '_NT': 'tests/test_gpu_train_graph.py::test_dense_ops_first_and_second_order_vs_torch_float64',
    '_NN': 'tests/test_gpu_train_graph.py::test_dense_ops_first_and_second_order_vs_torch_float64',
    '_TN': 'tests/test_gpu_train_graph.py::test_dense_ops_first_and_second_order_vs_torch_float64',
    '_StyleFactorsFn': 'tests/test_gpu_dense_routes.py (style factors, first and closed second order against float64)',
    '_StyleFactorsBwdFn': 'tests/test_gpu_train_graph.py::test_closed_double_backward_of_the_style_factors_vs_float64_autograd',
    '_FusedMultiplyAdd': 'tests/test_gpu_r6_ops.py::test_fma_float64_gradcheck_first_and_second_order',
    '_MulUnbroadcast': 'tests/test_gpu_r6_ops.py::test_fma_float64_gradcheck_first_and_second_order',
    '_Unbroadcast': 'tests/test_gpu_r6_ops.py::test_fma_float64_gradcheck_first_and_second_order',
    '_StashGradFn': 'first order only by design: under create_graph the gradient takes autograd\'s ordinary path (grad_ops.InputGradJoin)',
    '_RelayoutFn': 'a linear cast: its backward is the same Function again (tests/test_gpu_fp16.py)',
    '_ScaleCastFn': 'a linear cast: its backward is the same Function again (tests/test_gpu_fp16.py)',
}
