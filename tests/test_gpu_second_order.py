"""Second derivatives of every differentiable HIP operator against float64 autograd of the plain expression (run with -m gpu on an MI355X).

The table, the references and the functional are in tests/second_order_f64.py (checked on the CPU by tests/test_second_order_cpu.py): per
case y, every g1 and every g2 (the inputs and the cotangent gy) are compared with ``conftest.rel_err``; an unused gradient must be None or
all-zero on both sides.  Bars: the family's first-order bar for y and g1 (2e-5 convolutions, 1e-5 FIR / pointwise), twice that for g2 (two
kernels of the family in sequence), the project's half bars for the half tail, and for the layers max(3 e_ref, 5e-5) with e_ref the
distance of the float32 CPU oracle from the float64 one, per tensor.  Each case also asserts the autograd nodes that must and must not
appear in the graph of g1 (and of y, for the forward route): the table is the route table of the ``create_graph`` compositions.  Every figure is printed as
``SECOND <case> <tensor>: rel_err (bar)``."""
import numpy as np
import pytest
import torch

import second_order_f64 as so
from conftest import rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_REF = {}


def c(a):
    return None if a is None else a.detach().float().cpu().numpy() if a.dtype == torch.float16 else a.detach().cpu().numpy()


def to_dev(t):
    t = t.to(DEV)
    if t.dtype == torch.float16 and t.ndim == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.detach().requires_grad_(True)


def run_cpu(case, P, gy, U, q, dtype):
    """The plain expression on the CPU in ``dtype`` -> numpy arrays (y, g1, g2)."""
    leaf = lambda t: t.detach().to('cpu', dtype).clone().requires_grad_(True)      # noqa: E731
    y, g1, g2 = so.functional(case.ref, {k: leaf(v) for k, v in P.items()}, leaf(gy), {k: v.to(dtype) for k, v in U.items()}, q.to(dtype),
                              wrt1=case.wrt1, only=case.only, skip1=case.skip1)
    return c(y), {k: c(v) for k, v in g1.items()}, {k: c(v) for k, v in g2.items()}


def data(case):
    P = case.inputs()
    with torch.no_grad():
        shape = tuple(case.ref(**{k: v.double() for k, v in P.items()}).shape)
    return (P,) + so.aux_data(case.seed(), P, shape, case.half)


def reference(case):
    """The float64 side of a case, computed once per reference key and never modified (cases that differ only in an A/B switch share it)."""
    key = (case.family, case.refkey)
    if key not in _REF:
        P, gy, U, q = data(case)
        _REF[key] = run_cpu(case, P, gy, U, q, torch.float64)
        for a in [_REF[key][0]] + [v for d in _REF[key][1:] for v in d.values() if v is not None]:
            a.setflags(write=False)
    return _REF[key]


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def judge(self, tensor, got, want, bar):
        if want is None or not np.any(want):
            ok = got is None or not np.any(got)
            print(f'SECOND {self.case.id} {tensor}: unused on the reference side, {"unused" if ok else "NOT unused"} on the device')
            if not ok:
                self.bad.append(f'{tensor}: the reference has no gradient here, the device returned one')
            return
        if got is None:
            self.bad.append(f'{tensor}: missing on the device')
            return
        assert got.shape == want.shape, (tensor, got.shape, want.shape)
        e = rel_err(got, want)
        print(f'SECOND {self.case.id} {tensor}: {e:.3e} ({bar:.1e})')
        if not e <= bar:
            self.bad.append(f'{tensor}: {e:.3e} > {bar:.1e}')

    def nodes(self, fwd, bwd):
        """``fwd``: the nodes under y; ``bwd``: the nodes under the create_graph gradients (which reach the forward node only where the backward
        reads the saved output)."""
        custom = lambda ns: ' '.join(sorted(n for n in ns if n.endswith('Backward')))      # noqa: E731
        print(f'SECOND {self.case.id} nodes: y: {custom(fwd)} | g: {custom(bwd)}')
        if self.case.need - bwd:
            self.bad.append(f'nodes missing under the gradients: {sorted(self.case.need - bwd)}')
        if self.case.fwd - fwd:
            self.bad.append(f'nodes missing under y: {sorted(self.case.fwd - fwd)}')
        if self.case.forbid & (fwd | bwd):
            self.bad.append(f'forbidden nodes present: {sorted(self.case.forbid & (fwd | bwd))}')

    def done(self):
        assert not self.bad, f'{self.case.id} (seed {self.case.seed()}): ' + '; '.join(self.bad)


def run_device(case, P, gy, U, q):
    m = so.product()
    Pd = {k: to_dev(v) for k, v in P.items()}
    with so.switched(case.switches):
        y, g1, g2 = so.functional(lambda **kw: case.dev(m, **kw), Pd, to_dev(gy), {k: v.to(DEV) for k, v in U.items()}, q.to(DEV),
                                  wrt1=case.wrt1, only=case.only, ctx=m.gf.no_weight_gradients if case.nowg else None)
    nodes = (so.graph_nodes(y), so.graph_nodes(*g1.values()))
    return c(y), {k: c(v) for k, v in g1.items()}, {k: c(v) for k, v in g2.items()}, nodes


OPERATOR_CASES = [k.id for k in so.CASES if not k.layer and k.order == 2]
LAYER_CASES = [k.id for k in so.CASES if k.layer]


@pytest.mark.parametrize('cid', OPERATOR_CASES)
def test_operator_second_order_vs_float64(cid):
    case = so.BY_ID[cid]
    yr, g1r, g2r = reference(case)
    P, gy, U, q = data(case)
    y, g1, g2, nodes = run_device(case, P, gy, U, q)
    rep = Report(case)
    rep.nodes(*nodes)
    rep.judge('y', y, yr, case.bars('y', 0))
    for k in P:
        if k in g1 or k in g1r:
            rep.judge('g1_' + k, g1.get(k), g1r.get(k), case.bars(k, 1))
    for k in list(P) + ['gy']:
        rep.judge('g2_' + k, g2[k], g2r[k], case.bars(k, 2))
    rep.done()


@pytest.mark.parametrize('cid', LAYER_CASES)
def test_layer_second_order_vs_float64_oracle(cid):
    """A layer chains several kernels, so its bar is measured: max(3 e_ref, 5e-5) per tensor, e_ref = the float32 CPU oracle against the
    float64 one."""
    case = so.BY_ID[cid]
    yr, g1r, g2r = reference(case)
    P, gy, U, q = data(case)
    y32, g132, g232 = run_cpu(case, P, gy, U, q, torch.float32)
    y, g1, g2, nodes = run_device(case, P, gy, U, q)
    rep = Report(case)
    rep.nodes(*nodes)

    def bar(a32, a64):
        e_ref = rel_err(a32, a64) if a64 is not None and np.any(a64) else 0.0
        return max(so.LAYER_FACTOR * e_ref, so.LAYER_FLOOR)
    rep.judge('y', y, yr, bar(y32, yr))
    for k in g1r:
        rep.judge('g1_' + k, g1.get(k), g1r[k], bar(g132[k], g1r[k]))
    for k in list(P) + ['gy']:
        rep.judge('g2_' + k, g2[k], g2r[k], bar(g232[k], g2r[k]))
    rep.done()


def test_modconv_tail_third_order_vs_float64():
    """grad(grad(grad)) of the term trilinear in (gy, t, d): the ``is_grad_enabled()`` branch of _ModTailBwdFn.backward (tensor operators on the
    slope kernel).  Bars: y and g2 as in the table, g3 three times the pointwise bar (three passes in sequence)."""
    (case,) = [k for k in so.CASES if k.order == 3]
    P = case.inputs()
    gy, U, q = so.aux_data(case.seed(), P, tuple(P['t'].shape))
    _, V, _ = so.aux_data(case.seed() + 1, dict(P, gy=gy), tuple(P['t'].shape))
    leaf = lambda t: so.leaf64(t)      # noqa: E731
    yr, g2r, g3r = so.third_order(case.ref, {k: leaf(v) for k, v in P.items()}, leaf(gy), {k: v.double() for k, v in U.items()},
                                  {k: v.double() for k, v in V.items()})
    m = so.product()
    y, g2, g3 = so.third_order(lambda **kw: case.dev(m, **kw), {k: to_dev(v) for k, v in P.items()}, to_dev(gy), {k: v.to(DEV) for k, v in U.items()},
                               {k: v.to(DEV) for k, v in V.items()})
    rep = Report(case)
    rep.nodes(so.graph_nodes(y), so.graph_nodes(*g2.values()))
    rep.judge('y', c(y), c(yr), case.bars('y', 0))
    for k in g2r:
        rep.judge('g2_' + k, c(g2[k]), c(g2r[k]), case.bars(k, 2))
    for k in g3r:
        rep.judge('g3_' + k, c(g3[k]), c(g3r[k]), case.bars(k, 3))
    rep.done()


def test_modtail_unsupported_shape_is_declined():
    """H W % 4 != 0 in float32: ``modtail_supported`` is False and callers fall back to the per-operation form (the 5x5 synthesis layer of the
    table runs that fallback and forbids the tail nodes)."""
    m = so.product()
    assert not m.go.modtail_supported(torch.zeros(so.TAIL_UNSUPPORTED_SHAPE, device=DEV))
    assert m.go.modtail_supported(torch.zeros(2, 8, 4, 4, device=DEV))
