"""The float64 restatement of the dense / style family (tests/dense_f64.py) is itself right (CPU only).

Its closed-form backwards against ``torch.autograd.grad`` of the same forwards composed from tensor operators (``norm(inf)``, ``rsqrt``,
``matmul``), tie cases included; its ``dense`` against the reference's recorded outputs (tests/golden/small_ops.npz); its
``modconv_style_prep`` against the oracle's modulated convolution; and the two comparison functions of tests/test_gpu_dense_routes.py
against deliberately corrupted references."""
import math

import numpy as np
import pytest
import torch

import dense_f64 as ref
from conftest import load_golden, rel_err

TOL = 1e-12


def rnd(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape))


def close(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def composed_demod(w, prenorm):
    """stylegan.py:136-137,146,150-155, the weight side, from tensor operators."""
    if prenorm:
        w = w * (1 / math.sqrt(w[0].numel()) / w.norm(float('inf'), dim=list(range(1, w.ndim)), keepdim=True))
    wn = w * w.square().mean(list(range(1, w.ndim)), keepdim=True).rsqrt()
    return wn, wn.reshape(w.shape[0], w.shape[1], -1).square().sum(2)


def composed_style(s, wsq, prenorm):
    """stylegan.py:138,147,155, the style side, from tensor operators."""
    if prenorm:
        s = s / s.norm(float('inf'), dim=1, keepdim=True)
    s = s * s.square().mean().rsqrt()
    return s, (s.square().matmul(wsq.t()) + 1e-8).rsqrt()


@pytest.mark.parametrize('prenorm', [False, True])
@pytest.mark.parametrize('shape', [(3, 5, 3, 3), (4, 6, 1, 1), (2, 2, 3, 3), (1, 7, 9)])
@pytest.mark.parametrize('which', ['both', 'gwn', 'gwsq'])
def test_demod_weight_closed_backward_equals_autograd(shape, prenorm, which):
    with torch.enable_grad():
        w = rnd(1, *shape).requires_grad_(True)
        a, b = rnd(2, *shape), rnd(3, shape[0], shape[1])
        wn, wsq = composed_demod(w, prenorm)
        loss = (0 if which == 'gwsq' else (wn * a).sum()) + (0 if which == 'gwn' else (wsq * b).sum())
        (want,) = torch.autograd.grad(loss, [w])
    hn, hsq, sfac = ref.demod_weight(w, prenorm)
    assert close(hn, wn.detach()) < TOL and close(hsq, wsq.detach()) < TOL
    assert close(sfac[:, None] * w.detach().reshape(shape[0], -1), hn.reshape(shape[0], -1)) < TOL          # sfac = wn / w
    got = ref.demod_weight_backward(hn, sfac, None if which == 'gwsq' else a, None if which == 'gwn' else b)
    assert close(got, want) < TOL


def _style_inputs(n, i, o, ties):
    if ties:
        s, info = ref.tie_styles(n, i, seed=5)
        s = s.double()
    else:
        s, info = rnd(4, n, i) + 1.0, {}
    wsq = torch.from_numpy(np.random.RandomState(6).rand(o, i)) * 0.05
    return s, wsq, rnd(7, n, i), rnd(8, n, o), info


@pytest.mark.parametrize('which', ['both', 'gsn', 'gd'])
@pytest.mark.parametrize('n,i,o,prenorm,ties', [(3, 10, 7, False, False), (3, 10, 7, True, False), (1, 5, 2, True, False),
                                                (5, 9, 4, True, True), (4, 3, 1, True, True), (5, 9, 4, False, True)])
def test_style_factors_closed_backward_equals_autograd(n, i, o, prenorm, ties, which):
    s0, wsq0, a, b, _ = _style_inputs(n, i, o, ties)
    with torch.enable_grad():
        s, wsq = s0.clone().requires_grad_(True), wsq0.clone().requires_grad_(True)
        sn, d = composed_style(s, wsq, prenorm)
        loss = (0 if which == 'gd' else (sn * a).sum()) + (0 if which == 'gsn' else (d * b).sum())
        want_s, want_w = torch.autograd.grad(loss, [s, wsq], allow_unused=True)
    hsn, hd, aux = ref.style_factors(s0, wsq0, prenorm)
    assert close(hsn, sn.detach()) < TOL and close(hd, d.detach()) < TOL
    assert torch.equal(aux[:n], s0.abs().amax(1) if prenorm else torch.ones(n, dtype=torch.float64))
    gs, gw = ref.style_factors_backward(hsn, hd, wsq0, aux, None if which == 'gd' else a, None if which == 'gsn' else b, prenorm)
    assert close(gs, want_s) < TOL
    if which == 'gsn':
        assert want_w is None and not gw.any()
    else:
        assert close(gw, want_w) < TOL


def test_tied_maxima_share_the_derivative_and_a_near_tie_does_not():
    """Rows with a two-way and a three-way tie of mixed sign: every tied position receives the same share, of the sign of its element;
    the runner-up one float32 ulp below the maximum receives none (and autograd agrees: checked by the test above on the same rows)."""
    n, i, o = 5, 9, 4
    s0, wsq0, a, b, info = _style_inputs(n, i, o, True)
    s32 = ref.tie_styles(n, i, seed=5)[0]
    top, runner = s32[3, info[3][0][0]], s32[3, info[3][1]]
    assert float(runner) == -float(np.nextafter(np.float32(top), np.float32(0))) and abs(float(runner)) < float(top)
    sn, d, aux = ref.style_factors(s0, wsq0, True)
    gs, _ = ref.style_factors_backward(sn, d, wsq0, aux, a, b, True)
    g1, _ = ref.style_factors_backward(sn, d, wsq0, aux, a, b, False)
    corr, share = ref.tie_corrections(sn, aux, gs, g1)
    for row, (tied, runner_up) in info.items():
        assert abs(float(share[row])) > 1e-3                                   # a real correction, not a vanishing one
        for p in range(i):
            if p in tied:
                assert abs(float(corr[row, p]) - float(share[row])) <= 1e-13 * abs(float(share[row])), (row, p)
            else:
                assert abs(float(corr[row, p])) <= 1e-13 * abs(float(share[row])), (row, p, runner_up)
    # an untied row: the whole derivative of the maximum goes to the arg-max
    k = int(s0[0].abs().argmax())
    assert abs(float(corr[0, k]) - float(share[0])) <= 1e-13 * abs(float(share[0]))


def test_dense_reproduces_the_reference_records():
    """The three ``dense_*`` records of small_ops.npz (the reference's float32 ``addmm`` + lrelu_agc): elementwise within the worst-case
    float32 bound of a K-term sum, (K + 4) 2^-24 sum|x||w| (times the activation's gain)."""
    gd = load_golden('small_ops')
    for tag in ('mapping', 'affine', 'fc'):
        lr, use_act = (float(v) for v in gd[f'dense_{tag}__cfg'])
        x, w, b = (torch.from_numpy(gd[f'dense_{tag}__{k}']) for k in 'xwb')
        k = w.shape[1]
        wgain = lr / math.sqrt(k)
        y = ref.dense(x, w, b, wgain=wgain, bgain=lr, act=bool(use_act))
        gain = ref.SQRT2 if use_act else 1.0
        absprod = (x.double().abs() @ w.double().abs().t() * abs(wgain) + (b.double() * lr).abs()) * gain
        ratio, _ = ref.linear_excess(gd[f'dense_{tag}__y'], y, absprod, k + 4)
        assert ratio <= 1.0, (tag, ratio)
        assert rel_err(gd[f'dense_{tag}__y'], y.numpy()) < 1e-6, tag


def test_modconv_style_prep_agrees_with_the_oracle_modulation():
    """One small 3x3 layer evaluated at its centre pixel: oracle.modulated_conv2d(x, w, styles) = d[n,o] sum_ik x[n,i,k] wn[o,i,k] s[n,i]
    with (s, d) from the helper's ``modconv_style_prep`` and its [I][OP] table of squared normalised weights."""
    from oracle import shgan_oracle as orc
    n, i, o, op = 3, 5, 7, 64
    x, w, styles = rnd(9, n, i, 3, 3), rnd(10, o, i, 3, 3), rnd(11, n, i) + 1.0
    want = orc.modulated_conv2d(x, w, styles, padding=0, demodulate=True)
    assert want.shape == (n, o, 1, 1)
    wn, wsq, _ = ref.demod_weight(w)
    table = torch.zeros(i, op, dtype=torch.float64)
    table[:, :o] = wsq.t()
    s, d = ref.modconv_style_prep(styles, table, o)
    got = d * torch.einsum('nik,oik,ni->no', x.reshape(n, i, 9), wn.reshape(o, i, 9), s)
    assert close(got, want.reshape(n, o)) < TOL
    # without demodulation the styles are only scaled (toRGB: stylegan.py:325-337)
    want = orc.modulated_conv2d(x, w, styles * 0.25, padding=0, demodulate=False)
    s, d = ref.modconv_style_prep(styles, None, 0, demod=False, pre_gain=0.25)
    assert d is None and close(torch.einsum('nik,oik,ni->no', x.reshape(n, i, 9), w.reshape(o, i, 9), s), want.reshape(n, o)) < TOL


def test_products_normalize_and_colsum():
    a, b = rnd(12, 5, 7), rnd(13, 7, 3)
    assert torch.equal(ref.matmul_nn(a, b, 0.5), 0.5 * (a @ b))
    out, col = ref.matmul_tn(a, rnd(14, 5, 4), 2.0, -1.5)
    assert torch.equal(out, 2.0 * (a.t() @ rnd(14, 5, 4))) and torch.equal(col, -1.5 * a.sum(0))
    assert ref.matmul_tn(a, rnd(14, 5, 4))[1] is None
    x = rnd(15, 4, 9)
    x[2] = 0
    y = ref.normalize_2nd_moment(x)
    assert close(y[[0, 1, 3]].square().mean(1), torch.ones(3, dtype=torch.float64)) < 1e-7 and not y[2].any()


@pytest.mark.parametrize('kind', ['dropped', 'doubled'])
def test_linear_bound_catches_one_corrupted_term(kind):
    """The elementwise bound of the linear products: the float32 product itself passes it, a reference with ONE term of ONE element
    dropped (or counted twice) misses it by orders of magnitude -- while max-abs over max-abs of the whole matrix stays below 1e-5 for
    the large case, which is why the route table does not use that measure here."""
    for n, m, k, c in ((3, 5, 7, 5 // 16 + 1 + 18), (8, 1536, 64, 1536 // 16 + 18)):
        a, b = rnd(16, n, m).float(), rnd(17, m, k).float()
        want = ref.matmul_nn(a, b, 0.3)
        absprod = a.double().abs() @ b.double().abs() * 0.3
        got = (a @ b) * 0.3                                                      # a float32 evaluation
        assert ref.linear_excess(got, want, absprod, c)[0] <= 1.0
        # the smallest term of the element with the largest sum: the hardest single corruption to see
        e = int(want.abs().argmax())
        row, col = divmod(e, k)
        terms = a[row].double() * b[:, col].double() * 0.3
        t = terms[terms.abs().argmin() if m < 64 else terms.abs().argsort()[m // 2]]
        bad = want.clone()
        bad[row, col] += -t if kind == 'dropped' else t
        ratio, where = ref.linear_excess(got, bad, absprod, c)
        assert ratio > 10.0 and where == e, (n, m, k, ratio)
    assert rel_err(got.numpy(), bad.numpy()) < 1e-2                             # (the whole-matrix figure barely moves)


def test_row_measure_sees_a_bad_small_row_behind_a_large_one():
    want = rnd(18, 4, 50)
    want[0] *= 1e4
    got = want.clone()
    got[2, 7] += 1e-2                                                            # 1e-2 of a unit row: wrong
    assert rel_err(got.numpy(), want.numpy()) < 1e-6
    e, row = ref.row_rel_err(got, want)
    assert row == 2 and e > 1e-3
    assert ref.row_rel_err(want, want) == (0.0, 0)
    zero = torch.zeros(2, 3, dtype=torch.float64)
    assert ref.row_rel_err(zero, zero)[0] == 0.0 and ref.row_rel_err(zero + 1e-30, zero)[0] == math.inf
    assert ref.row_rel_err(zero + 1e-9, zero, scale=torch.ones(2))[0] == pytest.approx(1e-9)
