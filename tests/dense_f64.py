"""Float64 restatement of the dense / style family (csrc/dense.hip), plain torch on the CPU: one function per entry point.

The yardstick of tests/test_gpu_dense_routes.py.  The forwards state the formulas of stylegan.py:87-98 (dense), :343-344
(normalize_2nd_moment) and :136-155 (the weight and the style side of modulated_conv2d); the backwards are the closed forms written in
the kernels' comments.  tests/test_dense_f64_cpu.py holds every closed form against ``torch.autograd.grad`` of the same forward composed
from tensor operators, ``dense`` against the reference's recorded outputs and ``modconv_style_prep`` against the oracle's modulation.
Every function takes tensors (or arrays) of any float type and computes in float64."""
import math

import torch

SQRT2 = math.sqrt(2.0)
U32 = 2.0 ** -24                   # unit round-off of float32


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().to('cpu', torch.float64)


# ------------------------------------------------------------------------------------------------
# forwards and closed-form backwards
# ------------------------------------------------------------------------------------------------

def lrelu_agc(z, gain=1.0, alpha=0.2, act_gain=SQRT2, clamp=256.0):
    """common/utils.py:135-143: leaky-relu -> * (act_gain * gain) -> clamp(+-clamp * gain)."""
    z = torch.where(z < 0, z * alpha, z) * (act_gain * gain)
    return z.clamp(-clamp * gain, clamp * gain) if clamp is not None else z


def dense(x, w, b=None, wgain=1.0, bgain=1.0, act=False, gain=1.0, alpha=0.2, act_gain=SQRT2, clamp=256.0):
    """y = act(x @ (w * wgain)^T + b * bgain); without activation the layer multiplies by ``gain``."""
    z = f64(x) @ f64(w).t() * wgain
    if b is not None:
        z = z + f64(b) * bgain
    return lrelu_agc(z, gain, alpha, act_gain, clamp) if act else z * gain


def matmul_nn(a, b, scale=1.0):
    """scale * a[N,M] @ b[M,K]."""
    return scale * (f64(a) @ f64(b))


def matmul_tn(a, b, scale=1.0, colsum_scale=None):
    """(scale * a[N,M]^T @ b[N,K], colsum_scale * sum_n a[n,:] | None)."""
    a, b = f64(a), f64(b)
    return scale * (a.t() @ b), (None if colsum_scale is None else colsum_scale * a.sum(0))


def normalize_2nd_moment(x, eps=1e-8):
    x = f64(x)
    return x * (x.square().mean(1, keepdim=True) + eps).rsqrt()


def demod_weight(w, prenorm=False):
    """w [O,I,...] -> (wn, wsq [O,I], sfac [O]): w1 = w / (sqrt(I K) max|w[o]|) with ``prenorm`` else w; wn = w1 rsqrt(mean w1^2);
    wsq = sum_k wn^2; sfac = wn / w."""
    w = f64(w)
    o, i = w.shape[0], w.shape[1]
    w3 = w.reshape(o, i, -1)
    c = torch.ones(o, dtype=torch.float64)
    if prenorm:
        c = 1.0 / math.sqrt(w3[0].numel()) / w3.abs().amax(dim=(1, 2))
    w1 = w3 * c[:, None, None]
    r = w1.square().mean(dim=(1, 2)).rsqrt()
    wn = w1 * r[:, None, None]
    return wn.reshape(w.shape), wn.square().sum(2), c * r


def demod_weight_backward(wn, sfac, gwn=None, gwsq=None):
    """G = g_wn + 2 g_wsq[o,i] wn;  g_w = sfac (G - wn mean(G wn)) -- the pre-normalisation cancels in wn, so sfac is all it leaves."""
    wn, sfac, gwn, gwsq = f64(wn), f64(sfac), f64(gwn), f64(gwsq)
    o, i = wn.shape[0], wn.shape[1]
    u = wn.reshape(o, i, -1)
    g = torch.zeros_like(u)
    if gwn is not None:
        g = g + gwn.reshape(u.shape)
    if gwsq is not None:
        g = g + 2.0 * gwsq[:, :, None] * u
    return (sfac[:, None, None] * (g - u * (g * u).mean(dim=(1, 2), keepdim=True))).reshape(wn.shape)


def style_factors(s, wsq, prenorm=False):
    """s [N,I], wsq [O,I] | None -> (sn, d | None, aux [N+1]): s1 = s / max_i|s| per row with ``prenorm`` else s; sn = s1 rsqrt(mean s1^2)
    (the mean runs over the whole batch); d = rsqrt(sn^2 wsq^T + 1e-8); aux = (row maxima M_n -- 1 without prenorm --, r)."""
    s = f64(s)
    m = s.abs().amax(1) if prenorm else torch.ones(s.shape[0], dtype=torch.float64)
    s1 = s / m[:, None]
    r = s1.square().mean().rsqrt()
    sn = s1 * r
    d = None if wsq is None else (sn.square() @ f64(wsq).t() + 1e-8).rsqrt()
    return sn, d, torch.cat([m, r.reshape(1)])


def style_factors_backward(sn, d, wsq, aux, gsn=None, gd=None, prenorm=False):
    """(g_s [N,I], g_wsq [O,I]) from the gradients on sn and d (either may be None).  With q = -1/2 gd d^3:
        g_wsq = q^T sn^2,   g_tot = gsn + 2 sn (q wsq),   A_n = <g_tot[n], sn[n]> / r,   c = sum_n A_n,   B_n = <sn[n], sn[n]>,
        g1 = r g_tot - (r^2 c / (N I)) sn                                                    (through sn = s1 rsqrt(mean s1^2))
        g_s = g1 / M_n - T sign(sn) R_n / (M_n ties_n),   R_n = r A_n - (r c / (N I)) B_n      (through s1 = s / max|s|, prenorm only)
    The tie rule: T marks every position of row n that attains the row maximum of |s| -- after the forward these are the positions with
    |sn| = r exactly --, ties_n counts them, and each takes an equal share of the derivative of the maximum (what ``norm(inf)`` does
    under autograd); a position below the maximum, by however little, takes none."""
    sn, d, wsq, aux, gsn, gd = f64(sn), f64(d), f64(wsq), f64(aux), f64(gsn), f64(gd)
    n, i = sn.shape
    m, r = aux[:n], aux[n]
    q = torch.zeros_like(d) if gd is None else -0.5 * gd * d ** 3
    gwsq = q.t() @ sn.square()
    gtot = 2.0 * sn * (q @ wsq)
    if gsn is not None:
        gtot = gtot + gsn
    a = (gtot * sn).sum(1) / r
    c = a.sum()
    g1 = r * gtot - (r * r * c / (n * i)) * sn
    if not prenorm:
        return g1, gwsq
    rn = r * a - (r * c / (n * i)) * sn.square().sum(1)
    tied = sn.abs() == sn.abs().amax(1, keepdim=True)
    ties = tied.sum(1, keepdim=True).to(torch.float64)
    gs = g1 / m[:, None] - tied.to(torch.float64) * sn.sign() * (rn / m)[:, None] / ties
    return gs, gwsq


def modconv_style_prep(styles, wsq=None, o=0, demod=True, pre_gain=1.0):
    """styles [N,I], wsq [I,OP] (the transposed, column-padded table of the convolution weight: wsq[i, o] = sum_k wn[o,i,k]^2, columns
    o .. OP-1 padding) -> (s, d | None): v = styles * pre_gain; with ``demod`` s = v rsqrt(mean v^2) over the batch and
    d = rsqrt(s^2 wsq[:, :o] + 1e-8), else s = v."""
    v = f64(styles) * pre_gain
    if not demod:
        return v, None
    s = v * v.square().mean().rsqrt()
    return s, (s.square() @ f64(wsq)[:, :o] + 1e-8).rsqrt()


def tie_styles(n, i, seed=0):
    """float32 styles [n, i] (n >= 4, i >= 3) of exactly representable values (multiples of 1/16 below 2 in magnitude) whose rows 1, 2
    and 3 carry the tie cases of the fp16-row backward, at the positions (0, i // 2, i - 1):
        row 1  a two-way tie of mixed sign          +2.5, -2.5
        row 2  a three-way tie of mixed sign        +3, -3, +3
        row 3  a near tie                           the maximum 2.75 and, one float32 ulp below it, -nextafter(2.75, 0): NOT a tie
    -> (styles, {row: (tied positions, runner-up position | None)})."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(-31, 32, (n, i), generator=g).to(torch.float32) / 16.0)
    p = (0, i // 2, i - 1)
    assert n >= 4 and i >= 3 and len(set(p)) == 3
    s[1, p[0]], s[1, p[1]] = 2.5, -2.5
    s[2, p[0]], s[2, p[1]], s[2, p[2]] = 3.0, -3.0, 3.0
    top = torch.tensor(2.75, dtype=torch.float32)
    s[3, p[2]], s[3, p[0]] = top, -torch.nextafter(top, torch.tensor(0.0))
    return s, {1: (p[:2], None), 2: (p, None), 3: (p[2:], p[0])}


def tie_corrections(sn, aux, gs, g1):
    """The share of the derivative of the row maximum that each position received: gs - g1 / M_n (``g1``: the same backward without the
    pre-normalisation), times sign(sn) -> [N, I]; and its exact value at a tied position, -<g1[n], s1[n]> / (M_n ties_n) -> [N]."""
    sn, aux, gs, g1 = f64(sn), f64(aux), f64(gs), f64(g1)
    n = sn.shape[0]
    m, r = aux[:n], aux[n]
    tied = sn.abs() == sn.abs().amax(1, keepdim=True)
    share = -(g1 * sn / r).sum(1) / m / tied.sum(1)
    return (gs - g1 / m[:, None]) * sn.sign(), share


# ------------------------------------------------------------------------------------------------
# how a result is judged
# ------------------------------------------------------------------------------------------------

def row_rel_err(got, ref, scale=None):
    """max over the rows (first axis) of max|got - ref| / max|ref| of that row -> (worst figure, its row).  A vector is judged element by
    element.  A row whose reference is zero passes only with zeros.  ``scale`` [rows]: a lower limit of the row's denominator, for the
    few rows whose exact value is a complete cancellation (given by the caller as the magnitude of the terms that cancel)."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    g2, r2 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    num, den = (g2 - r2).abs().amax(1), r2.abs().amax(1)
    if scale is not None:
        den = torch.maximum(den, f64(scale).reshape(-1).expand_as(den))
    e = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, math.inf), torch.zeros_like(num)))
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    k = int(e.argmax())
    return float(e[k]), k


def linear_excess(got, ref, absprod, c, extra=None):
    """Elementwise judgement of a float32 sum of products: max of |got - ref| / (c 2^-24 absprod + extra) -> (worst ratio, flat index);
    the result is within its bound when the ratio is <= 1.  ``absprod`` = sum_k |a_k| |b_k| |scale| of each output element in float64,
    ``c`` the longest chain of float32 roundings on the way to one element, ``extra`` an additive allowance (the bias term)."""
    got, ref, bound = f64(got), f64(ref), c * U32 * f64(absprod)
    if extra is not None:
        bound = bound + f64(extra)
    assert got.shape == ref.shape == bound.shape, (tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    err = (got - ref).abs().reshape(-1)
    bound = bound.reshape(-1)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    k = int(ratio.argmax())
    return float(ratio[k]), k
