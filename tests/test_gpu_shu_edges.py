"""Edge table of the Spectral Hint Unit kernels, csrc/shu.hip (run with -m gpu on an MI355X).

Every kernel and instantiation shu.hip can launch, called directly (``kernels.shu_*``, or the C ABI where the wrapper never picks an
entry point: the ``_n<64>`` forms at the shipped geometry) with inputs this file controls, and judged per element against the float64
restatement tests/shu_f64.py (itself checked on the CPU by tests/test_shu_f64_cpu.py, which also shows that the cases below catch each of
a list of deliberate defects and that the table claims every launch site of the source):

    |got - ref| <= k * 2^-24 * A_e        A_e = the sum of the absolute terms of the element (the restatement's magnitude twin)

with k counted from the arithmetic of the kernel, never fitted to a result (TW = 4: a table twiddle within 2 ulp):
  shu_rfft2_shift_kernel, _n<64>, _n<128>   pass 1 S+1+TW, pass 2 (K = 2S) 2S+1+TW, scale 1                        k = 3S + 3 + 2TW
  shu_rfft2_shift_n_kernel<16|32>           pass 1 S+1+TW, pass 2 S+2+TW, scale 1                                  k = 2S + 4 + 2TW
  shu_spectral_kernel, _tail_kernel         stage 1 66 (K = 64, bias), carried through the ReLU (1-Lipschitz, the choice made here: no
                                            dyadic inputs); stage 2 cw * t 1, K = 64B: 64B + 1                      shu_f64.spectral_bar
  shu_split_irfft2_kernel, _n<S>            band sum B+1 (0 at B = 1); r < 64: (r+3+TW) + (r/2+2+TW) + 1;
                                            r >= 64: 1 + (2r+1+TW) + (r+1+TW) + 1; accumulate adds 2^-24 |old|      shu_f64.split_k
  shu_split_adjoint_kernel, _n<S>           per level (r+1+TW) + (r+2+TW) + 1 + levels, summed over the levels      shu_f64.adjoint_k
An element with A_e = 0 (a bin outside a level's crop, Im of the DC / Nyquist column of an impulse's spectrum where the restatement's
exact tables say so) must therefore be an exact zero.  All inputs come from seeded generators."""
import ctypes
import re

import numpy as np
import pytest
import torch

import shu_f64 as sf
from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT_BITS = 0x7A5C3B1D   # the sentinel: a finite float32 (2.86e35) no kernel here produces
SENT = float(np.array([SENT_BITS], np.uint32).view(np.float32)[0])

FWD, FWD_N = 'shu_rfft2_shift_kernel', 'shu_rfft2_shift_n_kernel'
SPEC, SPEC_T = 'shu_spectral_kernel', 'shu_spectral_tail_kernel'
SPLIT, SPLIT_N = 'shu_split_irfft2_kernel', 'shu_split_irfft2_n_kernel'
ADJ, ADJ_N = 'shu_split_adjoint_kernel', 'shu_split_adjoint_n_kernel'

SIZES = (16, 32, 64, 128)
PYRAMIDS = [(s, low) for s in SIZES for low in (4, 8, 16, 32, 64, 128) if low <= s]          # the 18 legal (size, lowest)
SPEC_PLANES = {4: (1, 4), 68: (4, 17), 144: (16, 9), 544: (32, 17), 2112: (64, 33), 8320: (128, 65)}


def levels_of(size, lowest):
    return [r for r in (4, 8, 16, 32, 64, 128) if lowest <= r <= size]


def rnd(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def uni(seed, lo, hi, *shape):
    return np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32)


def gauss_tables(res, seed=40):
    """One table [r, r/2+1] per level: random weights in (0.3, 1.3), so that a table read at the wrong row, column or level shows."""
    return [uni(seed + r, 0.3, 1.3, r, r // 2 + 1) for r in res]


def skip_set(pattern, res):
    nl = len(res)
    return {'none': (), 'low_only': tuple(range(1, nl)), 'top_only': tuple(range(nl - 1)), 'all_but_top': (nl - 1,),
            'alternate': tuple(range(1, nl, 2)), 'no64': (res.index(64),) if 64 in res else (),
            'no128': (res.index(128),) if 128 in res else (), 'all': tuple(range(nl))}[pattern]


# ------------------------------------------------------------------------------------------------
# host side of a case: inputs(case) -> dict of float32 arrays; reference(case, inp, defect) -> [(name, ref, bar) or None, ...]
# (numpy only: tests/test_shu_f64_cpu.py runs these without a GPU)
# ------------------------------------------------------------------------------------------------

def inputs(case):
    k = case['kind']
    if k == 'fwd':
        s = case['size']
        if case['data'] == 'random':
            return dict(x=rnd(1 + s, 2, 3, s, s))
        if case['data'] == 'c1':
            return dict(x=rnd(2 + s, 1, 1, s, s))
        pos = [0, 1, s // 2 - 1, s // 2, s - 1]
        x = np.zeros((1, 25, s, s), np.float32)
        val = uni(3 + s, 0.5, 1.5, 25) * np.where(np.arange(25) % 2 == 0, 1, -1).astype(np.float32)
        for ch, (h0, w0) in enumerate((a, b) for a in pos for b in pos):
            x[0, ch, h0, w0] = val[ch]
        return dict(x=x)
    if k == 'spec':
        h, w = SPEC_PLANES[case['p']]
        b = case['bands']
        return dict(t=rnd(5, 3, 64, h, w), w0=rnd(6, 64, 64) / 8, b0=rnd(7, 64) * 0.5, w1=rnd(8, 64 * b, 64) / 8,
                    cw=uni(9, 0.2, 1.0, b, h, w))
    s, res = case['size'], levels_of(case['size'], case['lowest'])
    n, c, b = case.get('n', 2), case.get('c', 3), case.get('bands', 1)
    inp = dict(gauss=gauss_tables(res))
    if k in ('split', 'dot'):
        if case.get('data') == 'bins':
            bins = sorted({(row, col) for r in res for row in (s // 2 - r // 2 + d for d in (-1, 0, r // 2 - 1, r - 1, r))
                           for col in (0, 1, r // 2 - 1, r // 2, r // 2 + 1) if 0 <= row < s and 0 <= col <= s // 2})
            c = 2 * len(bins)
            y = np.zeros((1, 2 * c, s, s // 2 + 1), np.float32)
            val = uni(11 + s, 0.5, 1.5, len(bins))
            for i, (row, col) in enumerate(bins):
                y[0, 2 * i, row, col] = val[i]                    # channel 2i: the bin in Re
                y[0, c + 2 * i + 1, row, col] = -val[i]           # channel 2i + 1: the bin in Im
            inp.update(y=y, bins=bins)
        else:
            inp['y'] = rnd(12 + s + case['lowest'], n, 2 * c * b, s, s // 2 + 1)
        if b > 1:
            inp['cw'] = uni(13, 0.2, 1.0, b, s, s // 2 + 1)
        if case.get('accumulate'):
            inp['old'] = [rnd(14 + r, n, c + 8, r, r) for r in res]
    if k in ('adj', 'dot'):
        if case.get('data') == 'impulse':
            r = res[-1]
            px = [(row, col) for row in (0, 31, 32, 63, 64, 127) if row < r for col in (0, 1, r - 1)]
            g = np.zeros((1, len(px), r, r), np.float32)
            val = uni(15 + r, 0.5, 1.5, len(px))
            for ch, (row, col) in enumerate(px):
                g[0, ch, row, col] = val[ch]
            inp['g'] = [np.zeros((1, len(px), q, q), np.float32) for q in res[:-1]] + [g]
        else:
            inp['g'] = [rnd(16 + r + s, n, c, r, r) for r in res]
    return inp


def reference(case, inp, defect=None):
    k = case['kind']
    if k == 'fwd':
        return [('T', sf.rfft2_shift(inp['x'], defect), sf.fwd_k(case['size']) * sf.U32 * sf.rfft2_shift(inp['x'], mag=True))]
    if k == 'spec':
        a = (inp['t'], inp['w0'], inp['b0'], inp['w1'], inp['cw'])
        return [('S', sf.spectral(*a, defect=defect), sf.spectral_bar(*a))]
    s, res = case['size'], levels_of(case['size'], case['lowest'])
    skip = skip_set(case.get('skip', 'none'), res)
    if k == 'split':
        b = case.get('bands', 1)
        old = None
        if case.get('accumulate'):
            c = inp['y'].shape[1] // (2 * b)
            old = [o[:, 5:5 + c] for o in inp['old']]
        ref = sf.split_irfft2(inp['y'], inp.get('cw'), inp['gauss'], res, old, skip, defect)
        mag = sf.split_irfft2(inp['y'], inp.get('cw'), inp['gauss'], res, None, skip, mag=True)
        return [None if l in skip else
                (f'out{r}', ref[l], sf.U32 * (sf.split_k(r, b) * mag[l] + (np.abs(sf.f64(old[l])) if old is not None else 0.0)))
                for l, r in enumerate(res)]
    if k == 'adj':
        grads = [None if l in skip else g for l, g in enumerate(inp['g'])]
        if len(skip) == len(res):
            n, c = inp['g'][0].shape[:2]
            z = np.zeros((n, 2 * c, s, s // 2 + 1))
            return [('GS', z, z)]
        return [('GS', sf.split_adjoint(grads, inp['gauss'], res, s, defect), sf.adjoint_bar(grads, inp['gauss'], res, s))]
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------

def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def _lib():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib as lib
    return lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cabi(name, *args):
    """One call of the C ABI on the current stream; a negative status raises ShgError."""
    lib = _lib()
    lib.check(getattr(lib.get_lib(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def _arrays(tensors):
    p, s = (ctypes.c_void_p * len(tensors))(), (ctypes.c_long * len(tensors))()
    for l, t in enumerate(tensors):
        p[l] = None if t is None else t.data_ptr()
        s[l] = 0 if t is None else t.stride(0)
    return p, s


def split_call(form, y, cw, gauss, outs, accumulate, res):
    """'wrapper': kernels.shu_split_irfft2 (the shipped kernel at 64 / five levels); 'n': shg_shu_split_irfft2_n_f32 whatever the size."""
    if form == 'wrapper':
        _kk().shu_split_irfft2(y, cw, gauss, outs, accumulate)
        return
    n, bands = y.shape[0], (1 if cw is None else cw.shape[0])
    g_arr, _ = _arrays(gauss)
    o_arr, s_arr = _arrays(outs)
    cabi('shg_shu_split_irfft2_n_f32', ptr(y), ptr(cw), g_arr, o_arr, s_arr, n, y.shape[1] // (2 * bands), bands, int(accumulate), y.shape[2],
         (ctypes.c_int * len(res))(*res), len(res))


def adjoint_call(form, grads, gauss, n, c, size, res):
    if form == 'wrapper':
        return _kk().shu_split_adjoint(grads, gauss, n, c, size)
    out = torch.full((n, 2 * c, size, size // 2 + 1), SENT, device=DEV)
    g_arr, s_arr = _arrays(grads)
    t_arr, _ = _arrays(gauss)
    cabi('shg_shu_split_adjoint_n_f32', g_arr, s_arr, t_arr, ptr(out), n, c, size, (ctypes.c_int * len(res))(*res), len(res))
    return out


def fwd_run(case, inp):
    s, x = case['size'], inp['x']
    n, c = x.shape[:2]
    wide = torch.full((n, c + 2, s, s), float('nan'), device=DEV)         # a channel slice: the batch stride is not C * S * S
    wide[:, 2:] = dev(x)
    view = wide[:, 2:]

    def call():
        if case['form'] == 'cabi':
            t = torch.full((n, 2 * c, s, s // 2 + 1), SENT, device=DEV)
            cabi('shg_shu_rfft2_shift_n_f32', ptr(view), view.stride(0), ptr(t), n, c, s)
            return [t]
        return [_kk().shu_rfft2_shift(view)]
    return call


def spec_run(case, inp):
    kk = _kk()
    b, (h, w) = case['bands'], SPEC_PLANES[case['p']]
    p = h * w
    t, b0, cw = dev(inp['t']), dev(inp['b0']), dev(inp['cw'])
    w0p = kk.mfma_pack_rows(dev(inp['w0']))
    w1p = kk.mfma_pack_rows(dev(inp['w1']).reshape(64, b, 64).permute(1, 0, 2).contiguous()).reshape(-1, 2, 64)      # [B][o][i], as SHU._packed

    def call():
        out = kk.shu_spectral(t, w0p, b0, w1p, cw)
        if not case.get('sentinel'):
            return [out]
        # the same call through the C ABI into a buffer with 64 more floats than [N,64,P]: a store at a position >= P of the last row
        # of the last sample would land there (one at any other row lands in the next row and breaks the bit equality below)
        n = t.shape[0]
        buf = torch.full((n * 64 * p + 64,), SENT, device=DEV)
        cabi('shg_shu_spectral_n_f32', ptr(t), ptr(w0p), ptr(b0), ptr(w1p), ptr(cw), ptr(buf), n, 64, p, b)
        torch.cuda.synchronize()
        assert bool((buf[n * 64 * p:].cpu().view(torch.int32) == SENT_BITS).all()), f'{SPEC_T}: stored at a position >= P = {p}'
        assert torch.equal(buf[:n * 64 * p].view_as(out), out), f'{SPEC_T}: the C ABI call and the wrapper differ'
        return [out]
    return call


def split_run(case, inp):
    s, res = case['size'], levels_of(case['size'], case['lowest'])
    b, acc = case.get('bands', 1), bool(case.get('accumulate'))
    skip = skip_set(case.get('skip', 'none'), res)
    y, cw, gauss = dev(inp['y']), dev(inp.get('cw')), [dev(g) for g in inp['gauss']]
    n, c = y.shape[0], y.shape[1] // (2 * b)

    def fresh():
        if acc:
            return [dev(o) for o in inp['old']]
        return [torch.full((n, c + 8, r, r), SENT, device=DEV) for r in res]

    def call():
        wide = fresh()
        before = [w_.clone() for w_ in wide]
        outs = [None if l in skip else w_[:, 5:5 + c] for l, w_ in enumerate(wide)]
        split_call(case['form'], y, cw, gauss, outs, acc, res)
        torch.cuda.synchronize()
        for l, r in enumerate(res):          # the channels beside the slice (and a skipped level as a whole) keep their bits
            keep = torch.ones(c + 8, dtype=torch.bool, device=DEV)
            if l not in skip:
                keep[5:5 + c] = False
            assert torch.equal(wide[l][:, keep].view(torch.int32), before[l][:, keep].view(torch.int32)), \
                f'level {r}: written outside the channel slice'
        if skip:                              # the levels kept: bit for bit what the call with no level skipped gives
            full = fresh()
            split_call(case['form'], y, cw, gauss, [w_[:, 5:5 + c] for w_ in full], acc, res)
            for l, r in enumerate(res):
                if l not in skip:
                    assert torch.equal(full[l][:, 5:5 + c].view(torch.int32), outs[l].view(torch.int32)), \
                        f'level {r}: differs from the call with no level skipped (skipped {[res[q] for q in skip]})'
        return outs
    return call


def adj_run(case, inp):
    s, res = case['size'], levels_of(case['size'], case['lowest'])
    skip = skip_set(case.get('skip', 'none'), res)
    gauss = [dev(g) for g in inp['gauss']]
    n, c = inp['g'][0].shape[:2]
    grads = []
    for l, g in enumerate(inp['g']):          # channel slices of wider tensors: the batch stride is not C * r * r
        wide = torch.full((n, c + 3, g.shape[2], g.shape[3]), float('nan'), device=DEV)
        wide[:, 1:1 + c] = dev(g)
        grads.append(None if l in skip else wide[:, 1:1 + c])

    def call():
        return [adjoint_call(case['form'], grads, gauss, n, c, s, res)]
    return call


def dot_run(case, inp):
    split, adj = split_run(dict(case, kind='split'), inp), adj_run(dict(case, kind='adj'), inp)

    def call():
        return split() + adj()
    return call


RUN = dict(fwd=fwd_run, spec=spec_run, split=split_run, adj=adj_run, dot=dot_run)


# ------------------------------------------------------------------------------------------------
# the table: id -> (case, expect, forbid)
# ------------------------------------------------------------------------------------------------

def _table():
    t = {}

    def add(cid, case, expect, forbid=()):
        assert cid not in t, cid
        t[cid] = (case, tuple(expect), tuple(forbid))

    # ---- forward transform: the shipped kernel (wrapper at 64), _n<16|32|128> (wrapper), _n<64> (C ABI only)
    for s, form, tag in ((16, 'wrapper', '16'), (32, 'wrapper', '32'), (64, 'wrapper', '64s'), (64, 'cabi', '64n'), (128, 'wrapper', '128')):
        exp, forb = ([FWD], [FWD_N]) if tag == '64s' else ([f'{FWD_N}<{s}>'], [FWD])
        for data in ('random', 'c1', 'impulse'):
            add(f'fwd_{tag}_{data}', dict(kind='fwd', size=s, form=form, data=data), exp, forb)
    # ---- spectral stage: whole tiles on shu_spectral_kernel, any P % 64 != 0 on the guarded twin
    for p, bands in [(4, 3), (144, 3), (544, 3), (8320, 3)] + [(p, b) for p in (68, 2112) for b in (1, 2, 7, 8)]:
        exp, forb = ([SPEC], [SPEC_T]) if p % 64 == 0 else ([SPEC_T], [SPEC])
        add(f'spec_p{p}_b{bands}', dict(kind='spec', p=p, bands=bands), exp, forb)
    add('spec_p68_b3_sentinel', dict(kind='spec', p=68, bands=3, sentinel=True), [SPEC_T], [SPEC])
    # ---- split stage and adjoint at the 18 pyramids; (64, 4) on the shipped kernels (wrapper) and on _n<64> (C ABI)
    for kind, ship, gen in (('split', SPLIT, SPLIT_N), ('adj', ADJ, ADJ_N)):
        def route(s, low, form):
            return ([ship], [gen]) if (s, low, form) == (64, 4, 'wrapper') else ([f'{gen}<{s}>'], [ship])
        for s, low in PYRAMIDS:
            add(f'{kind}_{s}_{low}', dict(kind=kind, size=s, lowest=low, form='wrapper'), *route(s, low, 'wrapper'))
        add(f'{kind}_64_4_n', dict(kind=kind, size=64, lowest=4, form='n'), *route(64, 4, 'n'))
        # skipped levels / None gradients
        for s, form, tag, pats in ((128, 'wrapper', '128_4', ('low_only', 'top_only', 'all_but_top', 'alternate', 'no64', 'no128')),
                                   (64, 'wrapper', '64_4', ('low_only', 'top_only', 'all_but_top')),
                                   (64, 'n', '64_4_n', ('low_only', 'top_only', 'all_but_top'))):
            for pat in pats + (('all',) if kind == 'adj' else ()):
                add(f'{kind}_skip_{pat}_{tag}', dict(kind=kind, size=s, lowest=4, form=form, skip=pat), *route(s, 4, form))
    # ---- split: bands, single bins, accumulate, channel counts
    for b in (2, 8):
        for s, low in ((16, 16), (64, 4), (128, 32)):
            add(f'split_b{b}_{s}_{low}', dict(kind='split', size=s, lowest=low, form='wrapper', bands=b),
                *(([SPLIT], [SPLIT_N]) if s == 64 else ([f'{SPLIT_N}<{s}>'], [SPLIT])))
    add('split_bins_128_4', dict(kind='split', size=128, lowest=4, form='wrapper', data='bins'), [f'{SPLIT_N}<128>'], [SPLIT])
    add('split_bins_64_4', dict(kind='split', size=64, lowest=4, form='wrapper', data='bins'), [SPLIT], [SPLIT_N])
    add('split_bins_64_4_n', dict(kind='split', size=64, lowest=4, form='n', data='bins'), [f'{SPLIT_N}<64>'], [SPLIT])
    for s, form, tag in ((16, 'wrapper', '16_4'), (64, 'wrapper', '64_4'), (64, 'n', '64_4_n'), (128, 'wrapper', '128_4')):
        add(f'split_acc_{tag}', dict(kind='split', size=s, lowest=4, form=form, accumulate=True),
            *(([SPLIT], [SPLIT_N]) if tag == '64_4' else ([f'{SPLIT_N}<{s}>'], [SPLIT])))
    add('split_c1_32_4', dict(kind='split', size=32, lowest=4, form='wrapper', c=1), [f'{SPLIT_N}<32>'], [SPLIT])
    add('split_c12_128_16', dict(kind='split', size=128, lowest=16, form='wrapper', c=12), [f'{SPLIT_N}<128>'], [SPLIT])
    add('split_c33_64_4', dict(kind='split', size=64, lowest=4, form='wrapper', c=33), [SPLIT], [SPLIT_N])
    add('split_c33_64_8', dict(kind='split', size=64, lowest=8, form='wrapper', c=33), [f'{SPLIT_N}<64>'], [SPLIT])
    # ---- adjoint: impulse gradients on the seams of the 32-row blocks
    add('adj_impulse_128_128', dict(kind='adj', size=128, lowest=128, form='wrapper', data='impulse'), [f'{ADJ_N}<128>'], [ADJ])
    add('adj_impulse_64_64', dict(kind='adj', size=64, lowest=64, form='wrapper', data='impulse'), [f'{ADJ_N}<64>'], [ADJ])
    add('adj_impulse_64_4', dict(kind='adj', size=64, lowest=4, form='wrapper', data='impulse'), [ADJ], [ADJ_N])
    # ---- the kernels against each other: <split(s), g> = <s, adjoint(g)>
    for s, form, tag in ((16, 'wrapper', '16_4'), (64, 'wrapper', '64_4'), (64, 'n', '64_4_n'), (128, 'wrapper', '128_4')):
        ship = tag == '64_4'
        add(f'dot_{tag}', dict(kind='dot', size=s, lowest=4, form=form),
            [SPLIT, ADJ] if ship else [f'{SPLIT_N}<{s}>', f'{ADJ_N}<{s}>'], [SPLIT_N, ADJ_N] if ship else [SPLIT, ADJ])
    return t


CASES = _table()


def _kernel_of(expect):
    return ' + '.join(expect)


@pytest.mark.parametrize('cid', sorted(CASES))
def test_edge(cid):
    case, expect, forbid = CASES[cid]
    inp = inputs(case)
    call = RUN[case['kind']](case, inp)
    torch.cuda.synchronize()
    got, names = launched(call, expect=expect)
    kern = sorted({re.sub(r'^void |\(.*$', '', n) for n in names if 'shu_' in n})
    for p in expect:
        assert any_hit(p, names), f'{cid}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not any_hit(p, names), f'{cid}: {p} must not run; ran {kern}'
    who = _kernel_of(expect)
    if case['kind'] == 'dot':
        recs = _dot_records(case, inp, got)
    else:
        recs = []
        for rec, g in zip(reference(case, inp), got):
            if rec is None:
                assert g is None
                continue
            name, ref, bar = rec
            assert tuple(g.shape) == ref.shape, f'{cid}: {who}: {name}: shape {tuple(g.shape)}, expected {ref.shape}'
            recs.append((name,) + sf.worst_ratio(g.cpu().numpy(), ref, bar))
        if case.get('data') in ('impulse', 'bins') and case['kind'] != 'adj':
            assert _exact_zero_elements(case, inp) > 0, f'{cid}: the case was to hold elements that must be exact zeros'
    print(f'SHUEDGE {cid} kernel={who} ' + ' '.join(f'{nm}={ratio:.3e}@{idx}' for nm, ratio, idx in recs))
    for nm, ratio, idx in recs:
        assert ratio <= 1.0, f'{cid}: {who}: {nm}: worst err / bar = {ratio:.3e} at index {idx}'


def _exact_zero_elements(case, inp):
    """How many elements the restatement pins to an exact zero (bar == 0) where these cases are built to have them: Im of columns 0 and
    S/2 of an impulse's spectrum; a level's output for a bin outside its crop."""
    bars = [rec[2] for rec in reference(case, inp) if rec is not None]
    if case['kind'] == 'fwd':
        c, s = inp['x'].shape[1], case['size']
        im = bars[0][:, c:]
        return int((im[..., 0] == 0).sum() + (im[..., s // 2] == 0).sum())
    return min(int((bar == 0).sum()) for bar in bars[:-1])          # (every level below the top has bins outside its crop)


def _dot_records(case, inp, got):
    """<split(s), g> and <s, adjoint(g)> in float64 from the device results; each is within its kernel's bars of the same exact number."""
    res = levels_of(case['size'], case['lowest'])
    outs, gs = got[:len(res)], got[len(res)]
    lhs = sum(float((o.cpu().double().numpy() * sf.f64(g)).sum()) for o, g in zip(outs, inp['g']))
    rhs = float((gs.cpu().double().numpy() * sf.f64(inp['y'])).sum())
    split_bars = reference(dict(case, kind='split'), inp)
    (_, _, adj_bar), = reference(dict(case, kind='adj'), inp)
    bound = sum(float((bar * np.abs(sf.f64(g))).sum()) for (_, _, bar), g in zip(split_bars, inp['g'])) + \
        float((adj_bar * np.abs(sf.f64(inp['y']))).sum())
    return [('<split s,g> - <s,adj g>', abs(lhs - rhs) / bound, (0,))]


def test_the_c_abi_accepts_exactly_the_18_pyramids():
    """shu_levels_ok of shu.hip from the outside: every (size, level list) of the grid is accepted by both size-general entry points if and
    only if it is one of the 18 (the legal ones are also the cases above; here they run once more on one tiny plane)."""
    lib = _lib()
    f_split, f_adj = lib.get_lib().shg_shu_split_irfft2_n_f32, lib.get_lib().shg_shu_split_adjoint_n_f32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    accepted = []
    for s in SIZES:
        for low in (2, 4, 8, 16, 32, 64, 128, 256):
            res = [r for r in (2, 4, 8, 16, 32, 64, 128, 256) if low <= r <= s]
            if not res:
                res = [low]
            y = torch.zeros(1, 2, s, s // 2 + 1, device=DEV)
            outs = [torch.zeros(1, 1, r, r, device=DEV) for r in res]
            gauss = [torch.ones(r, r // 2 + 1, device=DEV) for r in res]
            g_arr, _ = _arrays(gauss)
            o_arr, s_arr = _arrays(outs)
            ra = (ctypes.c_int * len(res))(*res)
            rc1 = f_split(ptr(y), None, g_arr, o_arr, s_arr, 1, 1, 1, 0, s, ra, len(res), stream)
            rc2 = f_adj(o_arr, s_arr, g_arr, ptr(y), 1, 1, s, ra, len(res), stream)
            torch.cuda.synchronize()
            assert (rc1 == 0) == (rc2 == 0), (s, res, rc1, rc2)
            if rc1 == 0:
                accepted.append((s, low))
    assert accepted == PYRAMIDS, accepted
