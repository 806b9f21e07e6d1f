"""The float64 restatement of the Spectral Hint Unit kernels (tests/shu_f64.py) is itself right, and the GPU table built on it
(tests/test_gpu_shu_edges.py) is sharp and complete (CPU only, no kernel runs).

  * the restatement, written with explicit cosine / sine matrices, against ``torch.fft.rfftn`` / ``irfftn`` and ``conv2d`` in float64 (the
    ``fft_form`` of tests/test_gpu_shu_geometry.py) to 1e-12 at all 18 pyramids; ``split_adjoint`` against the autograd transpose of the
    ``torch.fft`` form and as a transpose of ``split_irfft2`` (<split s, g> = <s, adjoint g>);
  * the magnitude twins dominate the values they belong to, and vanish exactly where the tests rely on exact zeros;
  * sensitivity: each deliberate defect of shu_f64 lies at least 100 bars away from the restatement on a named case of the GPU table;
  * coverage: every (kernel, instantiation) a ``hipLaunchKernelGGL`` site of shu.hip can launch is the expected route of a case;
  * the 18 legal pyramids are what ``kernels._shu_levels`` and the C ABI's level check accept, and the Gaussian staging area of
    ``shu_split_irfft2_n_kernel`` holds the scalar-level tables of every one of them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shu_f64 as sf
import test_gpu_shu_edges as table
from conftest import ROOT
from test_gpu_shu_edges import CASES, PYRAMIDS, inputs, levels_of, reference

TOL = 1e-12
SRC = os.path.join(ROOT, 'sh-gan_amd', 'csrc', 'shu.hip')


def rnd(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape)


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def torch_split(sre, sim, gauss, res, size):
    """shgan.py:326-334 with torch.fft on a band-summed spectrum."""
    sp = torch.complex(sre, sim)
    out = []
    for r, g in zip(res, gauss):
        s_ = sp[:, :, size // 2 - r // 2: size // 2 + r // 2, 0: r // 2 + 1] * g[None, None]
        s_ = torch.cat([s_[:, :, r - r // 2 - 1:], s_[:, :, :r - r // 2 - 1]], dim=2)
        out.append(torch.fft.irfftn(s_, dim=(2, 3), norm='forward'))
    return out


# ------------------------------------------------------------------------------------------------
# the restatement against torch.fft / conv2d
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('size', [16, 32, 64, 128])
def test_forward_matches_torch_fft(size):
    x = rnd(size, 2, 3, size, size)
    sp = torch.fft.rfftn(torch.from_numpy(x), dim=(2, 3), norm='forward')
    sp = torch.cat([sp[:, :, size // 2 + 1:], sp[:, :, :size // 2 + 1]], dim=2)
    want = torch.cat([sp.real, sp.imag], dim=1).numpy()
    got = sf.rfft2_shift(x)
    assert got.shape == (2, 6, size, size // 2 + 1)
    assert close(got, want) < TOL
    mag = sf.rfft2_shift(x, mag=True)
    assert (mag >= np.abs(got) * (1 - 1e-12)).all()


@pytest.mark.parametrize('bands', [1, 3])
def test_spectral_matches_conv2d(bands):
    t, w0, b0, w1, cw = rnd(1, 2, 64, 4, 17), rnd(2, 64, 64) / 8, rnd(3, 64) * 0.5, rnd(4, 64 * bands, 64) / 8, rnd(5, bands, 4, 17)
    tt = torch.relu(torch.nn.functional.conv2d(torch.from_numpy(t), torch.from_numpy(w0)[:, :, None, None], torch.from_numpy(b0)))
    y = torch.nn.functional.conv2d(tt, torch.from_numpy(w1)[:, :, None, None])                   # flat output channel o * bands + k
    want = (y.reshape(2, 64, bands, 4, 17) * torch.from_numpy(cw)[None, None]).sum(2).numpy()
    got = sf.spectral(t, w0, b0, w1, cw)
    assert close(got, want) < TOL
    assert 0.3 < float((tt == 0).double().mean()) < 0.7                                          # the ReLU cuts about half
    bar = sf.spectral_bar(t, w0, b0, w1, cw)
    assert (bar > 0).all() and (bar < 1e-3 * np.abs(want).max()).all()


@pytest.mark.parametrize('size,lowest', PYRAMIDS)
def test_split_and_adjoint_match_torch_fft_and_autograd(size, lowest):
    res, bands, n, c = levels_of(size, lowest), 2, 2, 3
    nh = size // 2 + 1
    y, cw = rnd(size + lowest, n, 2 * c * bands, size, nh), rnd(7, bands, size, nh)
    gauss = [rnd(8 + r, r, r // 2 + 1) for r in res]
    # band sum + split against torch.fft
    yt = torch.from_numpy(y).reshape(n, 2 * c, bands, size, nh)
    st = (yt * torch.from_numpy(cw)[None, None]).sum(2)
    want = torch_split(st[:, :c], st[:, c:], [torch.from_numpy(g) for g in gauss], res, size)
    got = sf.split_irfft2(y, cw, gauss, res)
    mag = sf.split_irfft2(y, cw, gauss, res, mag=True)
    for r, a, b, m in zip(res, got, want, mag):
        assert a.shape == (n, c, r, r)
        assert close(a, b.numpy()) < TOL, r
        assert (m >= np.abs(a) * (1 - 1e-12)).all(), r
    # the adjoint against the autograd transpose of the torch.fft form, and as a transpose of the restatement
    s = rnd(9, n, 2 * c, size, nh)
    grads = [rnd(10 + r, n, c, r, r) for r in res]
    with torch.enable_grad():
        sr = torch.from_numpy(s).requires_grad_(True)
        outs = torch_split(sr[:, :c], sr[:, c:], [torch.from_numpy(g) for g in gauss], res, size)
        (want_gs,) = torch.autograd.grad(sum((o * torch.from_numpy(g)).sum() for o, g in zip(outs, grads)), sr)
    got_gs = sf.split_adjoint(grads, gauss, res, size)
    assert close(got_gs, want_gs.numpy()) < TOL
    lhs = sum(float((o * g).sum()) for o, g in zip(sf.split_irfft2(s, None, gauss, res), grads))
    rhs = float((got_gs * s).sum())
    assert abs(lhs - rhs) < TOL * max(abs(lhs), float(np.abs(got_gs * s).sum()))
    # levels without a gradient: the sum over the others
    some = [g if l % 2 == 0 else None for l, g in enumerate(grads)]
    shares = sf.split_adjoint(grads, gauss, res, size, per_level=True)
    assert close(sf.split_adjoint(some, gauss, res, size), sum(sh for l, sh in enumerate(shares) if l % 2 == 0)) < TOL


def test_skip_and_accumulate_of_the_restatement():
    res = levels_of(64, 4)
    y, gauss = rnd(1, 1, 4, 64, 33), [rnd(2 + r, r, r // 2 + 1) for r in res]
    full = sf.split_irfft2(y, None, gauss, res)
    part = sf.split_irfft2(y, None, gauss, res, skip=(1, 3))
    assert part[1] is None and part[3] is None and all(np.array_equal(part[l], full[l]) for l in (0, 2, 4))
    old = [rnd(3 + r, 1, 2, r, r) for r in res]
    acc = sf.split_irfft2(y, None, gauss, res, accumulate_into=old)
    assert all(np.array_equal(a, o + f) for a, o, f in zip(acc, old, full))


def test_exact_zeros_of_the_twins():
    """An impulse's spectrum has Im exactly 0 on columns 0 and S/2 where (u h0) mod S/2 == 0 -- the twin says so by itself; a bin outside
    a level's crop leaves that level's twin at exactly 0."""
    case = CASES['fwd_64s_impulse'][0]
    inp = inputs(case)
    (_, ref, bar), = reference(case, inp)
    pos = [0, 1, 31, 32, 63]
    for ch, (h0, w0) in enumerate((a, b) for a in pos for b in pos):
        for col in (0, 32):
            for u in range(64):
                zero = (u * h0 + col * w0) % 32 == 0
                row = (u + 31) % 64
                assert (bar[0, 25 + ch, row, col] == 0) == zero, (h0, w0, u, col)
                if zero:
                    assert ref[0, 25 + ch, row, col] == 0
    assert table._exact_zero_elements(case, inp) > 0
    for cid in ('split_bins_64_4', 'split_bins_128_4'):
        case = CASES[cid][0]
        inp = inputs(case)
        res, size = levels_of(case['size'], 4), case['size']
        recs = reference(case, inp)
        for (name, ref, bar), r in zip(recs, res):
            for i, (row, col) in enumerate(inp['bins']):
                crop = size // 2 - r // 2
                inside = crop <= row < crop + r and col <= r // 2
                j = (row - crop - (r // 2 - 1)) % r                   # the un-shifted row: frequency j along y
                for ch in (2 * i, 2 * i + 1):
                    # (Im of a bin on the DC / Nyquist column does reach the output through the pass along y -- only Im AFTER that pass
                    # is dropped -- unless its row is the DC or Nyquist frequency as well: the bin of a real plane's real coefficient)
                    live = inside and not (ch == 2 * i + 1 and col in (0, r // 2) and j in (0, r // 2))
                    assert bool((bar[0, ch] > 0).any()) == live, (cid, r, row, col, ch)
                    if not live:
                        assert not ref[0, ch].any()


# ------------------------------------------------------------------------------------------------
# sensitivity: defect -> the GPU case that catches it at >= 100 bars
# ------------------------------------------------------------------------------------------------

DEFECTS = [
    ('row shift off by one', 'rowshift', 'fwd_64s_random'),
    ('row shift off by one (size-general)', 'rowshift', 'fwd_16_c1'),
    ('Im of the DC / Nyquist column not ignored in c2r', 'c2r_im', 'split_bins_64_4'),
    ('Im of the DC / Nyquist column not ignored in c2r (matrix-core levels)', 'c2r_im', 'split_128_64'),
    ('interior column weight 1, forward', 'colweight', 'split_16_4'),
    ('interior column weight 1, adjoint', 'colweight', 'adj_16_4'),
    ('crop start off by one row', 'crop', 'split_32_8'),
    ('crop start off by one row, adjoint', 'crop', 'adj_128_32'),
    ('un-shift off by one', 'unshift', 'split_128_64'),
    ('un-shift off by one, adjoint', 'unshift', 'adj_impulse_64_64'),
    ('one wrong twiddle index at k = S/2', 'twiddle', 'fwd_128_impulse'),
    ('one wrong twiddle index at k = S/2 (shipped)', 'twiddle', 'fwd_64s_impulse'),
    ('band B-1 dropped, split', 'band_drop', 'split_b8_64_4'),
    ('band B-1 dropped, spectral', 'band_drop', 'spec_p68_b8'),
    ('flat channel order k*O + o, split', 'chan_order', 'split_b2_16_16'),
    ('flat channel order k*O + o, spectral', 'chan_order', 'spec_p2112_b2'),
    ('positions of a partial last tile dropped', 'tail', 'spec_p68_b7'),
    ('positions of a partial last tile dropped (one tile)', 'tail', 'spec_p4_b3'),
    ('column S/2 of the forward transform dropped', 'nyq_col', 'fwd_64n_random'),
    ('a skipped level still counted', 'skip', 'split_skip_alternate_128_4'),
    ('accumulate overwriting', 'acc_overwrite', 'split_acc_16_4'),
    ('Re/Im plane offset wrong, forward (C = 3)', 'imoff', 'fwd_32_random'),
    ('Re/Im plane offset wrong, split (C = 12)', 'imoff', 'split_c12_128_16'),
    ('Re/Im plane offset wrong, adjoint (C = 3)', 'imoff', 'adj_64_4_n'),
]


@pytest.mark.parametrize('label,defect,cid', DEFECTS, ids=[f'{d[1]}-{d[2]}' for d in DEFECTS])
def test_each_defect_is_caught_by_a_named_case(label, defect, cid):
    case = CASES[cid][0]
    inp = inputs(case)
    good, bad = reference(case, inp), reference(case, inp, defect)
    worst = 0.0
    for g, b in zip(good, bad):
        if g is None:
            continue
        live = g[2] > 0                 # (an element pinned to an exact zero would make any change count as infinitely many bars)
        ratio, idx = sf.worst_ratio(b[1][live], g[1][live], g[2][live])
        worst = max(worst, ratio)
    print(f'{label}: case {cid} sees it at {worst:.3e} bars')
    assert worst >= 100.0, f'{label}: case {cid} sees the defect at only {worst:.3e} bars'


def test_every_defect_of_the_restatement_has_a_case():
    doc = sf.__doc__
    listed = set(re.findall(r'^  (\w+)  ', doc, re.M))
    assert listed == {d[1] for d in DEFECTS}, (sorted(listed), sorted({d[1] for d in DEFECTS}))


# ------------------------------------------------------------------------------------------------
# coverage of shu.hip
# ------------------------------------------------------------------------------------------------

def launch_pairs():
    """Every (kernel, instantiation) a hipLaunchKernelGGL site of shu.hip can launch, from the source."""
    with open(SRC) as fh:
        src = fh.read()
    macro = re.search(r'#define SHU_DISPATCH_SIZE\(size, LAUNCH\)\s*\\\n(.*)\n', src).group(1)
    sizes = [int(v) for v in re.findall(r'LAUNCH\((\d+)\)', macro)]
    pairs = set()
    for name, tmpl in re.findall(r'hipLaunchKernelGGL\(\s*(\w+)(<S>)?', src):
        pairs |= {f'{name}<{s}>' for s in sizes} if tmpl else {name}
    return pairs, sizes


def unclaimed(cases):
    pairs, _ = launch_pairs()
    claimed = {p.replace(' ', '') for _, exp, _ in cases.values() for p in exp}
    return sorted(pairs - claimed), sorted(claimed - pairs)


def test_the_table_claims_every_launch_site():
    pairs, sizes = launch_pairs()
    assert sizes == [16, 32, 64, 128]
    assert len(pairs) == 17, sorted(pairs)                 # three shipped kernels, two spectral kernels, 4 sizes x 3 size-general kernels
    with open(SRC) as fh:
        assert {k for k in re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', fh.read())} == {p.split('<')[0] for p in pairs}
    missing, naming_nothing = unclaimed(CASES)
    assert not missing, f'launch sites without a case: {missing}'
    assert not naming_nothing, f'claims that name no kernel of shu.hip: {naming_nothing}'
    assert all(exp for _, exp, _ in CASES.values())
    # the check bites: without the cases that claim it, a pair is reported; a claim of something else is reported too
    for pair in sorted(pairs):
        rest = {cid: v for cid, v in CASES.items() if pair not in v[1]}
        assert len(rest) < len(CASES) and unclaimed(rest)[0] == [pair], pair
    assert unclaimed(dict(CASES, bogus=(None, ('shu_split_irfft2_n_kernel<256>',), ())))[1] == ['shu_split_irfft2_n_kernel<256>']
    # the wrapper never picks the <64> forms at the shipped geometry: their cases go through the C ABI
    assert CASES['fwd_64n_random'][0]['form'] == 'cabi' and CASES['split_64_4_n'][0]['form'] == 'n' and CASES['adj_64_4_n'][0]['form'] == 'n'


# ------------------------------------------------------------------------------------------------
# the legal pyramids
# ------------------------------------------------------------------------------------------------

def test_the_18_pyramids_are_what_the_wrappers_and_the_c_abi_accept():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib, kernels
    assert len(PYRAMIDS) == 18
    ok = []
    for size in (8, 16, 32, 48, 64, 128, 256):
        for count in range(0, 9):
            try:
                res, arr = kernels._shu_levels(size, count, 'test')
            except _lib.ShgError:
                continue
            assert res == levels_of(size, res[0]) and (arr is None) == ((size, count) == (64, 5))
            ok.append((size, res[0]))
    assert sorted(ok) == sorted(PYRAMIDS)
    # shu_levels_ok, from the outside: with N = 0 a legal level list gets as far as the shape check, an illegal one stops before it
    lib = _lib.get_lib()
    P = ctypes.c_void_p(16)
    accepted = []
    for size in (16, 32, 64, 128):
        for low in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            res = [r for r in (1, 2, 4, 8, 16, 32, 64, 128, 256) if low <= r <= size] or [low]
            nl = len(res)
            arr, pp, ll = (ctypes.c_int * nl)(*res), (ctypes.c_void_p * nl)(*([16] * nl)), (ctypes.c_long * nl)()
            assert lib.shg_shu_split_irfft2_n_f32(P, None, pp, pp, ll, 0, 1, 1, 0, size, arr, nl, None) == -1
            split_ok = b'bad shape' in lib.shg_last_error()
            assert split_ok or b'consecutive powers of two' in lib.shg_last_error()
            assert lib.shg_shu_split_adjoint_n_f32(pp, ll, pp, P, 0, 1, size, arr, nl, None) == -1
            assert split_ok == (b'bad shape' in lib.shg_last_error())
            if split_ok:
                accepted.append((size, low))
    assert accepted == PYRAMIDS
    for res in ((8, 32), (16, 16), (32, 16), (4, 8, 16, 32, 64, 128, 128)):          # not consecutive, repeated, descending, seven levels
        arr, nl = (ctypes.c_int * len(res))(*res), len(res)
        pp, ll = (ctypes.c_void_p * nl)(*([16] * nl)), (ctypes.c_long * nl)()
        assert lib.shg_shu_split_irfft2_n_f32(P, None, pp, pp, ll, 0, 1, 1, 0, res[-1], arr, nl, None) == -1
        assert b'consecutive powers of two' in lib.shg_last_error(), res


def test_the_gaussian_staging_area_holds_every_pyramid():
    with open(SRC) as fh:
        src = fh.read()
    body = src[src.index('void shu_split_irfft2_n_kernel('):]
    decl = re.search(r'__shared__ float gl\[([0-9 +]+)\];', body).group(1)
    assert decl.replace(' ', '') == '12+40+144+544'
    room = sum(int(v) for v in decl.split('+'))
    need = {(s, low): sum(r * (r // 2 + 1) for r in levels_of(s, low) if r < 64) for s, low in PYRAMIDS}
    assert all(v <= room for v in need.values()), need
    assert need[(64, 4)] == need[(128, 4)] == room and need[(128, 64)] == 0
