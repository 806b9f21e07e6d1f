"""CPU (no GPU): the device tail of FID (sh-gan_amd/fid_stats.py ``gemm_f64`` / ``mean_cov_device`` / ``frechet_device``) -- the numpy
restatement of tests/fid_f64.py against its eigh yardstick and scipy's ``sqrtm`` inside the bounds the GPU tests use, the product's
iteration with a numpy stand-in for the kernel against that restatement, ``mean_cov_device`` against ``mean_cov``, the new symbols of
the C ABI and their argument checks, and EvalLoop's ``fid_tail`` option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, fid_stats

import fid_f64 as ref

NEW = ('shg_gemm_f64', 'shg_gemm_f64_tiles')
_STATS = {}


def case(c):
    """(stats, frechet_ns, (fid, trace) of frechet_eigh, tr sigma_f + tr sigma_r) of a case, computed once per session."""
    if c not in _STATS:
        st = ref.case_stats(*c)
        _STATS[c] = (st, ref.frechet_ns(*st), ref.frechet_eigh(*st), float(np.trace(st[1]) + np.trace(st[3])))
    return _STATS[c]


@pytest.mark.parametrize('c', ref.CASES)
def test_restatement_stays_inside_the_bounds_of_the_gpu_tests(c):
    """The bounds are conditions on the inputs: numpy's own Newton-Schulz trace must meet them, and scipy's sqrtm -- the reference's path --
    agrees where sigma has full rank."""
    D, N = c[:2]
    st, ns, (fid, tr), scale = case(c)
    err = abs(ns['fid'] - fid) / scale
    print(f"case {c}: FID {fid:.6f}, |ns - eigh| / (tr + tr) = {err:.3e} after {ns['iterations']} steps ({ns['stop']}, delta {ns['delta']:.3e})")
    assert err <= ref.bound_of(D, N)
    assert ns['stop'] in ('tol', 'turn') and 5 <= ns['iterations'] <= 60 and abs(ns['trace_sqrt'] - tr) <= ref.bound_of(D, N) * scale
    if N >= 4 * D:
        pytest.importorskip('scipy.linalg')
        host = fid_stats.fid_from_stats(*st)
        print(f'          |sqrtm - eigh| / (tr + tr) = {abs(host - fid) / scale:.3e}')
        assert abs(host - fid) <= ref.BOUND_FULL * scale and abs(ns['fid'] - host) <= ref.BOUND_FULL * scale


def test_identical_sides_and_a_zero_product():
    mu, sigma = case(ref.CASES[3])[0][:2]
    res = ref.frechet_ns(mu, sigma, mu, sigma)
    assert abs(res['fid']) <= 1e-7 * 2 * np.trace(sigma)
    zero = np.zeros_like(sigma)
    assert ref.frechet_ns(mu, zero, mu + 1.0, sigma) == dict(fid=len(mu) + float(np.trace(sigma)), trace_sqrt=0.0, iterations=0, delta=0.0, stop='tol')
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))        # noqa: E731
    got = fid_stats.frechet_device(t(mu), t(zero), t(mu + 1.0), t(sigma), matmul_fn=ref.numpy_matmul_fn)
    assert got['iterations'] == 0 and got['trace_sqrt'] == 0.0 and abs(got['fid'] - len(mu) - np.trace(sigma)) <= 1e-12 * np.trace(sigma)


@pytest.mark.parametrize('c', ref.CASES)
def test_frechet_device_with_a_numpy_matmul_follows_the_restatement(c):
    st, ns, _, scale = case(c)
    calls = []

    def matmul(a, b, **kw):
        calls.append((a.ndim, tuple(kw['out'].shape), kw['out'].data_ptr()))
        return ref.numpy_matmul_fn(a, b, **kw)
    got = fid_stats.frechet_device(*(torch.from_numpy(np.ascontiguousarray(x)) for x in st), matmul_fn=matmul)
    assert set(got) == {'fid', 'trace_sqrt', 'iterations', 'delta', 'stop'}
    assert abs(got['fid'] - ns['fid']) <= 1e-12 * scale and abs(got['trace_sqrt'] - ns['trace_sqrt']) <= 1e-12 * scale
    assert got['stop'] == ns['stop'] and abs(got['iterations'] - ns['iterations']) <= 1
    # the first product, then per step T and the batch of two: every output lies in the one allocation made before the loop
    assert len(calls) == 1 + 2 * got['iterations'] and [c_[0] for c_ in calls[1:]] == [2, 3] * got['iterations']
    n = len(st[0])
    assert len({p for _, _, p in calls}) <= 5 and max(p for _, _, p in calls) - min(p for _, _, p in calls) <= 4 * n * n * 8


def test_frechet_device_checks_its_arguments_and_raises_past_max_iter():
    st = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in case(ref.CASES[0])[0])
    with pytest.raises(_lib.ShgError, match='no stop within 3'):
        fid_stats.frechet_device(*st, max_iter=3, matmul_fn=ref.numpy_matmul_fn)
    with pytest.raises(_lib.ShgError, match='no CPU path'):
        fid_stats.frechet_device(*st)
    with pytest.raises(_lib.ShgError, match='no CPU path'):
        fid_stats.gemm_f64(st[1], st[3])
    for bad in ((st[0], st[1].float(), st[2], st[3]), (st[0][:-1], st[1], st[2], st[3]), (st[0], st[1], st[2], st[3][:-1]), (st[0], st[1][0], st[2], st[3]),
                (st[0].numpy(), st[1], st[2], st[3])):
        with pytest.raises(_lib.ShgError):
            fid_stats.frechet_device(*bad, matmul_fn=ref.numpy_matmul_fn)
    for kw in (dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(_lib.ShgError):
            fid_stats.frechet_device(*st, matmul_fn=ref.numpy_matmul_fn, **kw)
    assert [fid_stats.gemm_f64_tiles(n) for n in (1, 128, 129, 2048)] == [1, 1, 4, 256]


def _accumulate(S, feats, w):
    d = feats.shape[1]
    f = torch.cat([feats.double(), torch.ones(feats.shape[0], 1, dtype=torch.float64)], 1)
    S[:d + 1, :d + 1] += (f * (torch.ones(len(f), dtype=torch.float64) if w is None else w.double())[:, None]).t() @ f


def test_mean_cov_device_is_mean_cov():
    """The same arithmetic on the same moments: the same bits, the ``sample_n`` divisor and the empty-accumulator error included; what lies
    below the diagonal (the kernel never writes there) is not read."""
    d = 37
    st = fid_stats.FidStats(d, device='cpu', accumulate_fn=_accumulate)
    for fn in (st.mean_cov, st.mean_cov_device):
        with pytest.raises(ValueError, match='no samples'):
            fn()
    g = torch.Generator().manual_seed(3)
    st.add(torch.randn(50, d, generator=g) + 0.5, (torch.arange(50) % 7 > 0).float())
    st.S.copy_(torch.triu(st.S) + torch.tril(torch.full_like(st.S, 1e30), -1))
    for sample_n in (None, 48):
        n, mu, sigma = st.mean_cov(sample_n)
        n_d, mu_d, sigma_d = st.mean_cov_device(sample_n)
        assert n == n_d == 42.0 and mu_d.dtype == sigma_d.dtype == torch.float64 and sigma_d.shape == (d, d)
        assert np.array_equal(mu_d.numpy(), mu) and np.array_equal(sigma_d.numpy(), sigma)
        assert np.array_equal(sigma, sigma.T)
    assert not np.array_equal(st.mean_cov()[2], st.mean_cov(48)[2])


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    tiles = lib.shg_gemm_f64_tiles
    assert [tiles(n) for n in (1, 127, 128, 129, 256, 257, 2048, 46336)] == [1, 1, 1, 4, 4, 9, 256, 362 * 362]
    assert tiles(0) == 0 and tiles(-3) == 0 and tiles(46337) == 0
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    p = ctypes.c_void_p(4096)

    def run(A=p, B=p, C=p, n=64, lda=64, ldb=64, ldc=64, batch=1, sa=0, sb=0, sc=0, partials=p):      # (every call fails a check: nothing is launched)
        return lib.shg_gemm_f64(A, B, C, n, lda, ldb, ldc, 1.0, 0.0, batch, sa, sb, sc, partials, None)
    for kw in (dict(A=None), dict(B=None), dict(C=None)):
        assert run(**kw) == -1 and 'null' in err(), kw
    assert run(n=0) == -1 and run(n=46337, lda=50000, ldb=50000, ldc=50000) == -1 and '1..46336' in err()
    for kw in (dict(lda=63), dict(ldb=63), dict(ldc=63)):
        assert run(**kw) == -1 and 'leading dimension' in err(), kw
    assert run(batch=0) == -1 and run(batch=65536, sc=4096) == -1 and 'batch' in err()
    assert run(batch=2, sa=4096, sb=4096, sc=0) == -1 and 'share' in err()
    for kw in (dict(A=ctypes.c_void_p(4100)), dict(B=ctypes.c_void_p(4100)), dict(C=ctypes.c_void_p(4100)), dict(partials=ctypes.c_void_p(4100))):
        assert run(**kw) == -1 and '8-byte' in err(), kw


def test_fid_tail_option_is_checked_in_the_constructor():
    from shgan_amd import eval_harness as hz
    from shgan_amd.evaluators import check_fid_tail
    assert check_fid_tail('host') == ('host', {}) and check_fid_tail('device') == ('device', {})
    assert check_fid_tail(dict(tol=1e-9)) == ('device', dict(tol=1e-9))
    for bad in ('gpu', None, True, 1):
        with pytest.raises(ValueError, match='fid_tail must be'):
            hz.EvalLoop(None, 'cpu', 16, 8, fid_tail=bad, device_masks=False)
    with pytest.raises(ValueError, match=r"unknown fid_tail option\(s\) \['steps'\]"):
        hz.EvalLoop(None, 'cpu', 16, 8, fid_tail=dict(steps=3), device_masks=False)


def test_eval_loop_fid_tail_on_the_cpu_loop():
    """23 items of 12 stand-in features through the CPU loop of tests/test_ids_cpu.py: 'device' (with the numpy stand-in for the kernel) is
    ``frechet_device`` on both ``mean_cov_device`` and keeps its dict; the default leaves images, moments and the FID value as they were
    and calls ``fid_from_stats``."""
    pytest.importorskip('scipy.linalg')
    from test_ids_cpu import N_ITEMS, R, _loop_parts
    hz, step, acc, det, latents, Loader = _loop_parts()

    def run(**kw):
        loop = hz.EvalLoop(None, 'cpu', R, N_ITEMS, noise_mode='const', fid_dim=12, latent_fn=latents, device_masks=False, step_fn=step,
                           fid_accumulate_fn=acc, feature_fn=det, fid_real=True, **kw)
        loop.run(Loader(loop.ids))
        return loop, loop.gather()
    dev, (images, fid) = run(fid_tail=dict(matmul_fn=ref.numpy_matmul_fn))
    host, (images0, fid0) = run()
    assert torch.equal(images, images0) and torch.equal(fid.S, fid0.S) and torch.equal(dev.fid_real.S, host.fid_real.S)
    d_dev, d_host = dev.evaluators['detector'], host.evaluators['detector']
    assert set(vars(d_dev)) == set(vars(d_host)) and (d_host.fid_tail, d_dev.fid_tail) == ('host', 'device')
    assert dev.fid_tail_info is None and host.fid_tail_info is None                    # before the first fid_value()
    st = fid.mean_cov()[1:] + dev.fid_real.mean_cov()[1:]
    want_host = fid_stats.fid_from_stats(*st)
    assert host.fid_value() == want_host and host.fid_tail_info is None               # the parent's path, bit for bit
    got = dev.fid_value()
    info = dev.fid_tail_info
    assert got == info['fid'] and info['stop'] in ('tol', 'turn') and info['iterations'] >= 1
    ns = ref.frechet_ns(*st)
    scale = float(np.trace(st[1]) + np.trace(st[3]))
    print(f"CPU loop: host {want_host!r}, device tail {got!r} ({info['iterations']} steps, {info['stop']}), eigh {ref.frechet_eigh(*st)[0]!r}")
    assert abs(got - ns['fid']) <= 1e-12 * scale and info['stop'] == ns['stop'] and abs(info['iterations'] - ns['iterations']) <= 1
    assert abs(got - ref.frechet_eigh(*st)[0]) <= ref.BOUND_DEFICIENT * scale and abs(got - want_host) <= ref.BOUND_DEFICIENT * scale
    plain = hz.EvalLoop(None, 'cpu', R, N_ITEMS, fid_tail='device', device_masks=False)      # no detector: nothing to hang the option on
    assert 'detector' not in plain.evaluators and plain.fid_tail_info is None
