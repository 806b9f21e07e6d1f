"""CPU (no GPU): the host side of U-IDS / P-IDS (sh-gan_amd/ids_score.py) -- the float64 yardstick (tests/ids_f64.py) against sklearn's
LinearSVC, the product's truncated Newton fit with a numpy stand-in for the pass kernel, the refusal to score a fit that did not converge,
the new symbols of the C ABI and their argument checks, and EvalLoop's ``pids_uids`` option at world size 1 and under gloo at world size 2."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, ids_score

import ids_f64 as ref

NEW = ('shg_svm_pass_workspace_bytes', 'shg_svm_pass_f64')
_FITS = {}


def yardstick(case):
    """(real, fake, v = (w, b), info) of a case, fitted once per session."""
    if case not in _FITS:
        real, fake = ref.features(*ref.CASES[case])
        _FITS[case] = (real, fake) + ref.fit(real, fake)
    return _FITS[case]


@pytest.mark.parametrize('case', list(ref.CASES))
def test_yardstick_converges_and_gives_the_tabulated_scores(case):
    real, fake, v, info = yardstick(case)
    assert info['converged'] and info['grad_norm'] <= 1e-11 * info['grad_norm0']
    assert 1 <= info['newton'] <= 25 and info['products'] <= 400, info
    uids, pids, _, _ = ref.ids(v, real, fake)
    assert (round(uids, 4), round(pids, 4)) == ref.SCORES[case]


@pytest.mark.parametrize('case', ['A', 'B', 'C', 'D'])
def test_yardstick_against_sklearn(case):
    """The objective is LinearSVC(dual=False)'s: with tol=1e-12 liblinear stops within 4e-7 of the float64 optimum; 1e-5 |w*| checks the
    objective, not a solver.  The scores are 1 - score and mean(decision_function(fake) > decision_function(real))."""
    svm = pytest.importorskip('sklearn.svm')
    real, fake, v, _ = yardstick(case)
    X, y = np.concatenate([real, fake]), np.concatenate([np.ones(len(real)), -np.ones(len(fake))])
    clf = svm.LinearSVC(dual=False, tol=1e-12, max_iter=100000).fit(X, y)
    theirs = np.concatenate([clf.coef_.ravel(), clf.intercept_])
    dist = float(np.linalg.norm(theirs - v))
    print(f'case {case}: |(w, b) - sklearn| = {dist:.3e}, |w*| = {np.linalg.norm(v):.4f}')
    assert dist <= 1e-5 * np.linalg.norm(v)
    uids, pids, errors, wins = ref.ids(v, real, fake)
    # (as integer counts: 1.0 - score rounds differently from errors / 2N in the last bit)
    assert errors == len(X) - int(round(clf.score(X, y) * len(X))) and abs(uids - (1.0 - clf.score(X, y))) < 1e-15
    assert wins == int(np.sum(clf.decision_function(fake) > clf.decision_function(real)))
    assert pids == float(np.mean(clf.decision_function(fake) > clf.decision_function(real)))


@pytest.mark.parametrize('case', ['A', 'B', 'E'])
def test_fit_with_a_numpy_pass_meets_the_stopping_rule_and_the_yardsticks_scores(case):
    real, fake, v, _ = yardstick(case)
    tol = 1e-9
    res = ids_score.ids_from_features(torch.from_numpy(real), torch.from_numpy(fake), tol=tol, pass_fn=ref.torch_pass_fn)
    assert res['converged'] and res['grad_norm'] <= tol * res['grad_norm0'] and res['w'].dtype == torch.float64 and res['w'].shape == (real.shape[1],)
    got = np.concatenate([res['w'].numpy(), [res['b']]])
    Xt, y = ref.stack(real, fake)
    g = float(np.linalg.norm(ref.gradient(got, Xt, y)))
    g0 = float(np.linalg.norm(ref.gradient(np.zeros_like(got), Xt, y)))
    assert abs(res['grad_norm0'] - g0) <= 1e-12 * g0 and g <= tol * g0 * (1 + 1e-6)
    assert np.linalg.norm(got - v) <= g + 1e-11 * g0                     # 1-strong convexity: |v - v*| <= |grad f(v)|
    assert (res['uids_errors'], res['pids_wins'], res['n']) == ref.ids(v, real, fake)[2:] + (len(real),)
    assert (res['uids'], res['pids']) == ref.ids(v, real, fake)[:2]
    assert res['passes'] >= res['newton_iters'] + 2


def test_a_fit_that_did_not_converge_is_an_error_not_a_score():
    real, fake = ref.features(*ref.CASES['C'])
    real, fake = torch.from_numpy(real), torch.from_numpy(fake)
    fit = ids_score.fit_linear_svc(real, fake, max_newton=1, pass_fn=ref.torch_pass_fn)
    assert not fit['converged'] and fit['newton_iters'] == 1 and fit['grad_norm'] > 1e-9 * fit['grad_norm0']
    with pytest.raises(_lib.ShgError, match=r'did not converge.*gradient norm \d\.\d+e[-+]\d+.*\d\.\d+e[-+]\d+') as e:
        ids_score.ids_from_features(real, fake, max_newton=1, pass_fn=ref.torch_pass_fn)
    assert f"{fit['grad_norm']:.6e}" in str(e.value) and f"{fit['grad_norm0']:.6e}" in str(e.value)


def test_operands_are_checked_before_a_launch():
    f = torch.zeros(8, 16)
    for real, fake in ((f, f.double()), (f, f[:4]), (f, f[:, :8]), (f.t()[:8, :8], f[:, :8]), (f.numpy(), f), (torch.zeros(8, 5000), torch.zeros(8, 5000))):
        with pytest.raises(_lib.ShgError):
            ids_score.ids_from_features(real, fake, pass_fn=ref.torch_pass_fn)
    with pytest.raises(_lib.ShgError, match='no CPU path'):
        ids_score.ids_from_features(f, f)
    with pytest.raises(_lib.ShgError, match='no CPU path'):
        ids_score.fit_linear_svc(f, f)
    with pytest.raises(_lib.ShgError):                       # the wrapper itself: host tensors, an unknown mode
        ids_score.svm_pass(f, f, torch.zeros(17, dtype=torch.float64), 'grad')
    with pytest.raises(_lib.ShgError, match='mode'):
        ids_score.svm_pass(f, f, torch.zeros(17, dtype=torch.float64), 'hess')
    with pytest.raises(_lib.ShgError):
        ids_score.fit_linear_svc(f, f, C=0.0, pass_fn=ref.torch_pass_fn)


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    assert lib.shg_svm_pass_workspace_bytes.restype == ctypes.c_size_t
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    # one partial of D + 2 doubles per workgroup; four rows per workgroup until the persistent grid is full (512 up to D = 2048, 256 above)
    wsb = lib.shg_svm_pass_workspace_bytes
    assert wsb(50000, 50000, 2048) == 512 * 2050 * 8 and wsb(36500, 36500, 4096) == 256 * 4098 * 8 and wsb(1000, 1000, 2049) == 256 * 2051 * 8
    assert wsb(1, 0, 1) == 3 * 8 and wsb(3, 2, 24) == 2 * 26 * 8 and wsb(1023, 1024, 7) == 512 * 9 * 8
    assert wsb(0, 5, 8) == 0 and wsb(5, -1, 8) == 0 and wsb(5, 5, 0) == 0 and wsb(5, 5, 4097) == 0 and wsb(1 << 30, 1 << 30, 8) == 0
    p, big = ctypes.c_void_p(4096), 1 << 30

    def run(x0=p, n0=8, ld0=64, x1=p, n1=8, ld1=64, D=64, mode=0, v=p, z=p, a=p, q=p, ws=p, nbytes=big):
        return lib.shg_svm_pass_f64(x0, n0, ld0, 1.0, x1, n1, ld1, -1.0, D, mode, 1.0, v, z, a, q, ws, nbytes, None)
    assert run(mode=2) == -1 and 'mode' in err() and run(mode=-1) == -1
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.shg_svm_pass_f64(p, 8, 64, 1.0, p, 8, 64, -1.0, 64, 0, bad, p, p, p, p, p, big, None) == -1 and 'C must be' in err()
    assert lib.shg_svm_pass_f64(p, 8, 64, float('nan'), p, 8, 64, -1.0, 64, 0, 1.0, p, p, p, p, p, big, None) == -1 and 'labels' in err()
    assert lib.shg_svm_pass_f64(p, 8, 64, 1.0, p, 8, 64, float('inf'), 64, 0, 1.0, p, p, p, p, p, big, None) == -1 and 'labels' in err()
    for kw in (dict(x0=None), dict(v=None), dict(a=None), dict(q=None), dict(z=None)):
        assert run(**kw) == -1 and 'null' in err(), kw
    assert run(D=0) == -1 and run(D=4097, ld0=4097, ld1=4097) == -1 and '1..4096' in err()
    assert run(n0=0) == -1 and run(n1=-1) == -1 and run(n0=big, n1=big) == -1 and 'rows' in err()
    assert run(x1=None) == -1 and run(n1=0) == -1 and 'second row set' in err()
    assert run(ld0=63) == -1 and run(ld1=8) == -1 and 'pitch' in err()
    assert run(x0=ctypes.c_void_p(4098)) == -1 and run(x1=ctypes.c_void_p(4097)) == -1 and '4-byte' in err()
    for kw in (dict(v=ctypes.c_void_p(4100)), dict(z=ctypes.c_void_p(4100)), dict(q=ctypes.c_void_p(4100)), dict(ws=ctypes.c_void_p(4100))):
        assert run(**kw) == -1 and '8-byte' in err(), kw
    assert run(ws=None) == -1 and 'workspace' in err()
    assert run(nbytes=4 * 66 * 8 - 1) == -1 and 'too small' in err()


R, N_ITEMS, B, D = 16, 23, 4, 12


def _loop_parts():
    """Stand-ins shared by the world-1 test below (the world-2 script restates them: it runs in processes of its own)."""
    from shgan_amd import eval_harness as hz

    def step(x, z, out):
        out.copy_(((x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.2).tanh() * 127.5 + 127.5).clamp(0, 255).to(torch.uint8))
        return out

    def acc(S, feats, w):
        f = torch.cat([feats.double(), torch.ones(feats.shape[0], 1, dtype=torch.float64)], 1)
        S[:D + 1, :D + 1] += (f * (torch.ones(len(f), dtype=torch.float64) if w is None else w.double())[:, None]).t() @ f

    def det(img, input_range='0_255'):
        v = img.float() * 127.5 + 127.5 if input_range == 'pm1' else img.float()
        return hz.standin_features(v, D) / 64

    def latents(ids, b):
        g, out = torch.Generator(), torch.empty(b, 8)
        for k, i in enumerate(ids):
            g.manual_seed(100 + int(i))
            out[k].normal_(generator=g)
        return out

    class Loader:
        def __init__(self, ids):
            self.ids = ids

        def __iter__(self):
            for b0 in range(0, len(self.ids), B):
                ids, g, imgs = self.ids[b0:b0 + B], torch.Generator(), []
                for i in ids:
                    g.manual_seed(7000 + int(i))
                    imgs.append(torch.rand(3, R, R, generator=g) * 2 - 1)
                yield torch.stack(imgs), torch.ones(len(ids), R, R) * (torch.arange(R) % 3 > 0).float(), ids
    return hz, step, acc, det, latents, Loader


def test_eval_loop_option_at_world_1_and_its_checks():
    hz, step, acc, det, latents, Loader = _loop_parts()
    common = dict(noise_mode='const', fid_dim=D, latent_fn=latents, device_masks=False, step_fn=step, fid_accumulate_fn=acc)
    with pytest.raises(ValueError, match='fid_real'):
        hz.EvalLoop(None, 'cpu', R, N_ITEMS, feature_fn=det, pids_uids=True, **common)
    with pytest.raises(ValueError, match='feature_fn'):
        hz.EvalLoop(None, 'cpu', R, N_ITEMS, pids_uids=True, **common)
    with pytest.raises(ValueError, match=r"unknown pids_uids option\(s\) \['newton'\]"):
        hz.EvalLoop(None, 'cpu', R, N_ITEMS, feature_fn=det, fid_real=True, pids_uids=dict(newton=3), **common)

    def run(**kw):
        loop = hz.EvalLoop(None, 'cpu', R, N_ITEMS, feature_fn=det, fid_real=True, **common, **kw)
        loop.run(Loader(loop.ids))
        return loop, loop.gather()
    opts = dict(tol=1e-8, pass_fn=ref.torch_pass_fn)
    loop, (images, fid) = run(pids_uids=opts)
    with_kid, _ = run(pids_uids=opts, kid=dict(num_subsets=2, max_subset_size=5, sums_fn=__import__('kid_is_f64').kid_sums_f64))
    plain, (images0, fid0) = run()
    # off: no options, no buffer, no rows, and the accessor raises like its neighbours
    d0 = plain.evaluators['detector']
    assert d0.ids_opts is None and d0.kid_opts is None and d0.kid_local is None and plain.kid_features is None and d0.ids_value() is None
    assert set(vars(d0)) == set(vars(loop.evaluators['detector']))
    for fn in (plain.ids_value, plain.kid_value, loop.kid_value):          # kid_value stays None (raises) without kid
        with pytest.raises(ValueError, match='finished gather'):
            fn()
    assert torch.equal(images0, images) and torch.equal(fid0.S, fid.S)
    # on: the rows in dataset order, one pair of buffers with or without kid
    fake, real = loop.kid_features
    reals = torch.cat([x for x, _, _ in Loader(list(range(N_ITEMS)))])
    assert torch.equal(fake, det(images)) and torch.equal(real, det(reals, input_range='pm1'))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(with_kid.kid_features, loop.kid_features)) and isinstance(with_kid.kid_value(), float)
    want = ids_score.ids_from_features(real.contiguous(), fake.contiguous(), **opts)
    assert loop.ids_value() == (want['uids'], want['pids']) == with_kid.ids_value()
    v, info = ref.fit(real.numpy(), fake.numpy())
    assert info['converged'] and (want['uids_errors'], want['pids_wins']) == ref.ids(v, real.numpy(), fake.numpy())[2:]
    fresh = hz.EvalLoop(None, 'cpu', R, N_ITEMS, feature_fn=det, fid_real=True, pids_uids=True, **common)
    assert len(fresh.evaluators['detector'].kid_local) == 2 and fresh.evaluators['detector'].kid_opts is None
    with pytest.raises(ValueError):                          # before gather
        fresh.ids_value()


def test_gloo_world2_eval_loop_pids_uids():
    """World 2 over 23 items (rank 1 holds a padded duplicate): ids_value() on both ranks equals ids_from_features on the features of a
    hand-made single pass in dataset order, and the 1-rank loop's."""
    script = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd
from shgan_amd import ids_score
import ids_f64 as ref
import test_ids_cpu as T
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
hz, step, acc, det, latents, Loader = T._loop_parts()
OPTS = dict(tol=1e-8, pass_fn=ref.torch_pass_fn)
def run(rank, world, **kw):
    loop = hz.EvalLoop(None, "cpu", T.R, T.N_ITEMS, rank=rank, world=world, noise_mode="const", feature_fn=det, fid_dim=T.D, latent_fn=latents,
                       device_masks=False, step_fn=step, fid_accumulate_fn=acc, fid_real=True, pids_uids=OPTS, **kw)
    loop.run(Loader(loop.ids))
    return loop
loop = run(r, 2)
assert len(loop.ids) == 12
images, fid = loop.gather()
fake, real = loop.kid_features
assert fake.shape == real.shape == (T.N_ITEMS, T.D) and fake.dtype == torch.float32
reals = torch.cat([x for x, _, _ in Loader(list(range(T.N_ITEMS)))])
assert torch.equal(fake, det(images)) and torch.equal(real, det(reals, input_range="pm1"))
want = ids_score.ids_from_features(real.contiguous(), fake.contiguous(), **OPTS)
got = loop.ids_value()
assert got == (want["uids"], want["pids"]), (got, want)
try:
    loop.kid_value()
    raise SystemExit("kid_value() must raise without kid")
except ValueError:
    pass
dist.destroy_process_group()
one = run(0, 1)
one.gather()
assert one.ids_value() == got
print("rank", r, "ok", got)
'''
    port = str(39500 + os.getpid() % 2000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), SHG_ROOT=ROOT, SHG_PORT=port)
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out.decode()
