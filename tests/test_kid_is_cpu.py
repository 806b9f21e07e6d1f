"""CPU (no GPU): the host side of KID and the Inception Score -- the subset draws (sh-gan_amd/kid.py), the accumulator algebra and the split
rule (sh-gan_amd/inception_score.py), the new symbols of the C ABI and their argument checks, the optional classifier head of the detector,
and EvalLoop's ``kid`` / ``inception_score`` options under gloo at world size 2 with stand-ins for the kernels."""
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
from shgan_amd import _lib, inception, inception_score, kid

import kid_is_f64 as ref

NEW = ('shg_kid_sums_f64', 'shg_kid_workspace_bytes', 'shg_is_accumulate_f64', 'shg_inception_head_f32')


@pytest.mark.parametrize('n_f,n_r,cap,S,seed', [(70, 90, 37, 3, 0), (64, 64, 1000, 2, 5), (130, 101, 100, 4, 11), (5, 7, 2, 1, 3)])
def test_kid_subsets_are_the_seeded_draws_in_fake_then_real_order(n_f, n_r, cap, S, seed):
    idx_f, idx_r, m = kid.kid_subsets(n_f, n_r, S, cap, seed)
    assert m == min(n_f, n_r, cap) and idx_f.shape == idx_r.shape == (S, m) and idx_f.dtype == idx_r.dtype == np.int32
    rs = np.random.RandomState(seed)
    for s in range(S):
        assert np.array_equal(idx_f[s], rs.choice(n_f, m, replace=False))
        assert np.array_equal(idx_r[s], rs.choice(n_r, m, replace=False))
        assert len(set(idx_f[s])) == m and len(set(idx_r[s])) == m
        assert idx_f[s].min() >= 0 and idx_f[s].max() < n_f and idx_r[s].max() < n_r


def test_kid_from_features_with_a_stand_in_equals_the_yardstick_and_host_tensors_raise():
    g = np.random.RandomState(2)
    fake, real = g.randn(40, 64), g.randn(33, 64) + 0.1
    got = kid.kid_from_features(fake, real, 5, 20, seed=9, sums_fn=ref.kid_sums_f64)
    idx_f, idx_r, m = kid.kid_subsets(40, 33, 5, 20, 9)
    assert m == 20 and got == ref.kid_f64(fake, real, idx_f, idx_r)
    with pytest.raises(_lib.ShgError):
        kid.kid_from_features(torch.zeros(8, 64), torch.zeros(8, 64), 2, 4)
    with pytest.raises(_lib.ShgError):
        kid.kid_sums(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(_lib.ShgError):
        inception_score.is_accumulate(torch.zeros(2, 6, dtype=torch.float64), torch.zeros(3, 4), torch.zeros(3, dtype=torch.int32))


@pytest.mark.parametrize('num_splits', [1, 3, 10])
def test_accumulator_identity_equals_the_direct_formula(num_splits):
    """exp(A / n - sum pbar log pbar) per split == exp(mean_i sum_c p (log p - log pbar)); N = 23 is divisible by none of 3, 10."""
    N, C = 23, 17
    g = np.random.RandomState(num_splits)
    z = g.randn(N, C) * 2
    probs = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    splits = [inception_score.split_of(i, N, num_splits) for i in range(N)]
    acc = ref.is_accumulator_f64(probs, splits, num_splits)
    assert acc[:, C + 1].sum() == N
    mean, std = inception_score.is_from_accumulator(acc)
    want = ref.is_f64(probs, num_splits)
    assert abs(mean - want[0]) <= 1e-12 * want[0] and abs(std - want[1]) <= 1e-12 * max(want[0], 1.0), (mean, std, want)
    t = inception_score.is_from_accumulator(torch.from_numpy(acc))
    assert t == (mean, std)


def test_split_of_equals_the_slice_rule():
    N, S = 23, 10
    want = np.full(N, -1)
    for i in range(S):
        want[i * N // S:(i + 1) * N // S] = i
    assert [inception_score.split_of(j, N, S) for j in range(N)] == want.tolist()
    assert inception_score.split_of(N, N, S) == -1 and inception_score.split_of(-1, N, S) == -1
    for N, S in ((7, 10), (50000, 10), (24, 3), (5, 1)):          # fewer images than splits: some splits stay empty
        want = np.full(N, -1)
        for i in range(S):
            want[i * N // S:(i + 1) * N // S] = i
        ids = range(N) if N < 100 else list(range(0, N, 997)) + [4999, 5000, 5001, N - 1]
        assert all(inception_score.split_of(j, N, S) == want[j] for j in ids)


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    assert lib.shg_kid_workspace_bytes.restype == ctypes.c_size_t
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    # tiles of 64: T = ceil(m / 64); xx and yy walk T (T + 1) / 2 tiles each, xy T^2; one float64 per tile and subset
    assert lib.shg_kid_workspace_bytes(100, 1000) == 100 * (2 * 136 + 256) * 8
    assert lib.shg_kid_workspace_bytes(3, 37) == 3 * 3 * 8 and lib.shg_kid_workspace_bytes(1, 65) == (2 * 3 + 4) * 8
    assert lib.shg_kid_workspace_bytes(1, 1) == 0 and lib.shg_kid_workspace_bytes(0, 8) == 0
    p = ctypes.c_void_p(4096)

    def sums(fake=p, real=p, n_f=8, n_r=8, D=64, S=1, m=4, ws=p, nbytes=1 << 20, out=p, idx=p):
        return lib.shg_kid_sums_f64(fake, real, 0, n_f, n_r, D, idx, idx, S, m, ws, nbytes, out, None)
    assert sums(fake=None) == -1 and 'null' in err()
    assert sums(m=1) == -1 and 'm >= 2' in err()
    assert sums(D=32) == -1 and sums(D=66) == -1 and 'multiple of 4' in err()
    assert sums(S=0) == -1 and sums(S=70000) == -1
    assert sums(fake=ctypes.c_void_p(4100)) == -1 and 'aligned' in err()
    assert sums(ws=None) == -1 and 'workspace' in err()
    assert sums(nbytes=16) == -1 and 'too small' in err()
    assert lib.shg_is_accumulate_f64(None, p, p, 2, 8, 1, None) == -1
    assert lib.shg_is_accumulate_f64(p, p, p, 0, 8, 1, None) == -1 and lib.shg_is_accumulate_f64(p, p, p, 2, 8, 0, None) == -1
    assert lib.shg_inception_head_f32(p, p, None, None, 1, 8, 64, None) == -1
    assert lib.shg_inception_head_f32(p, p, None, p, 1, 8, 66, None) == -1
    assert lib.shg_inception_head_f32(p, p, None, p, 1, 20000, 2048, None) == -1 and 'LDS' in err()


def _sd_meta(**extra):
    sd = {k: torch.zeros(s) for k, s in inception.expected_shapes().items()}
    sd.update(extra)
    return sd


def test_head_weights_are_optional_and_probabilities_without_them_name_the_key():
    assert 'fc.weight' not in inception.expected_shapes()
    shapes = inception.expected_shapes(head_classes=1008)
    assert shapes['fc.weight'] == (1008, 2048) and shapes['fc.bias'] == (1008,)
    assert list(shapes)[:-2] == list(inception.expected_shapes())
    sd = _sd_meta()
    inception.validate_state_dict(sd)
    with pytest.raises(_lib.ShgError, match=r"fc\.weight"):
        inception.validate_state_dict(sd, head=True)
    inception.validate_state_dict(_sd_meta(**{'fc.weight': torch.zeros(1000, 2048), 'fc.bias': torch.zeros(1000)}), head=True)
    with pytest.raises(_lib.ShgError, match=r"fc\.bias.*\(1008,\)"):
        inception.validate_state_dict(_sd_meta(**{'fc.weight': torch.zeros(1000, 2048), 'fc.bias': torch.zeros(1008)}), head=True)
    with pytest.raises(_lib.ShgError, match=r"fc\.weight.*\(1000, 1024\)"):
        inception.validate_state_dict(_sd_meta(**{'fc.weight': torch.zeros(1000, 1024), 'fc.bias': torch.zeros(1000)}), head=True)
    det = inception.InceptionFeatures({}, 'cpu')            # a detector built without head weights
    assert det.num_classes is None
    for kw in ({'return_features': False}, {'with_probs': True}):
        with pytest.raises(_lib.ShgError, match=r"fc\.weight"):
            det(torch.zeros(1, 3, 8, 8), **kw)
    with pytest.raises(_lib.ShgError, match=r"fc\.weight"):
        det.probs(torch.zeros(1, 2048))
    with pytest.raises(_lib.ShgError):                      # no CPU path for the head either
        inception.head_probs(torch.zeros(1, 2048), torch.zeros(10, 2048))


def test_eval_loop_options_are_checked():
    from shgan_amd import eval_harness as hz
    feat = lambda img, **kw: img.reshape(img.shape[0], -1)[:, :6].float()        # noqa: E731
    with pytest.raises(ValueError, match='fid_real'):
        hz.EvalLoop(None, 'cpu', 8, 7, feature_fn=feat, fid_dim=6, kid=True)
    with pytest.raises(ValueError, match='feature_fn'):
        hz.EvalLoop(None, 'cpu', 8, 7, kid=True, fid_real=False)
    with pytest.raises(ValueError, match='subsets'):
        hz.EvalLoop(None, 'cpu', 8, 7, feature_fn=feat, fid_dim=6, fid_real=True, kid=dict(subsets=3))
    with pytest.raises(ValueError, match='feature_fn'):
        hz.EvalLoop(None, 'cpu', 8, 7, inception_score=dict(num_splits=2))
    with pytest.raises(ValueError, match='class count'):
        hz.EvalLoop(None, 'cpu', 8, 7, feature_fn=feat, fid_dim=6, inception_score=dict(num_splits=2))
    plain = hz.EvalLoop(None, 'cpu', 8, 7, feature_fn=feat, fid_dim=6)
    det = plain.evaluators['detector']                # the moments alone: no KID rows, no Inception Score accumulators or split table
    assert list(plain.evaluators) == ['detector'] and det.kid_local is None and det.is_splits is None and det.is_parts.parts == {}
    assert plain.kid_features is None and plain.is_acc is None
    for fn in (plain.kid_value, plain.is_value):
        with pytest.raises(ValueError):
            fn()


def test_gloo_world2_eval_loop_kid_and_inception_score():
    """Stand-ins for the generator step, the detector and the three kernels; world 2 over 11 items (rank 1 holds a padded duplicate):
    kid_value() and is_value() equal the yardsticks on the dataset-ordered features / probabilities of a hand-made single pass, and a
    1-rank loop gives the same numbers."""
    script = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd
from shgan_amd import eval_harness as hz, kid
import kid_is_f64 as ref
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
R, N, B, D, C, SPLITS = 16, 11, 4, 64, 9, 3
KID = dict(num_subsets=4, max_subset_size=6, seed=3)
def step(x, z, out):
    out.copy_(((x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.2).tanh() * 127.5 + 127.5).clamp(0, 255).to(torch.uint8))
    return out
def acc(S, feats, w):
    f = torch.cat([feats.double(), torch.ones(feats.shape[0], 1, dtype=torch.float64)], 1)
    S[:D + 1, :D + 1] += (f * (torch.ones(len(f), dtype=torch.float64) if w is None else w.double())[:, None]).t() @ f
W = torch.randn(C, D, generator=torch.Generator().manual_seed(1)) * 0.05
class Det:
    num_classes = C
    def __call__(self, img, input_range="0_255", with_probs=False, no_output_bias=True):
        v = img.float() * 127.5 + 127.5 if input_range == "pm1" else img.float()
        f = hz.standin_features(v, D) / 64
        # (one matrix-vector product per image: the same bits whatever batch the image arrives in)
        return (f, torch.softmax(torch.stack([W @ fi for fi in f]), 1)) if with_probs else f
def is_acc(a, probs, splits):
    a += torch.from_numpy(ref.is_accumulator_f64(probs.numpy(), splits.numpy(), a.shape[0]))
def latents(ids, b):
    g = torch.Generator(); out = torch.empty(b, 8)
    for k, i in enumerate(ids):
        g.manual_seed(100 + int(i)); out[k].normal_(generator=g)
    return out
class Loader:
    def __init__(self, ids): self.ids = ids
    def __iter__(self):
        for b0 in range(0, len(self.ids), B):
            ids = self.ids[b0:b0 + B]
            g = torch.Generator()
            imgs = []
            for i in ids:
                g.manual_seed(7000 + int(i)); imgs.append(torch.rand(3, R, R, generator=g) * 2 - 1)
            yield torch.stack(imgs), torch.ones(len(ids), R, R) * (torch.arange(R) % 3 > 0).float(), ids
def run(rank, world):
    loop = hz.EvalLoop(None, "cpu", R, N, rank=rank, world=world, noise_mode="const", feature_fn=Det(), fid_dim=D, latent_fn=latents,
                       device_masks=False, step_fn=step, fid_accumulate_fn=acc, fid_real=True, kid=dict(KID, sums_fn=ref.kid_sums_f64),
                       inception_score=dict(num_splits=SPLITS, accumulate_fn=is_acc))
    loop.run(Loader(loop.ids))
    return loop
loop = run(r, 2)
images, fid = loop.gather()
fake, real = loop.kid_features
assert fake.shape == real.shape == (N, D) and fake.dtype == torch.float32
# the single pass in dataset order, by hand
det = Det()
reals = torch.cat([x for x, _, _ in Loader(list(range(N)))])
f_fake, p_fake = det(images, with_probs=True)
f_real = det(reals, input_range="pm1")
assert torch.equal(fake, f_fake) and torch.equal(real, f_real)
idx_f, idx_r, m = kid.kid_subsets(N, N, **KID)
want_kid = ref.kid_f64(f_fake.numpy(), f_real.numpy(), idx_f, idx_r)
got_kid = loop.kid_value()
assert got_kid == want_kid, (got_kid, want_kid)
assert float(loop.is_acc[:, C + 1].sum()) == N            # the padded duplicate on rank 1 was skipped
want_is = ref.is_f64(p_fake.numpy(), SPLITS)
got_is = loop.is_value()
assert abs(got_is[0] - want_is[0]) <= 1e-12 * want_is[0] and abs(got_is[1] - want_is[1]) <= 1e-12 * want_is[0], (got_is, want_is)
# the options leave images and moments alone
plain = hz.EvalLoop(None, "cpu", R, N, rank=r, world=2, noise_mode="const", feature_fn=Det(), fid_dim=D, latent_fn=latents, device_masks=False,
                    step_fn=step, fid_accumulate_fn=acc, fid_real=True)
plain.run(Loader(plain.ids))
images0, fid0 = plain.gather()
assert torch.equal(images0, images) and torch.equal(fid0.S, fid.S) and torch.equal(plain.fid_real.S, loop.fid_real.S)
dist.destroy_process_group()
one = run(0, 1)                                           # the same evaluation on one rank, without a process group
one.gather()
assert one.kid_value() == got_kid
assert np.allclose(one.is_value(), got_is, rtol=1e-13, atol=0)
print("rank", r, "ok")
'''
    port = str(37500 + os.getpid() % 2000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), SHG_ROOT=ROOT, SHG_PORT=port)
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out.decode()
