"""CPU (no GPU): the host side of the improved precision / recall metric -- the float64 restatement of tests/pr_f64.py against a direct
transcription of the reference's loop in float64, ``pr_from_features`` plumbing with stand-ins for the kernels, the detector's key
validation, the area-resize bin table, the new symbols of the C ABI with their argument checks, and EvalLoop's ``pr`` option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, precision_recall as prm, vgg16
from shgan_amd import eval_harness as hz

import pr_f64 as ref

NEW = ('shg_pr_workspace_bytes', 'shg_pr_radii_f16', 'shg_pr_inside_f16', 'shg_vgg16_frontend_f32', 'shg_vgg16_maxpool2_f32')


def _feats(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.relu(torch.randn(n, D, generator=g)) * 3).to(torch.float16)


def _transcription(real, fake, k, row_batch=37):
    """precision_recall.py:49-59 for one rank, with float64 cdist in place of the fp16 one: per manifold batch kthvalue(k + 1) of the
    distances cast to fp16, per probe batch ``(dist <= kth).any(dim=1)``, the mean of the flags."""
    out = []
    for manifold, probes in ((real, fake), (fake, real)):
        md = manifold.double()
        kth = torch.cat([torch.cdist(mb.double()[None], md[None], compute_mode='donot_use_mm_for_euclid_dist')[0].to(torch.float16)
                         .to(torch.float32).kthvalue(k + 1).values.to(torch.float16) for mb in manifold.split(row_batch)])
        pred = [(torch.cdist(pb.double()[None], md[None], compute_mode='donot_use_mm_for_euclid_dist')[0].to(torch.float16) <= kth).any(dim=1)
                for pb in probes.split(row_batch)]
        out.append(float(torch.cat(pred).to(torch.float32).mean()))
    return tuple(out)


@pytest.mark.parametrize('k', [1, 3, 15])
@pytest.mark.parametrize('n,m,D', [(90, 70, 64), (40, 55, 128)])
def test_restatement_equals_the_transcribed_loop_in_float64(n, m, D, k):
    real, fake = _feats(n, D, 1), _feats(m, D, 2) * 1.05
    fake = fake.to(torch.float16)
    want = _transcription(real, fake, k)
    got = ref.pr16(real.numpy(), fake.numpy(), k)
    assert got == pytest.approx(want, abs=1e-7)                  # (the transcription averages in float32)
    r = ref.radii16(real.numpy(), k)
    assert r.dtype == np.float16 and np.array_equal(r, ref.radii_f64(real.numpy(), k).astype(np.float16))
    assert 0 < got[0] < 1 or 0 < got[1] < 1 or k == 15


def test_restatement_on_small_integers_is_exact_and_has_ties():
    """Rows from {0, 1, 2}, D = 64: every squared distance is an integer <= 256, and many probes sit exactly ON a radius."""
    g = np.random.RandomState(0)
    man, probes = g.randint(0, 3, (200, 64)).astype(np.float32), g.randint(0, 3, (150, 64)).astype(np.float32)
    d2 = ((man[:, None] - man[None]) ** 2).sum(-1)
    assert d2.max() <= 256 and np.array_equal(ref.dist16(man, man), np.sqrt(d2.astype(np.float64)).astype(np.float16))
    r = ref.radii16(man, 3)
    d = ref.dist16(probes, man)
    assert int(((d == r[None]).any(axis=1)).sum()) > 10
    assert (d <= r[None]).any(axis=1).sum() > (d < r[None]).any(axis=1).sum()


def test_pr_from_features_plumbing_with_stand_ins_and_host_tensors_raise():
    real, fake = _feats(60, 64, 3), _feats(45, 64, 4)
    calls = []

    def radii_fn(feats, k):
        calls.append(('radii', tuple(feats.shape), k))
        return torch.from_numpy(ref.radii16(feats.numpy(), k))

    def inside_fn(probes, manifold, radii):
        calls.append(('inside', tuple(probes.shape), tuple(manifold.shape)))
        return torch.from_numpy(ref.inside16(probes.numpy(), manifold.numpy(), radii.numpy()))
    got = prm.pr_from_features(real, fake, nhood_size=2, kernels_fn=(radii_fn, inside_fn))
    assert got == ref.pr16(real.numpy(), fake.numpy(), 2) and all(isinstance(v, float) for v in got)
    assert calls == [('radii', (60, 64), 2), ('inside', (45, 64), (60, 64)), ('radii', (45, 64), 2), ('inside', (60, 64), (45, 64))]
    same = prm.pr_from_features(real, real, kernels_fn=(radii_fn, inside_fn))
    assert same == (1.0, 1.0)
    for bad in (dict(nhood_size=0), dict(nhood_size=16)):
        with pytest.raises(ValueError, match='nhood_size'):
            prm.pr_from_features(real, fake, kernels_fn=(radii_fn, inside_fn), **bad)
    with pytest.raises(ValueError, match='rows'):
        prm.pr_from_features(real[:3], fake, nhood_size=3, kernels_fn=(radii_fn, inside_fn))
    with pytest.raises(ValueError, match='one D'):
        prm.pr_from_features(real, fake[:, :32], kernels_fn=(radii_fn, inside_fn))
    with pytest.raises(_lib.ShgError, match='HIP'):
        prm.pr_from_features(real, fake)
    with pytest.raises(_lib.ShgError, match='HIP'):
        prm.radii(real)
    with pytest.raises(_lib.ShgError, match='HIP'):
        prm.inside(fake, real, torch.zeros(60, dtype=torch.float16))


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name), name
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    assert lib.shg_pr_workspace_bytes.restype == ctypes.c_size_t
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    # tiles of 128 swept rows, at most 16 slices; radii: n norms (rounded up to 256 bytes) + slices * n lists of 4 / 8 / 16 floats
    assert lib.shg_pr_workspace_bytes(0, 200, 3) == 1024 + 2 * 200 * 4 * 4
    assert lib.shg_pr_workspace_bytes(0, 128, 4) == 512 + 1 * 128 * 8 * 4
    assert lib.shg_pr_workspace_bytes(0, 50000, 15) == 200192 + 16 * 50000 * 16 * 4
    assert lib.shg_pr_workspace_bytes(150, 200, 0) == 768 + 1024 + 2 * 150
    assert lib.shg_pr_workspace_bytes(5, 1, 0) == 0 and lib.shg_pr_workspace_bytes(0, 9, 0) == 0 and lib.shg_pr_workspace_bytes(9, 9, 16) == 0
    p = ctypes.c_void_p(4096)

    def radii(feats=p, n=8, D=64, k=3, ws=p, nbytes=1 << 20, out=p):
        return lib.shg_pr_radii_f16(feats, n, D, k, ws, nbytes, out, None)
    assert radii(feats=None) == -1 and 'null' in err()
    assert radii(k=0) == -1 and 'nhood_size' in err()
    assert radii(k=16) == -1 and 'nhood_size' in err()
    assert radii(n=3) == -1 and 'rows' in err()
    assert radii(D=56) == -1 and 'multiple of 8' in err()
    assert radii(D=68) == -1 and 'multiple of 8' in err()
    assert radii(feats=ctypes.c_void_p(4100)) == -1 and 'aligned' in err()
    assert radii(ws=None) == -1 and 'workspace' in err()
    assert radii(nbytes=16) == -1 and 'too small' in err()

    def inside(probes=p, m=8, man=p, n=8, D=64, r=p, ws=p, nbytes=1 << 20, out=p):
        return lib.shg_pr_inside_f16(probes, m, man, n, D, r, ws, nbytes, out, None)
    assert inside(r=None) == -1 and 'null' in err()
    assert inside(m=0) == -1 and 'probes' in err()
    assert inside(n=1) == -1 and 'manifold' in err()
    assert inside(D=32) == -1 and 'multiple of 8' in err()
    assert inside(man=ctypes.c_void_p(4104)) == -1 and 'aligned' in err()
    assert inside(nbytes=8) == -1 and 'too small' in err()
    c3 = (ctypes.c_float * 3)(1, 1, 1)
    z3 = (ctypes.c_float * 3)(1, 0, 1)
    assert lib.shg_vgg16_frontend_f32(None, None, 1.0, 0.0, c3, c3, p, 1, 8, 8, None) == -1 and 'null' in err()
    assert lib.shg_vgg16_frontend_f32(p, None, 1.0, 0.0, c3, z3, p, 1, 8, 8, None) == -1 and 'positive' in err()
    assert lib.shg_vgg16_frontend_f32(p, None, 1.0, 0.0, c3, c3, p, 0, 8, 8, None) == -1 and 'geometry' in err()
    assert lib.shg_vgg16_maxpool2_f32(p, None, 1, 1, 4, 4, None) == -1 and 'null' in err()
    assert lib.shg_vgg16_maxpool2_f32(p, p, 1, 1, 1, 4, None) == -1 and 'geometry' in err()


def test_build_recipe_lists_the_new_sources():
    src = open(os.path.join(ROOT, 'sh-gan_amd', 'build.py')).read()
    assert "'pr.hip'" in src and "'vgg16.hip'" in src


def test_vgg16_key_validation_names_the_key():
    sd = ref.random_state_dict(1)
    widths, f1, f = vgg16.validate_state_dict(sd)
    assert widths == [c // 8 for c in ref.TORCHVISION_WIDTHS] and (f1, f) == (128, 128)
    ok = dict(sd, **{'classifier.6.weight': torch.zeros(10, 128), 'classifier.6.bias': torch.zeros(10)})
    vgg16.validate_state_dict(ok)
    for key in ('features.0.weight', 'features.28.bias', 'classifier.0.weight', 'classifier.3.bias'):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(_lib.ShgError, match=re.escape(repr(key))):
            vgg16.Vgg16Features.from_state_dict(bad, device='cuda')          # raises before a device is touched
    with pytest.raises(_lib.ShgError, match=re.escape("'features.1.weight'")):
        vgg16.validate_state_dict(dict(sd, **{'features.1.weight': torch.zeros(1)}))
    with pytest.raises(_lib.ShgError, match=re.escape("'avgpool.x'")):
        vgg16.validate_state_dict(dict(sd, **{'avgpool.x': torch.zeros(1)}))
    for key, shape in (('features.5.weight', (16, 9, 3, 3)), ('features.7.weight', (16, 16, 5, 5)), ('features.10.bias', (31,)),
                       ('classifier.0.weight', (128, 64 * 36)), ('classifier.3.weight', (128, 64)), ('classifier.3.bias', (64,))):
        with pytest.raises(_lib.ShgError, match=re.escape(repr(key))):
            vgg16.validate_state_dict(dict(sd, **{key: torch.zeros(shape)}))
    with pytest.raises(_lib.ShgError, match='std'):
        vgg16.Vgg16Features.from_state_dict(sd, device='cuda', std=(1, 0, 1))
    assert vgg16.macs_per_image(ref.TORCHVISION_WIDTHS, 4096, 4096) == 15346630656 + 25088 * 4096 + 4096 * 4096


@pytest.mark.parametrize('size', [256, 299, 512, 1024, 160, 288, 224])
def test_area_bin_table_equals_interpolate_area(size):
    bins = vgg16.area_bins(size)
    assert len(bins) == 224 and bins[0][0] == 0 and bins[-1][1] == size and all(0 <= a < b <= size for a, b in bins)
    x = torch.rand(1, 1, 1, size, dtype=torch.float64, generator=torch.Generator().manual_seed(size))
    want = F.interpolate(x, size=(1, 224), mode='area')[0, 0, 0]
    got = torch.stack([x[0, 0, 0, a:b].mean() for a, b in bins])
    assert float((got - want).abs().max()) <= 1e-15
    assert torch.equal(ref.frontend_f64(torch.full((1, 3, size, 224), 7.0), mean=(1, 2, 3), std=(2, 2, 2))[0, :, 5, 5],
                       torch.tensor([3.0, 2.5, 2.0], dtype=torch.float64))


def test_eval_loop_pr_option_validation():
    det = lambda img, input_range=None: torch.zeros(img.shape[0], 6)        # noqa: E731
    with pytest.raises(ValueError, match='unknown pr option'):
        hz.EvalLoop(None, 'cpu', 8, 7, pr=dict(detector=det, dim=6, nhood=3))
    with pytest.raises(ValueError, match='detector'):
        hz.EvalLoop(None, 'cpu', 8, 7, pr=dict(nhood_size=3, dim=6))
    with pytest.raises(ValueError, match='dict'):
        hz.EvalLoop(None, 'cpu', 8, 7, pr=True)
    with pytest.raises(ValueError, match='feature width'):
        hz.EvalLoop(None, 'cpu', 8, 7, pr=dict(detector=det))
    with pytest.raises(ValueError, match='nhood_size'):
        hz.EvalLoop(None, 'cpu', 8, 7, pr=dict(detector=det, dim=6, nhood_size=16))
    plain = hz.EvalLoop(None, 'cpu', 8, 7)
    assert plain.evaluators == {} and plain.pr_opts is None and plain.pr_features is None          # no evaluator object, no buffer
    with pytest.raises(ValueError, match='pr=dict'):
        plain.pr_value()
    loop = hz.EvalLoop(None, 'cpu', 8, 7, pr=dict(detector=det, dim=6))
    assert list(loop.evaluators) == ['pr'] and loop.pr_opts == dict(nhood_size=3)
    rows = loop.evaluators['pr'].local
    assert len(rows) == 2 and all(t.shape == (7, 6) and t.dtype == torch.float16 for t in rows)
    assert loop.feature_fn is None and 'detector' not in loop.evaluators and loop.kid_features is None


def test_eval_loop_pr_on_the_cpu_with_stand_ins():
    """One rank, 11 items in batches of 4, stand-ins for the generator step, the detector and the kernels: pr_value() equals the
    yardstick on the detector's features of the gathered images and the loader's reals; the images equal those of a loop without pr."""
    R, N, B, D = 16, 11, 4, 64

    def step(x, z, out):
        out.copy_(((x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.2).tanh() * 127.5 + 127.5).clamp(0, 255).to(torch.uint8))
        return out

    class Det:
        dim = D

        def __call__(self, img, input_range=None):
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
    fns = (lambda f, k: torch.from_numpy(ref.radii16(f.numpy(), k)),
           lambda p, m, r: torch.from_numpy(ref.inside16(p.numpy(), m.numpy(), r.numpy())))

    def run(**kw):
        loop = hz.EvalLoop(None, 'cpu', R, N, noise_mode='const', latent_fn=latents, device_masks=False, step_fn=step, **kw)
        loop.run(Loader(loop.ids))
        return loop, loop.gather()[0]
    loop, images = run(pr=dict(detector=Det(), nhood_size=2, kernels_fn=fns))
    _, images0 = run()
    assert torch.equal(images, images0)
    fake, real = loop.pr_features
    assert fake.shape == real.shape == (N, D) and fake.dtype == torch.float16
    reals = torch.cat([x for x, _, _ in Loader(list(range(N)))])
    f_fake, f_real = Det()(images).to(torch.float16), Det()(reals, input_range='pm1').to(torch.float16)
    assert torch.equal(fake, f_fake) and torch.equal(real, f_real)
    assert loop.pr_value() == ref.pr16(f_real.numpy(), f_fake.numpy(), 2)
