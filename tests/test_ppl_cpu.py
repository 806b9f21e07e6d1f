"""CPU (no GPU): the host side of the perceptual path length (sh-gan_amd/ppl.py) and of ``lpips.LPIPS(net='vgg')`` -- the trimmed mean and
its index arithmetic against numpy, the gather interleave, the sampler's draw order with stand-in networks, weight validation, refusals.
On the commit before this feature every test here fails at ``from shgan_amd import ppl`` (the state-dict tests at ``net='vgg'``)."""
import numpy as np
import pytest
import torch

import ppl_f64 as ref
from shgan_amd import _lib, lpips


@pytest.fixture(scope='module')
def ppl():
    from shgan_amd import ppl
    return ppl


def _values(n, seed):
    return np.random.RandomState(seed).lognormal(3.0, 1.0, size=n)


@pytest.mark.parametrize('n', [1, 2, 99, 100, 101, 50000])
def test_trimmed_mean_against_numpy(ppl, n):
    d = _values(n, n)
    got, want = ppl.trimmed_mean(torch.from_numpy(d)), ref.trimmed_mean_np(d)
    # the kept values are the same set; torch adds them in sorted order, numpy pairwise in the given order: n roundings of float64 at most
    assert abs(got - want) <= n * 2.0 ** -52 * want, (n, got, want)


def test_trimmed_mean_ties_equal_values_and_inf(ppl):
    same = np.full(250, 7.25)
    assert ppl.trimmed_mean(torch.from_numpy(same)) == ref.trimmed_mean_np(same) == 7.25
    # ties at both bounds: n = 300 -> lo = sorted[2], hi = sorted[297]; four values tie with lo, five with hi: all of them are kept
    d = np.concatenate([[1.0], np.full(4, 2.0), np.linspace(3, 4, 290), np.full(5, 9.0)])
    assert d.size == 300
    np.random.RandomState(0).shuffle(d)
    got, want = ppl.trimmed_mean(torch.from_numpy(d)), ref.trimmed_mean_np(d)
    assert abs(got - want) <= 300 * 2.0 ** -52 * want
    assert abs(want - d[d >= 2.0].mean()) <= 1e-12          # the single 1.0 is the only value cut
    # an inf among the values: above hi for n = 300 (cut), inside [lo, hi] for n = 50 (hi is the maximum: the mean is inf)
    d[0] = np.inf
    assert abs(ppl.trimmed_mean(torch.from_numpy(d)) - ref.trimmed_mean_np(d)) <= 300 * 2.0 ** -52 * ref.trimmed_mean_np(d)
    assert np.isfinite(ref.trimmed_mean_np(d))
    e = _values(50, 3)
    e[7] = np.inf
    assert ppl.trimmed_mean(torch.from_numpy(e)) == ref.trimmed_mean_np(e) == np.inf
    with pytest.raises(_lib.ShgError):
        ppl.trimmed_mean(torch.zeros(0, dtype=torch.float64))


def test_percentile_indices_against_numpy(ppl):
    for n in list(range(1, 301)) + [49999, 50000]:
        a = np.arange(n, dtype=np.float64)
        want = (int(np.percentile(a, 1, method='lower')), int(np.percentile(a, 99, method='higher')))
        assert ppl.percentile_indices(n) == want, n


class _Ranks:
    """Stand-in for evaluators.Collective: ``rows`` returns every rank's values and counts its calls."""

    def __init__(self, per_rank):
        self.per_rank, self.calls = per_rank, []

    def rows(self, local, arrange=True):
        self.calls.append((tuple(local.shape), local.dtype, arrange))
        return torch.stack([torch.cat(r) for r in self.per_rank])


@pytest.mark.parametrize('world,num_samples,B', [(1, 12, 2), (2, 13, 2), (3, 20, 3), (2, 3, 2)])
def test_gather_interleave_and_truncation(ppl, world, num_samples, B):
    rounds = ppl.sampling_rounds(num_samples, B, world)
    assert rounds == len(range(0, num_samples, B * world))
    per_rank = [[torch.arange(B, dtype=torch.float64) + 100 * r + 10 * k for k in range(rounds)] for r in range(world)]
    full = torch.stack([torch.cat(r) for r in per_rank])
    got = ppl.interleave(full, B, num_samples)
    want = ref.interleave_np([[t.numpy() for t in r] for r in per_rank], B, num_samples)
    assert got.shape == (num_samples,) and np.array_equal(got.numpy(), want)

    # compute_ppl: every rank calls the sampler `rounds` times, ONE gather at the end, none per batch
    calls = []

    def vgg(img, factor, crop):
        calls.append(tuple(img.shape))
        return per_rank[1 % world][len(calls) - 1] * 1e-8
    coll = _Ranks([[t for t in r] for r in per_rank])
    value = ppl.compute_ppl(_G(), vgg, num_samples=num_samples, batch_size=B, rank=1 % world, world=world, collective=coll)
    assert len(calls) == rounds and calls[0] == (2 * B, 3, 16, 16)
    assert coll.calls == ([((rounds * B,), torch.float64, False)] if world > 1 else [])
    src = want if world > 1 else np.concatenate([t.numpy() for t in per_rank[0]])[:num_samples]
    assert abs(value - ref.trimmed_mean_np(src)) <= 1e-12 * abs(ref.trimmed_mean_np(src))


class _Layer(torch.nn.Module):
    def __init__(self, res):
        super().__init__()
        self.register_buffer('noise_const', torch.full([res, res], float(res)))
        self.weight = torch.nn.Parameter(torch.ones(1))


class _Mapping(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, z, c):
        self.log.append(('mapping', z.clone(), tuple(c.shape)))
        return (z[:, :4] * 2).unsqueeze(1).repeat(1, 3, 1)


class _Synthesis(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log
        self.l0, self.l1 = _Layer(4), _Layer(8)

    def forward(self, ws, noise_mode=None, force_fp32=False):
        self.log.append(('synthesis', ws.clone(), noise_mode, force_fp32, self.l0.noise_const.clone(), self.l1.noise_const.clone()))
        return torch.zeros(ws.shape[0], 3, 16, 16)


class _G(torch.nn.Module):
    """Stand-in plain generator: records what mapping and synthesis receive.  The log list is shared with deep copies on purpose."""
    z_dim, c_dim, img_resolution, img_channels = 6, 0, 16, 3

    def __init__(self):
        super().__init__()
        self.log = []
        self.mapping, self.synthesis = _Mapping(self.log), _Synthesis(self.log)

    def __deepcopy__(self, memo):
        new = _G()
        new.load_state_dict(self.state_dict())
        new.log = new.mapping.log = new.synthesis.log = self.log
        return new


@pytest.mark.parametrize('space,sampling', [('w', 'end'), ('w', 'full'), ('z', 'full'), ('z', 'end')])
def test_sampler_draw_order(ppl, space, sampling):
    G, B, eps = _G(), 3, 1e-4
    seen = []

    def vgg(img, factor, crop):
        seen.append((tuple(img.shape), factor, crop))
        return torch.arange(1, B + 1, dtype=torch.float64) * 1e-8
    sampler = ppl.PPLSampler(G, vgg, epsilon=eps, space=space, sampling=sampling, crop=True, generator=torch.Generator().manual_seed(5))
    dist = sampler(torch.zeros(B, 0))
    # the same draws, by hand, in the reference's order: t, z (one randn of [2B, z_dim]), then one randn per noise_const buffer
    g = torch.Generator().manual_seed(5)
    t = torch.rand([B], generator=g) * (1 if sampling == 'full' else 0)
    z0, z1 = torch.randn([2 * B, 6], generator=g).chunk(2)
    n0, n1 = torch.randn([4, 4], generator=g), torch.randn([8, 8], generator=g)
    assert [e[0] for e in G.log] == ['mapping', 'synthesis']
    _, zin, cshape = G.log[0]
    _, ws, noise_mode, force_fp32, l0, l1 = G.log[1]
    assert cshape == (2 * B, 0) and noise_mode == 'const' and force_fp32 is True
    if sampling == 'end':
        assert bool((t == 0).all())
    mapped = lambda z: (z[:, :4] * 2).unsqueeze(1).repeat(1, 3, 1)     # noqa: E731
    if space == 'w':
        assert torch.equal(zin, torch.cat([z0, z1]))                                  # ONE mapping call on the concatenation
        w0, w1 = mapped(z0), mapped(z1)
        tt = t.unsqueeze(1).unsqueeze(2)
        assert torch.equal(ws, torch.cat([w0.lerp(w1, tt), w0.lerp(w1, tt + eps)]))   # epsilon is added in w
        if sampling == 'end':
            assert torch.equal(ws[:B], w0) and not torch.equal(ws[B:], w0)
    else:
        want = torch.cat([ref.slerp(z0, z1, t.unsqueeze(1)), ref.slerp(z0, z1, t.unsqueeze(1) + eps)])
        assert torch.equal(zin, want) and torch.equal(ws, mapped(want))
    # noise_const is re-drawn on the sampler's copy only
    assert torch.equal(l0, n0) and torch.equal(l1, n1)
    assert torch.equal(G.synthesis.l0.noise_const, torch.full([4, 4], 4.0)) and torch.equal(G.synthesis.l1.noise_const, torch.full([8, 8], 8.0))
    assert seen == [((2 * B, 3, 16, 16), 0, True)]                                   # factor = 16 // 256
    assert dist.dtype == torch.float64 and torch.equal(dist, torch.arange(1, B + 1, dtype=torch.float64) * 1e-8 / eps ** 2)
    sampler(torch.zeros(B, 0))                                                        # the next call draws on: new noise
    assert not torch.equal(G.log[3][4], n0)


def test_refusals(ppl):
    from shgan_amd import configs
    inpainter = configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)
    with pytest.raises(_lib.ShgError, match='conditioned on the known pixels'):
        ppl.PPLSampler(inpainter, lambda *a, **k: None)
    with pytest.raises(_lib.ShgError, match='conditioned on the known pixels'):
        ppl.ppl2_wend(inpainter, lambda *a, **k: None)
    with pytest.raises(_lib.ShgError, match='needs a plain generator'):
        ppl.PPLSampler(torch.nn.Linear(2, 2), lambda *a, **k: None)
    G = _G()
    G.c_dim = 2
    with pytest.raises(NotImplementedError, match='c_dim'):
        ppl.PPLSampler(G, lambda *a, **k: None)
    with pytest.raises(_lib.ShgError, match="space must be"):
        ppl.PPLSampler(_G(), lambda *a, **k: None, space='x')
    with pytest.raises(_lib.ShgError, match='vgg must be'):
        ppl.PPLSampler(_G(), object())
    with pytest.raises(_lib.ShgError, match='unknown ppl2_wend option'):
        ppl.ppl2_wend(_G(), lambda *a, **k: None, epsilon=1e-3)
    assert ppl.frontend_side(3, 512, 512, 2, True) == 128 and ppl.frontend_side(3, 264, 264, 1, True) == 132
    assert ppl.frontend_side(1, 1024, 1024, 4, False) == 256 and ppl.frontend_side(3, 64, 64, 0, False) == 64
    assert ppl.frontend_side(2, 64, 64, 1, False) is None and ppl.frontend_side(3, 64, 32, 1, False) is None
    assert ppl.frontend_side(3, 258, 258, 4, False) is None
    with pytest.raises(_lib.ShgError, match='HIP'):
        ppl.frontend(torch.zeros(1, 3, 64, 64), 0)                                    # a CPU tensor: there is no CPU path


def test_vgg_state_dict_validation_touches_no_device():
    sd = ref.vgg_random_state_dict(seed=1)
    assert lpips.validate_vgg_state_dict(sd) == list(ref.NARROW)
    cw = lpips.canonical_vgg_weights(sd)
    assert cw['widths'] == ref.NARROW and [cw[f'lin{n}'].shape[0] for n in range(5)] == [8, 16, 24, 32, 32]
    assert torch.equal(cw['shift'], torch.tensor(lpips.SHIFT)) and all(v.device.type == 'cpu' for v in cw.values() if torch.is_tensor(v))
    # every refusal is raised by the loader itself, for a device that does not exist: validation comes first
    bad = dict(sd)
    del bad['net.slice3.12.bias']
    with pytest.raises(_lib.ShgError, match=r"lacks 'net\.slice3\.12\.bias'"):
        lpips.LPIPS(net='vgg', state_dict=bad, device='cuda:99')
    bad = dict(sd, **{'net.slice6.30.weight': torch.zeros(1)})
    with pytest.raises(_lib.ShgError, match=r"unexpected state_dict key 'net\.slice6\.30\.weight'"):
        lpips.LPIPS(net='vgg', state_dict=bad, device='cuda:99')
    bad = dict(sd, **{'net.slice2.7.weight': torch.zeros(16, 8, 3, 3)})
    with pytest.raises(_lib.ShgError, match=r"'net\.slice2\.7\.weight' has shape \(16, 8, 3, 3\), expected \(16, 16, 3, 3\)"):
        lpips.LPIPS(net='vgg', state_dict=bad, device='cuda:99')
    bad = dict(sd, **{'lin2.model.1.weight': torch.zeros(1, 16, 1, 1)})
    with pytest.raises(_lib.ShgError, match=r"'lin2\.model\.1\.weight' has shape \(1, 16, 1, 1\), expected \(1, 24, 1, 1\)"):
        lpips.LPIPS(net='vgg', state_dict=bad, device='cuda:99')
    bad = dict(sd, **{'net.slice1.0.weight': torch.zeros(8, 3, 5, 5)})
    with pytest.raises(_lib.ShgError, match=r"expected \(8, 3, 3, 3\)"):
        lpips.Lpips.from_state_dict(bad, device='cuda:99', net='vgg')
    # the two-file layout
    conv, lin = ref.vgg_random_state_dict(seed=1, layout='features')
    conv['classifier.0.weight'] = torch.zeros(4, 4)                                   # ignored
    assert lpips.validate_vgg_state_dicts(conv, lin) == list(ref.NARROW)
    two = lpips.canonical_vgg_weights(conv, lin)
    assert all(torch.equal(two[k], cw[k]) for k in cw if k != 'widths')
    with pytest.raises(_lib.ShgError, match=r"lin state_dict lacks 'lin4\.model\.1\.weight'"):
        lpips.LPIPS(net='vgg', state_dict=conv, lin_state_dict={k: v for k, v in lin.items() if not k.startswith('lin4')}, device='cuda:99')
    with pytest.raises(_lib.ShgError, match=r"unexpected vgg16 state_dict key 'features\.30\.weight'"):
        lpips.LPIPS(net='vgg', state_dict=dict(conv, **{'features.30.weight': torch.zeros(1)}), lin_state_dict=lin, device='cuda:99')
    with pytest.raises(_lib.ShgError, match='std positive'):
        lpips.LPIPS(net='vgg', state_dict=sd, device='cuda:99', std=(1, 0, 1))
    with pytest.raises(_lib.ShgError, match='net must be one of'):
        lpips.LPIPS(net='squeeze', state_dict=sd)
    with pytest.raises(_lib.ShgError, match='needs state_dict'):
        lpips.LPIPS(net='vgg')


def test_new_entry_points_are_declared_and_exported():
    import ctypes
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('shg_ppl_frontend_f32', 'shg_lpips_scaling_f32'):
        assert name + '(' in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 40
    # argument errors are decided on the host, before a launch: reachable without a device
    raw = _lib.get_lib()
    three = (ctypes.c_float * 3)(1, 1, 1)
    p = ctypes.c_void_p(64)
    for args, msg in (((2, 3, 64, 32, 1, 0), 'not square'), ((2, 2, 64, 64, 1, 0), 'channels'), ((1, 3, 258, 258, 4, 0), 'not divisible'),
                      ((1, 3, 4, 4, 1, 1), 'empty'), ((1, 3, 64, 64, -1, 0), 'factor')):
        assert raw.shg_ppl_frontend_f32(p, p, *args, three, three, None) == -1 and msg in raw.shg_last_error().decode()
    assert raw.shg_ppl_frontend_f32(None, p, 1, 3, 64, 64, 1, 0, three, three, None) == -1
    assert raw.shg_ppl_frontend_f32(p, p, 1, 3, 64, 64, 1, 0, three, (ctypes.c_float * 3)(1, 0, 1), None) == -1
