"""GPU: the three entry points of pluralistic sampling -- shg_plural_expand, shg_plural_composite_u8 (csrc/plural.hip) and
shg_lpips_head_pairs_f32 (csrc/lpips.hip) -- bit for bit against what they replace (``torch.repeat_interleave``, ``kernels.composite_u8`` on a
repeated input, ``lpips.head`` on gathered rows), the pair head also against float64 at the bound tests/test_gpu_lpips.py holds the head to.

Every comparison runs three more times through ``_checked``: with every fresh allocation pre-filled with NaN bytes and with large values
(tests/alloc_fill.py: the result may not depend on what a new buffer held) and with every buffer, operands included, between poisoned guard
bands (tests/alloc_guard.py: nothing outside a buffer may be touched).  The allocation sites of the new wrappers are newer than the site
tables of tests/test_gpu_alloc_fill.py / test_gpu_alloc_guard.py and have no entry there (the note above kernels.plural_composite_u8 says
how they stay out of those tables' scan); this module is where they are filled and guarded.

On the commit before this feature every test fails with a missing attribute (``kernels.plural_expand``, ``kernels.plural_composite_u8``,
``lpips.head_pairs``)."""
import numpy as np
import pytest
import torch

import alloc_fill
import alloc_guard
import lpips_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bytes(t):
    """The tensor's elements in logical order as raw bytes."""
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes() if t.numel() else b''


def _checked(run, host_inputs, site):
    """run(*device_inputs) -> list of tensors.  Plain run, then the same bits with fresh allocations filled ('nan', 'big') and with every
    buffer guarded (inputs sent to the device inside the guard, so they are housed too); ``site``: the wrapper's allocation site, which both
    helpers must have seen.  Returns the plain run's outputs."""
    base = run(*[t.to(DEV) for t in host_inputs])
    torch.cuda.synchronize()
    want = [_bytes(t) for t in base]
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got = run(*[t.to(DEV) for t in host_inputs])
            torch.cuda.synchronize()
        assert site in rec.sites, f'no allocation of {site} went through the filled factories: {sorted(rec.sites)}'
        assert [_bytes(t) for t in got] == want, f'the result depends on the old contents of a fresh allocation ({pattern})'
    with alloc_guard.guarded() as rec:
        got = run(*[t.to(DEV) for t in host_inputs])
        bad = rec.violations()
        assert site in rec.sites and not bad, bad
        assert [_bytes(t) for t in got] == want
    return base


# ------------------------------------------------------------------------------------------------ expansion

def _levels(n):
    """Host tensors [n, ...] with 4, 36, 96, 16 400 bytes per image (smallest; no multiple of 16; fp16 [3,4,4]; more than one workgroup of
    16-byte units plus a tail) and, beyond those, 24 bytes of float64 (8-byte units) and 6 bytes of fp16 (2-byte units)."""
    g = torch.Generator().manual_seed(100 + n)
    return [torch.randn(n, 1, generator=g),
            torch.randn(n, 3, 3, generator=g),
            torch.randn(n, 3, 4, 4, generator=g).to(torch.float16),
            torch.randint(0, 256, (n, 16400), generator=g, dtype=torch.uint8),
            torch.randn(n, 3, generator=g, dtype=torch.float64),
            torch.randn(n, 3, generator=g).to(torch.float16)]


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('N', [1, 2])
def test_expand_is_repeat_interleave_bit_for_bit(N, K):
    from shgan_amd import kernels

    def run(*ts):
        ts = list(ts)
        ts[2] = ts[2].contiguous(memory_format=torch.channels_last)          # the layout the float16 blocks hand over
        return kernels.plural_expand(ts, K)                                  # ONE launch for all levels
    hosts = _levels(N)
    assert [t[0].numel() * t.element_size() for t in hosts] == [4, 36, 96, 16400, 24, 6]
    outs = _checked(run, hosts, ('kernels.py', 'plural_expand'))
    for i, (t, o) in enumerate(zip(hosts, outs)):
        want = torch.repeat_interleave(t, K, dim=0)
        assert o.dtype == t.dtype and tuple(o.shape) == tuple(want.shape), i
        assert _bytes(o) == _bytes(want), f'level {i}'
    assert outs[2].is_contiguous(memory_format=torch.channels_last) and outs[0].is_contiguous()


def test_expand_takes_the_narrow_units_for_odd_addresses_and_sizes():
    """A level whose address is odd moves in single bytes, one at a 4-byte offset with 20 bytes per image in 4-byte units."""
    from shgan_amd import kernels
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(0, 256, (64,), generator=g, dtype=torch.uint8).to(DEV)
    odd = raw[1:1 + 2 * 7].view(2, 7)
    four = raw[20:20 + 2 * 20].view(2, 20)
    assert odd.data_ptr() % 2 == 1 and four.data_ptr() % 16 == 4
    with alloc_guard.guarded(operands=False) as rec:
        outs = kernels.plural_expand([odd, four], 3)
        assert not rec.violations()
    assert _bytes(outs[0]) == _bytes(odd.repeat_interleave(3, 0)) and _bytes(outs[1]) == _bytes(four.repeat_interleave(3, 0))
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError, match='rows'):
        kernels.plural_expand([odd, raw[:9].view(3, 3)], 2)


# ------------------------------------------------------------------------------------------------ composite

def _composite_inputs(N, K, H, W, seed):
    """x4 with a 0 / 1 mask that changes inside every row, known pixels and images on u8 levels +- a hair: values on both sides of the
    truncation edges, and some outside [-1, 1] for the clamp."""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(N, 1, H, W, generator=g) < 0.5).float()
    mask[:, :, :, 0], mask[:, :, :, W - 1] = 1.0, 0.0
    level = lambda *s: (torch.randint(0, 256, s, generator=g).float() + (torch.rand(s, generator=g) - 0.5) * 4e-3) / 127.5 - 1.0   # noqa: E731
    real = level(N, 3, H, W)
    img = level(N * K, 3, H, W)
    img.view(-1)[::7] *= 1.5
    return torch.cat([mask - 0.5, real * mask], dim=1), img


@pytest.mark.parametrize('N,K,H,W', [(2, 3, 16, 16), (1, 2, 2, 2), (2, 3, 3, 4), (2, 1, 16, 16)])
def test_plural_composite_is_composite_on_the_repeated_input(N, K, H, W):
    """(2, 2): the smallest extent shg_composite_u8's argument check takes (H*W a positive multiple of 4); (3, 4): an odd one."""
    from shgan_amd import kernels
    x4, img = _composite_inputs(N, K, H, W, seed=H * 10 + K)
    got, = _checked(lambda a, b: [kernels.plural_composite_u8(a, b, K)], [x4, img], ('kernels.py', 'plural_composite_u8'))
    want = kernels.composite_u8(x4.to(DEV).repeat_interleave(K, 0), img.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N * K, 3, H, W)
    assert torch.equal(got, want)
    m = (x4[:, :1] + 0.5).bool().repeat_interleave(K, 0).expand(-1, 3, -1, -1)
    assert bool(m.any()) and bool((~m).any()) and len(np.unique(got.cpu().numpy())) > 8
    out = torch.zeros_like(want)
    assert kernels.plural_composite_u8(x4.to(DEV), img.to(DEV), K, out=out) is out and torch.equal(out, want)


def test_plural_composite_refusals():
    from shgan_amd import _lib, kernels
    x4, img = (t.to(DEV) for t in _composite_inputs(2, 3, 4, 4, seed=1))
    with pytest.raises(_lib.ShgError, match='do not fit'):
        kernels.plural_composite_u8(x4, img, 2)
    with pytest.raises(_lib.ShgError, match='multiple of 4'):
        kernels.plural_composite_u8(x4[:, :, :3, :3].contiguous(), img[:, :, :3, :3].contiguous(), 3)


# ------------------------------------------------------------------------------------------------ pair head

IA = [0, 1, 2, 0, 3, 0, 1]          # M = 4, P = 7: (0,0) a row with itself; (1,2) and its reverse (2,1); (0,3) twice; (1,2) twice
IB = [0, 2, 1, 3, 2, 3, 2]


def _features(C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(4, C, h, w, generator=g)
    if C > 1:
        f = torch.relu(f)                       # ReLU-like maps, as the taps are; one pixel whose features are all zero in two of the rows
        f[:2, :, 0, 0] = 0
    else:
        f = f.abs() * torch.tensor([1.0, -1.0, 1.0, -1.0]).view(4, 1, 1, 1)     # one channel: f^ = +-1, so that pairs of unlike rows differ
    return f, torch.rand(C, generator=g) * 2 / C


@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (15, 15)])
@pytest.mark.parametrize('C', [64, 1])
def test_pair_head_is_the_head_on_the_gathered_rows(C, hw):
    """C = 1 is the smallest channel count shg_lpips_head_f32 takes (its check: C >= 1)."""
    from shgan_amd import lpips
    f, w = _features(C, *hw, seed=C + hw[0])
    ia, ib = torch.tensor(IA, dtype=torch.int32), torch.tensor(IB, dtype=torch.int32)

    def run(f_, w_):
        out = torch.full((7,), 1.5, dtype=torch.float64, device=DEV)            # ``out`` is added to
        return [lpips.head_pairs(f_, ia, ib, w_, out)]
    got, = _checked(run, [f, w], ('lpips.py', 'head_pairs'))
    fd, wd = f.to(DEV), w.to(DEV)
    want = lpips.head(fd[ia.long()], fd[ib.long()], wd, torch.full((7,), 1.5, dtype=torch.float64, device=DEV))
    assert torch.equal(got, want)                                               # bit for bit the existing head on (f[ia], f[ib])
    v = (got - 1.5).cpu()
    assert float(v[0]) == 0.0                                                   # a row against itself: exactly 0
    assert float(v[1]) == float(v[2]) == float(v[6])                            # a pair, its reverse, the pair again
    assert float(v[3]) == float(v[5])
    # the same pair alone (P = 1), from device-resident tables
    for p in (1, 4):
        one = lpips.head_pairs(fd, ia[p:p + 1].to(DEV), ib[p:p + 1].to(DEV), wd, torch.full((1,), 1.5, dtype=torch.float64, device=DEV))
        assert torch.equal(one, got[p:p + 1]), p
    ref64 = ref.head_f64(f[ia.long()], f[ib.long()], w)
    err = float((v - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))
    print(f'pair head C={C} {hw}: values {[f"{x:.4e}" for x in ref64.tolist()]} rel err {err:.2e}')
    assert float(ref64.max()) > 0 and err <= 1e-5, (C, hw, err)                 # the bound of test_gpu_lpips.test_head_against_float64


def test_pair_head_index_out_of_range():
    """Host tables: the argument error, nothing launched, ``out`` untouched.  Device tables: the documented clamp into [0, M) and the flag."""
    from shgan_amd import _lib, lpips
    f, w = _features(64, 3, 5, seed=3)
    fd, wd = f.to(DEV), w.to(DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)            # noqa: E731
    for ia, ib in (([0, 4], [1, 1]), ([0, 1], [1, -1])):
        out = torch.full((2,), 1.5, dtype=torch.float64, device=DEV)
        with pytest.raises(_lib.ShgError, match=r'outside \[0, 4\)'):
            lpips.head_pairs(fd, i32(ia), i32(ib), wd, out)
        torch.cuda.synchronize()
        assert out.tolist() == [1.5, 1.5]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with alloc_guard.guarded(operands=False) as rec:
        got = lpips.head_pairs(fd, i32([0, 5, 1]).to(DEV), i32([1, -2, 2]).to(DEV), wd, torch.zeros(3, dtype=torch.float64, device=DEV), err=flag)
        assert not rec.violations()
    want = lpips.head_pairs(fd, i32([0, 3, 1]), i32([1, 0, 2]), wd, torch.zeros(3, dtype=torch.float64, device=DEV))
    assert int(flag) == 1 and torch.equal(got, want)
    ok = torch.zeros(1, dtype=torch.int32, device=DEV)
    lpips.head_pairs(fd, i32([0, 3]).to(DEV), i32([1, 0]).to(DEV), wd, torch.zeros(2, dtype=torch.float64, device=DEV), err=ok)
    assert int(ok) == 0
    with pytest.raises(_lib.ShgError, match='int32'):
        lpips.head_pairs(fd, torch.tensor([0]), torch.tensor([1]), wd, torch.zeros(1, dtype=torch.float64, device=DEV))
