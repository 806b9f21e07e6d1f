"""No result may depend on the old contents of a fresh allocation (run the GPU part with -m gpu on an MI355X).

Every device buffer of the product comes from ``torch.empty`` / ``torch.empty_like`` / ``Tensor.new_empty`` (``_Launch.new`` and ``_new_cl``
go through ``torch.empty``; the HIP library never allocates), so every entry point is correct only if its kernels write each element
anything later reads: channel padding, the pitch padding of planes, ragged last tiles, slices the grid did not reach, the unused part of
a workspace.  In a fresh process a new block is almost always zero -- the one value that hides a violation.  Here the value is chosen
(tests/alloc_fill.py) and every case runs four times, built and called under the fill: 'zero', 'zero', 'nan', 'big'.

``independent`` then asserts, in this order:
  1. control: the two 'zero' runs are bit-equal (otherwise the case is not reproducible, which is another finding than a fill dependence);
  2. independence: the 'nan' and the 'big' results are bit-equal to the 'zero' result, every returned tensor;
  3. correctness under poison: the 'nan' result is finite and meets the bar the case already has against its float64 reference.
No tolerance is introduced here: each bar is the one of the route table or test the case comes from.

The last tests are host-only: every allocation site of the package (``sh-gan_amd/**/*.py``) is either claimed by cases that were seen to
reach it (``SITES``; each GPU case asserts its claims against what the fill recorded) or listed with the reason why the fill has nothing
to say about it (``NOT_FILLED``)."""
import ast
import contextlib
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from alloc_fill import PACKAGE_DIR, WRAPPERS, filled
from conftest import ROOT, load_golden, rel_err

gpu = pytest.mark.gpu
DEV = 'cuda:0'
ORDER = ('zero', 'zero', 'nan', 'big')

# Cases whose results are not bit-reproducible from run to run; the evidence is the kernel source itself.  Steps 1 and 2 are dropped for
# them and step 3 runs under all three fills.  This table may not grow without a source line that documents float atomics.
NOT_REPRODUCIBLE = {
    'ada:adjoint': ('ada.hip', 25, 'gx must be zero on entry.  The order of float atomics is not fixed: the gradient is not bit-reproducible.'),
}


# ------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------

def _tensors(out):
    """The tensors of a result, in order: nested lists / tuples / dicts are walked, None is skipped, numbers become float64 scalars."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out, key=str) for t in _tensors(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _tensors(o)]
    if isinstance(out, (bool, int, float, np.floating, np.integer)):
        return [torch.tensor(float(out), dtype=torch.float64)]
    if isinstance(out, np.ndarray):
        return [torch.from_numpy(np.ascontiguousarray(out))]
    raise TypeError(f'a case returned {type(out).__name__}')


def _bits(t):
    """An integer view of the bytes (NaN == NaN, -0.0 != 0.0)."""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _snapshot(out):
    return [t.detach().cpu().clone() for t in _tensors(out)]


def _difference(a, b):
    """None when two snapshots are bit-equal, otherwise where they differ: tensor index, count, the first positions and their bounding box
    (which tile edge or padding an unwritten element belongs to)."""
    if len(a) != len(b):
        return f'{len(a)} tensors against {len(b)}'
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype != y.dtype or tuple(x.shape) != tuple(y.shape):
            return f'tensor {k}: {x.dtype} {tuple(x.shape)} against {y.dtype} {tuple(y.shape)}'
        d = _bits(x) != _bits(y)
        if bool(d.any()):
            idx = d.nonzero()
            lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
            first = idx[:4].tolist()
            vals = [(float(x[tuple(i)]), float(y[tuple(i)])) for i in first] if x.dtype != torch.bool else []
            return (f'tensor {k} {tuple(x.shape)} {x.dtype}: {int(d.sum())} of {d.numel()} elements differ, first at {first} = {vals}, '
                    f'within {lo} .. {hi}')
    return None


def _reset_caches():
    """Prepared weights of the modules (``_ParamCache``): a module-level case must prepare them again under each fill."""
    import shgan_amd  # noqa: F401
    from shgan_amd.model_zoo import stylegan
    stylegan.invalidate_param_caches()


def _run(make, pattern):
    _reset_caches()
    with filled(pattern) as rec:
        call, ctx = make()
        out = call()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    return out, ctx, rec.sites


def independent(make, bars, reproducible=True, case=None, finite=True):
    """``make() -> (call, ctx)`` builds a case (its inputs, its weight preparation, its float64 reference), ``call()`` runs it and returns
    its results, ``bars(out, ctx)`` asserts the case's own bar.  ``finite=False``: the case's expected result holds infinities (its bar
    compares them bit for bit).  -> the allocation sites the fills saw."""
    sites = set()
    if not reproducible:
        assert case in NOT_REPRODUCIBLE, f'{case}: only the cases of NOT_REPRODUCIBLE may skip the bit comparison'
        for pattern in ('zero', 'nan', 'big'):
            out, ctx, seen = _run(make, pattern)
            sites |= seen
            assert all(bool(torch.isfinite(t).all()) for t in _tensors(out) if t.is_floating_point()), f'not finite under the {pattern!r} fill'
            with filled(pattern) as rec:
                bars(out, ctx)
            sites |= rec.sites
        return sites
    runs = []
    for pattern in ORDER:
        out, ctx, seen = _run(make, pattern)
        sites |= seen
        runs.append((out, ctx, _snapshot(out)))
    assert len(runs[0][2]) > 0, 'the case returned no tensor'
    diff = _difference(runs[0][2], runs[1][2])
    assert diff is None, f'NOT REPRODUCIBLE (two runs under the same zero fill differ; this says nothing about the fill): {diff}'
    for k, pattern in ((2, 'nan'), (3, 'big')):
        diff = _difference(runs[0][2], runs[k][2])
        assert diff is None, f'DEPENDS ON STALE MEMORY (the {pattern!r} fill against the zero fill): {diff}'
    out, ctx, snap = runs[2]
    for k, t in enumerate(snap):
        if finite and t.is_floating_point():
            assert bool(torch.isfinite(t).all()), f'NOT FINITE under the nan fill: tensor {k} {tuple(t.shape)}'
    with filled('nan') as rec:
        bars(out, ctx)
    return sites | rec.sites


def _claimed(case_id):
    return {site for site, ids in SITES.items() if case_id in ids}


def _finish(case_id, sites):
    print(f'SITES_SEEN {case_id} {sorted(sites)}')
    missing = _claimed(case_id) - sites
    assert not missing, f'{case_id} is listed in SITES for {sorted(missing)} but no allocation there was filled while it ran'


def _toy(write, post=lambda y: y, device='cpu'):
    """A stand-in entry point: allocates 6 floats, writes ``write`` of them from its input, returns post(buffer)."""
    def make():
        x = torch.arange(1.0, 7.0, device=device)

        def call():
            y = torch.empty(6, device=device)
            y[:write] = x[:write] * 2
            return post(y)
        return call, x * 2
    return make


def test_the_judge_on_host_stand_ins():
    """What each step of ``independent`` catches, shown on toy entry points (no GPU): a complete writer passes; an element left unwritten
    is a fill finding, also when a clamp (fmin: NaN -> the bound) or a ReLU would have turned the poison into a finite value; a result
    that changes from run to run is reported as such and not as a fill finding; a wrong result fails its bar."""
    def bar(out, ref):
        assert torch.equal(out, ref), 'bar'
    assert independent(_toy(6), bar) == set()
    with pytest.raises(AssertionError, match='DEPENDS ON STALE MEMORY.*1 of 6 elements differ.*within \\[5\\] .. \\[5\\]'):
        independent(_toy(5), bar)
    with pytest.raises(AssertionError, match="DEPENDS ON STALE MEMORY \\(the 'nan' fill"):
        independent(_toy(5, lambda y: torch.fmin(y, torch.tensor(4.0))), bar)
    with pytest.raises(AssertionError, match="DEPENDS ON STALE MEMORY \\(the 'big' fill"):
        independent(_toy(5, lambda y: torch.relu(torch.nan_to_num(y, nan=0.0))), bar)            # NaN -> 0 = the zero fill: only 'big' shows it
    count = [0]

    def drifting():
        call, ref = _toy(6)()

        def again():
            count[0] += 1
            return call() + count[0]
        return again, ref
    with pytest.raises(AssertionError, match='NOT REPRODUCIBLE'):
        independent(drifting, bar)
    with pytest.raises(AssertionError, match='bar'):
        independent(_toy(6, lambda y: y + 1), bar)
    with pytest.raises(AssertionError, match='NOT_REPRODUCIBLE'):
        independent(_toy(6), bar, reproducible=False, case='toy')


@gpu
def test_the_fill_and_the_judge_on_the_device():
    """The patterns of tests/alloc_fill.py on device memory (channels_last halves, float32, float64, the integer families), on the current
    stream, and the judge catching an element a device-side stand-in leaves unwritten."""
    for pattern, half, single, double, byte, wide in (('zero', 0.0, 0.0, 0.0, 0, 0), ('nan', None, None, None, 0xFF, 1),
                                                      ('big', 61280.0, 1.3e36, 6.5e286, 0x7B, 2)):
        with filled(pattern) as rec:
            h = torch.empty((2, 8, 3, 5), dtype=torch.float16, device=DEV, memory_format=torch.channels_last)
            f, d = torch.empty(7, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
            b, i = torch.empty(5, dtype=torch.uint8, device=DEV), h.new_empty((2, 2), dtype=torch.int32)
            like = torch.empty_like(h)
        assert rec.count == 6 and h.is_contiguous(memory_format=torch.channels_last) and like.stride() == h.stride()
        for t, want in ((h, half), (like, half), (f, single), (d, double)):
            if want is None:
                assert bool(torch.isnan(t).all()), (pattern, t.dtype)
            else:
                assert bool((t == t.reshape(-1)[0]).all()) and abs(float(t.reshape(-1)[0]) - want) <= 0.02 * want, (pattern, t.dtype, float(t.reshape(-1)[0]))
        assert bool((b == byte).all()) and bool((i == wide).all()), pattern
    bar = lambda out, ref: _assert(torch.equal(out, ref), 'bar')            # noqa: E731
    independent(_toy(6, device=DEV), bar)
    with pytest.raises(AssertionError, match='DEPENDS ON STALE MEMORY.*1 of 6 elements differ'):
        independent(_toy(5, device=DEV), bar)
    with pytest.raises(AssertionError, match="DEPENDS ON STALE MEMORY \\(the 'nan' fill"):
        independent(_toy(5, lambda y: torch.fmin(y, torch.tensor(4.0, device=DEV)), device=DEV), bar)


def test_the_not_reproducible_list_quotes_the_kernel_source():
    for case, (src, line, text) in NOT_REPRODUCIBLE.items():
        with open(os.path.join(PACKAGE_DIR, 'csrc', src)) as f:
            got = f.read().split('\n')[line - 1]
        assert text in got and 'atomic' in got, (case, src, line, got)


# ------------------------------------------------------------------------------------------------
# a. the three route tables, whole
# ------------------------------------------------------------------------------------------------

import test_gpu_dense_routes as RD      # noqa: E402
import test_gpu_routes_fp16 as R16      # noqa: E402
import test_gpu_routes_fp32 as R32      # noqa: E402


@gpu
@pytest.mark.parametrize('case', sorted(R32.CASES))
def test_fp32_route(case):
    kk = R32._kk()
    builder, _, _, switches = R32.CASES[case]

    def make():
        call, ref, tol = builder()
        return call, (ref, tol)

    def bars(got, ctx):
        ref, tol = ctx
        got = R32._flat(got).detach().double().cpu()
        assert tuple(got.shape) == tuple(ref.shape), (case, tuple(got.shape), tuple(ref.shape))
        e = rel_err(got.numpy(), ref.numpy())
        print(f'FILL fp32 {case} rel_err={e:.3e}')
        if tol == 0.0:
            assert torch.equal(got, ref), f'{case}: not bit-exact (rel err {e:.3e})'
        else:
            assert e < tol, f'{case}: rel err {e:.3e} >= {tol:.0e}'

    old = {k: getattr(kk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(kk, k, v)
        sites = independent(make, bars)
    finally:
        for k, v in old.items():
            setattr(kk, k, v)
    _finish(f'fp32:{case}', sites)


@gpu
@pytest.mark.parametrize('case', sorted(R16.CASES))
def test_fp16_route(case):
    builder, _, _, switches = R16.CASES[case]
    lib = R16._lib()

    def bars(got, judge):
        records = judge(got)
        print(f'FILL fp16 {case} ' + ' '.join(f'{label}: {v:.3e} (bar {bar:.0e})' for label, v, bar, _ in records))
        for label, v, bar, strict in records:
            assert (v < bar) if strict else (v <= bar), f'{case}: {label} {v:.3e} exceeds {bar:.0e}'

    old = lib.shg_conv2d_f16_set_routes(switches['routes']) if 'routes' in switches else None
    try:
        # (the relayout cases cast values beyond the half range on purpose: +-inf where torch's cast gives it, compared bit for bit)
        sites = independent(builder, bars, finite=not case.startswith('relayout_'))
    finally:
        if old is not None:
            lib.shg_conv2d_f16_set_routes(old)
    _finish(f'fp16:{case}', sites)


@gpu
@pytest.mark.parametrize('case', sorted(RD.CASES))
def test_dense_route(case):
    builder = RD.CASES[case][0]

    def bars(got, judge):
        recs = judge()
        print(f'FILL dense {case} ' + ' '.join(f'{nm}={e:.2e}/{b:.0e}' for nm, e, b in recs))
        for nm, e, b in recs:
            assert e <= b, f'{case}: {nm}: {e:.3e} exceeds {b:.0e}'

    _finish(f'dense:{case}', independent(builder, bars))


# ------------------------------------------------------------------------------------------------
# b. the fuzz families: the first 6 seeds of each
# ------------------------------------------------------------------------------------------------
import fuzz_cases  # noqa: E402

FUZZ_SEEDS = 6


@gpu
@pytest.mark.parametrize('family,seed', [(f, s0 + k) for f, (_, s0, _) in fuzz_cases.FAMILIES.items() for k in range(FUZZ_SEEDS)])
def test_fuzz_family(family, seed):
    fn = fuzz_cases.FAMILIES[family][0]
    results, sites = [], set()
    for pattern in ORDER:
        _reset_caches()
        with filled(pattern) as rec:
            results.append(fn(seed))
            torch.cuda.synchronize()
        sites |= rec.sites
    assert results[0] == results[1], (f'NOT REPRODUCIBLE: {family} seed {seed} gives other errors in a second run under the same zero fill: '
                                      f'{[(a, b) for a, b in zip(results[0], results[1]) if a != b]}')
    for k, pattern in ((2, 'nan'), (3, 'big')):
        assert results[k] == results[0], (f'DEPENDS ON STALE MEMORY: {family} seed {seed} under the {pattern!r} fill: '
                                          f'{[(a, b) for a, b in zip(results[0], results[k]) if a != b]}')
    bad = [f'{what}: {desc}: {e:.3e} (bound {b:.0e})' for res in results for what, e, b, desc in res if not e < b]
    assert not bad, f'{family} seed {seed}: ' + '; '.join(bad)
    _finish(f'fuzz:{family}', sites)


# ------------------------------------------------------------------------------------------------
# c. entry points outside the tables.  Each builder returns (call, check): ``call()`` -> the results, ``check(out)`` asserts the bar of the
# entry point's existing test against its reference.  Float64 references are computed once (``_once``) and shared by the four runs.
# ------------------------------------------------------------------------------------------------
_REFS = {}


def _once(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def _mods():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels, kernels_f16
    from oracle import shgan_oracle as orc
    return kernels, kernels_f16, orc


def _rnd(seed, *shape, lo=None):
    rs = np.random.RandomState(seed)
    a = rs.rand(*shape) + lo if lo is not None else rs.standard_normal(shape)
    return torch.from_numpy(a.astype(np.float32))


def _rel(got, want):
    return rel_err(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy() if torch.is_tensor(want) else want)


N, C, H, W = 2, 5, 6, 12          # the shape of the single-kernel entry points: HW % 4 == 0, nothing else a multiple of a tile
TOL_PW = R32.TOL_PW               # elementwise passes (tests/test_gpu_routes_fp32.py)


# ---- the NOT_ROUTED kernels of tests/test_gpu_routes_fp32.py

def planes_to_image_case():
    """The four phase planes [4, N, C, H+1, W+1] of a transposed convolution interleaved, rows / columns [1, 1 + 2H) + bias; a second call
    asks for one row and one column more than the (2H+1) x (2W+1) result has: zero (+ bias) there."""
    kk, _, _ = _mods()
    mid, b = _rnd(1, 4, N, C, H + 1, W + 1), _rnd(2, C)
    full = torch.zeros(N, C, 2 * H + 3, 2 * W + 3, dtype=torch.float64)
    for a in range(2):
        for c in range(2):
            full[:, :, a:2 * H + 1:2, c:2 * W + 1:2] = mid[a * 2 + c][:, :, :H + 1 - a, :W + 1 - c].double()
    want = [full[:, :, 1:1 + 2 * H, 1:1 + 2 * W] + b.double().view(1, C, 1, 1), full[:, :, 0:2 * H + 2, 0:2 * W + 2]]
    md, bd = mid.to(DEV), b.to(DEV)

    def check(out):
        for got, ref in zip(out, want):
            assert tuple(got.shape) == tuple(ref.shape) and _rel(got, ref) < TOL_PW
    return (lambda: [kk.planes_to_image(md, 1, 2 * H, 2 * W, bias=bd), kk.planes_to_image(md, 0, 2 * H + 2, 2 * W + 2)]), check


def modtail_backward_f32_case():
    """All four results, then sums alone and the noise gradient alone (``part`` and ``gnoise`` exist only when asked for); the reference and
    the 2e-5 bound are those of the round5 fuzz family."""
    kk, _, _ = _mods()
    gy, y, t, u = (_rnd(3 + k, N, C, H, W) for k in range(4))
    d, e = _rnd(7, N, C, lo=0.5), _rnd(8, N, C)
    yd = y.double()
    slope = torch.where(yd.abs() >= 1.5, torch.zeros_like(yd), torch.where(yd > 0, torch.full_like(yd, 2 ** 0.5), torch.full_like(yd, 0.2 * 2 ** 0.5)))
    gz = gy.double() * slope
    gt = gz * d.double().view(N, C, 1, 1) + u.double() * slope * e.double().view(N, C, 1, 1)
    s1, s0, gn = (gz * t.double()).sum([2, 3]), gz.sum([2, 3]), gz.sum(1, keepdim=True)
    a = [v.to(DEV) for v in (gy, y, t, d)]
    ud, ed = u.to(DEV), e.to(DEV)

    def call():
        kw = dict(act=True, gain=1.0, clamp=1.5, u=ud, e=ed)
        return [kk.modtail_backward(*a, want_sums=True, want_noise=True, **kw), kk.modtail_backward(*a, want_sums=True, want_noise=False, **kw),
                kk.modtail_backward(*a, want_sums=False, want_noise=True, **kw)]

    def check(out):
        for k, (ggt, gs1, gs0, ggn) in enumerate(out):
            assert _rel(ggt, gt) < 2e-5
            assert (gs1 is None) == (k == 2) and (ggn is None) == (k == 1)
            if gs1 is not None:
                assert _rel(gs1, s1) < 2e-5 and _rel(gs0, s0) < 2e-5
            if ggn is not None:
                assert tuple(ggn.shape) == (N, 1, H, W) and _rel(ggn, gn) < 2e-5
    return call, check


def sum_partials_case():
    kk, _, _ = _mods()
    part = _rnd(9, N, 7, 2, C)
    pd = part.to(DEV)
    return (lambda: kk.sum_partials(pd)), (lambda got: _assert(tuple(got.shape) == (N, 2, C) and _rel(got, part.double().sum(1)) < TOL_PW))


def _assert(ok, msg=''):
    assert ok, msg


def scale_channels_case():
    kk, _, _ = _mods()
    x, s = _rnd(10, N, C, H, W), _rnd(11, N * C, lo=0.5)
    xd, sd = x.to(DEV), s.to(DEV)
    return (lambda: kk.scale_channels(xd, sd)), (lambda got: _assert(torch.equal(got.cpu(), x * s.view(N, C, 1, 1)), 'one rounding: exact'))


def scale_cast_case():
    """half(x * gain) and float(h) * gain.  The product is one float32 rounding (2^-24 relative), the cast to half one more (2^-11 relative,
    2^-25 absolute among the denormals): the per-element bar of the fp16 route table, 2^-10 |ref| + 2^-24; the way back is one float32
    rounding of an exact product: the elementwise bar 1e-5."""
    kk, _, _ = _mods()
    x = _rnd(12, N, C, H, W) * 30
    h = x.half()
    xd, hd = x.to(DEV), h.to(DEV)

    def check(out):
        to_h, to_f = out
        assert to_h.dtype == torch.float16 and to_f.dtype == torch.float32 and to_h.is_contiguous() and to_f.is_contiguous()
        ref = x.double() * 0.37
        assert float(((to_h.double().cpu() - ref).abs() / (ref.abs() * 2.0 ** -10 + 2.0 ** -24)).max()) <= 1.0
        assert _rel(to_f, h.double() * 1.7) < TOL_PW
    return (lambda: [kk.scale_cast(xd, 0.37, True), kk.scale_cast(hd, 1.7, False)]), check


def composite_u8_case():
    kk, _, orc = _mods()
    rs = np.random.RandomState(13)
    mask = torch.from_numpy((rs.rand(N, 1, H, W) < 0.6).astype(np.float32))
    real = torch.from_numpy(rs.randint(0, 256, (N, 3, H, W)).astype(np.float32)) / 127.5 - 1.0
    x = torch.cat([mask - 0.5, real * mask], dim=1)
    img = torch.from_numpy((rs.standard_normal((N, 3, H, W)) * 0.7).astype(np.float32))
    want = orc.composite_u8(x, img)
    xd, imd = x.to(DEV), img.to(DEV)
    return (lambda: kk.composite_u8(xd, imd)), (lambda got: _assert(got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want.numpy())))


def assemble_input_case():
    kk, _, _ = _mods()
    rs = np.random.RandomState(14)
    real = torch.from_numpy(rs.uniform(-1, 1, (N, 3, H, W)).astype(np.float32))
    u8 = torch.from_numpy(rs.randint(0, 256, (N, 3, H, W)).astype(np.uint8))
    mask = torch.from_numpy((rs.rand(N, 1, H, W) < 0.6).astype(np.float32))
    want = [torch.cat([mask - 0.5, real * mask], dim=1), torch.cat([mask - 0.5, kk.u8_value_table('cpu')[u8.long()] * mask], dim=1)]
    rd, ud, md = real.to(DEV), u8.to(DEV), mask.to(DEV)

    def check(out):
        for got, ref in zip(out, want):
            assert torch.equal(got.cpu(), ref)                        # the same float32 operations as torch: bit-identical
    return (lambda: [kk.assemble_input(rd, md), kk.assemble_input(ud, md)]), check


def fma_case():
    """The public op forward and backward: fma_bcast, then mul_reduce over the broadcast dimensions of b and c (bars of test_gpu_r6_ops.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd.model_zoo.stylegan_utils import fma as fma_mod
    ops = [_rnd(15, N, C, H, W), _rnd(16, N, C, 1, 1), _rnd(17, N, 1, H, W)]
    go = _rnd(18, N, C, H, W)
    with torch.enable_grad():
        r = [t.double().requires_grad_(True) for t in ops]
        ref = r[0] * r[1] + r[2]
        rg = torch.autograd.grad(ref, r, go.double())

    def call():
        with torch.enable_grad():
            d = [t.to(DEV).requires_grad_(True) for t in ops]
            y = fma_mod.fma(*d)
            return [y.detach()] + list(torch.autograd.grad(y, d, go.to(DEV)))

    def check(out):
        assert _rel(out[0], ref.detach()) < 1e-6
        for got, want in zip(out[1:], rg):
            assert got.shape == want.shape and _rel(got, want) < 2e-6
    return call, check


# ---- the Spectral Hint Unit

def _shu_setup(cid):
    from test_shu_geometry_cpu import build_case
    shu, g, (n, ch, size, lowest, seed) = build_case(cid)
    x = np.random.RandomState(seed).standard_normal((n, ch, size, size)).astype(np.float32)
    keep = [int(v) for v in g[f'{cid}__channels']]
    return shu.to(DEV).eval().requires_grad_(False), g, x, keep


def shu_forward_case(cid):
    """Case A (fused spectral stage, partial last tile) / C (unfused, one level) of tests/test_gpu_shu_geometry.py against the reference's
    hints, 1e-4."""
    def make():
        shu, g, x, keep = _shu_setup(cid)
        xd = torch.from_numpy(x).to(DEV)

        def check(out):
            assert sorted(out) == shu.reslist
            for r in shu.reslist:
                got = out[r].cpu().numpy()
                e = rel_err(got[:, keep] if r >= 64 else got, g[f'{cid}__y{r}'])
                assert e < 1e-4, (cid, r, e)
        return (lambda: shu(xd)), check
    return make


def shu_training_case():
    """The training route of case C: hints (2e-5) and the four gradients (5e-5) against float64 torch.fft (test_gpu_shu_geometry.py)."""
    import test_gpu_shu_geometry as TS
    shu, g, x, keep = _shu_setup('C')
    ws = {r: np.random.RandomState(77).standard_normal(tuple(x.shape[:2]) + (r, r)) for r in shu.reslist}

    def reference():
        with torch.enable_grad():
            xr, pr, gauss, cw = TS.f64_setup(shu, x.astype(np.float64))
            ref = TS.fft_form(shu, xr, pr, gauss, cw)
            gref = torch.autograd.grad(sum((ref[r] * torch.tensor(ws[r])).sum() for r in shu.reslist), [xr] + pr)
        return {r: v.detach() for r, v in ref.items()}, [v.detach() for v in gref]
    ref, gref = _once('shu_training_C', reference)

    def call():
        with torch.enable_grad():
            shu.requires_grad_(True)
            try:
                xg = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
                got = shu(xg)
                loss = sum((got[r] * torch.tensor(ws[r], dtype=torch.float32, device=DEV)).sum() for r in shu.reslist)
                grads = torch.autograd.grad(loss, [xg, shu.conv0.weight, shu.conv0.bias, shu.df1.weight])
            finally:
                shu.requires_grad_(False)
        return [{r: v.detach() for r, v in got.items()}, list(grads)]

    def check(out):
        got, grads = out
        for r in shu.reslist:
            assert _rel(got[r], ref[r]) < 2e-5, r
        for name, a, b in zip(('x', 'conv0.weight', 'conv0.bias', 'df1.weight'), grads, gref):
            assert _rel(a, b) < 5e-5, name
    return call, check


# ---- Inception-v3 (the FID detector)

def _inc_sd():
    import inception_f64
    return _once('inc_sd', lambda: inception_f64.random_state_dict(7))


def inception_convs_case():
    """Every distinct convolution geometry of the network at B = 1, from a channel slice of a wider input into a channel slice of a wider
    buffer (tests/test_gpu_inception.py, 1e-5); the launch plan splits K where the grid is small: its workspace is an allocation."""
    import shgan_amd  # noqa: F401
    from shgan_amd import inception
    import test_gpu_inception as TI
    g = torch.Generator().manual_seed(1)
    items = []
    for name, i, o, k, s, p, h in TI._geometries():
        w = (torch.randn(o, i, *k, generator=g, dtype=torch.float64) * np.sqrt(2.0 / (i * k[0] * k[1]))).float()
        b = (torch.randn(o, generator=g, dtype=torch.float64) * 0.1).float()
        x = torch.randn(1, i + 5, h, h, generator=g).float()
        want = _once(('inc_conv', name), lambda: F.relu(F.conv2d(x[:, 3:3 + i].double(), w.double(), b.double(), stride=s, padding=p)))
        items.append((name, i, o, k, s, p, h, w, b, x.to(DEV), want))

    def call():
        outs = []
        for name, i, o, k, s, p, h, w, b, xd, _ in items:
            wp, bp = inception.pack_weight(w.to(DEV), b.to(DEV))
            op = inception.ConvOp(name, wp, bp, i, o, k, s, p)
            oh, ow = inception.out_size(h, k[0], s[0], p[0]), inception.out_size(h, k[1], s[1], p[1])
            y = torch.full((1, o + 24, oh, ow), 7.0, device=DEV)
            inception.conv_group([(op, xd, 3, y, 17)])
            outs.append(y)
        return outs

    def check(outs):
        for y, (name, i, o, *_, want) in zip(outs, items):
            got = y.cpu()
            assert torch.all(got[:, :17] == 7.0) and torch.all(got[:, 17 + o:] == 7.0), name
            assert TI._rel(got[:, 17:17 + o], want) <= 1e-5, name
    return call, check


def inception_grouped_splitk_case():
    """Four 1 x 1 branches over K = 1280 in one grouped launch with the split-K plan: the groups split differently (1e-5 against float64)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import inception
    import test_gpu_inception as TI
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1280, 8, 8, generator=g)
    ws = [torch.randn(o, 1280, 1, 1, generator=g) * 0.04 for o in (320, 384, 448, 192)]
    want = _once('inc_grouped', lambda: F.relu(F.conv2d(x.double(), torch.cat(ws).double())))
    xd = x.to(DEV)

    def call():
        ops = []
        for k, w in enumerate(ws):
            wp, bp = inception.pack_weight(w.to(DEV), torch.zeros(w.shape[0], device=DEV))
            ops.append(inception.ConvOp('abcd'[k], wp, bp, 1280, w.shape[0], (1, 1), (1, 1), (0, 0)))
        out = torch.full((2, 1344, 8, 8), 7.0, device=DEV)
        items, off = [], 0
        for op in ops:
            items.append((op, xd, 0, out, off))
            off += op.O
        inception.conv_group(items, split_k=True)
        return out
    return call, (lambda out: _assert(TI._rel(out, want) <= 1e-5))


def inception_pools_case():
    """The 3 x 3 stride-2 max pool of 288 channels at 35 x 35 written at channel offset 480 of a wider buffer (bit-exact), the same pool
    into a buffer of its own, and the average pool of the A blocks (1e-6)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import inception
    x = torch.randn(1, 288, 35, 35, generator=torch.Generator().manual_seed(289))
    xd = x.to(DEV)

    def call():
        y = torch.full((1, 288 + 480 + 8, 17, 17), 5.0, device=DEV)
        inception.pool(xd, 'max', 2, 0, y=y, y_coff=480)
        return [y, inception.pool(xd, 'max', 2, 0), inception.pool(xd, 'avg', 1, 1)]

    def check(out):
        wide, own, avg = (t.cpu() for t in out)
        assert torch.all(wide[:, :480] == 5.0) and torch.all(wide[:, 480 + 288:] == 5.0)
        assert torch.equal(wide[:, 480:480 + 288], F.max_pool2d(x, 3, 2, 0)) and torch.equal(own, F.max_pool2d(x, 3, 2, 0))
        assert _rel(avg, F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)) <= 1e-6
    return call, check


def inception_frontend_mean_head_case():
    """The (200, 300) front end on uint8 pixels and on [-1, 1] floats (1e-6), the global mean (1e-6), the classifier head (the rule of
    tests/test_gpu_kid_is.py: 4 x the distance of torch's CPU float32 from float64, at most 1e-3)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import inception
    import inception_f64
    import kid_is_f64
    import test_gpu_kid_is as TK
    g = torch.Generator().manual_seed(200 * 7 + 300)
    u8 = torch.randint(0, 256, (2, 3, 200, 300), generator=g, dtype=torch.uint8)
    pm1 = torch.rand(2, 3, 200, 300, generator=g) * 2 - 1
    xm = torch.rand(3, 2048, 8, 8, generator=torch.Generator().manual_seed(2))
    feats, w, b = TK._head_inputs(5, 1000, 1005)
    want = _once('inc_front', lambda: [inception_f64.frontend_f64(u8, '0_255'), inception_f64.frontend_f64(pm1, 'pm1')])
    head = _once('inc_head', lambda: kid_is_f64.softmax_head_f64(feats.numpy(), w.numpy(), b.numpy()))
    d = [t.to(DEV) for t in (u8, pm1, xm, feats, w, b)]

    def check(out):
        f0, f1, mean, probs = out
        assert f0.shape == (2, 3, 299, 299) and _rel(f0, want[0]) <= 1e-6 and _rel(f1, want[1]) <= 1e-6
        assert _rel(mean, xm.double().mean(dim=(2, 3))) <= 1e-6
        top = head.max(axis=1, keepdims=True)
        cpu = torch.softmax(F.linear(feats, w, b), dim=1).numpy().astype(np.float64)
        d_torch = float(np.max(np.abs(cpu - head) / top))
        d_kernel = float(np.max(np.abs(probs.cpu().numpy().astype(np.float64) - head) / top))
        assert d_kernel <= min(4 * d_torch, 1e-3), (d_kernel, d_torch)
    return (lambda: [inception.frontend(d[0], '0_255'), inception.frontend(d[1], 'pm1'), inception.global_mean(d[2]),
                     inception.head_probs(d[3], d[4], d[5])]), check


def inception_detector_case():
    """One pass of the whole detector (the concat buffers of the Mixed blocks) on one 128 x 128 image, weights packed under the fill:
    1e-4 against the float64 model (test_fid_stats_add_images_takes_the_detector)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import inception
    import inception_f64
    import test_gpu_inception as TI
    sd = _inc_sd()
    img = torch.randint(0, 256, (1, 3, 128, 128), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    want = _once('inc_det', lambda: inception_f64.detector_f64(sd, img.float()))
    det = inception.InceptionFeatures.from_state_dict(sd, device=DEV)
    imd = img.to(DEV)
    return (lambda: det(imd, return_features=True)), (lambda got: _assert(got.shape == (1, 2048) and TI._rel(got, want) <= 1e-4))


# ---- VGG16 (precision / recall) and LPIPS

def vgg16_case():
    """Front end at 160 x 288 on [-1, 1] floats and at 256 on uint8, maxpool2 at (1, 3, 7, 10) (bit-exact), one detector pass at
    (1, 224, 224): 1e-5 of each image's largest value (tests/test_gpu_pr.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import vgg16
    import pr_f64
    import test_gpu_pr as TP
    mean, std = (123.68, 116.779, 103.939), (58.4, 57.1, 57.4)
    sd = _once('vgg_sd', lambda: pr_f64.random_state_dict(3))
    a, b, img = TP._images(2, 160, 288, 160, pm1=True), TP._images(2, 256, 256, 256), TP._images(1, 224, 224, 11 + 1 + 224)
    xp = torch.randn((1, 3, 7, 10), generator=torch.Generator().manual_seed(7))
    want = _once('vgg', lambda: [pr_f64.frontend_f64(a, 'pm1', mean, std), pr_f64.frontend_f64(b, None, mean, std), pr_f64.features_f64(sd, img, None)])
    det = vgg16.Vgg16Features.from_state_dict(sd, device=DEV)
    d = [t.to(DEV) for t in (a, b, xp, img)]

    def check(out):
        fa, fb, mp, feats = out
        assert TP._rel_per_image(fa, want[0]) <= TP.BOUND and TP._rel_per_image(fb, want[1]) <= TP.BOUND
        assert torch.equal(mp.cpu(), F.max_pool2d(xp, 2))
        assert feats.shape == (1, 128) and TP._rel_per_image(feats, want[2]) <= TP.BOUND
    return (lambda: [vgg16.frontend(d[0], 'pm1', mean, std), vgg16.frontend(d[1], None, mean, std), vgg16.maxpool2(d[2]), det(d[3])]), check


def lpips_case():
    """The per-image distance at (200, 300) x 2, a uint8 composite against a float32 real: 1e-5 relative per image; the first convolution
    alone at 7 x 7, into a buffer of its own: 1e-5 of the largest output (tests/test_gpu_lpips.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import lpips
    import lpips_f64
    sd = _once('lpips_sd', lambda: lpips_f64.random_state_dict(11))
    pred_u8, real_u8 = lpips_f64.image_pairs(2, 200, 300, seed=202)
    real = real_u8.to(torch.float32).div(255) * 2 - 1
    want = _once('lpips', lambda: lpips_f64.lpips_f64(sd, pred_u8, real))
    u8 = torch.randint(0, 256, (2, 3, 7, 7), generator=torch.Generator().manual_seed(42), dtype=torch.uint8)
    c1 = _once('lpips_conv1', lambda: lpips_f64.conv1_f64(sd, lpips_f64.pred_values_f32(u8)))
    net = lpips.Lpips.from_state_dict(sd, device=DEV)
    pd, rd, ud = pred_u8.to(DEV), real.to(DEV), u8.to(DEV)

    def check(out):
        got, conv = out
        assert got.shape == (2,) and got.dtype == torch.float64 and float(want.min()) > 0
        assert float(((got.cpu() - want).abs() / want).max()) <= 1e-5
        assert conv.shape == c1.shape == (2, 64, 1, 1) and _rel(conv, c1) <= 1e-5
    return (lambda: [net(pd, rd), lpips.conv1(ud, *net.conv1_wb, 'pred', 'pm1')]), check


def lpips_vgg_case():
    """``LPIPS(net='vgg')`` at 40 x 56 (odd after the pools), a uint8 composite against a float32 real: 2 x E32 + 2^-22 relative, at least
    7e-8, E32 the distance of the float32 restatement from the float64 one on this case (tests/test_gpu_ppl.py); and the scaling layer alone."""
    import shgan_amd  # noqa: F401
    from shgan_amd import lpips
    import lpips_f64
    import ppl_f64
    sd = _once('lpips_vgg_sd', lambda: ppl_f64.vgg_random_state_dict(ppl_f64.NARROW, seed=3))
    pred_u8, real_u8 = lpips_f64.image_pairs(2, 40, 56, seed=40 + 56 + 2)
    real = real_u8.to(torch.float32).div(255) * 2 - 1
    want, w32 = _once('lpips_vgg', lambda: (ppl_f64.lpips_vgg(sd, pred_u8, real), ppl_f64.lpips_vgg(sd, pred_u8, real, dtype=torch.float32).to(torch.float64)))
    sc = _once('lpips_scaling', lambda: lpips_f64.scaling_f64(lpips_f64.pred_values_f32(pred_u8)))
    net = lpips.LPIPS(net='vgg', state_dict=sd, device=DEV)
    pd, rd = pred_u8.to(DEV), real.to(DEV)

    def check(out):
        got, scaled = out
        bound = torch.clamp(2 * (w32 - want).abs() / want + 2.0 ** -22, min=7e-8)
        assert got.shape == (2,) and bool((((got.cpu() - want).abs() / want) <= bound).all())
        # the scaling layer into a buffer of its own: (v - shift) / scale on float32 values, two float32 roundings, 2^-22 of the largest value
        assert tuple(scaled.shape) == (2, 3, 40, 56) and _rel(scaled, sc) <= 2.0 ** -22
    return (lambda: [net(pd, rd), lpips.scaling(pd, 'pred', 'pm1')]), check


# ---- metrics

def image_metrics_case():
    """PSNR / SSIM at B = 3, 37 x 53, window 11, uint8 against float and float against uint8 (tests/test_gpu_image_metrics.py: 1e-5, 2e-5)."""
    import shgan_amd  # noqa: F401
    from shgan_amd.image_metrics import MetricsAccumulator, image_metrics
    import test_gpu_image_metrics as TM
    pairs = [TM._pair((3, 3, 37, 53), 1, True, False), TM._pair((3, 1, 37, 53), 2, False, True)]
    want = _once('metrics', lambda: [TM.reference_metrics_f64(p, g, 11) for p, g in pairs])
    dev = [(p.to(DEV), g.to(DEV)) for p, g in pairs]

    def call():
        acc = MetricsAccumulator(5, DEV, metrics=('ssim',), window_size=11)          # SSIM alone: the PSNR of the pass goes to a throw-away buffer
        acc.add(dev[0][0], dev[0][1], 1)
        return [image_metrics(p, g, window_size=11) for p, g in dev] + [acc.values['ssim'][1:4]]

    def check(out):
        for (psnr, ssim), (p_ref, s_ref) in zip(out[:2], want):
            assert float((psnr.cpu() - p_ref).abs().max()) <= TM.PSNR_TOL and float((ssim.cpu() - s_ref).abs().max()) <= TM.SSIM_TOL
        assert float((out[2].cpu() - want[0][1]).abs().max()) <= TM.SSIM_TOL
    return call, check


def kid_is_fid_case():
    """KID sums with a ragged last tile (1e-11), the Inception Score accumulator over batches of 5 and 16 (1e-12), the FID moments over
    batches of 5 and 33 rows at D = 2048 (1e-12 of the largest moment): the bars of tests/test_gpu_kid_is.py and tests/test_fid_stats.py."""
    import shgan_amd  # noqa: F401
    from shgan_amd import fid_stats, inception_score as isc, kid
    import kid_is_f64
    import test_gpu_kid_is as TK
    n_f, n_r, m, S, D = 70, 90, 37, 3, 64
    fake, real = TK._features(n_f, D, 1, torch.float32), TK._features(n_r, D, 2, torch.float32)
    idx_f, idx_r, _ = kid.kid_subsets(n_f, n_r, S, m, seed=4)
    Cn, Sn = 1000, 3
    probs = TK._probs(21, Cn, Cn)
    splits = np.full(21, -1, np.int32)
    keep = [i for i in range(21) if i not in (3, 12)]
    splits[keep] = [isc.split_of(j, 19, Sn) for j in range(19)]
    rs = np.random.RandomState(7)
    batches = [((rs.standard_normal((b, 2048)) * rs.rand(2048) + rs.rand(2048)).astype(np.float32), (rs.rand(b) < 0.8).astype(np.float32)) for b in (5, 33)]

    def moments():
        S_ = np.zeros((2049, 2049))
        for x, w in batches:
            xa = np.concatenate([x.astype(np.float64), np.ones((len(x), 1))], axis=1)
            S_ += (xa * w[:, None].astype(np.float64)).T @ xa
        return S_
    want = _once('kid_is_fid', lambda: [kid_is_f64.kid_sums_f64(fake.numpy(), real.numpy(), idx_f, idx_r),
                                       kid_is_f64.is_accumulator_f64(probs.numpy(), splits, Sn), moments()])
    fd, rd, tf, tr = fake.to(DEV), real.to(DEV), torch.from_numpy(idx_f).to(DEV), torch.from_numpy(idx_r).to(DEV)
    pd, td = probs.to(DEV), torch.from_numpy(splits).to(DEV)
    bd = [(torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)) for x, w in batches]

    def call():
        acc = isc.new_accumulator(Sn, Cn, DEV)
        isc.is_accumulate(acc, pd[:5], td[:5])
        isc.is_accumulate(acc, pd[5:], td[5:])
        st = fid_stats.FidStats(2048, DEV)
        for x, w in bd:
            st.add(x, w)
        return [kid.kid_sums(fd, rd, tf, tr), acc, st.S]

    def check(out):
        sums, acc, S_ = (t.cpu().numpy() for t in out)
        assert TK._rel(sums, want[0]) <= 1e-11
        assert np.array_equal(acc[:, Cn + 1], want[1][:, Cn + 1]) and TK._rel(acc[:, :Cn + 1], want[1][:, :Cn + 1]) <= 1e-12
        got = S_[:2049, :2049]
        got = np.triu(got) + np.triu(got, 1).T
        assert np.abs(got - want[2]).max() <= 1e-12 * np.abs(want[2]).max()
    return call, check


def precision_recall_case():
    """radii and inside at (129, 65) with k = 3 on the exact integer data (bit for bit), and at (150, 90, D = 72) against the float64
    radii (1e-3) and the bracketing flags (tests/test_gpu_pr.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import precision_recall as prm
    import test_gpu_pr as TP
    k = 3
    man, probes = torch.from_numpy(TP._ints(129, 10 + 129)).to(DEV), torch.from_numpy(TP._ints(65, 20 + 65)).to(DEV)
    want_r, want_in, _, _ = TP._exact_ref(129, 65, k)
    a, b = TP._general(150, 72, 1), TP._general(90, 72, 2)
    gen_r, must, may, gen_in = TP._general_ref(150, 90, 72, k)['fwd']
    ad, bd = a.to(DEV), b.to(DEV)

    def call():
        r = prm.radii(man, k)
        gr = prm.radii(ad, k)
        return [r, prm.inside(probes, man, r), gr, prm.inside(bd, ad, gr)]

    def check(out):
        r, flags, gr, gflags = out
        assert r.dtype == torch.float16 and np.array_equal(r.cpu().numpy().view(np.uint16), want_r.view(np.uint16))
        assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), want_in)
        got_r, gf = gr.cpu().numpy().astype(np.float64), gflags.cpu().numpy()
        assert float(np.max(np.abs(got_r - gen_r) / gen_r)) <= 1e-3
        share = int((may & ~must).sum()) / len(b)
        assert share <= TP.OPEN_CAP and np.all(gf[must]) and np.all(may[gf]) and abs(float(gf.mean()) - float(gen_in.mean())) <= min(share, TP.OPEN_CAP)
    return call, check


# ---- input paths: the PPL front end, the two resizes, the random-scale crop

def ppl_frontend_case():
    """A copy (factor 0), and factor 3 with the grey repeat (no float4 form), against the float32 chain on the float64 box mean within
    one ulp of the mean (tests/test_gpu_ppl.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import ppl
    import test_gpu_ppl as TL
    cases = [((2, 3, 64, 64), 0, False), ((1, 1, 72, 72), 3, False)]
    xs = [TL._image(shape, shape[2] + factor) for shape, factor, _ in cases]
    xd = [x.to(DEV) for x in xs]

    def check(out):
        for got, x, (shape, factor, crop) in zip(out, xs, cases):
            exact, ok = TL._check_frontend(got, x, factor, crop, TL.MEAN, TL.STD)
            assert bool(ok.all()) and (factor > 1 or bool(exact.all()))
    return (lambda: [ppl.frontend(x, factor, crop, TL.MEAN, TL.STD) for x, (_, factor, crop) in zip(xd, cases)]), check


def resize_case():
    """The Pillow-exact bicubic resize (ragged batch of three to 37 x 37) and the aspect-fit-and-pad path (to 64 x 64), flips mixed, byte for
    byte against Pillow (tests/test_gpu_resize.py, tests/test_gpu_openimages.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import resize as rz
    import test_gpu_openimages as TO
    import test_gpu_resize as TR
    rs = np.random.RandomState(11)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((29, 41), (37, 37), (90, 64))]
    fit = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((64, 64), (21, 33), (192, 5), (70, 100))]
    flip, fflip = np.array([False, True, False]), np.array([True, False, False, True])
    want = _once('resize', lambda: [np.stack([TR._pillow(im, 37, bool(f)) for im, f in zip(imgs, flip)]),
                                    np.stack([TO._pillow_fit(im, 64, bool(f)) for im, f in zip(fit, fflip)])])

    def call():
        p, s = rz.pack_images(imgs)
        q, t = rz.pack_images(fit)
        return [rz.resize_bicubic_u8(p.to(DEV), s, 37, flip=flip), rz.resize_fit_pad_u8(q.to(DEV), t, 64, flip=fflip)]

    def check(out):
        for got, ref in zip(out, want):
            assert np.array_equal(got.cpu().numpy(), ref), int((got.cpu().numpy() != ref).sum())
    return call, check


def randcrop_case():
    """The unaligned ragged batch of tests/test_gpu_randcrop.py (widths 5, 7 and 33) at s = 16, within 2 x E_ref + 2^-22 of the float64 window."""
    import shgan_amd  # noqa: F401
    from shgan_amd import resize as rz
    import randcrop_f64
    import test_gpu_randcrop as TC
    rs = np.random.RandomState(5)
    imgs = [randcrop_f64.synthetic_image(rs, 6, 5), randcrop_f64.synthetic_image(rs, 9, 7), randcrop_f64.synthetic_image(rs, 11, 33)]
    params = [(19, 17, 2, 1, 0, 0), (16, 19, 0, 3, 1, 0), (18, 33, 1, 9, 0, 1)]

    def call():
        packed, shapes = rz.pack_images(imgs)
        return rz.randcrop_bicubic(packed.to(DEV), shapes, 16, np.asarray(params, np.int64).reshape(-1, 6))

    def check(out):
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (3, 3, 16, 16)
        for k in range(3):
            TC._check(f'fill ragged {k}', got[k], imgs[k], 16, params[k])
    return call, check


# ---- masks

def freeform_masks_case():
    """``rasterize`` at s = 32 and s = 64, with and without content boxes, against the CPU rasteriser (oracle/mask_raster_oracle.py), the
    hole counts too (those of the whole mask, before the box fill)."""
    import shgan_amd  # noqa: F401
    from oracle import mask_raster_oracle as mo
    from shgan_amd import masks
    tab = masks.disc_span_table()
    jobs = []
    for s, boxed in ((32, False), (32, True), (64, False), (64, True)):
        np.random.seed(100 + s + boxed)
        recs, offs, flips = [], [0], []
        for _ in range(3):
            r, f0, f1 = masks.mask_attempt_records(s, (0, 1))
            recs.append(r)
            offs.append(offs[-1] + len(r))
            flips.append((int(f0), int(f1)))
        boxes = np.array([[s - 5, s // 2], [s, s], [7, s - 1]], np.int32) if boxed else None
        ref = np.stack([mo.rasterize(r, bool(f[0]), bool(f[1]), s, tab) for r, f in zip(recs, flips)]).astype(np.float32)
        holes = (ref == 0).sum(axis=(1, 2))
        if boxed:
            for k, (bh, bw) in enumerate(boxes):
                ref[k, bh:, :] = 1
                ref[k, :, bw:] = 1
        jobs.append((np.concatenate(recs, axis=0) if offs[-1] else np.zeros((0, masks.REC), np.int32), offs, flips, s, boxes, ref, holes))

    def check(out):
        for (mask, holes), job in zip(out, jobs):
            assert np.array_equal(mask.cpu().numpy()[:, 0], job[5]) and np.array_equal(holes.cpu().numpy(), job[6])
    return (lambda: [masks.rasterize(j[0], j[1], j[2], j[3], DEV, j[4]) for j in jobs]), check


def lama_masks_case():
    """``lama_rasterize`` at s = 64 on hand-made lines and rectangles against the restatement of OpenCV's thick line, hole counts included
    (tests/test_gpu_lama.py)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import masks
    import test_gpu_lama as TA
    per_mask = [[TA.line_rec(c)] for c in TA.LINES[:8]] + [[TA.rect_rec(r)] for r in TA.RECTS[:2]] + [[]]
    per_mask.append([TA.line_rec(c) for c in TA.LINES[:13]] + [TA.rect_rec(TA.RECTS[0])])
    want = _once('lama', lambda: [TA.ref_painted(m, 64) for m in per_mask])
    offs = np.cumsum([0] + [len(m) for m in per_mask])
    recs = np.asarray([r for m in per_mask for r in m], dtype=np.int32).reshape(-1, 8)

    def check(out):
        mask, holes = out
        got = (1 - mask.cpu().numpy()[:, 0]).astype(np.uint8)
        for k in range(len(per_mask)):
            assert np.array_equal(got[k], want[k]) and int(holes[k]) == int(want[k].sum()), k
    return (lambda: masks.lama_rasterize(recs, offs, 64, DEV)), check


# ---- ADA and the optimiser

def ada_forward_case():
    """``ada_params`` (the tolerance rule of tests/test_gpu_ada.py on G_inv and the colour matrix, the margins equal) and ``ada_apply``
    forward with geometry and colour at (2, 3, 16, 24)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import ada
    import ada_f64 as R
    import test_gpu_ada as TA
    keys = R.GEOM_KEYS + R.COLOR_KEYS
    u, g = TA._draws(TA.PARAM_SEED)
    cfg = {k: 1 for k in keys}
    r64, r32 = _once('ada_params', lambda: (R.params(u, g, 1.0, cfg, 16, 24, torch.float64), R.params(u, g, 1.0, cfg, 16, 24, torch.float32)))
    pre = R.margins_pre(r64['G_inv'], 16, 24).numpy()
    c = TA.case((2, 3, 16, 24), 'rot_aniso_frac')
    pipe = ada.AugmentPipe(**cfg).to(DEV)
    ud, gd, x = u.to(DEV), g.to(DEV), c['x'].to(DEV)

    def call():
        G, Cm, margins, color = pipe.params((ud, gd), 3, 16, 24)
        assert color == (0, 3)
        return [G, Cm, margins, ada.ada_apply(x, **TA.dev_args(c))]

    def check(out):
        G, Cm, margins, y = out
        assert [int(v) for v in margins.cpu()] == [int(v) for v in np.ceil(pre)]
        TA.check('fill G_inv', G, r64['G_inv'], r32['G_inv'])
        TA.check('fill colour', Cm, r64['C'], r32['C'])
        TA.check('fill forward', y, c['ref'][torch.float64]['y'], c['ref'][torch.float32]['y'])
    return call, check


def ada_adjoint_case():
    """A^T w with geometry and colour, and with colour alone (the one adjoint output that is not zeroed first), against float64 autograd
    of the restatement.  Float atomics: NOT_REPRODUCIBLE."""
    import shgan_amd  # noqa: F401
    from shgan_amd import ada
    import ada_f64 as R
    import test_gpu_ada as TA
    c = TA.case((2, 3, 16, 24), 'rot_aniso_frac')
    w = c['w'].to(DEV)
    col = _once('ada_adjoint_colour', lambda: [R.adjoint(c['w'].to(dt), (2, 3, 16, 24), C34=c['Cm'].to(dt), channels=c['ch']) for dt in (torch.float64, torch.float32)])

    def check(out):
        TA.check('fill adjoint', out[0], c['ref'][torch.float64]['atw'], c['ref'][torch.float32]['atw'])
        TA.check('fill adjoint, colour alone', out[1], col[0], col[1])
    return (lambda: [ada.ada_apply_adjoint(w, **TA.dev_args(c)), ada.ada_apply_adjoint(w, Cm=c['Cm'].to(DEV), color_channels=c['ch'])]), check


BUCKET = [(5,), (7, 9), (1023,)]          # a three-tensor bucket, no size a multiple of 4


def adam_ema_case():
    """One ShgAdam step from the gradient bucket and one EmaUpdater launch on three tensors of 5, 63 and 1023 elements, under the 2 x rule
    of tests/test_gpu_optim.py: the error against the float64 yardstick at most twice that of torch's own float32 arithmetic."""
    import shgan_amd  # noqa: F401
    from shgan_amd import optim
    from shgan_amd.grad_sync import BucketedAllReduce
    import adam_f64
    rs = np.random.RandomState(21)
    init = [rs.standard_normal(s).astype(np.float32) for s in BUCKET]
    grads = [rs.standard_normal(s).astype(np.float32) for s in BUCKET]
    ema0 = [rs.standard_normal(s).astype(np.float32) for s in BUCKET]
    lr, betas, eps, beta = 0.002, (0.9, 0.999), 1e-8, 0.75

    class Net(torch.nn.Module):
        def __init__(self, arrays):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(a.copy())) for a in arrays])

    def call():
        net, ref_net, ema_net = Net(init).to(DEV), Net(init).to(DEV), Net(ema0).to(DEV)
        params, ref_params = list(net.parameters()), list(ref_net.parameters())
        sync = BucketedAllReduce(params, bucket_bytes=1 << 21)
        try:
            opt = optim.ShgAdam(params, lr=lr, betas=betas, eps=eps, sync=sync)
            ref = torch.optim.Adam(ref_params, lr=lr, betas=betas, eps=eps, foreach=True, fused=False)
            sync.zero_grad()
            with torch.enable_grad():
                sum((p * torch.from_numpy(g).to(DEV)).sum() for p, g in zip(params, grads)).backward()
            opt.step_from_buckets(world=1)
            for p, g in zip(ref_params, grads):
                p.grad = torch.from_numpy(g).to(DEV)
            ref.step()
            ema = optim.EmaUpdater(ema_net, net)
            ema.set_beta(beta)
            ema.launch()
            ema_ref = [p.detach().lerp(torch.from_numpy(e).to(DEV), float(np.float32(beta))) for p, e in zip(params, ema0)]
            return [[p.detach() for p in params], [opt.state[p]['exp_avg'] for p in params], [opt.state[p]['exp_avg_sq'] for p in params],
                    [p.detach() for p in ema_net.parameters()], [p.detach() for p in ref_params], [ref.state[p]['exp_avg'] for p in ref_params],
                    [ref.state[p]['exp_avg_sq'] for p in ref_params], ema_ref]
        finally:
            sync.remove()

    def check(out):
        p, m, v, pe, rp, rm, rv, re = [[t.cpu().numpy() for t in grp] for grp in out]
        y = [adam_f64.adam_step_f64(a.astype(np.float64), adam_f64.sanitize_f64(g, 1), np.zeros(a.shape), np.zeros(a.shape), 0, lr, betas[0], betas[1], eps)
             for a, g in zip(init, grads)]
        for k, (ours, theirs) in enumerate(((p, rp), (m, rm), (v, rv))):
            eo = max(adam_f64.rel_err(a, yy[k]) for a, yy in zip(ours, y))
            et = max(adam_f64.rel_err(a, yy[k]) for a, yy in zip(theirs, y))
            assert eo <= 2 * et, ('pmv'[k], eo, et)
        ye = [adam_f64.ema_f64(e.astype(np.float64), a, float(np.float32(beta))) for e, a in zip(ema0, p)]
        eo, et = max(adam_f64.rel_err(a, b) for a, b in zip(pe, ye)), max(adam_f64.rel_err(a, b) for a, b in zip(re, ye))
        assert eo <= 2 * et, ('ema', eo, et)
    return call, check


# ------------------------------------------------------------------------------------------------
# d. modules: the 256^2 generator of the suite's ``small_g`` configuration, and one phase each of the training loss
# ------------------------------------------------------------------------------------------------
SMALL = dict(ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)


def generator_fp32_case():
    """Forward in float32, batch 2, noise_mode='const', against the reference's image (tests/golden/generator_small.npz): 1e-3, the bound of
    test_generator_small_golden.  The module is built once; its prepared weights (``_ParamCache``) are dropped before every run."""
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, eval_harness
    from oracle import shgan_oracle as orc
    g = load_golden('generator_small')
    res, ch_base, ch_max, w_dim, z_dim, w0_dim = [int(v) for v in g['cfg']]
    assert (res, dict(ch_base=ch_base, ch_max=ch_max, w_dim=w_dim, z_dim=z_dim, w0_dim=w0_dim)) == (256, SMALL)

    def build():
        G = configs.build_generator(256, **SMALL)
        G.load_state_dict(orc.init_state_dict(256, seed=int(g['seed']), noise_strength=0.1, bias_std=0.1, **SMALL), strict=True)
        return G.eval().requires_grad_(False).to(DEV)
    G = _once('G_fp32', build)
    real = torch.from_numpy(g['real_u8'].astype(np.float32)) / 127.5 - 1.0
    mask = torch.from_numpy(np.unpackbits(g['mask_bits'])[: 2 * 256 * 256].reshape(2, 1, 256, 256).astype(np.float32))
    x, z, cnd = eval_harness.assemble_input(real, mask).to(DEV), torch.from_numpy(g['z']).to(DEV), torch.zeros(2, 0, device=DEV)
    return (lambda: G(x=x, z=z, c=cnd, noise_mode='const')), (lambda img: _assert(rel_err(img.cpu().numpy(), g['img_const']) < 1e-3))


def generator_fp16_case():
    """The same generator with fp16 blocks (encoder 256 / 128, synthesis 64 .. 256) against the reference's fp16 run (tests/golden/fp16.npz):
    2e-2, the bound of test_generator_fp16_blocks_vs_reference."""
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, eval_harness
    from oracle import shgan_oracle as orc
    g = load_golden('fp16')

    def build():
        G = configs.build_generator(256, use_fp16_before_res=64, use_fp16_after_res=32, **SMALL)
        G.load_state_dict(orc.init_state_dict(256, seed=int(g['G__seed']), noise_strength=0.1, bias_std=0.1, **SMALL), strict=True)
        return G.eval().requires_grad_(False).to(DEV)
    G = _once('G_fp16', build)
    real = torch.from_numpy(np.random.RandomState(74).randint(0, 256, size=(2, 3, 256, 256)).astype(np.uint8).astype(np.float32)) / 127.5 - 1.0
    mask = torch.from_numpy(np.unpackbits(g['G__mask_bits'])[: 2 * 256 * 256].reshape(2, 1, 256, 256).astype(np.float32))
    x, z, cnd = eval_harness.assemble_input(real, mask).to(DEV), torch.from_numpy(g['G__z']).to(DEV), torch.zeros(2, 0, device=DEV)

    def check(img):
        assert img.dtype == torch.float32 and rel_err(img.float().cpu().numpy()[:, :, ::4, ::4], g['G__img_eval']) < 2e-2
    return (lambda: G(x=x, z=z, c=cnd, noise_mode='const')), check


def training_phase_case(phase):
    """One phase of ``InpaintingLoss`` (ADA off, no style mixing, noise_mode='const') at batch 2 on the small generator and its critic: the
    per-sample loss and every parameter gradient of the network being trained.  Finite and bit-equal across the fills; the float64
    parity of these gradients stays with tests/test_gpu_backward.py."""
    def make():
        import shgan_amd  # noqa: F401
        from shgan_amd import losses
        import test_gpu_optim as TOp
        G, D = _once('train_nets', lambda: TOp.small_networks(5))
        real4 = TOp.real_batch(2, 6)
        z = torch.from_numpy(np.random.RandomState(1).standard_normal((2, 64)).astype(np.float32)).to(DEV)
        cnd = torch.zeros(2, 0, device=DEV)
        net, key = (D, 'Loss/D/loss') if phase == 'Dmain' else (G, 'Loss/G/loss')

        def call():
            L = losses.InpaintingLoss(DEV, G, D, composite_fake=True, noise_mode='const', style_mixing_prob=0)
            G.zero_grad(set_to_none=True)
            D.zero_grad(set_to_none=True)
            G.requires_grad_(net is G)
            D.requires_grad_(net is D)
            try:
                L.accumulate_gradients(phase, real4, cnd, z, cnd, sync=True, gain=1)
                grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
            finally:
                G.requires_grad_(False)
                D.requires_grad_(False)
                G.zero_grad(set_to_none=True)
                D.zero_grad(set_to_none=True)
            return [L.stats[key], grads]

        def check(out):
            loss, grads = out
            assert loss.shape[0] == 2 and len(grads) >= 0.9 * len(list(net.parameters())) and any(float(v.abs().max()) > 0 for v in grads.values())
        return call, check
    return make


def synthetic_items_case():
    """``eval_harness.synthetic_items``: three buffers drawn whole by the device RNG; x = cat([mask - 0.5, real * mask]) exactly."""
    import shgan_amd  # noqa: F401
    from shgan_amd import eval_harness as hz

    def check(out):
        x, z, real_u8, mask = out
        real = real_u8.to(torch.float32).div(127.5).sub(1.0)                  # (on the device, as the function itself computes it)
        assert set(np.unique(mask.cpu().numpy())) <= {0.0, 1.0} and bool(torch.isfinite(z).all())
        assert torch.equal(x, torch.cat([mask - 0.5, real * mask], dim=1))
    return (lambda: list(hz.synthetic_items([3, 0, 7], 64, z_dim=8, seed=2, device=DEV))), check


def eval_loop_case():
    """``EvalLoop`` over 5 items in batches of 2 (a ragged last batch), two slots: its result buffer equals ``run_generator`` batch by batch,
    bit for bit (test_eval_loop_equals_the_plain_per_batch_calls)."""
    import shgan_amd  # noqa: F401
    from shgan_amd import configs, eval_harness as hz, masks
    import test_gpu_eval_loop as TE
    G = _once('G_small5', lambda: configs.seeded_init_(configs.build_generator(256, **SMALL), seed=5, noise_strength=0.1, bias_std=0.1)
              .eval().requires_grad_(False).to(DEV))

    def call():
        loop = hz.EvalLoop(G, DEV, 256, 5, noise_mode='const', depth=2, latent_fn=TE._latents)
        np.random.seed(77)
        loop.run(hz.PinnedU8Loader(loop.ids, 2, 256, seed=9))
        images, _ = loop.gather()
        np.random.seed(77)
        outs = []
        for img, ids in hz.PinnedU8Loader(list(range(5)), 2, 256, seed=9):
            m = masks.random_masks(len(ids), 256, [0, 1], device=DEV)
            x = hz.assemble_input((img.to(torch.float32).div(255) * 2 - 1).to(DEV), m)
            outs.append(hz.run_generator(G, x, TE._latents(ids, len(ids)), noise_mode='const'))
        return [images, torch.cat(outs)]

    def check(out):
        images, want = out
        assert images.dtype == torch.uint8 and tuple(images.shape) == (5, 3, 256, 256) and torch.equal(images, want), int((images != want).sum())
    return call, check


EXTRA = {
    'ops:planes_to_image': planes_to_image_case,
    'ops:modtail_backward_f32': modtail_backward_f32_case,
    'ops:sum_partials': sum_partials_case,
    'ops:scale_channels': scale_channels_case,
    'ops:scale_cast': scale_cast_case,
    'ops:composite_u8': composite_u8_case,
    'ops:assemble_input': assemble_input_case,
    'ops:fma': fma_case,
    'shu:forward_A': shu_forward_case('A'),
    'shu:forward_C': shu_forward_case('C'),
    'shu:training_C': shu_training_case,
    'inception:convs_b1': inception_convs_case,
    'inception:grouped_splitk': inception_grouped_splitk_case,
    'inception:pools': inception_pools_case,
    'inception:frontend_mean_head': inception_frontend_mean_head_case,
    'inception:detector': inception_detector_case,
    'vgg16:frontend_pool_detector': vgg16_case,
    'lpips:distance': lpips_case,
    'lpips:vgg_distance': lpips_vgg_case,
    'metrics:psnr_ssim': image_metrics_case,
    'metrics:kid_is_fid': kid_is_fid_case,
    'metrics:precision_recall': precision_recall_case,
    'input:ppl_frontend': ppl_frontend_case,
    'input:resize': resize_case,
    'input:randcrop': randcrop_case,
    'masks:freeform': freeform_masks_case,
    'masks:lama': lama_masks_case,
    'ada:forward': ada_forward_case,
    'ada:adjoint': ada_adjoint_case,
    'optim:adam_ema': adam_ema_case,
    'harness:synthetic_items': synthetic_items_case,
    'harness:eval_loop': eval_loop_case,
    'module:generator_fp32': generator_fp32_case,
    'module:generator_fp16': generator_fp16_case,
    'module:loss_Dmain': training_phase_case('Dmain'),
    'module:loss_Gmain': training_phase_case('Gmain'),
}


@gpu
@pytest.mark.parametrize('case', sorted(EXTRA))
def test_entry_point(case):
    sites = independent(EXTRA[case], lambda out, check: check(out), reproducible=case not in NOT_REPRODUCIBLE, case=case)
    _finish(case, sites)


# ------------------------------------------------------------------------------------------------
# coverage (host-only): every allocation site of the package has a case, or a reason
# ------------------------------------------------------------------------------------------------
# (file, function) -> ids of GPU cases above that reach it; each of those cases asserts that the fill saw the site while it ran.
SITES = {
    ('ada.py', '_launch'): ['ada:adjoint', 'ada:forward'],
    ('ada.py', 'ada_params'): ['ada:forward'],
    ('eval_harness.py', '__init__'): ['harness:eval_loop'],
    ('eval_harness.py', '_draw'): ['harness:eval_loop'],
    ('eval_harness.py', 'synthetic_items'): ['harness:synthetic_items'],
    ('image_metrics.py', 'add'): ['metrics:psnr_ssim'],
    ('image_metrics.py', 'image_metrics'): ['metrics:psnr_ssim'],
    ('inception.py', '_new'): ['inception:detector'],
    ('inception.py', 'conv_group'): ['inception:convs_b1', 'inception:detector', 'inception:grouped_splitk'],
    ('inception.py', 'frontend'): ['inception:detector', 'inception:frontend_mean_head'],
    ('inception.py', 'global_mean'): ['inception:detector', 'inception:frontend_mean_head'],
    ('inception.py', 'head_probs'): ['inception:frontend_mean_head'],
    ('inception.py', 'pack_weight'): ['inception:convs_b1', 'inception:detector', 'inception:grouped_splitk'],
    ('inception.py', 'pool'): ['inception:detector', 'inception:pools', 'lpips:distance'],
    ('kernels.py', '_poly'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', '_wino_workspace'): ['fp32:same_i_1024', 'fp32:same_wino4_split', 'fp32:up_poly_split'],
    ('kernels.py', 'assemble_input'): ['harness:eval_loop', 'harness:synthetic_items', 'ops:assemble_input'],
    ('kernels.py', 'bias_act'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'bias_act_backward'): ['module:loss_Dmain', 'module:loss_Gmain', 'fp32:bias_act_backward_clamp'],
    ('kernels.py', 'composite_u8'): ['harness:eval_loop', 'ops:composite_u8'],
    ('kernels.py', 'conv1x1_thin_in'): ['harness:eval_loop', 'module:generator_fp32', 'module:loss_Dmain'],
    ('kernels.py', 'conv2d'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'conv2d_wgrad'): ['module:loss_Dmain', 'module:loss_Gmain', 'shu:training_C'],
    ('kernels.py', 'conv_weight_prep'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'demod_weight'): ['module:loss_Gmain'],
    ('kernels.py', 'demod_weight_backward'): ['module:loss_Gmain'],
    ('kernels.py', 'dense'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'fir_conv_down2'): ['fp32:downlayer_i_eq_min', 'fp32:fir_conv_down2_flat22', 'fp32:fir_conv_down2_flat43'],
    ('kernels.py', 'fma'): ['ops:fma'],
    ('kernels.py', 'matmul_nn'): ['module:loss_Dmain', 'module:loss_Gmain', 'dense:modulation_n33_composed'],
    ('kernels.py', 'matmul_tn'): ['module:loss_Dmain', 'module:loss_Gmain', 'dense:modulation_n33_composed'],
    ('kernels.py', 'minibatch_std'): ['fp32:mbstd_group_2_f2', 'fp32:mbstd_group_4', 'fp32:mbstd_group_clamped_to_n'],
    ('kernels.py', 'modconv_style_prep'): ['module:generator_fp16', 'dense:prep_i1000_o65', 'dense:prep_i1_o1'],
    ('kernels.py', 'modtail_backward'): ['module:loss_Dmain', 'module:loss_Gmain', 'ops:modtail_backward_f32'],
    ('kernels.py', 'mul_reduce'): ['ops:fma'],
    ('kernels.py', 'normalize_2nd_moment'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'planes_to_image'): ['ops:planes_to_image'],
    ('kernels.py', 'scale_cast'): ['module:loss_Dmain', 'module:loss_Gmain', 'ops:scale_cast'],
    ('kernels.py', 'scale_channels'): ['ops:scale_channels'],
    ('kernels.py', 'shu_rfft2_shift'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'shu_spectral'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'shu_split_adjoint'): ['module:loss_Gmain', 'shu:training_C'],
    ('kernels.py', 'style_factors'): ['module:loss_Gmain', 'dense:stylefn_n17_i64_o513', 'dense:stylefn_n17_i64_o513_half'],
    ('kernels.py', 'style_factors_backward'): ['module:loss_Gmain', 'dense:stylefn_n17_i64_o513', 'dense:stylefn_n17_i64_o513_half'],
    ('kernels.py', 'sum_partials'): ['module:loss_Dmain', 'module:loss_Gmain', 'ops:modtail_backward_f32'],
    ('kernels.py', 'torgb'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'upfir_planar'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'upfirdn2d'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'upfirdn2d_strided'): ['fp32:fir_strided_f16', 'fp32:fir_strided_f32', 'fp32:fir_strided_f64'],
    ('kernels.py', 'wino'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels.py', 'wino4'): ['harness:eval_loop', 'module:generator_fp16', 'module:generator_fp32'],
    ('kernels_f16.py', '_pad_channels'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kernels_f16.py', '_taps_weight'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kernels_f16.py', 'bias_act'): ['fp16:bias_act_c16', 'fp16:bias_act_c24', 'fp16:bias_act_c40'],
    ('kernels_f16.py', 'bias_act_backward'): ['module:loss_Gmain', 'fp16:bias_act_bwd_c24_9x7', 'fp16:bias_act_bwd_c8_2097229_past_cap'],
    ('kernels_f16.py', 'conv2d'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kernels_f16.py', 'conv2d_wgrad'): ['module:loss_Dmain', 'fp16:wgrad_1x1_18_blocks_on_16_slices', 'fp16:wgrad_1x1_one_block'],
    ('kernels_f16.py', 'conv_transpose2d'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kernels_f16.py', 'modtail'): ['module:generator_fp16', 'fp16:modtail_c16_per_noise', 'fp16:modtail_c16_shared_noise'],
    ('kernels_f16.py', 'modtail_backward'): ['module:loss_Dmain', 'fp16:mtb_c512_32x32_at_cap', 'fp16:mtb_c512_32x32_at_cap_ue'],
    ('kernels_f16.py', 'relayout'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kernels_f16.py', 'upfirdn2d'): ['module:generator_fp16', 'module:loss_Dmain', 'module:loss_Gmain'],
    ('kid.py', 'kid_sums'): ['metrics:kid_is_fid'],
    ('lpips.py', '<lambda>'): ['lpips:distance'],
    ('lpips.py', 'conv1'): ['lpips:distance'],
    ('lpips.py', 'features'): ['lpips:vgg_distance'],
    ('lpips.py', 'head'): ['lpips:distance', 'lpips:vgg_distance'],
    ('lpips.py', 'pack_conv1'): ['lpips:distance'],
    ('lpips.py', 'scaling'): ['lpips:vgg_distance'],
    ('masks.py', 'lama_rasterize'): ['masks:lama'],
    ('masks.py', 'rasterize'): ['harness:eval_loop', 'masks:freeform'],
    ('model_zoo/comodgan.py', '_all_styles'): ['harness:eval_loop', 'module:generator_fp32', 'module:loss_Dmain'],
    ('model_zoo/shgan.py', 'forward'): ['module:generator_fp16', 'module:loss_Gmain', 'shu:forward_A'],
    ('model_zoo/stylegan_utils/dense_ops.py', 'forward'): ['dense:modulation_n33_composed', 'dense:modulation_n33_composed_half'],
    ('ppl.py', 'frontend'): ['input:ppl_frontend'],
    ('precision_recall.py', 'inside'): ['metrics:precision_recall'],
    ('precision_recall.py', 'radii'): ['metrics:precision_recall'],
    ('resize.py', 'pack_images'): ['input:randcrop', 'input:resize'],
    ('resize.py', 'randcrop_bicubic'): ['input:randcrop'],
    ('resize.py', '_launch_resize'): ['input:resize'],
    ('vgg16.py', 'conv_trunk'): ['lpips:vgg_distance', 'vgg16:frontend_pool_detector'],
    ('vgg16.py', 'fc_relu'): ['vgg16:frontend_pool_detector'],
    ('vgg16.py', 'frontend'): ['vgg16:frontend_pool_detector'],
    ('vgg16.py', 'maxpool2'): ['lpips:vgg_distance', 'vgg16:frontend_pool_detector'],
}

# (file, function) -> why the fill has nothing to say about the site
NOT_FILLED = {
    ('eval_harness.py', 'broadcast_state'): 'the flat buffer of a broadcast: the source rank copies every element into it, RCCL writes it whole on the others',
    ('eval_harness.py', 'sharded_eval'): 'the output of all_gather_into_tensor: written whole by RCCL, no kernel of this project touches it',
    ('evaluators.py', 'rows'): 'the output of all_gather_into_tensor: written whole by RCCL, no kernel of this project touches it',
    ('fid_stats.py', 'gather_features'): 'the output of all_gather_into_tensor: written whole by RCCL, no kernel of this project touches it',
    ('losses.py', '_style_mix'): "a scalar that torch's random_ draws on the same line; the cases run with style mixing off to stay deterministic",
    ('model_zoo/shgan.py', '__init__'): "the storage of an nn.Parameter at construction, on the host: init='ones' or the state dict every user loads sets it",
    ('masks.py', 'random_masks'): 'the result for n = 0: a tensor of zero elements has no contents',
}


def scan_allocation_sites():
    """(file, function) of every ``torch.empty(``, ``empty_like(``, ``new_empty(``, ``L.new(`` (``L``: the ``_Launch`` of the call) and
    ``_new_cl(`` in sh-gan_amd/**/*.py; the two pass-through allocators themselves (``alloc_fill.WRAPPERS``) are not sites."""
    found = {}
    for base, _, files in os.walk(PACKAGE_DIR):
        for fn in sorted(files):
            if not fn.endswith('.py'):
                continue
            path = os.path.join(base, fn)
            rel = os.path.relpath(path, PACKAGE_DIR).replace(os.sep, '/')
            with open(path) as f:
                tree = ast.parse(f.read())

            def visit(node, func):
                for ch in ast.iter_child_nodes(node):
                    inner = func
                    if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        inner = ch.name
                    elif isinstance(ch, ast.Lambda):
                        inner = '<lambda>'
                    if isinstance(ch, ast.Call):
                        f_ = ch.func
                        hit = False
                        if isinstance(f_, ast.Attribute):
                            hit = ((f_.attr == 'empty' and isinstance(f_.value, ast.Name) and f_.value.id == 'torch') or f_.attr in ('empty_like', 'new_empty')
                                   or (f_.attr == 'new' and isinstance(f_.value, ast.Name) and f_.value.id == 'L'))
                        elif isinstance(f_, ast.Name):
                            hit = f_.id == '_new_cl'
                        if hit and (rel, func) not in WRAPPERS:
                            found[(rel, func)] = found.get((rel, func), 0) + 1
                    visit(ch, inner)
            visit(tree, '<module>')
    return found


def all_case_ids():
    ids = {f'fp32:{c}' for c in R32.CASES} | {f'fp16:{c}' for c in R16.CASES} | {f'dense:{c}' for c in RD.CASES}
    return ids | {f'fuzz:{f}' for f in fuzz_cases.FAMILIES} | set(EXTRA)


def test_every_allocation_site_has_a_case():
    found = scan_allocation_sites()
    assert sum(found.values()) >= 120 and len(found) >= 80, (len(found), sum(found.values()))        # the scan still finds the package
    both = set(SITES) & set(NOT_FILLED)
    assert not both, f'listed twice: {sorted(both)}'
    missing = sorted(set(found) - set(SITES) - set(NOT_FILLED))
    assert not missing, f'allocation sites without a case in SITES or a reason in NOT_FILLED: {missing}'
    stale = sorted((set(SITES) | set(NOT_FILLED)) - set(found))
    assert not stale, f'listed, but the scan finds no allocation there any more: {stale}'
    ids = all_case_ids()
    for site, cases in SITES.items():
        assert cases and all(c in ids for c in cases), f'{site}: unknown case id among {cases}'
    for site, reason in NOT_FILLED.items():
        assert len(reason) > 20 and 'not tested' not in reason.lower(), site
