"""No entry point may touch memory outside the buffers it is given (run the GPU part with -m gpu on an MI355X).

The HIP library never allocates: every output, workspace and scratch buffer is made in Python and the kernels receive bare pointers and
sizes.  tests/test_gpu_alloc_fill.py proves that every element later read was written; this file looks at the other side of the
boundary.  Every case of that file (the three route tables whole, the fuzz families, ``EXTRA``: imported, not copied) runs twice:

  1. control: under ``alloc_fill.filled('zero')``, results snapshotted;
  2. guarded run: under ``alloc_guard.guarded()``: every fresh buffer, and every host tensor sent to the device, is the interior of a raw
     buffer with 1 MiB of poison on either side and no slack.  ``WRITES OUTSIDE ITS BUFFER`` if a guard was damaged;
  3. same bits: the guarded results are bit-equal to the control, otherwise ``READS OUTSIDE ITS BUFFER (or takes another route under the
     guard)``: a guard value that reached a result is an over-read (a route change would be a defect of the helper);
  4. bar: the case's own bar holds on the guarded results, which are finite where the case's are (the guards are checked once more
     after the bar, which may launch kernels of its own).
For the cases of ``NOT_REPRODUCIBLE`` step 3 is dropped.  No tolerance and no shape is introduced here, and there is no list of
tolerated violations.  What the check cannot see is stated in tests/alloc_guard.py: an access further than the band from the buffer, a
store of the poison value itself, an over-read whose value never reaches a result.  Tensors from other functions than those the helper
replaces (``torch.tensor``, ``randn``, ``arange`` with a device) and what a case builds once per process (its ``_once`` objects, made in the
control run) keep their ordinary blocks; the weights prepared from them are made again, housed, in every run.

Host-only: the judge on stand-ins, and the coverage of the ``zeros`` / ``ones`` / ``full`` allocation sites of the package, which the
guard houses in addition to the ``empty`` sites of the fill test: each is claimed by cases that were seen to reach it (``INIT_SITES``;
each GPU case asserts its claims) or listed with the reason (``NOT_GUARDED``)."""
import ast
import os

import pytest
import torch

import alloc_guard
import test_gpu_alloc_fill as TF
from alloc_fill import PACKAGE_DIR, filled
from alloc_guard import guarded
from test_gpu_alloc_fill import EXTRA, NOT_REPRODUCIBLE, R16, R32, RD, _difference, _reset_caches, _snapshot, fuzz_cases

gpu = pytest.mark.gpu
DEV = 'cuda:0'
FUZZ_SEEDS = 3


# ------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------

def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _no_writes(rec, when):
    found = rec.violations()
    assert not found, f'WRITES OUTSIDE ITS BUFFER ({when}): {found}'


def contained(make, bars, reproducible=True, case=None, finite=True):
    """``make() -> (call, ctx)``, ``call()`` and ``bars(out, ctx)`` as for ``test_gpu_alloc_fill.independent``.  -> (the allocation sites
    the guard saw, those among them of the initialising factories)."""
    if not reproducible:
        assert case in NOT_REPRODUCIBLE, f'{case}: only the cases of NOT_REPRODUCIBLE may skip the bit comparison'
    _reset_caches()
    with filled('zero'):
        call, ctx = make()
        control = _snapshot(call())
        _sync()
    assert len(control) > 0, 'the case returned no tensor'
    _reset_caches()
    with guarded() as rec:
        call, ctx = make()
        out = call()
        _no_writes(rec, 'the guarded run')
        snap = _snapshot(out)
        if reproducible:
            diff = _difference(control, snap)
            assert diff is None, f'READS OUTSIDE ITS BUFFER (or takes another route under the guard): guarded against control: {diff}'
        for k, t in enumerate(snap):
            if finite and t.is_floating_point():
                assert bool(torch.isfinite(t).all()), f'NOT FINITE under the guard: tensor {k} {tuple(t.shape)}'
        bars(out, ctx)
        _no_writes(rec, "the case's bar")
        return set(rec.sites), rec.sites_of(alloc_guard.INITIALISING)


def _finish(case_id, seen):
    sites, init = seen
    print(f'GUARD_SITES_SEEN {case_id} {sorted(sites)}')
    print(f'GUARD_INIT_SITES_SEEN {case_id} {sorted(init)}')
    missing = TF._claimed(case_id) - sites
    assert not missing, f'{case_id} is listed in SITES for {sorted(missing)} but no allocation there was housed while it ran'
    missing = {site for site, ids in INIT_SITES.items() if case_id in ids} - init
    assert not missing, f'{case_id} is listed in INIT_SITES for {sorted(missing)} but no zeros / ones / full there was housed while it ran'


# ---- the judge on stand-ins

def _storage(t):
    """Every element of the storage behind ``t`` as a flat view, and the position of t[0] in it."""
    n = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((n,), (1,), 0), t.storage_offset()


def _stand_in(kind, device='cpu'):
    """A toy entry point: allocates 6 floats and writes twice its operand into them, with plain torch indexing on a flat view of its own
    storage.  Housed by the guard, that storage has room on either side, and the stand-in then (b) writes one element past the end,
    (c) one element in front, (d) adds the element past the end of its operand into its result, (e) writes the poison itself past the end;
    (a) stays inside, (f) stays inside and is wrong.  Without the guard there is no such room and all of them stay inside."""
    def make():
        x = torch.empty(6, device=device)
        x.copy_(torch.arange(1.0, 7.0))

        def call():
            y = torch.empty(6, device=device)
            y.copy_(x * 2)
            flat, at = _storage(y)
            room = at >= 1 and flat.numel() > at + 6
            if kind == 'b' and room:
                flat[at + 6] = 7.0
            if kind == 'c' and room:
                flat[at - 1] = 7.0
            if kind == 'd':
                xs, xat = _storage(x)
                if xs.numel() > xat + 6:
                    y[0] += xs[xat + 6]
            if kind == 'e' and room:
                flat.view(torch.int32)[at + 6] = -1
            return y + 1 if kind == 'f' else y
        return call, torch.arange(1.0, 7.0) * 2
    return make


def _bar(out, ref):
    assert torch.equal(out.cpu(), ref), 'bar'


def _judge_on_stand_ins(device):
    assert contained(_stand_in('a', device), _bar) == (set(), set())
    with pytest.raises(AssertionError, match=r'WRITES OUTSIDE ITS BUFFER.*empty \(6,\) torch.float32: side back, 4 bytes at offset 0 \.\. 3 \(elements 0 \.\. 0\), found \[7\.0'):
        contained(_stand_in('b', device), _bar)
    with pytest.raises(AssertionError, match=r'WRITES OUTSIDE ITS BUFFER.*side front, 4 bytes at offset -4 \.\. -1 \(elements -1 \.\. -1\)'):
        contained(_stand_in('c', device), _bar)
    with pytest.raises(AssertionError, match=r'READS OUTSIDE ITS BUFFER.*1 of 6 elements differ, first at \[\[0\]\]'):
        contained(_stand_in('d', device), _bar)
    contained(_stand_in('e', device), _bar)
    with pytest.raises(AssertionError, match='bar'):
        contained(_stand_in('f', device), _bar)
    with pytest.raises(AssertionError, match='NOT_REPRODUCIBLE'):
        contained(_stand_in('a', device), _bar, reproducible=False, case='toy')


def test_the_judge_on_host_stand_ins():
    """What each step of ``contained`` catches, on toy entry points (no GPU): (a) a writer that stays inside passes; (b) one element past
    the end and (c) one element in front are write findings with side, size and offset; (d) an operand element past the end that reaches
    the result is a read finding; (f) a wrong result fails its bar.  (e) A store of the poison value itself past the end (0xFFFFFFFF into
    a float guard) is NOT detected, by construction: a guard is compared with its poison and nothing else is known about it.  It passes
    here so that this limit is on record."""
    _judge_on_stand_ins('cpu')


@gpu
def test_the_guard_and_the_judge_on_the_device():
    """The same stand-ins on device memory, and what the helper promises about the tensors it hands out: shape, strides, dtype, memory
    format, pinned-ness and ``data_ptr() % 512`` of what the original factory returns (512 bytes is the granularity of torch's device
    allocator: the assumption the band size rests on is checked here), zero interior, initialised values, poisoned guards."""
    _judge_on_stand_ins(DEV)
    src = torch.zeros(2, 8, 3, 5, dtype=torch.float16, device=DEV).contiguous(memory_format=torch.channels_last)
    host = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).permute(2, 0, 1)
    perm = torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV).permute(2, 0, 1)
    makers = {
        'empty_cl': lambda: torch.empty((2, 8, 3, 5), dtype=torch.float16, device=DEV, memory_format=torch.channels_last),
        'empty_odd': lambda: torch.empty(7, device=DEV),
        'empty_f64': lambda: torch.empty(3, dtype=torch.float64, device=DEV),
        'empty_u8': lambda: torch.empty(5, dtype=torch.uint8, device=DEV),
        'new_empty_i32': lambda: src.new_empty((2, 2), dtype=torch.int32),
        'like': lambda: torch.empty_like(src),
        'like_permuted': lambda: torch.empty_like(perm),
        'zeros': lambda: torch.zeros(3, 5, device=DEV),
        'full_i64': lambda: torch.full((4,), 9, dtype=torch.int64, device=DEV),
        'ones_like': lambda: torch.ones_like(src),
        'new_full': lambda: src.new_full((3,), 2.5),
        'empty0': lambda: torch.empty((0, 4), device=DEV),
        'to': lambda: host.to(DEV),
        'cuda': lambda: host.cuda(),
        'pinned': lambda: torch.empty(6, dtype=torch.int32, pin_memory=True),
    }
    plain = {k: m() for k, m in makers.items()}
    with guarded() as rec:
        housed = {k: m() for k, m in makers.items()}
        assert rec.violations() == [] and rec.count == len(makers)
        for k, g in housed.items():
            p = plain[k]
            assert (g.shape, g.stride(), g.dtype, g.device, g.is_pinned()) == (p.shape, p.stride(), p.dtype, p.device, p.is_pinned()), k
            for fmt in (torch.contiguous_format, torch.channels_last):
                if g.dim() == 4:
                    assert g.is_contiguous(memory_format=fmt) == p.is_contiguous(memory_format=fmt), k
            assert g.is_contiguous() == p.is_contiguous(), k
            if g.is_cuda and g.numel():
                assert g.data_ptr() % 512 == p.data_ptr() % 512 == 0, (k, g.data_ptr() % 512, p.data_ptr() % 512)
            if k.startswith(('empty', 'like', 'new_empty', 'pinned')):
                assert not bool(g.any()), k
            else:
                assert torch.equal(g, p), k
        a = rec.allocations[1]
        assert a.nbytes == 28 and a.raw.numel() == 28 + 2 * rec.band and bool((a.raw[:rec.band] == 0xFF).all()) and bool((a.raw[rec.band + 28:] == 0xFF).all())
        assert bool(torch.isnan(a.raw[rec.band + 28:rec.band + 32].view(torch.float32)).all())
        a = rec.allocations[4]
        assert bool((a.raw[a.nbytes + rec.band:].view(torch.int32) == 3).all()) and bool((a.raw[:rec.band].view(torch.int32) == 3).all())


# ------------------------------------------------------------------------------------------------
# a. the three route tables, whole
# ------------------------------------------------------------------------------------------------

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
        e = TF.rel_err(got.numpy(), ref.numpy())
        print(f'GUARD fp32 {case} rel_err={e:.3e}')
        if tol == 0.0:
            assert torch.equal(got, ref), f'{case}: not bit-exact (rel err {e:.3e})'
        else:
            assert e < tol, f'{case}: rel err {e:.3e} >= {tol:.0e}'

    old = {k: getattr(kk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(kk, k, v)
        seen = contained(make, bars)
    finally:
        for k, v in old.items():
            setattr(kk, k, v)
    _finish(f'fp32:{case}', seen)


@gpu
@pytest.mark.parametrize('case', sorted(R16.CASES))
def test_fp16_route(case):
    builder, _, _, switches = R16.CASES[case]
    lib = R16._lib()

    def bars(got, judge):
        records = judge(got)
        print(f'GUARD fp16 {case} ' + ' '.join(f'{label}: {v:.3e} (bar {bar:.0e})' for label, v, bar, _ in records))
        for label, v, bar, strict in records:
            assert (v < bar) if strict else (v <= bar), f'{case}: {label} {v:.3e} exceeds {bar:.0e}'

    old = lib.shg_conv2d_f16_set_routes(switches['routes']) if 'routes' in switches else None
    try:
        # (the relayout cases cast values beyond the half range on purpose: the exception of the fill test, and the only one)
        seen = contained(builder, bars, finite=not case.startswith('relayout_'))
    finally:
        if old is not None:
            lib.shg_conv2d_f16_set_routes(old)
    _finish(f'fp16:{case}', seen)


@gpu
@pytest.mark.parametrize('case', sorted(RD.CASES))
def test_dense_route(case):
    builder = RD.CASES[case][0]

    def bars(got, judge):
        recs = judge()
        print(f'GUARD dense {case} ' + ' '.join(f'{nm}={e:.2e}/{b:.0e}' for nm, e, b in recs))
        for nm, e, b in recs:
            assert e <= b, f'{case}: {nm}: {e:.3e} exceeds {b:.0e}'

    _finish(f'dense:{case}', contained(builder, bars))


# ------------------------------------------------------------------------------------------------
# b. the fuzz families: the first 3 seeds of each
# ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('family,seed', [(f, s0 + k) for f, (_, s0, _) in fuzz_cases.FAMILIES.items() for k in range(FUZZ_SEEDS)])
def test_fuzz_family(family, seed):
    fn = fuzz_cases.FAMILIES[family][0]
    _reset_caches()
    with filled('zero'):
        control = fn(seed)
        torch.cuda.synchronize()
    _reset_caches()
    with guarded() as rec:
        got = fn(seed)
        _no_writes(rec, 'the guarded run')
        seen = set(rec.sites), rec.sites_of(alloc_guard.INITIALISING)
    assert got == control, (f'READS OUTSIDE ITS BUFFER (or takes another route under the guard): {family} seed {seed}: '
                            f'{[(a, b) for a, b in zip(control, got) if a != b]}')
    bad = [f'{what}: {desc}: {e:.3e} (bound {b:.0e})' for what, e, b, desc in got if not e < b]
    assert not bad, f'{family} seed {seed}: ' + '; '.join(bad)
    _finish(f'fuzz:{family}', seen)


# ------------------------------------------------------------------------------------------------
# c. the entry points outside the tables and the modules
# ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('case', sorted(EXTRA))
def test_entry_point(case):
    seen = contained(EXTRA[case], lambda out, check: check(out), reproducible=case not in NOT_REPRODUCIBLE, case=case)
    _finish(case, seen)


# ------------------------------------------------------------------------------------------------
# d. entry points whose buffers come from an initialising factory only, so that the fill test has no case for them: the tail of the ADA
# pipe and the empty reduction of ``mul_reduce`` (``torch.zeros`` results).  The shapes, references and bars are those of tests/test_gpu_ada_tail.py.
# ------------------------------------------------------------------------------------------------

def ada_tail_apply_case():
    """The fused filter + noise + cutout launch and its adjoint at (2, 4, 32, 24) and (1, 3, 70, 90), every category on."""
    import shgan_amd  # noqa: F401
    from shgan_amd import ada
    import test_gpu_ada_tail as TT
    cs = [TT.case(shape, 'all') for shape in ((2, 4, 32, 24), (1, 3, 70, 90))]
    dev = [(c['x'].to(DEV), c['w'].to(DEV), TT.dev(c['a']), TT.dev(c['lin'])) for c in cs]

    def call():
        return [[ada.ada_tail_apply(x, color_channels=c['ch'], **a), ada.ada_tail_apply_adjoint(w, color_channels=c['ch'], **lin)]
                for c, (x, w, a, lin) in zip(cs, dev)]

    def check(out):
        for c, (y, atw) in zip(cs, out):
            r64, r32 = c['ref'][torch.float64], c['ref'][torch.float32]
            TT.check('guard tail forward', y, r64['y'], r32['y'])
            TT.check('guard tail adjoint', atw, r64['atw'], r32['atw'])
    return call, check


def ada_tail_params_case():
    """The parameter kernel on the N = 8 fixed draws with every category on: taps, sigma and the box under the tolerance rule."""
    import shgan_amd  # noqa: F401
    from shgan_amd import ada
    import test_gpu_ada_tail as TT
    p, cfg = TT.PARAM_CASES['all']
    ut, gt = TT._draws(TT.PARAM_SEED)
    r64, r32 = TT.R.params(ut, gt, p, cfg, torch.float64), TT.R.params(ut, gt, p, cfg, torch.float32)
    pipe = ada.FullAugmentPipe(**cfg).to(DEV)
    pipe.p.fill_(p)
    utd, gtd = ut.to(DEV), gt.to(DEV)

    def check(out):
        for name, got in zip(('Hz', 'sigma', 'cut'), out):
            TT.check(f'guard tail {name}', got, r64[name], r32[name])
    return (lambda: list(pipe.tail_params((None, None, utd, gtd)))), check


def mul_reduce_empty_case():
    """``mul_reduce`` of a gradient of no elements into a non-empty shape (an empty batch through the backward of the public ``fma``): a sum
    of no terms, returned from ``torch.zeros`` without a launch; float32 and float64, with and without the second factor."""
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels as kk
    gs = [torch.zeros(0, 3, dtype=dt, device=DEV) for dt in (torch.float32, torch.float64)]
    bs = [torch.ones(1, 3, dtype=g.dtype, device=DEV) for g in gs]

    def check(out):
        for k, got in enumerate(out):
            assert tuple(got.shape) == (1, 3) and got.dtype == gs[k // 2].dtype and torch.equal(got.cpu(), torch.zeros(1, 3, dtype=got.dtype))
    return (lambda: [kk.mul_reduce(g, b, (1, 3)) for g, bb in zip(gs, bs) for b in (None, bb)]), check


ADDED = {
    'ada_tail:apply': ada_tail_apply_case,
    'ada_tail:params': ada_tail_params_case,
    'ops:mul_reduce_empty': mul_reduce_empty_case,
}


@gpu
@pytest.mark.parametrize('case', sorted(ADDED))
def test_initialising_entry_point(case):
    _finish(case, contained(ADDED[case], lambda out, check: check(out)))

# ------------------------------------------------------------------------------------------------
# coverage (host-only): every zeros / ones / full site of the package has a case, or a reason
# ------------------------------------------------------------------------------------------------
# (file, function) -> ids of GPU cases above that reach it; each of those cases asserts that the guard housed an allocation made there.
INIT_SITES = {
    ('ada.py', '__init__'): ['ada:forward', 'ada_tail:params'],
    ('ada.py', '_launch'): ['ada:adjoint'],
    ('ada.py', '_tail_launch'): ['ada_tail:apply'],
    ('ada.py', 'ada_tail_params'): ['ada_tail:params'],
    ('eval_harness.py', 'run_generator'): ['harness:eval_loop'],
    ('fid_stats.py', '__init__'): ['metrics:kid_is_fid'],
    ('grad_sync.py', '__init__'): ['optim:adam_ema'],
    ('image_metrics.py', '__init__'): ['metrics:psnr_ssim'],
    ('inception_score.py', 'new_accumulator'): ['metrics:kid_is_fid'],
    ('kernels.py', 'mul_reduce'): ['ops:mul_reduce_empty'],
    ('losses.py', '__init__'): ['module:loss_Dmain', 'module:loss_Gmain'],
    ('lpips.py', '__call__'): ['lpips:distance', 'lpips:vgg_distance'],
    ('masks.py', 'lama_rasterize'): ['masks:lama'],
    ('masks.py', 'rasterize'): ['harness:eval_loop', 'masks:freeform'],
    ('model_zoo/stylegan.py', '__init__'): ['fp32:downlayer_i_below_min', 'fp32:downlayer_i_eq_min', 'fp32:downlayer_poly_off'],
    ('optim.py', '__init__'): ['optim:adam_ema'],
    ('optim.py', '_ready'): ['optim:adam_ema'],
}

# (file, function) -> why no case houses the site
NOT_GUARDED = {
    ('ada.py', 'update'): "AdaController's 0-dim sample count, stacked with the sum of the signs by torch: no kernel of this project receives it",
    ('configs.py', 'seeded_init_'): "host-side initial values that torch's copy_ writes into an existing parameter; the cases build their seeded networks once per process, not in every run",
    ('configs.py', 'zero_or_noise'): "host-side initial values that torch's copy_ writes into an existing parameter; the cases build their seeded networks once per process, not in every run",
    ('evaluators.py', '__init__'): "this rank's result rows of the KID / LPIPS / precision-recall evaluators: torch's copy_ fills them row by row, and the LPIPS kernel that writes "
                                   "through an out= slice is the one lpips:distance runs into a housed buffer of the same kind",
    ('losses.py', '_style_mix'): "a scalar for torch.where on the line that draws the cutoff; the cases run with style mixing off to stay deterministic",
    ('model_zoo/shgan.py', '_adjoint_table'): 'a host table built once per process and size (the _ADJ_TABLE cache) and sent to the device: whichever test needs it first makes it, no case can claim it',
    ('model_zoo/shgan.py', 'build'): 'the zero bias substituted for a conv0 built without one; every configuration of the package builds conv0 with a bias',
    ('model_zoo/shgan.py', 'forward'): 'the start value of the plain-fma cold path of the heterogeneous filter, kept for drop-in completeness; the cases run the spectral stage, and ops:fma '
                                       'houses the operands of the kernel this path would launch',
    ('model_zoo/stylegan_utils/conv2d_gradfix.py', '_ones'): 'a table of ones cached per process and shape (_ONES): whichever test needs it first makes it, no case can claim it',
    ('model_zoo/stylegan_utils/fma.py', '_zero'): 'a 0-dim zero returned to autograd as the gradient of an operand that is not differentiated: never given to a kernel',
    ('model_zoo/stylegan_utils/upfirdn2d.py', 'upfirdn2d'): 'the 1 x 1 identity filter substituted for f=None; every caller in the package passes its filter',
    ('ppl.py', 'compute_ppl'): 'a [B, 0] label tensor and the result of zero sampling rounds: tensors of zero elements have no extent to overrun',
    ('ppl.py', 'path_distance'): 'the [B] float64 accumulator of lpips.head: the same launches into the same kind of buffer as lpips.py __call__, which lpips:distance and lpips:vgg_distance house',
    ('ppl.py', 'trimmed_mean'): "an operand of torch.where on sorted float64 distances: no kernel of this project receives it",
    ('train_stage.py', '__init__'): "PhaseGraphs' static inputs of a captured graph, written by torch's copy_ before each replay; the guard must not be active during a capture",
    ('train_stage.py', 'run_phases'): 'the [B, 0] label tensors substituted for c=None: tensors of zero elements have no extent to overrun',
}


def scan_initialising_sites():
    """(file, function) of every ``torch.zeros(`` / ``ones(`` / ``full(``, ``zeros_like(`` / ``ones_like(`` / ``full_like(`` and
    ``.new_zeros(`` / ``new_ones(`` / ``new_full(`` in sh-gan_amd/**/*.py (numpy's functions of the same names are not sites)."""
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
                    if isinstance(ch, ast.Call) and isinstance(ch.func, ast.Attribute):
                        f_ = ch.func
                        of_torch = isinstance(f_.value, ast.Name) and f_.value.id == 'torch'
                        if (f_.attr in ('zeros', 'ones', 'full', 'zeros_like', 'ones_like', 'full_like') and of_torch) or f_.attr in ('new_zeros', 'new_ones', 'new_full'):
                            found[(rel, func)] = found.get((rel, func), 0) + 1
                    visit(ch, inner)
            visit(tree, '<module>')
    return found


def test_every_initialising_site_has_a_case():
    found = scan_initialising_sites()
    assert sum(found.values()) >= 45 and len(found) >= 30, (len(found), sum(found.values()))        # the scan still finds the package
    both = set(INIT_SITES) & set(NOT_GUARDED)
    assert not both, f'listed twice: {sorted(both)}'
    missing = sorted(set(found) - set(INIT_SITES) - set(NOT_GUARDED))
    assert not missing, f'zeros / ones / full sites without a case in INIT_SITES or a reason in NOT_GUARDED: {missing}'
    stale = sorted((set(INIT_SITES) | set(NOT_GUARDED)) - set(found))
    assert not stale, f'listed, but the scan finds no such allocation there any more: {stale}'
    ids = TF.all_case_ids() | set(ADDED)
    for site, cases in INIT_SITES.items():
        assert cases and all(c in ids for c in cases), f'{site}: unknown case id among {cases}'
    for site, reason in NOT_GUARDED.items():
        assert len(reason) > 20 and 'not tested' not in reason.lower(), site
