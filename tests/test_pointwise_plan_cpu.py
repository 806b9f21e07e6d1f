"""The stride plans of ``kernels.fma`` and ``kernels.mul_reduce`` on the host (no GPU).

``kernels.fma_plan`` / ``kernels.mul_reduce_plan`` decide everything the kernels are told: which tensors' pointers they get, the collapsed
shape, one stride list per operand and, for the reduction, how many leading dimensions are kept and which mapping runs.  The emulator below
restates what ``fma_bcast_kernel`` and ``mul_reduce_kernel`` (csrc/pointwise.hip) do with those numbers -- ``ptr[sum_d i_d * stride_d]`` over
the row-major index of the collapsed shape -- with ``torch.as_strided`` on the CPU operands, in float64 on small integers, where every product
and sum is exact: the comparison with ``a * b + c`` and with ``torch.sum`` over the broadcast dimensions is ``torch.equal``.  A plan that
addresses an element outside an operand's storage makes ``as_strided`` raise, so an over-read is a finding here, without a launch."""
import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from shgan_amd import _lib, kernels

SWEEP = 300                 # seeded shape triples of the sweep
MAX_DIMS = 6                # SHG_BC_DIMS of csrc/pointwise.hip: the kernels decompose an index over at most six dimensions


# ------------------------------------------------------------------------------------------------
# the emulator
# ------------------------------------------------------------------------------------------------

def _strided(t, shape, strides):
    assert len(shape) == len(strides) <= MAX_DIMS, f'{len(shape)} sizes, {len(strides)} strides: the kernels take at most {MAX_DIMS} of each'
    return torch.as_strided(t, tuple(shape), tuple(strides), t.storage_offset())          # raises when the plan leaves the storage


def run_fma_plan(plan, has_c):
    """What fma_bcast_kernel writes for this plan: y[e] = a[ia] * b[ib] + c[ic] over the collapsed index, as the contiguous result."""
    assert len(plan.ops) == len(plan.strides) == (3 if has_c else 2)
    v = [_strided(t, plan.cshape, st) for t, st in zip(plan.ops, plan.strides)]
    y = v[0] * v[1]
    if has_c:
        y = y + v[2]
    return y.contiguous().reshape(tuple(plan.shape))


def run_mul_reduce_plan(plan, shape, dtype=torch.float64):
    """What mul_reduce_kernel writes: the kept dimensions come first and make the contiguous result, the rest is summed."""
    if plan.empty:
        return torch.zeros(tuple(shape), dtype=dtype)
    assert 0 <= plan.nk <= len(plan.cshape) and plan.inner_kept in (0, 1) and len(plan.ops) == len(plan.strides) in (1, 2)
    v = [_strided(t, plan.cshape, st) for t, st in zip(plan.ops, plan.strides)]
    p = v[0] * v[1] if len(v) == 2 else v[0]
    red = tuple(range(plan.nk, len(plan.cshape)))
    out = p.sum(red) if red else p.clone()
    return out.contiguous().reshape(tuple(shape))


def unbroadcast64(g, b, shape):
    """torch's ``_unbroadcast(g * b, shape)``: the sum over the leading extra dimensions and those where ``shape`` has 1."""
    p = g * b if b is not None else g
    full = (1,) * (g.ndim - len(shape)) + tuple(shape)
    dims = [i for i in range(g.ndim) if full[i] == 1]
    if dims:
        p = p.sum(dims, keepdim=True)
    return p.reshape(tuple(shape))


def fma_verdict(a, b, c, plan=None):
    """None when the emulated plan gives a * b + c, else what is wrong with it."""
    plan = kernels.fma_plan(a, b, c) if plan is None else plan
    ref = a * b + c if c is not None else a * b
    try:
        got = run_fma_plan(plan, c is not None)
    except (RuntimeError, AssertionError) as e:
        return f'not executable: {str(e)[:200]}'
    if tuple(got.shape) != tuple(ref.shape):
        return f'shape {tuple(got.shape)} for {tuple(ref.shape)}'
    return None if torch.equal(got, ref) else f'{int((got != ref).sum())} of {ref.numel()} elements differ'


def mul_reduce_verdict(g, b, shape, plan=None):
    plan = kernels.mul_reduce_plan(g, b, shape) if plan is None else plan
    ref = unbroadcast64(g, b, shape)
    try:
        got = run_mul_reduce_plan(plan, shape)
    except (RuntimeError, AssertionError) as e:
        return f'not executable: {str(e)[:200]}'
    return None if torch.equal(got, ref) else f'{int((got != ref).sum())} of {ref.numel()} elements differ'


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------

def ints(rs, shape):
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)).astype(np.float64))


def view_of(rs, shape, kind):
    """An integer-valued float64 tensor of ``shape`` that is: plain; an expanded size-1 operand; a transposed allocation; every second element
    of a wider allocation along one dimension; a contiguous view that starts inside its storage."""
    shape = tuple(shape)
    nd = len(shape)
    if kind == 'expanded' and nd:
        src = tuple(1 if rs.rand() < 0.5 else n for n in shape)
        return ints(rs, src).expand(shape)
    if kind == 'transposed' and nd >= 2:
        perm = list(rs.permutation(nd))
        return ints(rs, [shape[p] for p in perm]).permute([perm.index(i) for i in range(nd)])
    if kind == 'sliced' and nd:
        d = int(rs.randint(nd))
        wide = list(shape)
        wide[d] = 2 * shape[d] + 1
        return ints(rs, wide)[(slice(None),) * d + (slice(1, 1 + 2 * shape[d], 2),)]
    if kind == 'offset':
        n = int(np.prod(shape, dtype=np.int64))
        return ints(rs, (n + 5,))[3:3 + n].view(shape)
    return ints(rs, shape)


KINDS = ('plain', 'expanded', 'transposed', 'sliced', 'offset')


def _full_shape(rs):
    nd = int(rs.randint(0, 9))
    return tuple(0 if rs.rand() < 0.04 else int(rs.choice([1, 2, 2, 3, 3])) for _ in range(nd))


def _operand_shape(rs, full):
    """A shape that broadcasts to ``full``: some leading dimensions dropped, some extents 1."""
    drop = int(rs.randint(0, len(full) + 1)) if rs.rand() < 0.4 else 0
    return tuple(1 if rs.rand() < 0.4 else n for n in full[drop:])


def triple(seed):
    """Operands of one fma: 0 to 8 dimensions, extents 0 to 3, at least one operand of the full shape, every kind of view."""
    rs = np.random.RandomState(1000 + seed)
    full = _full_shape(rs)
    shapes = [full, _operand_shape(rs, full), _operand_shape(rs, full)]
    order = rs.permutation(3)
    ops = [view_of(rs, shapes[k], KINDS[int(rs.randint(len(KINDS)))]) for k in order]
    return ops[0], ops[1], (ops[2] if seed % 7 else None)


def reduction(seed):
    """(g, b | None, shape) of one mul_reduce: g of the full shape, b broadcast to it, ``shape`` an operand shape with 1s and dropped dimensions."""
    rs = np.random.RandomState(5000 + seed)
    full = _full_shape(rs)
    if seed % 10 == 3:                                            # kept and reduced dimensions interleaved, seven or eight of them
        full = tuple(int(rs.choice([2, 3])) for _ in range(7 + seed // 10 % 2))
        g = view_of(rs, full, KINDS[int(rs.randint(len(KINDS)))])
        b = view_of(rs, tuple(1 if rs.rand() < 0.3 else n for n in full), 'plain')
        return g, b, tuple(n if (i + seed // 20) % 2 else 1 for i, n in enumerate(full))
    g = view_of(rs, full, KINDS[int(rs.randint(len(KINDS)))])
    b = None if seed % 5 == 0 else view_of(rs, _operand_shape(rs, full), KINDS[int(rs.randint(len(KINDS)))])
    return g, b, _operand_shape(rs, full)


# ------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------

def test_sweep_of_fma_plans():
    seen = {'fallback': 0, 'six': 0, 'empty': 0, 'scalar': 0}
    for seed in range(SWEEP):
        a, b, c = triple(seed)
        plan = kernels.fma_plan(a, b, c)
        seen['fallback'] += len(kernels._collapse(plan.shape, [t.expand(plan.shape).stride() for t in (a, b, c) if t is not None])[0]) > MAX_DIMS
        seen['six'] += len(plan.cshape) == MAX_DIMS
        seen['empty'] += 0 in plan.shape
        seen['scalar'] += len(plan.cshape) == 0
        why = fma_verdict(a, b, c, plan)
        assert why is None, f'seed {seed}: a {tuple(a.shape)}/{a.stride()} b {tuple(b.shape)}/{b.stride()} c {None if c is None else tuple(c.shape)}: {why}'
    print(f'PLAN_SWEEP fma {seen}')
    assert min(seen.values()) > 0, f'the sweep no longer reaches every form: {seen}'


def test_sweep_of_mul_reduce_plans():
    seen = {'permuted': 0, 'both_mappings': set(), 'empty_to_zeros': 0, 'no_reduction': 0, 'all_reduced': 0}
    for seed in range(SWEEP):
        g, b, shape = reduction(seed)
        plan = kernels.mul_reduce_plan(g, b, shape)
        seen['permuted'] += len(plan.cshape) <= 2 and plan.ops[0].data_ptr() != g.data_ptr() and not plan.ops[0].is_contiguous()
        seen['both_mappings'].add(plan.inner_kept)
        seen['empty_to_zeros'] += bool(plan.empty)
        seen['no_reduction'] += plan.nk == len(plan.cshape)
        seen['all_reduced'] += plan.nk == 0 and len(plan.cshape) > 0
        why = mul_reduce_verdict(g, b, shape, plan)
        assert why is None, f'seed {seed}: g {tuple(g.shape)}/{g.stride()} b {None if b is None else (tuple(b.shape), b.stride())} -> {shape}: {why}'
    print(f'PLAN_SWEEP mul_reduce {seen}')
    assert seen['both_mappings'] == {0, 1} and all(v for v in seen.values()), f'the sweep no longer reaches every form: {seen}'


# ------------------------------------------------------------------------------------------------
# the named cases
# ------------------------------------------------------------------------------------------------
SIX = ((2, 3, 2, 3, 2, 3), (1, 3, 1, 3, 1, 3), (2, 1, 2, 1, 2, 1))
SEVEN = ((2, 3, 2, 3, 2, 3, 2), (1, 3, 1, 3, 1, 3, 1), (2, 1, 2, 1, 2, 1, 2))


def _named(shapes, seed=7):
    rs = np.random.RandomState(seed)
    return [ints(rs, s) for s in shapes]


def test_fma_exactly_six_dimensions_are_read_in_place():
    a, b, c = _named(SIX)
    plan = kernels.fma_plan(a, b, c)
    assert plan.cshape == [2, 3, 2, 3, 2, 3] and [t.data_ptr() for t in plan.ops] == [a.data_ptr(), b.data_ptr(), c.data_ptr()]
    assert plan.strides[1] == [0, 3, 0, 1, 0, 0] or plan.strides[1] == [0, 9, 0, 3, 0, 1]
    assert fma_verdict(a, b, c, plan) is None


def test_fma_seven_dimensions_take_the_fallback_inside_the_copies():
    a, b, c = _named(SEVEN)
    plan = kernels.fma_plan(a, b, c)
    assert plan.cshape == [a.numel()] and plan.strides == [[1], [1], [1]]
    assert all(t.is_contiguous() and tuple(t.shape) == tuple(a.shape) for t in plan.ops), 'the pointers must be those of the expanded copies'
    assert fma_verdict(a, b, c, plan) is None
    assert fma_verdict(a, b, None) is None


def test_seven_dimension_backward_plans():
    """The three gradients of the public op at SEVEN: db keeps 3 dimensions and reduces 4 interleaved ones, which no copy in the original
    order brings below seven; the copy with the kept dimensions in front leaves two."""
    a, b, c = _named(SEVEN)
    go = ints(np.random.RandomState(8), SEVEN[0])
    for other, t in ((b, a), (a, b), (None, c)):
        plan = kernels.mul_reduce_plan(go, other, t.shape)
        assert len(plan.cshape) <= MAX_DIMS
        assert mul_reduce_verdict(go, other, t.shape, plan) is None
    plan = kernels.mul_reduce_plan(go, a, b.shape)
    assert plan.cshape == [27, 16] and plan.nk == 1 and plan.inner_kept == 0 and plan.strides == [[16, 1], [16, 1]]
    for width in (7, 8):                                          # transposed on top: neither operand is contiguous to begin with
        shp = SEVEN[0] + (2,) * (width - 7)
        g = ints(np.random.RandomState(9), shp[::-1]).permute(*range(width - 1, -1, -1))
        bb = ints(np.random.RandomState(10), tuple(1 if i % 2 else n for i, n in enumerate(shp)))
        assert mul_reduce_verdict(g, bb, tuple(n if i % 2 else 1 for i, n in enumerate(shp))) is None


def test_empty_reduction_gives_zeros():
    g = torch.zeros(0, 3, dtype=torch.float64)
    for b in (None, torch.ones(1, 3, dtype=torch.float64)):
        plan = kernels.mul_reduce_plan(g, b, (1, 3))
        assert plan.empty
        assert torch.equal(run_mul_reduce_plan(plan, (1, 3)), unbroadcast64(g, b, (1, 3))) and unbroadcast64(g, b, (1, 3)).abs().sum() == 0
    assert not kernels.mul_reduce_plan(g, None, (0, 3)).empty                 # nothing to return: nothing to fill
    assert not kernels.mul_reduce_plan(torch.ones(2, 3), None, (1, 3)).empty


def test_scalars_and_absent_operands():
    rs = np.random.RandomState(11)
    s = [ints(rs, ()) for _ in range(3)]
    plan = kernels.fma_plan(*s)
    assert plan.cshape == [] and plan.strides == [[], [], []] and fma_verdict(*s, plan=plan) is None
    one = [ints(rs, (1, 1)), ints(rs, (1,)), ints(rs, ())]
    assert kernels.fma_plan(*one).cshape == [] and fma_verdict(*one) is None
    a, b = ints(rs, (4, 1, 3)), ints(rs, (2, 1, 5, 1))
    plan = kernels.fma_plan(a, b, None)
    assert len(plan.ops) == len(plan.strides) == 2 and fma_verdict(a, b, None, plan) is None
    g = ints(rs, (4, 2, 3))
    plan = kernels.mul_reduce_plan(g, None, (2, 1))
    assert len(plan.ops) == len(plan.strides) == 1 and mul_reduce_verdict(g, None, (2, 1), plan) is None
    assert mul_reduce_verdict(s[0], s[1], ()) is None and mul_reduce_verdict(s[0], None, ()) is None
    assert mul_reduce_verdict(g, s[0], ()) is None                            # everything reduced: nk = 0


def test_mul_reduce_plan_rejects_what_does_not_broadcast():
    g = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(_lib.ShgError, match='does not broadcast'):
        kernels.mul_reduce_plan(g, None, (2, 2))
    with pytest.raises(_lib.ShgError, match='fewer dimensions'):
        kernels.mul_reduce_plan(g, None, (1, 2, 3))


# ------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_r6_ops.py and ``ops:fma`` of tests/test_gpu_alloc_fill.py: the plans the previous revision computed for them
# (collapsed shape, strides of a / b / c; then per gradient da, db, dc: collapsed shape, strides of g [and the other factor], nk, inner_kept),
# recorded from it.  The kernels are unchanged, so equal plans are equal results, bit for bit.
# ------------------------------------------------------------------------------------------------
R6_CASES = {
    'x_d_noise': ((2, 5, 6, 7), (2, 5, 1, 1), (2, 1, 6, 7)),
    'x_d_noise_hw': ((2, 5, 6, 7), (2, 5, 1, 1), (6, 7)),
    'same': ((3, 4), (3, 4), (3, 4)),
    'corners': ((4, 1, 3), (2, 1, 5, 1), (5, 3)),
    'scalar_c': ((1,), (2, 3), ()),
    'c_enlarges': ((2, 3), (1,), (4, 2, 3)),
    'large_per_sample': ((3, 40, 64, 64), (3, 40, 1, 1), (3, 1, 64, 64)),
    'large_hw': ((3, 40, 64, 64), (3, 40, 1, 1), (64, 64)),
    'ops_fma': ((2, 5, 6, 12), (2, 5, 1, 1), (2, 1, 6, 12)),
}

RECORDED = {
    'c_enlarges': ([4, 6], [[0, 1], [0, 0], [6, 1]], [([6, 4], [[1, 6], [0, 0]], 1, 1), ([4, 6], [[6, 1], [0, 1]], 0, 0), ([24], [[1]], 1, 1)]),
    'corners': ([2, 4, 5, 3], [[0, 3, 0, 1], [5, 0, 1, 0], [0, 0, 3, 1]],
                [([4, 3, 2, 5], [[15, 1, 60, 3], [0, 0, 5, 1]], 2, 1), ([2, 5, 4, 3], [[60, 3, 15, 1], [0, 0, 3, 1]], 2, 0), ([15, 8], [[1, 15]], 1, 1)]),
    'large_hw': ([120, 4096], [[4096, 1], [1, 0], [0, 1]],
                 [([120, 4096], [[4096, 1], [1, 0]], 2, 1), ([120, 4096], [[4096, 1], [4096, 1]], 1, 0), ([4096, 120], [[1, 4096]], 1, 1)]),
    'large_per_sample': ([3, 40, 4096], [[163840, 4096, 1], [40, 1, 0], [4096, 0, 1]],
                         [([120, 4096], [[4096, 1], [1, 0]], 2, 1), ([120, 4096], [[4096, 1], [4096, 1]], 1, 0), ([3, 4096, 40], [[163840, 1, 4096]], 2, 1)]),
    'ops_fma': ([2, 5, 72], [[360, 72, 1], [5, 1, 0], [72, 0, 1]],
                [([10, 72], [[72, 1], [1, 0]], 2, 1), ([10, 72], [[72, 1], [72, 1]], 1, 0), ([2, 72, 5], [[360, 1, 72]], 2, 1)]),
    'same': ([12], [[1], [1], [1]], [([12], [[1], [1]], 1, 1), ([12], [[1], [1]], 1, 1), ([12], [[1]], 1, 1)]),
    'scalar_c': ([6], [[0], [1], [0]], [([6], [[1], [1]], 0, 0), ([6], [[1], [0]], 1, 1), ([6], [[1]], 0, 0)]),
    'x_d_noise': ([2, 5, 42], [[210, 42, 1], [5, 1, 0], [42, 0, 1]],
                  [([10, 42], [[42, 1], [1, 0]], 2, 1), ([10, 42], [[42, 1], [42, 1]], 1, 0), ([2, 42, 5], [[210, 1, 42]], 2, 1)]),
    'x_d_noise_hw': ([10, 42], [[42, 1], [1, 0], [0, 1]],
                     [([10, 42], [[42, 1], [1, 0]], 2, 1), ([10, 42], [[42, 1], [42, 1]], 1, 0), ([42, 10], [[1, 42]], 1, 1)]),
}


def _current_rule(cshape, sg, nk):
    """inner_kept as csrc/pointwise.hip describes it: 1 when there is nothing to reduce, or when the smallest non-zero stride of g among the
    kept dimensions is below the smallest among the reduced ones (a thread per output reads neighbouring addresses)."""
    k = [abs(s) for s in sg[:nk] if s]
    r = [abs(s) for s in sg[nk:] if s]
    if len(cshape) == nk:
        return 1
    return int(bool(nk) and (min(k) if k else float('inf')) < (min(r) if r else float('inf')))


@pytest.mark.parametrize('name', sorted(R6_CASES))
def test_plans_of_the_existing_cases_are_the_recorded_ones(name):
    sa, sb, sc = R6_CASES[name]
    a, b, c = (torch.zeros(s, dtype=torch.float64) for s in (sa, sb, sc))
    cshape, strides, grads = RECORDED[name]
    plan = kernels.fma_plan(a, b, c)
    assert (plan.cshape, plan.strides) == (cshape, strides) and [t.data_ptr() for t in plan.ops] == [a.data_ptr(), b.data_ptr(), c.data_ptr()]
    go = torch.zeros(tuple(plan.shape), dtype=torch.float64)
    for (other, shp), (rshape, rstrides, nk, inner_kept) in zip(((b, sa), (a, sb), (None, sc)), grads):
        p = kernels.mul_reduce_plan(go, other, shp)
        assert (p.cshape, p.strides, p.nk, p.inner_kept, p.empty) == (rshape, rstrides, nk, inner_kept, False), (name, shp, p)
        assert p.ops[0].data_ptr() == go.data_ptr() and (other is None or p.ops[1].data_ptr() == other.data_ptr())
        assert p.inner_kept == _current_rule(p.cshape, p.strides[0], p.nk)


def test_plan_of_the_strided_case_is_the_recorded_one():
    """The operands of test_fma_strided_and_expanded_operands_are_read_in_place: a channel slice with a column stride, an expanded
    operand and a transposed view, read where they lie."""
    a = torch.zeros(2, 8, 6, 10)[:, 2:7, :, ::2]
    b = torch.zeros(2, 5, 1, 1).expand(2, 5, 6, 5)
    c = torch.zeros(5, 6).t().contiguous().t()[None, None].transpose(2, 3)
    plan = kernels.fma_plan(a, b, c)
    assert (plan.cshape, plan.strides) == ([2, 5, 30], [[480, 60, 2], [5, 1, 0], [0, 0, 1]])
    assert [t.data_ptr() for t in plan.ops] == [a.data_ptr(), b.data_ptr(), c.data_ptr()] and a.storage_offset() == 120


def test_inner_kept_follows_the_rule_over_the_sweep():
    for seed in range(SWEEP):
        g, b, shape = reduction(seed)
        p = kernels.mul_reduce_plan(g, b, shape)
        assert p.inner_kept == _current_rule(p.cshape, p.strides[0], p.nk), seed
        full = (1,) * (g.ndim - len(shape)) + tuple(shape)
        kept = int(np.prod([n for n, f in zip(g.shape, full) if not (n > 1 and f == 1)], dtype=np.int64))
        assert int(np.prod(p.cshape[:p.nk], dtype=np.int64)) == kept, seed          # nk splits the sizes where the result's extent ends


# ------------------------------------------------------------------------------------------------
# the judge on stand-ins: plans that are wrong in known ways must be rejected
# ------------------------------------------------------------------------------------------------

def test_the_judge_on_host_stand_ins():
    """(a) The previous revision's fallback -- strides [1] over the ORIGINAL tensors -- leaves the storage of the two broadcast operands;
    (b) two strides of one operand exchanged read the wrong elements; (c) nk one too small or too large reduces the wrong dimensions.  The
    plans the package computes for the same operands pass."""
    a, b, c = _named(SEVEN)
    good = kernels.fma_plan(a, b, c)
    assert fma_verdict(a, b, c, good) is None
    old = kernels.FmaPlan(good.shape, [a, b, c], [a.numel()], [[1], [1], [1]])
    why = fma_verdict(a, b, c, old)
    assert why is not None and 'not executable' in why and 'out of bounds for storage' in why, why
    for k in (1, 2):                                              # each broadcast operand on its own is enough
        ops = list(good.ops)
        ops[k] = (a, b, c)[k]
        assert 'out of bounds' in (fma_verdict(a, b, c, good._replace(ops=ops)) or '')

    a, b, c = _named(SIX)
    good = kernels.fma_plan(a, b, c)
    assert fma_verdict(a, b, c, good) is None
    for k in range(3):
        st = [list(s) for s in good.strides]
        st[k][0], st[k][1] = st[k][1], st[k][0]
        why = fma_verdict(a, b, c, good._replace(strides=st))
        assert why is not None and ('differ' in why or 'out of bounds' in why), (k, why)

    go = ints(np.random.RandomState(12), SIX[0])
    for other, shp in ((b, SIX[0]), (a, SIX[1]), (None, SIX[2]), (a, (3,))):
        good = kernels.mul_reduce_plan(go, other, shp)
        assert mul_reduce_verdict(go, other, shp, good) is None
        for nk in (good.nk - 1, good.nk + 1):
            if 0 <= nk <= len(good.cshape):
                why = mul_reduce_verdict(go, other, shp, good._replace(nk=nk))
                assert why is not None, (shp, nk)
        st = [list(s) for s in good.strides]
        if len(st[0]) >= 2 and st[0][0] != st[0][-1]:
            st[0][0], st[0][-1] = st[0][-1], st[0][0]
            assert mul_reduce_verdict(go, other, shp, good._replace(strides=st)) is not None, shp
