"""Host side of the training tail (sh-gan_amd/optim.py, csrc/optim.hip): the float64 yardstick against torch, segment tables against a
brute-force enumeration, the torch-layout state dict, what raises, the exported symbols.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from shgan_amd import _lib, optim
from shgan_amd.grad_sync import BucketedAllReduce

import adam_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('shg_adam_tick', 'shg_adam_buckets_f32', 'shg_ema_lerp_f32')
LAZY = 0.99 ** (16 / 17)


def make_params(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


@pytest.mark.parametrize('betas', [(0.0, LAZY), (0.9, 0.999)])
def test_yardstick_equals_torch_adam_in_float64(betas):
    """adam_f64 (average -> sanitise -> Adam) against torch.optim.Adam(foreach=False) on float64 tensors over six steps, with NaN, the
    infinities, denormals and zeros in the buckets and a step without a gradient; and the lerp against torch's in float64."""
    rs = np.random.RandomState(3)
    p0 = rs.standard_normal(257)
    p_t = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p_t], lr=0.002 * 16 / 17, betas=betas, eps=1e-8, foreach=False)
    p, m, v, t = p0.copy(), np.zeros(257), np.zeros(257), 0
    for step in range(6):
        bucket = rs.standard_normal(257).astype(np.float32)
        bucket[:6] = [np.nan, np.inf, -np.inf, 1e-41, 0.0, -0.0]
        if step == 3:                                   # no gradient: nothing moves
            p_t.grad = None
            opt.step()
            continue
        g = adam_f64.sanitize_f64(bucket, world=3)
        want_g = torch.nan_to_num(torch.tensor(bucket, dtype=torch.float64) / 3, nan=0.0, posinf=1e5, neginf=-1e5)
        assert np.array_equal(g, want_g.numpy())
        p_t.grad = want_g.clone()
        opt.step()
        p, m, v, t = adam_f64.adam_step_f64(p, g, m, v, t, 0.002 * 16 / 17, betas[0], betas[1], 1e-8)
    st = opt.state[p_t]
    assert int(st['step']) == t == 5
    for name, a, b in (('p', p, p_t), ('exp_avg', m, st['exp_avg']), ('exp_avg_sq', v, st['exp_avg_sq'])):
        err = adam_f64.rel_err(a, b.detach().numpy())
        assert err < 2e-15, (name, err)
    a, b = rs.standard_normal(100), rs.standard_normal(100)
    for beta in (0.0, 0.3, 0.998):
        want = torch.tensor(b).lerp(torch.tensor(a), beta).numpy()
        assert adam_f64.rel_err(adam_f64.ema_f64(a, b, beta), want) < 2e-15


def brute_force_chunks(numels):
    """(segment, first element, elements) of every chunk, by enumeration."""
    out = []
    for s, n in enumerate(numels):
        for e in range(0, n, optim.CHUNK):
            out.append((s, e, min(optim.CHUNK, n - e)))
    return out


def test_segment_tables_against_brute_force():
    """ShgAdam's table over buckets that split (1-element parameters, odd offsets, a parameter of several chunks): every row points at
    its parameter and at the same offset of the bucket and of both moment buffers, the chunk column enumerates ceil(n / CHUNK) chunks per
    segment, the touched column follows the set."""
    shapes = [(1,), (3,), (7, 9), (1,), (4,), (5,), (1023,), (1025,), (3 * optim.CHUNK + 1,), (2, optim.CHUNK)]
    params = make_params(shapes)
    opt = optim.ShgAdam(params, lr=0.01, betas=(0.0, 0.99), bucket_bytes=4 * 9000)
    sync = opt.sync
    assert len(sync.buckets) >= 3                                     # the layout splits
    touched = frozenset(id(p) for p in params[::2])
    tab = opt.host_table(touched)
    assert tab.shape == (len(params) + 1, optim.ADAM_ROW)
    order = sorted(params, key=lambda p: sync.slot(p)[:2])
    chunks = brute_force_chunks([p.numel() for p in order])
    assert tab[-1, -1] == len(chunks)
    odd = 0
    for i, p in enumerate(order):
        bi, off, n = sync.slot(p)
        odd += off % 2
        row = tab[i]
        assert row[0] == p.data_ptr() and row[4] == n == p.numel()
        assert row[1] == sync.buckets[bi].data_ptr() + 4 * off == p.grad.data_ptr()
        assert row[2] == opt.exp_avg[bi].data_ptr() + 4 * off == opt.state[p]['exp_avg'].data_ptr()
        assert row[3] == opt.exp_avg_sq[bi].data_ptr() + 4 * off == opt.state[p]['exp_avg_sq'].data_ptr()
        assert row[5] == (1 if id(p) in touched else 0) and row[6] == i and row[7] == 0
        assert [c for c in range(len(chunks)) if chunks[c][0] == i] == list(range(row[-1], tab[i + 1, -1]))
    assert odd > 0
    assert opt.host_table(None)[:-1, 5].all()
    for c, (s, e, n) in enumerate(chunks):                            # the bisection the kernels do
        assert int(np.searchsorted(tab[:-1, -1], c, side='right')) - 1 == s
    # two groups: the group column
    opt2 = optim.ShgAdam([{'params': params[:4]}, {'params': params[4:], 'lr': 0.5}], lr=0.01, sync=sync)
    t2 = opt2.host_table(None)
    assert {int(r[7]) for r in t2[:-1] if r[0] in {p.data_ptr() for p in params[4:]}} == {1}
    pairs = [(p.data_ptr(), q.data_ptr(), p.numel(), optim.EMA_LERP) for p, q in zip(params, make_params(shapes, 1))]
    et = optim.build_ema_table(pairs)
    assert et[-1, -1] == len(brute_force_chunks([p.numel() for p in params])) and list(et[:-1, 2]) == [p.numel() for p in params]


def test_out_of_range_table_entries_are_rejected_on_the_host():
    params = make_params([(5,), (1025,), (3,)])
    opt = optim.ShgAdam(params, lr=0.01, bucket_bytes=4 * 1030)
    good = opt.host_table(None)
    bases = [(g.data_ptr(), m.data_ptr(), v.data_ptr(), g.numel()) for g, m, v in zip(opt.sync.buckets, opt.exp_avg, opt.exp_avg_sq)]
    optim.validate_adam_table(good, bases, 3, 1)

    def bad(edit, match):
        t = good.copy()
        edit(t)
        with pytest.raises(_lib.ShgError, match=match):
            optim.validate_adam_table(t, bases, 3, 1)
    bad(lambda t: t.__setitem__((0, 4), t[0, 4] + 4000), 'leaves its bucket|chunk column')
    bad(lambda t: t.__setitem__((1, 1), t[1, 1] + 16), 'leaves its bucket|congruent')
    bad(lambda t: t.__setitem__((1, 2), t[1, 2] + 16), 'leaves its bucket|congruent')
    bad(lambda t: t.__setitem__((0, 1), t[0, 1] - 4096), 'leaves its bucket|congruent')
    bad(lambda t: t.__setitem__((0, 4), 0), 'elements')
    bad(lambda t: t.__setitem__((0, 0), t[0, 0] + 2), 'misaligned')
    bad(lambda t: t.__setitem__((2, 6), 3), 'scalar slot')
    bad(lambda t: t.__setitem__((2, 6), t[1, 6]), 'scalar slot')
    bad(lambda t: t.__setitem__((1, 7), 1), 'group')
    bad(lambda t: t.__setitem__((1, 5), 2), 'touched')
    bad(lambda t: t.__setitem__((-1, -1), t[-1, -1] + 1), 'chunk column')
    bad(lambda t: t.__setitem__((1, -1), 5), 'chunk column')
    with pytest.raises(_lib.ShgError):
        optim.validate_adam_table(good.astype(np.int32), bases, 3, 1)
    with pytest.raises(_lib.ShgError, match='bucket'):
        optim.build_adam_table([(params[0].data_ptr(), 7, 0, 5, 0, 0)], bases)
    a, b = torch.zeros(10), torch.zeros(10)
    ext = [(a.data_ptr(), 40), (b.data_ptr(), 40)]
    et = optim.build_ema_table([(a.data_ptr(), b.data_ptr(), 10, optim.EMA_LERP)])
    optim.validate_ema_table(et, ext)
    for col, val, match in ((2, 11, 'leaves|chunk'), (2, 0, 'malformed'), (3, 2, 'malformed'), (1, b.data_ptr() + 4, 'leaves'), (0, a.data_ptr() + 1, 'malformed')):
        t = et.copy()
        t[0, col] = val
        with pytest.raises(_lib.ShgError, match=match):
            optim.validate_ema_table(t, ext)
    # the C entry points check their scalars before any launch, too
    lib = _lib.get_lib()
    one = ctypes.c_void_p(16)
    assert lib.shg_adam_buckets_f32(None, 1, 1, one, 1.0, 0, 1, None) == -1
    assert lib.shg_adam_buckets_f32(one, 0, 1, one, 1.0, 0, 1, None) == -1
    assert lib.shg_adam_buckets_f32(one, 2, 1, one, 1.0, 0, 1, None) == -1
    assert lib.shg_adam_buckets_f32(one, 1, 1, one, 2.5, 1, 1, None) == -1
    assert lib.shg_adam_buckets_f32(one, 1, 1, one, 2.0, 3, 1, None) == -1
    assert lib.shg_adam_tick(one, 1, None, 1, one, one, None) == -1 and lib.shg_adam_tick(one, 1, one, 0, one, one, None) == -1
    assert lib.shg_ema_lerp_f32(one, 1, 1, None, None) == -1 and lib.shg_ema_lerp_f32(one, 3, 2, one, None) == -1


def test_state_dict_round_trip_through_torch_adam_both_ways():
    """torch.optim.Adam -> ShgAdam -> torch.optim.Adam: the moments land at their bucket offsets, steps on the device counters, and a
    torch optimiser that loads our state dict continues exactly like the one that never left."""
    shapes = [(3,), (7, 9), (1,), (130,)]
    kw = dict(lr=0.003, betas=(0.5, 0.99), eps=1e-8)
    pa = make_params(shapes)
    ta = torch.optim.Adam(pa, **kw)
    rs = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in pa[:3]:                                   # the last parameter never gets a gradient: no entry in torch's state
            p.grad = torch.randn(p.shape, generator=rs)
        ta.step()
    sd = ta.state_dict()
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ours = optim.ShgAdam(pb, lr=1.0, betas=(0.1, 0.2), eps=1.0, bucket_bytes=4 * 64)
    ours.load_state_dict(sd)
    assert ours.param_groups[0]['lr'] == 0.003 and tuple(ours.param_groups[0]['betas']) == (0.5, 0.99)
    for i, p in enumerate(pb):
        bi, off, n = ours.sync.slot(p)
        st = ours.state[p]
        want = ta.state[pa[i]] if i < 3 else {'step': torch.tensor(0.0), 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)}
        assert float(st['step']) == float(want['step'])
        assert torch.equal(st['exp_avg'], want['exp_avg']) and torch.equal(st['exp_avg_sq'], want['exp_avg_sq'])
        assert st['exp_avg'].data_ptr() == ours.exp_avg[bi].data_ptr() + 4 * off            # views of the flat buffers
        assert torch.equal(ours.exp_avg_sq[bi][off:off + n], want['exp_avg_sq'].reshape(-1))
    back = ours.state_dict()
    assert set(back) == {'state', 'param_groups'} and set(back['state']) == {0, 1, 2, 3}
    assert set(back['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert set(back['param_groups'][0]) == set(sd['param_groups'][0])                       # torch's keys, all of them
    assert back['state'][1]['exp_avg'].data_ptr() != ours.state[pb[1]]['exp_avg'].data_ptr()      # copies
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    tc = torch.optim.Adam(pc, lr=9.0)
    tc.load_state_dict(back)
    for _ in range(2):
        for a, c in zip(pa, pc):
            a.grad = torch.randn(a.shape, generator=rs)
            c.grad = a.grad.clone()
        ta.step()
        tc.step()
    for a, c in zip(pa, pc):
        assert torch.equal(a, c)
        assert torch.equal(ta.state[a]['exp_avg_sq'], tc.state[c]['exp_avg_sq']) and float(ta.state[a]['step']) == float(tc.state[c]['step'])
    sd2 = ta.state_dict()
    sd2['state'][0]['step'] = 5                            # a number, as old checkpoints carry it
    ours.load_state_dict(sd2)
    assert float(ours.state[pb[0]]['step']) == 5.0


def test_every_unsupported_option_raises():
    p = make_params([(4,)])
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(differentiable=True), dict(foreach=True),
               dict(fused=True), dict(lr=torch.tensor(0.1)), dict(betas=(1.0, 0.9)), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            optim.ShgAdam(p, **kw)
    for bad in (torch.nn.Parameter(torch.zeros(4, dtype=torch.float64)), torch.nn.Parameter(torch.zeros(4, dtype=torch.float16)),
                torch.nn.Parameter(torch.zeros(4, 4).t())):
        with pytest.raises(TypeError):
            optim.ShgAdam([bad])
    other = BucketedAllReduce(make_params([(4,)]))
    with pytest.raises(ValueError, match='not in the gradient buckets'):
        optim.ShgAdam(p, sync=other)
    opt = optim.ShgAdam(p, lr=0.1)
    with pytest.raises(_lib.ShgError, match='no CPU path'):            # never a silent fallback
        opt.step()
    opt.param_groups[0]['weight_decay'] = 0.5                          # set after construction: caught at the step
    with pytest.raises((ValueError, _lib.ShgError)):
        opt.step_from_buckets()
    sd = torch.optim.Adam(make_params([(4,)]), amsgrad=True).state_dict()
    with pytest.raises(ValueError):
        optim.ShgAdam(make_params([(4,)])).load_state_dict(sd)
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 3)
    with pytest.raises(ValueError):
        optim.EmaUpdater(a, b)
    with pytest.raises(TypeError):
        optim.EmaUpdater(torch.nn.Linear(3, 2).double(), torch.nn.Linear(3, 2).double())
    ema = optim.EmaUpdater(torch.nn.Linear(3, 2), torch.nn.Linear(3, 2))
    with pytest.raises(_lib.ShgError, match='no CPU path'):
        ema.update(32, 1000)


def test_make_phases_hands_the_buckets_to_the_optimiser_and_keeps_torch_as_it_was():
    from shgan_amd import train_stage as ts
    G, D = torch.nn.Linear(4, 3), torch.nn.Linear(3, 1)
    kw = dict(lr=0.002, betas=(0.0, 0.99), eps=1e-8)
    phases = ts.make_phases(G, D, kw, kw, opt_class=optim.ShgAdam)
    assert [ph.name for ph in phases] == ['Gmain', 'Greg', 'Dmain', 'Dreg']
    assert phases[0].opt is phases[1].opt and phases[0].sync is phases[1].sync is phases[0].opt.sync
    assert phases[0].opt.param_groups[0]['lr'] == pytest.approx(0.002 * 4 / 5) and phases[2].opt.param_groups[0]['betas'][1] == pytest.approx(0.99 ** (16 / 17))
    torch_phases = ts.make_phases(torch.nn.Linear(4, 3), torch.nn.Linear(3, 1), kw, kw)
    assert type(torch_phases[0].opt) is torch.optim.Adam and torch_phases[0].sync is None


def test_exports_signatures_and_abi_number():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40 and _lib.get_lib().shg_abi_version() == 40     # symbols were added, nothing changed
    for macro, val in (('SHG_OPT_CHUNK', optim.CHUNK), ('SHG_ADAM_ROW', optim.ADAM_ROW), ('SHG_ADAM_SCALARS', optim.ADAM_SCALARS),
                       ('SHG_EMA_ROW', optim.EMA_ROW)):
        assert re.search(r'#define %s %d\b' % (macro, val), hdr), macro
