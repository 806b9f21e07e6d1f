"""CPU (no GPU): the host side of a training run -- symbols and table validators of the statistics kernels, ``Collector`` arithmetic on
hand-made tables (the launch replaced by the float64 numpy yardstick, tests/train_stats_f64.py), the tick block of ``train`` against a
stand-in loss, snapshots (round trip, atomic write, version / world checks) and a bit-exact resume with ``torch.optim.Adam``."""
import copy
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
import train_stats_f64 as y
from conftest import ROOT
from shgan_amd import _lib, ada, optim, train_stage as ts, training_stats as tstats
from shgan_amd._lib import ShgError

NEW = ('shg_stats_moments_f64', 'shg_adam_buckets_health_f32', 'shg_health_reduce_f64', 'shg_image_grid_u8')


def test_symbols_declared_exported_and_the_abi_stays_40():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40 and _lib.get_lib().shg_abi_version() == 40
    assert tstats.STATS_ROW == 4 and optim.HEALTH_COLS == 5 and '#define SHG_STATS_ROW 4' in hdr and '#define SHG_HEALTH_COLS 5' in hdr


def test_host_argument_checks_of_the_new_entry_points():
    """Argument checks are host code: they return before any launch."""
    lib = _lib.get_lib()
    p = ctypes.c_void_p(64)
    assert lib.shg_stats_moments_f64(p, 0, p, 4, None) == 0                  # rows = 0: nothing to do
    assert lib.shg_stats_moments_f64(p, -1, p, 4, None) == -1 and lib.shg_stats_moments_f64(p, 1, p, 0, None) == -1
    assert lib.shg_stats_moments_f64(None, 1, p, 4, None) == -1
    assert lib.shg_adam_buckets_health_f32(p, 1, 1, p, 1.0, 0, 1, None, None) == -1
    assert lib.shg_adam_buckets_health_f32(p, 2, 1, p, 1.0, 0, 1, p, None) == -1
    assert lib.shg_health_reduce_f64(p, 1, 1, p, p, None, None) == -1
    assert lib.shg_image_grid_u8(p, None, None, p, 2, 4, 4, 1, 1, 0.0, 1.0, None) == -1       # C = 2
    assert lib.shg_image_grid_u8(p, p, None, p, 3, 4, 4, 1, 1, 0.0, 1.0, None) == -1          # real without mask
    assert lib.shg_image_grid_u8(p, None, None, p, 3, 4, 4, 1, 1, 0.0, float('nan'), None) == -1


def test_stats_table_validator_raises_before_any_launch():
    good = tstats.build_stats_table([(4096, 5, 0), (8192, 1, 2)])
    assert good.shape == (3, 4) and good.dtype == np.int64 and tuple(good[-1]) == (0, 0, -1, 0)
    tstats.validate_stats_table(good, 3, extents=[(4096, 20), (8192, 4)])
    for rows, slots, what in (([(4096, 0, 0)], 3, 'elements'), ([(4098, 5, 0)], 3, 'misaligned'), ([(4096, 5, 3)], 3, 'slot 3 of 3'),
                              ([(4096, 5, -1)], 3, 'slot -1'), ([(0, 5, 0)], 3, 'misaligned')):
        with pytest.raises(ShgError, match=what):
            tstats.validate_stats_table(tstats.build_stats_table(rows), slots)
    with pytest.raises(ShgError, match='leaves its tensor'):
        tstats.validate_stats_table(good, 3, extents=[(4096, 16), (8192, 4)])
    with pytest.raises(ShgError, match='int64'):
        tstats.validate_stats_table(good.astype(np.int32), 3)
    with pytest.raises(ShgError, match='sentinel'):
        tstats.validate_stats_table(good[:-1], 3)
    c = tstats.Collector('cpu', accumulate_fn=y.accumulate_fn)
    with pytest.raises(ShgError, match='float32'):
        c.report('a', torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ShgError, match='empty'):
        c.report('a', torch.zeros(0))
    with pytest.raises(ShgError, match='contiguous'):
        c.report('a', torch.zeros(4, 4).t())
    with pytest.raises(ShgError, match='no CPU path'):
        tstats.Collector('cpu').report('a', torch.zeros(3))
    assert c.launches == 0


def test_collector_arithmetic_from_hand_made_rows():
    c = tstats.Collector('cpu', slots=8, accumulate_fn=y.accumulate_fn)
    c.report_many({'a': torch.tensor([1.0, 2.0, 3.0, float('nan')]), 'b': torch.tensor([5.0, 5.0])})
    c.report('a', torch.tensor([6.0, float('inf')]))
    c.report0('n', 2.0)
    c.report0('n', 4.0)
    c._slot('empty')
    assert c.launches == 2 and c.names == {'a': 0, 'b': 1, 'n': 2, 'empty': 3}
    c.update()
    assert float(c.acc.abs().sum()) == 0.0                                  # reset
    d = c.as_dict()
    assert d['a']['num'] == 4 and d['a']['mean'] == 3.0 and d['a']['nonfinite'] == 2
    assert abs(d['a']['std'] - math.sqrt((1 + 4 + 9 + 36) / 4 - 9)) < 1e-15
    assert d['b'] == {'num': 2, 'mean': 5.0, 'std': 0.0}                    # 25 - 25, clamped at 0 whatever the rounding
    assert d['n'] == {'num': 2, 'mean': 3.0, 'std': 1.0}
    assert d['empty']['num'] == 0 and math.isnan(d['empty']['mean']) and math.isnan(d['empty']['std']) and 'nonfinite' not in d['b']
    # std clamped: a hand-made row whose sumsq / count - mean^2 is negative (as round-off makes it for a constant tensor)
    c._totals[1] = (3.0, 0.3, 0.0299999, 0.0)
    assert 0.0299999 / 3 - 0.1 * 0.1 < 0 and c.as_dict()['b']['std'] == 0.0
    c.update()                                                              # nothing reported since: every slot empty again
    assert all(v['num'] == 0 for v in c.as_dict().values())
    small = tstats.Collector('cpu', slots=1, accumulate_fn=y.accumulate_fn)
    small.report0('x', 1)
    with pytest.raises(ShgError, match='more than 1 names'):
        small.report0('y', 1)


def test_collector_update_is_one_collective_and_sums_the_ranks():
    script = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd, train_stats_f64 as y
from shgan_amd import training_stats as tstats
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
calls = []
orig = dist.all_reduce
def counted(t, *a, **k):
    calls.append(tuple(t.shape)); return orig(t, *a, **k)
dist.all_reduce = counted
with torch.no_grad():
    c = tstats.Collector("cpu", slots=4, accumulate_fn=y.accumulate_fn)
    c.report_many({"a": torch.full([3 + r], float(r + 1)), "b": torch.tensor([float("nan")] * (r + 1))})
    c.update()
d = c.as_dict()
assert calls == [(4, 4)] and c.collectives == 1, calls
assert d["a"] == {"num": 7, "mean": 11.0 / 7, "std": (19.0 / 7 - (11.0 / 7) ** 2) ** 0.5}, d
assert d["b"]["num"] == 0 and d["b"]["nonfinite"] == 3, d
dist.destroy_process_group()
print("rank", r, "ok")
'''
    port = str(37500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, '-c', script], env=dict(os.environ, RANK=str(rank), SHG_ROOT=ROOT, SHG_PORT=port),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for rank in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for rank, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f'rank {rank} ok' in o, o


# ---- the run: stand-in networks and a stand-in loss that draws from every host generator ----------------------------------------------------
class _Loss:
    """A least-squares 'GAN' whose gradients depend on ``torch.randn`` and ``np.random`` draws and on a running state (``pl_mean``)."""

    def __init__(self, G, D, collector=None):
        self.G, self.D, self.collector, self.stats = G, D, collector, {}
        self.pl_mean = torch.zeros([])
        self.augment_pipe = ada.AugmentPipe(xflip=1)

    def state_dict(self):
        return {'pl_mean': self.pl_mean.clone()}

    def load_state_dict(self, sd):
        self.pl_mean.copy_(sd['pl_mean'])

    def accumulate_gradients(self, phase, real_img, real_c, gen_z, gen_c, sync, gain):
        noise = torch.randn(gen_z.shape) * float(np.random.uniform(0.5, 1.5))
        with torch.enable_grad():
            fake = self.G(gen_z + 0.1 * noise)
            if phase.startswith('G'):
                out = self.D(fake)
                loss = (out - 1.0 - self.pl_mean).square()
                self.pl_mean.copy_(self.pl_mean.lerp(out.detach().mean(), 0.1))
                self.stats['Loss/G/loss'] = loss.detach()
            else:
                real_logits = self.D(real_img.flatten(1))
                loss = self.D(fake.detach()).square() + (real_logits - 1.0).square()
                self.stats['Loss/signs/real'] = real_logits.detach().sign()
                self.stats['Loss/D/loss'] = loss.detach()
            (loss.mean() * gain).backward()
        if self.collector is not None:
            self.collector.report_many({k: self.stats[k] for k in (('Loss/G/loss',) if phase.startswith('G') else ('Loss/signs/real', 'Loss/D/loss'))})


def _nets(seed):
    torch.manual_seed(seed)
    G = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.Tanh(), torch.nn.Linear(8, 12)).requires_grad_(False)
    D = torch.nn.Sequential(torch.nn.Linear(12, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)).requires_grad_(False)
    return G, D


KW = dict(lr=0.01, betas=(0.0, 0.99), eps=1e-8)
DATA = [torch.randn(4, 3, 2, 2, generator=torch.Generator().manual_seed(50 + i)) for i in range(12)]


def _batches(start):
    return (DATA[i] for i in range(start, len(DATA)))


def _objects(seed=0, collector=None):
    G, D = _nets(seed)
    G_ema = copy.deepcopy(G)
    loss = _Loss(G, D, collector)
    phases = ts.make_phases(G, D, KW, KW, g_reg_interval=2, d_reg_interval=3)
    ctl = ada.AdaController(loss.augment_pipe, ada_target=0.6, ada_interval=2, ada_kimg=0.1)
    return G, D, G_ema, loss, phases, ctl


def _run(objs, total_kimg, log_dir=None, resume=None, collector=None, **mkw):
    G, D, G_ema, loss, phases, ctl = objs
    m = None if log_dir is None else ts.Maintenance(log_dir, print_fn=None, **mkw)
    out = ts.train(G, D, G_ema, loss, _batches, phases, z_dim=6, batch_size=4, batch_gpu=4, total_kimg=total_kimg, kimg_per_tick=0.008,
                   ema_kimg=0.01, ada=ctl, collector=collector, maintenance=m, resume=resume, device='cpu')
    return out, m


def _state(objs):
    G, D, G_ema, loss, phases, ctl = objs
    out = [p.detach().clone() for m in (G, D, G_ema) for p in m.parameters()] + [loss.pl_mean.clone(), loss.augment_pipe.p.clone()]
    for ph in (phases[0], phases[2]):
        for st in ph.opt.state_dict()['state'].values():
            out += [torch.as_tensor(st['step']).clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()]
    return out + [torch.randn(5), torch.from_numpy(np.random.standard_normal(5))]


def _seed():
    torch.manual_seed(7)
    np.random.seed(8)


def test_tick_block_conditions_order_and_the_jsonl_line(tmp_path, monkeypatch):
    order = []
    real_save = ts.save_snapshot
    monkeypatch.setattr(ts, 'save_snapshot', lambda path, *a, **k: (order.append(('snapshot', k['progress']['cur_tick'] - 1)), real_save(path, *a, **k))[1])
    c = tstats.Collector('cpu', accumulate_fn=y.accumulate_fn)
    objs = _objects(collector=c)
    _seed()
    metrics = {'toy': lambda G_ema: (order.append(('metrics', None)), {'toy_full': 1.5})[1]}
    (nimg, idx), m = _run(objs, 0.024, tmp_path, collector=c, snapshot_ticks=2, metric_ticks=3, metrics=metrics)
    # 6 iterations of 4 images, a tick every 8 images after the first iteration: ticks 0..3 at 4, 12, 20, 24 (done) images
    assert (nimg, idx) == (24, 6) and len(m.lines) == 4
    assert order == [('metrics', None), ('snapshot', 0), ('snapshot', 2), ('metrics', None), ('snapshot', 3)]      # tick 0; 2; 3 = done: metrics first
    def strict(token):
        raise AssertionError(f'stats.jsonl holds {token}, which is not JSON')
    lines = [json.loads(s, parse_constant=strict) for s in open(tmp_path / 'stats.jsonl')]
    assert len(lines) == 4 and [ln['Progress/tick']['mean'] for ln in lines] == [0.0, 1.0, 2.0, 3.0]
    assert [ln['Progress/kimg']['mean'] for ln in lines] == [0.004, 0.012, 0.02, 0.024]
    want = {'Progress/tick', 'Progress/kimg', 'Progress/augment', 'Timing/total_sec', 'Timing/sec_per_tick', 'Timing/sec_per_kimg',
            'Timing/maintenance_sec', 'Loss/G/loss', 'Loss/signs/real', 'Loss/D/loss', 'Metrics/toy_full', 'timestamp'}
    assert set(lines[0]) == want == set(lines[3])
    # a name that received nothing in a tick is left out of its line (metrics run at ticks 0 and 3 only)
    assert 'Metrics/toy_full' not in lines[1] and 'Metrics/toy_full' not in lines[2] and set(lines[1]) == want - {'Metrics/toy_full'}
    assert lines[3]['Metrics/toy_full'] == {'num': 1, 'mean': 1.5, 'std': 0.0}
    # tick 1 covers iterations 1 and 2: Gmain twice + Greg once (index 2), 4 samples each; Dmain twice
    assert lines[1]['Loss/G/loss']['num'] == 12 and lines[1]['Loss/signs/real']['num'] == 8
    assert set(lines[0]['Loss/D/loss']) == {'num', 'mean', 'std'} and isinstance(lines[0]['timestamp'], float)
    assert sorted(os.listdir(tmp_path / 'weight')) == ['G_ema-000000.pth', 'network-snapshot-000000.pt']
    assert c.launches == sum(len(r) for r in ([1, 1, 1, 1], [1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1]))     # one per loss call


def test_jsonl_fields_are_strict_json_and_health_prefixes_never_collide():
    nan = float('nan')
    stats = {'a': {'num': 2, 'mean': 1.0, 'std': 0.0}, 'empty': {'num': 0, 'mean': nan, 'std': nan},
             'bad': {'num': 0, 'mean': nan, 'std': nan, 'nonfinite': 3}, 'inf': {'num': 1, 'mean': float('inf'), 'std': nan}}
    got = ts.jsonl_fields(stats)
    assert got == {'a': stats['a'], 'bad': {'num': 0, 'mean': None, 'std': None, 'nonfinite': 3}, 'inf': {'num': 1, 'mean': None, 'std': None}}
    json.dumps(got, allow_nan=False)

    class _Opt:
        health = True
    g, greg, d, plain = _Opt(), _Opt(), _Opt(), _Opt()
    plain.health = False
    P = lambda name, opt: ts.Phase(name, None, opt, 1)
    assert ts.health_prefixes([P('Gmain', g), P('Greg', g), P('Dmain', d), P('Dreg', d)]) == [('G', g), ('D', d)]
    assert ts.health_prefixes([P('Gboth', g), P('Dboth', plain)]) == [('G', g)]
    # two optimisers with one stem, and phases without a common stem, keep their whole keys: nothing folds into one slot
    assert ts.health_prefixes([P('Gmain', g), P('Greg', greg), P('Dmain', d)]) == [('Gmain', g), ('Greg', greg), ('D', d)]
    assert ts.health_prefixes([P('Gmain', g), P('critic', g), P('Dmain', d)]) == [('Gmain+critic', g), ('D', d)]


def test_snapshot_round_trip_atomic_write_and_mismatches(tmp_path):
    objs = _objects()
    _seed()
    _run(objs, 0.012)
    G, D, G_ema, loss, phases, ctl = objs
    path = tmp_path / 'weight' / 'snap.pt'
    prog = dict(cur_nimg=12, batch_idx=3, cur_tick=2, tick_start_nimg=12)
    snap = ts.save_snapshot(path, G, D, G_ema, phases=phases, loss=loss, ada=ctl, progress=prog, device='cpu')
    assert sorted(snap) == ['D', 'G', 'G_ema', 'ada', 'augment_pipe', 'loss', 'opt', 'progress', 'rng', 'version', 'world']
    assert sorted(snap['opt']) == ['Dmain+Dreg', 'Gmain+Greg'] and snap['world'] == 1 and len(snap['rng']) == 1
    assert sorted(os.listdir(tmp_path / 'weight')) == ['G_ema-000000.pth', 'snap.pt']
    want = _state(objs)                                                     # (draws from both host generators: after the snapshot)
    fresh = _objects(seed=3)
    assert ts.load_snapshot(path, *fresh[:3], phases=fresh[4], loss=fresh[3], ada=fresh[5], device='cpu') == prog
    got = _state(fresh)
    assert len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(want, got))
    assert fresh[5].iters == ctl.iters == 3 and fresh[5].last_mean == ctl.last_mean and torch.equal(fresh[5].acc, ctl.acc)
    # the bare G_ema file loads as it is
    G2 = _nets(9)[0]
    G2.load_state_dict(torch.load(tmp_path / 'weight' / 'G_ema-000000.pth', weights_only=True), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(G2.parameters(), G_ema.parameters()))
    # a writer that raises midway leaves the previous file intact and no temporary file behind
    before = open(path, 'rb').read()

    def broken(obj, tmp):
        with open(tmp, 'wb') as fh:
            fh.write(b'half a file')
        raise OSError('disk full')
    with pytest.raises(OSError, match='disk full'):
        ts.save_snapshot(path, G, D, G_ema, phases=phases, loss=loss, ada=ctl, progress=prog, device='cpu', save_fn=broken)
    assert open(path, 'rb').read() == before and sorted(os.listdir(tmp_path / 'weight')) == ['G_ema-000000.pth', 'snap.pt']
    # version / world mismatch: both named
    for key, value, what in (('version', 99, 'format version 99, this code reads version 1'), ('world', 4, 'written by 4 ranks, this run has 1')):
        bad = tmp_path / f'bad_{key}.pt'
        torch.save(dict(snap, **{key: value}), bad)
        with pytest.raises(RuntimeError, match=what):
            ts.load_snapshot(bad, *fresh[:3], phases=fresh[4], loss=fresh[3], ada=fresh[5], device='cpu')


def test_g_ema_file_loads_strictly_into_a_fresh_generator(tmp_path):
    from shgan_amd import configs
    cfg = dict(ch_base=512, ch_max=8, w_dim=16, z_dim=16, w0_dim=32)
    G = configs.seeded_init_(configs.build_generator(256, **cfg), seed=5, noise_strength=0.1, bias_std=0.1)
    D = torch.nn.Linear(2, 1)
    ts.save_snapshot(tmp_path / 's.pt', G, D, G, progress=dict(cur_nimg=123456), device='cpu')
    fresh = configs.build_generator(256, **cfg)
    fresh.load_state_dict(torch.load(tmp_path / 'G_ema-000123.pth', weights_only=True), strict=True)
    a, b = G.state_dict(), fresh.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_resumed_run_equals_the_uninterrupted_run_bit_for_bit(tmp_path):
    """6 iterations straight against 3 + snapshot + fresh objects + resume + 3: parameters, Adam state, the loss state, the augment
    probability and the next draws of torch's and numpy's host generators."""
    straight = _objects()
    _seed()
    _run(straight, 0.024)
    want = _state(straight)
    again = _objects()
    _seed()
    _run(again, 0.024)
    assert all(torch.equal(a, b) for a, b in zip(want, _state(again)))      # the precondition: a straight run repeats itself
    first = _objects()
    _seed()
    (nimg, idx), m = _run(first, 0.012, tmp_path, snapshot_ticks=1)
    assert (nimg, idx) == (12, 3) and m.snapshots[-1] == m.snapshot_path(12)
    torch.manual_seed(12345)                                                # everything that is not restored would show
    np.random.seed(54321)
    second = _objects(seed=4)
    (nimg, idx), _ = _run(second, 0.024, resume=m.snapshots[-1])
    assert (nimg, idx) == (24, 6)
    got = _state(second)
    diff = [i for i, (a, b) in enumerate(zip(want, got)) if not torch.equal(a, b)]
    assert len(want) == len(got) and not diff, diff
    # resuming a finished run runs nothing
    done = _objects(seed=4)
    (nimg, idx), m2 = _run(done, 0.012, tmp_path / 'b', snapshot_ticks=1, resume=m.snapshots[-1])
    assert (nimg, idx) == (12, 3) and m2.lines == []
