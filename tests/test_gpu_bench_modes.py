"""``bench.py`` without and with ``--full`` on one device, at 256^2 batch 4: a plain run prints the headline and nothing it had to run extra
work for; ``--full`` adds the one-batch-alone latency, the instrumented per-kernel pass, the evaluation-loop block and the CPU baseline, and
leaves the headline loop's output as the plain run computes it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

COMMON = ['--gpus', '1', '--steps', '2', '--warmup', '1', '--resolution', '256', '--batch', '4', '--noise-mode', 'const']
FULL_ONLY = ('roofline', 'hbm', 'shu', 'eval_loop', 'second_config', 'fp16_blocks_eval', 'train_step', 'cpu_baseline')


def _bench(extra, out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + COMMON + ['--dump-outputs', str(out_dir)] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')][-1])


def test_bench_plain_and_full(tmp_path):
    plain = _bench([], tmp_path / 'plain')
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in plain, key
    assert plain['value'] > 0 and plain['ms_per_step'] > 0 and plain['full'] is False
    assert not set(FULL_ONLY) & set(plain), sorted(set(FULL_ONLY) & set(plain))
    assert plain['pipeline']['ms_per_step_single_stream'] is None

    full = _bench(['--full', '--profile-steps', '1', '--cpu-images', '1', '--cpu-forwards', '1'], tmp_path / 'full')
    assert full['full'] is True and set(FULL_ONLY) <= set(full)
    assert full['pipeline']['ms_per_step_single_stream'] > 0
    assert full['roofline']['classes'] and full['hbm']['classes']
    assert full['eval_loop']['result_ok'] and full['eval_loop']['n_gpus'] == 1
    assert full['second_config'] is None and full['train_step'] is None          # 512^2 at the default batch only
    assert full['cpu_baseline']['value'] > 0

    # the headline loop computes the same composite either way (one batch, same seeds; only uint8 truncation flips may differ)
    a, b = np.load(tmp_path / 'plain' / 'composite.npy'), np.load(tmp_path / 'full' / 'composite.npy')
    assert a.shape == b.shape == (4, 3, 256, 256)
    d = np.abs(a - b)
    assert float(d.max()) <= 1 and float((d > 0).mean()) < 1e-3
