"""RCCL with N > 1 ranks -- two ranks, one per GPU, wherever ``torch.cuda.device_count() >= 2``.  RCCL refuses two ranks on one device
("Duplicate GPU detected"), so a one-GPU machine runs the same entry points in a one-rank RCCL group: the nccl process group, its barriers,
all-reduces and all-gathers execute there too, and the multi-rank logic is covered on one device over gloo (tests/test_gpu_bench_ranks.py)
and on the CPU (world 2).  Two entry points: ``bench.py --gpus N`` (its own launcher, one rank per GPU, backend nccl; one rank: joined as a
torch.distributed.run rank) and ``eval_harness.sharded_eval(gather=True)`` + ``grad_sync.BucketedAllReduce`` in an N-rank nccl group
(batch sharding of config 4 and the gradient all-reduce of config 5)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
WORLD = min(2, torch.cuda.device_count())       # ranks of the RCCL group: one per device, at most two


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return str(port)


def test_bench_two_ranks_over_rccl():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    if WORLD == 1:                                # one device: bench.py joins a one-rank RCCL group as a torch.distributed.run rank
        env.update(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port())
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(WORLD), '--steps', '3', '--warmup', '1', '--no-cpu-baseline',
                        '--no-second-config', '--full', '--all-blocks', '--train-steps', '1'], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    line = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == WORLD and line['config']['collective_backend'] == 'nccl' and line['config']['ranks_all_reduced'] == WORLD
    assert not line['config']['ranks_share_devices'] and line['config']['global_batch'] == 16 * WORLD
    assert line['train_step']['grad_all_reduce'] == ('nccl' if WORLD > 1 else None) and line['train_step']['losses_finite']


def test_sharded_eval_and_gradient_buckets_two_ranks_over_rccl():
    script = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"])
import shgan_amd
from shgan_amd import configs, eval_harness as hz
from shgan_amd.grad_sync import BucketedAllReduce
r = int(os.environ["RANK"])
torch.cuda.set_device(r)
dev = torch.device("cuda", r)
world = int(os.environ["WORLD"])
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=r, world_size=world, device_id=dev)
kw = dict(ch_base=2048, ch_max=32, w_dim=64, z_dim=48, w0_dim=96)
G = configs.seeded_init_(configs.build_generator(256, **kw), seed=5).eval().requires_grad_(False).to(dev)
with torch.no_grad():
    order, merged = hz.sharded_eval(G, n_items=7, batch_size=2, resolution=256, seed=3, device=dev, rank=r, world=world, gather=True, z_dim=48)
    ids, alone = hz.sharded_eval(G, n_items=7, batch_size=2, resolution=256, seed=3, device=dev, rank=0, world=1, gather=False, z_dim=48)
assert order == list(range(7)) and np.array_equal(merged, alone.cpu().numpy())      # sharded over the GPUs == one GPU, in dataset order
w = torch.nn.Parameter(torch.zeros(5000, device=dev))
sync = BucketedAllReduce([w], bucket_bytes=8192, always_reduce=True)         # (one rank: the all-reduce still runs in the RCCL group)
sync.zero_grad()
(w.sum() * (1.0 if r == 0 else 10.0)).backward()
sync.arm()
(w.sum() * (2.0 if r == 0 else 20.0)).backward()
sync.finish()
assert torch.allclose(w.grad, torch.full_like(w, 16.5 if world == 2 else 3.0))      # mean over the ranks of 3 (rank 0) and 30 (rank 1)
dist.destroy_process_group()
print("rank", r, "ok")
'''
    port = str(36500 + os.getpid() % 2000)
    procs = []
    for rank in range(WORLD):
        env = dict(os.environ, RANK=str(rank), WORLD=str(WORLD), SHG_ROOT=ROOT, SHG_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for rank, p in enumerate(procs):
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0 and f'rank {rank} ok'.encode() in out, out.decode()[-3000:]
