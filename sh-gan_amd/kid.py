"""Kernel Inception Distance on the device (reference lib/evaluator/stylegan_metrics/kernel_inception_distance.py:34-44; the
``kid50k_full`` metric of metric_main.py).

The reference draws ``num_subsets`` random subsets of ``m`` rows of each side's [n, 2048] features on the host, forms three m x m
polynomial-kernel matrices per subset in numpy float32 and sums them.  Here the index tables are drawn on the host in the reference's
order (``kid_subsets``) and ONE call of the fp64-MFMA kernel of csrc/kid.hip returns the three sums of every subset: rows are gathered
through the tables while the operands are staged and the cube and the sums happen on the accumulator registers, so neither a gathered
subset nor a kernel matrix exists in memory.  The few remaining operations on [S, 3] numbers run on the host in float64.

Deviation from the reference: the subsets come from ``numpy.random.RandomState(seed)`` instead of numpy's global generator (the
reference never seeds it), so that a value can be reproduced.  There is no CPU path: host tensors raise."""
import numpy as np
import torch

from . import _lib, kernels
from ._lib import check


def kid_subsets(n_fake, n_real, num_subsets=100, max_subset_size=1000, seed=0):
    """-> (idx_f [S, m] int32, idx_r [S, m] int32, m): m = min(n_fake, n_real, max_subset_size) (line 35); per subset first the fake
    draw, then the real draw, each ``choice(n, m, replace=False)`` (lines 38-39) of one ``RandomState(seed)``."""
    n_fake, n_real, num_subsets = int(n_fake), int(n_real), int(num_subsets)
    m = min(n_fake, n_real, int(max_subset_size))
    if num_subsets < 1 or m < 1:
        raise ValueError('kid_subsets: need at least one subset and one row per side')
    rs = np.random.RandomState(seed)
    idx_f = np.empty((num_subsets, m), dtype=np.int32)
    idx_r = np.empty((num_subsets, m), dtype=np.int32)
    for s in range(num_subsets):
        idx_f[s] = rs.choice(n_fake, m, replace=False)
        idx_r[s] = rs.choice(n_real, m, replace=False)
    return idx_f, idx_r, m


def kid_sums(fake, real, idx_f, idx_r):
    """fake [n_f, D], real [n_r, D] (float32 or float64, one dtype) and int32 index tables [S, m], all on one HIP device -> [S, 3]
    float64 on it: per subset sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j) with k(u, v) = (u.v / D + 1)^3
    (lines 40-42).  Two launches on the current stream, no synchronisation."""
    L = kernels._Launch()
    dt = fake.dtype if isinstance(fake, torch.Tensor) and fake.dtype == torch.float64 else torch.float32
    fake, real = L.req(fake, 'fake', dtype=dt), L.req(real, 'real', dtype=dt)
    idx_f, idx_r = L.req(idx_f, 'idx_f', dtype=torch.int32), L.req(idx_r, 'idx_r', dtype=torch.int32)
    if fake.ndim != 2 or real.ndim != 2 or fake.shape[1] != real.shape[1]:
        raise _lib.ShgError(f'kid_sums: features must be [n, D] with one D (got {tuple(fake.shape)} and {tuple(real.shape)})')
    if idx_f.ndim != 2 or idx_f.shape != idx_r.shape:
        raise _lib.ShgError(f'kid_sums: the index tables must both be [S, m] (got {tuple(idx_f.shape)} and {tuple(idx_r.shape)})')
    S, m = idx_f.shape
    lib = _lib.get_lib()
    nbytes = int(lib.shg_kid_workspace_bytes(S, m))
    ws = L.new((max(1, nbytes // 8),), dtype=torch.float64)
    out = L.new((S, 3), dtype=torch.float64)
    with L:
        check(lib.shg_kid_sums_f64(kernels._ptr(fake), kernels._ptr(real), int(dt == torch.float64), fake.shape[0], real.shape[0], fake.shape[1],
                                   kernels._ptr(idx_f), kernels._ptr(idx_r), S, m, kernels._ptr(ws), nbytes, kernels._ptr(out), L.stream()), 'kid_sums')
    return out


def kid_from_sums(sums, m):
    """[S, 3] sums -> the KID: t_s = (a_xx + a_yy) / (m - 1) - 2 b / m (line 42), kid = sum_s t_s / S / m (line 43), in float64."""
    sums = np.asarray(sums, dtype=np.float64)
    t = (sums[:, 0] + sums[:, 1]) / (m - 1) - sums[:, 2] * 2 / m
    return float(t.sum() / sums.shape[0] / m)


def kid_from_features(fake, real, num_subsets=100, max_subset_size=1000, seed=0, sums_fn=None):
    """The KID of two feature sets on the device.  ``sums_fn(fake, real, idx_f, idx_r) -> [S, 3]`` replaces the kernel (CPU tests)."""
    idx_f, idx_r, m = kid_subsets(fake.shape[0], real.shape[0], num_subsets, max_subset_size, seed)
    if m < 2:
        raise ValueError('kid_from_features: a subset needs at least 2 rows per side')
    if sums_fn is not None:
        return kid_from_sums(sums_fn(fake, real, idx_f, idx_r), m)
    if not isinstance(fake, torch.Tensor) or not fake.is_cuda:
        raise _lib.ShgError('kid_from_features: the features must reside on a HIP (cuda) device: libshgan_hip has no CPU path')
    sums = kid_sums(fake, real, torch.from_numpy(idx_f).to(fake.device), torch.from_numpy(idx_r).to(fake.device))
    return kid_from_sums(sums.cpu().numpy(), m)
