"""Inception Score without storing probabilities (reference lib/evaluator/stylegan_metrics/inception_score.py:30-36; the ``is50k``
metric of metric_main.py).

The reference keeps every image's [C] softmax row on the host and, per split, evaluates exp(mean_i sum_c p_ic (log p_ic - log pbar_c)).
That equals exp(A / n - sum_c pbar_c log pbar_c) with A = sum_i sum_c p_ic log p_ic, P_c = sum_i p_ic and pbar = P / n, so a split needs
only n, A and P[C]: a float64 ``[num_splits, C + 2]`` accumulator (columns 0..C-1 = P, column C = A, column C + 1 = n) that the kernel of
csrc/kid.hip updates in place per batch, like the FID moments.

Deviation from the reference: a probability of exactly 0 contributes 0 to A (the limit of p log p); the reference's numpy evaluates
0 * log 0 = NaN there and the whole score becomes NaN."""
import numpy as np
import torch

from . import _lib, kernels
from ._lib import check


def split_of(dataset_id, n_items, num_splits):
    """The split an image belongs to: line 32 slices ``probs[i * N // S : (i + 1) * N // S]``; -1 for an id outside [0, N)."""
    dataset_id, n_items, num_splits = int(dataset_id), int(n_items), int(num_splits)
    if not 0 <= dataset_id < n_items:
        return -1
    i = dataset_id * num_splits // n_items                        # within one of the true split: the bounds are floors
    while i + 1 < num_splits and dataset_id >= (i + 1) * n_items // num_splits:
        i += 1
    while i > 0 and dataset_id < i * n_items // num_splits:
        i -= 1
    return i


def new_accumulator(num_splits, num_classes, device):
    return torch.zeros((int(num_splits), int(num_classes) + 2), dtype=torch.float64, device=device)


def is_accumulate(acc, probs, splits):
    """acc [num_splits, C + 2] float64 += probs [B, C] float32 with ``splits`` [B] int32 (negative = skip: a padded duplicate); one
    launch on the current stream, fixed order over the batch, no atomics."""
    L = kernels._Launch()
    probs = L.req(probs, 'probs')
    splits = L.req(splits, 'splits', dtype=torch.int32)
    L.req(acc, 'acc', dtype=torch.float64)
    if not acc.is_contiguous():
        raise _lib.ShgError('is_accumulate: the accumulator must be contiguous (it is updated in place)')
    if probs.ndim != 2 or acc.ndim != 2 or acc.shape[1] != probs.shape[1] + 2 or splits.shape != (probs.shape[0],):
        raise _lib.ShgError(f'is_accumulate: probs [B, C], splits [B], acc [S, C + 2] (got {tuple(probs.shape)}, {tuple(splits.shape)}, '
                            f'{tuple(acc.shape)})')
    with L:
        check(_lib.get_lib().shg_is_accumulate_f64(kernels._ptr(probs), kernels._ptr(splits), kernels._ptr(acc), probs.shape[0], probs.shape[1],
                                                   acc.shape[0], L.stream()), 'is_accumulate')
    return acc


def is_from_accumulator(acc):
    """[num_splits, C + 2] -> (mean, std) of the per-split scores, on the host in float64 (``np.std``: population form, line 36).  A split
    without images gives NaN, as the reference's mean over an empty slice does."""
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = a.astype(np.float64)
    C = a.shape[1] - 2
    scores = []
    for row in a:
        n = row[C + 1]
        if not n > 0:
            scores.append(float('nan'))
            continue
        pbar = row[:C] / n
        nz = pbar > 0
        scores.append(np.exp(row[C] / n - np.sum(pbar[nz] * np.log(pbar[nz]))))
    return float(np.mean(scores)), float(np.std(scores))
