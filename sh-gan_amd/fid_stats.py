"""FID statistics around the generator (reference lib/evaluator/eva_fid.py:194-277 and the
broadcast-based ``sync`` of lib/evaluator/eva_base.py:96-188).

What the reference does per batch: every rank broadcasts its [B,2048] features (and file names) to every other rank with
3 x world ``dist.broadcast`` calls, rank 0 keeps python lists of float64 arrays and at the end computes
``mu, sigma = mean, x^T x / n - mu mu^T`` in numpy and ``sqrtm`` in scipy.

MI355X-first form:
  * ``FidStats``: float64 second moments of the augmented feature [x, 1] accumulated ON the device by an fp64-MFMA kernel
    (csrc/fid_stats.hip); samples that exist only because ``DistributedSampler(extend=True)`` padded the last round are
    given weight 0 (the reference drops them with ``[0:sample_n]`` after re-interleaving);
  * ONE ``all_reduce`` of the [D+1, D+1] moments (33.6 MB of float64 at D = 2048, RCCL over xGMI) at the end of the
    evaluation replaces all per-batch collectives;
  * ``gather_features``: the reference's own semantics when the features themselves are wanted in dataset order --
    one ``all_gather_into_tensor`` + the zipzap re-interleave instead of 3 x world broadcasts;
  * ``fid_from_stats``: the host tail (``scipy.linalg.sqrtm`` on numpy ``mean_cov``), as eva_fid.py:259-261 -- the default;
  * ``frechet_device`` on ``mean_cov_device``: the same distance without leaving the device.  FID needs only the TRACE of
    sqrt(sigma_f sigma_r); a coupled Newton-Schulz iteration gives it from matrix products alone, on the tiled fp64-MFMA GEMM of
    csrc/gemm_f64.hip (``gemm_f64``), with the traces and the Frobenius norm out of the GEMM's epilogue.
The reference's Inception-v3 feature detector is a TorchScript download (eva_fid.py:30,145-158); the same network runs on
HIP kernels in inception.py, with weights loaded from a torchvision-layout state_dict."""
import math

import numpy as np
import torch

from . import _lib, kernels
from ._lib import check
from .data import zipzap_arrange


class FidStats:
    def __init__(self, dim=2048, device='cuda', accumulate_fn=None):
        self.dim = int(dim)
        self.dp = (self.dim + 1 + 31) // 32 * 32
        self.device = torch.device(device)
        self.S = torch.zeros((self.dp, self.dp), dtype=torch.float64, device=self.device)
        self._accumulate = accumulate_fn            # tests inject a numpy stand-in on CPU; the product path is the HIP kernel

    def add(self, feats, weights=None):
        """feats [B, dim] float32 / float64 on the device; weights [B] float32 (1 = count the sample, 0 = padded duplicate)."""
        if self._accumulate is not None:
            self._accumulate(self.S, feats, weights)
            return
        L = kernels._Launch()
        feats = L.req(feats, 'feats', dtype=feats.dtype if isinstance(feats, torch.Tensor) and feats.dtype == torch.float64 else torch.float32)
        weights = L.req(weights, 'weights')
        L.req(self.S, 'S', dtype=torch.float64)
        if feats.ndim != 2 or feats.shape[1] != self.dim:
            raise _lib.ShgError(f'FidStats.add: features must be [B, {self.dim}]')
        with L:
            check(_lib.get_lib().shg_fid_accumulate_f64(kernels._ptr(feats), int(feats.dtype == torch.float64), kernels._ptr(weights),
                                                        kernels._ptr(self.S), feats.shape[0], self.dim, self.dp, L.stream()), 'fid_accumulate')

    def add_shard(self, feats, k0, rank, world, sample_n):
        """Features of this rank's items k0 .. k0+B-1 (positions in its ``DistributedSampler(extend=True)`` list): item k of
        rank r sits at position k*world + r of the re-interleaved list, which the reference truncates to ``sample_n``."""
        b = feats.shape[0]
        pos = (torch.arange(k0, k0 + b, device=feats.device) * world + rank)
        self.add(feats, (pos < sample_n).to(torch.float32))

    def add_images(self, detector, images, k0=None, rank=0, world=1, sample_n=None):
        """The detector hand-off of ``fid_evaluator.add_batch`` (eva_fid.py:194-206): ``images`` [B,3,H,W] in 0..255 (the uint8
        composite of ``run_generator`` or ``real*127.5+127.5``, shgan_default.py:281-288) -> ``detector(images.float(),
        return_features=True)`` -> moments.  ``detector`` is the caller's Inception-v3 TorchScript module (a download,
        eva_fid.py:20,145-158: not shipped and not reproduced); any callable with that signature works.  With ``k0`` the batch
        is this rank's items k0.. of its sampler list and padded duplicates beyond ``sample_n`` get weight 0 (``add_shard``)."""
        with torch.no_grad():
            feats = detector(images.to(self.device).float(), return_features=True)
        if feats.ndim != 2 or feats.shape[1] != self.dim:
            raise _lib.ShgError(f'FidStats.add_images: the detector returned {tuple(feats.shape)}, expected [B, {self.dim}]')
        if k0 is None:
            self.add(feats)
        else:
            self.add_shard(feats, k0, rank, world, sample_n)
        return feats

    def all_reduce(self):
        """Sum the moments over all ranks (one collective per evaluation)."""
        from .evaluators import Collective
        Collective(self.device, 0, 1).sum_(self.S)           # (a 1-rank group goes through the collective too: same path as N ranks)
        return self

    def mean_cov(self, sample_n=None):
        """-> (n, mu [dim], sigma [dim, dim]) numpy float64; ``mu = mean``, ``sigma = x^T x / sample_n - mu mu^T`` as
        eva_fid.py:252-255 (the reference divides the second moment by ``sample_n``, not by the row count; they differ only
        when fewer than ``sample_n`` features exist -- default: the accumulated count)."""
        S = self.S.cpu().numpy()
        S = np.triu(S) + np.triu(S, 1).T                     # the kernel keeps tiles on / above the diagonal
        d = self.dim
        n = float(S[d, d])
        if not n > 0:
            raise ValueError('FidStats.mean_cov: no samples accumulated (empty accumulator, or every sample had weight 0)')
        mu = S[:d, d] / n
        sigma = S[:d, :d] / (n if sample_n is None else float(sample_n)) - np.outer(mu, mu)
        return n, mu, sigma

    def mean_cov_device(self, sample_n=None):
        """``mean_cov`` without the copy to the host: -> (n, mu [dim], sigma [dim, dim]), float64 tensors on the accumulator's device,
        the same definitions in the same order (the mirrored upper triangle, ``sigma = x^T x / sample_n - mu mu^T``).  Plain torch
        operators: three passes over the moments, once per evaluation.  The count is the one value read back (an empty accumulator raises)."""
        d = self.dim
        launch = kernels._Launch()
        launch.view(self.S, 'S')
        with torch.no_grad():
            n = float(self.S[d, d])
            if not n > 0:
                raise ValueError('FidStats.mean_cov_device: no samples accumulated (empty accumulator, or every sample had weight 0)')
            block = self.S[:d, :d]
            sigma = launch.new((d, d), torch.float64)
            torch.triu(block, out=sigma)                     # the kernel keeps tiles on / above the diagonal
            sigma += torch.triu(block, 1).t()
            # (divisors as [dim]-shaped device tensors: an elementwise division on every device, never a product with a rounded reciprocal)
            count = self.S[d, d].expand(d)
            mu = self.S[:d, d] / count
            sigma /= (count if sample_n is None else torch.tensor(float(sample_n), dtype=torch.float64, device=self.S.device).expand(d))[:, None]
            sigma -= torch.outer(mu, mu)
        return n, mu, sigma


def gemm_f64_tiles(n):
    """The number of 128 x 128 tiles of an n x n product: the length of a row of ``partials``."""
    return ((int(n) + 127) // 128) ** 2


def _gemm_operand(launch, t, name, n=None):
    """A float64 HIP matrix [n, n] or stack [batch, n, n] with unit column stride and a row pitch >= n -> (tensor, n, batch, ld, stride):
    views are served as they are, never copied (the kernel takes a row pitch and a batch stride)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
        raise _lib.ShgError(f'gemm_f64: {name} must be a float64 tensor on a HIP (cuda) device: libshgan_hip has no CPU path')
    if t.ndim not in (2, 3) or t.shape[-1] != t.shape[-2] or t.shape[-1] < 1 or (n is not None and t.shape[-1] != n) or t.shape[0] < 1:
        raise _lib.ShgError(f'gemm_f64: {name} must be [n, n] or [batch, n, n] with one n >= 1 (got {tuple(t.shape)})')
    n = t.shape[-1]
    if n > 1 and (t.stride(-1) != 1 or t.stride(-2) < n):
        raise _lib.ShgError(f'gemm_f64: {name} must have contiguous rows at a pitch >= n (strides {tuple(t.stride())})')
    launch.view(t, name)
    batch = t.shape[0] if t.ndim == 3 else 1
    return t, n, batch, (max(t.stride(-2), n) if n > 1 else 1), (t.stride(0) if t.ndim == 3 and batch > 1 else 0)


def _spans(t, n, batch, ld, stride):
    base = t.data_ptr()
    return [(base + 8 * k * stride, base + 8 * (k * stride + (n - 1) * ld + n)) for k in range(batch)]


def gemm_f64(a, b, alpha=1.0, beta_diag=0.0, out=None, partials=None):
    """``out = alpha * a @ b + beta_diag * I`` on the fp64 MFMA (csrc/gemm_f64.hip): float64 HIP tensors [n, n] or [batch, n, n], any n >= 1,
    contiguous rows at any pitch >= n (views are not copied; a 2-D operand beside a stacked one is shared by the batch).  ``out`` (made
    when None) must not overlap ``a`` or ``b``; nothing beside ``out[..., :n, :n]`` is written.  ``partials``: a contiguous float64
    [2, tiles] ([batch, 2, tiles] for a stack), tiles = ``gemm_f64_tiles(n)``, receives per tile the sum of the diagonal entries (row 0)
    and of the squared entries (row 1) of ``out``; ``partials.sum(-1)`` is (tr out, |out|_F^2).  One launch on the current stream, no
    synchronisation, no atomics: the same bits on every run.  -> out"""
    launch = kernels._Launch()               # (``launch``, not ``L``: the allocation tests cover this function from tests/test_gpu_fid_tail.py)
    a, n, ba, lda, sa = _gemm_operand(launch, a, 'a')
    b, _, bb, ldb, sb = _gemm_operand(launch, b, 'b', n)
    batch = max(ba, bb)
    if (ba != batch and ba != 1) or (bb != batch and bb != 1):
        raise _lib.ShgError(f'gemm_f64: a and b must hold one batch size, or one of them a single matrix (got {ba} and {bb})')
    stacked = a.ndim == 3 or b.ndim == 3
    if out is None:
        out = launch.new((batch, n, n) if stacked else (n, n), torch.float64)
    out, _, bc, ldc, sc = _gemm_operand(launch, out, 'out', n)
    if bc != batch or (out.ndim == 3) != stacked:
        raise _lib.ShgError(f'gemm_f64: out must be {"[%d, n, n]" % batch if stacked else "[n, n]"} (got {tuple(out.shape)})')
    for other, spans in (('a', _spans(a, n, ba, lda, sa)), ('b', _spans(b, n, bb, ldb, sb))):
        if any(lo < hi2 and lo2 < hi for lo, hi in _spans(out, n, bc, ldc, sc) for lo2, hi2 in spans):
            raise _lib.ShgError(f'gemm_f64: out overlaps {other} (the product is not computed in place)')
    lib = _lib.get_lib()
    if partials is not None:
        tiles = int(lib.shg_gemm_f64_tiles(n))
        want = (batch, 2, tiles) if stacked else (2, tiles)
        if not isinstance(partials, torch.Tensor) or tuple(partials.shape) != want or not partials.is_contiguous():        # (written: never a copy)
            raise _lib.ShgError(f'gemm_f64: partials must be a contiguous float64 {list(want)}')
        partials = launch.req(partials, 'partials', dtype=torch.float64)
    with launch:
        check(lib.shg_gemm_f64(kernels._ptr(a), kernels._ptr(b), kernels._ptr(out), n, lda, ldb, ldc, float(alpha), float(beta_diag), batch,
                               sa, sb, sc, kernels._ptr(partials), launch.stream()), 'gemm_f64')
    return out


def frechet_device(mu_f, sigma_f, mu_r, sigma_r, tol=1e-10, max_iter=100, matmul_fn=None):
    """The Frechet distance of ``fid_from_stats`` from float64 tensors on the device (``FidStats.mean_cov_device``) without a matrix
    square root: ``fid = |mu_f - mu_r|^2 + tr sigma_f + tr sigma_r - 2 tr sqrt(sigma_f sigma_r)``, the trace from the coupled
    Newton-Schulz iteration on the same non-symmetric product the reference hands to ``sqrtm``:

        A = sigma_f sigma_r,  s = |A|_F,  Y_0 = A / s,  Z_0 = I;   T = 1.5 I - 0.5 Z Y,  Y <- Y T,  Z <- T Z;   tr sqrt(A) = sqrt(s) tr Y

    Every step is two launches of ``gemm_f64`` (T; then Y T and T Z as one batch of two), whose epilogue hands back t_k = tr Y_k; only
    traces are ever used.  With d_k = |t_k - t_(k-1)| / |t_k| the iteration
      * stops at the first d_k <= tol and takes t_k                                                       (``stop = 'tol'``),
      * stops and takes t_(k-1) when d_k > d_(k-1) while d_(k-1) < 1e-3, or when d_k is not finite      (``stop = 'turn'``): for a
        singular or nearly singular A (a rank-deficient sigma: fewer rows than features) the iteration converges as far as float64
        allows and then turns round -- a fixed step count would run into the divergence,
      * raises past ``max_iter`` steps.
    The decision is made on the host: one 8-byte read of t_k per step (an end-of-run tail).  Five [n, n] buffers (Y, Z, their successors
    and T) are made once, as one allocation, and swapped; nothing is allocated inside the loop.  ``matmul_fn(a, b, alpha=, beta_diag=, out=,
    partials=)`` replaces ``gemm_f64`` (CPU tests); without it host tensors raise.
    -> dict(fid, trace_sqrt, iterations (steps taken, the discarded one of a 'turn' included), delta (the d of the trace taken), stop)."""
    run = matmul_fn if matmul_fn is not None else gemm_f64
    tol, max_iter = float(tol), int(max_iter)
    if not tol > 0 or max_iter < 1:
        raise _lib.ShgError(f'frechet_device: need tol > 0 and max_iter >= 1 (got {tol}, {max_iter})')
    for t, name in ((mu_f, 'mu_f'), (sigma_f, 'sigma_f'), (mu_r, 'mu_r'), (sigma_r, 'sigma_r')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != sigma_f.device:
            raise _lib.ShgError(f'frechet_device: {name} must be a float64 tensor on the device of sigma_f')
    n = sigma_f.shape[-1]
    if sigma_f.ndim != 2 or n < 1 or tuple(sigma_f.shape) != (n, n) or sigma_r.shape != sigma_f.shape or tuple(mu_f.shape) != (n,) or mu_r.shape != mu_f.shape:
        raise _lib.ShgError(f'frechet_device: need mu [n] and sigma [n, n] with one n on both sides (got {tuple(mu_f.shape)}, {tuple(sigma_f.shape)}, '
                            f'{tuple(mu_r.shape)}, {tuple(sigma_r.shape)})')
    if matmul_fn is None and not sigma_f.is_cuda:
        raise _lib.ShgError('frechet_device: the statistics must reside on a HIP (cuda) device: libshgan_hip has no CPU path')
    launch = kernels._Launch()
    launch.view(sigma_f, 'sigma_f')
    with torch.no_grad():
        base = float(torch.square(mu_f - mu_r).sum() + sigma_f.diagonal().sum() + sigma_r.diagonal().sum())
        # slots: Y_even, Y_odd, T, Z_even, Z_odd -- in this order every pair a batched launch needs has a positive stride
        W = launch.new((5, n, n), torch.float64)
        P = launch.new((2, 2, gemm_f64_tiles(n)), torch.float64)
        pair = lambda i, j: W.as_strided((2, n, n), ((j - i) * n * n, n, 1), W.storage_offset() + i * n * n)       # noqa: E731
        run(sigma_f, sigma_r, out=W[0], partials=P[0])
        s = P[0, 1].sum().sqrt()
        scale = float(s)
        if not math.isfinite(scale):
            raise _lib.ShgError(f'frechet_device: |sigma_f sigma_r|_F is {scale} (non-finite statistics?)')
        if scale == 0.0:                         # a zero product has a zero square root
            return dict(fid=base, trace_sqrt=0.0, iterations=0, delta=0.0, stop='tol')
        W[0] /= s.expand(n, n)
        W[3].zero_()
        W[3].diagonal().fill_(1.0)
        t_prev, d_prev, cur = float(W[0].diagonal().sum()), None, 0
        for k in range(1, max_iter + 1):
            run(W[3 + cur], W[cur], alpha=-0.5, beta_diag=1.5, out=W[2])
            run(pair(cur, 2), pair(2, 3 + cur), out=pair(1 - cur, 4 - cur), partials=P)
            t = float(P[0, 0].sum())
            d = abs(t - t_prev) / abs(t) if math.isfinite(t) and t != 0.0 else float('nan')
            if not math.isfinite(d):
                taken, d_taken, stop = t_prev, d_prev, 'turn'
                break
            if d <= tol:
                taken, d_taken, stop = t, d, 'tol'
                break
            if d_prev is not None and d > d_prev and d_prev < 1e-3:
                taken, d_taken, stop = t_prev, d_prev, 'turn'
                break
            t_prev, d_prev, cur = t, d, 1 - cur
        else:
            raise _lib.ShgError(f'frechet_device: no stop within {max_iter} Newton-Schulz steps (last tr Y = {t!r}, delta = {d!r})')
    trace_sqrt = math.sqrt(scale) * taken
    return dict(fid=base - 2.0 * trace_sqrt, trace_sqrt=trace_sqrt, iterations=k, delta=d_taken, stop=stop)


def fid_from_stats(mu_fake, sigma_fake, mu_real, sigma_real):
    """eva_fid.py:258-261."""
    import scipy.linalg
    m = np.square(mu_fake - mu_real).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_fake, sigma_real), disp=False)
    return float(np.real(m + np.trace(sigma_fake + sigma_real - s * 2)))


def gather_features(local_feats, n_items, rank, world):
    """All ranks' [B_r, D] features -> numpy [n_items, D] in dataset order: ``all_gather_into_tensor`` + zipzap
    (replaces ``base_evaluator.sync`` + ``zipzap_arrange``, eva_fid.py:217-229).  Every rank must hold the same count
    (DistributedSampler(extend=True) guarantees it)."""
    import torch.distributed as dist
    if world == 1:
        return local_feats.detach().cpu().numpy()[:n_items]
    full = torch.empty((world * local_feats.shape[0],) + tuple(local_feats.shape[1:]), dtype=local_feats.dtype, device=local_feats.device)
    dist.all_gather_into_tensor(full, local_feats.contiguous())
    full = full.view((world,) + tuple(local_feats.shape))
    return zipzap_arrange([full[r].cpu().numpy() for r in range(world)])[:n_items]
