"""Improved precision and recall (Kynkaanniemi et al. 2019) on the device: the ``pr50k3_full`` metric of the reference's
lib/evaluator/stylegan_metrics/precision_recall.py:19-60 and metric_main.py, on the fp16-MFMA kernels of csrc/pr.hip.

    precision, recall = pr_from_features(real_feats, fake_feats, nhood_size=3)        # [n, 4096] fc2 features of vgg16.Vgg16Features

Semantics (what the tests hold):

1. features are rounded to IEEE fp16 first (lines 42, 46: ``.to(torch.float16)``);
2. ``d(i, j)`` is the Euclidean distance of the fp16 rows: ``sqrt(max(0, |a|^2 + |b|^2 - 2 a.b))`` with the dot product on the fp16 MFMA
   (products of two halves are exact there, sums are fp32), fp32 row norms and one fp32 square root, rounded ONCE to fp16: ``d16``;
3. ``radius_j`` = the ``(nhood_size + 1)``-th smallest ``d16(j, .)`` over the whole manifold, the point itself included (line 53);
4. ``inside_p`` = some ``j`` has ``d16(p, j) <= radius_j``, compared as fp16 values (line 58);
5. the result is ``inside.mean()``; precision: reals are the manifold, fakes the probes; recall: the other way round.

Deliberate departure from the reference: its distances come from ``torch.cdist`` on fp16 operands (line 51), whose own arithmetic in
half precision is far noisier than one fp16 rounding (a CPU ``torch.cdist`` on halves returns a self-distance of 0.55 where the true
value is 0).  That noise is not reproduced: the kernels compute what it approximates, to one rounding.  The reference also materialises
``row_batch x n`` distance matrices, broadcasts them between ranks and runs ``kthvalue`` on the host; here no distance reaches memory
(csrc/pr.hip) and the sweep runs on one device.  There is no CPU path: host tensors raise."""
import torch

from . import _lib, kernels
from ._lib import ShgError, check

MAX_NHOOD = 15


def _half_rows(L, t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ShgError(f'{name} must reside on a HIP (cuda) device: libshgan_hip has no CPU path')
    if t.dtype not in (torch.float32, torch.float16):
        raise ShgError(f'{name} must be float32 or float16 (got {t.dtype})')
    if t.ndim != 2:
        raise ShgError(f'{name} must be [n, D] (got {tuple(t.shape)})')
    return L.req(t.to(torch.float16), name, dtype=torch.float16)          # round to nearest even: step 1


def radii(feats, nhood_size=3):
    """feats [n, D] (float32 or float16, on a HIP device) -> [n] float16: every row's distance to its ``nhood_size``-th nearest
    neighbour in its own set (the ``(nhood_size + 1)``-th smallest of its row of distances, itself included).  Three launches on the
    current stream, no synchronisation."""
    L = kernels._Launch()
    x = _half_rows(L, feats, 'feats')
    n, D = x.shape
    k = int(nhood_size)
    lib = _lib.get_lib()
    nbytes = int(lib.shg_pr_workspace_bytes(n, n, k))
    ws = L.new((max(1, nbytes // 4),), dtype=torch.float32)
    out = L.new((n,), dtype=torch.float16)
    with L:
        check(lib.shg_pr_radii_f16(kernels._ptr(x), n, D, k, kernels._ptr(ws), nbytes, kernels._ptr(out), L.stream()), 'pr_radii')
    return out


def inside(probes, manifold, radii):
    """probes [m, D], manifold [n, D], radii [n] float16 (``radii(manifold, k)``) -> [m] bool: the probe lies in at least one of the
    manifold's balls.  Four launches on the current stream, no synchronisation."""
    L = kernels._Launch()
    p, x = _half_rows(L, probes, 'probes'), _half_rows(L, manifold, 'manifold')
    r = L.req(radii, 'radii', dtype=torch.float16)
    if p.shape[1] != x.shape[1]:
        raise ShgError(f'pr_inside: probes and manifold must share D (got {tuple(p.shape)} and {tuple(x.shape)})')
    if r.ndim != 1 or r.shape[0] != x.shape[0]:
        raise ShgError(f'pr_inside: radii must be [{x.shape[0]}] (got {tuple(r.shape)})')
    m, n, D = p.shape[0], x.shape[0], x.shape[1]
    lib = _lib.get_lib()
    nbytes = int(lib.shg_pr_workspace_bytes(m, n, 0))
    ws = L.new((max(1, nbytes // 4 + 1),), dtype=torch.float32)
    out = L.new((m,), dtype=torch.uint8)
    with L:
        check(lib.shg_pr_inside_f16(kernels._ptr(p), m, kernels._ptr(x), n, D, kernels._ptr(r), kernels._ptr(ws), nbytes, kernels._ptr(out),
                                    L.stream()), 'pr_inside')
    return out.bool()


def pr_from_features(real, fake, nhood_size=3, kernels_fn=None):
    """-> (precision, recall) of two feature sets [n, D] on one HIP device.  ``kernels_fn = (radii_fn, inside_fn)`` with the signatures
    of ``radii`` and ``inside`` replaces the two kernels (CPU tests)."""
    k = int(nhood_size)
    if not 1 <= k <= MAX_NHOOD:
        raise ValueError(f'pr_from_features: nhood_size must be 1..{MAX_NHOOD} (got {nhood_size})')
    if real.ndim != 2 or fake.ndim != 2 or real.shape[1] != fake.shape[1]:
        raise ValueError(f'pr_from_features: features must be [n, D] with one D (got {tuple(real.shape)} and {tuple(fake.shape)})')
    if real.shape[0] < k + 1 or fake.shape[0] < k + 1:
        raise ValueError(f'pr_from_features: each side needs at least nhood_size + 1 = {k + 1} rows')
    if kernels_fn is not None:
        radii_fn, inside_fn = kernels_fn
    else:
        if not (isinstance(real, torch.Tensor) and isinstance(fake, torch.Tensor) and real.is_cuda and fake.is_cuda):
            raise ShgError('pr_from_features: the features must reside on a HIP (cuda) device: libshgan_hip has no CPU path')
        radii_fn, inside_fn = radii, inside
    out = []
    for manifold, probes in ((real, fake), (fake, real)):                    # precision, then recall (lines 44-47)
        flags = inside_fn(probes, manifold, radii_fn(manifold, k))
        flags = torch.as_tensor(flags)
        out.append(int(flags.to(torch.int64).sum()) / flags.numel())         # the count over m, one correctly rounded division
    return tuple(out)
