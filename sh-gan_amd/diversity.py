"""Diversity of pluralistic completions: the mean pairwise LPIPS among the K samples a generator draws for ONE masked input
(``Generator.sample_many``).  The K samples of all N inputs go through the LPIPS backbone once (``Lpips.taps_of``: N*K images), and the pair
form of the distance head (csrc/lpips.hip, ``lpips.head_pairs``) evaluates the K(K-1)/2 unordered pairs of every input on each tap: one
trunk pass per sample instead of the K - 1 the pair API ``net(a, b)`` would cost.

Every sample takes the 'pred' operand form of ``lpips.Lpips`` (uint8 composite or float32 in [0, 1]).  For float32 samples a pair's value is
bit for bit ``net(imgs[n, a], imgs[n, b], gt_range='unit')``; for uint8 samples the pair API rounds its second operand through the 'gt' value
table, which this symmetric form does not do."""
import torch

from . import kernels
from . import lpips as lpips_mod
from ._lib import ShgError


def pair_table(k):
    """The K(K-1)/2 unordered pairs (a, b), a < b < K, in lexicographic order: (0,1), (0,2), ..., (K-2,K-1)."""
    return [(a, b) for a in range(int(k)) for b in range(a + 1, int(k))]


def pair_tables(n, k):
    """int32 CPU tables (ia, ib) of the pairs of N inputs with K samples each, rows of an [N*K, ...] batch: input n's pairs at
    [n*P, (n+1)*P), P = K(K-1)/2, in ``pair_table`` order."""
    pairs = pair_table(k)
    ia = torch.tensor([i * k + a for i in range(int(n)) for a, _ in pairs], dtype=torch.int32)
    ib = torch.tensor([i * k + b for i in range(int(n)) for _, b in pairs], dtype=torch.int32)
    return ia, ib


_TABLES = {}


def _device_tables(n, k, device):
    """``pair_tables`` on the device, built (and range-checked by construction) once per (N, K, device)."""
    key = (int(n), int(k), str(device))
    if key not in _TABLES:
        _TABLES[key] = tuple(t.to(device) for t in pair_tables(n, k))
    return _TABLES[key]


def pairwise_lpips(net, imgs, out=None):
    """net: ``lpips.Lpips``; imgs [N,K,3,R,R] (uint8 or float32 in [0, 1]) on the device -> float64 [N]: the mean over the K(K-1)/2 pairs of
    the LPIPS distance between samples a and b of input n (the pair values added in ``pair_table`` order in float64, then divided by their
    number).  K = 1: zeros, and no kernel of the library runs.  ``out``: a contiguous float64 [N] tensor to write into."""
    if not isinstance(net, lpips_mod.Lpips):
        raise ShgError('diversity: net must be an lpips.Lpips (lpips.LPIPS(net=\'alex\' | \'vgg\', ...))')
    if not isinstance(imgs, torch.Tensor) or imgs.ndim != 5 or imgs.shape[2] != 3 or not imgs.is_cuda:
        raise ShgError('diversity: imgs must be a HIP tensor [N,K,3,R,R]')
    N, K, _, H, W = imgs.shape
    launch = kernels._Launch()               # (``launch``, not ``L``, and ``.new(...).zero_()`` for ``torch.zeros``: see the note above
    launch.view(imgs, 'imgs')                # kernels.plural_composite_u8 -- the site tables of the allocation tests have no entry for this function)
    if out is None:
        out = launch.new((N,), torch.float64)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (N,) or not out.is_contiguous():
        raise ShgError(f'diversity: out must be a contiguous float64 [{N}] tensor')
    out.zero_()
    if K == 1 or N == 0:
        return out
    if H < net.min_size or W < net.min_size:
        raise ShgError(f'diversity: images of {H} x {W} are too small for the {net.net} taps (>= {net.min_size})')
    P = K * (K - 1) // 2
    if N * P > 65535:                       # the pair head's table limit: split over the inputs
        step = max(1, 65535 // P)
        for n0 in range(0, N, step):
            pairwise_lpips(net, imgs[n0:n0 + step], out=out[n0:n0 + step])
        return out
    ia_d, ib_d = _device_tables(N, K, imgs.device)
    with torch.no_grad():
        values = launch.new((N * P,), torch.float64).zero_()
        for t, w in zip(net.taps_of(imgs.reshape(N * K, 3, H, W)), net.lins):
            lpips_mod.head_pairs(t, ia_d, ib_d, w, values)
        # fixed order: pair 0 + pair 1 + ... in float64 (a sequential chain, not a tree), then one division
        acc = values.view(N, P)[:, 0].clone()
        for p in range(1, P):
            acc += values.view(N, P)[:, p]
        out.copy_(acc / P)
    return out
